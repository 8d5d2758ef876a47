"""YIN f0 extraction without a GPU: sanity of the float64 oracle (tests/yin_oracle.py), the conditions on
the test inputs that the GPU tests rest on (decision margins, the cap on skipped frames, voiced and unvoiced
frames in every case), the error of the fp32 FFT route against the oracle, pwg_yin_frames and the argument
checks of the C-ABI, the Python signatures, and the preprocess CLI's file handling with the extractors
replaced by the oracles.

Measured here: no frame of any case is below its margin (smallest margin 3.1e-4 at R, where eps = 2.1e-4;
6.1e-4 at S / S4, where eps = 1.1e-5); the fp32 FFT route decides every frame as the oracle does and its c
is within 1.37e-4 (relative) of the oracle's, which sets R_MAX = 1.4e-4 (tests/yin_helpers.py)."""

import ctypes
import inspect
import os
import wave

import numpy as np
import pytest
import torch
import yaml

import logmel_oracle as mel_orc
import yin_oracle as orc
from yin_helpers import (CASES, GEOMETRIES, P, R_MAX, SHORT, THRESHOLD, TILE, case_signal, compared, eps_of, fft_route,
                         fft_route_errors, oracle, plan_create, signal)
from parallelwavegan_amd import LogMelExtractor, YinF0Extractor, _lib, f0_torchyin, yin_estimate

@pytest.mark.parametrize("fs, p", [(8000, 20), (24000, 100), (16000, 57)])
def test_oracle_pure_tone_returns_its_period(fs, p):
    tau_min, tau_max = orc.lag_bounds(fs, fs / (2 * p + 8), fs / 3.0)
    x = 0.5 * np.sin(2 * np.pi * np.arange(6 * tau_max) / p)
    res = orc.analyse(x, fs, tau_min, tau_max, p)
    assert len(res["k"]) == orc.n_frames(len(x), tau_max, p) > 1
    assert (res["k"] + tau_min + 1 == p).all()
    assert np.array_equal(res["f0"], np.full(len(res["k"]), np.float32(fs) / np.float32(p), np.float32))
    assert np.array_equal(orc.log_f0(res["f0"]), np.log(res["f0"]))


def test_oracle_silence_and_noise_are_unvoiced():
    z = orc.analyse(np.zeros(400), 8000, 0, 32, 16)
    assert (z["c"] == 0).all() and (z["k"] == 0).all() and (z["f0"] == 0).all()  # fb == 0: unvoiced
    n = orc.analyse(0.05 * np.random.RandomState(0).standard_normal(4000), 8000, 0, 32, 16)
    assert (n["k"] == 0).all() and n["c"].min() > THRESHOLD
    assert np.array_equal(orc.log_f0(z["f0"]), z["f0"])  # zeros stay 0 in log mode
    with pytest.raises(ValueError):
        orc.frames(np.zeros(0), 32, 16)


def test_oracle_frames_and_fit():
    x = np.arange(100.0)
    fr = orc.frames(x, 16, 10)
    assert fr.shape == (1 + (100 - 32) // 10, 32) and fr[3, 0] == 30 and fr[-1, -1] == 91
    short = orc.frames(x[:20], 16, 10)
    assert short.shape == (1, 32) and (short[0, :20] == x[:20]).all() and (short[0, 20:] == 0).all()
    assert orc.frames(x[:32], 16, 10).shape == (1, 32)
    assert [orc.n_frames(t, 16, 10) for t in (1, 31, 32, 41, 42, 100)] == [1, 1, 1, 1, 2, 7]
    assert np.array_equal(orc.fit(np.array([1, 2, 3]), 5), [1, 2, 3, 3, 3]) and np.array_equal(orc.fit(np.array([1, 2, 3]), 2), [1, 2])
    # the search's special cases: fb == 0 is unvoiced, a falling tail ends on L - 1
    assert orc.search(np.array([0.05, 0.5, 0.05]), 0.1) == 0
    assert orc.search(np.array([0.5, 0.09, 0.08, 0.07]), 0.1) == 3
    assert orc.search(np.array([0.5, 0.09, 0.08, 0.08, 0.01]), 0.1) == 2  # a zero slope ends the descent
    assert orc.search(np.array([0.5, 0.2]), 0.1) == 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%d" % (c[0], c[1], c[3]))
def test_inputs_are_decided_with_margin(case):
    """The condition the exact comparison of k* rests on, from the oracle alone: at most 2 % of a case's
    frames are below the margin eps = 2 (W + tau_max) 2^-24, and a voiced and an unvoiced frame remain."""
    res, keep = oracle(case), compared(case)
    print(f"{case}: {len(keep)} frames, {int((~keep).sum())} below the margin, smallest margin {res['margin'].min():.2e} "
          f"(eps {eps_of(case[0]):.1e}), voiced {int((res['k'][keep] > 0).sum())}, unvoiced {int((res['k'][keep] == 0).sum())}")
    assert len(keep) == case[1]
    assert (~keep).sum() <= 0.02 * len(keep)
    assert (res["k"][keep] > 0).any() and (res["k"][keep] == 0).any()


def test_short_input_is_one_unvoiced_frame_with_margin():
    g, T, seed = SHORT
    fs, hop, tau_min, tau_max, sweep = GEOMETRIES[g]
    res = orc.analyse(signal(T, fs, sweep, seed), fs, tau_min, tau_max, hop)
    assert T < 2 * tau_max and len(res["k"]) == 1 and res["margin"][0] > eps_of(g)


def test_eps_is_the_derived_bound():
    assert abs(eps_of("R") - 2.1e-4) < 1e-5 and abs(eps_of("S") - 1.1e-5) < 1e-6 and eps_of("S4") == eps_of("S")


def test_fft_route_agrees_with_the_oracle_within_r_max():
    """The package's route (fp32, d through rfft / irfft and cumulative energies) against the oracle: the
    same k* on every frame of every case and c within R_MAX, which the GPU bar max(R_MAX, eps) rests on."""
    errs = fft_route_errors()
    for case, e in errs.items():
        print(f"{case}: fp32 FFT route vs oracle, relative error of c {e:.2e}")
    assert set(errs) == set(CASES)
    assert max(errs.values()) <= R_MAX
    for case in CASES:
        fs, hop, tau_min, tau_max, _ = GEOMETRIES[case[0]]
        _, k, f0 = fft_route(case_signal(case), fs, tau_min, tau_max, hop)
        assert np.array_equal(k, oracle(case)["k"]) and np.array_equal(f0, oracle(case)["f0"])


def test_frame_count(built_lib):
    L = built_lib
    assert [L.pwg_yin_frames(t, 600, 300) for t in (1, 1199, 1200, 1499, 1500, 13200)] == [1, 1, 1, 1, 2, 41]
    assert [L.pwg_yin_frames(t, 16, 10) for t in (1, 31, 32, 41, 42, 100)] == [1, 1, 1, 1, 2, 7]
    assert L.pwg_yin_frames(1 << 40, 1, 1) == (1 << 40) - 1
    assert L.pwg_yin_frames(0, 32, 16) == -1 and L.pwg_yin_frames(100, 0, 16) == -1 and L.pwg_yin_frames(100, 32, 0) == -1
    assert _lib.PWG_YIN_FRAME_TILE == TILE == 8
    src = open(os.path.join(_lib.REPO_DIR, "include", "pwg_yin.h")).read()
    assert "PWG_YIN_FRAME_TILE = 8" in src and "PWG_YIN_MAX_TAU = 1680" in src and _lib.PWG_YIN_MAX_TAU == 1680


def test_plan_argument_checks_come_before_any_device_call(built_lib):
    """Every failing check returns its status without a HIP call (this test runs without a GPU)."""
    L, INV, UNS = built_lib, _lib.PWG_ERR_INVALID, _lib.PWG_ERR_UNSUPPORTED
    assert plan_create(L, plan=None) == INV
    for fs in (0.0, -8000.0, float("nan"), float("inf")):
        assert plan_create(L, fs=fs) == INV, fs
    assert plan_create(L, hop=0) == INV and plan_create(L, hop=-16) == INV and b"hop" in L.pwg_last_error()
    assert plan_create(L, tau_min=-1) == INV and b"tau_min" in L.pwg_last_error()
    for tau_min, tau_max in ((0, 1), (31, 32), (40, 32), (0, 0), (0, -5)):
        assert plan_create(L, tau_min=tau_min, tau_max=tau_max) == INV, (tau_min, tau_max)
    for thr in (0.0, -0.1, float("nan"), float("inf")):
        assert plan_create(L, threshold=thr) == INV, thr
    assert plan_create(L, log_f0=2) == INV
    # the unsupported one, reported only when nothing is invalid
    assert plan_create(L, tau_max=1681) == UNS and b"LDS" in L.pwg_last_error()
    assert plan_create(L, tau_max=1 << 30) == UNS
    assert plan_create(L, tau_max=1681, hop=0) == INV
    with pytest.raises(NotImplementedError, match="PWG_YIN_MAX_TAU"):
        _lib.check(plan_create(L, tau_max=5000))
    with pytest.raises(ValueError, match="threshold"):
        _lib.check(plan_create(L, threshold=0.0))


def test_run_argument_checks_come_before_any_device_call(built_lib):
    """pwg_yin_run's checks of the boundaries and the row counts read nothing of the plan and make no HIP
    call: every failing call below returns before `plan` (a pointer that is never followed) is used."""
    L, INV = built_lib, _lib.PWG_ERR_INVALID
    ll = ctypes.c_longlong

    def run(starts=(0, 100, 250), frames=(3, 4), rows=7, plan=P, wave_=P, f0=P, n=None, no_starts=False):
        st = None if no_starts else (ll * len(starts))(*starts)
        fr = (ll * len(frames))(*frames)
        return L.pwg_yin_run(plan, wave_, st, len(starts) - 1 if n is None else n, fr, f0, None, None, rows, None)

    assert run(plan=None) == INV and run(wave_=None) == INV and run(f0=None) == INV and run(no_starts=True) == INV
    assert b"null" in L.pwg_last_error()
    assert run(n=0) == INV and run(n=-1) == INV
    assert run(starts=(-1, 100, 250)) == INV and b"negative" in L.pwg_last_error()
    assert run(starts=(0, 100, 50)) == INV and b"decrease" in L.pwg_last_error()
    assert run(starts=(0, 100, 100)) == INV and b"empty" in L.pwg_last_error()
    assert run(starts=(0, 0, 100)) == INV and b"utterance 0 is empty" in L.pwg_last_error()
    assert run(frames=(3, 0)) == INV and b"out_frames[1]" in L.pwg_last_error()
    assert run(frames=(-2, 4)) == INV
    assert run(rows=8) == INV and b"out_rows" in L.pwg_last_error()
    assert run(rows=6) == INV
    assert L.pwg_yin_plan_destroy(None) is None  # a null plan is fine to destroy
    with pytest.raises(ValueError, match="out_rows"):
        _lib.check(run(rows=0))


def test_python_signatures_and_argument_handling():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(yin_estimate) == [("signal", E), ("sample_rate", E), ("pitch_min", 20), ("pitch_max", 20000),
                                    ("frame_stride", 0.01), ("threshold", 0.1)]
    assert params(f0_torchyin) == [("audio", E), ("sampling_rate", E), ("hop_size", 256), ("frame_length", None),
                                   ("pitch_min", 40), ("pitch_max", 10000)]
    assert params(YinF0Extractor.__init__)[1:] == [("sampling_rate", E), ("hop_size", E), ("frame_length", None),
                                                   ("pitch_min", 40), ("pitch_max", 10000), ("threshold", 0.1), ("log", True)]
    ex = YinF0Extractor.from_config(dict(sampling_rate=24000, hop_size=300, win_length=1200, fft_size=2048))
    assert (ex.tau_min, ex.tau_max, ex.hop_size, ex.log, ex.threshold) == (2, 600, 300, True, 0.1)
    assert [ex.frames(t) for t in (1, 1199, 1200, 1500, 13200)] == [1, 1, 1, 2, 41]
    ex = YinF0Extractor(8000, 16, pitch_min=250, pitch_max=2000, log=False)
    assert (ex.tau_min, ex.tau_max) == (4, 32) == orc.lag_bounds(8000, 250, 2000)
    assert (YinF0Extractor(22050, 256).tau_min, YinF0Extractor(22050, 256).tau_max) == (2, 551)
    with pytest.raises(ValueError, match="hop"):
        YinF0Extractor(8000, 0)
    with pytest.raises(ValueError, match="no lag"):
        YinF0Extractor(8000, 16, pitch_min=4000, pitch_max=5000)
    with pytest.raises(ValueError, match="threshold"):
        YinF0Extractor(8000, 16, threshold=0.0)
    with pytest.raises(NotImplementedError, match="1680"):
        YinF0Extractor(24000, 300, pitch_min=10)
    with pytest.raises(ValueError, match="pitch_min"):
        YinF0Extractor(24000, 300, pitch_min=0)
    ex = YinF0Extractor(8000, 16, pitch_min=250)
    assert ex.extract_batch([]) == []
    with pytest.raises(ValueError, match=r"\(T,\)"):
        ex.extract_batch([np.zeros((2, 500), np.float32)], device="cuda:0")
    with pytest.raises(ValueError, match="empty"):
        ex.extract_batch([np.zeros(0, np.float32)], device="cuda:0")
    with pytest.raises(ValueError, match="frames"):
        ex.extract_batch([np.zeros(500, np.float32)], frames=[3, 4], device="cuda:0")
    with pytest.raises(ValueError, match="frames"):
        ex.extract_batch([np.zeros(500, np.float32)], frames=[0], device="cuda:0")
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        ex.extract_batch([torch.zeros(500)], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        yin_estimate(torch.zeros(2, 4000), 8000)
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        yin_estimate(torch.zeros(1, 2, 4000), 8000)
    import copy
    import pickle

    ex._plans = {"key": ctypes.c_void_p(1)}  # what a run leaves: not picklable
    for other in (copy.deepcopy(ex), pickle.loads(pickle.dumps(ex))):
        assert other._plans == {} and (other.tau_min, other.tau_max) == (ex.tau_min, ex.tau_max)
    ex._plans = {}


# ------------------------------------------------------------------ the preprocess CLI's file handling
CONFIG = dict(sampling_rate=8000, fft_size=128, hop_size=50, win_length=80, window="hann", num_mels=16, fmin=None,
              fmax=None, format="npy", trim_silence=False, global_gain_scale=1.0)


def _write_wav(path, x, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(x * 32768.0).astype("<i2").tobytes())


def _oracle_mel_batch(self, waves, device=None):
    return [torch.from_numpy(mel_orc.logmel(np.asarray(w), self.fft_size, self.hop_size, self.win_length, self.melmat,
                                            self.eps, self.log_base, self.amp_floor, self.mean, self.scale).astype(np.float32))
            for w in waves]


def _oracle_f0_batch(self, waves, frames=None, device=None):
    """YinF0Extractor.extract_batch by the float64 oracle, on the CPU."""
    frames = [None] * len(waves) if frames is None else frames
    out = [orc.analyse(np.asarray(w), self.sampling_rate, self.tau_min, self.tau_max, self.hop_size, self.threshold, n)["f0"]
           for w, n in zip(waves, frames)]
    return [torch.from_numpy(orc.log_f0(f) if self.log else f) for f in out]


@pytest.fixture
def wav_dir(tmp_path):
    root = tmp_path / "wavs"
    (root / "spk1").mkdir(parents=True)
    xs = {"utt_a": signal(1500, 8000, (250.0, 400.0), 40), "utt_b": signal(4007, 8000, (220.0, 380.0), 41)}
    _write_wav(root / "utt_a.wav", xs["utt_a"], 8000)
    _write_wav(root / "spk1" / "utt_b.wav", xs["utt_b"], 8000)
    with open(tmp_path / "conf.yml", "w") as f:
        yaml.safe_dump(CONFIG, f)
    return tmp_path, xs


def test_preprocess_cli_writes_f0_only_with_the_flag(wav_dir, monkeypatch):
    from parallelwavegan_amd.bin import preprocess

    tmp, xs = wav_dir
    monkeypatch.setattr(LogMelExtractor, "extract_batch", _oracle_mel_batch)
    monkeypatch.setattr(YinF0Extractor, "extract_batch", _oracle_f0_batch)
    base = ["--rootdir", str(tmp / "wavs"), "--config", str(tmp / "conf.yml"), "--verbose", "0"]
    assert preprocess.main(base + ["--dumpdir", str(tmp / "plain")]) == 0
    assert sorted(os.listdir(tmp / "plain")) == ["utt_a-feats.npy", "utt_a-wave.npy", "utt_b-feats.npy", "utt_b-wave.npy"]
    for dump, extra in (("f0", []), ("f0_1", ["--batch-samples", "1"])):
        assert preprocess.main(base + ["--dumpdir", str(tmp / dump), "--extract-f0-yin"] + extra) == 0
        assert sorted(os.listdir(tmp / dump)) == ["utt_a-f0.npy", "utt_a-feats.npy", "utt_a-wave.npy", "utt_b-f0.npy",
                                                  "utt_b-feats.npy", "utt_b-wave.npy"]  # and no -excitation.npy
    for utt, x in xs.items():
        feats, audio, f0 = (np.load(tmp / "f0" / f"{utt}-{kind}.npy") for kind in ("feats", "wave", "f0"))
        # the flag changes nothing else
        assert np.array_equal(feats, np.load(tmp / "plain" / f"{utt}-feats.npy"))
        assert np.array_equal(audio, np.load(tmp / "plain" / f"{utt}-wave.npy"))
        assert f0.dtype == np.float32 and f0.shape == (len(feats),) and len(audio) == len(feats) * 50
        # win_length 80 -> pitch_min 200 Hz -> tau_max 40; computed on the fitted audio, fitted to the mel length
        own = orc.n_frames(len(audio), 40, 50)
        assert own < len(feats)  # the contour is shorter than the mel: its last value is held
        want = orc.f0_torchyin(audio, 8000, hop_size=50, frame_length=80, frames=len(feats))
        assert np.array_equal(f0, want) and (f0[own:] == f0[own - 1]).all()
        assert np.array_equal(np.load(tmp / "f0_1" / f"{utt}-f0.npy"), f0)  # one utterance per launch


def test_preprocess_cli_refusals_come_before_any_write(wav_dir, monkeypatch):
    from parallelwavegan_amd.bin import preprocess

    tmp, xs = wav_dir
    monkeypatch.setattr(LogMelExtractor, "extract_batch", _oracle_mel_batch)
    monkeypatch.setattr(YinF0Extractor, "extract_batch", _oracle_f0_batch)

    def run(config=None, extra=()):
        path = tmp / "c.yml"
        with open(path, "w") as f:
            yaml.safe_dump(dict(CONFIG, **(config or {})), f)
        return preprocess.main(["--dumpdir", str(tmp / "dump"), "--verbose", "0", "--config", str(path), "--rootdir",
                                str(tmp / "wavs"), "--extract-f0-yin"] + list(extra))

    # the config keys raise as before, with the flag too
    for config in (dict(use_f0=True), dict(use_f0_and_excitation=True)):
        with pytest.raises(NotImplementedError, match="f0 / excitation extraction is not available"):
            run(config)
    with pytest.raises(NotImplementedError, match="1680"):
        run(dict(win_length=4000, fft_size=4096))            # tau_max 2000: beyond what the kernel's tile holds
    with pytest.raises(ValueError, match="no lag"):
        run(dict(win_length=2, fft_size=128))                # tau_max 1
    with pytest.raises(ValueError, match="different sampling rate"):
        run(dict(sampling_rate=16000))
    assert not os.path.exists(tmp / "dump")
