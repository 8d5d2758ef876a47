"""Log-mel extraction without a GPU: the float64 oracle (tests/logmel_oracle.py) against torch.stft in
float64 and against the reference fixtures (tests/golden/logmel, made by make_golden_logmel.py), the
condition on the test inputs (the reference's own fp32 path stays within 1e-5 of the oracle on them),
slaney_mel_basis, pwg_mel_frames, the argument checks of the C-ABI and of the Python classes that need no
device, and the preprocess CLI's file handling with the extractor replaced by the oracle.

Measured here: oracle vs torch.stft float64 amplitude 6.8e-14 at the most; oracle vs the reference
fixtures 8.7e-7 (log10), 2.1e-6 (log2); the reference's fp32 path vs the oracle over the test
inputs r = 3.48e-6 at the most (R_MAX of tests/test_gpu_logmel.py is set from it)."""

import ctypes
import os
import wave

import numpy as np
import pytest
import torch
import yaml

import logmel_oracle as orc
from logmel_helpers import CASES, FIXTURES, P, load_fixture, plan_create, reference_fp32_errors, signal
from parallelwavegan_amd import LogMelExtractor, MelSpectrogram, _lib, logmelfilterbank, slaney_mel_basis


def test_fixture_set_is_complete():
    assert FIXTURES == ["lm_A_T165_log2", "lm_A_T33", "lm_B75_T320_ln", "lm_B80_T320", "lm_libritts_T1025",
                        "lm_libritts_T2700", "lm_lj_T2916"]
    for name in FIXTURES:
        fx = load_fixture(name)
        m = fx["meta"]
        assert "slaney_mel_basis" in m["mel_basis"]
        assert fx["y"].shape == (1 + len(fx["x"]) // m["hop_size"], m["num_mels"])
        assert fx["melmat"].shape == (m["num_mels"], m["fft_size"] // 2 + 1) and fx["melmat"].dtype == np.float32


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_fixture(name):
    """The reference's STFT, clamps, matmul and log (fp32, CPU) against the float64 oracle: 1e-5, in the
    fixture's own log base."""
    fx = load_fixture(name)
    m = fx["meta"]
    want = orc.logmel(fx["x"], m["fft_size"], m["hop_size"], m["win_length"], fx["melmat"], m["eps"], m["log_base"],
                      amp_floor=True)
    err = float(np.abs(want - fx["y"]).max())
    print(f"{name}: max|oracle - reference| {err:.2e} (log base {m['log_base']})")
    assert err <= 1e-5


@pytest.mark.parametrize("n_fft, hop, win, T", [(64, 16, 64, 33), (128, 50, 75, 333), (1024, 256, 1024, 2916),
                                                (2048, 300, 1200, 2700)])
def test_oracle_amplitude_is_torch_stft_in_float64(n_fft, hop, win, T):
    x = np.random.RandomState(T).standard_normal(T)
    st = torch.stft(torch.from_numpy(x)[None], n_fft, hop, win, window=torch.hann_window(win, dtype=torch.float64),
                    center=True, return_complex=True)[0]
    want = st.abs().numpy().T
    got = orc.amplitude(x, n_fft, hop, win)
    err = float(np.abs(got - want).max())
    print(f"{n_fft}/{hop}/{win}: max|oracle - torch.stft float64| {err:.1e}")
    assert got.shape == want.shape and err <= 1e-10


def test_short_utterance_is_where_torch_refuses():
    x = torch.zeros(1, 1024)
    with pytest.raises(RuntimeError):
        torch.stft(x, 2048, 300, 1200, window=torch.hann_window(1200), center=True, return_complex=True)
    assert torch.stft(torch.zeros(1, 1025), 2048, 300, 1200, window=torch.hann_window(1200), center=True,
                      return_complex=True).shape[-1] == 4
    with pytest.raises(ValueError):
        orc.frames(np.zeros(1024), 2048, 300)
    assert orc.frames(np.zeros(1025), 2048, 300).shape == (4, 2048)


def test_inputs_keep_the_reference_fp32_path_within_1e5():
    """The condition on the inputs that ORACLE_ATOL rests on: on every non-silent test signal the
    reference's own fp32 path (CPU torch.stft + fp32 matmul) is within 1e-5 of the oracle."""
    errs = reference_fp32_errors()
    for case, e in errs.items():
        print(f"{case}: reference fp32 vs oracle {e:.2e}")
    assert set(errs) == set(CASES)
    assert max(errs.values()) <= 1e-5


def test_slaney_mel_basis_properties():
    w = slaney_mel_basis(24000, 2048, 80, 80, 7600)
    assert w.shape == (80, 1025) and w.dtype == np.float32
    assert (w >= 0).all() and (w.max(axis=1) > 0).all()                  # no empty filter
    assert int((w > 0).sum(axis=0).max()) == 2                           # at most 2 filters per bin
    assert abs(float(w.max()) - 0.027976695) <= 1e-9
    nz = lambda i: np.flatnonzero(w[i])  # noqa: E731
    assert (nz(0)[0], nz(0)[-1]) == (7, 12) and (nz(79)[0], nz(79)[-1]) == (603, 648)
    # defaults: fmin None -> 0, fmax None -> sr / 2; the triangles then end on the Nyquist bin with weight 0
    d = slaney_mel_basis(16000, 128, 16)
    assert np.array_equal(d, slaney_mel_basis(16000, 128, 16, 0, 8000)) and d[:, -1].max() == 0
    # Slaney norm: every triangle has unit area over the frequency axis (in Hz), up to the bin grid
    area = w.sum(axis=1) * (24000 / 2048)
    assert np.abs(area - 1).max() < 0.1


def test_frame_count(built_lib):
    L = built_lib
    assert [L.pwg_mel_frames(t, 300) for t in (0, 299, 300, 1025, 2700)] == [1, 1, 2, 4, 10]
    assert L.pwg_mel_frames(33, 16) == 3 and L.pwg_mel_frames(1 << 40, 1) == (1 << 40) + 1
    assert L.pwg_mel_frames(-1, 16) == -1 and L.pwg_mel_frames(16, 0) == -1
    assert _lib.PWG_MEL_FRAME_TILE == 64
    src = open(os.path.join(_lib.REPO_DIR, "include", "pwg_mel.h")).read()
    assert "PWG_MEL_FRAME_TILE = 64" in src and "PWG_MEL_MAX_MELS = 128" in src


def test_plan_argument_checks_come_before_any_device_call(built_lib):
    """Every failing check returns its status without a HIP call (this test runs without a GPU)."""
    L, INV, UNS = built_lib, _lib.PWG_ERR_INVALID, _lib.PWG_ERR_UNSUPPORTED
    assert plan_create(L, melmat=None) == INV and plan_create(L, plan=None) == INV
    for n_fft in (63, 0, -64, 1):
        assert plan_create(L, n_fft=n_fft, win=1, count=4 * (n_fft // 2 + 1)) == INV, n_fft
    assert plan_create(L, n_fft=64, win=66) == INV and b"win_length" in L.pwg_last_error()
    assert plan_create(L, win=0) == INV
    assert plan_create(L, hop=0) == INV and plan_create(L, hop=-16) == INV
    assert plan_create(L, num_mels=0, count=0) == INV and plan_create(L, num_mels=-1, count=-33) == INV
    assert plan_create(L, count=4 * 33 + 1) == INV and b"melmat" in L.pwg_last_error()
    assert plan_create(L, count=4 * 32) == INV
    for eps in (-1e-10, float("nan"), float("inf")):
        assert plan_create(L, eps=eps) == INV, eps
    assert plan_create(L, amp_floor=2) == INV
    assert plan_create(L, mean=P) == INV and plan_create(L, scale=P) == INV
    # the unsupported ones, reported only when nothing is invalid
    assert plan_create(L, window=1) == UNS and b"Hann" in L.pwg_last_error()
    for base in (3.0, 1.0, -10.0, float("nan")):
        assert plan_create(L, log_base=base) == UNS, base
    assert plan_create(L, num_mels=129) == UNS
    assert plan_create(L, n_fft=1 << 17, win=64) == UNS
    assert plan_create(L, n_fft=8192, win=8192, hop=2048) == UNS and b"LDS" in L.pwg_last_error()
    # a legal geometry whose basis would take 8 GB of host memory is refused, not attempted
    assert plan_create(L, n_fft=65536, win=30000, hop=1) == UNS and b"1 GiB" in L.pwg_last_error()
    assert plan_create(L, window=1, hop=0) == INV  # invalid wins over unsupported
    with pytest.raises(NotImplementedError, match="log_base"):
        _lib.check(plan_create(L, log_base=3.0))
    with pytest.raises(ValueError, match="hop"):
        _lib.check(plan_create(L, hop=0))


def test_run_argument_checks_without_a_plan(built_lib):
    L = built_lib
    starts = (ctypes.c_longlong * 2)(0, 100)
    assert L.pwg_mel_run(None, P, starts, 1, P, 7, None) == _lib.PWG_ERR_INVALID
    assert L.pwg_mel_plan_destroy(None) is None  # a null plan is fine to destroy


def test_modules_copy_and_pickle_without_their_plans():
    import copy
    import pickle

    m = MelSpectrogram()
    m._plans = {"key": ctypes.c_void_p(1)}  # what a forward leaves: not picklable
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert other._plans == {} and torch.equal(other.melmat, m.melmat) and other.hop_size == 256
    ex = LogMelExtractor(16000, num_mels=8)
    ex._plans = {"key": ctypes.c_void_p(1)}
    for other in (copy.deepcopy(ex), pickle.loads(pickle.dumps(ex))):
        assert other._plans == {} and np.array_equal(other.melmat, ex.melmat)
    m._plans = ex._plans = {}  # (the fake handles must not reach a destructor)


def test_python_argument_handling():
    with pytest.raises(NotImplementedError, match="window"):
        LogMelExtractor(16000, window="hamming")
    with pytest.raises(NotImplementedError, match="window"):
        MelSpectrogram(window="hamming")
    with pytest.raises(ValueError, match="not implemented"):
        MelSpectrogram(window="nonsense")  # the reference's own refusal
    for kw in (dict(normalized=True), dict(onesided=False), dict(center=False)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            MelSpectrogram(**kw)
    for cls, sr in ((lambda **k: LogMelExtractor(16000, **k), None), (MelSpectrogram, None)):
        with pytest.raises(ValueError, match="fft_size"):
            cls(fft_size=1023)
        with pytest.raises(ValueError, match="win_length"):
            cls(fft_size=512, win_length=1024)
        with pytest.raises(ValueError, match="hop_size"):
            cls(hop_size=0)
        with pytest.raises(ValueError, match="num_mels"):
            cls(num_mels=0)
        with pytest.raises(ValueError, match="log_base"):
            cls(log_base=3.0)
        with pytest.raises(NotImplementedError, match="num_mels"):
            cls(num_mels=129)
    with pytest.raises(ValueError, match="melmat"):
        LogMelExtractor(16000, fft_size=64, hop_size=16, num_mels=4, melmat=np.zeros((4, 32), np.float32))
    with pytest.raises(ValueError, match="num_mels"):
        LogMelExtractor(16000, num_mels=8, stats=np.zeros((2, 80), np.float32))
    with pytest.raises(ValueError, match="stats"):
        LogMelExtractor(16000, num_mels=8, stats=np.zeros((3, 8), np.float32))
    m = MelSpectrogram()
    assert (m.fft_size, m.win_length, m.hop_size, m.center, m.normalized, m.onesided, m.window, m.eps, m.log_base) == \
        (1024, 1024, 256, True, False, True, "hann", 1e-10, 10.0)
    assert tuple(m.melmat.shape) == (513, 80) and list(m.state_dict()) == ["melmat"]
    assert np.array_equal(m.melmat.numpy().T, slaney_mel_basis(22050, 1024, 80, 80, 7600))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        m(torch.zeros(2, 4096))
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        m(torch.zeros(4096))
    ex = LogMelExtractor.from_config(dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=1200, num_mels=80,
                                          fmin=80, fmax=7600), stats=np.ones((2, 80), np.float32))
    assert (ex.fft_size, ex.hop_size, ex.win_length, ex.num_mels, ex.frames(2700)) == (2048, 300, 1200, 80, 10)
    assert np.array_equal(ex.melmat, slaney_mel_basis(24000, 2048, 80, 80, 7600)) and ex.amp_floor is False
    with pytest.raises(ValueError, match=r"\(T,\)"):
        ex.extract_batch([np.zeros((2, 5000), np.float32)], device="cuda:0")
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        ex.extract_batch([torch.zeros(5000)], device="cpu")
    assert ex.extract_batch([]) == []
    assert callable(logmelfilterbank)


# ------------------------------------------------------------------ the preprocess CLI's file handling
CONFIG = dict(sampling_rate=16000, fft_size=128, hop_size=50, win_length=80, window="hann", num_mels=16, fmin=None,
              fmax=None, format="npy", trim_silence=False, global_gain_scale=1.0)


def _write_wav(path, x, sr, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(np.repeat(x, channels) * 32768.0).astype("<i2").tobytes())


def _oracle_extract_batch(self, waves, device=None):
    """LogMelExtractor.extract_batch by the float64 oracle, on the CPU."""
    return [torch.from_numpy(orc.logmel(np.asarray(w), self.fft_size, self.hop_size, self.win_length, self.melmat, self.eps,
                                        self.log_base, self.amp_floor, self.mean, self.scale).astype(np.float32))
            for w in waves]


@pytest.fixture
def wav_dir(tmp_path):
    root = tmp_path / "wavs"
    (root / "spk1").mkdir(parents=True)
    xs = {"utt_a": signal(333, 16000, 20, 40), "utt_b": signal(1207, 16000, 50, 41)}
    _write_wav(root / "utt_a.wav", xs["utt_a"], 16000)
    _write_wav(root / "spk1" / "utt_b.wav", xs["utt_b"], 16000)
    with open(tmp_path / "conf.yml", "w") as f:
        yaml.safe_dump(CONFIG, f)
    return tmp_path, xs


def test_preprocess_cli_files(wav_dir, monkeypatch):
    from parallelwavegan_amd.bin import preprocess

    tmp, xs = wav_dir
    monkeypatch.setattr(LogMelExtractor, "extract_batch", _oracle_extract_batch)
    stats = np.stack([np.linspace(-5, -3, 16), np.linspace(0.5, 2, 16)]).astype(np.float32)
    np.save(tmp / "stats.npy", stats)
    for dump, extra in (("dump", []), ("dump_norm", ["--stats", str(tmp / "stats.npy")]), ("dump_1", ["--batch-samples", "1"])):
        assert preprocess.main(["--rootdir", str(tmp / "wavs"), "--dumpdir", str(tmp / dump), "--config",
                                str(tmp / "conf.yml"), "--verbose", "0"] + extra) == 0
        assert sorted(os.listdir(tmp / dump)) == ["utt_a-feats.npy", "utt_a-wave.npy", "utt_b-feats.npy", "utt_b-wave.npy"]
    for utt, x in xs.items():
        feats, audio = np.load(tmp / "dump" / f"{utt}-feats.npy"), np.load(tmp / "dump" / f"{utt}-wave.npy")
        assert feats.dtype == np.float32 and audio.dtype == np.float32
        assert feats.shape == (1 + len(x) // 50, 16) and len(audio) == len(feats) * 50
        # the PCM16 signal comes back exactly; past its end the last sample is held (bin/preprocess.py:403)
        n = min(len(x), len(audio))
        assert np.array_equal(audio[:n], x[:n]) and (audio[n:] == x[-1]).all()
        want = orc.logmel(x, 128, 50, 80, slaney_mel_basis(16000, 128, 16), amp_floor=False)
        assert np.abs(feats - want).max() <= 1e-6
        norm = np.load(tmp / "dump_norm" / f"{utt}-feats.npy")
        assert np.abs(norm - (want - stats[0]) / stats[1]).max() <= 2e-6
        assert np.array_equal(np.load(tmp / "dump_1" / f"{utt}-feats.npy"), feats)  # one utterance per launch


def test_preprocess_cli_refusals(wav_dir, monkeypatch):
    from parallelwavegan_amd.bin import preprocess

    tmp, xs = wav_dir
    monkeypatch.setattr(LogMelExtractor, "extract_batch", _oracle_extract_batch)
    base = ["--dumpdir", str(tmp / "dump"), "--verbose", "0"]

    def run(config=None, rootdir=True, extra=()):
        path = tmp / "c.yml"
        with open(path, "w") as f:
            yaml.safe_dump(dict(CONFIG, **(config or {})), f)
        return preprocess.main(base + ["--config", str(path)] + (["--rootdir", str(tmp / "wavs")] if rootdir else [])
                               + list(extra))

    with pytest.raises(ValueError, match="different sampling rate"):
        run(dict(sampling_rate=22050))
    with pytest.raises(NotImplementedError, match="kaldiio"):
        run(extra=["--scp", "wav.scp"])
    with pytest.raises(NotImplementedError, match="kaldiio"):
        run(extra=["--segments", "segments"])
    with pytest.raises(ValueError, match="--rootdir"):
        run(rootdir=False)
    for config, match in ((dict(format="hdf5"), "hdf5"), (dict(trim_silence=True), "trim_silence"),
                          (dict(sampling_rate_for_feats=8000), "resampling"), (dict(global_gain_scale=0.5), "global_gain"),
                          (dict(use_f0_and_excitation=True), "f0"), (dict(window="hamming"), "window")):
        with pytest.raises(NotImplementedError, match=match):
            run(config)
    with pytest.raises(NotImplementedError, match="stats.npy"):
        run(extra=["--stats", "stats.h5"])
    assert not os.path.exists(tmp / "dump")  # every refusal came before the first write
    _write_wav(tmp / "wavs" / "stereo.wav", xs["utt_a"], 16000, channels=2)
    with pytest.raises(ValueError, match="multi-channel"):
        run()
    os.remove(tmp / "wavs" / "stereo.wav")
    _write_wav(tmp / "wavs" / "short.wav", xs["utt_a"][:64], 16000)
    with pytest.raises(ValueError, match="too short"):
        run()
