"""Audio conditioning without a GPU (include/pwg_wave.h): the float64 oracle (tests/wave_oracle.py) against
scipy and on hand-built cases, the length helpers against the closed forms, every C-ABI argument check that
comes before a HIP call, the CLI's refusals, and the margin condition of the GPU trim tests: in the oracle
every frame's decision of every case is further than 1e-3 (relative) from the threshold, while the kernel's
fp32 power is within (fl + 2) 2^-24 <= 1.3e-4 of the oracle's, so no decision can flip and no frame is left
out of the comparison."""

import ctypes
import os
import wave as wave_module

import numpy as np
import pytest
import yaml

import wave_oracle as orc
from wave_helpers import (F, GEOMETRIES, LENGTHS, MARGIN, P, PAD_MODES, RATIOS, TILE, TRIM_CASES, length_for_outputs,
                          resample_plan_create, resample_signal, samples_for_frames, starts, trim_oracle,
                          trim_plan_create, trim_power_bound, trim_signal)
from parallelwavegan_amd import _lib, audio

INVALID, UNSUPPORTED = _lib.PWG_ERR_INVALID, _lib.PWG_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("up, down", RATIOS, ids=lambda v: str(v))
def test_oracle_resampler_and_taps_match_scipy(up, down):
    signal = pytest.importorskip("scipy.signal")
    taps = orc.kaiser_taps(up, down)
    half = 10 * max(up, down)
    want = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert taps.shape == want.shape and np.abs(taps - want).max() <= 1e-12
    mine = audio.kaiser_lowpass_taps(up, down)                                    # the package's own restatement
    assert mine.dtype == np.float64 and mine.shape == want.shape and np.abs(mine - want).max() <= 1e-12
    assert np.array_equal(audio.kaiser_lowpass_taps(2 * up, 2 * down), mine)      # reduced by the gcd first
    for T in LENGTHS:
        x = resample_signal(T, 3).astype(np.float64)
        got, ref = orc.resample(x, up, down), signal.resample_poly(x, up, down)
        assert got.shape == ref.shape == (orc.resample_out_len(T, up, down),)
        assert np.abs(got - ref).max() <= 1e-12, (T, np.abs(got - ref).max())


def test_oracle_resampler_copy_and_custom_taps():
    x = resample_signal(50, 1)
    assert np.array_equal(orc.resample(x, 3, 3), x.astype(np.float64))
    y = orc.resample(x, 1, 2, taps=[0.0, 1.0, 0.0])   # a unit tap: plain decimation
    assert np.array_equal(y, x[::2].astype(np.float64))
    y = orc.resample(x, 2, 1, taps=[0.5, 1.0, 0.5])   # linear interpolation
    assert np.array_equal(y[::2], x.astype(np.float64)) and np.allclose(y[1:-1:2], (x[:-1].astype(np.float64) + x[1:]) / 2)


def test_trim_oracle_all_zero_is_kept_whole():
    for fl, hop, top_db in GEOMETRIES.values():
        for mode in PAD_MODES:
            assert orc.trim_bounds(np.zeros(5 * hop + 3), fl, hop, top_db, mode) == (0, 5 * hop + 3)
    assert orc.trim_bounds(np.zeros(1), 64, 16, 20) == (0, 1)


def test_trim_oracle_burst_with_known_lead_and_tail():
    """A burst of constant power on [10 h, 20 h) in exact silence. At 64 / 16 / 20 dB a frame is kept when it
    holds more than 1 % of a full frame's power, which one sample of the burst already gives: the frames
    centred at 9 h (it reaches to 11 h) to 21 h (it starts at 19 h), so the bounds are [9 h, 22 h)."""
    fl, hop, top_db = 64, 16, 20
    T = 30 * hop
    x = np.zeros(T)
    x[10 * hop:20 * hop] = 0.5
    n = orc.trim_frames(T, fl, hop)
    overlap = np.array([len(range(max(10 * hop, t * hop - 32), min(20 * hop, t * hop + 32))) for t in range(n)])
    keep = np.flatnonzero(overlap / 64.0 > 0.01)          # P[t] / P_max > 10^-2 with P_max = 0.25
    want = (keep[0] * hop, min(T, (keep[-1] + 1) * hop))
    assert want == (9 * hop, 22 * hop)
    assert orc.trim_bounds(x, fl, hop, top_db) == want
    a, b = want
    assert (x[:a] == 0).all() and (x[b:] == 0).all() and x[a:b].any()


def test_trim_oracle_pad_modes_differ_on_loud_edges():
    """Loud in its first hop: the zero pad leaves the first frame 16 loud samples of 64, the mirror 31. With the
    threshold between the two shares the zero pad trims the beginning and the mirror keeps it."""
    fl, hop = 64, 16
    x = np.full(40 * hop, 1e-4)
    x[:hop] = 0.5
    x[20 * hop:22 * hop] = 1.0
    pz, pr = orc.trim_power(x, fl, hop, orc.PAD_ZERO), orc.trim_power(x, fl, hop, orc.PAD_REFLECT)
    assert abs(pz[0] / (0.25 * 16 / 64) - 1) < 1e-3 and abs(pr[0] / (0.25 * 31 / 64) - 1) < 1e-3
    assert np.array_equal(orc.padded(x, 32, orc.PAD_REFLECT), np.pad(x, 32, mode="reflect"))
    assert np.array_equal(orc.padded(x[:5], 32, orc.PAD_REFLECT), np.pad(x[:5], 32, mode="reflect"))  # many mirrors
    assert pz.max() == pr.max() and abs(pz.max() - 0.5) < 1e-6
    top_db = -10 * np.log10(0.18)                        # at 0.18 of the maximum: between 0.125 and 0.242
    assert orc.trim_bounds(x, fl, hop, top_db, orc.PAD_ZERO)[0] > hop
    assert orc.trim_bounds(x, fl, hop, top_db, orc.PAD_REFLECT)[0] == 0


# ------------------------------------------------------------------------------------- length helpers
def test_frames_and_out_len_match_the_closed_forms(built_lib):
    L = built_lib
    for fl, hop in ((64, 16), (50, 16), (51, 16), (500, 160), (2048, 512), (7, 3), (1, 1)):
        for T in (1, 2, max(1, hop - 1), hop, hop + 1, fl, fl + 1, 10 * hop + 7, 12345):
            want = 1 + (T + 2 * (fl // 2) - fl) // hop
            assert L.pwg_trim_frames(T, fl, hop) == want == orc.trim_frames(T, fl, hop) == audio.trim_frames(T, fl, hop)
            if fl % 2 == 0:
                assert want == 1 + T // hop
            assert want == 1 + (len(np.pad(np.zeros(T), fl // 2)) - fl) // hop   # librosa's centred framing
    for up, down in RATIOS + ((2, 4), (441, 480), (640, 1), (1, 640)):
        for T in LENGTHS + (1 << 33,):
            want = -(-T * up // down)
            assert L.pwg_resample_out_len(T, up, down) == want == audio.resample_out_len(T, up, down)
    assert L.pwg_trim_frames(0, 64, 16) == -1 and L.pwg_trim_frames(5, 0, 16) == -1 and L.pwg_trim_frames(5, 64, 0) == -1
    assert L.pwg_resample_out_len(0, 1, 2) == -1 and L.pwg_resample_out_len(5, 0, 2) == -1 and L.pwg_resample_out_len(5, 1, 0) == -1


def test_case_builders():
    for g, (fl, hop, _) in GEOMETRIES.items():
        for n in (F - 1, F, F + 1, 2 * F + 3):
            assert orc.trim_frames(samples_for_frames(n, fl, hop), fl, hop) == n
    for up, down in RATIOS:
        for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
            got = orc.resample_out_len(length_for_outputs(n, up, down), up, down)
            assert got >= n and (got == n or up > down)
    counts = {g: sorted(orc.trim_frames(c[1], *GEOMETRIES[g][:2]) for c in TRIM_CASES if c[0] == g) for g in GEOMETRIES}
    for g in ("g64", "g50", "g500"):
        assert {F - 1, F, F + 1, 2 * F + 3} <= set(counts[g]) and len(counts[g]) == 8
    assert len(counts["g2048"]) == 1


# ---------------------------------------------------------------------------------- the margin condition
@pytest.mark.parametrize("pad_mode", PAD_MODES)
def test_every_trim_decision_has_margin(pad_mode):
    worst = np.inf
    for case in TRIM_CASES:
        res = trim_oracle(case, pad_mode)
        fl = GEOMETRIES[case[0]][0]
        assert trim_power_bound(fl) <= 1.3e-4 < MARGIN
        assert res["margin"].min() > MARGIN, (case, res["margin"].min())    # every frame: none is left out
        a, b = res["bounds"]
        assert 0 <= a < b <= case[1]
        worst = min(worst, res["margin"].min())
    # the cases trim something on both sides somewhere
    assert any(trim_oracle(c, pad_mode)["bounds"][0] > 0 for c in TRIM_CASES)
    assert any(trim_oracle(c, pad_mode)["bounds"][1] < c[1] for c in TRIM_CASES)
    print(f"{pad_mode}: smallest margin over {len(TRIM_CASES)} cases {worst:.3g}")


def test_trim_cases_follow_their_lead_and_tail():
    """The bounds lie within a frame of the tone's edges."""
    for case in TRIM_CASES:
        g, T, lead, tail, _ = case
        fl, hop, _ = GEOMETRIES[g]
        a, b = trim_oracle(case, orc.PAD_ZERO)["bounds"]
        assert lead - fl <= a <= lead and T - tail <= b <= min(T, T - tail + fl), (case, a, b)


# ------------------------------------------------------------------------------- C-ABI argument checks
def test_trim_argument_checks(built_lib):
    L = built_lib
    assert trim_plan_create(L, plan=None) == INVALID and b"null" in L.pwg_last_error()
    for kw in (dict(fl=0), dict(hop=0), dict(top_db=0.0), dict(top_db=-3.0), dict(top_db=float("nan")),
               dict(top_db=float("inf")), dict(pad_mode=2), dict(pad_mode=-1)):
        assert trim_plan_create(L, **kw) == INVALID, kw
    assert b"pad_mode" in L.pwg_last_error()
    assert trim_plan_create(L, fl=_lib.PWG_TRIM_MAX_TILE_SPAN, hop=1) == UNSUPPORTED
    assert trim_plan_create(L, fl=2048, hop=2400) == UNSUPPORTED and b"LDS" in L.pwg_last_error()
    assert trim_plan_create(L, fl=0, hop=1 << 20) == INVALID         # INVALID is checked first
    run = L.pwg_trim_run
    ok = starts(0, 100, 250)
    for args in ((None, P, ok, 2, P), (P, None, ok, 2, P), (P, P, None, 2, P), (P, P, ok, 2, None)):
        assert run(*args, None, 0, None) == INVALID and b"null" in L.pwg_last_error()
    assert run(P, P, ok, 0, P, None, 0, None) == INVALID
    assert run(P, P, starts(-1, 100), 1, P, None, 0, None) == INVALID and b"negative" in L.pwg_last_error()
    assert run(P, P, starts(0, 100, 50), 2, P, None, 0, None) == INVALID and b"decrease" in L.pwg_last_error()
    assert run(P, P, starts(0, 100, 100), 2, P, None, 0, None) == INVALID and b"empty" in L.pwg_last_error()
    L.pwg_trim_plan_destroy(None)


def test_resample_argument_checks(built_lib):
    L = built_lib
    assert resample_plan_create(L, plan=None) == INVALID and resample_plan_create(L, taps=None) == INVALID
    for kw in (dict(up=0), dict(down=0), dict(up=-2), dict(tap_count=0), dict(tap_count=40), dict(tap_count=-1)):
        assert resample_plan_create(L, **kw) == INVALID, kw
    assert b"odd" in L.pwg_last_error()
    assert resample_plan_create(L, up=641, down=1) == UNSUPPORTED and b"MAX_RATE" in L.pwg_last_error()
    assert resample_plan_create(L, up=1, down=641) == UNSUPPORTED
    assert resample_plan_create(L, up=1, down=2, tap_count=_lib.PWG_RESAMPLE_MAX_TAPS + 2) == UNSUPPORTED
    assert resample_plan_create(L, up=641, down=1, tap_count=40) == INVALID      # INVALID is checked first
    run = L.pwg_resample_run
    ok = starts(0, 100, 250)
    for args in ((None, P, ok, 2, P), (P, None, ok, 2, P), (P, P, None, 2, P), (P, P, ok, 2, None)):
        assert run(*args, 125, None) == INVALID and b"null" in L.pwg_last_error()
    assert run(P, P, ok, 0, P, 0, None) == INVALID
    assert run(P, P, starts(-5, 100), 1, P, 50, None) == INVALID
    assert run(P, P, starts(0, 100, 50), 2, P, 50, None) == INVALID and b"decrease" in L.pwg_last_error()
    assert run(P, P, starts(0, 0, 50), 2, P, 50, None) == INVALID and b"empty" in L.pwg_last_error()
    L.pwg_resample_plan_destroy(None)
    assert L.pwg_resample_plan_tile(None) == -1


def test_fit_argument_checks(built_lib):
    L = built_lib
    run = L.pwg_wave_fit_run
    s, n, o = starts(0, 100), starts(100, 50), starts(0, 120, 130)
    one = ctypes.c_float(1.0)
    for args in ((None, s, n, P, o), (P, None, n, P, o), (P, s, None, P, o), (P, s, n, None, o), (P, s, n, P, None)):
        assert run(*args, 2, one, None, None) == INVALID and b"null" in L.pwg_last_error()
    assert run(P, s, n, P, o, 0, one, None, None) == INVALID
    assert run(P, starts(0, -1), n, P, o, 2, one, None, None) == INVALID and b"src_start" in L.pwg_last_error()
    assert run(P, s, starts(100, 0), P, o, 2, one, None, None) == INVALID and b"src_len" in L.pwg_last_error()
    assert run(P, s, n, P, starts(0, 120, 100), 2, one, None, None) == INVALID and b"decrease" in L.pwg_last_error()
    assert run(P, s, n, P, starts(0, 120, 120), 2, one, None, None) == INVALID and b"empty" in L.pwg_last_error()
    assert run(P, s, n, P, starts(-1, 120, 130), 2, one, None, None) == INVALID
    for g in (float("nan"), float("inf"), -float("inf")):
        assert run(P, s, n, P, o, 2, ctypes.c_float(g), None, None) == INVALID and b"gain" in L.pwg_last_error()


def test_python_checks_come_before_a_device():
    with pytest.raises(ValueError):
        audio.kaiser_lowpass_taps(0, 1)
    with pytest.raises(ValueError, match="trim_threshold_in_db"):
        audio.AudioConditioner(16000, trim_silence=True, trim_threshold_in_db=0)
    with pytest.raises(NotImplementedError, match="640"):
        audio.AudioConditioner(16000, sampling_rate_for_feats=16001)
    with pytest.raises(NotImplementedError):
        audio.AudioConditioner(24000, trim_silence=True, trim_frame_size=1 << 16)
    c = audio.AudioConditioner.from_config(dict(sampling_rate=22050, trim_silence=True, trim_threshold_in_db=60,
                                                trim_frame_size=2048, trim_hop_size=512, global_gain_scale=0.0))
    assert c.trim_silence and c.global_gain_scale == 1.0 and (c.trim_frame_size, c.trim_hop_size) == (2048, 512)
    with pytest.raises(ValueError, match="empty"):
        c.trim_batch([np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match=r"\(T,\)"):
        c.fit_batch([np.zeros((4, 2), np.float32)], [4])
    import pickle

    c._plans["x"] = object()
    assert pickle.loads(pickle.dumps(c))._plans == {}


# ------------------------------------------------------------------------------------------------- CLI
CONFIG = dict(sampling_rate=16000, fft_size=128, hop_size=50, win_length=80, window="hann", num_mels=16, fmin=20, fmax=7000,
              format="npy", trim_silence=False, global_gain_scale=1.0)


def _write_wav(path, x, sr):
    with wave_module.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.asarray(x) * 32768.0).astype("<i2").tobytes())


def test_cli_refusals_with_and_without_the_flags(tmp_path):
    """Every refusal comes before the first write (and before a GPU is needed)."""
    from parallelwavegan_amd.bin import preprocess

    (tmp_path / "wavs").mkdir()
    _write_wav(tmp_path / "wavs" / "a.wav", trim_signal(800, 100, 100, 1), 16000)

    def run(config=None, extra=()):
        with open(tmp_path / "c.yml", "w") as f:
            yaml.safe_dump(dict(CONFIG, **(config or {})), f)
        return preprocess.main(["--dumpdir", str(tmp_path / "dump"), "--verbose", "0", "--config", str(tmp_path / "c.yml"),
                                "--rootdir", str(tmp_path / "wavs")] + list(extra))

    # without the flags: the old refusals, their messages now naming the flag
    for config, exc, match in ((dict(trim_silence=True), NotImplementedError, "trim_silence.*--condition-audio"),
                               (dict(sampling_rate_for_feats=8000), NotImplementedError, "resampling.*--condition-audio"),
                               (dict(global_gain_scale=0.8), NotImplementedError, "global_gain.*--condition-audio"),
                               (dict(sampling_rate=22050), ValueError, "different sampling rate.*--resample-input")):
        with pytest.raises(exc, match=match):
            run(config)
    # --resample-input alone does not unlock the config keys, --condition-audio alone not the other rate
    with pytest.raises(NotImplementedError, match="trim_silence"):
        run(dict(trim_silence=True), ["--resample-input"])
    with pytest.raises(ValueError, match="different sampling rate"):
        run(dict(sampling_rate=22050), ["--condition-audio"])
    # with the flag: --scp and hdf5 still refuse, and so do a hop that does not divide and a ratio out of range
    with pytest.raises(NotImplementedError, match="kaldiio"):
        run(extra=["--condition-audio", "--scp", "wav.scp"])
    with pytest.raises(NotImplementedError, match="hdf5"):
        run(dict(format="hdf5"), ["--condition-audio"])
    with pytest.raises(ValueError, match="hop_size must be int"):
        run(dict(sampling_rate_for_feats=12000, hop_size=50), ["--condition-audio"])
    with pytest.raises(NotImplementedError, match="640"):
        run(dict(sampling_rate=16001), ["--resample-input"])
    with pytest.raises(ValueError, match="trim_threshold_in_db"):
        run(dict(trim_silence=True, trim_threshold_in_db=-60, trim_frame_size=64, trim_hop_size=16), ["--condition-audio"])
    _write_wav(tmp_path / "wavs" / "short.wav", trim_signal(100, 10, 10, 2), 16000)
    with pytest.raises(ValueError, match="too short"):          # 100 samples at 16 kHz are 50 at 8 kHz: <= 64
        run(dict(sampling_rate_for_feats=8000, hop_size=50), ["--condition-audio"])
    assert not os.path.exists(tmp_path / "dump")
