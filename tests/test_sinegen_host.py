"""SineGen without a GPU: the float64 exact-phase oracle (tests/sinegen_oracle.py) against the reference
fixtures (tests/golden/sinegen, made by make_golden_sinegen.py), its fp32 increments against torch bit
for bit, the closed forms of pwg_sine_frames against a sequential accumulation, the C-ABI's argument
checks, and the argument handling of SineGen, the UHiFiGAN methods and the decode CLI's flag."""

import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

import sinegen_oracle as orc
from parallelwavegan_amd import SineGen, UHiFiGANGenerator, _lib, configs
from sinegen_helpers import E2E, FIXTURES, gen_args, load_fixture

ATOL = 1e-4  # the project's parity bar


def test_fixture_set_is_complete():
    assert FIXTURES == ["sg_hold_h5_T33_harm7", "sg_hold_h8_T19", "sg_tile_h1_T19", "sg_tile_h300_T7", "sg_tile_h8_T1",
                        "sg_tile_h8_T19", "sg_tile_h8_T5_unvoiced"]
    assert load_fixture(E2E)["y"].shape == (180, 1)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_fixture(name):
    """Measured here: at most 1.2e-7 (sg_tile_h300_T7); the reference's own fp32 sums are the difference."""
    fx = load_fixture(name)
    m = fx["meta"]
    sr, dim, amp, nstd, thr = gen_args(m)
    ext = orc.expand(fx["f0"], m["hop"], m["layout"])
    sine, uv, noise = orc.sinegen(ext, sr, dim - 1, amp, nstd, thr, fx["ini"], fx["n"])
    e_sine, e_noise = np.abs(sine - fx["sine"]).max(), np.abs(noise - fx["noise"]).max()
    print(f"{name}: max|oracle - reference| sine {e_sine:.2e} noise {e_noise:.2e}")
    assert np.array_equal(uv, fx["uv"])
    assert e_sine < ATOL and e_noise < ATOL


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_rad_is_torchs_fp32(name):
    fx = load_fixture(name)
    m = fx["meta"]
    sr, dim = m["samp_rate"], m["harmonic_num"] + 1
    ext = torch.from_numpy(orc.expand(fx["f0"], m["hop"], m["layout"]))
    buf = torch.zeros(ext.numel(), dim)
    buf[:, 0] = ext
    for idx in np.arange(dim - 1):  # layers/sine.py:126-129
        buf[:, idx + 1] = buf[:, 0] * (idx + 2)
    want = ((buf / sr) % 1).numpy()
    got = orc.rad_fp32(ext.numpy(), dim, sr)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_oracle_rad_of_negative_and_tiny_f0():
    f = np.array([-100.0, -1e-12, 0.0, 24000.0, 36000.0, -36000.0], np.float32)
    want = ((torch.from_numpy(f)[:, None] / 24000) % 1).numpy()
    got = orc.rad_fp32(f, 1, 24000)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[1, 0] == 1.0  # the remainder of a tiny negative value rounds up to 1: q wraps to 0
    assert orc.q_of_rad(got)[1, 0] == 0
    _, uv, _ = orc.sinegen(f, 24000)
    assert uv.tolist() == [0, 0, 0, 1, 1, 0]


def test_q_is_the_64_bit_fraction():
    rad = np.array([0.0, 0.5, 0.75, 1.0, 1.5, 2.0, 2.0 ** -24, 1 - 2.0 ** -24], np.float32)
    want = [0, 1 << 63, 3 << 62, 0, 1 << 63, 0, 1 << 40, (1 << 64) - (1 << 40)]
    assert [int(v) for v in orc.q_of_rad(rad)] == want
    assert int(orc.q_of_rad(np.array([np.nan], np.float32))[0]) == 0


@pytest.mark.parametrize("layout", ["tile", "hold"])
@pytest.mark.parametrize("hop, T, dim", [(8, 19, 1), (5, 33, 8), (1, 7, 2), (300, 3, 2), (4, 1, 3)])
def test_closed_forms_equal_sequential_accumulation(layout, hop, T, dim):
    rs = np.random.RandomState(hop + T)
    f0 = (rs.rand(T) * 800).astype(np.float32)
    f0[rs.rand(T) < 0.2] = 0
    ini = rs.rand(dim).astype(np.float32)
    q, _ = orc.increments(orc.expand(f0, hop, layout), dim, 22050, ini)
    want = orc.phase_sequential(q)
    got = orc.phase_closed_form(f0, hop, layout, dim, 22050, ini)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(np.cumsum(q, axis=0, dtype=np.uint64), want)  # and uint64 cumsum wraps natively


def test_tile_is_the_references_expansion():
    f0 = np.arange(1, 8, dtype=np.float32)
    ref = torch.from_numpy(f0).reshape(1, 1, -1).repeat(1, 5, 1).reshape(-1).numpy()  # bin/preprocess.py:431-436
    assert np.array_equal(orc.expand(f0, 5, "tile"), ref)
    assert np.array_equal(orc.expand(f0, 5, "hold"), np.repeat(f0, 5))


# ------------------------------------------------------------------ C-ABI argument checks (no launch)
P = ctypes.c_void_p(4096)  # a non-null, aligned pointer no check dereferences


def _samples(L, f0=P, start=P, n_utts=1, rows=8, sr=24000.0, dim=1, sine=P, scratch=P, nbytes=1 << 20, flag=P):
    return L.pwg_sine_samples(f0, start, n_utts, rows, sr, dim, 0.1, 0.003, 0.0, None, None, sine, None, None, scratch,
                              nbytes, flag, None)


def _frames(L, f0=P, start=P, n_utts=1, frames=8, hop=4, layout=0, sr=24000.0, dim=1, sine=P, scratch=P,
            nbytes=1 << 20, flag=P):
    return L.pwg_sine_frames(f0, start, n_utts, frames, hop, layout, sr, dim, 0.1, 0.003, 0.0, None, None, sine, None,
                             None, scratch, nbytes, flag, None)


def test_scratch_bytes(built_lib):
    L = built_lib
    B = _lib.PWG_SINE_SCAN_BLOCK
    assert L.pwg_sine_scratch_bytes(0, 1) == 64 * 2
    assert L.pwg_sine_scratch_bytes(B, 1) == 64 * 3 and L.pwg_sine_scratch_bytes(B + 1, 3) == 64 * 8
    assert L.pwg_sine_frames_scratch_bytes(10, 2) == 64 * 14
    assert L.pwg_sine_scratch_bytes(-1, 1) == -1 and L.pwg_sine_frames_scratch_bytes(1, -1) == -1


@pytest.mark.parametrize("call", [_samples, _frames], ids=["samples", "frames"])
def test_capi_argument_checks(built_lib, call):
    L = built_lib
    for null in ("f0", "start", "sine", "scratch", "flag"):
        assert call(L, **{null: None}) == _lib.PWG_ERR_INVALID, null
    assert call(L, n_utts=0) == _lib.PWG_ERR_INVALID
    assert call(L, **{"rows" if call is _samples else "frames": -1}) == _lib.PWG_ERR_INVALID
    assert call(L, scratch=ctypes.c_void_p(4100)) == _lib.PWG_ERR_INVALID
    assert call(L, nbytes=64) == _lib.PWG_ERR_INVALID
    assert b"scratch" in L.pwg_last_error()
    for dim in (0, -1, 9):
        assert call(L, dim=dim) == _lib.PWG_ERR_UNSUPPORTED, dim
    for sr in (0.0, -16000.0, float("inf"), float("nan")):
        assert call(L, sr=sr) == _lib.PWG_ERR_UNSUPPORTED, sr
    # an empty batch is fine and launches nothing (the pointers are never dereferenced)
    assert call(L, **{"rows" if call is _samples else "frames": 0}) == _lib.PWG_OK
    with pytest.raises(NotImplementedError, match="dim"):
        _lib.check(call(L, dim=9))


def test_capi_frames_only_checks(built_lib):
    L = built_lib
    assert _frames(L, hop=0) == _lib.PWG_ERR_UNSUPPORTED and _frames(L, hop=-3) == _lib.PWG_ERR_UNSUPPORTED
    assert _frames(L, layout=2) == _lib.PWG_ERR_UNSUPPORTED and _frames(L, layout=-1) == _lib.PWG_ERR_UNSUPPORTED
    assert _frames(L, frames=1 << 40, hop=1 << 30, nbytes=1 << 62) == _lib.PWG_ERR_INVALID  # frames * hop overflows
    assert _lib.PWG_SINE_LAYOUTS == {"tile": 0, "hold": 1}


# ------------------------------------------------------------------ Python argument handling
def test_sinegen_constructor_and_refusals():
    g = SineGen(24000, harmonic_num=3, sine_amp=0.2, noise_std=0.01, voiced_threshold=10)
    assert (g.sampling_rate, g.harmonic_num, g.dim, g.sine_amp, g.noise_std, g.voiced_threshold, g.flag_for_pulse) == \
        (24000, 3, 4, 0.2, 0.01, 10, False)
    d = SineGen(16000)
    assert (d.harmonic_num, d.dim, d.sine_amp, d.noise_std, d.voiced_threshold) == (0, 1, 0.1, 0.003, 0)
    assert not list(d.parameters()) and not d.state_dict()
    with pytest.raises(NotImplementedError, match="flag_for_pulse"):
        SineGen(24000, flag_for_pulse=True)
    with pytest.raises(NotImplementedError, match="harmonic_num"):
        SineGen(24000, harmonic_num=8)
    with pytest.raises(NotImplementedError, match="samp_rate"):
        SineGen(0)
    with pytest.raises(ValueError, match=r"\(B, T, 1\)"):
        d(torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        d(torch.zeros(2, 5, 1))
    with pytest.raises(TypeError):
        d(torch.zeros(2, 5, 1), torch.zeros(2, 1))  # rand_ini and noise are keyword-only


def test_uhifigan_from_f0_argument_handling():
    m = UHiFiGANGenerator(**configs.uhifigan_params("uhifigan_noadd_nobias_test"))
    c, f0 = np.zeros((3, 16), np.float32), np.zeros(3, np.float32)
    for call in (lambda **k: m.excitation_from_f0([f0], **k), lambda **k: m.inference_from_f0(f0, c, **k),
                 lambda **k: m.inference_batch_from_f0([c], [f0], **k)):
        with pytest.raises(ValueError, match="layout"):
            call(sampling_rate=24000, layout="repeat")
        with pytest.raises(ValueError, match="sampling_rate"):
            call(sampling_rate=0)
        with pytest.raises(RuntimeError, match="ROCm GPU only"):
            call(sampling_rate=24000)
    # the methods that take an excitation keep their behaviour
    with pytest.raises(ValueError, match="needs excitation"):
        m.inference(f0=f0, c=c)
    with pytest.raises(ValueError, match="needs c and excitation"):
        m(torch.zeros(1, 16, 3), torch.zeros(1, 3))


def _config(tmp, generator_type, params, **extra):
    ckpt = os.path.join(tmp, "checkpoint-1steps.pkl")
    with open(os.path.join(tmp, "config.yml"), "w") as f:
        yaml.safe_dump(dict(generator_type=generator_type, generator_params=params, sampling_rate=24000, format="npy",
                            **extra), f)
    return ckpt


def test_decode_cli_flag_handling(tmp_path):
    from parallelwavegan_amd.bin import decode

    dump = tmp_path / "dump"
    dump.mkdir()
    for u, t in (("utt_a", 4), ("utt_b", 6)):
        np.save(dump / f"{u}-feats.npy", np.zeros((t, 16), np.float32))
    np.save(dump / "utt_a-f0.npy", np.zeros(4, np.float32))
    common = ["--dumpdir", str(dump), "--outdir", str(tmp_path / "wav"), "--verbose", "0"]
    ckpt = _config(str(tmp_path), "UHiFiGANGenerator", configs.uhifigan_params("uhifigan_noadd_nobias_test"))
    with pytest.raises(FileNotFoundError, match="utt_b-f0.npy"):
        decode.main(common + ["--checkpoint", ckpt, "--excitation-from-f0", "tile"])
    with pytest.raises(FileNotFoundError, match="utt_a-excitation.npy"):  # without the flag nothing changes
        decode.main(common + ["--checkpoint", ckpt])
    with pytest.raises(SystemExit):
        decode.main(common + ["--checkpoint", ckpt, "--excitation-from-f0", "repeat"])
    other = tmp_path / "other"
    other.mkdir()
    ckpt = _config(str(other), "HiFiGANGenerator", configs.vocoder_params("hifigan_test")[1])
    with pytest.raises(NotImplementedError, match="--excitation-from-f0 applies to a UHiFiGANGenerator"):
        decode.main(common + ["--checkpoint", ckpt, "--excitation-from-f0", "hold"])


def test_decode_cli_fits_f0_to_the_mel_length():
    from parallelwavegan_amd.bin.decode import fit_f0

    f = np.array([[1.0], [2.0], [3.0]])  # (T, 1) as the reference dumps it before squeezing
    assert fit_f0(f, 3).tolist() == [1, 2, 3] and fit_f0(f, 2).tolist() == [1, 2]
    got = fit_f0(f, 5)
    assert got.dtype == np.float32 and got.tolist() == [1, 2, 3, 3, 3]
    with pytest.raises(ValueError):
        fit_f0(np.zeros(0), 2)
