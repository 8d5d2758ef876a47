"""SineGen on the GPU: pwg_sine_samples and pwg_sine_frames (include/pwg_sine.h) against the float64
exact-phase oracle (tests/sinegen_oracle.py) and the reference fixtures (tests/golden/sinegen), no drift
over 2^20 samples, bit identity between the two entry points and across batch positions, the status
flag, the SineGen module, UHiFiGANGenerator's *_from_f0 methods and the decode CLI's flag.

ORACLE_ATOL is derived, not measured: the integer phase is exact; its reduction to the sine's fp32
argument loses at most 2^-26 of a cycle (2 pi 2^-26 x 0.1 = 1e-8); sinpif and the two fp32 roundings of
sin * amp * uv + noise cost a few 1e-8 at |sine| <= 0.1 + noise. 1e-6 is about ten times that.
Measured on an MI355X: 1.4e-8 at the most against the oracle (1.0e-8 over 2^20 + 3
samples), 1.1e-7 against the reference fixtures, 1.7e-6 at the output of the end-to-end UHiFiGAN fixture."""

import numpy as np
import pytest
import torch

import sinegen_oracle as orc
from parallelwavegan_amd import SineGen, _lib
from sinegen_helpers import BLOCK, E2E, FIXTURES, contour, gen_args, load_fixture, run_frames, run_samples

pytestmark = pytest.mark.gpu

ORACLE_ATOL = 1e-6
ATOL = 1e-4  # the project's parity bar, for the comparison with the reference's fp32 sums

# lengths around the scan's block (pwg_sine_samples: BLOCK rows per workgroup) and around the 256-frame
# chunk of pwg_sine_frames' per-utterance scan
LENGTHS = (1, 2, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5)
LEN_ARGS = (22050, 3, 0.1, 0.003, 0.0)  # sr, dim, sine_amp, noise_std, voiced_threshold


def _oracle(ext, args, ini, n):
    sr, dim, amp, nstd, thr = args
    return orc.sinegen(ext, sr, dim - 1, amp, nstd, thr, ini, n)


def _check(label, got, want, atol):
    sine, uv, noise = want
    e_sine, e_noise = np.abs(got["sine"] - sine).max(), np.abs(got["noise"] - noise).max()
    print(f"{label}: max|d| sine {e_sine:.2e} noise {e_noise:.2e}")
    assert got["flag"] == 0
    assert np.array_equal(got["uv"], uv), label
    assert e_sine <= atol and e_noise <= atol, label


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_inputs_against_oracle_and_reference(built_lib, cuda_device, name):
    """Both entry points on a fixture's f0 with its recorded ini and n: within 1e-6 of the oracle and
    within 1e-4 of the reference's outputs; uv exact."""
    fx = load_fixture(name)
    m, args = fx["meta"], gen_args(fx["meta"])
    ext = orc.expand(fx["f0"], m["hop"], m["layout"])
    want = _oracle(ext, args, fx["ini"], fx["n"])
    ref = (fx["sine"], fx["uv"], fx["noise"])
    for label, got in (("samples", run_samples(cuda_device, [ext], args, [fx["ini"]], [fx["n"]])),
                       ("frames", run_frames(cuda_device, [fx["f0"]], m["hop"], m["layout"], args, [fx["ini"]], [fx["n"]]))):
        _check(f"{name} {label} vs oracle", got, want, ORACLE_ATOL)
        _check(f"{name} {label} vs reference", got, ref, ATOL)


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_against_oracle(built_lib, cuda_device, length):
    """Three channels with initial phases: pwg_sine_samples on `length` samples, pwg_sine_frames on
    `length` frames of hop 3 in both layouts."""
    rs = np.random.RandomState(length)
    dim = LEN_ARGS[1]
    f0, ini = contour(length, seed=length), rs.rand(dim).astype(np.float32)
    n = rs.standard_normal((length, dim)).astype(np.float32)
    _check(f"samples N {length}", run_samples(cuda_device, [f0], LEN_ARGS, [ini], [n]), _oracle(f0, LEN_ARGS, ini, n),
           ORACLE_ATOL)
    n3 = rs.standard_normal((length * 3, dim)).astype(np.float32)
    for layout in ("tile", "hold"):
        want = _oracle(orc.expand(f0, 3, layout), LEN_ARGS, ini, n3)
        _check(f"frames {layout} T {length}", run_frames(cuda_device, [f0], 3, layout, LEN_ARGS, [ini], [n3]), want,
               ORACLE_ATOL)


def test_no_drift_over_a_million_samples(built_lib, cuda_device):
    """One utterance of 2^20 + 3 samples of varying f0: the same 1e-6 bar (a float scan cannot meet
    it: the reference's own sums are 4.5e-6 off at 900,000 samples)."""
    N = (1 << 20) + 3
    args = (24000, 1, 0.1, 0.003, 0.0)
    f0 = contour(N, seed=5, lo=80.0, hi=1100.0)
    got = run_samples(cuda_device, [f0], args)
    sine, uv, _ = _oracle(f0, args, None, None)
    err = np.abs(got["sine"] - sine)
    print(f"N {N}: max|d| {err.max():.2e}, over the last 1000 samples {err[-1000:].max():.2e}, voiced {int(uv.sum())}")
    assert got["flag"] == 0 and np.array_equal(got["uv"], uv)
    assert err.max() <= ORACLE_ATOL


@pytest.fixture(scope="module")
def ragged(built_lib, cuda_device):
    """Five frame-rate utterances (hop 7, two channels) with draws, and both entry points' batched
    outputs per layout (computed once)."""
    rs = np.random.RandomState(11)
    hop, args = 7, (24000, 2, 0.1, 0.003, 0.0)
    T = (3, 150, 1, 300, 41)  # 1050 and 2100 rows: utterances that span workgroups of the final passes
    f0s = [contour(t, seed=40 + i) for i, t in enumerate(T)]
    inis = [rs.rand(2).astype(np.float32) for _ in T]
    ns = [rs.standard_normal((t * hop, 2)).astype(np.float32) for t in T]
    out = {}
    for layout in ("tile", "hold"):
        exts = [orc.expand(f, hop, layout) for f in f0s]
        out[layout] = (run_frames(cuda_device, f0s, hop, layout, args, inis, ns), run_samples(cuda_device, exts, args, inis, ns),
                       exts)
    return hop, args, f0s, inis, ns, out


@pytest.mark.parametrize("layout", ["tile", "hold"])
def test_frames_equal_samples_on_the_expanded_f0(ragged, layout):
    fr, sm, _ = ragged[5][layout]
    assert fr["flag"] == 0 and sm["flag"] == 0
    for key in ("sine", "uv", "noise"):
        assert np.array_equal(fr[key].view(np.uint32), sm[key].view(np.uint32)), key
    assert np.isfinite(fr["sine"]).all()


@pytest.mark.parametrize("layout", ["tile", "hold"])
def test_batch_against_oracle(ragged, layout):
    hop, args, f0s, inis, ns, out = ragged
    fr, _, exts = out[layout]
    want = [_oracle(e, args, i, n) for e, i, n in zip(exts, inis, ns)]
    _check(f"ragged {layout}", fr, tuple(np.concatenate([w[k] for w in want]) for k in range(3)), ORACLE_ATOL)


@pytest.mark.parametrize("layout", ["tile", "hold"])
def test_utterance_alone_equals_it_inside_the_batch(cuda_device, ragged, layout):
    hop, args, f0s, inis, ns, out = ragged
    fr, sm, exts = out[layout]
    lo = sum(len(f) for f in f0s[:3]) * hop
    hi = lo + len(f0s[3]) * hop
    solo_f = run_frames(cuda_device, [f0s[3]], hop, layout, args, [inis[3]], [ns[3]])
    solo_s = run_samples(cuda_device, [exts[3]], args, [inis[3]], [ns[3]])
    for key in ("sine", "uv", "noise"):
        assert np.array_equal(solo_f[key], fr[key][lo:hi]), key
        assert np.array_equal(solo_s[key], sm[key][lo:hi]), key


def test_null_noise_equals_zero_noise(cuda_device, ragged):
    hop, args, f0s, inis, ns, out = ragged
    zeros = [np.zeros_like(n) for n in ns]
    for layout in ("tile", "hold"):
        a = run_frames(cuda_device, f0s, hop, layout, args, inis, None)
        b = run_frames(cuda_device, f0s, hop, layout, args, inis, zeros)
        assert np.array_equal(a["sine"].view(np.uint32), b["sine"].view(np.uint32))
        assert not a["noise"].any() and not b["noise"].any()
    exts = out["hold"][2]
    a, b = run_samples(cuda_device, exts, args, inis, None), run_samples(cuda_device, exts, args, inis, zeros)
    assert np.array_equal(a["sine"].view(np.uint32), b["sine"].view(np.uint32))
    # the optional outputs may be left out
    c = run_samples(cuda_device, exts, args, inis, None, with_uv_noise=False)
    assert np.array_equal(a["sine"], c["sine"])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_f0_sets_the_flag(built_lib, cuda_device, bad):
    """A non-finite f0 in the middle utterance: PWG_SINE_BAD_F0, its samples are the unvoiced value
    (sine_amp / 3 * n) with a zero increment, and the neighbouring utterances are unchanged."""
    rs = np.random.RandomState(3)
    hop, args = 4, (24000, 2, 0.1, 0.003, 0.0)
    f0s = [contour(t, seed=60 + i) for i, t in enumerate((9, 12, 6))]
    ns = [rs.standard_normal((len(f) * hop, 2)).astype(np.float32) for f in f0s]
    clean = run_frames(cuda_device, f0s, hop, "hold", args, None, ns)
    assert clean["flag"] == 0
    f0s[1] = f0s[1].copy()
    f0s[1][5] = bad
    exts = [orc.expand(f, hop, "hold") for f in f0s]
    want = [_oracle(e, args, None, n) for e, n in zip(exts, ns)]
    lo, hi = 9 * hop, (9 + 12) * hop
    for got in (run_frames(cuda_device, f0s, hop, "hold", args, None, ns), run_samples(cuda_device, exts, args, None, ns)):
        assert got["flag"] == _lib.PWG_SINE_BAD_F0
        assert np.isfinite(got["sine"]).all()
        rows = slice(lo + 5 * hop, lo + 6 * hop)
        assert not got["uv"][rows].any()
        third = np.float32(0.1) / np.float32(3)
        assert np.array_equal(got["sine"][rows], third * ns[1][5 * hop:6 * hop])
        assert np.array_equal(got["noise"][rows], got["sine"][rows])
        for key in ("sine", "uv", "noise"):
            assert np.array_equal(got[key][:lo], clean[key][:lo]) and np.array_equal(got[key][hi:], clean[key][hi:]), key
        assert np.abs(got["sine"] - np.concatenate([w[0] for w in want])).max() <= ORACLE_ATOL
    with pytest.raises(ValueError, match="PWG_SINE_BAD_F0"):
        SineGen(24000)(torch.from_numpy(exts[1]).to(cuda_device).reshape(1, -1, 1))


def test_utterance_boundaries_are_clamped(built_lib, cuda_device):
    """Boundaries outside the row range are clamped: utterance 0 owns the rows from 0, the last one the
    rows to the end (include/pwg_sine.h), so these calls equal the ones with the true boundaries."""
    rs = np.random.RandomState(2)
    hop, args = 5, (24000, 2, 0.1, 0.003, 0.0)
    f0s = [contour(3, seed=1), contour(4, seed=2)]
    inis = [rs.rand(2).astype(np.float32) for _ in f0s]
    exts = [orc.expand(f, hop, "tile") for f in f0s]
    a = run_frames(cuda_device, f0s, hop, "tile", args, inis)
    b = run_frames(cuda_device, f0s, hop, "tile", args, inis, starts=[-5, 3, 1 << 40])
    c = run_samples(cuda_device, exts, args, inis, starts=[-(1 << 50), 15, 36])
    assert a["flag"] == 0 and b["flag"] == 0 and c["flag"] == 0
    for key in ("sine", "uv", "noise"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key


def test_negative_f0_follows_the_reference(built_lib, cuda_device):
    args = (24000, 2, 0.1, 0.003, 0.0)
    f0 = np.array([220.0, -100.0, -1e-12, 330.0, -36000.0, 440.0] * 3, np.float32)
    got = run_samples(cuda_device, [f0], args)
    _check("negative f0", got, _oracle(f0, args, None, None), ORACLE_ATOL)
    assert got["uv"].tolist() == [1, 0, 0, 1, 0, 1] * 3


def test_both_entry_points_replay_from_a_captured_graph(cuda_device, ragged):
    """Launches only, no host synchronisation: both calls are captured on a side stream (the scratch and
    the flag's zeroing become part of the graph) and the replay writes the eager call's bits."""
    from parallelwavegan_amd import sinegen

    hop, args, f0s, inis, ns, out = ragged
    sr, dim, amp, nstd, thr = args
    dev = cuda_device
    T = [len(f) for f in f0s]
    fstart = torch.from_numpy(np.concatenate([[0], np.cumsum(T)]).astype(np.int64)).to(dev)
    rstart = fstart * hop
    rows = sum(T) * hop
    f_fr = torch.from_numpy(np.concatenate(f0s)).to(dev)
    f_sm = torch.from_numpy(np.concatenate(out["hold"][2])).to(dev)
    ini = torch.from_numpy(np.concatenate(inis)).to(dev)
    n = torch.from_numpy(np.concatenate(ns)).to(dev)
    o_fr, o_sm = torch.zeros(rows, dim, device=dev), torch.zeros(rows, dim, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            flag_fr = sinegen.sine_call("pwg_sine_frames", dev, f_fr, fstart, len(T), sum(T),
                                        (hop, _lib.PWG_SINE_LAYOUTS["hold"]), float(sr), dim, amp, nstd, thr, ini, n, o_fr,
                                        None, None)
            flag_sm = sinegen.sine_call("pwg_sine_samples", dev, f_sm, rstart, len(T), rows, (), float(sr), dim, amp, nstd,
                                        thr, ini, n, o_sm, None, None)
        g.replay()
        torch.cuda.synchronize()
    assert int(flag_fr.item()) == 0 and int(flag_sm.item()) == 0
    want = out["hold"][0]["sine"]
    assert np.array_equal(o_fr.cpu().numpy(), want) and np.array_equal(o_sm.cpu().numpy(), want)


# ------------------------------------------------------------------ the module
def test_module_matches_fixture_with_pinned_draws(built_lib, cuda_device):
    fx = load_fixture("sg_hold_h5_T33_harm7")
    m = fx["meta"]
    gen = SineGen(m["samp_rate"], harmonic_num=m["harmonic_num"], voiced_threshold=m["voiced_threshold"])
    ext = orc.expand(fx["f0"], m["hop"], m["layout"])
    f0 = torch.from_numpy(np.stack([ext, ext[::-1].copy()])).to(cuda_device)[:, :, None]
    ini = np.stack([fx["ini"], fx["ini"]])
    n = np.stack([fx["n"], fx["n"][::-1]])
    sine, uv, noise = gen(f0, rand_ini=ini, noise=n)
    assert sine.shape == (2, 165, 8) and uv.shape == (2, 165, 1) and noise.shape == (2, 165, 8)
    assert sine.device == cuda_device and sine.dtype == torch.float32
    err = np.abs(sine[0].cpu().numpy() - fx["sine"]).max()
    print(f"module vs reference: {err:.2e}")
    assert err < ATOL and np.array_equal(uv[0, :, 0].cpu().numpy(), fx["uv"])
    assert np.array_equal(noise[0].cpu().numpy(), fx["noise"])  # noise_amp * n: one fp32 product, as the reference
    want = _oracle(ext[::-1], gen_args(m), fx["ini"], fx["n"][::-1])
    assert np.abs(sine[1].cpu().numpy() - want[0]).max() <= ORACLE_ATOL


def test_module_draws_on_the_device(built_lib, cuda_device):
    gen = SineGen(24000, harmonic_num=1)
    f0 = torch.zeros(2, 4096, 1, device=cuda_device)
    f0[0] = 200.0
    torch.manual_seed(0)
    sine, uv, noise = gen(f0)
    torch.manual_seed(0)
    again, _, _ = gen(f0)
    assert torch.equal(sine, again)
    assert torch.equal(uv[:, 0, 0].cpu(), torch.tensor([1.0, 0.0]))
    std_v, std_u = float(noise[0].std()), float(noise[1].std())
    assert abs(std_v / 0.003 - 1) < 0.1 and abs(std_u / (0.1 / 3) - 1) < 0.1
    assert torch.equal(sine[1], noise[1])
    # the fundamental starts at phase 0, the overtone at a drawn one
    clean = (sine[0] - noise[0]).cpu().numpy()
    assert abs(clean[0, 0] - 0.1 * np.sin(2 * np.pi * 200 / 24000)) < 1e-6


# ------------------------------------------------------------------ UHiFiGAN
@pytest.fixture(scope="module")
def uhg(built_lib, cuda_device):
    from uhifigan_helpers import fixture_module

    fx = load_fixture(E2E)
    m, _, _ = fixture_module(fx["meta"])
    return m.to(cuda_device), fx


def test_uhifigan_from_f0_matches_the_end_to_end_fixture(uhg):
    m, fx = uhg
    sr = fx["meta"]["samp_rate"]
    exc = m.excitation_from_f0([fx["f0"]], sr, "tile", noise=[fx["n"]])
    assert len(exc) == 1 and exc[0].shape == (180,) and exc[0].is_cuda
    e_exc = np.abs(exc[0].cpu().numpy() - fx["excitation"]).max()
    y = m.inference_from_f0(fx["f0"], fx["c"], sr, "tile", noise=fx["n"])
    assert torch.equal(y, m.inference(excitation=exc[0], c=fx["c"]))
    e_y = np.abs(y.cpu().numpy() - fx["y"]).max()
    print(f"excitation vs reference {e_exc:.2e}, y vs reference {e_y:.2e} (e_ref {fx['meta']['e_ref']:.1e})")
    assert y.shape == fx["y"].shape and e_exc < ATOL and e_y < ATOL
    hold = m.inference_from_f0(fx["f0"], fx["c"], sr, "hold", noise=fx["n"])
    assert hold.shape == y.shape and not torch.equal(hold, y)


def test_uhifigan_ragged_batch_from_f0_equals_single_calls(uhg):
    from parallelwavegan_amd import synthetic

    m, fx = uhg
    hop, T = m.upsample_factor, (9, 1, 30)
    rs = np.random.RandomState(8)
    cs = [synthetic.make_mel(t, m.in_channels, seed=70 + i) for i, t in enumerate(T)]
    f0s = [contour(t, seed=80 + i) for i, t in enumerate(T)]
    ns = [rs.standard_normal(t * hop).astype(np.float32) for t in T]
    outs = [o.clone() for o in m.inference_batch_from_f0(cs, f0s, 24000, "tile", noises=ns)]
    for c, f, n, o in zip(cs, f0s, ns, outs):
        assert o.shape == (c.shape[0] * hop, 1)
        assert torch.equal(m.inference_from_f0(f, c, 24000, "tile", noise=n), o)
    with pytest.raises(ValueError, match="f0 has 8 frames, c has 9"):
        m.inference_from_f0(f0s[0][:-1], cs[0], 24000)
    with pytest.raises(ValueError, match="noise has"):
        m.inference_from_f0(f0s[0], cs[0], 24000, noise=ns[0][:-1])
    # without pinned noise the draws come from the device generator
    torch.manual_seed(3)
    a = m.inference_from_f0(f0s[0], cs[0], 24000).clone()
    torch.manual_seed(3)
    assert torch.equal(a, m.inference_from_f0(f0s[0], cs[0], 24000))


def test_decode_cli_excitation_from_f0(tmp_path, built_lib, cuda_device):
    import yaml

    from parallelwavegan_amd import UHiFiGANGenerator, configs, synthetic
    from parallelwavegan_amd.bin import decode
    from parallelwavegan_amd.utils import load_model, read_pcm16_wav

    cfg = "uhifigan_noadd_nobias_test"
    params = configs.uhifigan_params(cfg)
    holder = UHiFiGANGenerator(**configs.uhifigan_params(cfg))
    state = {k: torch.from_numpy(v) for k, v in synthetic.make_module_state_dict(holder, seed=4).items()}
    ckpt = str(tmp_path / "checkpoint-10steps.pkl")
    torch.save({"model": {"generator": state}, "steps": 10}, ckpt)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(dict(generator_type="UHiFiGANGenerator", generator_params=params, sampling_rate=24000,
                            sampling_rate_for_feats=16000, format="npy"), f)
    dump = tmp_path / "dump"
    dump.mkdir()
    lengths = {"utt_a": 9, "utt_b": 14}
    for i, (u, t) in enumerate(lengths.items()):
        np.save(dump / f"{u}-feats.npy", synthetic.make_mel(t, 16, seed=50 + i))
        np.save(dump / f"{u}-f0.npy", contour(t + (2 if i else -3), seed=90 + i).reshape(-1, 1))  # trimmed / padded
    common = ["--dumpdir", str(dump), "--checkpoint", ckpt, "--verbose", "0", "--batch-frames", "64"]
    with pytest.raises(FileNotFoundError, match="excitation.npy"):
        decode.main(common + ["--outdir", str(tmp_path / "none")])
    out = tmp_path / "wav"
    assert decode.main(common + ["--outdir", str(out), "--excitation-from-f0", "tile", "--excitation-seed", "7"]) == 0
    m = load_model(ckpt)
    m.remove_weight_norm()
    m = m.eval().to(cuda_device)
    cs = [np.load(dump / f"{u}-feats.npy") for u in lengths]
    f0s = [decode.fit_f0(np.load(dump / f"{u}-f0.npy"), t) for u, t in lengths.items()]
    torch.manual_seed(7)
    ys = m.inference_batch_from_f0(cs, f0s, 16000, "tile")
    for (u, t), y in zip(lengths.items(), ys):
        z, sr = read_pcm16_wav(str(out / f"{u}_gen.wav"))
        assert sr == 24000 and z.shape == (t * 20,)
        # PCM16-exact: the integers write_pcm16_wav makes of the drop-in's output
        want = np.clip(np.round(y.view(-1).cpu().numpy().astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
        assert np.array_equal(np.round(z.astype(np.float64) * 32767.0).astype(np.int16), want)
        assert want.any()
