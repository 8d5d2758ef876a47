"""YIN f0 extraction on the GPU (include/pwg_yin.h) against the float64 oracle (tests/yin_oracle.py).

The discrete comparison: on every frame the oracle decided with margin (tests/yin_helpers.py:compared; all
frames of every case, as tests/test_yin_host.py asserts), k* is equal and f0 is bit-equal to the fp32
fs / (k* + tau_min + 1), in log mode within 1 ulp of np.log on float32. The continuous comparison: the cmdf
output within max(R_MAX, eps) of the oracle's c (relative), R_MAX = 1.4e-4 being the error of the fp32 FFT
route on the same inputs (tests/test_yin_host.py) and eps = 2 (W + tau_max) 2^-24 the derived bound of the
direct form. Every test prints its measured figure.

Measured on an MI355X: k* equal and f0 bit-equal on every frame of every case (none is
below the margin); c within 1.2e-6 of the oracle at tau_max 32 (bar 1.4e-4) and 2.3e-6 at tau_max 600 (bar
2.1e-4); log f0 at most 1 ulp from np.log; batches, orders, optional outputs and graph replay bit-identical."""

import ctypes

import numpy as np
import pytest
import torch

import yin_oracle as orc
from yin_helpers import CASES, GEOMETRIES, R_MAX, SHORT, TILE, case_signal, compared, eps_of, oracle, rel_err, run_raw, signal
from parallelwavegan_amd import LogMelExtractor, YinF0Extractor, _lib, f0_torchyin, yin_estimate
from parallelwavegan_amd.yin import YinPlan

pytestmark = pytest.mark.gpu


def bar(geometry):
    return max(R_MAX, eps_of(geometry))


def check(got, want, geometry, keep=None, log=False, label=""):
    """One utterance's kernel outputs against the oracle's (both fitted to the same rows)."""
    fs, _, tau_min, _, _ = GEOMETRIES[geometry]
    keep = want["margin"] > eps_of(geometry) if keep is None else keep
    assert got["f0"].shape == want["f0"].shape and got["f0"].dtype == np.float32
    if got["k"] is not None:
        assert got["k"].dtype == np.int32 and np.array_equal(got["k"][keep], want["k"][keep])
    f0 = want["f0"]
    if log:
        lo = orc.log_f0(f0)
        ulp = np.abs(got["f0"][keep].view(np.int32).astype(np.int64) - lo[keep].view(np.int32).astype(np.int64))
        assert ulp.max() <= 1 and (got["f0"][keep][f0[keep] == 0] == 0).all()
    else:
        assert np.array_equal(got["f0"][keep].view(np.int32), f0[keep].view(np.int32))
    err = None
    if got["c"] is not None:
        err = rel_err(got["c"], want["c"])
        assert err <= bar(geometry), (label, err)
    print(f"{label}: {len(keep)} rows, {int(keep.sum())} compared, voiced {int((want['k'][keep] > 0).sum())}, "
          f"c vs oracle {'-' if err is None else '%.2e' % err} (bar {bar(geometry):.1e})")
    return err


@pytest.mark.parametrize("case", CASES[:7], ids=lambda c: "%s-%d" % (c[0], c[1]))
def test_kernel_matches_the_oracle(case, built_lib, cuda_device):
    """S at F - 1, F, F + 1 and 2 F + 3 frames of the kernel's frame tile F, S and S4 at 201 frames, R at 41."""
    out, = run_raw(cuda_device, [case_signal(case)], case[0])
    assert len(out["f0"]) == case[1]
    check(out, oracle(case), case[0], compared(case), label=str(case))
    keep = compared(case)
    assert (oracle(case)["k"][keep] > 0).any() and (oracle(case)["k"][keep] == 0).any()


def test_tile_cases_cover_the_frame_tile():
    assert [c[1] for c in CASES[:4]] == [TILE - 1, TILE, TILE + 1, 2 * TILE + 3]


@pytest.mark.parametrize("T", [SHORT[1], 64, 1], ids=["T<W", "T==W", "T==1"])
def test_short_utterances_give_one_frame(T, built_lib, cuda_device):
    """T < W: one frame, zero-padded at its end; T == W: exactly one frame."""
    g, _, seed = SHORT
    fs, hop, tau_min, tau_max, sweep = GEOMETRIES[g]
    x = signal(max(T, 8), fs, sweep, seed)[:T] if T < 64 else case_signal(("S", 201, 0, 20))[1000:1000 + T]
    want = orc.analyse(x, fs, tau_min, tau_max, hop)
    assert len(want["k"]) == 1 and want["margin"][0] > eps_of(g)
    out, = run_raw(cuda_device, [x], g)
    check(out, want, g, label=f"T = {T}")


def test_ragged_batch_is_bit_identical_to_single_runs_in_any_order(built_lib, cuda_device):
    cases = [CASES[7], CASES[8], CASES[9], CASES[2]]
    xs = [case_signal(c) for c in cases] + [signal(SHORT[1], 8000, (300.0, 900.0), SHORT[2])]
    batch = run_raw(cuda_device, xs, "S")
    for c, o in zip(cases, batch):
        check(o, oracle(c), "S", compared(c), label="batch " + str(c))
    order = [3, 0, 4, 2, 1]
    shuffled = run_raw(cuda_device, [xs[i] for i in order], "S")
    for pos, i in enumerate(order):
        alone, = run_raw(cuda_device, [xs[i]], "S")
        for name in ("f0", "k", "c"):
            a, b, s = alone[name], batch[i][name], shuffled[pos][name]
            assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), s.view(np.int32))


def test_more_than_one_launch_chunk(built_lib, cuda_device):
    """70 utterances: two launches of up to 64; every utterance as alone."""
    x = case_signal(CASES[8])
    xs = [x[: len(x) - 3 * (i % 5)] for i in range(70)]
    batch = run_raw(cuda_device, xs, "S")
    alone = {n: run_raw(cuda_device, [x[:n]], "S")[0] for n in {len(v) for v in xs}}
    for v, o in zip(xs, batch):
        for name in ("f0", "k", "c"):
            assert np.array_equal(o[name].view(np.int32), alone[len(v)][name].view(np.int32))


@pytest.mark.parametrize("log", [False, True], ids=["hz", "log"])
def test_out_frames_hold_and_cut(log, built_lib, cuda_device):
    """Rows beyond an utterance's frames hold the last frame's values; fewer rows cut the contour."""
    cases = [CASES[3], CASES[7], CASES[8]]          # 19, 40 and 5 frames
    rows = [19 + 2 * TILE + 1, 33, 5]               # held across tiles, cut inside a tile, as it is
    xs = [case_signal(c) for c in cases]
    outs = run_raw(cuda_device, xs, "S", out_frames=rows, log=log)
    own = run_raw(cuda_device, xs, "S", log=log)
    for c, n, o, w in zip(cases, rows, outs, own):
        fs, hop, tau_min, tau_max, _ = GEOMETRIES[c[0]]
        want = orc.analyse(case_signal(c), fs, tau_min, tau_max, hop, out_frames=n)
        check(o, want, "S", log=log, label=f"{c} -> {n} rows")
        m = min(n, c[1])
        for name in ("f0", "k", "c"):
            assert np.array_equal(o[name][:m].view(np.int32), w[name][:m].view(np.int32))
            assert (o[name][m:] == w[name][c[1] - 1]).all()


def test_optional_outputs_do_not_change_f0(built_lib, cuda_device):
    case = CASES[3]
    x = case_signal(case)
    full, = run_raw(cuda_device, [x], "S")
    for want_tau, want_cmdf in ((False, False), (True, False), (False, True)):
        part, = run_raw(cuda_device, [x], "S", want_tau=want_tau, want_cmdf=want_cmdf)
        assert (part["k"] is None) == (not want_tau) and (part["c"] is None) == (not want_cmdf)
        assert np.array_equal(part["f0"].view(np.int32), full["f0"].view(np.int32))
        check(part, oracle(case), "S", compared(case), label=f"tau {want_tau} cmdf {want_cmdf}")


def test_log_mode_is_within_one_ulp_of_numpy(built_lib, cuda_device):
    for case in (CASES[4], CASES[6]):
        hz, = run_raw(cuda_device, [case_signal(case)], case[0], want_cmdf=False)
        lg, = run_raw(cuda_device, [case_signal(case)], case[0], log=True, want_cmdf=False)
        assert np.array_equal(hz["k"], lg["k"]) and np.array_equal(lg["f0"] == 0, hz["f0"] == 0)
        check(lg, oracle(case), case[0], compared(case), log=True, label=f"log {case}")


def test_threshold_is_an_argument(built_lib, cuda_device):
    case = CASES[4]
    fs, hop, tau_min, tau_max, _ = GEOMETRIES["S"]
    want = orc.analyse(case_signal(case), fs, tau_min, tau_max, hop, 0.3)
    assert not np.array_equal(want["k"], oracle(case)["k"])
    out, = run_raw(cuda_device, [case_signal(case)], "S", threshold=0.3)
    keep = want["margin"] > eps_of("S")
    assert keep.mean() >= 0.98
    check(out, want, "S", keep, label="threshold 0.3")


def test_wrong_device_argument_and_null_outputs(built_lib, cuda_device):
    L = built_lib
    plan = YinPlan(cuda_device, 8000, 0, 32, 16)
    x = torch.zeros(100, device=cuda_device)
    starts = (ctypes.c_longlong * 2)(0, 100)
    f0 = torch.full((3,), -1.0, device=cuda_device)
    assert L.pwg_yin_run(plan._h, x.data_ptr(), starts, 1, None, f0.data_ptr(), None, None, 2, None) == _lib.PWG_ERR_INVALID
    assert b"out_rows" in L.pwg_last_error()
    assert L.pwg_yin_run(plan._h, x.data_ptr(), starts, 1, None, f0.data_ptr(), None, None, 3, None) == _lib.PWG_OK
    torch.cuda.synchronize(cuda_device)
    assert (f0 == 0).all()  # silence: unvoiced
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert L.pwg_yin_run(plan._h, x.data_ptr(), starts, 1, None, f0.data_ptr(), None, None, 3, None) == _lib.PWG_ERR_INVALID
            assert b"device" in L.pwg_last_error()


def test_graph_capture_replays_the_same_bits(built_lib, cuda_device):
    L = built_lib
    case = CASES[3]
    fs, hop, tau_min, tau_max, _ = GEOMETRIES["S"]
    x = case_signal(case)
    plan = YinPlan(cuda_device, fs, tau_min, tau_max, hop)
    wave = torch.from_numpy(x).to(cuda_device)
    rows = case[1] + 4
    direct = plan.run(wave, [len(x)], [rows], True, True)
    torch.cuda.synchronize(cuda_device)
    outs = [torch.zeros_like(t) for t in direct]
    starts, frames = (ctypes.c_longlong * 2)(0, len(x)), (ctypes.c_longlong * 1)(rows)
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _lib.check(L.pwg_yin_run(plan._h, wave.data_ptr(), starts, 1, frames, outs[0].data_ptr(), outs[1].data_ptr(),
                                 outs[2].data_ptr(), rows, torch.cuda.current_stream(cuda_device).cuda_stream))
    torch.cuda.synchronize(cuda_device)
    assert all((o == 0).all() for o in outs)  # capture launches nothing
    graph.replay()
    torch.cuda.synchronize(cuda_device)
    for o, d in zip(outs, direct):
        assert torch.equal(o.view(-1).view(torch.int32), d.view(-1).view(torch.int32))
    assert (direct[1] > 0).any()


def test_yin_estimate_on_a_batch(built_lib, cuda_device):
    """(B, T) and (T,): Hz, 0 where unvoiced; the hop is int(frame_stride * sample_rate) = 16."""
    case = CASES[10]
    x = case_signal(case)
    xb = torch.from_numpy(np.stack([x, x[::-1].copy(), np.zeros_like(x)])).to(cuda_device)
    got = yin_estimate(xb, 8000, pitch_min=250, pitch_max=20000, frame_stride=0.002)
    assert got.shape == (3, case[1]) and got.dtype == torch.float32 and got.is_cuda
    keep = compared(case)
    assert np.array_equal(got[0].cpu().numpy()[keep], oracle(case)["f0"][keep]) and (got[2] == 0).all()
    rev = orc.analyse(x[::-1], 8000, 0, 32, 16)
    rk = rev["margin"] > eps_of("S")
    assert rk.mean() >= 0.98 and np.array_equal(got[1].cpu().numpy()[rk], rev["f0"][rk])
    assert torch.equal(yin_estimate(xb[0], 8000, 250, 20000, 0.002), got[0])
    print(f"yin_estimate: {int(keep.sum())} + {int(rk.sum())} frames compared, voiced {int((got[0] > 0).sum())}")


def test_drop_ins_match_the_oracle(built_lib, cuda_device):
    """f0_torchyin (ndarray in, log-f0 ndarray out) and YinF0Extractor (ragged, fitted to given frame counts)."""
    case = CASES[11]                                  # R, 12 frames
    x = case_signal(case)
    got = f0_torchyin(x, 24000, hop_size=300, frame_length=1200)
    want = orc.f0_torchyin(x, 24000, hop_size=300, frame_length=1200)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape == (12,)
    keep = compared(case)
    ulp = np.abs(got[keep].view(np.int32).astype(np.int64) - want[keep].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (got[keep] > 0).any() and (got[keep][want[keep] == 0] == 0).all()
    ex = YinF0Extractor.from_config(dict(sampling_rate=24000, hop_size=300, win_length=1200), log=False)
    xs = [x, case_signal(CASES[6])[:6000], torch.from_numpy(x[:700]).to(cuda_device).view(-1, 1)]
    frames = [16, 10, 3]
    outs = ex.extract_batch(xs, frames=frames)
    base = outs[0].untyped_storage().data_ptr()
    for w, n, o in zip(xs, frames, outs):
        w = w.cpu().numpy().reshape(-1) if isinstance(w, torch.Tensor) else w
        ref = orc.analyse(w, 24000, 2, 600, 300, out_frames=n)
        kp = ref["margin"] > eps_of("R")
        assert o.shape == (n,) and o.is_cuda and o.untyped_storage().data_ptr() == base and kp.mean() >= 0.98
        assert np.array_equal(o.cpu().numpy()[kp], ref["f0"][kp])
    own = ex.extract_batch(xs)
    assert [len(o) for o in own] == [12, 17, 1] and torch.equal(own[0], outs[0][:12]) and torch.equal(ex.extract(x), own[0])
    print(f"f0_torchyin: {int(keep.sum())} frames compared, largest log difference {int(ulp.max())} ulp")


def test_wav_to_uhifigan_end_to_end(built_lib, cuda_device):
    """wav -> LogMelExtractor + YinF0Extractor -> UHiFiGANGenerator.inference_batch_from_f0 on the small
    test config, against the same call fed the oracle's f0 under the same noise: identical, since k* agrees
    on every frame of these signals (asserted)."""
    from parallelwavegan_amd import UHiFiGANGenerator, configs, synthetic

    m = UHiFiGANGenerator(**configs.uhifigan_params("uhifigan_test"))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_module_state_dict(m, seed=4).items()})
    m = m.eval().to(cuda_device)
    hop = m.upsample_factor
    assert hop == 12
    config = dict(sampling_rate=8000, fft_size=256, hop_size=hop, win_length=64, num_mels=80, fmin=0, fmax=4000)
    xs = [signal(1200, 8000, (300.0, 900.0), 60), signal(700, 8000, (300.0, 600.0), 61)]
    mels = LogMelExtractor.from_config(config).extract_batch(xs)
    ex = YinF0Extractor.from_config(config, log=False)
    assert (ex.tau_min, ex.tau_max) == (0, 32)
    frames = [len(c) for c in mels]
    f0s = ex.extract_batch(xs, frames=frames)
    refs = [orc.analyse(x, 8000, 0, 32, hop, out_frames=n) for x, n in zip(xs, frames)]
    for f0, ref in zip(f0s, refs):
        assert ref["margin"].min() > eps_of("S") and (ref["k"] > 0).any() and (ref["k"] == 0).any()
        assert np.array_equal(f0.cpu().numpy().view(np.int32), ref["f0"].view(np.int32))  # k* agrees on every frame
    rs = np.random.RandomState(9)
    noises = [rs.standard_normal(n * hop).astype(np.float32) for n in frames]
    got = [y.clone() for y in m.inference_batch_from_f0(mels, f0s, 8000, "tile", noises=noises)]
    want = m.inference_batch_from_f0(mels, [r["f0"] for r in refs], 8000, "tile", noises=noises)
    for g, w, n in zip(got, want, frames):
        assert g.shape == (n * hop, 1) and torch.isfinite(g).all() and g.abs().max() > 0 and torch.equal(g, w)
    print(f"end to end: {frames} frames, voiced {[int((r['k'] > 0).sum()) for r in refs]}, outputs identical")
