"""Audio conditioning on the GPU (include/pwg_wave.h) against the float64 oracle (tests/wave_oracle.py).

Trim: the bounds equal the oracle's exactly in both pad modes on every case (tests/test_wave_host.py asserts
that every frame of every case is decided with a margin above 1e-3, so none is left out), and the power rows
are within (fl + 2) 2^-24 (relative). Resample: per output |y - oracle| <= (n_m + 3) 2^-24 sum |hf x|, n_m the
taps used: the derived bound of an fp32 fma chain over once-rounded taps. Fit: bit-equal to NumPy's cut, edge
pad and fp32 product, the peaks equal to np.abs(out).max(). Ragged batches, permuted orders, a second launch
chunk and graph replay are bit-identical to the lone run. Every test prints its measured figure.

Measured on an MI355X: the bounds equal on all 25 cases in both pad modes; the power rows within
1.9e-7 of the oracle (bars 3.1e-6 to 1.2e-4); the resampled outputs at most 0.21 of the derived bound over the six
ratios (0.38 at 640/1 with 12,801 taps); fit, peaks, batches, orders and graph replays bit-identical; the CLI's
conditioned wave bit-equal to the oracle's and its features identical to LogMelExtractor's on the trimmed audio."""

import ctypes
import logging
import wave as wave_module

import numpy as np
import pytest
import torch
import yaml

import wave_oracle as orc
from wave_helpers import (GEOMETRIES, LENGTHS, PAD_MODES, RATIOS, TILE, TRIM_CASES, bits, length_for_outputs,
                          resample_oracle, resample_signal, run_fit, run_resample, run_trim, starts, trim_case_signal,
                          trim_oracle, trim_power_bound, trim_signal, worst_ratio)
from parallelwavegan_amd import (AudioConditioner, LogMelExtractor, _lib, kaiser_lowpass_taps, resample, resample_poly,
                                 trim_silence)
from parallelwavegan_amd.audio import ResamplePlan, TrimPlan

pytestmark = pytest.mark.gpu

BIG = 1e6  # what the neighbours of an utterance are filled with in the isolation tests


def _rel(got, want):
    return float((np.abs(got.astype(np.float64) - want) / want).max())


# ------------------------------------------------------------------------------------------------ trim
@pytest.mark.parametrize("pad_mode", PAD_MODES)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_trim_bounds_equal_the_oracle(geometry, pad_mode, built_lib, cuda_device):
    """Per geometry the four shapes of the signal family and F - 1, F, F + 1, 2 F + 3 frames of the power
    kernel's frame tile F (2048 / 512 / 60: one case)."""
    fl = GEOMETRIES[geometry][0]
    worst = 0.0
    cases = [c for c in TRIM_CASES if c[0] == geometry]
    for case in cases:
        want = trim_oracle(case, pad_mode)
        (bounds, power), = run_trim(cuda_device, [trim_case_signal(case)], geometry, pad_mode)
        assert bounds == want["bounds"], (case, bounds, want["bounds"])
        assert power.dtype == np.float32 and power.shape == want["power"].shape
        err = _rel(power, want["power"])
        worst = max(worst, err)
        assert err <= trim_power_bound(fl), (case, err)
        (b2, p2), = run_trim(cuda_device, [trim_case_signal(case)], geometry, pad_mode, want_power=False)
        assert p2 is None and b2 == bounds                  # the bounds kernel's own powers decide alike
    print(f"{geometry} {pad_mode}: {len(cases)} cases, power vs oracle {worst:.2e} (bar {trim_power_bound(fl):.2e})")


def test_trim_silence_and_tiny_utterances(built_lib, cuda_device):
    """All-zero input is kept whole; utterances shorter than a frame, down to one sample."""
    for g, (fl, hop, top_db) in GEOMETRIES.items():
        xs = [np.zeros(5 * hop + 3, np.float32), np.full(1, 0.25, np.float32), trim_signal(fl // 2 + 1, 0, 0, 5),
              np.zeros(1, np.float32)]
        for mode in PAD_MODES:
            for x, (bounds, power) in zip(xs, run_trim(cuda_device, xs, g, mode)):
                want = orc.trim_analyse(x, fl, hop, top_db, mode)
                assert bounds == want["bounds"] and len(power) == len(want["power"])
                assert want["margin"].min() > 1e-3
            assert run_trim(cuda_device, xs, g, mode)[0][0] == (0, 5 * hop + 3)


# -------------------------------------------------------------------------------------------- resample
def _resample_lengths(up, down):
    return sorted(set(LENGTHS) | {length_for_outputs(n, up, down) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)})


@pytest.mark.parametrize("up, down", RATIOS, ids=lambda v: str(v))
def test_resample_within_the_derived_bound(up, down, built_lib, cuda_device):
    worst = 0.0
    for T in _resample_lengths(up, down):
        want, bound = resample_oracle(T, up, down)
        got, = run_resample(cuda_device, [resample_signal(T, 7)], up, down)
        assert got.shape == want.shape and got.dtype == np.float32
        r = worst_ratio(got, want, bound)
        worst = max(worst, r)
        assert r <= 1.0, (T, r)
    assert ResamplePlan(cuda_device, up, down).tile == TILE
    print(f"resample {up}/{down}: lengths {_resample_lengths(up, down)}, worst |y - oracle| / bound {worst:.3f}")


def test_resample_small_tile_copy_and_custom_taps(built_lib, cuda_device):
    """1/640 with 12801 taps: the tile shrinks to what the LDS holds next to the taps, and the 44 outputs span
    more than one. up == down is a copy. Caller's taps: a unit tap decimates, (0.5, 1, 0.5) interpolates."""
    T = 28000
    x = resample_signal(T, 11)
    plan = ResamplePlan(cuda_device, 1, 640)
    assert 1 <= plan.tile < 44 == plan.out_len(T)
    y, cnt, mag = orc.resample(x, 1, 640, with_bound=True)
    got, = run_resample(cuda_device, [x], 1, 640)
    r = worst_ratio(got, y, (cnt + 3) * 2.0 ** -24 * mag)
    assert r <= 1.0
    y, cnt, mag = orc.resample(x[:50], 640, 1, with_bound=True)
    got, = run_resample(cuda_device, [x[:50]], 640, 1)
    r2 = worst_ratio(got, y, (cnt + 3) * 2.0 ** -24 * mag)
    assert r2 <= 1.0 and len(got) == 32000
    print(f"resample 1/640 (tile {plan.tile}) and 640/1: worst ratio to the bound {r:.3f}, {r2:.3f}")
    for w in run_resample(cuda_device, [x[:777], x[777:800]], 3, 3), run_resample(cuda_device, [x[:777], x[777:800]], 1, 1):
        assert np.array_equal(bits(np.concatenate(w)), bits(x[:800]))
    got, = run_resample(cuda_device, [x[:101]], 1, 2, taps=np.array([0.0, 1.0, 0.0]))
    assert np.array_equal(bits(got), bits(x[:101:2]))
    got, = run_resample(cuda_device, [x[:101]], 2, 1, taps=np.array([0.5, 1.0, 0.5]))
    assert np.array_equal(bits(got[::2]), bits(x[:101])) and np.array_equal(got[1:-1:2], np.float32(0.5) * x[:100] + np.float32(0.5) * x[1:101])


# ------------------------------------------------------------------------------------------------- fit
@pytest.mark.parametrize("gain", [1.0, 0.8, 0.5])
def test_fit_is_bit_equal_to_numpy(gain, built_lib, cuda_device):
    """out_len below, at and above the source length, and 1; a cut of an inner range; more than one block."""
    wave = resample_signal(9000, 21)
    src = [(0, 777), (777, 500), (1300, 1), (1400, 2049), (3500, 5000), (100, 300)]
    outs = [500, 500, 7, 1, 2 * 2048 + 1500 + 5000, 2048]
    got, peaks = run_fit(cuda_device, wave, [s for s, _ in src], [n for _, n in src], outs, gain)
    for (s, n), m, y, pk in zip(src, outs, got, peaks):
        want = np.pad(wave[s:s + n], (0, max(0, m - n)), mode="edge")[:m] * np.float32(gain)
        assert np.array_equal(bits(want), bits(orc.fit(wave, s, n, m, gain)))
        assert y.dtype == np.float32 and np.array_equal(bits(y), bits(want))
        assert pk == np.abs(want).max() and pk.dtype == np.float32
    none, no_peak = run_fit(cuda_device, wave, [0], [777], [800], gain, want_peak=False)
    assert no_peak is None and np.array_equal(bits(none[0]), bits(orc.fit(wave, 0, 777, 800, gain)))
    z, pk = run_fit(cuda_device, np.zeros(10, np.float32), [0], [10], [20], gain)
    assert (z[0] == 0).all() and pk[0] == 0


# ------------------------------------------------------------------------------------------- isolation
def _between(xs):
    """Each utterance between neighbours filled with BIG, ragged; returns (batch, positions of xs)."""
    batch, pos = [np.full(37, BIG, np.float32)], []
    for i, x in enumerate(xs):
        pos.append(len(batch))
        batch += [x, np.full(11 + 29 * i, BIG, np.float32)]
    return batch, pos


@pytest.mark.parametrize("pad_mode", PAD_MODES)
def test_trim_batch_is_bit_identical_to_single_runs_in_any_order(pad_mode, built_lib, cuda_device):
    cases = [c for c in TRIM_CASES if c[0] == "g50"][:5]
    xs = [trim_case_signal(c) for c in cases]
    alone = [run_trim(cuda_device, [x], "g50", pad_mode)[0] for x in xs]
    batch, pos = _between(xs)
    res = run_trim(cuda_device, batch, "g50", pad_mode)
    order = list(reversed(range(len(batch))))
    rev = run_trim(cuda_device, [batch[i] for i in order], "g50", pad_mode)
    for c, a, p in zip(cases, alone, pos):
        assert a[0] == trim_oracle(c, pad_mode)["bounds"]
        for b in (res[p], rev[order.index(p)]):
            assert b[0] == a[0] and np.array_equal(bits(b[1]), bits(a[1]))
    for i, x in enumerate(batch):
        if i not in pos:
            assert res[i][0] == (0, len(x))       # a constant utterance is kept whole


def test_resample_batch_is_bit_identical_to_single_runs_in_any_order(built_lib, cuda_device):
    for up, down in ((80, 147), (3, 2)):
        xs = [resample_signal(T, 7) for T in (1, 5, 777, 2000, length_for_outputs(TILE + 1, up, down))]
        alone = [run_resample(cuda_device, [x], up, down)[0] for x in xs]
        batch, pos = _between(xs)
        res = run_resample(cuda_device, batch, up, down)
        order = list(reversed(range(len(batch))))
        rev = run_resample(cuda_device, [batch[i] for i in order], up, down)
        for a, p in zip(alone, pos):
            assert np.abs(a).max() < 2.0
            assert np.array_equal(bits(res[p]), bits(a)) and np.array_equal(bits(rev[order.index(p)]), bits(a))


def test_fit_reads_only_its_source_range(built_lib, cuda_device):
    x = resample_signal(600, 3)
    wave = np.concatenate([np.full(50, BIG, np.float32), x, np.full(50, BIG, np.float32)])
    src_s, src_n, outs = [0, 50, 650, 50, 350], [50, 600, 50, 300, 300], [80, 900, 20, 300, 250]
    got, peaks = run_fit(cuda_device, wave, src_s, src_n, outs, 0.8)
    order = [3, 1, 4, 0, 2]
    perm, ppeaks = run_fit(cuda_device, wave, [src_s[i] for i in order], [src_n[i] for i in order], [outs[i] for i in order], 0.8)
    for i in (1, 3, 4):
        want = orc.fit(wave, src_s[i], src_n[i], outs[i], 0.8)
        assert np.abs(want).max() < 1.0 and peaks[i] == np.abs(want).max() == ppeaks[order.index(i)]
        assert np.array_equal(bits(got[i]), bits(want)) and np.array_equal(bits(perm[order.index(i)]), bits(want))
    assert peaks[0] == np.float32(0.8) * np.float32(BIG)


def test_more_than_one_launch_chunk(built_lib, cuda_device):
    """65 short utterances: two launches of up to 64; every utterance as alone."""
    case = [c for c in TRIM_CASES if c[0] == "g64"][3]                # 3 hops
    x = trim_case_signal(case)
    xs = [x[: len(x) - (i % 5)] for i in range(65)]
    lone = {n: run_trim(cuda_device, [x[:n]], "g64")[0] for n in {len(v) for v in xs}}
    for v, (b, p) in zip(xs, run_trim(cuda_device, xs, "g64")):
        assert b == lone[len(v)][0] and np.array_equal(bits(p), bits(lone[len(v)][1]))
    lone = {n: run_resample(cuda_device, [x[:n]], 2, 3)[0] for n in {len(v) for v in xs}}
    for v, y in zip(xs, run_resample(cuda_device, xs, 2, 3)):
        assert np.array_equal(bits(y), bits(lone[len(v)]))
    wave = np.concatenate(xs)
    s = np.concatenate([[0], np.cumsum([len(v) for v in xs])[:-1]])
    outs = [len(v) + (i % 3) - 1 for i, v in enumerate(xs)]
    got, peaks = run_fit(cuda_device, wave, s, [len(v) for v in xs], outs, 0.5)
    for i, (v, m, y) in enumerate(zip(xs, outs, got)):
        want = orc.fit(v, 0, len(v), m, 0.5)
        assert np.array_equal(bits(y), bits(want)) and peaks[i] == np.abs(want).max()


# --------------------------------------------------------------------------------------- graph capture
def _capture(dev, launch):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return graph


def test_graph_capture_replays_the_same_bits(built_lib, cuda_device):
    L, dev = built_lib, cuda_device
    case = [c for c in TRIM_CASES if c[0] == "g64"][0]
    x = trim_case_signal(case)
    wave = torch.from_numpy(x).to(dev)
    st = starts(0, len(x))

    plan = TrimPlan(dev, 64, 16, 20.0)
    direct = plan.run(wave, [len(x)])
    torch.cuda.synchronize(dev)
    outs = [torch.zeros_like(t) for t in direct]
    graph = _capture(dev, lambda s: _lib.check(L.pwg_trim_run(plan._h, wave.data_ptr(), st, 1, outs[0].data_ptr(),
                                                              outs[1].data_ptr(), outs[1].numel(), s)))
    assert all((o == 0).all() for o in outs)  # capture launches nothing
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(outs[0], direct[0]) and torch.equal(outs[1].view(torch.int32), direct[1].view(torch.int32))
    assert tuple(outs[0][0].tolist()) == trim_oracle(case, orc.PAD_ZERO)["bounds"]

    rplan = ResamplePlan(dev, 80, 147)
    rdirect = rplan.run(wave, [len(x)])
    torch.cuda.synchronize(dev)
    rout = torch.zeros_like(rdirect)
    graph = _capture(dev, lambda s: _lib.check(L.pwg_resample_run(rplan._h, wave.data_ptr(), st, 1, rout.data_ptr(),
                                                                  rout.numel(), s)))
    assert (rout == 0).all()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(rout.view(torch.int32), rdirect.view(torch.int32)) and rdirect.abs().max() > 0

    n = len(x)
    fout, fpeak = torch.zeros(n + 40, device=dev), torch.full((1,), 7.0, device=dev)
    graph = _capture(dev, lambda s: _lib.check(L.pwg_wave_fit_run(wave.data_ptr(), starts(0), starts(n), fout.data_ptr(),
                                                                  starts(0, n + 40), 1, ctypes.c_float(0.8), fpeak.data_ptr(), s)))
    assert (fout == 0).all() and fpeak[0] == 7.0
    for _ in range(2):                        # the peak is cleared inside the run: a replay gives it again
        graph.replay()
        torch.cuda.synchronize(dev)
        want = orc.fit(x, 0, n, n + 40, 0.8)
        assert np.array_equal(bits(fout.cpu().numpy()), bits(want)) and fpeak.cpu().numpy()[0] == np.abs(want).max()


def test_wrong_power_rows_and_out_total(built_lib, cuda_device):
    L = built_lib
    x = torch.zeros(100, device=cuda_device)
    st = starts(0, 100)
    plan, rplan = TrimPlan(cuda_device, 64, 16, 20.0), ResamplePlan(cuda_device, 1, 2)
    b, p = torch.zeros(2, dtype=torch.int64, device=cuda_device), torch.zeros(8, device=cuda_device)
    assert L.pwg_trim_run(plan._h, x.data_ptr(), st, 1, b.data_ptr(), p.data_ptr(), 8, None) == _lib.PWG_ERR_INVALID
    assert b"power_rows" in L.pwg_last_error()
    assert L.pwg_trim_run(plan._h, x.data_ptr(), st, 1, b.data_ptr(), p.data_ptr(), 7, None) == _lib.PWG_OK
    assert L.pwg_resample_run(rplan._h, x.data_ptr(), st, 1, p.data_ptr(), 51, None) == _lib.PWG_ERR_INVALID
    assert b"out_total" in L.pwg_last_error()
    torch.cuda.synchronize(cuda_device)
    assert b.tolist() == [0, 100]


# ------------------------------------------------------------------------------------------ Python API
def test_python_api(built_lib, cuda_device):
    case = [c for c in TRIM_CASES if c[0] == "g500"][0]
    x = trim_case_signal(case)
    for mode in PAD_MODES:
        y, idx = trim_silence(x, top_db=40, frame_length=500, hop_length=160, pad_mode=mode)
        a, b = trim_oracle(case, mode)["bounds"]
        assert isinstance(idx, np.ndarray) and tuple(idx) == (a, b) and np.array_equal(y, x[a:b])
    want, bound = resample_oracle(777, 80, 147)
    got = resample(resample_signal(777, 7), 44100, 24000)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and worst_ratio(got, want, bound) <= 1.0
    xd = torch.from_numpy(np.stack([resample_signal(777, 7), resample_signal(777, 8)])).to(cuda_device)
    yb = resample_poly(xd, 80, 147)
    assert yb.shape == (2, len(want)) and yb.is_cuda and worst_ratio(yb[0].cpu().numpy(), want, bound) <= 1.0
    assert torch.equal(resample_poly(xd[1], 160, 294), yb[1])
    y2 = resample_poly(xd[0], 2, 1, taps=np.array([0.5, 1.0, 0.5]))
    assert torch.equal(y2[::2], xd[0])
    assert kaiser_lowpass_taps(80, 147).shape == (2941,)

    # an LJSpeech-style config
    config = dict(sampling_rate=22050, fft_size=1024, hop_size=256, win_length=None, trim_silence=True,
                  trim_threshold_in_db=60, trim_frame_size=2048, trim_hop_size=512, global_gain_scale=1.0)
    cond = AudioConditioner.from_config(config)
    big = [c for c in TRIM_CASES if c[0] == "g2048"][0]
    xs = [trim_case_signal(big), torch.from_numpy(trim_signal(9000, 3000, 2500, 9)).to(cuda_device).view(-1, 1)]
    views, bounds = cond.trim_batch(xs)
    assert bounds.shape == (2, 2) and bounds.dtype == np.int64 and tuple(bounds[0]) == trim_oracle(big, orc.PAD_ZERO)["bounds"]
    assert tuple(bounds[1]) == orc.trim_bounds(xs[1].cpu().numpy().reshape(-1), 2048, 512, 60)
    base = views[0].untyped_storage().data_ptr()
    for v, w, (a, b) in zip(views, xs, bounds):
        w = w.cpu().numpy().reshape(-1) if isinstance(w, torch.Tensor) else w
        assert v.is_cuda and v.untyped_storage().data_ptr() == base and np.array_equal(v.cpu().numpy(), w[a:b])
    lens = [len(views[0]) + 100, len(views[1]) - 100]
    fitted, peaks = cond.fit_batch(views, lens, gain=0.8)
    for v, n, y, pk in zip(views, lens, fitted, peaks.cpu().numpy()):
        want_fit = orc.fit(v.cpu().numpy(), 0, len(v), n, 0.8)
        assert np.array_equal(bits(y.cpu().numpy()), bits(want_fit)) and pk == np.abs(want_fit).max()
    ys = cond.resample_batch([resample_signal(777, 7), resample_signal(5, 7)], 44100, 24000)
    assert worst_ratio(ys[0].cpu().numpy(), want, bound) <= 1.0 and len(ys[1]) == orc.resample_out_len(5, 80, 147)
    assert len(cond._plans) == 2
    import copy

    assert copy.deepcopy(cond)._plans == {}


# ------------------------------------------------------------------------------------------------- CLI
CONFIG = dict(sampling_rate=16000, fft_size=128, hop_size=50, win_length=80, window="hann", num_mels=16, fmin=20, fmax=7000,
              format="npy", trim_silence=True, trim_threshold_in_db=40, trim_frame_size=64, trim_hop_size=16,
              global_gain_scale=0.8)
ORACLE_ATOL = 4 * 3.5e-6   # tests/test_gpu_logmel.py's bar on raw log10 features


def _write_wav(path, x, sr):
    with wave_module.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(np.asarray(x, np.float64) * 32768.0).astype("<i2").tobytes())


def _pcm16(x):
    """x rounded to PCM16 steps, as a wav gives it back (+ 0.0: a sample that rounds to -0.0 comes back +0.0)."""
    return (np.round(np.asarray(x, np.float64) * 32768.0) / 32768.0 + 0.0).astype(np.float32)


def test_preprocess_cli_conditions_the_audio(built_lib, cuda_device, tmp_path, caplog):
    """wavs -> --condition-audio (trim, gain 0.8) -> the dump, against the oracle's trimmed, fitted and scaled
    audio (bit for bit) and LogMelExtractor on the oracle's trimmed audio; with a gain of 1.3 the loud wav
    clips and is skipped with the reference's warning."""
    from parallelwavegan_amd.bin import preprocess

    xs = {"utt_a": _pcm16(trim_signal(2000, 437, 611, 50)), "utt_b": _pcm16(trim_signal(1207, 0, 0, 51)),
          "utt_loud": _pcm16(np.clip(2.6 * trim_signal(900, 100, 100, 52), -0.999, 0.999))}
    (tmp_path / "wavs").mkdir()
    for utt, x in xs.items():
        _write_wav(tmp_path / "wavs" / f"{utt}.wav", x, 16000)
    with open(tmp_path / "conf.yml", "w") as f:
        yaml.safe_dump(CONFIG, f)
    common = ["--rootdir", str(tmp_path / "wavs"), "--config", str(tmp_path / "conf.yml"), "--verbose", "0"]
    for x in xs.values():
        assert orc.trim_analyse(x, 64, 16, 40)["margin"].min() > 1e-3
    with caplog.at_level(logging.WARNING):
        assert preprocess.main(common + ["--dumpdir", str(tmp_path / "dump"), "--condition-audio", "--extract-f0-yin"]) == 0
    assert "clipping" not in caplog.text
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == [f"{u}-{k}.npy" for u in xs for k in ("f0", "feats", "wave")]
    ex = LogMelExtractor.from_config(CONFIG)
    for utt in xs:
        trimmed, want = orc.condition(xs[utt], CONFIG, lambda n: 1 + n // 50)
        feats, audio = np.load(tmp_path / "dump" / f"{utt}-feats.npy"), np.load(tmp_path / "dump" / f"{utt}-wave.npy")
        assert audio.dtype == np.float32 and np.array_equal(bits(audio), bits(want))
        assert len(feats) * 50 == len(audio) and np.load(tmp_path / "dump" / f"{utt}-f0.npy").shape == (len(feats),)
        ref = ex.extract(trimmed).cpu().numpy()
        err = float(np.abs(feats - ref).max())
        print(f"{utt}: {len(xs[utt])} -> {len(trimmed)} samples, {len(feats)} frames, feats vs extractor {err:.2e}")
        assert feats.shape == ref.shape and err <= ORACLE_ATOL
    assert len(orc.condition(xs["utt_a"], CONFIG, lambda n: 1)[0]) < 2000 - 437 - 611 + 2 * 64
    # a gain of 1.3: utt_loud reaches 1.0 and is skipped, the others are written
    hot = dict(CONFIG, global_gain_scale=1.3)
    with open(tmp_path / "hot.yml", "w") as f:
        yaml.safe_dump(hot, f)
    loud = orc.condition(xs["utt_loud"], hot, lambda n: 1 + n // 50)[1]
    assert np.abs(loud).max() >= 1.0 > np.abs(orc.condition(xs["utt_a"], hot, lambda n: 1 + n // 50)[1]).max()
    with caplog.at_level(logging.WARNING):
        assert preprocess.main(["--rootdir", str(tmp_path / "wavs"), "--config", str(tmp_path / "hot.yml"), "--verbose", "0",
                                "--dumpdir", str(tmp_path / "hot"), "--condition-audio"]) == 0
    assert "utt_loud causes clipping" in caplog.text
    assert sorted(p.name for p in (tmp_path / "hot").iterdir()) == [f"{u}-{k}.npy" for u in ("utt_a", "utt_b")
                                                                    for k in ("feats", "wave")]
    assert np.array_equal(bits(np.load(tmp_path / "hot" / "utt_a-wave.npy")),
                          bits(orc.condition(xs["utt_a"], hot, lambda n: 1 + n // 50)[1]))
    # too short after the trim: raised for that file by name
    _write_wav(tmp_path / "wavs" / "blip.wav", _pcm16(trim_signal(900, 400, 498, 53)), 16000)
    with pytest.raises(ValueError, match=r"blip\.wav.*too short"):
        preprocess.main(common + ["--dumpdir", str(tmp_path / "dump2"), "--condition-audio"])


def test_preprocess_cli_resamples_the_input(built_lib, cuda_device, tmp_path):
    """An 8 kHz copy under a 16 kHz config with --resample-input: the dump of the oracle-resampled audio,
    within the resampler's bound."""
    from parallelwavegan_amd.bin import preprocess

    x = _pcm16(0.6 * resample_signal(1203, 31))
    (tmp_path / "wavs").mkdir()
    _write_wav(tmp_path / "wavs" / "utt_8k.wav", x, 8000)
    config = dict(CONFIG, trim_silence=False, global_gain_scale=1.0)
    with open(tmp_path / "conf.yml", "w") as f:
        yaml.safe_dump(config, f)
    assert preprocess.main(["--rootdir", str(tmp_path / "wavs"), "--config", str(tmp_path / "conf.yml"), "--verbose", "0",
                            "--dumpdir", str(tmp_path / "dump"), "--resample-input"]) == 0
    y, cnt, mag = orc.resample(x, 2, 1, with_bound=True)
    bound = (cnt + 3) * 2.0 ** -24 * mag
    audio, feats = np.load(tmp_path / "dump" / "utt_8k-wave.npy"), np.load(tmp_path / "dump" / "utt_8k-feats.npy")
    assert len(y) == 2406 and len(feats) == 1 + 2406 // 50 and len(audio) == len(feats) * 50
    n = min(len(y), len(audio))
    r = worst_ratio(audio[:n], y[:n], bound[:n])
    print(f"--resample-input: {len(x)} -> {len(y)} samples, worst ratio to the bound {r:.3f}")
    assert r <= 1.0 and (audio[n:] == audio[n - 1]).all()
    assert n == len(y)            # the fit padded: the first n samples are the resampled audio the mel was taken of
    ref = LogMelExtractor.from_config(config).extract(audio[:n]).cpu().numpy()
    assert np.abs(feats - ref).max() <= ORACLE_ATOL
