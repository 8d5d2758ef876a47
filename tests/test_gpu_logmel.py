"""Log-mel extraction on the GPU: pwg_mel_run (include/pwg_mel.h) against the float64 oracle
(tests/logmel_oracle.py) and the reference fixtures (tests/golden/logmel) over the tile boundaries, hops
that are no power of two, windows shorter than the frame, the real recipe geometries, ragged batches
(bit identity alone / in any order), silence, the log bases and statistics, the drop-in classes, the
status codes, graph capture, the preprocess CLI and an end-to-end vocoder run.

Two tolerances. ATOL = 1e-4 is the project's parity bar (against the reference's fp32 fixtures, and end
to end). ORACLE_ATOL = 4 R_MAX bounds the raw log10 output against the oracle: R_MAX is the worst error
of the REFERENCE's own fp32 path (CPU torch.stft + fp32 matmul) against the oracle over the test inputs
(tests/logmel_helpers.py:CASES; tests/test_logmel_host.py asserts it stays within 1e-5), and the factor
4 is how much more rounding a K-term fp32 sum collects than an FFT of K points: sqrt(K) against
log2(K), sqrt(2048) / 11 = 4. With statistics the bar is divided by the smallest scale; for log base 2 or
e it is multiplied by log2(10) or ln 10.

Measured: the reference's fp32 path is 3.48e-6 from the oracle at the most (the CLI test's 256/3/200
geometry; 2.55e-6 at LibriTTS with an 80 dB tilt, 1.3e-7 to 1.8e-6 on the other inputs, 8.7e-7 on the
fixtures), which R_MAX rounds up. The engine, measured on an
MI355X against the oracle (raw log10): 2.05e-6 at the most (the CLI test's geometry), 1.63e-6 at 1024/256/1024,
7.2e-7 at 2048/300/1200, 1.46e-6 at 64/16/64; 1.91e-6 from the reference fixtures; 1.2e-6 on the end-to-end
audio. Every test prints its own figure."""

import ctypes

import numpy as np
import pytest
import torch

import logmel_oracle as orc
from logmel_helpers import (CASES, FIXTURES, GEOMETRIES, TILE, case_signal, load_fixture, melmat_of, run_raw,
                            samples_for, synthetic_stats)
from parallelwavegan_amd import (LogMelExtractor, MelSpectrogram, ParallelWaveGANGenerator, _lib, configs,
                                 logmelfilterbank, synthetic)
from parallelwavegan_amd.logmel import MelPlan

pytestmark = pytest.mark.gpu

ATOL = 1e-4
R_MAX = 3.5e-6
ORACLE_ATOL = 4 * R_MAX
LOG_FACTOR = {10.0: 1.0, 2.0: float(np.log2(10.0)), None: float(np.log(10.0))}


def _oracle(case_or_x, geometry, amp_floor, log_base=10.0, stats=None):
    _, n_fft, hop, win, *_ = GEOMETRIES[geometry]
    mean, scale = stats if stats is not None else (None, None)
    return orc.logmel(case_or_x, n_fft, hop, win, melmat_of(geometry), 1e-10, log_base, amp_floor, mean, scale)


def _close(label, got, want, atol):
    assert got.shape == want.shape and got.dtype == np.float32, label
    err = float(np.abs(got - want).max())
    print(f"{label}: max|d| {err:.2e} (bar {atol:.1e})")
    assert np.isfinite(got).all() and err <= atol, label


def _cases(*geometries):
    return [c for c in CASES if c[0] in geometries]


@pytest.mark.parametrize("amp_floor", [False, True], ids=["preprocess", "mel_loss"])
@pytest.mark.parametrize("case", _cases("A"), ids=lambda c: f"T{c[1]}")
def test_geometry_a_tile_boundaries(built_lib, cuda_device, case, amp_floor):
    """n_fft 64, hop 16: 3 frames (T = 33, the shortest legal length, every frame reflecting on both
    sides), TILE - 1, TILE, TILE + 1 and 2 TILE + 3 frames."""
    x = case_signal(case)
    frames = 1 + len(x) // 16
    assert frames in (3, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
    got = run_raw(cuda_device, [x], "A", amp_floor)[0]
    _close(f"A frames {frames} amp_floor {amp_floor}", got, _oracle(x, "A", amp_floor), ORACLE_ATOL)


@pytest.mark.parametrize("amp_floor", [False, True], ids=["preprocess", "mel_loss"])
@pytest.mark.parametrize("case", _cases("B80", "B75")[:4], ids=lambda c: f"{c[0]}_T{c[1]}")
def test_geometry_b_hop_50_short_windows(built_lib, cuda_device, case, amp_floor):
    """n_fft 128, hop 50 (no power of two), win 80 (offset 24) and 75 (odd remainder: offset 26)."""
    x = case_signal(case)
    assert 1 + len(x) // 50 in (7, TILE + 2)
    got = run_raw(cuda_device, [x], case[0], amp_floor)[0]
    _close(f"{case[0]} T {len(x)} amp_floor {amp_floor}", got, _oracle(x, case[0], amp_floor), ORACLE_ATOL)


@pytest.mark.parametrize("case", _cases("lj", "libritts"), ids=lambda c: f"{c[0]}_T{c[1]}_tilt{c[2]}")
def test_real_geometries(built_lib, cuda_device, case):
    """LJSpeech 1024/256/1024 (513 bins) and LibriTTS 2048/300/1200 (1025 bins, K = 1200), 80 mels."""
    x = case_signal(case)
    for amp_floor in (False, True):
        got = run_raw(cuda_device, [x], case[0], amp_floor)[0]
        _close(f"{case} amp_floor {amp_floor}", got, _oracle(x, case[0], amp_floor), ORACLE_ATOL)


def test_ragged_batch_is_bit_identical_alone_and_in_any_order(built_lib, cuda_device):
    """Three utterances of 65, 50 TILE + 7 and 333 samples: each one's rows are the same bits alone, in
    the batch and in every batch order, so nothing leaks through the reflection or a tile's tail."""
    xs = [case_signal(c) for c in _cases("B80")[2:5]]
    assert [len(x) for x in xs] == [65, 50 * TILE + 7, 333]
    alone = [run_raw(cuda_device, [x], "B80", False)[0] for x in xs]
    for x, a in zip(xs, alone):
        _close(f"alone T {len(x)}", a, _oracle(x, "B80", False), ORACLE_ATOL)
    for order in ((0, 1, 2), (2, 1, 0), (1, 0, 2), (1, 2, 0)):
        got = run_raw(cuda_device, [xs[i] for i in order], "B80", False)
        for i, g in zip(order, got):
            assert np.array_equal(g.view(np.uint32), alone[i].view(np.uint32)), (order, i)
    # a loud neighbour on either side changes nothing either
    loud = np.full(400, 0.999, np.float32)
    got = run_raw(cuda_device, [loud, xs[0], loud], "B80", False)[1]
    assert np.array_equal(got.view(np.uint32), alone[0].view(np.uint32))


@pytest.mark.parametrize("amp_floor", [False, True], ids=["preprocess", "mel_loss"])
def test_silence(built_lib, cuda_device, amp_floor):
    x = np.zeros(samples_for(TILE + 1, 16), np.float32)
    got = run_raw(cuda_device, [x], "A", amp_floor)[0]
    _close(f"silence amp_floor {amp_floor}", got, _oracle(x, "A", amp_floor), ORACLE_ATOL)
    if not amp_floor:
        assert np.abs(got + 10.0).max() <= 1e-6  # log10(eps)


@pytest.mark.parametrize("amp_floor", [False, True], ids=["preprocess", "mel_loss"])
@pytest.mark.parametrize("case", _cases("D64", "D100"), ids=lambda c: f"{c[0]}_T{c[1]}")
def test_dense_matrix_reaches_the_dc_and_nyquist_bins(built_lib, cuda_device, case, amp_floor):
    """A dense caller-given matrix whose largest weights sit on bin 0 and on the Nyquist bin (every Slaney
    bank above has zeros there, and on most (bin tile, mel tile) pairs): the Nyquist bin's ride in bin 0's
    sine slot, its own eps floor, its column's add in the epilogue and every mask bit. D100 has n_fft / 2 =
    50, no multiple of 32, so the last bin tile ends in rows that must count for nothing, and 40 mels in
    two row tiles. T = 33 / 51 are the shortest legal lengths."""
    x = case_signal(case)
    mm = melmat_of(case[0])
    assert (mm > 0).all() and mm[:, 0].min() >= mm[:, 1:-1].max() and mm[:, -1].min() >= mm[:, 1:-1].max()
    got = run_raw(cuda_device, [x], case[0], amp_floor)[0]
    want = _oracle(x, case[0], amp_floor)
    _close(f"{case} dense amp_floor {amp_floor}", got, want, ORACLE_ATOL)
    # the two edge columns carry weight in the result: without either the oracle itself is far from `want`
    _, n_fft, hop, win, *_ = GEOMETRIES[case[0]]
    for col in (0, -1):
        cut = mm.copy()
        cut[:, col] = 0
        assert np.abs(orc.logmel(x, n_fft, hop, win, cut, amp_floor=amp_floor) - want).max() > 100 * ORACLE_ATOL


@pytest.mark.parametrize("amp_floor", [False, True], ids=["preprocess", "mel_loss"])
@pytest.mark.parametrize("geometry", ["D64", "D100"])
def test_dense_matrix_silence(built_lib, cuda_device, geometry, amp_floor):
    """All-zero input through a dense matrix: with amp_floor every bin, DC and Nyquist included, counts
    sqrt(eps), so a bin left out or counted twice moves the result; without it the result is log10(eps)."""
    _, n_fft, hop, *_ = GEOMETRIES[geometry]
    x = np.zeros(samples_for(TILE + 2, hop), np.float32)
    got = run_raw(cuda_device, [x], geometry, amp_floor)[0]
    want = _oracle(x, geometry, amp_floor)
    _close(f"{geometry} dense silence amp_floor {amp_floor}", got, want, ORACLE_ATOL)
    if amp_floor:
        mm = melmat_of(geometry).astype(np.float64)
        one_bin = np.abs(np.log10(1 + mm.min() / mm.sum(axis=1).max()))  # what one bin more or less would move
        assert one_bin > 20 * ORACLE_ATOL
    else:
        assert np.abs(got + 10.0).max() <= 1e-6


def test_dense_matrix_through_the_extractor(built_lib, cuda_device):
    """LogMelExtractor(melmat=...) and a ragged batch on the D100 geometry, bit-identical to each alone."""
    sr, n_fft, hop, win, num_mels, *_ = GEOMETRIES["D100"]
    mm = melmat_of("D100")
    ex = LogMelExtractor(sr, n_fft, hop, win, num_mels, melmat=mm, amp_floor=True)
    xs = [case_signal(c) for c in _cases("D100")]
    outs = ex.extract_batch(xs)
    for x, o in zip(xs, outs):
        _close(f"extractor dense T {len(x)}", o.cpu().numpy(), orc.logmel(x, n_fft, hop, win, mm, amp_floor=True), ORACLE_ATOL)
        assert torch.equal(ex.extract(x), o)


@pytest.mark.parametrize("with_stats", [False, True], ids=["raw", "stats"])
@pytest.mark.parametrize("log_base", [10.0, 2.0, None], ids=["log10", "log2", "ln"])
def test_log_bases_and_stats(built_lib, cuda_device, log_base, with_stats):
    case = _cases("B80")[1]
    x = case_signal(case)
    stats = synthetic_stats(16) if with_stats else None
    bar = ORACLE_ATOL * LOG_FACTOR[log_base] / (float(stats[1].min()) if with_stats else 1.0)
    got = run_raw(cuda_device, [x], "B80", True, log_base=log_base, stats=stats)[0]
    _close(f"log {log_base} stats {with_stats}", got, _oracle(x, "B80", True, log_base, stats), bar)


@pytest.mark.parametrize("name", FIXTURES)
def test_mel_spectrogram_drop_in_against_fixture_and_oracle(built_lib, cuda_device, name):
    fx = load_fixture(name)
    m = fx["meta"]
    mod = MelSpectrogram(fs=m["fs"], fft_size=m["fft_size"], hop_size=m["hop_size"], win_length=m["win_length"],
                         num_mels=m["num_mels"], fmin=m["fmin"], fmax=m["fmax"], log_base=m["log_base"]).to(cuda_device)
    assert np.array_equal(mod.melmat.cpu().numpy().T, fx["melmat"])
    x = torch.from_numpy(np.stack([fx["x"], fx["x"][::-1].copy()])).to(cuda_device)
    y3, y2 = mod(x[:, None, :]), mod(x)
    frames = 1 + x.shape[1] // m["hop_size"]
    assert tuple(y3.shape) == (2, m["num_mels"], frames) and y3.device == x.device and torch.equal(y3, y2)
    got = y3[0].T.contiguous().cpu().numpy()
    factor = LOG_FACTOR[m["log_base"]]
    _close(f"{name} vs reference", got, fx["y"], ATOL)
    want = orc.logmel(fx["x"], m["fft_size"], m["hop_size"], m["win_length"], fx["melmat"], m["eps"], m["log_base"], True)
    _close(f"{name} vs oracle", got, want.astype(np.float64), ORACLE_ATOL * factor)
    want_rev = orc.logmel(fx["x"][::-1], m["fft_size"], m["hop_size"], m["win_length"], fx["melmat"], m["eps"],
                          m["log_base"], True)
    _close(f"{name} reversed vs oracle", y3[1].T.contiguous().cpu().numpy(), want_rev, ORACLE_ATOL * factor)


def test_logmelfilterbank_and_extractor(built_lib, cuda_device):
    fx = load_fixture("lm_B80_T320")
    m = fx["meta"]
    kw = dict(fft_size=128, hop_size=50, win_length=80, num_mels=16)
    want = orc.logmel(fx["x"], 128, 50, 80, fx["melmat"], amp_floor=False)
    got = logmelfilterbank(fx["x"], 16000, **kw)
    assert isinstance(got, np.ndarray)
    _close("logmelfilterbank vs oracle", got, want, ORACLE_ATOL)
    _close("logmelfilterbank vs reference fixture", got, fx["y"], ATOL)  # the power clamp never binds on this input
    t = logmelfilterbank(torch.from_numpy(fx["x"]).to(cuda_device), 16000, **kw)
    assert t.device.type == "cuda" and np.array_equal(t.cpu().numpy(), got)
    stats = synthetic_stats(16)
    ex = LogMelExtractor(16000, stats=np.stack(stats), **kw)
    other = case_signal(("B80", 777, 30, 50))
    outs = ex.extract_batch([fx["x"][:, None], torch.from_numpy(other).to(cuda_device)])
    assert [tuple(o.shape) for o in outs] == [(7, 16), (16, 16)] and all(o.device.type == "cuda" for o in outs)
    assert outs[0].untyped_storage().data_ptr() == outs[1].untyped_storage().data_ptr()  # views of one buffer
    _close("extractor with stats", outs[0].cpu().numpy(), (want - stats[0]) / stats[1], ORACLE_ATOL / float(stats[1].min()))
    pair = LogMelExtractor(16000, stats=stats, **kw).extract(fx["x"])
    assert torch.equal(pair, outs[0])
    assert m["hop_size"] == 50


def test_status_codes_and_python_errors(built_lib, cuda_device):
    L = built_lib
    mm = melmat_of("libritts")
    plan = MelPlan(cuda_device, 2048, 1200, 300, mm, 1e-10, 10.0, 0)
    wave = torch.zeros(4096, device=cuda_device)
    out = torch.full((32, 80), 7.0, device=cuda_device)

    def run(starts, rows, wave_ptr=wave.data_ptr(), out_ptr=out.data_ptr(), n=None, h=plan._h):
        arr = (ctypes.c_longlong * len(starts))(*starts)
        return L.pwg_mel_run(h, wave_ptr, arr, len(starts) - 1 if n is None else n, out_ptr, rows, None)

    INV = _lib.PWG_ERR_INVALID
    assert run([0, 1024], 4) == INV and b"n_fft / 2" in L.pwg_last_error()   # T <= n_fft // 2
    assert run([0, 1025, 2049], 8) == INV                                      # the second one is 1024 long
    assert run([0, 1025], 5) == INV and b"out_rows" in L.pwg_last_error()
    assert run([0, 2000, 1500], 8) == INV and run([-5, 1500], 6) == INV
    assert run([0, 1025], 4, wave_ptr=None) == INV and run([0, 1025], 4, out_ptr=None) == INV
    assert run([0, 1025], 4, n=0) == INV and run([0, 1025], 4, h=None) == INV
    assert L.pwg_mel_run(plan._h, wave.data_ptr(), None, 1, out.data_ptr(), 4, None) == INV
    torch.cuda.synchronize(cuda_device)
    assert (out == 7.0).all()  # nothing was launched
    assert run([0, 1025], 4) == _lib.PWG_OK
    torch.cuda.synchronize(cuda_device)
    assert torch.isfinite(out[:4]).all() and (out[4:] == 7.0).all()

    # the plan's checks with a device present, and the Python classes on top of them
    fp = mm.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    for args, want in (((2047, 1200, 300, 0, 80, fp, mm.size), INV), ((1024, 1200, 300, 0, 80, fp, 80 * 513), INV),
                       ((2048, 1200, 0, 0, 80, fp, mm.size), INV), ((2048, 1200, 300, 0, 0, fp, 0), INV),
                       ((2048, 1200, 300, 0, 80, fp, mm.size - 1), INV), ((2048, 1200, 300, 0, 40, fp, mm.size), INV)):
        assert L.pwg_mel_plan_create(*args, 1e-10, 10.0, 0, None, None, ctypes.byref(h)) == want, args
    assert L.pwg_mel_plan_create(2048, 1200, 300, 0, 80, fp, mm.size, 1e-10, 3.0, 0, None, None, ctypes.byref(h)) == \
        _lib.PWG_ERR_UNSUPPORTED
    assert not h.value
    with pytest.raises(ValueError, match="melmat"):
        MelPlan(cuda_device, 2048, 1200, 300, mm[:, :-1], 1e-10, 10.0, 0)
    with pytest.raises(NotImplementedError, match="log_base"):
        MelPlan(cuda_device, 2048, 1200, 300, mm, 1e-10, 3.0, 0)
    ex = LogMelExtractor(24000, 2048, 300, 1200, 80, 80, 7600)
    with pytest.raises(ValueError, match="too short"):
        ex.extract_batch([np.zeros(5000, np.float32), np.zeros(1024, np.float32)])
    assert tuple(ex.extract(np.zeros(1025, np.float32)).shape) == (4, 80)
    with pytest.raises(ValueError, match="too short"):
        MelSpectrogram(fs=24000, fft_size=2048, hop_size=300, win_length=1200)(torch.zeros(2, 1024, device=cuda_device))


def test_modules_copy_and_pickle_after_a_forward(built_lib, cuda_device):
    """The plans hold C handles: a deep copy, a pickle or a torch.save of a module that has run drops them
    and the copy builds its own."""
    import copy
    import io
    import pickle

    x = torch.from_numpy(case_signal(_cases("B80")[0])).to(cuda_device)[None]
    mod = MelSpectrogram(fs=16000, fft_size=128, hop_size=50, win_length=80, num_mels=16, fmin=None, fmax=None).to(cuda_device)
    y = mod(x)
    assert mod._plans
    buf = io.BytesIO()
    torch.save(mod, buf)
    buf.seek(0)
    for other in (copy.deepcopy(mod), pickle.loads(pickle.dumps(mod)), torch.load(buf, weights_only=False)):
        assert not other._plans and torch.equal(other(x), y)
    ex = LogMelExtractor(16000, 128, 50, 80, 16)
    f = ex.extract(x[0])
    assert ex._plans and torch.equal(copy.deepcopy(ex).extract(x[0]), f) and torch.equal(pickle.loads(pickle.dumps(ex)).extract(x[0]), f)


def test_graph_capture_replays_the_same_bits(built_lib, cuda_device):
    L = built_lib
    case = _cases("B80")[1]
    x = case_signal(case)
    plan = MelPlan(cuda_device, 128, 80, 50, melmat_of("B80"), 1e-10, 10.0, 1)
    wave = torch.from_numpy(x).to(cuda_device)
    direct = plan.run(wave, [len(x)])
    torch.cuda.synchronize(cuda_device)
    rows = direct.shape[0]
    out = torch.zeros_like(direct)
    starts = (ctypes.c_longlong * 2)(0, len(x))
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _lib.check(L.pwg_mel_run(plan._h, wave.data_ptr(), starts, 1, out.data_ptr(), rows,
                                 torch.cuda.current_stream(cuda_device).cuda_stream))
    torch.cuda.synchronize(cuda_device)
    assert (out == 0).all()  # capture launches nothing
    graph.replay()
    torch.cuda.synchronize(cuda_device)
    assert torch.equal(out.view(torch.int32), direct.view(torch.int32))


def _write_wav(path, x, sr):
    import wave

    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(x * 32768.0).astype("<i2").tobytes())


def test_preprocess_cli_feature_values_and_decode(built_lib, cuda_device, tmp_path):
    """wavs -> preprocess CLI -> decode CLI -> *_gen.wav without leaving the package; the dumped
    features against the oracle, raw and normalised."""
    import yaml

    from parallelwavegan_amd.bin import decode, preprocess
    from parallelwavegan_amd.utils import generator_class, read_pcm16_wav

    gtype, params = configs.vocoder_params("hifigan_noadd_test")  # 80 mels in, 3 samples per frame
    sr, n_fft, hop, win, num_mels, fmin, fmax = GEOMETRIES["cli"]
    assert (n_fft, hop, win) == (256, 3, 200)
    conf = dict(sampling_rate=sr, fft_size=n_fft, hop_size=hop, win_length=win, window="hann", num_mels=num_mels, fmin=fmin,
                fmax=fmax, format="npy", trim_silence=False, global_gain_scale=1.0, generator_type=gtype,
                generator_params=params)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(conf, f)
    sd = synthetic.make_module_state_dict(generator_class(gtype)(**params), seed=4)
    torch.save({"model": {"generator": {k: torch.from_numpy(v) for k, v in sd.items()}}, "steps": 1},
               tmp_path / "checkpoint-1steps.pkl")
    xs = {"utt_a": case_signal(("cli", 400, 20, 60)), "utt_b": case_signal(("cli", 1001, 40, 61))}
    (tmp_path / "wavs").mkdir()
    for utt, x in xs.items():
        _write_wav(tmp_path / "wavs" / f"{utt}.wav", x, 16000)
    stats = np.stack(synthetic_stats(80))
    np.save(tmp_path / "stats_in.npy", stats)
    common = ["--rootdir", str(tmp_path / "wavs"), "--config", str(tmp_path / "config.yml"), "--verbose", "0"]
    assert preprocess.main(common + ["--dumpdir", str(tmp_path / "raw")]) == 0
    assert preprocess.main(common + ["--dumpdir", str(tmp_path / "norm"), "--stats", str(tmp_path / "stats_in.npy")]) == 0
    mm = LogMelExtractor.from_config(conf).melmat
    for utt, x in xs.items():
        want = orc.logmel(x, 256, 3, 200, mm, amp_floor=False)
        feats, audio = np.load(tmp_path / "raw" / f"{utt}-feats.npy"), np.load(tmp_path / "raw" / f"{utt}-wave.npy")
        assert len(audio) == len(feats) * 3
        _close(f"cli {utt}", feats, want, ORACLE_ATOL)
        _close(f"cli {utt} normalised", np.load(tmp_path / "norm" / f"{utt}-feats.npy"), (want - stats[0]) / stats[1],
               ORACLE_ATOL / float(stats[1].min()))
    assert decode.main(["--dumpdir", str(tmp_path / "raw"), "--outdir", str(tmp_path / "gen"), "--checkpoint",
                        str(tmp_path / "checkpoint-1steps.pkl"), "--verbose", "0"]) == 0
    for utt, x in xs.items():
        y, sr = read_pcm16_wav(str(tmp_path / "gen" / f"{utt}_gen.wav"))
        assert sr == 16000 and len(y) == 3 * (1 + len(x) // 3) and np.isfinite(y).all()


def test_end_to_end_features_into_parallel_wavegan(built_lib, cuda_device):
    """ljspeech_v1 with synthetic weights (as smoke()): extract_batch's features and the oracle's features
    (cast to fp32) through the same generator with the same noise; the audio agrees within 1e-4."""
    params = configs.generator_params("ljspeech_v1")
    sd = synthetic.make_state_dict(params, seed=0)
    model = ParallelWaveGANGenerator(**configs.generator_params("ljspeech_v1"))
    model.remove_weight_norm()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.eval().to(cuda_device)
    x = case_signal(("lj", 2304, 40, 70))
    ex = LogMelExtractor(22050, 1024, 256, 1024, 80, 80, 7600)
    feats = ex.extract_batch([torch.from_numpy(x).to(cuda_device)])
    want = orc.logmel(x, 1024, 256, 1024, ex.melmat, amp_floor=False).astype(np.float32)
    assert tuple(feats[0].shape) == want.shape == (10, 80)
    noise = np.asarray(synthetic.make_noise(10 * 256, seed=2), np.float32).reshape(-1, 1)
    with torch.no_grad():
        y_engine = model.inference_batch(feats, [noise])[0].cpu().numpy()
        y_oracle = model.inference_batch([torch.from_numpy(want)], [noise])[0].cpu().numpy()
    err = float(np.abs(y_engine - y_oracle).max())
    print(f"end to end: max|d audio| {err:.2e}, max|d feats| {float(np.abs(feats[0].cpu().numpy() - want).max()):.2e}")
    assert y_engine.shape == (2560, 1) and np.isfinite(y_engine).all() and err <= ATOL
