"""Helpers shared by the audio-conditioning tests (tests/test_wave_host.py, tests/test_gpu_wave.py): the trim
geometries and signal family, the resampler's ratios and lengths, derived bounds, and raw calls of the C-ABI
over ragged batches. Not a test module."""

import ctypes
import functools

import numpy as np
import torch

import wave_oracle as orc
from parallelwavegan_amd import _lib
from parallelwavegan_amd.audio import ResamplePlan, TrimPlan, fit_run

F = _lib.PWG_TRIM_FRAME_TILE
TILE = _lib.PWG_RESAMPLE_OUT_TILE
PAD_MODES = (orc.PAD_ZERO, orc.PAD_REFLECT)
MARGIN = 1e-3  # every frame's decision in the float64 oracle must be further than this from the threshold

# name: (fl, hop, top_db)
GEOMETRIES = {"g64": (64, 16, 20), "g50": (50, 16, 40), "g500": (500, 160, 40), "g2048": (2048, 512, 60)}


def trim_power_bound(fl):
    """(fl + 2) 2^-24: fl squares added by fma (lane partials, then a 6-step butterfly: fewer roundings than
    a serial chain of fl) and one division, each rounded once; all terms non-negative."""
    return (fl + 2) * 2.0 ** -24


def trim_signal(T, lead, tail, seed):
    """Seeded noise of sigma 1e-4 over the whole utterance; on [lead, T - tail) an amplitude-modulated tone."""
    n = np.arange(T)
    x = 1e-4 * np.random.RandomState(seed).standard_normal(T)
    tone = 0.5 * np.sin(2 * np.pi * 0.031 * n) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.0007 * n))
    x[lead:T - tail] += tone[lead:T - tail]
    return x.astype(np.float32)


def samples_for_frames(n, fl, hop):
    """The smallest T with trim_frames(T) == n."""
    T = max(1, (n - 1) * hop - 2 * (fl // 2) + fl)
    assert orc.trim_frames(T, fl, hop) == n and (T == 1 or orc.trim_frames(T - 1, fl, hop) == n - 1)
    return T


def _trim_cases():
    cases = []
    for g, (fl, h, _) in GEOMETRIES.items():
        if g == "g2048":
            cases.append((g, 40 * h + 3, 7 * h + 5, 9 * h + 1, 1))
            continue
        shapes = [(40 * h + 3, 7 * h + 5, 9 * h + 1), (65 * h, 0, 11 * h), (17 * h + h // 2, 5 * h, 0), (3 * h, h, h)]
        shapes += [(samples_for_frames(n, fl, h), 2 * h, 3 * h) for n in (F - 1, F, F + 1, 2 * F + 3)]
        cases += [(g, T, lead, tail, 100 + i) for i, (T, lead, tail) in enumerate(shapes)]
    return tuple(cases)


# (geometry, T, lead, tail, seed): every trim input of the GPU tests
TRIM_CASES = _trim_cases()


def trim_case_signal(case):
    _, T, lead, tail, seed = case
    return trim_signal(T, lead, tail, seed)


@functools.lru_cache(maxsize=None)
def trim_oracle(case, pad_mode):
    """The oracle's analysis of a case, computed once and shared (read-only)."""
    fl, hop, top_db = GEOMETRIES[case[0]]
    res = orc.trim_analyse(trim_case_signal(case), fl, hop, top_db, pad_mode)
    res["power"].setflags(write=False)
    res["margin"].setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------- resample
RATIOS = ((1, 2), (3, 2), (2, 3), (80, 147), (160, 147), (147, 160))
LENGTHS = (1, 5, 777, 2000)


def length_for_outputs(n, up, down):
    """The smallest T whose output length is >= n (exactly n whenever up <= down)."""
    T = -(-((n - 1) * down + 1) // up)
    assert orc.resample_out_len(T, up, down) >= n and (T == 1 or orc.resample_out_len(T - 1, up, down) < n)
    return T


def resample_signal(T, seed):
    rs = np.random.RandomState(seed)
    n = np.arange(T)
    return (0.4 * np.sin(2 * np.pi * 0.013 * n + 0.3) + 0.2 * np.sin(2 * np.pi * 0.11 * n) + 0.05 * rs.standard_normal(T)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def resample_oracle(T, up, down, seed=7):
    """(y float64, bound per output = (n_m + 3) 2^-24 sum |hf x|), computed once and shared (read-only)."""
    y, cnt, mag = orc.resample(resample_signal(T, seed), up, down, with_bound=True)
    bound = (cnt + 3) * 2.0 ** -24 * mag
    y.setflags(write=False)
    bound.setflags(write=False)
    return y, bound


def worst_ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 (no input under the taps) got must equal want."""
    err = np.abs(np.asarray(got, np.float64) - want)
    zero = bound == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ----------------------------------------------------------------------------------- raw runs on a device
def _packed(waves, dev):
    return torch.from_numpy(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in waves])).to(dev)


def run_trim(dev, waves, geometry, pad_mode=orc.PAD_ZERO, want_power=True):
    """pwg_trim_run over the ragged batch: per utterance ((start, end), power rows or None)."""
    fl, hop, top_db = GEOMETRIES[geometry]
    plan = TrimPlan(dev, fl, hop, top_db, pad_mode)
    bounds, power = plan.run(_packed(waves, dev), [len(w) for w in waves], want_power)
    torch.cuda.synchronize(dev)
    bounds = bounds.cpu().numpy()
    rows = [orc.trim_frames(len(w), fl, hop) for w in waves]
    pw = np.split(power.cpu().numpy(), np.cumsum(rows)[:-1]) if want_power else [None] * len(waves)
    return [((int(b[0]), int(b[1])), p) for b, p in zip(bounds, pw)]


def run_resample(dev, waves, up, down, taps=None):
    plan = ResamplePlan(dev, up, down, taps)
    out = plan.run(_packed(waves, dev), [len(w) for w in waves])
    torch.cuda.synchronize(dev)
    return np.split(out.cpu().numpy(), np.cumsum([plan.out_len(len(w)) for w in waves])[:-1])


def run_fit(dev, wave, src_start, src_len, out_lengths, gain, want_peak=True):
    """pwg_wave_fit_run on one source buffer: (per utterance outputs, peaks ndarray or None)."""
    out, peak = fit_run(torch.from_numpy(np.asarray(wave, np.float32)).to(dev), src_start, src_len, out_lengths, gain, want_peak)
    torch.cuda.synchronize(dev)
    return np.split(out.cpu().numpy(), np.cumsum(out_lengths)[:-1]), (peak.cpu().numpy() if want_peak else None)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------ raw C-ABI calls for the argument checks
P = ctypes.c_void_p(4096)  # a non-null, aligned pointer no check dereferences
LL = ctypes.c_longlong


def starts(*v):
    return (LL * len(v))(*v)


def trim_plan_create(L, fl=64, hop=16, top_db=20.0, pad_mode=0, plan="byref"):
    """pwg_trim_plan_create with arguments that pass every check unless overridden; returns the status. Only
    calls that fail a check are made without a device."""
    h = ctypes.c_void_p()
    return L.pwg_trim_plan_create(fl, hop, top_db, pad_mode, ctypes.byref(h) if plan == "byref" else plan)


def resample_plan_create(L, up=1, down=2, taps="default", tap_count=None, plan="byref"):
    h = ctypes.c_void_p()
    buf = np.zeros(41 if tap_count is None else max(1, tap_count), np.float32)
    return L.pwg_resample_plan_create(up, down, buf.ctypes.data if taps == "default" else taps,
                                      buf.size if tap_count is None else tap_count, ctypes.byref(h) if plan == "byref" else plan)
