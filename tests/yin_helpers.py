"""Helpers shared by the YIN tests (tests/test_yin_host.py, tests/test_gpu_yin.py): the test geometries and
signals, the derived error bound, an fp32 torch restatement of the estimator that takes the difference
function through rfft / irfft and cumulative energies (the route of the package the reference calls), and
raw calls of the C-ABI over ragged batches. Not a test module."""

import ctypes
import functools

import numpy as np
import torch

import yin_oracle as orc
from parallelwavegan_amd import _lib
from parallelwavegan_amd.yin import YinPlan

TILE = _lib.PWG_YIN_FRAME_TILE
THRESHOLD = 0.1
# The fp32 FFT route's worst relative error in c against the oracle over CASES (measured on the CPU: 1.37e-4;
# tests/test_yin_host.py asserts it). The GPU bar on c is max(R_MAX, eps_of(geometry)).
R_MAX = 1.4e-4

# name: sampling rate, hop, tau_min, tau_max, sweep (Hz)
GEOMETRIES = {
    "S": (8000, 16, 0, 32, (300.0, 900.0)),
    "S4": (8000, 16, 4, 32, (300.0, 900.0)),     # pitch_max 2000
    "R": (24000, 300, 2, 600, (110.0, 330.0)),   # LibriTTS: hop 300, win_length 1200
}


def eps_of(geometry):
    """2 (W + tau_max) 2^-24: the worst-case relative error of a W-term non-negative fp32 sum (each term
    a rounded difference, squared and added by one fma) followed by a tau_max-term one."""
    _, _, _, tau_max, _ = GEOMETRIES[geometry]
    return 2.0 * (2 * tau_max + tau_max) * 2.0 ** -24


def samples_for(frames, geometry, extra=0):
    """A length that gives `frames` frames: W + (frames - 1) hop + extra, extra < hop."""
    _, hop, _, tau_max, _ = GEOMETRIES[geometry]
    assert 0 <= extra < hop
    return 2 * tau_max + (frames - 1) * hop + extra


def signal(T, fs, sweep, seed):
    """Seeded and rounded to PCM16 steps: a leading quarter of white noise at 0.05 (unvoiced), then a
    four-harmonic sweep from sweep[0] to sweep[1] Hz with a 2 % vibrato plus noise at 0.002, and a trailing
    eighth of exact zeros (unvoiced through the fb == 0 rule)."""
    rs = np.random.RandomState(seed)
    n0, n2 = T // 4, T // 8
    n1 = T - n0 - n2
    t = np.arange(n1) / fs
    f = np.linspace(sweep[0], sweep[1], n1) * (1.0 + 0.02 * np.sin(2 * np.pi * 6.0 * t))
    phase = 2 * np.pi * np.cumsum(f) / fs
    voiced = sum(a * np.sin(h * phase + p) for h, a, p in ((1, 0.3, 0.0), (2, 0.15, 0.5), (3, 0.1, 1.1), (4, 0.05, 2.3)))
    x = np.concatenate([0.05 * rs.standard_normal(n0), voiced + 0.002 * rs.standard_normal(n1), np.zeros(n2)])
    return (np.round(np.clip(x, -1.0, 32767.0 / 32768.0) * 32768.0) / 32768.0).astype(np.float32)


# (geometry, frames, extra samples, seed): every input of the GPU tests that is compared with the oracle
CASES = (
    [("S", f, 3, 10 + i) for i, f in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE + 3))]
    + [("S", 201, 0, 20), ("S4", 201, 0, 21), ("R", 41, 0, 122)]
    + [("S", 40, 5, 30), ("S", 5, 0, 31), ("S", 77, 9, 32)]       # the ragged batch
    + [("S", 64, 0, 40), ("R", 12, 100, 41)]                        # drop-ins and the end-to-end run
)
SHORT = ("S", 41, 50)   # T < W: (geometry, T, seed); one zero-padded frame
LONG_FRAMES = {"S": 201, "S4": 201, "R": 41}


def case_signal(case):
    """The case's signal. A case of fewer than 30 frames is a cut from the geometry's long signal around
    the place where the noise ends and the sweep begins, so that it too holds unvoiced and voiced frames
    (a whole signal that short would sweep too fast to be periodic)."""
    g, frames, extra, seed = case
    fs, _, _, _, sweep = GEOMETRIES[g]
    T = samples_for(frames, g, extra)
    if frames >= 30:
        return signal(T, fs, sweep, seed)
    T_long = samples_for(LONG_FRAMES[g], g)
    start = T_long // 4 - T // 3
    return signal(T_long, fs, sweep, seed)[start:start + T].copy()


@functools.lru_cache(maxsize=None)
def oracle(case, out_frames=None):
    """The oracle's analysis of a case, computed once and shared (read-only)."""
    fs, hop, tau_min, tau_max, _ = GEOMETRIES[case[0]]
    res = orc.analyse(case_signal(case), fs, tau_min, tau_max, hop, THRESHOLD, out_frames)
    for v in res.values():
        v.setflags(write=False)
    return res


def compared(case, res=None):
    """Mask of the frames the oracle decided with margin (above the geometry's eps), from the oracle alone."""
    res = oracle(case) if res is None else res
    return res["margin"] > eps_of(case[0])


def rel_err(got, want):
    """max |got - want| / |want| over the entries; where want is exactly 0, got must be too."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    if zero.any() and np.abs(got[zero]).max() != 0:
        return float("inf")
    if zero.all():
        return 0.0
    return float((np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])).max())


def fft_route(x, fs, tau_min, tau_max, hop, threshold=THRESHOLD):
    """The estimator in fp32 torch on the CPU, d through the autocorrelation: d(tau) = E_head(tau) + E_tail(tau)
    - 2 r(tau) with r by rfft / irfft of the zero-padded frame and the energies by a cumulative sum, then
    cumsum, the threshold and the first-minimum search by argmax. Returns (c (N, L) float32, k (N,) int64,
    f0 (N,) float32)."""
    x = torch.from_numpy(np.asarray(x, np.float32)).reshape(-1)
    W = 2 * tau_max
    if x.numel() < W:
        x = torch.nn.functional.pad(x, (0, W - x.numel()))
    fr = x.unfold(0, W, hop)                                                     # (N, W)
    spec = torch.fft.rfft(fr, 2 * W)
    r = torch.fft.irfft(spec * spec.conj(), 2 * W)[:, :tau_max]
    cs = torch.nn.functional.pad(torch.cumsum(fr * fr, 1), (1, 0))               # cs[n] = sum_{j < n} x[j]^2
    tau = torch.arange(tau_max)
    d = cs[:, W - tau] + (cs[:, W:W + 1] - cs[:, tau]) - 2.0 * r
    lag = torch.arange(1, tau_max, dtype=torch.float32)
    c = (d[:, 1:] * lag / torch.clamp(torch.cumsum(d[:, 1:], 1), min=1e-5))[:, tau_min:]
    L = c.shape[1]
    fall = torch.arange(L, 0, -1)[None]           # argmax over mask * fall: the first True, 0 when there is none
    below = c < threshold
    fb = (below * fall).argmax(1)
    rising = torch.cat([(c[:, 1:] - c[:, :-1]) >= 0, torch.ones(len(c), 1, dtype=torch.bool)], 1)
    k = ((rising & (torch.arange(L)[None] >= fb[:, None])) * fall).argmax(1) * (fb > 0)
    f0 = torch.where(k > 0, torch.tensor(float(fs)) / (k + tau_min + 1).float(), torch.zeros(len(c)))
    return c.numpy(), k.numpy(), f0.numpy()


@functools.lru_cache(maxsize=1)
def fft_route_errors():
    """{case: worst relative error of the fp32 FFT route's c against the oracle}."""
    out = {}
    for case in CASES:
        fs, hop, tau_min, tau_max, _ = GEOMETRIES[case[0]]
        c, _, _ = fft_route(case_signal(case), fs, tau_min, tau_max, hop)
        out[case] = rel_err(c, oracle(case)["c"])
    return out


def run_raw(dev, waves, geometry, out_frames=None, log=False, want_tau=True, want_cmdf=True, threshold=THRESHOLD):
    """pwg_yin_run over the ragged batch `waves` in a geometry of GEOMETRIES: per utterance a dict of the
    f0, k (or None) and c (or None) arrays."""
    fs, hop, tau_min, tau_max, _ = GEOMETRIES[geometry]
    plan = YinPlan(dev, fs, tau_min, tau_max, hop, threshold, log)
    packed = torch.from_numpy(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in waves])).to(dev)
    f0, tau, cmdf = plan.run(packed, [len(w) for w in waves], out_frames, want_tau, want_cmdf)
    torch.cuda.synchronize(dev)
    rows = out_frames if out_frames is not None else [orc.n_frames(len(w), tau_max, hop) for w in waves]
    cut = np.cumsum(rows)[:-1]
    split = lambda t: np.split(t.cpu().numpy(), cut) if t is not None else [None] * len(waves)  # noqa: E731
    return [dict(f0=a, k=b, c=c) for a, b, c in zip(split(f0), split(tau), split(cmdf))]


# ------------------------------------------------------------------ raw C-ABI calls for the argument checks
P = ctypes.c_void_p(4096)  # a non-null, aligned pointer no check dereferences


def plan_create(L, fs=8000.0, tau_min=0, tau_max=32, hop=16, threshold=0.1, log_f0=0, plan="byref"):
    """pwg_yin_plan_create with arguments that pass every check unless overridden; returns the status.
    Only calls that fail a check are made without a device."""
    h = ctypes.c_void_p()
    return L.pwg_yin_plan_create(fs, tau_min, tau_max, hop, threshold, log_f0, ctypes.byref(h) if plan == "byref" else plan)
