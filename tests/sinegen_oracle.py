"""Float64 exact-phase oracle of SineGen (include/pwg_sine.h; reference layers/sine.py without
flag_for_pulse). Not a test module.

The per-sample increment is computed in fp32 exactly as torch does ((f_h / sr) % 1, the first
sample's + ini), turned into q = floor(rad * 2^64) mod 2^64, and accumulated with np.cumsum over
uint64, which wraps natively. The sine is then evaluated in float64 on the phase folded into
[-1/2, 1/2) of a cycle, so nothing of the oracle's own rounding exceeds 1e-15."""

import numpy as np

TWO64 = float(2 ** 64)


def expand(f0, hop, layout):
    """Frame-rate f0 (T,) to the sample rate: ``tile`` is what the reference's preprocessing builds
    (ext[i] = f0[i % T], bin/preprocess.py:431-436), ``hold`` is ext[i] = f0[i // hop]."""
    f0 = np.asarray(f0, np.float32).reshape(-1)
    i = np.arange(f0.size * hop)
    return f0[i % f0.size] if layout == "tile" else f0[i // hop]


def rad_fp32(f0, dim, sr):
    """(N, dim) fp32: torch's (f_h / sr) % 1 with f_h = f0 (h = 0), f0 * (h + 1) otherwise."""
    f0 = np.asarray(f0, np.float32).reshape(-1, 1)
    mult = np.arange(1, dim + 1, dtype=np.float32)[None]
    with np.errstate(all="ignore"):
        f = np.where(mult == 1, f0, f0 * mult).astype(np.float32)
        r = np.fmod(f / np.float32(sr), np.float32(1)).astype(np.float32)
        r = np.where(r < 0, r + np.float32(1), r).astype(np.float32)
    return r


def q_of_rad(rad):
    """floor(rad * 2^64) mod 2^64 as uint64, for fp32 rad in [0, 2]; 0 where rad is not finite."""
    rad = np.asarray(rad, np.float32)
    ok = np.isfinite(rad)
    r = np.where(ok, rad, 0).astype(np.float64)  # an fp32 value and its fraction are exact in float64
    fr = r - np.floor(r)
    hi = np.floor(fr * 2.0 ** 32)                # split the 64-bit fraction: float64 -> uint64 stays exact
    lo = np.floor((fr * 2.0 ** 32 - hi) * 2.0 ** 32)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def increments(f0, dim, sr, ini=None):
    """(N, dim) uint64 increments of one utterance and the (N,) mask of non-finite f0."""
    f0 = np.asarray(f0, np.float32).reshape(-1)
    rad = rad_fp32(f0, dim, sr)
    bad = ~np.isfinite(f0)[:, None] | ~np.isfinite(rad)
    if ini is not None and f0.size:
        rad = rad.copy()
        rad[0] = rad[0] + np.asarray(ini, np.float32).reshape(dim)
    q = q_of_rad(rad)
    q[bad] = 0
    return q, ~np.isfinite(f0)


def phase_to_sin(phase):
    signed = phase.astype(np.int64)  # reinterpretation: [-1/2, 1/2) of a cycle
    return np.sin(2.0 * np.pi * (signed.astype(np.float64) / TWO64))


def sinegen(f0, sr, harmonic_num=0, sine_amp=0.1, noise_std=0.003, voiced_threshold=0, ini=None, n=None):
    """One utterance at the sample rate: f0 (N,) -> (sine (N, dim), uv (N,), noise (N, dim)) in float64."""
    dim = harmonic_num + 1
    f0 = np.asarray(f0, np.float32).reshape(-1)
    q, nonfinite = increments(f0, dim, sr, ini)
    phase = np.cumsum(q, axis=0, dtype=np.uint64)
    uv = ((f0 > np.float32(voiced_threshold)) & ~nonfinite).astype(np.float64)
    # the noise amplitude as the reference's fp32 arithmetic gives it
    namp = np.where(uv > 0, np.float32(noise_std), np.float32(sine_amp) / np.float32(3)).astype(np.float64)
    nz = np.zeros((f0.size, dim)) if n is None else np.asarray(n, np.float64).reshape(f0.size, dim)
    noise = namp[:, None] * nz
    sine = phase_to_sin(phase) * float(np.float32(sine_amp)) * uv[:, None] + noise
    return sine, uv, noise


def phase_sequential(q):
    """Plain sequential wrapping accumulation (Python ints), the definition the closed forms restate."""
    out = np.zeros(q.shape, np.uint64)
    for h in range(q.shape[1]):
        acc = 0
        for i in range(q.shape[0]):
            acc = (acc + int(q[i, h])) & (2 ** 64 - 1)
            out[i, h] = acc
    return out


def phase_closed_form(f0, hop, layout, dim, sr, ini=None):
    """The phase of every sample from the frame-rate prefix P, total S and the ini correction, as
    pwg_sine_frames computes it (wrapping uint64 throughout)."""
    f0 = np.asarray(f0, np.float32).reshape(-1)
    T = f0.size
    q, _ = increments(f0, dim, sr)
    P = np.cumsum(q, axis=0, dtype=np.uint64)
    S = P[-1]
    delta = np.zeros(dim, np.uint64)
    if ini is not None:
        qi, _ = increments(f0[:1], dim, sr, ini)
        delta = qi[0] - q[0]
    i = np.arange(T * hop, dtype=np.uint64)
    with np.errstate(over="ignore"):
        if layout == "tile":
            return (i // np.uint64(T))[:, None] * S[None] + P[(i % np.uint64(T)).astype(np.int64)] + delta[None]
        t = (i // np.uint64(hop)).astype(np.int64)
        j = i % np.uint64(hop)
        return np.uint64(hop) * (P[t] - q[t]) + (j + np.uint64(1))[:, None] * q[t] + delta[None]
