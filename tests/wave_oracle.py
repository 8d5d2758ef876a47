"""Float64 NumPy oracle of the audio conditioning (include/pwg_wave.h): the closed forms, written for
clarity. Not a test module."""

import math

import numpy as np

PAD_ZERO, PAD_REFLECT = "constant", "reflect"


# ------------------------------------------------------------------------------------------------ trim
def trim_frames(T, fl, hop):
    return 1 + (T + 2 * (fl // 2) - fl) // hop


def padded(x, p, pad_mode):
    """x with p samples before and after: zeros, or the mirror at the utterance's own ends (period
    2 (T - 1), the end samples not repeated)."""
    x = np.asarray(x, np.float64)
    T = len(x)
    i = np.arange(-p, T + p)
    if pad_mode == PAD_ZERO:
        out = np.zeros(T + 2 * p)
        out[p:p + T] = x
        return out
    if T == 1:
        return np.full(T + 2 * p, x[0])
    m = np.mod(i, 2 * (T - 1))
    return x[np.where(m < T, m, 2 * (T - 1) - m)]


def trim_power(x, fl, hop, pad_mode=PAD_ZERO):
    """P[t] = mean of the squares of frame t, (n,) float64."""
    p = fl // 2
    xp = padded(x, p, pad_mode)
    n = trim_frames(len(x), fl, hop)
    return np.array([np.sum(xp[t * hop:t * hop + fl] ** 2) for t in range(n)]) / fl


def trim_analyse(x, fl, hop, top_db, pad_mode=PAD_ZERO):
    """dict(power (n,), bounds (start, end), margin (n,): |lhs / rhs - 1| of every frame's decision)."""
    T = len(x)
    P = trim_power(x, fl, hop, pad_mode)
    lhs = np.maximum(1e-10, P)
    rhs = max(1e-10, P.max()) * 10.0 ** (-top_db / 10.0)
    keep = np.flatnonzero(lhs > rhs)
    a, b = keep[0], keep[-1]
    return dict(power=P, bounds=(int(a * hop), int(min(T, (b + 1) * hop))), margin=np.abs(lhs / rhs - 1.0))


def trim_bounds(x, fl, hop, top_db, pad_mode=PAD_ZERO):
    return trim_analyse(x, fl, hop, top_db, pad_mode)["bounds"]


# -------------------------------------------------------------------------------------------- resample
def kaiser_taps(up, down, zeros=10, beta=5.0):
    g = math.gcd(up, down)
    up, down = up // g, down // g
    mx = max(up, down)
    half = zeros * mx
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(k / mx) / mx * np.kaiser(2 * half + 1, beta)
    return h / h.sum() * up


def resample_out_len(T, up, down):
    g = math.gcd(up, down)
    return -(-T * (up // g) // (down // g))


def resample(x, up, down, taps=None, with_bound=False):
    """y[m] = sum_i x[i] hf[m down + half - i up] in float64 over the closed form's range of i. With
    with_bound also (n_m: taps used per output, sum_i |x[i] hf[...]|)."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    x = np.asarray(x, np.float64)
    T = len(x)
    if up == down:
        return (x.copy(), np.ones(T, np.int64), np.abs(x)) if with_bound else x.copy()
    hf = np.asarray(kaiser_taps(up, down) if taps is None else taps, np.float64)
    assert len(hf) % 2 == 1
    half = len(hf) // 2
    n_out = -(-T * up // down)
    y, cnt, mag = np.zeros(n_out), np.zeros(n_out, np.int64), np.zeros(n_out)
    for m in range(n_out):
        lo = max(0, -((half - m * down) // up))          # ceil((m down - half) / up)
        hi = min(T - 1, (m * down + half) // up)
        i = np.arange(lo, hi + 1)
        terms = x[i] * hf[m * down + half - i * up]
        y[m], cnt[m], mag[m] = terms.sum(), len(i), np.abs(terms).sum()
    return (y, cnt, mag) if with_bound else y


# ------------------------------------------------------------------------------------------------- fit
def fit(x, start, length, out_len, gain):
    """float32: the cut x[start : start + length], edge-padded or cut to out_len, times the fp32 gain."""
    x = np.asarray(x, np.float32)[start:start + length]
    out = x[np.minimum(np.arange(out_len), length - 1)]
    return out * np.float32(gain)


def condition(x, config, frames_of):
    """The reference's order on one utterance (bin/preprocess.py:359-452) without resampling: trim, fit to
    frames_of(len(trimmed)) * hop_size, gain. Returns (trimmed float32, fitted and scaled float32)."""
    x = np.asarray(x, np.float32)
    if config.get("trim_silence"):
        a, b = trim_bounds(x, config["trim_frame_size"], config["trim_hop_size"], config["trim_threshold_in_db"])
        x = x[a:b]
    n = frames_of(len(x)) * config["hop_size"]
    audio = np.pad(x, (0, config["fft_size"]), mode="edge")[:n]
    assert len(audio) == n
    gain = config.get("global_gain_scale", 1.0)
    return x, audio * np.float32(gain) if gain > 0 else audio
