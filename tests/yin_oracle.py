"""The yardstick of the YIN tests: the estimator of include/pwg_yin.h in float64 NumPy, frame by frame,
with no FFT (de Cheveigne & Kawahara 2002, eqs. 6 and 8, with the conventions of the reference's
bin/preprocess.py:f0_torchyin as pinned in DESIGN.md 3.11). Not a test module."""

import numpy as np


def lag_bounds(fs, pitch_min, pitch_max):
    """(tau_min, tau_max) = (int(fs / pitch_max), int(fs / pitch_min))."""
    return int(fs / pitch_max), int(fs / pitch_min)


def n_frames(T, tau_max, hop):
    W = 2 * tau_max
    return 1 if T < W else 1 + (T - W) // hop


def frames(x, tau_max, hop):
    """(N, W) float64 frames of x: frame t covers x[t hop : t hop + W); an utterance shorter than W
    is zero-padded at its end."""
    x = np.asarray(x, np.float64).reshape(-1)
    W = 2 * tau_max
    if len(x) < 1:
        raise ValueError("an empty utterance has no frame")
    if len(x) < W:
        x = np.concatenate([x, np.zeros(W - len(x))])
    N = 1 + (len(x) - W) // hop
    return np.stack([x[t * hop:t * hop + W] for t in range(N)])


def difference(frame, tau_max):
    """d(tau) = sum_{j = 0}^{W - 1 - tau} (x[j] - x[j + tau])^2, tau = 0 .. tau_max - 1."""
    W = len(frame)
    d = np.zeros(tau_max)
    for tau in range(1, tau_max):
        diff = frame[:W - tau] - frame[tau:]
        d[tau] = np.dot(diff, diff)
    return d


def cmdf(frame, tau_min, tau_max):
    """c[k], k = 0 .. L - 1, tau = k + tau_min + 1: d(tau) tau / max(sum_{s = 1}^{tau} d(s), 1e-5)."""
    d = difference(frame, tau_max)
    tau = np.arange(1, tau_max)
    c = d[1:] * tau / np.maximum(np.cumsum(d[1:]), 1e-5)
    return c[tau_min:]


def search(c, threshold):
    """k* of one frame's c (0: unvoiced)."""
    below = np.flatnonzero(c < threshold)
    if len(below) == 0 or below[0] == 0:
        return 0
    k = int(below[0])
    while k < len(c) - 1 and c[k + 1] - c[k] < 0:
        k += 1
    return k


def margin(c, threshold):
    """The smallest relative margin of the decisions `search` took on c: |c[k] - thr| / max(c[k], thr)
    over every k it compared with the threshold, |c[k + 1] - c[k]| / (c[k + 1] + c[k]) over every slope
    it examined."""
    below = np.flatnonzero(c < threshold)
    last = len(c) - 1 if len(below) == 0 else int(below[0])
    m = float((np.abs(c[:last + 1] - threshold) / np.maximum(c[:last + 1], threshold)).min())
    if len(below) and below[0] > 0:
        k = last
        while k < len(c) - 1:
            m = min(m, float(abs(c[k + 1] - c[k]) / (c[k + 1] + c[k])))
            if c[k + 1] - c[k] >= 0:
                break
            k += 1
    return m


def fit(v, n):
    """Cut to n rows or hold the last one."""
    v = np.asarray(v)
    if len(v) >= n:
        return v[:n]
    return np.concatenate([v, np.repeat(v[-1:], n - len(v), axis=0)])


def analyse(x, fs, tau_min, tau_max, hop, threshold=0.1, out_frames=None):
    """dict(k, c, margin, f0): per frame the int k*, the float64 c rows, the decision margins and the
    float32 f0 = fs / (k* + tau_min + 1) (0 where unvoiced), fitted to out_frames rows when given."""
    fr = frames(x, tau_max, hop)
    c = np.stack([cmdf(f, tau_min, tau_max) for f in fr])
    k = np.array([search(row, threshold) for row in c], np.int64)
    m = np.array([margin(row, threshold) for row in c])
    f0 = np.where(k > 0, np.float32(fs) / (k + tau_min + 1).astype(np.float32), np.float32(0)).astype(np.float32)
    out = dict(k=k, c=c, margin=m, f0=f0)
    if out_frames is not None:
        out = {name: fit(v, out_frames) for name, v in out.items()}
    return out


def log_f0(f0):
    """The reference's log mode: voiced values replaced by their natural log (float32), zeros kept."""
    f0 = np.array(f0, np.float32)
    nz = f0 != 0
    f0[nz] = np.log(f0[nz])
    return f0


def f0_torchyin(audio, sampling_rate, hop_size=256, frame_length=None, pitch_min=40, pitch_max=10000, frames=None):
    """bin/preprocess.py:f0_torchyin by the oracle: the float32 log-f0 contour."""
    if frame_length is not None:
        pitch_min = sampling_rate / (frame_length / 2)
    tau_min, tau_max = lag_bounds(sampling_rate, pitch_min, pitch_max)
    return log_f0(analyse(audio, sampling_rate, tau_min, tau_max, hop_size, 0.1, frames)["f0"])
