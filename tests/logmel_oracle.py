"""Float64 NumPy restatement of the log-mel semantics of include/pwg_mel.h: explicit framing with
reflect padding, the periodic Hann window centred in the n_fft frame, a direct DFT with the angle
reduced in integers, the float32 mel matrix widened to float64, clamp, log, statistics. Independent of
the engine; its amplitude agrees with torch.stft in float64 within 3e-12. Not a test module."""

import functools

import numpy as np


def window(n_fft, win_length):
    """The periodic Hann window of win_length taps at offset (n_fft - win_length) // 2 of the frame."""
    w = np.zeros(n_fft, np.float64)
    off = (n_fft - win_length) // 2
    n = np.arange(win_length, dtype=np.float64)
    w[off:off + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    return w


@functools.lru_cache(maxsize=4)
def dft_basis(n_fft):
    """(cos, -sin)(2 pi n k / n_fft) for k in [0, n_fft // 2], n in [0, n_fft): two (bins, n_fft) arrays."""
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft
    return np.cos(ang), -np.sin(ang)


def n_frames(T, hop):
    return 1 + T // hop


def frames(x, n_fft, hop):
    """(frames, n_fft): frame t holds x[t hop + n - n_fft // 2], mirrored at the utterance's ends."""
    x = np.asarray(x, np.float64).reshape(-1)
    T, half = len(x), n_fft // 2
    if T <= half:
        raise ValueError(f"{T} samples cannot be reflect-padded by {half}")
    idx = np.arange(n_frames(T, hop))[:, None] * hop + np.arange(n_fft)[None, :] - half
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)
    return x[idx]


def amplitude(x, n_fft, hop, win_length, eps=1e-10, amp_floor=False):
    """(frames, n_fft // 2 + 1) magnitudes of the STFT."""
    fr = frames(x, n_fft, hop) * window(n_fft, win_length)[None, :]
    c, s = dft_basis(n_fft)
    re, im = fr @ c.T, fr @ s.T
    power = re * re + im * im
    if amp_floor:
        power = np.maximum(power, eps)
    return np.sqrt(power)


def log_of(log_base):
    return {None: np.log, 2.0: np.log2, 10.0: np.log10}[log_base]


def logmel(x, n_fft, hop, win_length, melmat, eps=1e-10, log_base=10.0, amp_floor=False, mean=None, scale=None):
    """(frames, num_mels) float64; melmat (num_mels, n_fft // 2 + 1) of any float type."""
    amp = amplitude(x, n_fft, hop, win_length, eps, amp_floor)
    mel = np.maximum(eps, amp @ np.asarray(melmat, np.float64).T)
    out = log_of(log_base)(mel)
    if mean is not None:
        out = (out - np.asarray(mean, np.float64)) / np.asarray(scale, np.float64)
    return out
