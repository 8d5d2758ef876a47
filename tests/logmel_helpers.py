"""Helpers shared by the log-mel tests (tests/test_logmel_host.py, tests/test_gpu_logmel.py): the test
geometries and signals, the fixtures of tests/golden/logmel, a CPU restatement of the reference's fp32
path, and raw calls of the C-ABI over ragged batches. Not a test module."""

import ctypes
import functools
import glob
import json
import os

import numpy as np
import torch

import logmel_oracle as orc
from conftest import GOLDEN_DIR
from parallelwavegan_amd import _lib
from parallelwavegan_amd.logmel import MelPlan, slaney_mel_basis

LM_DIR = os.path.join(GOLDEN_DIR, "logmel")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(LM_DIR, "lm_*.npz")))
TILE = _lib.PWG_MEL_FRAME_TILE

# name: sampling rate, n_fft, hop, win_length, num_mels, fmin, fmax
GEOMETRIES = {
    "A": (16000, 64, 16, 64, 20, 0, 8000),
    "B80": (16000, 128, 50, 80, 16, None, None),      # window offset 24
    "B75": (16000, 128, 50, 75, 16, None, None),      # odd remainder: offset 26
    "lj": (22050, 1024, 256, 1024, 80, 80, 7600),
    "libritts": (24000, 2048, 300, 1200, 80, 80, 7600),
    "cli": (16000, 256, 3, 200, 80, 0, 8000),         # the preprocess -> decode test: hop 3, offset 28
    # dense caller-given matrices (fmin = "dense": see melmat_of): weight on bin 0 and on the Nyquist bin
    "D64": (16000, 64, 16, 64, 20, "dense", None),
    "D100": (16000, 100, 30, 70, 40, "dense", None),  # n_fft / 2 = 50: the last bin tile has a tail; two mel-row tiles
}


def samples_for(frames, hop, extra=5):
    """A length that gives `frames` frames: (frames - 1) hop + extra, extra < hop."""
    assert 0 <= extra < hop
    return (frames - 1) * hop + extra


# (geometry, T, spectral tilt in dB, seed): every non-silent input of the GPU tests
CASES = (
    [("A", 33, 20, 1)] + [("A", samples_for(f, 16), 10 * i, 2 + i) for i, f in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE + 3))]
    + [(g, samples_for(f, 50), t, 10 + i) for i, (g, f, t) in enumerate((("B80", 7, 30), ("B80", TILE + 2, 60), ("B75", 7, 0),
                                                                         ("B75", TILE + 2, 40)))]
    + [("lj", samples_for(12, 256, 100), 60, 20), ("libritts", 2700, 0, 21), ("libritts", 2700, 40, 22),
       ("libritts", 2700, 80, 23), ("libritts", 1025, 40, 24)]
    + [("B80", 65, 20, 30), ("B80", 50 * TILE + 7, 50, 31), ("B80", 333, 70, 32)]  # the ragged batch
    + [("B80", 777, 30, 50), ("cli", 400, 20, 60), ("cli", 1001, 40, 61), ("lj", 2304, 40, 70)]  # extractor, CLI, end to end
    + [("D64", 33, 10, 80), ("D64", samples_for(TILE + 1, 16), 40, 81), ("D100", 51, 0, 82),
       ("D100", samples_for(TILE + 3, 30), 30, 83)]  # dense matrices: the DC and Nyquist columns
)


def dense_melmat(num_mels, n_bins, seed=11):
    """A dense positive matrix as a caller may pass (a linear or HTK-style bank has weight on bin 0 and on
    the Nyquist bin, which Slaney banks never have): uniform in [0.002, 0.03], the two edge columns the
    largest of their rows so that a mistake there cannot hide."""
    w = np.random.RandomState(seed).uniform(0.002, 0.03, (num_mels, n_bins))
    w[:, 0] = 0.03 + 0.01 * np.arange(num_mels) / num_mels
    w[:, -1] = 0.04 - 0.01 * np.arange(num_mels) / num_mels
    return w.astype(np.float32)


def melmat_of(geometry):
    sr, n_fft, _, _, num_mels, fmin, fmax = GEOMETRIES[geometry]
    if fmin == "dense":
        return dense_melmat(num_mels, n_fft // 2 + 1)
    return slaney_mel_basis(sr, n_fft, num_mels, fmin, fmax)


def signal(T, sr, tilt_db, seed):
    """Seeded Gaussian noise whose spectrum falls by tilt_db towards Nyquist, plus the harmonics of
    150 Hz at the noise's level, scaled to peak 0.5 and rounded to PCM16 steps: every band holds
    signal, not only leakage (log-mel is ill-conditioned where a band is empty)."""
    rs = np.random.RandomState(seed)
    n = max(T, 256)
    spec = np.fft.rfft(rs.standard_normal(n))
    f = np.arange(len(spec)) / (len(spec) - 1)  # 0 .. 1 = Nyquist
    x = np.fft.irfft(spec * 10.0 ** (-tilt_db * f / 20.0), n)[:T]
    t = np.arange(T) / sr
    for h in range(1, int(sr / 2 / 150.0)):
        x = x + 10.0 ** (-tilt_db * (150.0 * h / (sr / 2)) / 20.0) * np.sin(2 * np.pi * 150.0 * h * t + rs.rand() * 6.28)
    x = 0.5 * x / np.abs(x).max()
    return (np.round(x * 32768.0) / 32768.0).astype(np.float32)


def case_signal(case):
    g, T, tilt, seed = case
    return signal(T, GEOMETRIES[g][0], tilt, seed)


def synthetic_stats(num_mels, seed=7):
    """(mean, scale) with scale in [0.5, 2]."""
    rs = np.random.RandomState(seed)
    return (rs.uniform(-6.0, -2.0, num_mels).astype(np.float32), rs.uniform(0.5, 2.0, num_mels).astype(np.float32))


def reference_fp32(x, n_fft, hop, win_length, melmat, eps=1e-10, amp_floor=True):
    """The reference's fp32 path on the CPU (losses/mel_loss.py:95-110): torch.stft with a periodic Hann
    window, power, optional clamp, sqrt, fp32 matmul, clamp, log10. (frames, num_mels) float32."""
    x = torch.from_numpy(np.asarray(x, np.float32)).reshape(1, -1)
    st = torch.stft(x, n_fft, hop, win_length, window=torch.hann_window(win_length), center=True, return_complex=True)
    power = (st.real ** 2 + st.imag ** 2).transpose(1, 2)
    if amp_floor:
        power = torch.clamp(power, min=eps)
    mel = torch.clamp(torch.matmul(torch.sqrt(power), torch.from_numpy(np.asarray(melmat, np.float32).T.copy())), min=eps)
    return torch.log10(mel)[0].numpy()


@functools.lru_cache(maxsize=1)
def reference_fp32_errors():
    """{case: max |reference fp32 - oracle| in log10} over CASES, in the MelSpectrogram form."""
    out = {}
    for case in CASES:
        _, n_fft, hop, win, *_ = GEOMETRIES[case[0]]
        x, mm = case_signal(case), melmat_of(case[0])
        want = orc.logmel(x, n_fft, hop, win, mm, amp_floor=True)
        out[case] = float(np.abs(reference_fp32(x, n_fft, hop, win, mm) - want).max())
    return out


def load_fixture(name):
    with np.load(os.path.join(LM_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def log_code(log_base):
    return 0.0 if log_base is None else float(log_base)


def run_raw(dev, waves, geometry, amp_floor, log_base=10.0, eps=1e-10, stats=None, melmat=None):
    """pwg_mel_run over the ragged batch `waves` (list of (T_u,) float32 arrays) in a geometry of
    GEOMETRIES (or a (n_fft, hop, win_length) triple with `melmat`): list of (frames_u, num_mels) arrays."""
    if isinstance(geometry, str):
        _, n_fft, hop, win, *_ = GEOMETRIES[geometry]
        melmat = melmat_of(geometry) if melmat is None else melmat
    else:
        n_fft, hop, win = geometry
    mean, scale = stats if stats is not None else (None, None)
    plan = MelPlan(dev, n_fft, win, hop, melmat, eps, log_code(log_base), amp_floor, mean, scale)
    packed = torch.from_numpy(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in waves])).to(dev)
    out = plan.run(packed, [len(w) for w in waves])
    torch.cuda.synchronize(dev)
    rows = np.cumsum([1 + len(w) // hop for w in waves])[:-1]
    return np.split(out.cpu().numpy(), rows)


# ------------------------------------------------------------------ raw C-ABI calls for the argument checks
P = ctypes.c_void_p(4096)  # a non-null, aligned pointer no check dereferences


def plan_create(L, n_fft=64, win=64, hop=16, window=0, num_mels=4, melmat=P, count=None, eps=1e-10, log_base=10.0,
                amp_floor=0, mean=None, scale=None, plan="byref"):
    """pwg_mel_plan_create with arguments that pass every check unless overridden; returns the status.
    Only calls that fail a check are made without a device: a passing call would allocate."""
    h = ctypes.c_void_p()
    count = num_mels * (n_fft // 2 + 1) if count is None else count
    return L.pwg_mel_plan_create(n_fft, win, hop, window, num_mels, melmat, count, eps, log_base, amp_floor, mean, scale,
                                 ctypes.byref(h) if plan == "byref" else plan)
