"""Generate the log-mel fixtures in tests/golden/logmel/*.npz from the REFERENCE implementation
(parallel_wavegan/losses/mel_loss.py:MelSpectrogram).

Runs only where the reference is mounted; no test runs it. The reference is imported read-only; no
reference file is touched or copied. mel_loss.py imports librosa, which is absent: a stub module named
``librosa`` is installed whose ``filters.mel`` is parallelwavegan_amd.logmel.slaney_mel_basis (the
restatement of librosa's Slaney filter bank). So the STFT, the clamps, the matmul and the log in the
fixtures are the reference's own (torch on the CPU, fp32); only the mel basis is ours, and each
fixture's meta says so (``mel_basis``). bin/preprocess.py:logmelfilterbank needs librosa.stft and
cannot be run; tests/logmel_oracle.py covers it.

Per case: the signal of tests/logmel_helpers.py:signal (noise with a spectral tilt plus harmonics,
PCM16 steps) -> x (T,), melmat (num_mels, bins) as the module holds it, y (frames, num_mels) = the
module's output transposed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_logmel.py
"""

import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from logmel_helpers import GEOMETRIES, signal  # noqa: E402
from parallelwavegan_amd.logmel import slaney_mel_basis  # noqa: E402

REFERENCE = os.environ.get("PWG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "logmel")

# name, geometry, T, tilt (dB), seed, log_base
CASES = [
    ("lm_A_T33", "A", 33, 20, 101, 10.0),
    ("lm_A_T165_log2", "A", 165, 40, 102, 2.0),
    ("lm_B80_T320", "B80", 320, 30, 103, 10.0),
    ("lm_B75_T320_ln", "B75", 320, 10, 104, None),
    ("lm_lj_T2916", "lj", 2916, 60, 105, 10.0),
    ("lm_libritts_T2700", "libritts", 2700, 40, 106, 10.0),
    ("lm_libritts_T1025", "libritts", 1025, 80, 107, 10.0),
]


def import_reference():
    def mel(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
        return slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax)

    librosa = types.ModuleType("librosa")
    librosa.filters = types.ModuleType("librosa.filters")
    librosa.filters.mel = mel
    sys.modules["librosa"] = librosa
    sys.modules["librosa.filters"] = librosa.filters
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "ref_mel_loss", os.path.join(REFERENCE, "parallel_wavegan", "losses", "mel_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MelSpectrogram


def main():
    warnings.simplefilter("ignore")
    RefMel = import_reference()
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    for name, g, T, tilt, seed, log_base in CASES:
        sr, n_fft, hop, win, num_mels, fmin, fmax = GEOMETRIES[g]
        x = signal(T, sr, tilt, seed)
        m = RefMel(fs=sr, fft_size=n_fft, hop_size=hop, win_length=win, num_mels=num_mels, fmin=fmin, fmax=fmax,
                   log_base=log_base)
        with torch.no_grad():
            y3 = m(torch.from_numpy(x).reshape(1, 1, -1))
            y2 = m(torch.from_numpy(x).reshape(1, -1))
        assert torch.equal(y3, y2) and tuple(y3.shape) == (1, num_mels, 1 + T // hop)
        meta = dict(name=name, geometry=g, fs=sr, fft_size=n_fft, hop_size=hop, win_length=win, num_mels=num_mels,
                    fmin=fmin, fmax=fmax, log_base=log_base, eps=1e-10, tilt_db=tilt, seed=seed,
                    mel_basis="parallelwavegan_amd.logmel.slaney_mel_basis (librosa is absent; everything else is the "
                              "reference's MelSpectrogram on the CPU)", torch=torch.__version__)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), x=x, melmat=m.melmat.numpy().T.copy(),
                            y=y3[0].numpy().T.copy(), meta=np.array(json.dumps(meta)))
        print(f"{name}: x {x.shape} y {tuple(y3[0].T.shape)} range [{float(y3.min()):.2f}, {float(y3.max()):.2f}]")


if __name__ == "__main__":
    main()
