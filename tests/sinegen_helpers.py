"""Helpers shared by the SineGen tests (tests/test_sinegen_host.py, tests/test_gpu_sinegen.py): the
fixtures of tests/golden/sinegen, f0 contours, and raw calls of the two C-ABI entry points over ragged
batches. Not a test module."""

import glob
import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from parallelwavegan_amd import _lib, sinegen

SG_DIR = os.path.join(GOLDEN_DIR, "sinegen")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SG_DIR, "sg_[th]*.npz")))
E2E = "sg_e2e_noadd_T9"
BLOCK = _lib.PWG_SINE_SCAN_BLOCK


def load_fixture(name):
    with np.load(os.path.join(SG_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def gen_args(meta):
    """(sr, dim, sine_amp, noise_std, voiced_threshold) of a fixture."""
    return (meta["samp_rate"], meta["harmonic_num"] + 1, meta["sine_amp"], meta["noise_std"], meta["voiced_threshold"])


def contour(n, seed, lo=70.0, hi=900.0, unvoiced=0.2):
    """n values of f0 that glide between lo and hi, with unvoiced (0) stretches; the first is voiced."""
    rs = np.random.RandomState(seed)
    f = np.clip(np.abs(lo + (hi - lo) * rs.rand() + np.cumsum(rs.standard_normal(n)) * 0.02 * (hi - lo)), lo, hi)
    gate = np.repeat(rs.rand(n // 16 + 1) < unvoiced, 16)[:n]
    f[gate] = 0.0
    f[0] = f[0] or 220.0
    return f.astype(np.float32)


def _pack(dev, arrays, shape_tail=()):
    if arrays is None:
        return None
    flat = np.concatenate([np.asarray(a, np.float32).reshape((-1,) + shape_tail) for a in arrays])
    return torch.from_numpy(np.ascontiguousarray(flat)).to(dev)


def _starts(lengths, dev):
    s = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=s[1:])
    return torch.from_numpy(s).to(dev), int(s[-1])


def _call(entry, dev, f0s, lengths, rows, extra, args, inis, ns, with_uv_noise=True, starts=None):
    """``starts``: the n_utts + 1 boundaries handed to the kernel instead of the true ones."""
    sr, dim, amp, nstd, thr = args
    true_starts, items = _starts(lengths, dev)
    starts = true_starts if starts is None else torch.tensor(starts, dtype=torch.int64, device=dev)
    sine = torch.full((rows, dim), np.nan, device=dev)
    uv = torch.full((rows,), np.nan, device=dev) if with_uv_noise else None
    noise = torch.full((rows, dim), np.nan, device=dev) if with_uv_noise else None
    flag = sinegen.sine_call(entry, dev, _pack(dev, f0s), starts, len(lengths), items, extra, float(sr), dim, amp, nstd,
                             thr, _pack(dev, inis, (dim,)), _pack(dev, ns, (dim,)), sine, uv, noise)
    torch.cuda.synchronize(dev)
    out = dict(sine=sine.cpu().numpy(), flag=int(flag.item()))
    if with_uv_noise:
        out.update(uv=uv.cpu().numpy(), noise=noise.cpu().numpy())
    return out


def run_samples(dev, f0s, args, inis=None, ns=None, **kw):
    """pwg_sine_samples over the ragged batch of sample-rate contours ``f0s`` (list of (N_u,))."""
    lengths = [len(f) for f in f0s]
    return _call("pwg_sine_samples", dev, f0s, lengths, sum(lengths), (), args, inis, ns, **kw)


def run_frames(dev, f0s, hop, layout, args, inis=None, ns=None, **kw):
    """pwg_sine_frames over the ragged batch of frame-rate contours ``f0s`` (list of (T_u,))."""
    lengths = [len(f) for f in f0s]
    return _call("pwg_sine_frames", dev, f0s, lengths, sum(lengths) * hop, (hop, _lib.PWG_SINE_LAYOUTS[layout]), args,
                 inis, ns, **kw)
