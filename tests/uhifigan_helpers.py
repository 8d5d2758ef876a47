"""Helpers shared by the UHiFiGAN tests (tests/test_uhifigan_host.py, tests/test_gpu_uhifigan.py): the
fixtures of tests/golden/uhifigan and the drop-in built with a fixture's weights. Not a test module."""

import glob
import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from parallelwavegan_amd import configs, synthetic
from parallelwavegan_amd.cnet import PwgCnetOp, PwgCnetSrc
from parallelwavegan_amd.engine import fold_weight_norm

UHG_DIR = os.path.join(GOLDEN_DIR, "uhifigan")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(UHG_DIR, "*.npz")))


def load_fixture(name):
    with np.load(os.path.join(UHG_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def fixture_module(meta, weight_norm=True):
    """(drop-in with the fixture's weights, params, folded state dict)."""
    from parallelwavegan_amd import UHiFiGANGenerator

    params = configs.uhifigan_params(meta["config"])
    m = UHiFiGANGenerator(**configs.uhifigan_params(meta["config"]))
    sd = synthetic.make_module_state_dict(m, seed=meta["weight_seed"], gain=meta["gain"])
    folded = fold_weight_norm(sd)
    if weight_norm:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    else:
        m.remove_weight_norm()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in folded.items()}, strict=True)
    return m.eval(), params, folded


def utterances(fx):
    """Per utterance (c (T, in), excitation (T * hop,), y (T * hop, 1)) of a fixture."""
    c, e, y = fx["c"], fx["excitation"], fx["y"]
    if fx["meta"]["mode"] == "inference":
        return [(c, e, y)]
    return [(c[b].T, e[b, 0], y[b].T) for b in range(c.shape[0])]


def dump_program(P):
    """Every PwgCnetOp / PwgCnetSrc field of ``P.c_ops()`` with the buffers, op names and weight
    layout, as JSON-able data (the format of tests/golden/uhifigan/hifigan_programs.json)."""
    ops = []
    for c in P.c_ops():
        d = {f: getattr(c, f) for f, _ in PwgCnetOp._fields_ if f != "src"}
        srcs = [{f: getattr(c.src[j], f) for f, _ in PwgCnetSrc._fields_} for j in range(2)]
        d["src"] = [s if s["buf"] >= 0 else {"buf": -1} for s in srcs]
        ops.append(d)
    return dict(channels=list(P.channels), rate=list(P.rate), names=list(P.names),
                weights=[list(kv) for kv in P.weights.items()], ops=ops)
