"""Helpers shared by the StyleMelGAN tests (tests/test_stylemelgan_host.py, tests/test_gpu_stylemelgan.py):
the fixtures of tests/golden/stylemelgan and the drop-in built with a fixture's weights. Not a test
module."""

import glob
import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from parallelwavegan_amd import configs, synthetic
from parallelwavegan_amd.engine import fold_weight_norm

SMG_DIR = os.path.join(GOLDEN_DIR, "stylemelgan")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SMG_DIR, "*.npz")))


def load_fixture(name):
    with np.load(os.path.join(SMG_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def fixture_module(meta):
    """(drop-in with the fixture's weights, params, folded state dict)."""
    from parallelwavegan_amd import StyleMelGANGenerator

    params = configs.style_melgan_params(meta["config"])
    m = StyleMelGANGenerator(**configs.style_melgan_params(meta["config"]))
    sd = synthetic.make_module_state_dict(m, seed=meta["weight_seed"], gain=meta["gain"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval(), params, fold_weight_norm(sd)


def utterances(fx):
    """Per utterance (c (T, aux), z (Lz, in), y (T * hop, out)) of a fixture."""
    c, z, y = fx["c"], fx["z"], fx["y"]
    if fx["meta"]["mode"] == "inference":
        return [(c, z[0].T, y)]
    return [(c[b].T, z[b].T, y[b].T) for b in range(c.shape[0])]
