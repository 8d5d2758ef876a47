"""Helpers shared by the token StyleMelGAN tests (tests/test_dsym_stylemelgan_host.py,
tests/test_gpu_dsym_stylemelgan.py): the fixtures of tests/golden/dsym_stylemelgan and the drop-in built
with a fixture's weights. Not a test module."""

import glob
import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from parallelwavegan_amd import configs, synthetic
from parallelwavegan_amd.engine import fold_weight_norm

DSMG_DIR = os.path.join(GOLDEN_DIR, "dsym_stylemelgan")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DSMG_DIR, "*.npz")))


def load_fixture(name):
    with np.load(os.path.join(DSMG_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def config_module(config, seed=0, gain=1.0):
    """(drop-in with seeded weights, params, folded state dict) of a configs.DSYM_STYLE_MELGAN_PARAMS entry."""
    from parallelwavegan_amd import DiscreteSymbolStyleMelGANGenerator

    params = configs.dsym_style_melgan_params(config)
    m = DiscreteSymbolStyleMelGANGenerator(**configs.dsym_style_melgan_params(config))
    sd = synthetic.make_module_state_dict(m, seed=seed, gain=gain)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval(), params, fold_weight_norm(sd)


def fixture_module(meta):
    return config_module(meta["config"], meta["weight_seed"], meta["gain"])


def utterances(fx):
    """Per utterance (ids (T, 2), z (Lz, in), y (T * hop, out)) of a fixture."""
    ids, z, y = fx["ids"], fx["z"], fx["y"]
    if fx["meta"]["mode"] == "inference":
        return [(ids, z[0].T, y)]
    return [(ids[b].T, z[b].T, y[b].T) for b in range(ids.shape[0])]
