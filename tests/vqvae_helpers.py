"""Helpers shared by the VQVAE tests (tests/test_vqvae_host.py, tests/test_gpu_vqvae.py,
tests/test_gpu_vqvae_cli.py): the fixtures of tests/golden/vqvae and the drop-in built with a fixture's
weights. Not a test module."""

import glob
import json
import os

import numpy as np
import torch

import vqvae_oracle
from conftest import GOLDEN_DIR
from parallelwavegan_amd import configs, synthetic
from parallelwavegan_amd.engine import fold_weight_norm

VQ_DIR = os.path.join(GOLDEN_DIR, "vqvae")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(VQ_DIR, "*.npz")))
EXPECTED = ("vq_a_T200", "vq_a_T61", "vq_a_T8", "vq_a_dup", "vq_a_fwd_B3_T64", "vq_b_T131", "vq_b_T9",
            "vq_v3_fwd_B1_T256")
WITH_Y = tuple(n for n in EXPECTED if n not in ("vq_a_T8", "vq_b_T9"))  # the reference's decoder needs 4 frames


def load_fixture(name):
    with np.load(os.path.join(VQ_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def fixture_state(meta, module=None):
    """The fixture's weight-norm state dict (numpy), its codebook placed as the maker placed it."""
    from parallelwavegan_amd import VQVAE

    m = module if module is not None else VQVAE(**configs.vqvae_params(meta["config"]))
    sd = synthetic.make_module_state_dict(m, seed=meta["weight_seed"], gain=meta["gain"])
    sd["codebook.embedding.weight"] = vqvae_oracle.fixture_codebook(
        sd["codebook.embedding.weight"], meta["code_scale"], vqvae_oracle.codebook_shift(sd), meta["dup"], meta["dup_swap"])
    return sd


_MODULES = {}


def fixture_module(meta, weight_norm=True):
    """(drop-in with the fixture's weights, params, folded state dict); cached per weight set."""
    from parallelwavegan_amd import VQVAE

    key = (meta["config"], meta["weight_seed"], meta["gain"], meta["code_scale"], str(meta["dup"]), meta["dup_swap"],
           weight_norm)
    if key not in _MODULES:
        m = VQVAE(**configs.vqvae_params(meta["config"]))
        sd = fixture_state(meta, m)
        folded = fold_weight_norm(sd)
        if weight_norm:
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        else:
            m.remove_weight_norm()
            m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in folded.items()}, strict=True)
        _MODULES[key] = (m.eval(), configs.vqvae_params(meta["config"]), folded)
    return _MODULES[key]


def utterances(fx):
    """Per utterance (x (T,), l (T', num_local) or None, g int or None, z_e (T', D), idx (T',), y (T' * hop, 1)
    or None) of a fixture."""
    out = []
    for b in range(fx["x"].shape[0]):
        l = fx["l"][b].T if fx["l"].size else None
        g = int(fx["g"][b]) if fx["g"].size else None
        y = fx["y"][b].T if fx["meta"]["has_y"] else None
        out.append((fx["x"][b, 0], l, g, fx["z_e"][b].T, fx["idx"][b], y))
    return out
