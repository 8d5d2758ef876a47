"""PWG_OPT_FRAGMENT_AHEAD ("fragment_ahead"): the split16 per-layer kernels that read each MFMA
step's weight fragments from LDS one step ahead, with explicit counted waits, against the kernels
that leave those reads to the compiler. Both forms issue the same MFMAs in the same order per
accumulator, so the outputs are compared with np.array_equal, to each other and to the arrays
recorded in tests/golden/layer_body/ (read only; recorded before either change to the body).

Shapes, the smallest that reach every path of the block body (the fixture's own):
  * LibriTTS v1, ragged T' = [9, 2, 5]: dilations 1 .. 512 (tap shifts that are and are not
    multiples of 16, so both the AL and the generic kernel), an utterance below Fmin, partial last
    blocks, gaps; whole and half blocks, first_conv fused or not;
  * the causal config, T' = [6]: tap centre 2.
Each forward also reports which launches made it: the residual-layer launch count, the reruns, and
how many of the launches took the read-ahead form (Engine.fragment_ahead_launches)."""

import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_body")
BIG = 1 << 30
CASES = {
    "libritts_ragged": dict(cfg="libritts_v1", over={}, lengths=[9, 2, 5]),
    "libritts_causal": dict(cfg="libritts_v1", over={"use_causal_conv": True}, lengths=[6]),
}
WEIGHT_SEED, INPUT_SEED = 0, 5
LAYERS = 30


def option_key(opt):
    return "default" if opt is None else "fuse%d_half%d_sync%d_pipe%d" % tuple(int(bool(v)) for v in opt)


@functools.lru_cache(maxsize=None)
def recorded(case, key):
    with np.load(os.path.join(FIXTURE_DIR, case + ".npz"), allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
        ref = z[meta["outputs"][key]]
    ref.setflags(write=False)
    return ref


def forward(case, opt, ahead, dev):
    """One forward of the case under (fuse_first_conv, half_blocks, sync, pipeline) (None: the
    engine's defaults) with the switch at `ahead`: (flat output, residual-layer launches, reruns,
    launches in the read-ahead form)."""
    from parallelwavegan_amd import Engine, configs, synthetic

    c = CASES[case]
    params = configs.generator_params(c["cfg"], **c["over"])
    assert params["layers"] == LAYERS
    eng = Engine(params, dev)
    eng.load_state_dict(synthetic.make_state_dict(params, seed=WEIGHT_SEED))
    assert eng.get_option("fragment_ahead") == 1  # the default
    if opt is not None:
        # "pipeline" first: it drops the cached plans
        for name, v in zip(("pipeline", "fuse_first_conv", "half_blocks", "sync"), (opt[3], opt[0], opt[1], opt[2])):
            eng.set_option(name, v)
    eng.set_option("fragment_ahead", ahead)
    assert eng.get_option("fragment_ahead") == ahead
    hop = eng.upsample_factor
    rs = np.random.RandomState(INPUT_SEED)
    mels = [torch.from_numpy(rs.standard_normal((f, 80)).astype(np.float32)).to(dev) for f in c["lengths"]]
    noises = [torch.from_numpy(rs.standard_normal((f * hop, 1)).astype(np.float32)).to(dev) for f in c["lengths"]]
    eng.set_timing(True)
    eng.collect_timing()
    y = np.concatenate([y.cpu().numpy().reshape(-1) for y in eng.infer(mels, noises)])
    launches = eng.collect_timing()["residual_layer"][1]
    eng.set_timing(False)
    return y, launches, eng.sync_reruns + eng.range_reruns, eng.fragment_ahead_launches()


def both_forms(case, opt, key, dev):
    """The forward with the switch on and off: both equal the recorded array of `key`, bit for bit.
    Returns ((launches, read-ahead launches) on, (launches, read-ahead launches) off)."""
    ref = recorded(case, key)
    counts = []
    outs = []
    for ahead in (1, 0):
        got, launches, reruns, fa = forward(case, opt, ahead, dev)
        print("%s %s fragment_ahead=%d: %d residual-layer launches, %d in the read-ahead form, %d reruns"
              % (case, option_key(opt), ahead, launches, fa, reruns))
        assert reruns == 0
        assert np.isfinite(got).all()
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), "fragment_ahead=%d: %d of %d samples differ, max|d| = %.3e" % (
            ahead, int((got != ref).sum()), ref.size, float(np.abs(got - ref).max()))
        outs.append(got)
        counts.append((launches, fa))
    assert np.array_equal(outs[0], outs[1])
    return counts


@pytest.mark.parametrize("fuse, half", [(1, 0), (1, BIG), (0, 0), (0, BIG)],
                         ids=["fused_whole", "fused_half", "unfused_whole", "unfused_half"])
def test_ragged_per_layer_launches_both_forms_equal_recorded(fuse, half, built_lib, cuda_device):
    opt = (fuse, half, 0, 0)
    on, off = both_forms("libritts_ragged", opt, option_key(opt), cuda_device)
    assert on == (LAYERS, LAYERS)  # every per-layer kernel has the read-ahead form
    assert off == (LAYERS, 0)


@pytest.mark.parametrize("opt", [None, (1, 0, 0, 0), (1, BIG, 0, 0)], ids=["default", "whole", "half"])
def test_causal_both_forms_equal_recorded(opt, built_lib, cuda_device):
    """Tap centre 2. The engine's defaults put this plan on the grid-synchronised launch, where only
    the launches outside it (the last layer, layer 0 on whole blocks) have the read-ahead form; the
    two per-layer option sets run all 30 launches in it. Every option set of the case gives the bits
    recorded under "default"."""
    on, off = both_forms("libritts_causal", opt, "default", cuda_device)
    assert off[1] == 0
    if opt is None:
        assert 1 <= on[1] <= on[0]
    else:
        assert on == (LAYERS, LAYERS) and off[0] == LAYERS


@pytest.mark.parametrize("opt, launches, ahead", [((1, 0, BIG, 0), 3, 2), ((1, BIG, BIG, 0), 2, 1),
                                                  ((1, 0, 0, 1 << 24), 1, 0)],
                         ids=["sync_whole", "sync_half", "pipeline"])
def test_synchronised_and_pipelined_launches_keep_their_form(opt, launches, ahead, built_lib, cuda_device):
    """The grid-synchronised and the pipelined kernel have one form: with the switch on, only the
    per-layer launches beside them (the last layer; layer 0 with the fused first_conv on whole
    blocks) take the read-ahead kernels, and the output is the recorded one either way."""
    on, off = both_forms("libritts_ragged", opt, option_key(opt), cuda_device)
    assert on == (launches, ahead)
    assert off == (launches, 0)
