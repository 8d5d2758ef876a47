"""PWG_OPT_SKIP_AHEAD ("skip_ahead"): the split16 per-layer kernels that request a block's old skip
sums before the center tap's MFMAs, against the kernels that request them after GEMM 1. The loads
only move: the seeds enter the same accumulators before the same MFMAs, so option 1 and option 0
are compared with np.array_equal.

Setup: the 30-layer LibriTTS v1 generator with seeded weights; "sync", "pipeline" and "half_blocks"
at 0, so that these small plans run 30 whole-block per-layer launches (asserted). Thirty layers
cover dilations under 16 (the generic kernel) and from 16 on (AL), layer 0's summed-bias seeds
(skip0, the other side of the one branch on `first`) and the last-layer kernel with the head.
Shapes, the smallest that reach each path:
  * T' = [1]: 300 samples, ten blocks, the last one partial;
  * T' = [2, 5] ragged: the gap between utterances, blocks that span two frames; with first_conv
    fused into layer 0 and as its own kernel;
  * the causal configuration (tap center 2);
  * "half_blocks" on: the 16-column work units (NTN = 1) of every layer but the last."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 1 << 30
WEIGHT_SEED, INPUT_SEED = 0, 7
LAYERS = 30


def forward(lengths, over, fuse, half, ahead, dev):
    """(flat output, residual-layer launches, of them in the read-ahead form, reruns)"""
    from parallelwavegan_amd import Engine, configs, synthetic

    params = configs.generator_params("libritts_v1", **over)
    assert params["layers"] == LAYERS
    eng = Engine(params, dev)
    eng.load_state_dict(synthetic.make_state_dict(params, seed=WEIGHT_SEED))
    assert eng.get_option("skip_ahead") == 1  # the default
    # "pipeline" first: it drops the cached plans
    for name, v in (("pipeline", 0), ("sync", 0), ("half_blocks", half), ("fuse_first_conv", fuse)):
        eng.set_option(name, v)
    eng.set_option("skip_ahead", ahead)
    assert eng.get_option("skip_ahead") == ahead
    assert eng.get_option("fragment_ahead") == 1
    hop = eng.upsample_factor
    rs = np.random.RandomState(INPUT_SEED)
    mels = [torch.from_numpy(rs.standard_normal((f, 80)).astype(np.float32)).to(dev) for f in lengths]
    noises = [torch.from_numpy(rs.standard_normal((f * hop, 1)).astype(np.float32)).to(dev) for f in lengths]
    eng.set_timing(True)
    eng.collect_timing()
    y = np.concatenate([y.cpu().numpy().reshape(-1) for y in eng.infer(mels, noises)])
    launches = eng.collect_timing()["residual_layer"][1]
    eng.set_timing(False)
    return y, launches, eng.fragment_ahead_launches(), eng.sync_reruns + eng.range_reruns


@pytest.mark.parametrize("lengths, over, fuse, half", [
    ([1], {}, 1, 0),
    ([2, 5], {}, 1, 0),
    ([2, 5], {}, 0, 0),
    ([2, 5], {"use_causal_conv": True}, 1, 0),
    ([2, 5], {}, 1, BIG),
], ids=["one_frame", "ragged", "ragged_unfused", "causal", "half_blocks"])
def test_skip_ahead_equals_option_off(lengths, over, fuse, half, built_lib, cuda_device):
    outs = []
    for ahead in (0, 1):
        y, launches, fa, reruns = forward(lengths, over, fuse, half, ahead, cuda_device)
        print("T'=%s %s fuse=%d half=%d skip_ahead=%d: %d residual-layer launches, %d read-ahead, %d reruns"
              % (lengths, over, fuse, int(bool(half)), ahead, launches, fa, reruns))
        assert reruns == 0
        assert (launches, fa) == (LAYERS, LAYERS)  # per-layer launches only, all in the form the option acts on
        assert y.size == 300 * sum(lengths)
        assert np.isfinite(y).all()
        outs.append(y)
    ref, got = outs
    assert np.abs(ref).max() > 0
    assert np.array_equal(got, ref), "skip_ahead=1: %d of %d samples differ, max|d| = %.3e" % (
        int((got != ref).sum()), ref.size, float(np.abs(got - ref).max()))
