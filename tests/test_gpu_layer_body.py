"""The split16 residual-layer body (csrc/pwg_split16.hip s16_block and its three kernels) against
outputs RECORDED from the commit before its addressing / VALU trim, bit for bit: every accumulator
must still sum the same products in the same order and every converted value take the same
instruction sequence, so np.array_equal, not a tolerance. The fixtures under
tests/golden/layer_body/ hold only outputs (weights and inputs are seeded); a fixture maps every
option set of a case to one of its stored arrays (identical outputs are stored once).

Cases, the smallest that reach every path of the body:
  * LibriTTS v1 (30 layers, dilations 1 .. 512: tap shifts that are and are not multiples of 16),
    ragged T' = [9, 2, 5]: an utterance below Fmin (the small aux table), partial last blocks
    (9 * 300 and 5 * 300 are no multiples of 32) and gaps between utterances; with first_conv
    fused or not, whole or half blocks (NTN = 2 / 1), per-layer or grid-synchronised launches,
    and the layer pipeline;
  * the causal LibriTTS config (tap centre 2), T' = [6];
  * ljspeech_v1, T' = 7, through the drop-in inference().
Every option set of a case gives the same bits, and the engine redoes a synchronised or pipelined
run that did not complete on the per-layer launches, so each case also checks which launches made
its output: the residual-layer launch count of the forward (30 per-layer launches; the
synchronised launch plus the last layer, plus layer 0 on whole blocks with first_conv fused; one
pipelined launch) and that nothing was rerun.
GPU only; every forward goes through include/pwg.h."""

import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_body")
BIG = 1 << 30

# option sets: (fuse_first_conv, half_blocks, sync, pipeline)
SWEEP = [(f, h, s, 0) for f, h, s in itertools.product((1, 0), (0, BIG), (0, BIG))] + [(1, 0, 0, 1 << 24)]
ENGINE_CASES = {
    "libritts_ragged": dict(cfg="libritts_v1", over={}, lengths=[9, 2, 5], options=SWEEP + [None]),
    "libritts_causal": dict(cfg="libritts_v1", over={"use_causal_conv": True}, lengths=[6], options=[None]),
}
WEIGHT_SEED, INPUT_SEED = 0, 5


def option_key(opt):
    return "default" if opt is None else "fuse%d_half%d_sync%d_pipe%d" % tuple(int(bool(v)) for v in opt)


def expected_launches(opt, layers):
    """Residual-layer launches of one forward under an explicit option set."""
    fuse, half, sync, pipe = opt
    if pipe:
        return 1
    if sync:
        return 3 if fuse and not half else 2
    return layers


def run_engine_case(case, opt, dev):
    """The case's forward under one option set (None: the engine's defaults): (one flat array,
    residual-layer launches of the forward, reruns of any kind)."""
    from parallelwavegan_amd import Engine, configs, synthetic

    c = ENGINE_CASES[case]
    params = configs.generator_params(c["cfg"], **c["over"])
    eng = Engine(params, dev)
    eng.load_state_dict(synthetic.make_state_dict(params, seed=WEIGHT_SEED))
    if opt is not None:
        # "pipeline" first: it drops the cached plans
        for name, v in zip(("pipeline", "fuse_first_conv", "half_blocks", "sync"), (opt[3], opt[0], opt[1], opt[2])):
            eng.set_option(name, v)
    hop = eng.upsample_factor
    rs = np.random.RandomState(INPUT_SEED)
    mels = [torch.from_numpy(rs.standard_normal((f, 80)).astype(np.float32)).to(dev) for f in c["lengths"]]
    noises = [torch.from_numpy(rs.standard_normal((f * hop, 1)).astype(np.float32)).to(dev) for f in c["lengths"]]
    eng.set_timing(True)
    eng.collect_timing()
    y = np.concatenate([y.cpu().numpy().reshape(-1) for y in eng.infer(mels, noises)])
    launches = eng.collect_timing()["residual_layer"][1]
    eng.set_timing(False)
    return y, launches, eng.sync_reruns + eng.range_reruns


def run_dropin_case(dev):
    """ljspeech_v1, T' = 7, through the drop-in module's inference()."""
    from parallelwavegan_amd import ParallelWaveGANGenerator, configs, synthetic

    params = configs.generator_params("ljspeech_v1")
    m = ParallelWaveGANGenerator(**params)
    m.remove_weight_norm()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(params, seed=WEIGHT_SEED).items()})
    m = m.eval().to(dev)
    mel = synthetic.make_mel(7, 80, seed=1)
    noise = synthetic.make_noise(7 * 256, seed=2)
    with torch.no_grad():
        return m.inference(mel, noise).cpu().numpy().reshape(-1)


def _recorded(case, key):
    with np.load(os.path.join(FIXTURE_DIR, case + ".npz"), allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
        return z[meta["outputs"][key]]


@pytest.mark.parametrize("case, opt", [(case, opt) for case, c in ENGINE_CASES.items() for opt in c["options"]],
                         ids=lambda v: v if isinstance(v, str) else option_key(v))
def test_layer_body_bitwise_equal_to_recorded(case, opt, built_lib, cuda_device):
    got, launches, reruns = run_engine_case(case, opt, cuda_device)
    ref = _recorded(case, option_key(opt))
    print("%s %s: %d residual-layer launches, %d reruns" % (case, option_key(opt), launches, reruns))
    assert reruns == 0
    if opt is not None:
        from parallelwavegan_amd import configs

        c = ENGINE_CASES[case]
        assert launches == expected_launches(opt, configs.generator_params(c["cfg"], **c["over"])["layers"])
    assert np.isfinite(got).all()
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "%d of %d samples differ, max|d| = %.3e" % (
        int((got != ref).sum()), ref.size, float(np.abs(got - ref).max()))


def test_layer_body_dropin_inference_bitwise_equal_to_recorded(built_lib, cuda_device):
    got = run_dropin_case(cuda_device)
    ref = _recorded("ljspeech_dropin", "default")
    assert np.isfinite(got).all()
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "%d of %d samples differ, max|d| = %.3e" % (
        int((got != ref).sum()), ref.size, float(np.abs(got - ref).max()))
