"""StyleMelGANGenerator drop-in, host side (no GPU): state-dict keys against the reference's (recorded
in the fixtures), weight counts, refusals, plan checks, the packing range check, and the float64
oracle (tests/stylemelgan_oracle.py) against every fixture."""

import ctypes

import numpy as np
import pytest

from parallelwavegan_amd import _lib, configs, synthetic
from parallelwavegan_amd.engine import fold_weight_norm
from stylemelgan_helpers import FIXTURES, fixture_module, load_fixture, utterances
from stylemelgan_oracle import Oracle

def test_fixture_set():
    assert len(FIXTURES) == 7
    for name in FIXTURES:
        assert load_fixture(name)["meta"]["e_ref"] < 1e-5


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_match_reference(built_lib, name):
    meta = load_fixture(name)["meta"]
    m, _, _ = fixture_module(meta)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["keys"]
    h = m.host_handle()
    # the reference order holds the folded weights: every tensor but the weight-norm gains
    assert h.ref_weight_count == sum(int(np.prod(s)) for k, s in meta["keys"] if not k.endswith("weight_g"))
    m.remove_weight_norm()
    assert h.ref_weight_count == sum(p.numel() for p in m.parameters())


def test_public_surface(built_lib):
    import parallelwavegan_amd

    m = parallelwavegan_amd.StyleMelGANGenerator()
    assert m.in_channels == 128 and int(m.upsample_factor) == 256 and int(m.noise_upsample_factor) == 88
    assert any(k.endswith("weight_g") for k in m.state_dict())
    assert "style_melgan_v1" not in configs.VOCODER_PARAMS
    assert configs.style_melgan_params("style_melgan_v1")["upsample_scales"] == [2, 2, 2, 2, 2, 2, 2, 2, 1]
    for name in ("apply_weight_norm", "remove_weight_norm", "reset_parameters", "register_stats", "inference_batch"):
        assert callable(getattr(m, name))


@pytest.mark.parametrize("override, exc", [
    (dict(upsample_mode="linear"), NotImplementedError),
    (dict(noise_upsample_activation="ReLU", noise_upsample_activation_params={}), NotImplementedError),
    (dict(channels=40), NotImplementedError),
    (dict(channels=128), NotImplementedError),
    (dict(aux_channels=144), NotImplementedError),
    (dict(kernel_size=8), NotImplementedError),
    (dict(kernel_size=13), NotImplementedError),
    (dict(gated_function="relu"), ValueError),
])
def test_refusals(built_lib, override, exc):
    from parallelwavegan_amd import StyleMelGANGenerator

    with pytest.raises(exc):
        StyleMelGANGenerator(**configs.style_melgan_params("style_melgan_test", **override))


def test_cpu_module_raises_runtime_error(built_lib):
    from parallelwavegan_amd import StyleMelGANGenerator

    m = StyleMelGANGenerator(**configs.style_melgan_params("style_melgan_test"))
    with pytest.raises(RuntimeError):
        m.inference(np.zeros((3, 80), np.float32))


def test_c_abi_refuses_what_the_class_refuses(built_lib):
    from parallelwavegan_amd.stylemelgan import make_smg_config

    h = ctypes.c_void_p()
    for over in (dict(channels=40), dict(aux_channels=144), dict(kernel_size=8), dict(kernel_size=13)):
        a = dict(in_channels=32, aux_channels=80, channels=64, out_channels=1, kernel_size=9, dilation=2, bias=True,
                 noise_upsample_scales=[4, 2], noise_slope=0.2, upsample_scales=[2, 1], gated_function="softmax")
        a.update(over)
        cfg = make_smg_config(**a)
        assert built_lib.pwg_smg_create(ctypes.byref(cfg), -1, ctypes.byref(h)) == _lib.PWG_ERR_UNSUPPORTED, over


def test_plan_checks(built_lib):
    from parallelwavegan_amd import StyleMelGANGenerator

    m = StyleMelGANGenerator(**configs.style_melgan_params("style_melgan_test"))
    h = m.host_handle()
    p = h.plan([3, 40, 19], [1, 5, 3])
    assert p.out_rows == (3 + 40 + 19) * 8
    assert p.workspace_bytes > 0 and p.workspace_bytes % 256 == 0
    off, rows, ld = p.tensor(0, _lib.PWG_SMG_X_IN)
    assert rows == (1 + 5 + 3) * 8 and ld == 64 and off % 256 == 0
    off2, rows2, _ = p.tensor(3, _lib.PWG_SMG_X_OUT)
    assert rows2 == rows * 8 and off2 + rows2 * 64 * 4 <= p.workspace_bytes
    assert p.tensor(2, _lib.PWG_SMG_STATS_MID)[1:] == (3, 128)
    with pytest.raises(ValueError):
        p.tensor(4, _lib.PWG_SMG_X_IN)
    with pytest.raises(ValueError):
        h.plan([9], [1])  # 1 * 8 rows do not cover 9 frames
    with pytest.raises(ValueError):
        h.plan([0], [1])
    with pytest.raises(ValueError):
        h.plan([], [])


def test_pack_range_check(built_lib):
    from parallelwavegan_amd import StyleMelGANGenerator

    m = StyleMelGANGenerator(**configs.style_melgan_params("style_melgan_odd_test"))
    sd = synthetic.make_module_state_dict(m, seed=0)
    h = m.host_handle()
    packed = h.pack(sd)
    assert packed.shape == (h.packed_weight_count,) and np.isfinite(packed).all()
    folded = fold_weight_norm(sd)
    folded["blocks.1.gated_conv1.weight"][3, 2, 1] = 7e4
    with pytest.raises(_lib.RangeError):
        h.pack(folded)


def test_pack_fragment_order(built_lib):
    """One conv's fragments, restated: step s, m-tile m, lane l holds row 16 m + (l & 15), chunk
    q = 2 s + (l >> 5) = tap * cs + cb, channels 16 cb + 8 ((l >> 4) & 1) + j, as hi then lo halves."""
    from parallelwavegan_amd import StyleMelGANGenerator

    m = StyleMelGANGenerator(**configs.style_melgan_params("style_melgan_odd_nobias_test"))
    sd = synthetic.make_module_state_dict(m, seed=0)
    h = m.host_handle()
    packed = h.pack(sd)
    w = fold_weight_norm(sd)["blocks.0.tade1.aux_conv.0.weight"]  # (32, 16, 5): cs = 1, 5 chunks, 3 steps
    cout, cin, K = w.shape
    cs, mt = cin // 16, cout // 16
    nsteps = (K * cs + 1) // 2
    frag = np.zeros((nsteps, mt, 2, 64, 8), np.float16)
    for s in range(nsteps):
        for mi in range(mt):
            for lane in range(64):
                q = 2 * s + (lane >> 5)
                if q >= K * cs:
                    continue
                tap, cb = divmod(q, cs)
                v = w[16 * mi + (lane & 15), 16 * cb + 8 * ((lane >> 4) & 1):][:8, tap]
                hi = v.astype(np.float16)
                frag[s, mi, 0, lane] = hi
                frag[s, mi, 1, lane] = (v - hi.astype(np.float32)).astype(np.float16)
    want = frag.reshape(-1).view(np.float32)
    # the noise stages come first in the image: [2 s][cin][cout] + bias slot, each padded to 64 floats
    off = sum((2 * s * ci * 32 + 63) // 64 * 64 + 64 for s, ci in zip((3, 2), (32, 32)))
    assert np.array_equal(packed[off:off + want.size].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_fixture(name):
    fx = load_fixture(name)
    _, params, folded = fixture_module(fx["meta"])
    orc = Oracle(folded, params)
    for c, z, y in utterances(fx):
        got = orc(c, z).numpy()
        assert got.shape == y.shape
        err = np.abs(got - y).max()
        print(f"{name}: oracle vs fixture {err:.2e}")
        assert err < 1e-5
