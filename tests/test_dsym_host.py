"""DiscreteSymbolHiFiGANGenerator (parallelwavegan_amd/dsym.py) without a GPU: checkpoint loading,
state-dict layout, the lowered program, the shared HiFiGAN lowering, refusals, host-side id checks,
the argument checks of pwg_embed_rows, and the oracle against the reference fixtures."""

import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN_DIR
from parallelwavegan_amd import DiscreteSymbolHiFiGANGenerator, _lib, configs, synthetic
from parallelwavegan_amd.cnet import CnetEngine, PwgCnetOp, PwgCnetSrc
from parallelwavegan_amd.engine import fold_weight_norm
from parallelwavegan_amd.hifigan import HiFiGANGenerator
from parallelwavegan_amd.utils import load_model

DSYM_DIR = os.path.join(GOLDEN_DIR, "dsym")
DSYM_CONFIGS = ["dsym_hifigan_test", "dsym_hifigan_nospk_test", "dsym_hifigan_feats_test", "dsym_hubert_v1",
                "dsym_token_v1"]
DSYM_GOLDEN = ["dsym_hifigan_test_T9", "dsym_hifigan_test_g_T6", "dsym_hifigan_test_fwd_B3_T5",
               "dsym_hifigan_nospk_T7", "dsym_hifigan_feats_T5", "dsym_hubert_v1_T2", "dsym_token_v1_T2"]


def load_dsym_golden(name):
    with np.load(os.path.join(DSYM_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def dsym_module(cfg, seed=0):
    """(drop-in with seeded weights loaded, params, weight-norm-folded state dict)."""
    _, params = configs.vocoder_params(cfg)
    m = DiscreteSymbolHiFiGANGenerator(**configs.vocoder_params(cfg)[1])
    sd = synthetic.make_module_state_dict(m, seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval(), params, fold_weight_norm(sd)


def oracle_features(ids, g, folded):
    """emb[ids] (+ spk_emb[g]) in fp32, (in_channels, T)."""
    f = np.asarray(folded["emb.weight"], np.float32)[ids]
    if g is not None:
        f = f + np.asarray(folded["spk_emb.weight"], np.float32)[g]
    return f.T


def oracle_golden(g, folded, params):
    """The fixture's output from the embedding lookup followed by oracle.melgan_numpy.hifigan_forward."""
    from oracle import melgan_numpy

    c, meta = g["c"], g["meta"]
    if params.get("use_embedding_feats") and params["num_spk_embs"] <= 0:
        return melgan_numpy.hifigan_forward(c.T, folded, params).T
    if meta["mode"] == "forward":
        return np.stack([melgan_numpy.hifigan_forward(oracle_features(c[b, 0], int(c[b, 1, 0]), folded), folded, params)
                         for b in range(c.shape[0])])
    spk = meta["options"].get("g")
    if spk is None and params["num_spk_embs"] > 0:
        spk = int(c[0, 1])
    return melgan_numpy.hifigan_forward(oracle_features(c[:, 0], spk, folded), folded, params).T


def test_every_fixture_is_listed():
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DSYM_DIR, "*.npz"))) == sorted(DSYM_GOLDEN)


def test_load_model_returns_dropin(tmp_path):
    """A checkpoint + config.yml of generator_type DiscreteSymbolHiFiGANGenerator loads (it raised
    NotImplementedError before this generator was supported)."""
    _, params = configs.vocoder_params("dsym_hifigan_test")
    m, _, _ = dsym_module("dsym_hifigan_test", seed=4)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    ckpt = str(tmp_path / "checkpoint-10steps.pkl")
    torch.save({"model": {"generator": state}, "steps": 10}, ckpt)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(dict(generator_type="DiscreteSymbolHiFiGANGenerator", generator_params=params,
                            sampling_rate=16000, format="npy", version="0.6.1"), f)
    got = load_model(ckpt)
    assert isinstance(got, DiscreteSymbolHiFiGANGenerator)
    sd = got.state_dict()
    assert list(sd) == list(state)
    for k, v in state.items():
        assert torch.equal(sd[k], v), k
    assert not hasattr(got, "mean") and getattr(got, "pqmf", None) is None
    assert got.upsample_factor == 8


@pytest.mark.parametrize("name", DSYM_GOLDEN)
def test_state_dict_matches_reference_keys(name):
    meta = load_dsym_golden(name)["meta"]
    m = DiscreteSymbolHiFiGANGenerator(**configs.vocoder_params(meta["vocoder"])[1])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["keys"]
    m.remove_weight_norm()
    assert not any(k.endswith(("weight_g", "weight_v")) for k in m.state_dict())
    m.apply_weight_norm()
    assert [[k, list(v.shape)] for k, v in sorted(m.state_dict().items())] == sorted(meta["keys"])


def test_constructor_defaults_are_the_reference_ones():
    """models/hifigan.py:870-890; the reference's own defaults trip its in_channels == spk_emb_dim
    assertion, and so do these."""
    import inspect

    sig = inspect.signature(DiscreteSymbolHiFiGANGenerator.__init__).parameters
    want = dict(in_channels=512, out_channels=1, channels=512, num_embs=100, num_spk_embs=128, spk_emb_dim=128,
                concat_spk_emb=False, kernel_size=7, upsample_scales=(8, 8, 2, 2),
                upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], use_additional_convs=True, bias=True,
                nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                use_weight_norm=True, use_embedding_feats=False)
    assert list(sig)[1:] == list(want)
    assert {k: sig[k].default for k in want} == want
    with pytest.raises(AssertionError):
        DiscreteSymbolHiFiGANGenerator()


@pytest.mark.parametrize("cfg", DSYM_CONFIGS)
def test_program_accepted_by_host_engine(built_lib, cfg):
    """The lowered program (incl. the 768 -> 512 k = 7 input conv of dsym_token_v1) creates a
    host-only handle, packs, and plans a ragged batch."""
    m, params, _ = dsym_module(cfg)
    P = m.program()
    assert P.channels[0] == params["in_channels"] and P.channels[-1] == 1
    assert "emb.weight" not in P.weights and "spk_emb.weight" not in P.weights
    eng = CnetEngine(P, None, host_only=True)
    state = {k: v for k, v in m.state_dict().items() if not k.startswith(("emb.", "spk_emb."))}
    packed = eng.pack(state)
    assert packed.shape == (eng.packed_weight_count,) and np.isfinite(packed).all() and eng.split_range_ok
    plan = eng.plan([3, 1, 5])
    assert eng.hop == int(np.prod(params["upsample_scales"]))
    assert plan.out_rows == 9 * eng.hop


def _program_table(P):
    ops = []
    for c in P.c_ops():
        d = {}
        for f, _ in PwgCnetOp._fields_:
            if f != "src":
                d[f] = getattr(c, f)
                continue
            d["src"] = []
            for s in c.src:  # an unused source has only ``buf`` (-1) set
                d["src"].append({g: getattr(s, g) for g, _ in PwgCnetSrc._fields_} if s.buf >= 0 else {"buf": s.buf})
        ops.append(d)
    return dict(channels=list(P.channels), rate=list(P.rate), names=list(P.names),
                weights=[[k, n] for k, n in P.weights.items()], ops=ops)


@pytest.mark.parametrize("cfg", ["hifigan_test", "hifigan_v1", "hifigan_noadd_test", "hifigan_causal_test"])
def test_hifigan_program_unchanged(cfg):
    """HiFiGANGenerator.program() now goes through the lowering it shares with the token vocoder.
    tests/golden/dsym/hifigan_program_ops.json holds what program() emitted before that change
    (every PwgCnetOp / PwgCnetSrc field of c_ops(), the buffers, op names and weight layout),
    recorded from the method as it was: the program must be the same, field by field."""
    with open(os.path.join(DSYM_DIR, "hifigan_program_ops.json")) as f:
        want = json.load(f)[cfg]
    got = _program_table(HiFiGANGenerator(**configs.vocoder_params(cfg)[1]).program())
    assert list(got) == list(want)
    for key in ("channels", "rate", "names", "weights"):
        assert got[key] == want[key], key
    assert len(got["ops"]) == len(want["ops"])
    for i, (a, b) in enumerate(zip(got["ops"], want["ops"])):
        for f in b:
            assert a[f] == b[f], (i, got["names"][i], f)
        assert list(a) == list(b)


@pytest.mark.parametrize("over, match", [
    (dict(concat_spk_emb=True), "concat_spk_emb"),
    (dict(upsample_kernel_sizes=[8, 6]), "twice"),
    (dict(upsample_scales=[3, 2], upsample_kernel_sizes=[6, 4]), "odd upsample scale"),
])
def test_refusals(over, match):
    with pytest.raises(NotImplementedError, match=match):
        DiscreteSymbolHiFiGANGenerator(**configs.vocoder_params("dsym_hifigan_test", **over)[1])


@pytest.mark.parametrize("bad", [-1, 11])
def test_host_ids_out_of_range_raise_before_any_gpu_use(bad):
    """numpy / CPU-tensor ids are checked before upload: the module is still on the CPU, where
    reaching the engine would raise RuntimeError instead."""
    m, _, _ = dsym_module("dsym_hifigan_test")
    c = np.stack([np.arange(6), np.full(6, 2)], 1).astype(np.int64)
    c[4, 0] = bad
    with pytest.raises(IndexError, match="token id"):
        m.inference(c)
    with pytest.raises(IndexError, match="token id"):
        m.inference(torch.from_numpy(c).float())
    with pytest.raises(IndexError, match="token id"):
        m(torch.from_numpy(c.T[None]))
    ok = np.stack([np.arange(6), np.full(6, 2)], 1).astype(np.int64)
    for g in (-1, 5):
        with pytest.raises(IndexError, match="speaker id"):
            m.inference(ok, g=g)
    ok[0, 1] = 5
    with pytest.raises(IndexError, match="speaker id"):
        m.inference(ok)
    with pytest.raises(AssertionError):
        m.inference(ok[:, :1])  # a speaker table needs the speaker column (or g=)
    with pytest.raises(AssertionError, match="No statistics"):
        m.inference(ok, normalize_before=True)
    ok[0, 1] = 2
    with pytest.raises(RuntimeError, match="ROCm GPU"):  # valid ids do reach the engine
        m.inference(ok)


def test_embed_rows_argument_checks(built_lib):
    """pwg_embed_rows validates its arguments before any HIP call (none of these calls launches):
    null pointers, dim not a multiple of 16, negative counts, a speaker table without spk_ids /
    row_start, misaligned tables -> PWG_ERR_INVALID with a message."""
    L = built_lib
    P = 0x10000  # never dereferenced: every call below returns from the host-side checks

    def call(emb=P, num_embs=10, spk=P, num_spk=4, dim=48, ids=P, spk_ids=P, row_start=P, n_utts=2, rows=8, out=P,
             flag=P):
        return L.pwg_embed_rows(emb, num_embs, spk, num_spk, dim, ids, spk_ids, row_start, n_utts, rows, out, flag, None)

    bad = [dict(emb=None), dict(ids=None), dict(out=None), dict(flag=None), dict(dim=24), dict(dim=0), dict(dim=-16),
           dict(num_embs=0), dict(num_embs=-3), dict(rows=-1), dict(num_spk=-1), dict(num_spk=0), dict(n_utts=-1),
           dict(n_utts=0), dict(spk_ids=None), dict(row_start=None), dict(spk=None, num_spk=-1),
           dict(spk=None, n_utts=-1), dict(emb=P + 4), dict(spk=P + 8), dict(out=P + 4)]
    for kw in bad:
        assert call(**kw) == _lib.PWG_ERR_INVALID, kw
        assert b"pwg_embed_rows" in L.pwg_last_error(), kw
    # nothing to do is not an error (and launches nothing)
    assert call(rows=0) == _lib.PWG_OK
    assert call(rows=0, spk=None, spk_ids=None, row_start=None, n_utts=0, num_spk=0) == _lib.PWG_OK
    with pytest.raises(ValueError, match="multiple of 16"):
        _lib.check(call(dim=40))


def test_synthetic_embedding_tables_are_unit_normal():
    m, params, folded = dsym_module("dsym_hubert_v1")
    e = folded["emb.weight"]
    assert e.shape == (100, 512) and abs(float(e.std()) - 1.0) < 0.02 and abs(float(e.mean())) < 0.02
    assert folded["spk_emb.weight"].shape == (128, 512)


@pytest.mark.parametrize("name", DSYM_GOLDEN)
def test_oracle_matches_reference_fixture(name):
    g = load_dsym_golden(name)
    m, params, folded = dsym_module(g["meta"]["vocoder"], seed=g["meta"]["weight_seed"])
    y = oracle_golden(g, folded, params)
    assert y.shape == g["y"].shape
    err = float(np.abs(y - g["y"]).max())
    assert err < 2e-5, f"{name}: oracle vs reference {err:.2e}"
