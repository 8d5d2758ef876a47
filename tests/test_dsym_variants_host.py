"""DiscreteSymbolDurationGenerator and DiscreteSymbolF0Generator (parallelwavegan_amd/
dsym_variants.py) without a GPU: state-dict layout against the reference fixtures, refusals,
host-side id / f0 / duration checks, the argument checks of the new C entry points, checkpoint
loading, and the float64 oracle against the fixtures."""

import glob
import json
import os

import numpy as np
import pytest
import torch
import yaml

import dsym_variants_oracle as vo
from conftest import GOLDEN_DIR
from parallelwavegan_amd import DiscreteSymbolDurationGenerator, DiscreteSymbolF0Generator, _lib, configs, synthetic
from parallelwavegan_amd.cnet import CnetEngine
from parallelwavegan_amd.dsym_variants import plan_frame_limit
from parallelwavegan_amd.engine import fold_weight_norm
from parallelwavegan_amd.utils import GENERATORS, generator_class, load_model

VAR_DIR = os.path.join(GOLDEN_DIR, "dsym_variants")
DURATION_GOLDEN = ["dsym_duration_pred_T12", "dsym_duration_ds_T9", "dsym_duration_zeros_T5",
                   "dsym_duration_fwd_B3_T6", "dsym_duration_v1_T3", "dsym_token_duration_16k_T3"]
F0_GOLDEN = ["dsym_f0_T8", "dsym_f0_spk_T7", "dsym_f0_wsum_T6", "dsym_f0_wsum_fix_T6", "dsym_f0_v1_T2"]
VAR_GOLDEN = DURATION_GOLDEN + F0_GOLDEN
CLASSES = {"DiscreteSymbolDurationGenerator": DiscreteSymbolDurationGenerator,
           "DiscreteSymbolF0Generator": DiscreteSymbolF0Generator}


def load_var_golden(name):
    with np.load(os.path.join(VAR_DIR, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def var_module(cfg, seed=0, linear_bias=None):
    """(drop-in with seeded weights loaded, params, weight-norm-folded state dict); linear_bias: the
    fixtures' override of duration_predictor.linear.bias."""
    cls, params = configs.vocoder_params(cfg)
    m = CLASSES[cls](**configs.vocoder_params(cfg)[1])
    sd = synthetic.make_module_state_dict(m, seed=seed)
    if linear_bias is not None:
        sd["duration_predictor.linear.bias"] = np.asarray(linear_bias, np.float32).reshape(1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval(), params, fold_weight_norm(sd)


def golden_module(g):
    return var_module(g["meta"]["vocoder"], g["meta"]["weight_seed"], g.get("linear_bias"))


def oracle_golden(g, folded, params):
    """(audio, log durations or None, durations or None) of a fixture from the float64 oracle."""
    meta, c = g["meta"], g["c"]
    if "dur" not in g:
        L = params["layer_num"] if params.get("use_weight_sum") else 1
        spk = int(c[0, 1]) if params["num_spk_embs"] > 0 else None
        return vo.f0_generator(c if L > 1 else c[:, 0], folded, params, g["f0"], spk), None, None
    given = "ds" in meta["options"]
    if meta["mode"] == "forward":
        total = int(max(d.sum() or len(d) for d in g["dur"]))
        got = [vo.duration_generator(c[b, 0], folded, params, g["dur"][b], total) for b in range(c.shape[0])]
        return np.stack([x[0] for x in got]).transpose(0, 2, 1), np.stack([x[1] for x in got]), g["dur"]
    y, log_d, used = vo.duration_generator(c[:, 0], folded, params, g["dur"] if given else None)
    return y, log_d, used


def test_every_fixture_is_listed():
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(VAR_DIR, "*.npz"))) == sorted(VAR_GOLDEN)


@pytest.mark.parametrize("name", VAR_GOLDEN)
def test_state_dict_matches_reference_keys_and_loads_strictly(name):
    g = load_var_golden(name)
    m, _, _ = golden_module(g)  # load_state_dict(strict=True) of every reference key
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == g["meta"]["keys"]
    keys = [k for k, _ in g["meta"]["keys"]]
    if "dur" in g:
        assert "duration_predictor.conv.0.0.weight" in keys and "duration_predictor.conv.0.0.weight_g" not in keys
        assert "duration_predictor.conv.1.2.bias" in keys and "duration_predictor.linear.weight" in keys
    else:
        assert "input_conv.weight" in keys and "input_conv.weight_g" not in keys and "f0_embedding.weight" in keys


def test_constructor_defaults_are_the_reference_ones():
    import inspect

    common = dict(kernel_size=7, upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                  resblock_kernel_sizes=(3, 7, 11), resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)],
                  use_additional_convs=True, bias=True, nonlinear_activation="LeakyReLU",
                  nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True)
    want_d = dict(in_channels=512, out_channels=1, channels=512, num_embs=100, num_spk_embs=128, spk_emb_dim=128,
                  concat_spk_emb=False, duration_layers=2, duration_chans=384, duration_kernel_size=3,
                  duration_offset=1.0, duration_dropout_rate=0.5, **common)
    want_f = dict(in_channels=512, out_channels=1, channels=512, linear_channel=256, num_embs=100, num_spk_embs=128,
                  spk_emb_dim=128, concat_spk_emb=False, **common, use_embedding_feats=False, use_weight_sum=False,
                  layer_num=12, use_fix_weight=False, use_f0=True)
    for cls, want in ((DiscreteSymbolDurationGenerator, want_d), (DiscreteSymbolF0Generator, want_f)):
        sig = inspect.signature(cls.__init__).parameters
        assert list(sig)[1:] == list(want)
        assert {k: sig[k].default for k in want} == want


def test_duration_refusals():
    with pytest.raises(NotImplementedError, match="reference class cannot"):
        DiscreteSymbolDurationGenerator(**configs.vocoder_params("dsym_duration_test", num_spk_embs=5)[1])
    for over in (dict(duration_kernel_size=5), dict(duration_layers=5), dict(duration_layers=0), dict(duration_chans=40),
                 dict(duration_chans=1040), dict(concat_spk_emb=True, num_spk_embs=5),
                 dict(upsample_kernel_sizes=[8, 6])):
        with pytest.raises(NotImplementedError):
            DiscreteSymbolDurationGenerator(**configs.vocoder_params("dsym_duration_test", **over)[1])


@pytest.mark.parametrize("over, match", [
    (dict(use_embedding_feats=True), "use_embedding_feats"),
    (dict(use_weight_sum=True, layer_num=3, num_spk_embs=5), "speaker table"),
    (dict(use_weight_sum=True, layer_num=17), "layer_num"),
    (dict(linear_channel=24), "linear_channel"),
    (dict(num_spk_embs=5, concat_spk_emb=True), "concat_spk_emb"),
])
def test_f0_refusals(over, match):
    with pytest.raises(NotImplementedError, match=match):
        DiscreteSymbolF0Generator(**configs.vocoder_params("dsym_f0_test", **over)[1])


def test_duration_host_checks_come_before_any_gpu_use():
    """The module is on the CPU, where reaching the engine raises RuntimeError: id num_embs (the
    padding row) is valid, num_embs + 1 and -1 are not; durations are checked on the host too."""
    m, params, _ = var_module("dsym_duration_test")
    E = params["num_embs"]
    c = (np.arange(6) % E).astype(np.int64)[:, None]
    for bad in (-1, E + 1):
        cb = c.copy()
        cb[4, 0] = bad
        for form in (cb, torch.from_numpy(cb).float()):
            with pytest.raises(IndexError, match="token id"):
                m.inference(form)
            with pytest.raises(IndexError, match="token id"):
                m.inference(form, ds=np.ones(6, np.int64))
            with pytest.raises(IndexError, match="token id"):
                m.predict_durations([form])
        with pytest.raises(IndexError, match="token id"):
            m(torch.from_numpy(cb.T[None]), torch.ones(1, 6, dtype=torch.long))
    ok = c.copy()
    ok[4, 0] = E  # the extra row of the table
    with pytest.raises(RuntimeError, match="ROCm GPU"):  # valid ids do reach the engine
        m.inference(ok)
    with pytest.raises(ValueError, match="5 durations for 6 tokens"):
        m.inference(ok, ds=np.ones(5, np.int64))
    with pytest.raises(ValueError, match="duration outside"):
        m.inference(ok, ds=np.asarray([1, 1, -1, 1, 1, 1]))
    with pytest.raises(ValueError, match="one duration vector per utterance"):
        m.inference_batch([ok, ok], ds=[np.ones(6, np.int64)])
    with pytest.raises(AssertionError, match="No statistics"):
        m.inference(ok, normalize_before=True)


def test_f0_host_checks_come_before_any_gpu_use():
    m, params, _ = var_module("dsym_f0_spk_test")
    c = np.stack([np.arange(6), np.full(6, 2)], 1).astype(np.int64)
    f0 = np.linspace(0, 5, 6).astype(np.float32)
    for bad in (-1, params["num_embs"]):
        cb = c.copy()
        cb[3, 0] = bad
        with pytest.raises(IndexError, match="token id"):
            m.inference(cb, f0)
        with pytest.raises(IndexError, match="token id"):
            m(torch.from_numpy(cb.T[None]), torch.from_numpy(f0)[None, None])
    with pytest.raises(IndexError, match="speaker id"):
        m.inference(c, f0, g=5)
    for wrong in (f0[:5], np.concatenate([f0, f0]), f0[:, None]):
        with pytest.raises(ValueError, match="f0"):
            m.inference(c, wrong)
    with pytest.raises(ValueError, match="f0"):
        m.inference(c)  # use_f0 is set: f0 is required
    with pytest.raises(ValueError, match="f0"):
        m(torch.from_numpy(c.T[None]))
    with pytest.raises(ValueError, match="f0"):
        m.inference_batch([c, c], [f0])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.inference(c, f0)
    w, wp, _ = var_module("dsym_f0_wsum_test")
    cw = np.tile(np.arange(6)[:, None], (1, 3)).astype(np.int64)
    cw[2, 1] = wp["num_embs"]
    with pytest.raises(IndexError, match="token id 11 at frame 2"):
        w.inference(cw, f0)
    with pytest.raises(AssertionError):
        w.inference(cw[:, :2], f0)  # (T, layer_num) ids are needed


def test_f0_off_behaves_as_the_parent():
    """use_f0=False: no f0_embedding, a plain in_channels wide input conv, f0 ignored."""
    m = DiscreteSymbolF0Generator(**configs.vocoder_params("dsym_f0_test", use_f0=False)[1])
    keys = list(m.state_dict())
    assert "f0_embedding.weight" not in keys and m.input_conv.in_channels == 48 and m.program().channels[0] == 48
    c = np.arange(6, dtype=np.int64)[:, None]
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.inference(c, np.zeros(3, np.float32))  # the wrong length does not matter: f0 is not looked at
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(torch.from_numpy(c.T[None]))


@pytest.mark.parametrize("cfg", ["dsym_duration_test", "dsym_f0_test", "dsym_f0_spk_test", "dsym_f0_wsum_test",
                                 "dsym_duration_v1", "dsym_token_duration_16k", "dsym_f0_v1"])
def test_program_accepted_by_host_engine(built_lib, cfg):
    """The body program is the HiFiGAN lowering; for the f0 class buffer 0 is in_channels +
    linear_channel wide; no front-end weight is part of it."""
    m, params, _ = var_module(cfg)
    P = m.program()
    assert P.channels[0] == params["in_channels"] + (params.get("linear_channel", 0)) and P.channels[-1] == 1
    assert not any(k.startswith(m._front_prefixes) for k in P.weights)
    eng = CnetEngine(P, None, host_only=True)
    packed = eng.pack({k: v for k, v in m.state_dict().items() if not k.startswith(m._front_prefixes)})
    assert packed.shape == (eng.packed_weight_count,) and np.isfinite(packed).all() and eng.split_range_ok
    hop = int(np.prod(params["upsample_scales"]))
    assert eng.plan([3, 1, 5]).out_rows == 9 * hop
    # the frame limit the duration class checks before it allocates is the plan builder's own
    lim = plan_frame_limit(P)
    assert lim > 10000
    with pytest.raises(NotImplementedError, match="too large"):
        eng.plan([lim + 1])


P = 0x10000  # never dereferenced: every call below returns from the host-side checks


def _expect_invalid(L, fn, call, bad):
    for kw in bad:
        assert call(**kw) == _lib.PWG_ERR_INVALID, kw
        assert fn.encode() in L.pwg_last_error(), kw


def test_durpred_layer_argument_checks(built_lib):
    L = built_lib

    def call(x=None, emb=P, num_embs=10, ids=P, cin=48, cout=32, k=3, w=P, bias=P, ln_g=P, ln_b=P, lin_w=P, lin_b=P,
             offset=1.0, row_start=P, n_utts=2, rows=8, y=P, logdur=P, dur=P, flag=P):
        return L.pwg_durpred_layer(x, emb, num_embs, ids, cin, cout, k, w, bias, ln_g, ln_b, lin_w, lin_b, offset,
                                   row_start, n_utts, rows, y, logdur, dur, flag, None)

    _expect_invalid(L, "pwg_durpred_layer", call, [
        dict(w=None), dict(bias=None), dict(ln_g=None), dict(ln_b=None), dict(row_start=None), dict(flag=None),
        dict(emb=None), dict(ids=None), dict(x=P), dict(num_embs=0), dict(lin_b=None), dict(logdur=None), dict(dur=None),
        dict(lin_w=None), dict(lin_w=None, lin_b=None, logdur=None, dur=None, y=None), dict(cin=24), dict(cin=0),
        dict(cout=-16), dict(cout=40), dict(k=0), dict(k=4), dict(k=-3), dict(rows=-1), dict(n_utts=0), dict(n_utts=-1),
        dict(emb=P + 4), dict(w=P + 8), dict(y=P + 4), dict(x=P + 4, emb=None, ids=None)])
    for kw in (dict(k=5), dict(cin=1040), dict(cout=2048)):
        assert call(**kw) == _lib.PWG_ERR_UNSUPPORTED, kw
        assert b"pwg_durpred_layer" in L.pwg_last_error()
    assert call(rows=0) == _lib.PWG_OK
    assert call(rows=0, x=P, emb=None, ids=None, lin_w=None, lin_b=None, logdur=None, dur=None) == _lib.PWG_OK
    with pytest.raises(NotImplementedError, match="kernel_size 3"):
        _lib.check(call(k=7))


def test_regulate_argument_checks(built_lib):
    L = built_lib

    def scan(ds=P, row_start=P, n_utts=2, tokens=8, prefix=P, totals=P, flag=P):
        return L.pwg_regulate_scan(ds, row_start, n_utts, tokens, prefix, totals, flag, None)

    _expect_invalid(L, "pwg_regulate_scan", scan, [dict(ds=None), dict(row_start=None), dict(prefix=None),
                                                   dict(totals=None), dict(flag=None), dict(n_utts=0),
                                                   dict(n_utts=-2), dict(tokens=-1)])

    def rows(emb=P, num_embs=10, dim=48, ids=P, prefix=P, totals=P, row_start=P, out_start=P, n_utts=2, tokens=8,
             out_rows=20, out=P, flag=P):
        return L.pwg_regulate_rows(emb, num_embs, dim, ids, prefix, totals, row_start, out_start, n_utts, tokens,
                                   out_rows, out, flag, None)

    _expect_invalid(L, "pwg_regulate_rows", rows, [
        dict(emb=None), dict(ids=None), dict(prefix=None), dict(totals=None), dict(row_start=None),
        dict(out_start=None), dict(out=None), dict(flag=None), dict(num_embs=0), dict(dim=24), dict(dim=0),
        dict(dim=-16), dict(n_utts=0), dict(tokens=-1), dict(out_rows=-1), dict(emb=P + 4), dict(out=P + 8)])
    assert rows(out_rows=0) == _lib.PWG_OK


def test_embed_rows_f0_argument_checks(built_lib):
    L = built_lib

    def call(emb=P, num_embs=10, n_tables=1, tw=None, spk=P, num_spk=4, dim=48, lin=16, f0=P, lin_w=P, lin_b=P, ids=P,
             spk_ids=P, row_start=P, n_utts=2, rows=8, out=P, flag=P):
        return L.pwg_embed_rows_f0(emb, num_embs, n_tables, tw, spk, num_spk, dim, lin, f0, lin_w, lin_b, ids, spk_ids,
                                   row_start, n_utts, rows, out, flag, None)

    _expect_invalid(L, "pwg_embed_rows_f0", call, [
        dict(emb=None), dict(ids=None), dict(out=None), dict(flag=None), dict(dim=24), dict(dim=0), dict(dim=-16),
        dict(lin=8), dict(lin=-16), dict(f0=None), dict(lin_w=None), dict(lin_b=None), dict(num_embs=0), dict(rows=-1),
        dict(n_tables=2), dict(n_tables=-1), dict(tw=P, n_tables=0, spk=None), dict(num_spk=0), dict(n_utts=0),
        dict(spk_ids=None), dict(row_start=None), dict(spk=None, num_spk=-1), dict(spk=None, n_utts=-1),
        dict(emb=P + 4), dict(spk=P + 8), dict(out=P + 4), dict(lin_w=P + 4), dict(lin_b=P + 8)])
    for kw in (dict(tw=P, n_tables=17, spk=None), dict(tw=P, n_tables=3)):  # too many tables; weighted sum + speakers
        assert call(**kw) == _lib.PWG_ERR_UNSUPPORTED, kw
        assert b"pwg_embed_rows_f0" in L.pwg_last_error()
    assert call(rows=0) == _lib.PWG_OK
    assert call(rows=0, lin=0, f0=None, lin_w=None, lin_b=None, spk=None, tw=P, n_tables=16) == _lib.PWG_OK


@pytest.mark.parametrize("cfg", ["dsym_duration_test", "dsym_f0_wsum_test"])
def test_load_model_returns_dropin(tmp_path, cfg):
    cls, params = configs.vocoder_params(cfg)
    assert cls in GENERATORS and generator_class(cls) is CLASSES[cls]
    m, _, _ = var_module(cfg, seed=4)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    ckpt = str(tmp_path / "checkpoint-10steps.pkl")
    torch.save({"model": {"generator": state}, "steps": 10}, ckpt)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(dict(generator_type=cls, generator_params=params, sampling_rate=16000, format="npy",
                            version="0.6.1"), f)
    got = load_model(ckpt)
    assert type(got) is CLASSES[cls]
    sd = got.state_dict()
    assert list(sd) == list(state)
    for k, v in state.items():
        assert torch.equal(sd[k], v), k
    assert got.upsample_factor == 8
    with pytest.raises(NotImplementedError):
        generator_class("StyleMelGANGenerator")


@pytest.mark.parametrize("name", VAR_GOLDEN)
def test_oracle_matches_reference_fixture(name):
    g = load_var_golden(name)
    _, params, folded = golden_module(g)
    y, log_d, used = oracle_golden(g, folded, params)
    assert y.shape == g["y"].shape
    err = float(np.abs(y - g["y"]).max())
    assert err < 2e-5, f"{name}: oracle vs reference {err:.2e}"
    if "dur" in g:
        assert np.array_equal(used, g["dur"])
        assert np.array_equal(vo.durations(log_d, params.get("duration_offset", 1.0)),
                              vo.durations(g["logdur"].astype(np.float64), params.get("duration_offset", 1.0)))
        ref_err = float(np.abs(log_d - g["logdur"]).max())
        assert ref_err <= float(g["logdur_ref_err"]) * (1 + 1e-6) + 1e-12  # the recorded reference error


def test_oracle_regulator_rules():
    rows = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(vo.regulate(rows, [0, 2, 0, 1]), rows[[1, 1, 3]])
    assert np.array_equal(vo.regulate(rows, [0, 0, 0, 0]), rows)  # all zero -> all ones
    out = vo.regulate(rows, [1, 0, 0, 0], total=3)
    assert np.array_equal(out[0], rows[0]) and not out[1:].any()
    assert vo.durations(np.log([3.2, 4.7, 1.2, 0.2, np.nan]), 1.0).tolist() == [2, 4, 0, 0, 0]
