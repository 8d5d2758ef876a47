"""VQVAE without a GPU: the oracle against every fixture (z_e, y, and the indices under the parity
rule), constructor and state-dict layout against the reference's recorded keys, every refusal,
load_model, the C-ABI argument checks of include/pwg_vq.h (they return before any HIP call), the
grouped-conv weight image and the decode CLI's argument handling."""

import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import yaml

import vqvae_oracle
from parallelwavegan_amd import VQVAE, _lib, cnet, configs, synthetic
from parallelwavegan_amd.utils import GENERATORS, generator_class, load_model
from parallelwavegan_amd.vqvae import lower_encoder_tail
from vqvae_helpers import EXPECTED, FIXTURES, WITH_Y, fixture_module, fixture_state, load_fixture, utterances

CONFIGS = sorted(configs.VQVAE_PARAMS)
FIXTURE_OF = {"vqvae_test_a": "vq_a_T61", "vqvae_test_b": "vq_b_T131", "vqvae_v3": "vq_v3_fwd_B1_T256"}


def test_fixture_set():
    assert tuple(FIXTURES) == EXPECTED
    for name in FIXTURES:
        meta = load_fixture(name)["meta"]
        assert meta["e_ref"] <= 1e-5 and meta["y_max"] < 0.99
        assert meta["under_share"] <= 0.01
        assert meta["has_y"] == (name in WITH_Y)
    dup = load_fixture("vq_a_dup")
    # the reference (torch.min on the CPU) returns the lower of the two equal codes, never the copy
    assert dup["meta"]["dup"] == [7, 31] and dup["meta"]["dup_hits"] >= 1
    assert (dup["idx"] == 7).sum() == dup["meta"]["dup_hits"] and not (dup["idx"] == 31).any()


@pytest.mark.parametrize("name", EXPECTED)
def test_oracle_reproduces_the_fixture(name):
    fx = load_fixture(name)
    _, params, folded = fixture_module(fx["meta"])
    book = folded["codebook.embedding.weight"]
    for x, l, g, z_e, idx, y in utterances(fx):
        for dtype in (torch.float64, torch.float32):
            z, own, yy = None, None, None
            z = vqvae_oracle.encoder(x, folded, params["encoder_conf"], dtype)
            own = vqvae_oracle.nearest(z, torch.from_numpy(book).to(dtype))
            ez = float((z.double() - torch.from_numpy(z_e).double()).abs().max())
            print(f"{name} {dtype}: max|z - z_e| = {ez:.2e}")
            assert ez < 1e-5
            viol, under, mism = vqvae_oracle.index_rule(z_e, book, own.numpy(), idx, z_used=z.double().numpy())
            print(f"{name} {dtype}: violations {viol}, under allowance {under}, mismatches {mism} of {len(idx)} frames")
            assert viol == 0 and mism == 0 and under <= vqvae_oracle.cap(len(idx))
            if y is not None:
                rows = vqvae_oracle.decoder_rows(idx, l, g, folded, dtype)
                yy = vqvae_oracle.melgan_decoder(rows, folded, params["decoder_conf"], dtype)
                ey = float((yy.double() - torch.from_numpy(y).double()).abs().max())
                print(f"{name} {dtype}: max|y - y_ref| = {ey:.2e}")
                assert ey < 1e-5


def test_index_rule_counts_what_it_should():
    """The rule flags a wrong index on a clear row, lets either of two near-tied codes pass but counts
    the frame as under its allowance, and fails a case above the cap instead of passing it vacuously."""
    rs = np.random.RandomState(0)
    e = rs.standard_normal((6, 16))
    z = e[[2, 4, 1]] + 1e-3 * rs.standard_normal((3, 16))
    assert vqvae_oracle.index_rule(z, e, [2, 4, 1], [2, 4, 1]) == (0, 0, 0)
    assert vqvae_oracle.index_rule(z, e, [2, 4, 3], [2, 4, 1]) == (1, 0, 1)
    e2 = e.copy()
    e2[5] = e2[2] + 1e-9  # a near tie: within tau of code 2
    z2 = e2[[2]] * 1.0
    v, under, m = vqvae_oracle.index_rule(z2, e2, [5], [2])
    assert (v, under, m) == (0, 1, 0)
    assert vqvae_oracle.cap(1) == 1 and vqvae_oracle.cap(33) == 1 and vqvae_oracle.cap(100) == 2
    e3 = e.copy()
    e3[5] = e3[2]  # an exact copy is one code: the lower index, and no frame counts as near-tied
    assert vqvae_oracle.index_rule(e3[[2]], e3, [2], [2]) == (0, 0, 0)


def test_constructor_defaults_match_the_reference():
    sig = inspect.signature(VQVAE.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert got == dict(
        in_channels=1, out_channels=1, num_embeds=512, embed_dim=256, num_local_embeds=None, local_embed_dim=None,
        num_global_embeds=None, global_embed_dim=None, encoder_type="MelGANDiscriminator",
        decoder_type="MelGANGenerator",
        encoder_conf={"out_channels": 256, "downsample_scales": [4, 4, 2, 2], "max_downsample_channels": 1024},
        decoder_conf={"in_channels": 256, "upsample_scales": [4, 4, 2, 2], "channels": 512, "stacks": 3},
        use_weight_norm=True)
    VQVAE(encoder_conf={"out_channels": 256, "downsample_scales": [2, 2], "max_downsample_channels": 32},
          decoder_conf={"in_channels": 256, "upsample_scales": [2, 2], "channels": 32, "stacks": 1})
    # the defaults are copied, never updated in place (the reference adds in_channels / out_channels to them)
    assert "in_channels" not in sig.parameters["encoder_conf"].default
    assert "out_channels" not in sig.parameters["decoder_conf"].default


def _folded_names(keys):
    out = []
    for k, shape in keys:
        if k.endswith(".weight_g"):
            continue
        out.append((k[:-2] if k.endswith(".weight_v") else k, tuple(shape)))
    return sorted(out)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_state_dict_keys_match_the_reference(cfg):
    meta = load_fixture(FIXTURE_OF[cfg])["meta"]
    m = VQVAE(**configs.vqvae_params(cfg))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["keys"]
    heads = {k.split(".")[0] for k in m.state_dict()}
    want = {"encoder", "codebook", "decoder"}
    if configs.vqvae_params(cfg).get("num_local_embeds") is not None:
        want |= {"local_embed", "global_embed"}
    assert heads == want
    # use_weight_norm=False leaves the encoder plain; the decoder keeps the weight norm of its own
    # constructor, as in the reference (models/vqvae.py:78-83)
    plain = VQVAE(**configs.vqvae_params(cfg, use_weight_norm=False))
    assert not any(k.endswith("weight_g") for k in plain.state_dict() if not k.startswith("decoder."))
    assert any(k.endswith("weight_g") for k in plain.state_dict() if k.startswith("decoder."))
    m.remove_weight_norm()
    assert not any(k.endswith("weight_g") for k in m.state_dict())
    assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == _folded_names(meta["keys"])
    m.apply_weight_norm()
    assert sorted(m.state_dict()) == sorted(k for k, _ in meta["keys"])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_load_state_dict_round_trips(cfg):
    meta = load_fixture(FIXTURE_OF[cfg])["meta"]
    sd = fixture_state(meta)
    m = VQVAE(**configs.vqvae_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    got = m.state_dict()
    assert sorted(got) == sorted(sd)
    for k, v in sd.items():
        np.testing.assert_array_equal(got[k].numpy(), v)
    a, _, folded = fixture_module(meta, weight_norm=True)
    b, _, _ = fixture_module(meta, weight_norm=False)
    for k, v in b.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), folded[k])
    # both checkpoint forms give the dense tail the same flat weights
    pa, pb = lower_encoder_tail(a.encoder), lower_encoder_tail(b.encoder)
    np.testing.assert_array_equal(pa.flatten({k: v.numpy() for k, v in a.encoder.state_dict().items()}),
                                  pb.flatten({k: v.numpy() for k, v in b.encoder.state_dict().items()}))


def _enc(**over):
    return dict(configs.vqvae_params("vqvae_test_a")["encoder_conf"], **over)


@pytest.mark.parametrize("over, match", [
    (dict(encoder_type="HiFiGANMultiScaleDiscriminator"), "encoder_type"),
    (dict(decoder_type="HiFiGANGenerator"), "decoder_type"),
    (dict(in_channels=4), "in_channels"),
    (dict(out_channels=4), "out_channels"),
    (dict(encoder_conf=_enc(nonlinear_activation="ReLU", nonlinear_activation_params={})), "nonlinear_activation"),
    (dict(encoder_conf=_enc(pad="ReplicationPad1d")), "pad"),
    (dict(encoder_conf=_enc(kernel_sizes=[7, 5])), "kernel_sizes"),
    (dict(encoder_conf=_enc(downsample_scales=[5, 2])), "scales"),
    (dict(encoder_conf=_enc(downsample_scales=[4, 1])), "scales"),
    (dict(encoder_conf=_enc(channels=24)), "channels"),
    (dict(encoder_conf=_enc(channels=16, downsample_scales=[3], max_downsample_channels=64)), "outputs per group"),
    (dict(encoder_conf=_enc(channels=64, downsample_scales=[2], max_downsample_channels=32)), "outputs per group"),
    (dict(embed_dim=24, encoder_conf=_enc(out_channels=24)), "embed_dim"),
    (dict(local_embed_dim=8), "local_embed_dim"),
    (dict(local_embed_dim=None), "num_local_embeds"),
    (dict(global_embed_dim=8), "global_embed_dim"),
    (dict(decoder_conf=dict(configs.vqvae_params("vqvae_test_a")["decoder_conf"], nonlinear_activation="Tanh",
                            nonlinear_activation_params={})), "Tanh"),
])
def test_refusals_name_the_argument(over, match):
    m = None
    with pytest.raises(NotImplementedError, match=match):
        m = VQVAE(**configs.vqvae_params("vqvae_test_a", **over))
        # (a decoder configuration the MelGANGenerator drop-in refuses shows when its program is lowered)
        m.decoder.program(False)


def test_cpu_module_refuses_to_run_and_checks_inputs():
    m = VQVAE(**configs.vqvae_params("vqvae_test_b"))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.encode(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.decode(torch.zeros(1, 4, dtype=torch.long))


def test_registration():
    assert "VQVAE" in GENERATORS and generator_class("VQVAE") is VQVAE


def test_encoder_tail_program(built_lib):
    """The dense tail as a host-only plan: buffer 0 the last level's channels, embed_dim out, rate 1."""
    for cfg in CONFIGS:
        m = VQVAE(**configs.vqvae_params(cfg))
        P = lower_encoder_tail(m.encoder)
        assert P.channels[0] == m.encoder.layers[-2][0].in_channels and P.channels[-1] == m.embed_dim
        assert P.rate == [1, 1, 1] and [op["kind"] for op in P.ops] == [cnet.CONV, cnet.CONV]
        assert all(op["post_act"] == cnet.ACT_NONE for op in P.ops)
        eng = cnet.CnetEngine(P, None, host_only=True)
        enc = {k: v for k, v in synthetic.make_module_state_dict(m.encoder, seed=0).items()}
        assert np.isfinite(eng.pack(enc)).all()
        for frames in ([1], [8, 1, 25]):
            assert eng.plan(frames).out_rows == sum(frames)


def _make_ckpt(tmp, cfg="vqvae_test_a", **extra):
    params = configs.vqvae_params(cfg)
    m = VQVAE(**configs.vqvae_params(cfg))
    state = {k: torch.from_numpy(v) for k, v in synthetic.make_module_state_dict(m, seed=4).items()}
    torch.save({"model": {"generator": state}, "steps": 10}, os.path.join(tmp, "checkpoint-10steps.pkl"))
    with open(os.path.join(tmp, "config.yml"), "w") as f:
        yaml.safe_dump(dict(generator_type="VQVAE", generator_params=params, sampling_rate=24000, format="npy",
                            version="0.6.1", use_local_condition=True, use_global_condition=True, **extra), f)
    return os.path.join(tmp, "checkpoint-10steps.pkl"), state


def test_load_model_builds_the_class_and_registers_no_stats(tmp_path):
    ckpt, state = _make_ckpt(str(tmp_path))
    np.save(tmp_path / "stats.npy", np.zeros((2, 80), np.float32))  # present, and not for this generator
    m = load_model(ckpt)
    assert isinstance(m, VQVAE)
    assert not hasattr(m, "mean") and not hasattr(m, "scale")
    got = m.state_dict()
    assert sorted(got) == sorted(state)
    for k, v in state.items():
        assert torch.equal(got[k], v), k


# ---------------------------------------------------------------------------------------------- C-ABI
P1 = ctypes.c_void_p(0x1000)  # a non-null, aligned stand-in: every call below returns before it is read


def test_wave_rows_argument_checks(built_lib):
    L = built_lib
    ok = np.asarray([0, 8, 20], np.int64)
    short = np.asarray([0, 7, 20], np.int64)
    f = ctypes.c_float(0.2)

    def call(x=P1, w=P1, C=16, K=15, rs=P1, host=ok, n=2, rows=20, out=P1):
        return L.pwg_vq_wave_rows(x, w, None, C, K, f, rs, host.ctypes.data if host is not None else None, n, rows, out, None)

    for kw in (dict(x=None), dict(w=None), dict(rs=None), dict(host=None), dict(out=None), dict(n=0), dict(rows=-1),
               dict(out=ctypes.c_void_p(0x1004)), dict(host=short), dict(rows=21)):
        assert call(**kw) == _lib.PWG_ERR_INVALID, kw
    assert b"shorter" in L.pwg_last_error() or b"row_start" in L.pwg_last_error()
    assert call(host=short) == _lib.PWG_ERR_INVALID and b"shorter" in L.pwg_last_error()
    for kw in (dict(K=14), dict(K=33), dict(K=0), dict(C=24), dict(C=8), dict(C=1024, K=31)):
        assert call(**kw) == _lib.PWG_ERR_UNSUPPORTED, kw
    assert call(host=np.asarray([0, 0], np.int64), n=1, rows=0, K=1) == _lib.PWG_OK  # zero rows: nothing launched


def test_gsconv_argument_checks(built_lib):
    L = built_lib
    f = ctypes.c_float(0.2)

    def call(x=P1, rs_in=P1, rows_in=64, cin=16, w=P1, cout=64, s=4, y=P1, rs_out=P1, rows_out=16, n=1):
        return L.pwg_vq_gsconv(x, rs_in, rows_in, cin, w, None, cout, s, f, y, rs_out, rows_out, n, None)

    for kw in (dict(x=None), dict(rs_in=None), dict(w=None), dict(y=None), dict(rs_out=None), dict(n=0),
               dict(rows_in=-1), dict(rows_out=-1), dict(y=ctypes.c_void_p(0x1008))):
        assert call(**kw) == _lib.PWG_ERR_INVALID, kw
    for kw in (dict(s=5), dict(s=1), dict(cin=16, cout=48, s=3), dict(cin=24), dict(cin=16, cout=128),
               dict(cin=512, cout=2048, s=4), dict(cin=64, cout=32, s=2)):
        assert call(**kw) == _lib.PWG_ERR_UNSUPPORTED, kw  # (16 -> 48: 12 outputs per group)
    assert call(rows_out=0) == _lib.PWG_OK


def test_nearest_and_decode_rows_argument_checks(built_lib):
    L = built_lib

    def near(z=P1, rows=4, D=32, e=P1, en=P1, N=48, idx=P1, zq=None, flag=P1):
        return L.pwg_vq_nearest(z, rows, D, e, en, N, idx, zq, flag, None)

    for kw in (dict(z=None), dict(e=None), dict(en=None), dict(idx=None), dict(flag=None), dict(rows=-1), dict(N=0),
               dict(zq=ctypes.c_void_p(0x1004))):
        assert near(**kw) == _lib.PWG_ERR_INVALID, kw
    for kw in (dict(D=24), dict(D=0), dict(D=1040)):
        assert near(**kw) == _lib.PWG_ERR_UNSUPPORTED, kw
    assert near(rows=0) == _lib.PWG_OK
    assert L.pwg_vq_code_norms(None, 4, 32, P1, None) == _lib.PWG_ERR_INVALID
    assert L.pwg_vq_code_norms(P1, 4, 24, P1, None) == _lib.PWG_ERR_UNSUPPORTED

    def dec(e=P1, N=48, D=32, idx=P1, local=P1, nl=2, wl=P1, bl=P1, Ld=16, glob=P1, NG=5, G=16, gid=P1, rs=P1, n=1,
            rows=4, out=P1, flag=P1):
        return L.pwg_vq_decode_rows(e, N, D, idx, local, nl, wl, bl, Ld, glob, NG, G, gid, rs, n, rows, out, flag, None)

    for kw in (dict(out=None), dict(flag=None), dict(e=None, local=None, glob=None), dict(idx=None), dict(N=0),
               dict(rows=-1), dict(gid=None), dict(rs=None), dict(NG=0), dict(n=0), dict(nl=0),
               dict(wl=None, Ld=16), dict(wl=None, bl=None, nl=16, Ld=32), dict(out=ctypes.c_void_p(0x1004))):
        assert dec(**kw) == _lib.PWG_ERR_INVALID, kw
    for kw in (dict(D=24), dict(Ld=8), dict(G=24), dict(wl=None, bl=None, nl=8, Ld=8)):
        assert dec(**kw) == _lib.PWG_ERR_UNSUPPORTED, kw
    assert dec(rows=0) == _lib.PWG_OK


def _packed_position(cin, cout, s, o, i, k):
    """Python restatement of the image: [group][tap][64], element l = 16 * i + (o mod 16 within the
    group's m-tile): the A fragment of v_mfma_f32_16x16x4_f32 (row l & 15, k = l >> 4)."""
    groups = cin // 4
    opg = cout // groups
    g = o // opg
    m_base = (g * opg) // 16 * 16
    return (g * (10 * s + 1) + k) * 64 + 16 * i + (o - m_base)


@pytest.mark.parametrize("cin, cout, s", [(16, 64, 4), (64, 128, 2), (64, 64, 2), (32, 64, 3), (256, 512, 2)])
def test_gsconv_pack(built_lib, cin, cout, s):
    L = built_lib
    K = 10 * s + 1
    n = L.pwg_vq_gsconv_packed_count(cin, cout, s)
    assert n == (cin // 4) * K * 64
    assert L.pwg_vq_gsconv_packed_count(cin, cout, 5) == -1 and L.pwg_vq_gsconv_packed_count(16, 48, 3) == -1
    rs = np.random.RandomState(cin + cout + s)
    for _ in range(6):
        o, i, k = rs.randint(cout), rs.randint(4), rs.randint(K)
        w = np.zeros((cout, 4, K), np.float32)
        w[o, i, k] = 3.5
        packed = np.full(n, np.nan, np.float32)
        assert L.pwg_vq_gsconv_pack(w.ctypes.data, cin, cout, s, packed.ctypes.data) == _lib.PWG_OK
        assert np.flatnonzero(packed).tolist() == [_packed_position(cin, cout, s, o, i, k)]
        assert packed[_packed_position(cin, cout, s, o, i, k)] == 3.5
    # a full weight: every entry appears exactly once, the rest of the image is zero
    w = (1.0 + np.arange(cout * 4 * K, dtype=np.float32)).reshape(cout, 4, K)
    packed = np.empty(n, np.float32)
    assert L.pwg_vq_gsconv_pack(w.ctypes.data, cin, cout, s, packed.ctypes.data) == _lib.PWG_OK
    assert sorted(packed[packed != 0].tolist()) == sorted(w.reshape(-1).tolist())
    assert L.pwg_vq_gsconv_pack(None, cin, cout, s, packed.ctypes.data) == _lib.PWG_ERR_INVALID
    assert L.pwg_vq_gsconv_pack(w.ctypes.data, cin, cout, 5, packed.ctypes.data) == _lib.PWG_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- decode CLI
def test_decode_cli_condition_files_and_refusals(tmp_path):
    from parallelwavegan_amd.bin import decode

    dump = tmp_path / "dump"
    dump.mkdir()
    for u in ("utt_a", "utt_b"):
        np.save(dump / f"{u}-wave.npy", np.zeros(64, np.float32))
        np.save(dump / f"{u}-local.npy", np.zeros((8, 2), np.float32))
    np.save(dump / "utt_a-global.npy", np.asarray(3))
    waves = sorted(str(p) for p in dump.glob("*-wave.npy"))
    loc, glo = decode.vq_condition_files(waves, True, False)
    assert [os.path.basename(p) for p in loc] == ["utt_a-local.npy", "utt_b-local.npy"] and glo is None
    assert decode.vq_condition_files(waves, False, False) == [None, None]
    with pytest.raises(FileNotFoundError, match="utt_b-global.npy"):
        decode.vq_condition_files(waves, True, True)
    ckpt, _ = _make_ckpt(str(tmp_path))
    with pytest.raises(NotImplementedError, match="kaldiio.*wave.npy"):
        decode.main(["--scp", str(tmp_path / "wav.scp"), "--outdir", str(tmp_path / "wav"), "--checkpoint", ckpt,
                     "--verbose", "0"])
    cfg = yaml.safe_load(open(tmp_path / "config.yml"))
    cfg["format"] = "hdf5"
    yaml.safe_dump(cfg, open(tmp_path / "config_h5.yml", "w"))
    with pytest.raises(NotImplementedError, match="h5py"):
        decode.main(["--dumpdir", str(dump), "--outdir", str(tmp_path / "wav"), "--checkpoint", ckpt,
                     "--config", str(tmp_path / "config_h5.yml"), "--verbose", "0"])
