"""UHiFiGANGenerator without a GPU: constructor and state-dict layout against the reference's recorded
keys, checkpoint forms, every refusal, host-only plans of the three configs (rows per buffer, the
schedule), the executor's checks of the new op kind and of the external buffer, the unchanged HiFiGAN
programs, load_model and the decode CLI's excitation files. One GPU test: the decode CLI end to end."""

import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch
import yaml

from parallelwavegan_amd import UHiFiGANGenerator, _lib, cnet, configs, synthetic
from parallelwavegan_amd.hifigan import HiFiGANGenerator, lower_hifigan
from parallelwavegan_amd.utils import load_model, read_pcm16_wav
from uhifigan_helpers import FIXTURES, UHG_DIR, dump_program, fixture_module, load_fixture

CONFIGS = sorted(configs.UHIFIGAN_PARAMS)
FIXTURE_OF = {"uhifigan_test": "uhg_test_inf_T7", "uhifigan_noadd_nobias_test": "uhg_noadd_inf_T9",
              "uhifigan_v1": "uhg_v1_fwd_B1_T2"}


def test_fixture_set():
    assert len(FIXTURES) == 7
    for name in FIXTURES:
        meta = load_fixture(name)["meta"]
        assert meta["e_ref"] <= 1e-5 and meta["y_max"] < 0.99


def test_constructor_defaults_match_the_reference():
    sig = inspect.signature(UHiFiGANGenerator.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert got == dict(
        in_channels=80, out_channels=1, channels=512, kernel_size=7, downsample_scales=(8, 8, 2, 2),
        downsample_kernel_sizes=(16, 16, 4, 4), upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
        resblock_kernel_sizes=(3, 7, 11), resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], dropout=0.3,
        use_additional_convs=True, bias=True, nonlinear_activation="LeakyReLU",
        nonlinear_activation_params={"negative_slope": 0.1}, use_causal_conv=False, use_weight_norm=True)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_state_dict_keys_match_the_reference(cfg):
    meta = load_fixture(FIXTURE_OF[cfg])["meta"]
    m = UHiFiGANGenerator(**configs.uhifigan_params(cfg))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["keys"]
    heads = {k.split(".")[0] for k in m.state_dict()}
    assert heads == {"input_conv", "downsamples", "downsamples_mrf", "hidden_conv", "upsamples", "upsamples_mrf",
                     "output_conv"}


def test_load_state_dict_accepts_both_checkpoint_forms():
    meta = load_fixture("uhg_test_inf_T7")["meta"]
    a, _, folded = fixture_module(meta, weight_norm=True)
    b, _, _ = fixture_module(meta, weight_norm=False)
    assert any(k.endswith("weight_g") for k in a.state_dict()) and not any(k.endswith("weight_g") for k in b.state_dict())
    pa, pb = a.program(), b.program()
    fa = pa.flatten({k: v.numpy() for k, v in a.state_dict().items()})
    fb = pb.flatten({k: v.numpy() for k, v in b.state_dict().items()})
    np.testing.assert_array_equal(fa, fb)
    a.remove_weight_norm()
    assert sorted(a.state_dict()) == sorted(folded)
    a.apply_weight_norm()
    a.reset_parameters()


@pytest.mark.parametrize("over, match", [
    (dict(use_causal_conv=True), "use_causal_conv"),
    (dict(downsample_scales=[2, 2, 3]), "downsample_scales"),
    (dict(upsample_kernel_sizes=[4, 4, 5]), "upsample_kernel_sizes"),
    (dict(downsample_kernel_sizes=[6, 4, 5]), "downsample_kernel_sizes"),
    (dict(downsample_scales=[9, 2, 2], downsample_kernel_sizes=[18, 4, 4], upsample_scales=[2, 2, 9],
          upsample_kernel_sizes=[4, 4, 18]), "scales"),
    (dict(out_channels=2), "out_channels"),
    (dict(nonlinear_activation="ReLU", nonlinear_activation_params={}), "nonlinear_activation"),
])
def test_refusals_name_the_argument(over, match):
    with pytest.raises(NotImplementedError, match=match):
        UHiFiGANGenerator(**configs.uhifigan_params("uhifigan_test", **over))


def test_cpu_module_refuses_to_run():
    m = UHiFiGANGenerator(**configs.uhifigan_params("uhifigan_test"))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.inference(excitation=np.zeros(12, np.float32), c=np.zeros((1, 80), np.float32))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_host_only_plans(built_lib, cfg):
    m = UHiFiGANGenerator(**configs.uhifigan_params(cfg))
    P = m.program()
    hop = int(np.prod(m.upsample_scales))
    assert P.rate[P.external] == hop and P.rate[-1] == hop and P.channels[P.external] == m.channels
    eng = cnet.CnetEngine(P, None, host_only=True)
    packed = eng.pack(synthetic.make_module_state_dict(m, seed=0))
    assert np.isfinite(packed).all() and eng.split_range_ok
    kinds = [op["kind"] for op in P.ops]
    n_levels = len(m.upsample_scales)
    assert kinds.count(cnet.SCONV) == n_levels and kinds.count(cnet.CONVT) == n_levels
    assert all(len(op["srcs"]) == 2 for op in P.ops if op["kind"] == cnet.CONVT)
    for T in (1, 7, 33):
        plan = eng.plan([T])
        for b in range(len(P.channels)):
            assert built_lib.pwg_cnet_plan_rows(plan._p, b) == T * P.rate[b]
        assert plan.out_rows == T * hop
        sched, order = eng.schedule(plan)
        launched = {P.ops[_op_of(eng, ph)]["kind"] for ph, _ in sched}
        assert cnet.SCONV in launched and cnet.CONVT in launched
        assert sorted(order) == list(range(len(sched)))
        # the external buffer is the caller's: it takes no workspace slot
        with pytest.raises(ValueError):
            plan.buffer(P.external)
    if m.num_blocks > 1:  # the parallel residual blocks of encoder and decoder stages run concurrently
        eng.set_streams(2)
        sched, _ = eng.schedule(eng.plan([7]))
        first_sconv = min(i for i, (ph, _) in enumerate(sched) if P.ops[_op_of(eng, ph)]["kind"] == cnet.SCONV)
        assert {st for _, st in sched[:first_sconv]} != {0}
        assert {st for _, st in sched[first_sconv:]} != {0}


def _op_of(eng, phase):
    """Program op of a launch's first phase: one phase per op, except a ConvTranspose1d's ``stride``."""
    p = 0
    for i, op in enumerate(eng.program.ops):
        n = op["stride"] if op["kind"] == cnet.CONVT else 1
        if phase < p + n:
            return i
        p += n
    raise AssertionError("phase past the program")


def _sconv_program(taps=None, stride=2, src_rate=None, **op_over):
    P = cnet.Program(16)
    x = P.external_buffer(32, stride if src_rate is None else src_rate)
    h = P.buffer(64, 1)
    P.sconv("down", h, 64, P.src(x, 32, taps=2 * stride if taps is None else taps, pad=1, weight="w"), stride, 1,
            bias="b", post_act=cnet.ACT_LRELU, post_slope=0.1)
    P.ops[-1].update(op_over)
    y = P.buffer(64, 1)
    P.conv("mix", y, 64, [P.src(h, 64, weight="w2")])
    return P


def test_create_checks_strided_convs(built_lib):
    cnet.CnetEngine(_sconv_program(), None, host_only=True)
    for P, match in ((_sconv_program(taps=3), "taps must be 2 \\* stride"),
                     (_sconv_program(stride=9), "stride must be 2..8"),
                     (_sconv_program(src_rate=3), "source rate must be stride \\* destination rate"),
                     (_sconv_program(accumulate=True), "no residual / accumulate")):
        with pytest.raises(NotImplementedError, match=match):
            cnet.CnetEngine(P, None, host_only=True)
    P = _sconv_program()
    nb = len(P.channels)
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="weights out of range"):  # a reference vector shorter than the weights
        _lib.check(built_lib.pwg_cnet_create(P.c_ops(), len(P.ops), nb, (ctypes.c_int * nb)(*P.channels),
                                             (ctypes.c_int * nb)(*P.rate), 1000, -1, ctypes.byref(h)))


def test_external_buffer_rules(built_lib):
    P = _sconv_program()
    eng = cnet.CnetEngine(P, None, host_only=True)
    L = eng._lib
    with pytest.raises(NotImplementedError, match="one external buffer"):
        _lib.check(L.pwg_cnet_set_external(eng._h, 2))
    P2 = _sconv_program()
    P2.external = -1
    eng2 = cnet.CnetEngine(P2, None, host_only=True)
    with pytest.raises(ValueError, match="no writer"):
        _lib.check(L.pwg_cnet_set_external(eng2._h, 2))  # the strided conv writes buffer 2
    for bad in (0, len(P2.channels) - 1):
        with pytest.raises(ValueError, match="internal buffer"):
            _lib.check(L.pwg_cnet_set_external(eng2._h, bad))
    eng2.plan([3])
    with pytest.raises(ValueError, match="before the first plan"):
        _lib.check(L.pwg_cnet_set_external(eng2._h, 1))


def test_two_source_convt_checks(built_lib):
    def prog(rate_b=1, pad_mode=cnet.PAD_ZERO):
        P = cnet.Program(32)
        b = P.external_buffer(32, rate_b)
        h = P.buffer(32, 2)
        P.convt("up", h, 32, P.src(0, 32, weight="w"), 2, 1, 0, src2=P.src(b, 32, pad_mode=pad_mode))
        y = P.buffer(32, 2)
        P.conv("mix", y, 32, [P.src(h, 32, weight="w2")])
        return P

    P = prog()
    assert P.weights["w"] == 64 * 32 * 4
    cnet.CnetEngine(P, None, host_only=True)
    with pytest.raises(NotImplementedError, match="stride\\*T"):
        cnet.CnetEngine(prog(rate_b=2), None, host_only=True)
    with pytest.raises(NotImplementedError, match="two-source ConvTranspose1d"):
        cnet.CnetEngine(prog(pad_mode=cnet.PAD_REPLICATE), None, host_only=True)


def test_hifigan_programs_are_unchanged():
    """lower_hifigan after the MRF stage moved into lower_mrf: op for op what the parent commit
    lowered (tests/golden/uhifigan/hifigan_programs.json, recorded there with dump_program)."""
    want = json.load(open(os.path.join(UHG_DIR, "hifigan_programs.json")))
    for name in ("hifigan_test", "hifigan_v1"):
        _, params = configs.vocoder_params(name)
        got = json.loads(json.dumps(dump_program(lower_hifigan(HiFiGANGenerator(**params)))))
        assert got == want[name], name


def _make_ckpt(tmp, cfg="uhifigan_test"):
    params = configs.uhifigan_params(cfg)
    m = UHiFiGANGenerator(**configs.uhifigan_params(cfg))
    state = {k: torch.from_numpy(v) for k, v in synthetic.make_module_state_dict(m, seed=4).items()}
    torch.save({"model": {"generator": state}, "steps": 10}, os.path.join(tmp, "checkpoint-10steps.pkl"))
    with open(os.path.join(tmp, "config.yml"), "w") as f:
        yaml.safe_dump(dict(generator_type="UHiFiGANGenerator", generator_params=params, sampling_rate=24000,
                            format="npy", version="0.6.1"), f)
    return os.path.join(tmp, "checkpoint-10steps.pkl"), state


def _make_dump(dump, lengths, hop, skip_excitation=()):
    dump.mkdir()
    for i, (u, f) in enumerate(lengths.items()):
        np.save(dump / f"{u}-feats.npy", synthetic.make_mel(f, 80, seed=50 + i))
        if u not in skip_excitation:
            np.save(dump / f"{u}-excitation.npy", (0.5 * np.random.RandomState(60 + i).standard_normal(f * hop)).astype(np.float32))
    np.save(dump / "utt_a-f0.npy", np.zeros(lengths["utt_a"], np.float32))  # read and ignored; others have none


def test_load_model_builds_the_class(tmp_path):
    ckpt, state = _make_ckpt(str(tmp_path))
    m = load_model(ckpt)
    assert isinstance(m, UHiFiGANGenerator)
    got = m.state_dict()
    for k, v in state.items():
        assert torch.equal(got[k], v), k


def test_decode_cli_needs_every_excitation_file(tmp_path):
    from parallelwavegan_amd.bin import decode

    ckpt, _ = _make_ckpt(str(tmp_path))
    lengths = {"utt_a": 9, "utt_b": 4}
    _make_dump(tmp_path / "dump", lengths, 12)
    feats = sorted(str(p) for p in (tmp_path / "dump").glob("*-feats.npy"))
    assert [os.path.basename(p) for p in decode.excitation_files(feats)] == ["utt_a-excitation.npy", "utt_b-excitation.npy"]
    _make_dump(tmp_path / "dump2", lengths, 12, skip_excitation=("utt_b",))
    with pytest.raises(FileNotFoundError, match="utt_b-excitation.npy"):
        decode.main(["--dumpdir", str(tmp_path / "dump2"), "--outdir", str(tmp_path / "wav"), "--checkpoint", ckpt,
                     "--verbose", "0"])


@pytest.mark.gpu
def test_decode_cli_end_to_end(tmp_path, built_lib, cuda_device):
    from parallelwavegan_amd.bin import decode

    ckpt, _ = _make_ckpt(str(tmp_path))
    lengths = {"utt_a": 9, "utt_b": 23, "utt_c": 5}
    _make_dump(tmp_path / "dump", lengths, 12)
    out = tmp_path / "wav"
    assert decode.main(["--dumpdir", str(tmp_path / "dump"), "--outdir", str(out), "--checkpoint", ckpt,
                        "--verbose", "0", "--batch-frames", "30"]) == 0
    m = load_model(ckpt)
    m.remove_weight_norm()
    m = m.eval().to(cuda_device)
    for u, f in lengths.items():
        z, sr = read_pcm16_wav(str(out / f"{u}_gen.wav"))
        assert sr == 24000 and z.shape == (f * 12,)
        y = m.inference(excitation=np.load(tmp_path / "dump" / f"{u}-excitation.npy"),
                        c=np.load(tmp_path / "dump" / f"{u}-feats.npy")).view(-1).cpu().numpy()
        np.testing.assert_allclose(z, np.clip(y, -1, 1), atol=1.5 / 32767)
