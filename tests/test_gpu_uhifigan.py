"""UHiFiGANGenerator on the GPU: parity with the reference fixtures (tests/golden/uhifigan, made by
make_golden_uhifigan.py) and with the float64 oracle (tests/uhifigan_oracle.py) level by level, ragged
batches, the input forms, both numeric modes, the range behaviour, and the two new executor ops on
their own (strided conv, two-source transposed conv) against torch in float64."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parallelwavegan_amd import _lib, cnet, synthetic
from uhifigan_helpers import FIXTURES, fixture_module, load_fixture, utterances
from uhifigan_oracle import Oracle

pytestmark = pytest.mark.gpu

ATOL = 1e-4  # the project's parity bar (BASELINE.json); the fixtures' own fp32 error is under 1e-5

RAGGED_T = (1, 7, 33)  # hop 12: 12, 84 and 396 sample-rate rows (396 = 3 x 128 + 12)
EDGE = 4.0             # magnitude of the utterances' edge samples / frames in the ragged batch


def _run_fixture(m, fx, dev):
    if fx["meta"]["mode"] == "inference":
        return m.inference(excitation=fx["excitation"], f0=None, c=fx["c"]).cpu().numpy()
    return m(torch.from_numpy(fx["c"]).to(dev), None, torch.from_numpy(fx["excitation"]).to(dev)).cpu().numpy()


@pytest.fixture(scope="module")
def test_model(built_lib, cuda_device):
    """uhifigan_test with the fixtures' weights, on the GPU, and its float64 oracle."""
    meta = load_fixture("uhg_test_fwd_B3_T5")["meta"]
    m, params, folded = fixture_module(meta)
    return m.to(cuda_device), Oracle(folded, params)


@pytest.fixture(scope="module")
def ragged(test_model):
    """Inputs, the batched outputs and the oracle's outputs of the ragged batch (computed once).
    Every utterance starts and ends with large samples / frames: a tap that read across an utterance
    boundary would change the batched result against the solo run."""
    m, orc = test_model
    cs, es = [], []
    for i, t in enumerate(RAGGED_T):
        c = synthetic.make_mel(t, 80, seed=20 + i).copy()
        e = (0.5 * np.random.RandomState(30 + i).standard_normal(t * 12)).astype(np.float32)
        c[0] = EDGE * np.sign(c[0] + 1e-3)
        c[-1] = -EDGE * np.sign(c[-1] + 1e-3)
        e[:3] = EDGE
        e[-3:] = -EDGE
        cs.append(c)
        es.append(e)
    outs = [o.clone() for o in m.inference_batch(cs, es)]
    want = [orc(c, e).numpy() for c, e in zip(cs, es)]
    return cs, es, outs, want


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity(built_lib, cuda_device, name):
    fx = load_fixture(name)
    m, _, _ = fixture_module(fx["meta"])
    y = _run_fixture(m.to(cuda_device), fx, cuda_device)
    assert y.shape == fx["y"].shape
    assert np.isfinite(y).all()
    err = np.abs(y - fx["y"]).max()
    print(f"{name}: max|y - fixture| {err:.2e} (e_ref {fx['meta']['e_ref']:.1e})")
    assert err < ATOL


@pytest.mark.parametrize("name", [n for n in FIXTURES if "_v1_" not in n])
def test_fixture_parity_exact_fp32(built_lib, cuda_device, name):
    fx = load_fixture(name)
    m, _, _ = fixture_module(fx["meta"])
    m = m.to(cuda_device)
    m.engine().set_split_f16(False)
    y = _run_fixture(m, fx, cuda_device)
    assert not m.engine().split_f16
    assert y.shape == fx["y"].shape and np.isfinite(y).all()
    err = np.abs(y - fx["y"]).max()
    print(f"{name} (exact fp32): max|y - fixture| {err:.2e} (e_ref {fx['meta']['e_ref']:.1e})")
    assert err < ATOL


def test_levels_against_oracle(built_lib, cuda_device):
    """Every tensor the oracle returns -- the front end's output, every encoder MRF average and
    strided-conv output, hidden_conv's output, every transposed-conv output and decoder MRF average --
    read from the workspace after a forward of the B = 3 fixture, at 1e-4 absolutely."""
    fx = load_fixture("uhg_test_fwd_B3_T5")
    m, params, folded = fixture_module(fx["meta"])
    m = m.to(cuda_device)
    orc = Oracle(folded, params)
    eng = m.engine()
    eng.set_streams(2)  # every buffer its own workspace slot (pwg_cnet_plan_buffer)
    utts = utterances(fx)
    keep = {}
    outs = m._run([c for c, _, _ in utts], [e for _, e, _ in utts], keep=keep)
    torch.cuda.synchronize()
    plan, ws, P = keep["plan"], keep["workspace"], eng.program
    want = []
    for c, e, _ in utts:
        lv = {}
        orc(c, e, levels=lv)
        want.append(lv)

    def read(buf):
        if buf == P.external:
            return keep["ext"].view(-1, P.channels[buf]).cpu().numpy()
        off, rows, ld = plan.buffer(buf)
        t = ws[off:off + rows * ld * 4].view(torch.float32).reshape(rows, ld).cpu().numpy()
        assert not t[:, P.channels[buf]:].any(), "padding channels must be zero"
        return t[:, :P.channels[buf]]

    def check(label, buf, pick):
        got = read(buf)
        n = got.shape[0] // len(utts)
        for u in range(len(utts)):
            w = pick(want[u]).numpy()
            assert got[u * n:(u + 1) * n].shape == w.shape, label
            err = np.abs(got[u * n:(u + 1) * n] - w).max()
            print(f"{label} utt {u}: {err:.2e}")
            assert err < ATOL, label

    check("excite", m.taps["excite"], lambda lv: lv["excite"])
    check("hidden", m.taps["hidden"], lambda lv: lv["hidden"])
    for key in ("down_mrf", "down", "up", "up_mrf"):
        for i, buf in enumerate(m.taps[key]):
            check(f"{key}[{i}]", buf, lambda lv, key=key, i=i: lv[key][i])
    for (c, e, y), o in zip(utts, outs):
        assert np.abs(o.cpu().numpy() - y).max() < ATOL


def test_ragged_batch_equals_solo_runs(test_model, ragged):
    m, _ = test_model
    cs, es, outs, _ = ragged
    for c, e, o in zip(cs, es, outs):
        assert o.shape == (c.shape[0] * 12, 1)
        assert torch.equal(m.inference(excitation=e, c=c), o)


def test_ragged_batch_against_oracle(test_model, ragged):
    _, _, outs, want = ragged
    for o, w in zip(outs, want):
        y = o.cpu().numpy()
        assert np.isfinite(y).all()
        err = np.abs(y - w).max()
        print(f"ragged T' = {w.shape[0] // 12}: {err:.2e}")
        assert err < ATOL


def test_two_runs_are_identical(test_model, ragged):
    m, _ = test_model
    cs, es, outs, _ = ragged
    again = m.inference_batch(cs, es)
    assert all(torch.equal(a, o) for a, o in zip(again, outs))


def test_forward_equals_inference(test_model, cuda_device):
    m, _ = test_model
    fx = load_fixture("uhg_test_fwd_B3_T5")
    y = m(torch.from_numpy(fx["c"]).to(cuda_device), None, torch.from_numpy(fx["excitation"]).to(cuda_device))
    assert y.shape == fx["y"].shape
    for b, (c, e, _) in enumerate(utterances(fx)):
        assert torch.equal(m.inference(excitation=e, f0=np.zeros(c.shape[0], np.float32), c=c), y[b].T)


def test_input_forms_agree(test_model, cuda_device):
    m, _ = test_model
    fx = load_fixture("uhg_test_inf_T7")
    c, e = fx["c"], fx["excitation"]
    y_np = m.inference(excitation=e, c=c)
    y_cpu = m.inference(excitation=torch.from_numpy(e), c=torch.from_numpy(c))
    y_gpu = m.inference(excitation=torch.from_numpy(e).to(cuda_device), c=torch.from_numpy(c).to(cuda_device))
    assert torch.equal(y_np, y_cpu) and torch.equal(y_np, y_gpu)
    with pytest.raises(ValueError, match="excitation has 83 samples"):
        m.inference(excitation=e[:-1], c=c)


def test_inf_excitation_raises_range_error(built_lib, cuda_device):
    """A non-finite excitation reaches the program output through the front end, the strided convs
    and the two-source transposed convs: pwg_cnet_run_status reports it (the drop-in's call then
    reruns in exact fp32, as for every range error), and the next clean call matches its fixture."""
    fx = load_fixture("uhg_test_inf_T7")
    m, _, _ = fixture_module(fx["meta"])
    m = m.to(cuda_device)
    eng = m.engine()
    bad = fx["excitation"].copy()
    bad[40] = np.inf
    y = m.inference(excitation=bad, c=fx["c"])
    assert eng.range_reruns == 1 and eng.split_f16
    assert not torch.isfinite(y).all()
    # the raw path reports the flag instead of rerunning
    plan = eng.plan([7])
    ext, _ = m._excite(torch.from_numpy(bad).to(cuda_device), [7], cuda_device)
    out = torch.empty(plan.out_rows, device=cuda_device)
    eng.run(plan, torch.from_numpy(fx["c"]).to(cuda_device).reshape(-1), out, check=False, ext=ext)
    with pytest.raises(_lib.RangeError):
        eng.run_status(plan)
    y = m.inference(excitation=fx["excitation"], c=fx["c"]).cpu().numpy()
    assert eng.range_reruns == 1
    assert np.abs(y - fx["y"]).max() < ATOL


# ------------------------------------------------------------------ the new ops on their own
UNIT_COLS = (1, 2, 129)  # output columns per utterance: under a tile, and a 64-column tile pair + 1


def _unit_engine(P, state, dev):
    eng = cnet.CnetEngine(P, dev)
    eng.load_state_dict(state)
    return eng


def _rand(rs, *shape, fan_in):
    return (rs.standard_normal(shape) / np.sqrt(fan_in)).astype(np.float32)


@pytest.mark.parametrize("split", [True, False], ids=["split_f16", "exact_fp32"])
@pytest.mark.parametrize("cin", [32, 256])
@pytest.mark.parametrize("s", [2, 3, 5, 8])
def test_strided_conv_unit(built_lib, cuda_device, s, cin, split):
    """Strided conv + LeakyReLU + a 1x1 to the output, against conv1d in float64. The high-rate
    source is the program's external buffer; buffer 0 (16 channels) is not read."""
    rs = np.random.RandomState(100 * s + cin)
    cout, pad = 2 * cin, s // 2 + s % 2
    P = cnet.Program(16)
    x = P.external_buffer(cin, s)
    h = P.buffer(cout, 1)
    P.sconv("down", h, cout, P.src(x, cin, taps=2 * s, pad=pad, weight="down.weight"), s, pad, bias="down.bias",
            post_act=cnet.ACT_LRELU, post_slope=0.1)
    y = P.buffer(cout, 1)
    P.conv("mix", y, cout, [P.src(h, cout, weight="mix.weight")], bias="mix.bias")
    state = {"down.weight": _rand(rs, cout, cin, 2 * s, fan_in=cin * 2 * s), "down.bias": _rand(rs, cout, fan_in=100),
             "mix.weight": _rand(rs, cout, cout, 1, fan_in=cout), "mix.bias": _rand(rs, cout, fan_in=100)}
    eng = _unit_engine(P, state, cuda_device)
    eng.set_split_f16(split)
    xs = [rs.standard_normal((n * s, cin)).astype(np.float32) for n in UNIT_COLS]
    for v in xs:  # large edges: a tap reading the neighbouring utterance's rows shows
        v[0] = 8.0
        v[-1] = -8.0
    ext = torch.from_numpy(np.concatenate(xs)).to(cuda_device).reshape(-1)
    mel = torch.zeros(sum(UNIT_COLS) * 16, device=cuda_device)
    outs = eng.infer_rows(list(UNIT_COLS), mel, ext=ext)
    w = {k: torch.from_numpy(v).double() for k, v in state.items()}
    for n, v, o in zip(UNIT_COLS, xs, outs):
        t = F.conv1d(torch.from_numpy(v).double().T[None], w["down.weight"], w["down.bias"], stride=s, padding=pad)
        ref = F.conv1d(F.leaky_relu(t, 0.1), w["mix.weight"], w["mix.bias"])[0].T.numpy()
        assert o.shape == (n, cout)
        err = np.abs(o.cpu().numpy() - ref).max()
        print(f"s {s} cin {cin} cols {n}: {err:.2e}")
        assert err < ATOL


@pytest.mark.parametrize("split", [True, False], ids=["split_f16", "exact_fp32"])
@pytest.mark.parametrize("s", [2, 3])
def test_two_source_convt_unit(built_lib, cuda_device, s, split):
    """ConvTranspose1d over [a; b] (64 + 64 -> 32 channels) + a 1x1 to the output, against
    conv_transpose1d on the concatenation in float64; the halves are filled differently (b three
    times a's scale, another seed), so swapped halves fail."""
    rs = np.random.RandomState(7 + s)
    ca = cb = 64
    cout, pad, opad = 32, s // 2 + s % 2, s % 2
    P = cnet.Program(ca)
    b = P.external_buffer(cb, 1)
    h = P.buffer(cout, s)
    P.convt("up", h, cout, P.src(0, ca, pre_slope=0.1, weight="up.weight"), s, pad, opad, bias="up.bias",
            src2=P.src(b, cb, pre_slope=0.1))
    y = P.buffer(cout, s)
    P.conv("mix", y, cout, [P.src(h, cout, weight="mix.weight")], bias="mix.bias")
    state = {"up.weight": _rand(rs, ca + cb, cout, 2 * s, fan_in=(ca + cb) * 2), "up.bias": _rand(rs, cout, fan_in=100),
             "mix.weight": _rand(rs, cout, cout, 1, fan_in=cout), "mix.bias": _rand(rs, cout, fan_in=100)}
    eng = _unit_engine(P, state, cuda_device)
    eng.set_split_f16(split)
    xa = [rs.standard_normal((n, ca)).astype(np.float32) for n in UNIT_COLS]
    xb = [(3.0 * rs.standard_normal((n, cb))).astype(np.float32) for n in UNIT_COLS]
    mel = torch.from_numpy(np.concatenate(xa)).to(cuda_device).reshape(-1)
    ext = torch.from_numpy(np.concatenate(xb)).to(cuda_device).reshape(-1)
    outs = eng.infer_rows(list(UNIT_COLS), mel, ext=ext)
    w = {k: torch.from_numpy(v).double() for k, v in state.items()}
    for n, va, vb, o in zip(UNIT_COLS, xa, xb, outs):
        cat = torch.cat((torch.from_numpy(va).double().T, torch.from_numpy(vb).double().T))[None]
        t = F.conv_transpose1d(F.leaky_relu(cat, 0.1), w["up.weight"], w["up.bias"], stride=s, padding=pad,
                               output_padding=opad)
        ref = F.conv1d(t, w["mix.weight"], w["mix.bias"])[0].T.numpy()
        assert o.shape == (n * s, cout)
        err = np.abs(o.cpu().numpy() - ref).max()
        print(f"s {s} cols {n}: {err:.2e}")
        assert err < ATOL
