"""DiscreteSymbolDurationGenerator and DiscreteSymbolF0Generator on the GPU: the length-regulated
gather (bit-exact against torch.repeat_interleave), the duration predictor kernel against the
float64 oracle, the f0 / weighted-sum front end, parity of the whole generators with the reference
fixtures, input forms, the out-of-range flags, and the decode CLI."""

import numpy as np
import pytest
import torch
import yaml

import dsym_variants_oracle as vo
from parallelwavegan_amd import _lib, configs
from parallelwavegan_amd.utils import read_pcm16_wav
from test_dsym_variants_host import DURATION_GOLDEN, F0_GOLDEN, golden_module, load_var_golden, var_module

pytestmark = pytest.mark.gpu

ATOL = 1e-4  # the project's parity bound (tests/test_gpu_vocoders.py)
EPS = 2.0 ** -23


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _i64(a, dev):
    return torch.as_tensor(np.asarray(a, np.int64), device=dev)


def _mask(a, dev):
    return torch.as_tensor(np.asarray(a, bool), device=dev)


# ------------------------------------------------------------------ length-regulated gather
def _regulate(L, emb, ids, ds, counts, extra, flag):
    """scan + gather over a ragged batch; utterance u gets total(u) + extra[u] output rows.
    Returns (out (rows, dim), prefix, totals) as the kernels wrote them."""
    dev = emb.device
    n, tokens = len(counts), int(sum(counts))
    rs = _i64(np.concatenate([[0], np.cumsum(counts)]), dev)
    prefix = torch.full((tokens,), -7, dtype=torch.int64, device=dev)
    totals = torch.full((n,), -7, dtype=torch.int64, device=dev)
    _lib.check(L.pwg_regulate_scan(ds.data_ptr(), rs.data_ptr(), n, tokens, prefix.data_ptr(), totals.data_ptr(),
                                   flag.data_ptr(), _stream(dev)))
    tot = totals.cpu().numpy()
    frames = [int(t) + int(e) for t, e in zip(tot, extra)]
    os_ = _i64(np.concatenate([[0], np.cumsum(frames)]), dev)
    out = torch.full((sum(frames), emb.shape[1]), float("nan"), device=dev)
    _lib.check(L.pwg_regulate_rows(emb.data_ptr(), emb.shape[0], emb.shape[1], ids.data_ptr(), prefix.data_ptr(),
                                   totals.data_ptr(), rs.data_ptr(), os_.data_ptr(), n, tokens, sum(frames),
                                   out.data_ptr(), flag.data_ptr(), _stream(dev)))
    return out, prefix.cpu().numpy(), tot, frames


def _durations_for(T, rs):
    """Durations with a leading zero, a trailing zero, a run of zeros and one of 70 (T = 33); all
    zeros (T = 7: the ones rule); a single token of 2 (T = 1)."""
    if T == 33:
        d = rs.randint(0, 5, size=T)
        d[0], d[-1], d[10:14], d[20], d[1] = 0, 0, 0, 70, 3
        return d.astype(np.int64)
    return np.zeros(T, np.int64) if T == 7 else np.full(T, 2, np.int64)


@pytest.mark.parametrize("dim", [48, 768])
def test_regulated_gather_bit_exact(built_lib, cuda_device, dim):
    """Utterances of 1, 7 and 33 tokens in three orders. The 33-token one has a leading zero, a
    trailing zero, a run of zeros and a duration of 70 (one token spanning several waves' row
    groups); the 7-token one is all zeros and must come out as all ones with its neighbours
    untouched. Rows equal torch.repeat_interleave bit for bit; rows an utterance is given beyond its
    total are zeros; prefix sums and totals are the exclusive scan; no flag bit is set."""
    rs = np.random.RandomState(dim)
    num_embs = 37
    emb = torch.from_numpy(rs.standard_normal((num_embs, dim)).astype(np.float32)).to(cuda_device)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    for counts in ([1, 7, 33], [7, 1, 33], [33, 7, 1]):
        ids_h = rs.randint(0, num_embs, size=sum(counts)).astype(np.int64)
        ids_h[0], ids_h[-1] = num_embs - 1, 0
        ds_h = np.concatenate([_durations_for(T, rs) for T in counts])
        ids, ds = _i64(ids_h, cuda_device), _i64(ds_h, cuda_device)
        for extra in ([0, 0, 0], [3, 0, 5]):
            out, prefix, tot, frames = _regulate(built_lib, emb, ids, ds, counts, extra, flag)
            o = t0 = 0
            for u, T in enumerate(counts):
                d = ds_h[t0:t0 + T].copy()
                if d.sum() == 0:
                    d[:] = 1
                assert tot[u] == d.sum() and np.array_equal(prefix[t0:t0 + T], np.cumsum(d) - d), (counts, u)
                want = torch.repeat_interleave(emb[ids[t0:t0 + T]], _i64(d, cuda_device), 0)
                assert torch.equal(out[o:o + int(d.sum())], want), (counts, extra, u)
                assert not out[o + int(d.sum()):o + frames[u]].any(), (counts, extra, u)  # pad_list rows
                o, t0 = o + frames[u], t0 + T
    assert int(flag.item()) == 0


def test_regulated_gather_flags(built_lib, cuda_device):
    """A negative duration sets PWG_EMBED_BAD_DURATION and counts as 0, nothing else changes; a token
    id one past either end of the table (the table is the middle of a larger tensor) gives zero
    rows and PWG_EMBED_BAD_TOKEN, every other row is exact."""
    rs = np.random.RandomState(1)
    emb = torch.from_numpy(rs.standard_normal((1 + 11 + 1, 48)).astype(np.float32)).to(cuda_device)[1:12]
    counts = [4, 6]
    ids_h = rs.randint(0, 11, size=10).astype(np.int64)
    ds_h = np.asarray([2, 0, 1, 3, 1, 1, 0, 2, 4, 1], np.int64)
    ids = _i64(ids_h, cuda_device)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    ref, _, tot0, _ = _regulate(built_lib, emb, ids, _i64(ds_h, cuda_device), counts, [0, 0], flag)
    assert int(flag.item()) == 0
    neg = ds_h.copy()
    neg[1], neg[6] = -3, -(1 << 40)
    out, _, tot, _ = _regulate(built_lib, emb, ids, _i64(neg, cuda_device), counts, [0, 0], flag)
    assert int(flag.item()) == 4 and np.array_equal(tot, tot0) and torch.equal(out, ref)
    for bad_at, bad_id in ((2, 11), (7, -1)):
        flag.zero_()
        b = ids_h.copy()
        b[bad_at] = bad_id
        out, _, _, _ = _regulate(built_lib, emb, _i64(b, cuda_device), _i64(ds_h, cuda_device), counts, [0, 0], flag)
        src = np.repeat(np.arange(10), ds_h)
        assert int(flag.item()) == 1
        hit, rest = _mask(src == bad_at, cuda_device), _mask(src != bad_at, cuda_device)
        assert hit.any() and not out[hit].any() and torch.equal(out[rest], ref[rest])


# ------------------------------------------------------------------ duration predictor kernel
PREDICTOR_FIXTURE = {"dsym_duration_test": "dsym_duration_pred_T12", "dsym_duration_v1": "dsym_duration_v1_T3",
                     "dsym_token_duration_16k": "dsym_token_duration_16k_T3"}


@pytest.mark.parametrize("cfg", list(PREDICTOR_FIXTURE))
def test_predictor_kernel_against_float64_oracle(built_lib, cuda_device, cfg):
    """(idim, chans) = (48, 32), (512, 384), (1024, 384); ragged batches of 1, 2, 17 and 33 tokens in
    two orders (T = 1 and 2 are shorter than the kernel, 17 and 33 cross the 16-row tile edges, the
    single-token utterance sits between two longer ones: a tap leaking across an utterance boundary
    shows). max |log duration - float64 oracle| <= 4 x logdur_ref_err of the matching fixture (the
    reference's own fp32 CPU error; the factor 4 allows another accumulation order and stays two
    orders below an f16-operand path). Durations are those of the float64 log durations wherever
    exp(x) - offset is not within twice that bound of a rounding edge (an error of at most the bound
    cannot move such a token across the edge).
    Measured on an MI355X (printed below): 48 -> 32: 6.97e-07 (bound 3.66e-06); 512 -> 384: 1.33e-06
    (3.93e-06); 1024 -> 384: 8.12e-07 (2.68e-06)."""
    g = load_var_golden(PREDICTOR_FIXTURE[cfg])
    m, params, folded = golden_module(g)
    m = m.to(cuda_device)
    bound = 4.0 * float(g["logdur_ref_err"])
    E, offset = params["num_embs"] + 1, params.get("duration_offset", 1.0)
    rs = np.random.RandomState(5)
    worst = 0.0
    for counts in ([17, 1, 33, 2], [2, 33, 1, 17]):
        toks = [rs.randint(0, E, size=T).astype(np.int64) for T in counts]
        toks[0][0] = E - 1  # the padding row of the table
        _, dev, rs_d, ids_d, _, _ = m._tokens_to_device(toks)
        with torch.cuda.device(dev):
            logdur, dur = m._predict(ids_d, rs_d, len(counts), sum(counts), torch.cuda.current_stream(dev))
        logdur, dur = logdur.cpu().numpy().astype(np.float64), dur.cpu().numpy()
        want = np.concatenate([vo.predictor_log_durations(folded["emb.weight"][t], folded) for t in toks])
        err = np.abs(logdur - want)
        worst = max(worst, float(err.max()))
        v = np.exp(want) - offset
        clear = np.abs(v - (np.floor(v) + 0.5)) > 2.0 * bound * np.exp(want)
        assert np.array_equal(dur[clear], vo.durations(want, offset)[clear]), counts
        assert (dur >= 0).all()
    print(f"{cfg}: max|log duration - float64| = {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound


def test_predictor_layer_input_forms_and_flag(built_lib, cuda_device):
    """Layer 0 fed rows that pwg_embed_rows-style indexing wrote (x) equals the gather by id bit for
    bit; an id one past either end of the table (the middle of a larger tensor) reads as a zero row
    and sets PWG_EMBED_BAD_TOKEN."""
    L = built_lib
    rs = np.random.RandomState(2)
    cin, cout, E = 48, 32, 11
    emb = torch.from_numpy(rs.standard_normal((E + 2, cin)).astype(np.float32)).to(cuda_device)[1:E + 1]
    w = torch.from_numpy((rs.standard_normal((3, cin, cout)) / 12).astype(np.float32)).to(cuda_device)
    vec = [torch.from_numpy(rs.standard_normal(cout).astype(np.float32)).to(cuda_device) for _ in range(3)]
    counts = [5, 1, 19]
    rows = sum(counts)
    rs_d = _i64(np.concatenate([[0], np.cumsum(counts)]), cuda_device)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)

    def run(x, ids):
        y = torch.full((rows, cout), float("nan"), device=cuda_device)
        _lib.check(L.pwg_durpred_layer(x.data_ptr() if x is not None else None, emb.data_ptr() if x is None else None,
                                       E if x is None else 0, ids.data_ptr() if x is None else None, cin, cout, 3,
                                       w.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), None, None,
                                       1.0, rs_d.data_ptr(), len(counts), rows, y.data_ptr(), None, None,
                                       flag.data_ptr(), _stream(cuda_device)))
        return y

    ids_h = rs.randint(0, E, size=rows).astype(np.int64)
    ids = _i64(ids_h, cuda_device)
    y0 = run(None, ids)
    assert torch.isfinite(y0).all() and torch.equal(run(emb[ids].contiguous(), None), y0)
    assert int(flag.item()) == 0
    for bad_at, bad_id in ((7, E), (24, -1)):
        b = ids_h.copy()
        b[bad_at] = bad_id
        x = emb[_i64(np.clip(b, 0, E - 1), cuda_device)].contiguous()
        x[bad_at] = 0.0
        flag.zero_()
        assert torch.equal(run(None, _i64(b, cuda_device)), run(x, None))
        assert int(flag.item()) == 1


# ------------------------------------------------------------------ f0 / weighted-sum front end
def _embed_f0(L, emb, tw, spk, ids, spk_ids, counts, f0, lin_w, lin_b, flag):
    dev = emb.device
    rows, dim, lin = int(sum(counts)), emb.shape[-1], 0 if lin_w is None else lin_w.numel()
    rs_d = _i64(np.concatenate([[0], np.cumsum(counts)]), dev)
    out = torch.full((rows, dim + lin), float("nan"), device=dev)
    num_embs = emb.shape[-2]
    _lib.check(L.pwg_embed_rows_f0(
        emb.data_ptr(), num_embs, emb.shape[0] if tw is not None else 1, tw.data_ptr() if tw is not None else None,
        spk.data_ptr() if spk is not None else None, spk.shape[0] if spk is not None else 0, dim, lin,
        f0.data_ptr() if f0 is not None else None, lin_w.data_ptr() if lin_w is not None else None,
        lin_b.data_ptr() if lin_b is not None else None, ids.data_ptr(),
        spk_ids.data_ptr() if spk is not None else None, rs_d.data_ptr(), len(counts), rows, out.data_ptr(),
        flag.data_ptr(), _stream(dev)))
    return out


def _f0_inputs(rs, rows, lin, dev):
    f0 = rs.uniform(4.0, 6.0, size=rows).astype(np.float32)
    f0[::5] = 0.0
    w, b = rs.standard_normal(lin).astype(np.float32), rs.standard_normal(lin).astype(np.float32)
    return f0, w, b, [torch.from_numpy(a).to(dev) for a in (f0, w, b)]


def _check_f0_columns(out, dim, f0, w, b):
    got = out[:, dim:].cpu().numpy().astype(np.float64)
    f, w, b = f0.astype(np.float64)[:, None], w.astype(np.float64)[None], b.astype(np.float64)[None]
    assert (np.abs(got - (f * w + b)) <= EPS * (np.abs(f * w) + np.abs(b))).all()
    assert np.array_equal(got[f0 == 0.0], np.repeat(b, int((f0 == 0.0).sum()), 0))  # f0 = 0 gives exactly b


@pytest.mark.parametrize("with_spk", [True, False], ids=["spk", "nospk"])
@pytest.mark.parametrize("dim, lin", [(48, 16), (768, 256)])
def test_f0_front_end_token_columns_bit_exact(built_lib, cuda_device, dim, lin, with_spk):
    rs = np.random.RandomState(dim + with_spk)
    num_embs = 29
    emb = torch.from_numpy(rs.standard_normal((num_embs, dim)).astype(np.float32)).to(cuda_device)
    spk = torch.from_numpy(rs.standard_normal((5, dim)).astype(np.float32)).to(cuda_device) if with_spk else None
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    for counts, speakers in (([1, 7, 33], [4, 0, 2]), ([7, 1, 33], [0, 4, 1]), ([33, 7, 1], [3, 2, 4])):
        rows = sum(counts)
        ids_h = rs.randint(0, num_embs, size=rows).astype(np.int64)
        ids_h[0], ids_h[-1] = num_embs - 1, 0
        ids, g = _i64(ids_h, cuda_device), _i64(speakers, cuda_device)
        f0, w, b, (f0_d, w_d, b_d) = _f0_inputs(rs, rows, lin, cuda_device)
        out = _embed_f0(built_lib, emb, None, spk, ids, g, counts, f0_d, w_d, b_d, flag)
        want = emb[ids]
        if with_spk:
            want = want + spk[torch.repeat_interleave(g, _i64(counts, cuda_device))]
        assert torch.equal(out[:, :dim], want), counts
        _check_f0_columns(out, dim, f0, w, b)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("dim, lin", [(48, 16), (768, 0)])
@pytest.mark.parametrize("n_tables", [3, 12])
def test_f0_front_end_weighted_sum(built_lib, cuda_device, n_tables, dim, lin):
    """sum_l w_l emb_l[ids[r, l]] within L 2^-23 sum_l |w_l e_l| of the float64 sum (the dot-product
    rounding bound); with lin = 0 there are no f0 columns."""
    rs = np.random.RandomState(n_tables * dim)
    num_embs = 23
    emb_h = rs.standard_normal((n_tables, num_embs, dim)).astype(np.float32)
    tw_h = rs.standard_normal(n_tables).astype(np.float32)
    emb, tw = torch.from_numpy(emb_h).to(cuda_device), torch.from_numpy(tw_h).to(cuda_device)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    counts = [7, 1, 33]
    rows = sum(counts)
    ids_h = rs.randint(0, num_embs, size=(rows, n_tables)).astype(np.int64)
    ids_h[0, :], ids_h[-1, :] = num_embs - 1, 0
    f0 = w = b = f0_d = w_d = b_d = None
    if lin:
        f0, w, b, (f0_d, w_d, b_d) = _f0_inputs(rs, rows, lin, cuda_device)
    out = _embed_f0(built_lib, emb, tw, None, _i64(ids_h, cuda_device), None, counts, f0_d, w_d, b_d, flag)
    assert out.shape == (rows, dim + lin) and int(flag.item()) == 0
    terms = np.stack([tw_h[l].astype(np.float64) * emb_h[l].astype(np.float64)[ids_h[:, l]] for l in range(n_tables)])
    got = out[:, :dim].cpu().numpy().astype(np.float64)
    assert (np.abs(got - terms.sum(0)) <= n_tables * EPS * np.abs(terms).sum(0)).all()
    if lin:
        _check_f0_columns(out, dim, f0, w, b)


def test_f0_front_end_flags(built_lib, cuda_device):
    """Ids one past either end of their table (tables in the middle of larger tensors): the row is
    zeros over all dim + lin columns, the other rows are exact, the flag holds exactly the bits."""
    rs = np.random.RandomState(3)
    emb = torch.from_numpy(rs.standard_normal((13, 48)).astype(np.float32)).to(cuda_device)[1:12]
    spk = torch.from_numpy(rs.standard_normal((7, 48)).astype(np.float32)).to(cuda_device)[1:6]
    embs = torch.from_numpy(rs.standard_normal((5, 11, 48)).astype(np.float32)).to(cuda_device)[1:4]
    tw = torch.from_numpy(rs.standard_normal(3).astype(np.float32)).to(cuda_device)
    counts = [3, 6, 2]
    f0, w, b, (f0_d, w_d, b_d) = _f0_inputs(rs, 11, 16, cuda_device)
    ids_h = rs.randint(0, 11, size=(11, 3)).astype(np.int64)
    g_h = np.asarray([1, 3, 0], np.int64)
    utt = np.repeat(np.arange(3), counts)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    ref1 = _embed_f0(built_lib, emb, None, spk, _i64(ids_h[:, 0].copy(), cuda_device), _i64(g_h, cuda_device), counts,
                     f0_d, w_d, b_d, flag)
    ref3 = _embed_f0(built_lib, embs, tw, None, _i64(ids_h, cuda_device), None, counts, f0_d, w_d, b_d, flag)
    assert int(flag.item()) == 0
    for bad_tok, bad_spk, bits in (({4: 11}, {}, 1), ({}, {2: 5}, 2), ({0: -1, 10: 11}, {1: -1}, 3)):
        ids, g = ids_h[:, 0].copy(), g_h.copy()
        for k, v in bad_tok.items():
            ids[k] = v
        for k, v in bad_spk.items():
            g[k] = v
        flag.zero_()
        out = _embed_f0(built_lib, emb, None, spk, _i64(ids, cuda_device), _i64(g, cuda_device), counts, f0_d, w_d, b_d,
                        flag)
        zero = np.asarray([r in bad_tok or utt[r] in bad_spk for r in range(11)])
        zero, rest = _mask(zero, cuda_device), _mask(~zero, cuda_device)
        assert int(flag.item()) == bits and not out[zero].any() and torch.equal(out[rest], ref1[rest])
    for l, bad_id in ((0, -1), (2, 11)):
        ids = ids_h.copy()
        ids[5, l] = bad_id
        flag.zero_()
        out = _embed_f0(built_lib, embs, tw, None, _i64(ids, cuda_device), None, counts, f0_d, w_d, b_d, flag)
        keep = _mask(np.arange(11) != 5, cuda_device)
        assert int(flag.item()) == 1 and not out[5].any() and torch.equal(out[keep], ref3[keep])


# ------------------------------------------------------------------ whole generators
_MODULES = {}


def _module(g, device):
    """One module per (config, bias override) for the whole file: the engines are built once."""
    key = (g["meta"]["vocoder"], None if "linear_bias" not in g else float(g["linear_bias"][0]))
    if key not in _MODULES:
        _MODULES[key] = golden_module(g)[0].to(device)
    return _MODULES[key]


def _run_golden(m, g, device):
    meta, c = g["meta"], g["c"]
    with torch.no_grad():
        if "dur" not in g:
            return m.inference(c, g["f0"]).cpu().numpy(), None
        if meta["mode"] == "forward":
            y, log_d = m(torch.from_numpy(c).to(device), torch.from_numpy(g["dur"]).to(device))
            return y.cpu().numpy(), log_d.cpu().numpy()
        ds = g["dur"] if "ds" in meta["options"] else None
        return m.inference(c, ds=ds).cpu().numpy(), None


@pytest.mark.parametrize("name", DURATION_GOLDEN + F0_GOLDEN)
def test_parity_with_reference_fixture(built_lib, cuda_device, name):
    """The reference's output shape exactly (so: its durations exactly) and max|d| < ATOL; the
    predicted integer durations and the forward's log durations are the reference's."""
    g = load_var_golden(name)
    m = _module(g, cuda_device)
    y, log_d = _run_golden(m, g, cuda_device)
    assert y.shape == g["y"].shape and np.isfinite(y).all()
    err = float(np.abs(y - g["y"]).max())
    print(f"{name}: max|d| = {err:.2e}")
    assert err < ATOL
    if "dur" in g and "ds" not in g["meta"]["options"]:
        with torch.no_grad():
            (d,) = m.predict_durations([g["c"]])
        assert d.dtype == torch.int64 and np.array_equal(d.cpu().numpy(), g["dur"])
    if log_d is not None:
        assert log_d.shape == g["logdur"].shape
        # (the kernel is within 4 x logdur_ref_err of float64, the reference within 1 x)
        assert float(np.abs(log_d - g["logdur"]).max()) <= 5.0 * float(g["logdur_ref_err"])


def test_duration_ragged_batch_and_input_forms(built_lib, cuda_device):
    """inference_batch on a ragged batch equals per-utterance inference bit for bit; numpy, float CPU
    tensor and device tensor ids agree bit for bit, so do host- and device-resident durations; and
    inference(c, ds=predict_durations(c)) equals inference(c) bit for bit."""
    g = load_var_golden("dsym_duration_pred_T12")
    m = _module(g, cuda_device)
    rs = np.random.RandomState(4)
    cs = [rs.randint(0, 12, size=(T, 1)).astype(np.int64) for T in (5, 1, 12, 3)]
    cs[2] = g["c"]
    with torch.no_grad():
        ys = m.inference_batch(cs)
        ds = m.predict_durations(cs)
        assert [tuple(d.shape) for d in ds] == [(5,), (1,), (12,), (3,)]
        for c, d, y in zip(cs, ds, ys):
            y1 = m.inference(c)
            total = int(d.sum()) or len(c)
            assert y1.shape == (total * 8, 1) and torch.equal(y, y1)
            assert torch.equal(m.inference(c, ds=d), y1)                    # device-resident durations
            assert torch.equal(m.inference(c, ds=d.cpu().numpy()), y1)      # host-resident: no read-back
            assert torch.equal(m.inference(torch.from_numpy(c).float(), ds=d.cpu()), y1)
            assert torch.equal(m.inference(torch.from_numpy(c).to(cuda_device)), y1)
            assert torch.equal(m.inference(torch.from_numpy(c).to(cuda_device).float() + 0.75), y1)
        for a, b in zip(m.inference_batch(cs, ds=ds), ys):
            assert torch.equal(a, b)
        for a, b in zip(m.inference_batch(cs, ds=[d.cpu().numpy() for d in ds]), ys):
            assert torch.equal(a, b)
    assert np.array_equal(ds[2].cpu().numpy(), g["dur"])


def test_f0_ragged_batch_and_input_forms(built_lib, cuda_device):
    g = load_var_golden("dsym_f0_spk_T7")
    m = _module(g, cuda_device)
    c, f0 = g["c"], g["f0"]
    rs = np.random.RandomState(6)
    cs = [np.stack([rs.randint(0, 11, size=T), np.full(T, s)], 1).astype(np.int64) for T, s in ((4, 0), (1, 4))] + [c]
    f0s = [rs.uniform(0, 6, size=len(x)).astype(np.float32) for x in cs[:2]] + [f0]
    with torch.no_grad():
        ys = m.inference_batch(cs, f0s)
        for x, f, y in zip(cs, f0s, ys):
            assert torch.equal(m.inference(x, f), y)
        y0 = ys[2]
        dev_c, dev_f = torch.from_numpy(c).to(cuda_device), torch.from_numpy(f0).to(cuda_device)
        for cf, ff in ((torch.from_numpy(c).float(), torch.from_numpy(f0)), (dev_c, dev_f), (dev_c.float() + 0.75, f0),
                       (c, dev_f)):
            assert torch.equal(m.inference(cf, ff), y0)
        assert torch.equal(m.inference(c[:, :1], f0, g=int(c[0, 1])), y0)
        fwd = m(torch.from_numpy(c.T[None]).to(cuda_device), dev_f[None, None])
        assert torch.equal(fwd[0].transpose(0, 1), y0)
    w = load_var_golden("dsym_f0_wsum_T6")
    mw = _module(w, cuda_device)
    with torch.no_grad():
        yw = mw.inference(w["c"], w["f0"])
        assert torch.equal(mw.inference(torch.from_numpy(w["c"]).to(cuda_device), torch.from_numpy(w["f0"])), yw)
        assert torch.equal(mw(torch.from_numpy(w["c"].T[None]), torch.from_numpy(w["f0"])[None, None])[0].transpose(0, 1),
                           yw)


def test_invalid_ids_on_device_raise_and_modules_recover(built_lib, cuda_device):
    """One id one past its table in a device tensor (nothing is checked on the host): IndexError
    through the flag word, and the next valid call on the same module gives the fixture's result."""
    g = load_var_golden("dsym_duration_pred_T12")
    m = _module(g, cuda_device)
    c = g["c"].copy()
    c[5, 0] = 12  # num_embs + 1 (11 is the valid padding row)
    bad = torch.from_numpy(c).to(cuda_device)
    with torch.no_grad():
        for call in (lambda: m.inference(bad), lambda: m.predict_durations([bad]),
                     lambda: m.inference(bad, ds=np.ones(12, np.int64))):
            with pytest.raises(IndexError, match="a token id outside"):
                call()
        with pytest.raises(ValueError, match="a duration outside"):
            m.inference(g["c"], ds=torch.tensor([1] * 11 + [-2], device=cuda_device))
        y = m.inference(torch.from_numpy(g["c"]).to(cuda_device)).cpu().numpy()
    assert y.shape == g["y"].shape and float(np.abs(y - g["y"]).max()) < ATOL
    f = load_var_golden("dsym_f0_spk_T7")
    mf = _module(f, cuda_device)
    for what in ("token", "speaker"):
        c = f["c"].copy()
        if what == "token":
            c[3, 0] = 11
        else:
            c[:, 1] = 5
        with torch.no_grad():
            with pytest.raises(IndexError, match=f"a {what} id outside"):
                mf.inference(torch.from_numpy(c).to(cuda_device), f["f0"])
            y = mf.inference(torch.from_numpy(f["c"]).to(cuda_device), f["f0"]).cpu().numpy()
        assert float(np.abs(y - f["y"]).max()) < ATOL


def test_batch_beyond_one_plan_raises_before_allocating(built_lib, cuda_device):
    g = load_var_golden("dsym_duration_pred_T12")
    m = _module(g, cuda_device)
    c = np.zeros((2, 1), np.int64)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(cuda_device)
    with pytest.raises(ValueError, match="utterance 1 brings the batch"):
        m.inference_batch([c, c], ds=[np.asarray([3, 1]), np.asarray([1 << 30, 1 << 30])])
    with pytest.raises(ValueError, match="utterance 0 brings the batch"):
        m.inference(c, ds=torch.tensor([1 << 30, 1 << 30], device=cuda_device))
    assert torch.cuda.memory_allocated(cuda_device) - before < (1 << 20)


# ------------------------------------------------------------------ decode CLI
def _checkpoint(tmp_path, cfg, linear_bias=None):
    cls, params = configs.vocoder_params(cfg)
    m, _, _ = var_module(cfg, seed=4, linear_bias=linear_bias)
    ckpt = str(tmp_path / "checkpoint-10steps.pkl")
    torch.save({"model": {"generator": {k: v.clone() for k, v in m.state_dict().items()}}, "steps": 10}, ckpt)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(dict(generator_type=cls, generator_params=params, sampling_rate=16000, format="npy",
                            version="0.6.1"), f)
    return ckpt, m


@pytest.mark.parametrize("batch", ["20", None], ids=["batch20", "auto"])
def test_decode_cli_duration(built_lib, cuda_device, tmp_path, batch):
    from parallelwavegan_amd.bin import decode

    ckpt, m = _checkpoint(tmp_path, "dsym_duration_test", linear_bias=1.0)
    m.remove_weight_norm()
    m = m.to(cuda_device)
    dump = tmp_path / "dump"
    dump.mkdir()
    rs = np.random.RandomState(12)
    feats = {u: rs.randint(0, 12, size=(T, 1)).astype(np.float32) for u, T in (("utt_a", 9), ("utt_b", 23), ("utt_c", 5))}
    for u, c in feats.items():
        np.save(dump / f"{u}-feats.npy", c)  # float ids, as the recipes dump them
    out = tmp_path / "wav"
    argv = ["--dumpdir", str(dump), "--outdir", str(out), "--checkpoint", ckpt, "--verbose", "0"]
    assert decode.main(argv + (["--batch-frames", batch] if batch else [])) == 0
    for u, c in feats.items():
        with torch.no_grad():
            (d,) = m.predict_durations([c])
            y = m.inference(c).view(-1).cpu().numpy()
        z, sr = read_pcm16_wav(str(out / f"{u}_gen.wav"))
        assert sr == 16000 and z.shape == ((int(d.sum()) or len(c)) * 8,)
        np.testing.assert_allclose(z, y, atol=1.0 / 32767)
    with pytest.raises(NotImplementedError, match="--use-f0"):
        decode.main(argv + ["--use-f0"])


def test_decode_cli_f0(built_lib, cuda_device, tmp_path):
    from parallelwavegan_amd.bin import decode

    ckpt, m = _checkpoint(tmp_path, "dsym_f0_spk_test")
    m.remove_weight_norm()
    m = m.to(cuda_device)
    dump = tmp_path / "dump"
    dump.mkdir()
    rs = np.random.RandomState(13)
    feats, f0s = {}, {}
    for u, (T, s) in {"utt_a": (9, 1), "utt_b": (23, 4), "utt_c": (5, 0)}.items():
        feats[u] = np.stack([rs.randint(0, 11, size=T), np.full(T, s)], 1).astype(np.float32)
        f0s[u] = rs.uniform(0, 6, size=T).astype(np.float32)
        np.save(dump / f"{u}-feats.npy", feats[u])
        np.save(dump / f"{u}-f0.npy", f0s[u])
    out = tmp_path / "wav"
    argv = ["--dumpdir", str(dump), "--outdir", str(out), "--checkpoint", ckpt, "--verbose", "0"]
    assert decode.main(argv + ["--use-f0", "--batch-frames", "20"]) == 0
    for u, c in feats.items():
        z, sr = read_pcm16_wav(str(out / f"{u}_gen.wav"))
        assert sr == 16000 and z.shape == (len(c) * 8,)
        with torch.no_grad():
            y = m.inference(c, f0s[u]).view(-1).cpu().numpy()
        np.testing.assert_allclose(z, y, atol=1.0 / 32767)
    with pytest.raises(ValueError, match="--use-f0"):
        decode.main(argv)
