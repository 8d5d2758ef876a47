"""VQVAE on the GPU: every entry point of include/pwg_vq.h alone against the float64 oracle, and the
drop-in's encode / decode / forward / ragged batches against the fixtures of tests/golden/vqvae under
the index parity rule of tests/vqvae_oracle.index_rule. Every case prints its figures before it asserts."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vqvae_oracle
from parallelwavegan_amd import _lib, configs
from vqvae_helpers import EXPECTED, WITH_Y, fixture_module, load_fixture, utterances

pytestmark = pytest.mark.gpu
FORWARD = ("vq_a_fwd_B3_T64", "vq_v3_fwd_B1_T256")


def _dev(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def _starts(lens):
    s = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=s[1:])
    return s


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


_GPU_MODULES = {}


def gpu_module(meta, dev):
    """The fixture's drop-in on the GPU (a module of its own: the host tests keep theirs on the CPU)."""
    from parallelwavegan_amd import VQVAE

    m, params, folded = fixture_module(meta)
    if id(m) not in _GPU_MODULES:
        g = VQVAE(**configs.vqvae_params(meta["config"]))
        g.load_state_dict(m.state_dict(), strict=True)
        _GPU_MODULES[id(m)] = g.eval().to(dev)
    return _GPU_MODULES[id(m)], params, folded


# ---------------------------------------------------------------------------------------------- kernels
def test_wave_rows_ragged(built_lib, cuda_device):
    """[8, 61, 23] samples: the boundaries fall inside one workgroup's rows (64 rows per workgroup at
    16 channels); 8 samples is the shortest legal utterance (7 mirrored on either side)."""
    L, dev = built_lib, cuda_device
    meta = load_fixture("vq_a_T61")["meta"]
    _, params, folded = fixture_module(meta)
    lens = [8, 61, 23]
    rs = np.random.RandomState(5)
    xs = [(0.3 * rs.standard_normal(n)).astype(np.float32) for n in lens]
    w, b = folded["encoder.layers.0.1.weight"], folded["encoder.layers.0.1.bias"]
    C, K = w.shape[0], w.shape[2]
    host = _starts(lens)
    rows = int(host[-1])
    out = torch.full((rows, C), float("nan"), device=dev)
    x_d, w_d, b_d, rs_d = _dev(np.concatenate(xs), dev), _dev(w.reshape(C, K), dev), _dev(b, dev), _dev(host, dev, torch.int64)
    _lib.check(L.pwg_vq_wave_rows(x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), C, K, ctypes.c_float(0.2),
                                  rs_d.data_ptr(), host.ctypes.data, len(lens), rows, out.data_ptr(), _stream(dev)))
    got = out.cpu().numpy()
    for u, x in enumerate(xs):
        taps = []
        vqvae_oracle.encoder(x, folded, params["encoder_conf"], torch.float64, taps=taps)
        err = float(np.abs(got[host[u]:host[u + 1]] - taps[0].numpy()).max())
        print(f"wave_rows utterance {u} ({lens[u]} samples): max|d| = {err:.2e}")
        assert err < 1e-5


def _gsconv(L, dev, x, lens_in, wp, b, cin, cout, s, slope):
    lens_out = [(n + s - 1) // s for n in lens_in]
    hi, ho = _starts(lens_in), _starts(lens_out)
    y = torch.full((int(ho[-1]), cout), float("nan"), device=dev)
    rs_i, rs_o = _dev(hi, dev, torch.int64), _dev(ho, dev, torch.int64)
    _lib.check(L.pwg_vq_gsconv(x.data_ptr(), rs_i.data_ptr(), int(hi[-1]), cin, wp.data_ptr(),
                               b.data_ptr() if b is not None else None, cout, s, ctypes.c_float(slope), y.data_ptr(),
                               rs_o.data_ptr(), int(ho[-1]), len(lens_in), _stream(dev)))
    torch.cuda.synchronize(dev)
    return y, lens_out, ho


@pytest.mark.parametrize("cin, cout, s, bias", [(16, 64, 4, True), (64, 64, 2, True), (16, 32, 2, False), (32, 64, 3, True),
                                                (256, 512, 2, True)])
def test_gsconv_ragged(built_lib, cuda_device, cin, cout, s, bias):
    """16, 4, 8, 8 and 8 outputs per group at s = 4, 2, 2, 3, 2 (the last with 16 channel blocks); row
    counts 300, 131, 5, 64 are no multiples of s or of the 64-column tile, 300 and 131 span two tiles."""
    L, dev = built_lib, cuda_device
    rs = np.random.RandomState(cin + cout + s)
    K = 10 * s + 1
    lens = [300, 131, 5, 64]
    w = (rs.standard_normal((cout, 4, K)) / np.sqrt(4 * K)).astype(np.float32)
    b = (0.05 * rs.standard_normal(cout)).astype(np.float32) if bias else None
    xs = [rs.standard_normal((n, cin)).astype(np.float32) for n in lens]
    packed = np.empty(L.pwg_vq_gsconv_packed_count(cin, cout, s), np.float32)
    _lib.check(L.pwg_vq_gsconv_pack(w.ctypes.data, cin, cout, s, packed.ctypes.data))
    wp, b_d = _dev(packed, dev), (_dev(b, dev) if bias else None)
    y, lens_out, ho = _gsconv(L, dev, _dev(np.concatenate(xs), dev), lens, wp, b_d, cin, cout, s, 0.2)
    assert lens_out == [-(-n // s) for n in lens]
    got = y.cpu().numpy()
    for u, x in enumerate(xs):
        ref = F.leaky_relu(F.conv1d(torch.from_numpy(x).double().T.unsqueeze(0), torch.from_numpy(w).double(),
                                    torch.from_numpy(b).double() if bias else None, stride=s, padding=5 * s,
                                    groups=cin // 4), 0.2)[0].T.numpy()
        assert ref.shape[0] == lens_out[u]  # the reference's floor((T - 1) / s) + 1 is the ceil chain
        err = float(np.abs(got[ho[u]:ho[u + 1]] - ref).max())
        print(f"gsconv {cin}->{cout} s={s} utterance {u} ({lens[u]} -> {lens_out[u]} rows): max|d| = {err:.2e}")
        assert err < 1e-5
    # an utterance's rows do not depend on its neighbours' contents
    other = [x if u == 1 else rs.standard_normal(x.shape).astype(np.float32) * 3 for u, x in enumerate(xs)]
    y2, _, _ = _gsconv(L, dev, _dev(np.concatenate(other), dev), lens, wp, b_d, cin, cout, s, 0.2)
    assert torch.equal(y[ho[1]:ho[2]], y2[ho[1]:ho[2]])
    assert not torch.equal(y[ho[0]:ho[1]], y2[ho[0]:ho[1]])
    # slope 1.0: no activation
    y3, _, _ = _gsconv(L, dev, _dev(xs[2], dev), lens[2:3], wp, b_d, cin, cout, s, 1.0)
    ref = F.conv1d(torch.from_numpy(xs[2]).double().T.unsqueeze(0), torch.from_numpy(w).double(),
                   torch.from_numpy(b).double() if bias else None, stride=s, padding=5 * s, groups=cin // 4)[0].T.numpy()
    assert float(np.abs(y3.cpu().numpy() - ref).max()) < 1e-5


def _nearest(L, dev, z, book, want_zq=True):
    z_d, e_d = _dev(z, dev), _dev(book, dev)
    rows, D = z.shape
    N = book.shape[0]
    en = torch.empty(N, device=dev)
    idx = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    zq = torch.full((rows, D), float("nan"), device=dev) if want_zq else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.pwg_vq_code_norms(e_d.data_ptr(), N, D, en.data_ptr(), _stream(dev)))
    _lib.check(L.pwg_vq_nearest(z_d.data_ptr(), rows, D, e_d.data_ptr(), en.data_ptr(), N, idx.data_ptr(),
                                zq.data_ptr() if want_zq else None, flag.data_ptr(), _stream(dev)))
    return idx.cpu().numpy(), (zq.cpu().numpy() if want_zq else None), int(flag.item())


def _fixture_rows(fx):
    z = fx["z_e"]
    return z.transpose(0, 2, 1).reshape(-1, z.shape[1]), fx["idx"].reshape(-1)


@pytest.mark.parametrize("name", EXPECTED)
def test_nearest_on_fixture_rows(built_lib, cuda_device, name):
    fx = load_fixture(name)
    _, _, folded = fixture_module(fx["meta"])
    book = folded["codebook.embedding.weight"]
    z, ref_idx = _fixture_rows(fx)
    idx, zq, flag = _nearest(built_lib, cuda_device, z, book)
    assert flag == 0 and idx.min() >= 0 and idx.max() < book.shape[0]
    viol, under, mism = vqvae_oracle.index_rule(z, book, idx, ref_idx)
    print(f"nearest {name}: {len(idx)} rows, violations {viol}, under tau {under}, mismatches on clear rows {mism}, "
          f"differing from the reference {int((idx != ref_idx).sum())}")
    assert viol == 0 and mism == 0 and under <= vqvae_oracle.cap(len(idx))
    np.testing.assert_array_equal(zq, book[idx])
    if fx["meta"]["dup"]:
        lo, hi = fx["meta"]["dup"]
        assert (idx == lo).sum() == fx["meta"]["dup_hits"] and not (idx == hi).any()  # the lower index wins


@pytest.mark.parametrize("rows, D, N", [(37, 32, 48), (37, 32, 33), (64, 256, 512), (5, 16, 1), (17, 1024, 19)])
def test_nearest_random_rows(built_lib, cuda_device, rows, D, N):
    """Rows spread over the whole codebook (the fixtures' frames share a few codes); N = 33 and 48 are no
    multiples of the 16-code tile, N = 1 and 19 leave waves without a tile; a NaN row and an infinite one
    give index 0 and the flag."""
    rs = np.random.RandomState(rows + D + N)
    book = rs.standard_normal((N, D)).astype(np.float32)
    z = (book[rs.randint(N, size=rows)] + 0.3 * rs.standard_normal((rows, D))).astype(np.float32)
    idx, zq, flag = _nearest(built_lib, cuda_device, z, book)
    ref = vqvae_oracle.nearest(torch.from_numpy(z).double(), torch.from_numpy(book).double()).numpy()
    viol, under, mism = vqvae_oracle.index_rule(z, book, idx, ref)
    print(f"nearest random {rows}x{D}, N={N}: distinct {len(np.unique(idx))}, violations {viol}, under tau {under}, "
          f"mismatches {mism}")
    assert flag == 0 and idx.min() >= 0 and idx.max() < N
    assert viol == 0 and mism == 0 and under <= vqvae_oracle.cap(rows)
    np.testing.assert_array_equal(zq, book[idx])
    bad = z.copy()
    bad[1, 3] = np.nan
    bad[rows - 1, D - 1] = np.inf
    idx2, _, flag2 = _nearest(built_lib, cuda_device, bad, book, want_zq=False)
    assert flag2 == _lib.PWG_VQ_BAD_INPUT and idx2[1] == 0 and idx2[rows - 1] == 0
    keep = np.ones(rows, bool)
    keep[[1, rows - 1]] = False
    np.testing.assert_array_equal(idx2[keep], idx[keep])
    assert idx2.min() >= 0 and idx2.max() < N


def _decode_rows(L, dev, book, idx, local, wl, bl, glob, gids, lens):
    rows = int(sum(lens))
    D = book.shape[1]
    Ld = (wl.shape[0] if wl is not None else local.shape[1]) if local is not None else 0
    G = glob.shape[1] if glob is not None else 0
    out = torch.full((rows, D + Ld + G), float("nan"), device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    t = dict(book=_dev(book, dev), idx=_dev(idx, dev, torch.int64), rs=_dev(_starts(lens), dev, torch.int64))
    for k, v, dt in (("local", local, torch.float32), ("wl", wl, torch.float32), ("bl", bl, torch.float32),
                     ("glob", glob, torch.float32), ("gids", gids, torch.int64)):
        t[k] = _dev(v, dev, dt) if v is not None else None

    def p(k):
        return t[k].data_ptr() if t[k] is not None else None

    _lib.check(L.pwg_vq_decode_rows(p("book"), book.shape[0], D, p("idx"), p("local"), local.shape[1] if local is not None else 0,
                                    p("wl"), p("bl"), Ld, p("glob"), glob.shape[0] if glob is not None else 0, G, p("gids"),
                                    p("rs"), len(lens), rows, out.data_ptr(), flag.data_ptr(), _stream(dev)))
    return out.cpu().numpy(), int(flag.item())


def test_decode_rows(built_lib, cuda_device):
    L, dev = built_lib, cuda_device
    meta = load_fixture("vq_a_T61")["meta"]
    _, _, folded = fixture_module(meta)
    book, glob = folded["codebook.embedding.weight"], folded["global_embed.weight"]
    wl, bl = folded["local_embed.weight"][:, :, 0], folded["local_embed.bias"]
    rs = np.random.RandomState(9)
    lens = [8, 1, 25, 3]
    rows = sum(lens)
    idx = rs.randint(book.shape[0], size=rows).astype(np.int64)
    local = rs.standard_normal((rows, 2)).astype(np.float32)
    gids = np.asarray([3, 0, 4, 1], np.int64)
    D, Ld = book.shape[1], wl.shape[0]
    out, flag = _decode_rows(L, dev, book, idx, local, wl, bl, glob, gids, lens)
    assert flag == 0
    np.testing.assert_array_equal(out[:, :D], book[idx])
    np.testing.assert_array_equal(out[:, D + Ld:], glob[np.repeat(gids, lens)])
    ref = local.astype(np.float64) @ wl.astype(np.float64).T + bl.astype(np.float64)
    err = float(np.abs(out[:, D:D + Ld] - ref).max())
    print(f"decode_rows local projection: max|d| = {err:.2e}")
    assert err < 1e-6
    # each part alone, and local rows copied when there is no projection
    o, _ = _decode_rows(L, dev, book, idx, None, None, None, None, None, lens)
    np.testing.assert_array_equal(o, book[idx])
    wide = rs.standard_normal((rows, 16)).astype(np.float32)
    o, _ = _decode_rows(L, dev, book, idx, wide, None, None, glob, gids, lens)
    np.testing.assert_array_equal(o, np.concatenate([book[idx], wide, glob[np.repeat(gids, lens)]], 1))
    # a code id of N and a global id of -1: zero rows, their flag bits, no other row changed
    bad_idx = idx.copy()
    bad_idx[10] = book.shape[0]
    bad_g = gids.copy()
    bad_g[3] = -1
    o, flag = _decode_rows(L, dev, book, bad_idx, local, wl, bl, glob, bad_g, lens)
    assert flag == _lib.PWG_VQ_BAD_CODE | _lib.PWG_VQ_BAD_GLOBAL
    zero = np.zeros(rows, bool)
    zero[10] = True
    zero[rows - 3:] = True
    assert not o[zero].any()
    np.testing.assert_array_equal(o[~zero], out[~zero])
    _, flag = _decode_rows(L, dev, book, bad_idx, local, wl, bl, glob, gids, lens)
    assert flag == _lib.PWG_VQ_BAD_CODE


# ---------------------------------------------------------------------------------------------- the model
def _check_encode(name, z_ref, book, idx_ref, z_gpu, idx_gpu):
    ez = float(np.abs(z_gpu - z_ref).max())
    viol, under, mism = vqvae_oracle.index_rule(z_ref, book, idx_gpu, idx_ref, z_used=z_gpu)
    print(f"encode {name}: {len(idx_gpu)} frames, max|z - z_e| = {ez:.2e}, violations {viol}, under allowance {under}, "
          f"mismatches on clear frames {mism}, differing from the reference {int((idx_gpu != idx_ref).sum())}")
    assert ez < 1e-4
    assert viol == 0 and mism == 0 and under <= vqvae_oracle.cap(len(idx_gpu))


@pytest.mark.parametrize("name", EXPECTED)
def test_encode_fixture(built_lib, cuda_device, name):
    fx = load_fixture(name)
    m, params, folded = gpu_module(fx["meta"], cuda_device)
    x = torch.from_numpy(fx["x"]).to(cuda_device)
    with torch.no_grad():
        idx = m.encode(x)
        keep = {}
        z, idx_rows, _, frames = m._encode_rows([x[b, 0] for b in range(x.size(0))], keep=keep)
    assert idx.shape == fx["idx"].shape and idx.dtype == torch.int64
    assert torch.equal(idx.reshape(-1), idx_rows)
    # every level is packed at its true length: the ceil chain
    n = fx["x"].shape[2]
    for (rows, lens), s in zip(keep["levels"], (1,) + tuple(params["encoder_conf"]["downsample_scales"])):
        n = -(-n // s)
        assert lens == [n] * x.size(0) and rows.numel() % sum(lens) == 0
    assert frames == [fx["meta"]["frames"]] * x.size(0)
    z_ref, idx_ref = (fx["z_e"].transpose(0, 2, 1).reshape(-1, fx["z_e"].shape[1]), fx["idx"].reshape(-1))
    _check_encode(name, z_ref, folded["codebook.embedding.weight"], idx_ref, z.cpu().numpy(), idx_rows.cpu().numpy())


@pytest.mark.parametrize("fixture, lens", [("vq_a_T61", [8, 61, 200, 23]), ("vq_b_T131", [9, 131])])
def test_encode_ragged_batch(built_lib, cuda_device, fixture, lens):
    """Against per-utterance float64 oracle runs, and bitwise against per-utterance GPU runs."""
    meta = load_fixture(fixture)["meta"]
    m, params, folded = gpu_module(meta, cuda_device)
    book = folded["codebook.embedding.weight"]
    rs = np.random.RandomState(31)
    xs = [(0.3 * rs.standard_normal(n)).astype(np.float32) for n in lens]
    hop = int(np.prod(params["encoder_conf"]["downsample_scales"]))
    with torch.no_grad():
        z, idx, _, frames = m._encode_rows(xs)
        idxs = m.encode_batch(xs)
    assert frames == [-(-n // hop) for n in lens]
    assert [tuple(i.shape) for i in idxs] == [(f,) for f in frames] and torch.equal(torch.cat(idxs), idx)
    z_ref = np.concatenate([vqvae_oracle.encoder(x, folded, params["encoder_conf"], torch.float64).numpy() for x in xs])
    idx_ref = vqvae_oracle.nearest(torch.from_numpy(z_ref), torch.from_numpy(book).double()).numpy()
    _check_encode(f"{fixture} ragged {lens}", z_ref, book, idx_ref, z.cpu().numpy(), idx.cpu().numpy())
    off = 0
    for x, f in zip(xs, frames):
        with torch.no_grad():
            z1, idx1, _, _ = m._encode_rows([x])
        assert torch.equal(z1, z[off:off + f]) and torch.equal(idx1, idx[off:off + f])
        off += f


@pytest.mark.parametrize("name", WITH_Y)
def test_decode_fixture(built_lib, cuda_device, name):
    fx = load_fixture(name)
    m, _, _ = gpu_module(fx["meta"], cuda_device)
    dev = cuda_device
    l = torch.from_numpy(fx["l"]).to(dev) if fx["l"].size else None
    g = torch.from_numpy(fx["g"]).to(dev) if fx["g"].size else None
    with torch.no_grad():
        y = m.decode(torch.from_numpy(fx["idx"]).to(dev), l, g)
    assert tuple(y.shape) == fx["y"].shape
    err = float(np.abs(y.cpu().numpy() - fx["y"]).max())
    print(f"decode {name}: max|y - y_ref| = {err:.2e} over {y.numel()} samples")
    assert err < 1e-4


@pytest.mark.parametrize("name", FORWARD)
def test_forward_fixture(built_lib, cuda_device, name):
    fx = load_fixture(name)
    m, params, folded = gpu_module(fx["meta"], cuda_device)
    dev = cuda_device
    book = folded["codebook.embedding.weight"]
    l = torch.from_numpy(fx["l"]).to(dev) if fx["l"].size else None
    g = torch.from_numpy(fx["g"]).to(dev) if fx["g"].size else None
    with torch.no_grad():
        x_bar, z_e, z_q = m(torch.from_numpy(fx["x"]).to(dev), l, g)
        idx = m.encode(torch.from_numpy(fx["x"]).to(dev)).cpu().numpy()
    assert tuple(x_bar.shape) == fx["y"].shape and tuple(z_e.shape) == fx["z_e"].shape == tuple(z_q.shape)
    ez = float(np.abs(z_e.cpu().numpy() - fx["z_e"]).max())
    np.testing.assert_array_equal(z_q.cpu().numpy(), book[idx].transpose(0, 2, 1))
    hop = x_bar.shape[2] // idx.shape[1]
    same = np.repeat(idx == fx["idx"], hop, axis=1)[:, None, :]
    # x_bar against the reference where its frame's index matched, and everywhere against the float64
    # oracle decoding the indices the GPU chose
    err = float(np.abs(x_bar.cpu().numpy() - fx["y"])[same].max()) if same.all() else float("nan")
    own = []
    for b, (x, lu, gu, _, _, _) in enumerate(utterances(fx)):
        rows = vqvae_oracle.decoder_rows(idx[b], lu, gu, folded, torch.float64)
        own.append(vqvae_oracle.melgan_decoder(rows, folded, params["decoder_conf"], torch.float64).numpy().T)
    err_own = float(np.abs(x_bar.cpu().numpy() - np.stack(own)).max())
    print(f"forward {name}: max|z_e - ref| = {ez:.2e}, frames matching the reference {int((idx == fx['idx']).sum())} of "
          f"{idx.size}, max|x_bar - y_ref| = {err:.2e}, max|x_bar - oracle(own indices)| = {err_own:.2e}")
    assert ez < 1e-4 and err_own < 1e-4
    if same.all():
        assert err < 1e-4


@pytest.mark.parametrize("fixture, lens", [("vq_a_T61", [61, 200, 37, 64]), ("vq_b_T131", [131, 18])])
def test_inference_batch(built_lib, cuda_device, fixture, lens):
    """inference_batch equals decode_batch(encode_batch) bitwise, and the ragged batch equals
    per-utterance runs bitwise."""
    meta = load_fixture(fixture)["meta"]
    m, params, _ = gpu_module(meta, cuda_device)
    rs = np.random.RandomState(17)
    xs = [(0.3 * rs.standard_normal(n)).astype(np.float32) for n in lens]
    hop = int(np.prod(params["encoder_conf"]["downsample_scales"]))
    frames = [-(-n // hop) for n in lens]
    ls = gs = None
    if params.get("num_local_embeds") is not None:
        ls = [rs.standard_normal((f, params["num_local_embeds"])).astype(np.float32) for f in frames]
        gs = [int(v) for v in rs.randint(params["num_global_embeds"], size=len(lens))]
    with torch.no_grad():
        ys, idxs = m.inference_batch(xs, ls, gs)
        idxs2 = m.encode_batch(xs)
        ys2 = m.decode_batch(idxs2, ls, gs)
    for u, f in enumerate(frames):
        assert tuple(ys[u].shape) == (f * hop, 1) and tuple(idxs[u].shape) == (f,)
        assert torch.equal(idxs[u], idxs2[u]) and torch.equal(ys[u], ys2[u])
        with torch.no_grad():
            y1, i1 = m.inference_batch([xs[u]], None if ls is None else [ls[u]], None if gs is None else [gs[u]])
        assert torch.equal(i1[0], idxs[u]) and torch.equal(y1[0], ys[u])
        assert np.isfinite(ys[u].cpu().numpy()).all()


def test_input_errors(built_lib, cuda_device):
    meta = load_fixture("vq_a_T61")["meta"]
    m, _, _ = gpu_module(meta, cuda_device)
    with pytest.raises(ValueError, match="7 samples"):
        m.encode(torch.zeros(1, 1, 7, device=cuda_device))
    idx = torch.zeros(1, 8, dtype=torch.long, device=cuda_device)
    with pytest.raises(ValueError, match="local"):
        m.decode(idx, None, torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="global"):
        m.decode(idx, torch.zeros(1, 2, 8), None)
    mb, _, _ = gpu_module(load_fixture("vq_b_T131")["meta"], cuda_device)
    with pytest.raises(ValueError, match="local"):
        mb.decode(idx, torch.zeros(1, 2, 8), None)
    with pytest.raises(IndexError, match="code index"):
        mb.decode(torch.full((1, 8), 33, dtype=torch.long, device=cuda_device))
