"""DiscreteSymbolHiFiGANGenerator on the GPU: the embedding kernel alone (bit-exact against torch
indexing), parity with the reference fixtures, ragged batches against the CPU oracle, the
out-of-range flag for device-resident ids, and the decode CLI on a dump of unit ids."""

import numpy as np
import pytest
import torch
import yaml

from parallelwavegan_amd import _lib, configs
from parallelwavegan_amd.utils import load_model, read_pcm16_wav
from test_dsym_host import DSYM_GOLDEN, dsym_module, load_dsym_golden, oracle_features

pytestmark = pytest.mark.gpu

ATOL = 1e-4  # the project's parity bound (tests/test_gpu_vocoders.py)


def _embed(L, emb, spk, ids, spk_ids, frames, flag):
    dev = emb.device
    rows, dim = int(ids.numel()), emb.shape[1]
    row_start = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int64, device=dev)
    out = torch.full((rows, dim), float("nan"), device=dev)
    rc = L.pwg_embed_rows(emb.data_ptr(), emb.shape[0], spk.data_ptr() if spk is not None else None,
                          spk.shape[0] if spk is not None else 0, dim, ids.data_ptr(),
                          spk_ids.data_ptr() if spk is not None else None, row_start.data_ptr(), len(frames), rows,
                          out.data_ptr(), flag.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc)
    return out


@pytest.mark.parametrize("with_spk", [True, False], ids=["spk", "nospk"])
@pytest.mark.parametrize("dim, num_embs", [(48, 11), (512, 100), (768, 1025)])
def test_embed_kernel_bit_exact(built_lib, cuda_device, dim, num_embs, with_spk):
    """out = emb[ids] + spk[g(utterance)] equals torch indexing bit for bit; utterances of 1, 7 and
    33 rows in three orders (the single-row utterance first, in the middle, last: its rows sit in
    one wave's row group with a neighbour's), ids 0 and num_embs - 1 present, a different speaker
    per utterance (first and last table row included); no flag bit is set."""
    rs = np.random.RandomState(dim + with_spk)
    emb = torch.from_numpy(rs.standard_normal((num_embs, dim)).astype(np.float32)).to(cuda_device)
    spk = torch.from_numpy(rs.standard_normal((5, dim)).astype(np.float32)).to(cuda_device) if with_spk else None
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    for frames, speakers in (([1, 7, 33], [4, 0, 2]), ([7, 1, 33], [0, 4, 1]), ([33, 7, 1], [3, 2, 4])):
        ids_h = rs.randint(0, num_embs, size=sum(frames)).astype(np.int64)
        ids_h[0], ids_h[-1], ids_h[frames[0]] = num_embs - 1, 0, num_embs - 1
        ids = torch.from_numpy(ids_h).to(cuda_device)
        g = torch.tensor(speakers, dtype=torch.int64, device=cuda_device)
        out = _embed(built_lib, emb, spk, ids, g, frames, flag)
        want = emb[ids]
        if with_spk:
            want = want + spk[torch.repeat_interleave(g, torch.tensor(frames, device=cuda_device))]
        assert torch.equal(out, want), (frames, speakers)
    assert int(flag.item()) == 0


def test_embed_kernel_flags_and_zeroes_bad_rows(built_lib, cuda_device):
    """A token id equal to num_embs / a speaker id equal to num_spk and an id of -1 (one row past
    either end of the table; the tables are the middle of larger tensors, so even a wrong guard
    would read inside the allocation): those rows are zeros, every other row is exact, and the flag
    holds exactly the bits of what was wrong."""
    rs = np.random.RandomState(0)
    emb = torch.from_numpy(rs.standard_normal((1 + 11 + 1, 48)).astype(np.float32)).to(cuda_device)[1:12]
    spk = torch.from_numpy(rs.standard_normal((1 + 5 + 1, 48)).astype(np.float32)).to(cuda_device)[1:6]
    frames = [3, 6, 2]
    ids_h = rs.randint(0, 11, size=11).astype(np.int64)
    for bad_tok, bad_spk, bits in (({4: 11}, {}, 1), ({}, {2: 5}, 2), ({0: -1, 10: 11}, {1: -1}, 3)):
        ids, g = ids_h.copy(), np.asarray([1, 3, 0], np.int64)
        for k, v in bad_tok.items():
            ids[k] = v
        for k, v in bad_spk.items():
            g[k] = v
        flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        out = _embed(built_lib, emb, spk, torch.from_numpy(ids).to(cuda_device), torch.from_numpy(g).to(cuda_device),
                     frames, flag).cpu().numpy()
        utt = np.repeat(np.arange(3), frames)
        e, s = emb.cpu().numpy(), spk.cpu().numpy()
        for r in range(11):
            if r in bad_tok or utt[r] in bad_spk:
                assert not out[r].any(), r
            else:
                np.testing.assert_array_equal(out[r], e[ids[r]] + s[g[utt[r]]])
        assert int(flag.item()) == bits


@pytest.fixture(scope="module")
def small_model(built_lib, cuda_device):
    m, params, folded = dsym_module("dsym_hifigan_test")
    return m.to(cuda_device), params, folded


def _run_golden(m, g, device):
    meta, c = g["meta"], g["c"]
    with torch.no_grad():
        if meta["mode"] == "forward":
            return m(torch.from_numpy(c).to(device)).cpu().numpy()
        return m.inference(c, g=meta["options"].get("g")).cpu().numpy()


@pytest.mark.parametrize("name", DSYM_GOLDEN)
def test_parity_with_reference_fixture(built_lib, cuda_device, name):
    g = load_dsym_golden(name)
    m, _, _ = dsym_module(g["meta"]["vocoder"], seed=g["meta"]["weight_seed"])
    y = _run_golden(m.to(cuda_device), g, cuda_device)
    assert y.shape == g["y"].shape and np.isfinite(y).all()
    err = float(np.abs(y - g["y"]).max())
    print(f"{name}: max|d| = {err:.2e}")
    assert err < ATOL


def test_inference_input_forms_agree(small_model, cuda_device):
    """(T, 2) ids as int64 numpy, float32 CPU tensor (what the recipes dump) and device tensor,
    and (T, 1) + g=, give the same samples bit for bit."""
    m, _, _ = small_model
    c = load_dsym_golden("dsym_hifigan_test_T9")["c"]
    with torch.no_grad():
        y0 = m.inference(c)
        for form in (torch.from_numpy(c).float(), torch.from_numpy(c).to(cuda_device),
                     torch.from_numpy(c).to(cuda_device).float() + 0.75):
            assert torch.equal(m.inference(form), y0)
        assert torch.equal(m.inference(c[:, :1], g=int(c[0, 1])), y0)
        assert torch.equal(m.inference(torch.from_numpy(c[:, :1]).to(cuda_device), g=int(c[0, 1])), y0)


def test_ragged_batch_matches_oracle(small_model, cuda_device):
    from oracle import melgan_numpy

    m, params, folded = small_model
    frames, speakers = [3, 9, 4], [0, 4, 2]
    rs = np.random.RandomState(9)
    cs = [np.stack([rs.randint(0, 11, size=f), np.full(f, s)], 1).astype(np.int64) for f, s in zip(frames, speakers)]
    with torch.no_grad():
        ys = m.inference_batch(cs)
        ys_g = m.inference_batch([torch.from_numpy(c[:, :1]).to(cuda_device) for c in cs], g=speakers)
    for c, s, y, yg in zip(cs, speakers, ys, ys_g):
        ref = melgan_numpy.hifigan_forward(oracle_features(c[:, 0], s, folded), folded, params).T
        assert y.shape == ref.shape
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print(f"T' = {len(c)}, speaker {s}: max|d| = {err:.2e}")
        assert err < ATOL
        assert torch.equal(y, yg)


@pytest.mark.parametrize("what", ["token", "speaker"])
def test_invalid_id_on_device_raises_and_module_recovers(small_model, cuda_device, what):
    """Exactly one id one past its table, in a device tensor (nothing is checked on the host):
    IndexError naming it, and the next valid call on the same module gives the fixture's result."""
    m, _, _ = small_model
    g = load_dsym_golden("dsym_hifigan_test_T9")
    c = g["c"].copy()
    if what == "token":
        c[5, 0] = 11
    else:
        c[:, 1] = 5
    with torch.no_grad():
        with pytest.raises(IndexError, match=f"a {what} id outside"):
            m.inference(torch.from_numpy(c).to(cuda_device))
        y = m.inference(torch.from_numpy(g["c"]).to(cuda_device)).cpu().numpy()
    assert float(np.abs(y - g["y"]).max()) < ATOL


def test_decode_cli_on_unit_dump(built_lib, cuda_device, tmp_path):
    from parallelwavegan_amd.bin import decode

    _, params = configs.vocoder_params("dsym_hifigan_test")
    m, _, _ = dsym_module("dsym_hifigan_test", seed=4)
    ckpt = str(tmp_path / "checkpoint-10steps.pkl")
    torch.save({"model": {"generator": {k: v.clone() for k, v in m.state_dict().items()}}, "steps": 10}, ckpt)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(dict(generator_type="DiscreteSymbolHiFiGANGenerator", generator_params=params,
                            sampling_rate=16000, format="npy", version="0.6.1"), f)
    dump = tmp_path / "dump"
    dump.mkdir()
    rs = np.random.RandomState(12)
    feats = {}
    for u, (f, s) in {"utt_a": (9, 1), "utt_b": (23, 4), "utt_c": (5, 0)}.items():
        feats[u] = np.stack([rs.randint(0, 11, size=f), np.full(f, s)], 1).astype(np.float32)  # as the recipes dump
        np.save(dump / f"{u}-feats.npy", feats[u])
    out = tmp_path / "wav"
    assert decode.main(["--dumpdir", str(dump), "--outdir", str(out), "--checkpoint", ckpt, "--verbose", "0"]) == 0
    ref = load_model(ckpt)
    ref.remove_weight_norm()
    ref = ref.eval().to(cuda_device)
    for u, c in feats.items():
        z, sr = read_pcm16_wav(str(out / f"{u}_gen.wav"))
        assert sr == 16000 and z.shape == (len(c) * 8,)
        with torch.no_grad():
            y = ref.inference(c).view(-1).cpu().numpy()
        np.testing.assert_allclose(z, y, atol=1.0 / 32767)
