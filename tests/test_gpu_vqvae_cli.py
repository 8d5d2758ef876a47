"""The decode CLI's VQ-WAV2WAV branch end to end on the GPU: three ``*-wave.npy`` files of different
lengths with local and global dumps on vqvae_test_a; wav files of the right lengths and the ``text`` file
with the indices ``encode_batch`` returns."""

import os

import numpy as np
import pytest
import torch
import yaml

from parallelwavegan_amd import VQVAE, configs, synthetic
from parallelwavegan_amd.utils import load_model, read_pcm16_wav

pytestmark = pytest.mark.gpu


def test_decode_cli_vq_end_to_end(tmp_path, built_lib, cuda_device):
    from parallelwavegan_amd.bin import decode

    params = configs.vqvae_params("vqvae_test_a")
    m = VQVAE(**configs.vqvae_params("vqvae_test_a"))
    state = {k: torch.from_numpy(v) for k, v in synthetic.make_module_state_dict(m, seed=4).items()}
    # a codebook where the encoder outputs are (the N(0, 1) table would give every frame one code)
    state["codebook.embedding.weight"] = 0.04 * state["codebook.embedding.weight"] + state["encoder.layers.4.bias"][None, :]
    ckpt = str(tmp_path / "checkpoint-10steps.pkl")
    torch.save({"model": {"generator": state}, "steps": 10}, ckpt)
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(dict(generator_type="VQVAE", generator_params=params, sampling_rate=24000, format="npy",
                            version="0.6.1", use_local_condition=True, use_global_condition=True), f)
    np.save(tmp_path / "stats.npy", np.zeros((2, 80), np.float32))  # present and never registered
    lengths = {"utt_a": 61, "utt_b": 200, "utt_c": 8 * 5}
    dump = tmp_path / "dump"
    dump.mkdir()
    rs = np.random.RandomState(70)
    for i, (u, n) in enumerate(lengths.items()):
        np.save(dump / f"{u}-wave.npy", (0.3 * rs.standard_normal(n)).astype(np.float32))
        np.save(dump / f"{u}-local.npy", rs.standard_normal((-(-n // 8), 2)).astype(np.float32))
        np.save(dump / f"{u}-global.npy", np.asarray(i + 1, np.int64))
    out = tmp_path / "wav"
    assert decode.main(["--dumpdir", str(dump), "--outdir", str(out), "--checkpoint", ckpt, "--verbose", "0",
                        "--batch-frames", "30"]) == 0
    model = load_model(ckpt)
    model.remove_weight_norm()
    model = model.eval().to(cuda_device)
    text = dict(line.split(" ", 1) for line in open(out / "text").read().splitlines())
    assert sorted(text) == sorted(lengths)
    for i, (u, n) in enumerate(lengths.items()):
        frames = -(-n // 8)
        z, sr = read_pcm16_wav(str(out / f"{u}_gen.wav"))
        assert sr == 24000 and z.shape == (frames * 8,)
        with torch.no_grad():
            idx = model.encode_batch([np.load(dump / f"{u}-wave.npy")])[0]
            y = model.decode_batch([idx], [np.load(dump / f"{u}-local.npy")], [i + 1])[0].view(-1).cpu().numpy()
        assert [int(v) for v in text[u].split()] == idx.cpu().tolist()
        np.testing.assert_allclose(z, np.clip(y, -1, 1), atol=1.5 / 32767)
    assert len({v for line in text.values() for v in line.split()}) > 1
    assert not os.path.exists(out / "utt_d_gen.wav")
