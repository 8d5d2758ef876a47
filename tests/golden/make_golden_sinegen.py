"""Generate the SineGen fixtures in tests/golden/sinegen/*.npz from the REFERENCE implementation
(parallel_wavegan/layers/sine.py:SineGen, and for one end-to-end case models/uhifigan.py).

Runs only where the reference is mounted; no test runs it. The reference is imported read-only with
the shim of make_golden_uhifigan.py (scipy.signal.kaiser alias, h5py stub); no reference file is
touched or copied.

Per case: a frame-rate f0 contour is expanded to the sample rate (``tile``: exactly the expression
of bin/preprocess.py:431-436; ``hold``: repeat_interleave) and goes through the reference's
SineGen.forward on the CPU after torch.manual_seed(seed). The forward's internal draws are replayed
from the same seed (``ini = torch.rand(B, dim)`` with column 0 zeroed, then ``n = torch.randn(B, N,
dim)``) and checked against the returned noise bit for bit, so the fixture records the draws
themselves: f0 (T,), ini (dim,), n (N, dim) and the reference's sine (N, dim), uv (N,), noise (N, dim).

``sg_e2e_*`` takes the tile excitation through the reference UHiFiGANGenerator (the smallest reduced
config of parallelwavegan_amd.configs, weights from parallelwavegan_amd.synthetic as in
make_golden_uhifigan.py): c, f0, n, excitation, y.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sinegen.py
"""

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from parallelwavegan_amd import configs, synthetic  # noqa: E402

REFERENCE = os.environ.get("PWG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "sinegen")

# name, layout, hop, T, SineGen arguments, contour
CASES = [
    ("sg_tile_h8_T19", "tile", 8, 19, dict(samp_rate=24000), "sung"),
    ("sg_hold_h8_T19", "hold", 8, 19, dict(samp_rate=24000), "sung"),
    ("sg_tile_h300_T7", "tile", 300, 7, dict(samp_rate=24000), "sung"),
    ("sg_hold_h5_T33_harm7", "hold", 5, 33, dict(samp_rate=16000, harmonic_num=7, voiced_threshold=100), "low"),
    ("sg_tile_h8_T1", "tile", 8, 1, dict(samp_rate=24000), "sung"),
    ("sg_tile_h1_T19", "tile", 1, 19, dict(samp_rate=24000), "sung"),
    ("sg_tile_h8_T5_unvoiced", "tile", 8, 5, dict(samp_rate=24000), "unvoiced"),
]
E2E = ("sg_e2e_noadd_T9", "uhifigan_noadd_nobias_test", 9, 24000)


def import_reference():
    import scipy.signal
    import scipy.signal.windows

    scipy.signal.kaiser = scipy.signal.windows.kaiser  # layers/pqmf.py:11 on scipy >= 1.13
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))  # utils/utils.py:16, not on the path
    sys.path.insert(0, REFERENCE)
    from parallel_wavegan.layers import SineGen
    from parallel_wavegan.models import UHiFiGANGenerator

    return SineGen, UHiFiGANGenerator


def contour(kind, T, seed):
    """A frame-rate f0 contour: voiced stretches that glide, unvoiced frames of 0."""
    rs = np.random.RandomState(seed)
    if kind == "unvoiced":
        return np.zeros(T, np.float32)
    lo, hi = (60.0, 180.0) if kind == "low" else (110.0, 620.0)  # "low" straddles a threshold of 100
    f = lo + (hi - lo) * rs.rand() + np.cumsum(rs.standard_normal(T) * 0.05 * (hi - lo))
    f = np.clip(np.abs(f), lo, hi)
    if T >= 5:
        f[rs.rand(T) < 0.25] = 0.0
        f[0] = f[0] or lo * 1.5  # the first frame voiced: the initial phase shows
    return f.astype(np.float32)


def expand(f0, hop, layout):
    if layout == "tile":  # bin/preprocess.py:431-436
        return torch.from_numpy(f0).reshape(1, 1, -1).repeat(1, hop, 1).reshape(1, -1, 1)
    return torch.from_numpy(f0).repeat_interleave(hop).reshape(1, -1, 1)


def run_sinegen(SineGen, f0, hop, layout, kwargs, seed):
    gen = SineGen(**kwargs)
    ext = expand(f0, hop, layout)
    torch.manual_seed(seed)
    sine, uv, noise = gen(ext)
    torch.manual_seed(seed)
    ini = torch.rand(1, gen.dim)
    ini[:, 0] = 0
    n = torch.randn(1, ext.shape[1], gen.dim)
    amp = uv * gen.noise_std + (1 - uv) * gen.sine_amp / 3
    assert torch.equal(amp * n, noise), "the replayed draws are not the forward's"
    return dict(f0=f0, ini=ini[0].numpy(), n=n[0].numpy(), sine=sine[0].numpy(), uv=uv[0, :, 0].numpy(),
                noise=noise[0].numpy())


def main():
    SineGen, RefUHG = import_reference()
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)
    for idx, (name, layout, hop, T, kwargs, kind) in enumerate(CASES):
        f0 = contour(kind, T, seed=100 + idx)
        arrays = run_sinegen(SineGen, f0, hop, layout, kwargs, seed=idx)
        meta = dict(name=name, layout=layout, hop=hop, T=T, seed=idx, samp_rate=kwargs["samp_rate"],
                    harmonic_num=kwargs.get("harmonic_num", 0), voiced_threshold=kwargs.get("voiced_threshold", 0),
                    sine_amp=0.1, noise_std=0.003, torch=torch.__version__)
        arrays["meta"] = np.array(json.dumps(meta))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        print(f"{name}: f0 {f0.shape} voiced {int((f0 > meta['voiced_threshold']).sum())} sine {arrays['sine'].shape}")

    name, cfg, T, sr = E2E
    from parallelwavegan_amd.uhifigan import UHiFiGANGenerator

    params = configs.uhifigan_params(cfg)
    hop = int(np.prod(params["upsample_scales"]))
    sd = synthetic.make_module_state_dict(UHiFiGANGenerator(**configs.uhifigan_params(cfg)), seed=0, gain=1.0)
    f0 = contour("sung", T, seed=300)
    sg = run_sinegen(SineGen, f0, hop, "tile", dict(samp_rate=sr), seed=50)
    c = synthetic.make_mel(T, params["in_channels"], seed=1)
    ys = []
    for dtype in (torch.float32, torch.float64):
        model = RefUHG(**configs.uhifigan_params(cfg))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.eval().to(dtype)
        with torch.no_grad():
            ys.append(model.inference(excitation=torch.from_numpy(sg["sine"][:, 0]).to(dtype), f0=torch.zeros(T),
                                      c=torch.from_numpy(c).to(dtype)))
    e_ref = float((ys[0].double() - ys[1]).abs().max())
    assert e_ref <= 1e-5 and float(ys[0].abs().max()) < 0.99
    meta = dict(name=name, config=cfg, mode="inference", shape=T, weight_seed=0, gain=1.0, weight_norm=True,
                e_ref=e_ref, y_max=float(ys[0].abs().max()), samp_rate=sr, layout="tile", hop=hop,
                torch=torch.__version__)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), c=c, f0=f0, n=sg["n"][:, 0], excitation=sg["sine"][:, 0],
                        y=ys[0].numpy().astype(np.float32), meta=np.array(json.dumps(meta)))
    print(f"{name}: c {c.shape} excitation {sg['sine'].shape} y {ys[0].shape} e_ref {e_ref:.1e}")


if __name__ == "__main__":
    main()
