#!/usr/bin/env python3
"""Time DiscreteSymbolStyleMelGANGenerator (the TADE kernels with the token staging and the trimmed plan,
include/pwg_smg.h) against torch eager on the GPU.

Workload: dsym_style_melgan_hubert_v1, 16 ragged utterances of 400 to 900 frames (RandomState(3); 8 to 18 s
at 50 frames per second), fixed ids, speakers and noise. Two legs, alternated step by step in one process:
  hip    ``inference_batch``: one pwg_smg_run_tokens over the whole batch;
  eager  the torch restatement of the network (tests/dsym_stylemelgan_oracle.py) in fp32 on the same
         GPU, utterance by utterance (instance norm forbids padding a batch).
Each step is timed with a host clock around work that ends in a device synchronise; reported per
leg: median, min, max. A separate pass with per-launch HIP events (pwg_smg_set_timing) gives the
engine's milliseconds per kernel kind. The two legs' outputs are compared.

    python tools/dsym_stylemelgan_bench.py --out profiles/dsym_stylemelgan.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from parallelwavegan_amd import DiscreteSymbolStyleMelGANGenerator, configs, synthetic  # noqa: E402
from parallelwavegan_amd.engine import fold_weight_norm  # noqa: E402
from dsym_stylemelgan_oracle import TokenOracle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dsym_style_melgan_hubert_v1")
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gain", type=float, default=0.7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a ROCm GPU")
    dev = torch.device("cuda:0")
    params = configs.dsym_style_melgan_params(args.config)
    m = DiscreteSymbolStyleMelGANGenerator(**configs.dsym_style_melgan_params(args.config))
    sd = synthetic.make_module_state_dict(m, seed=0, gain=args.gain)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.eval().to(dev)
    orc = TokenOracle(fold_weight_norm(sd), params, dtype=torch.float32, device=dev)
    frames = [int(f) for f in np.random.RandomState(3).randint(400, 901, size=args.utts)]
    nf, hop = int(m.noise_upsample_factor), int(m.upsample_factor)
    rs = np.random.RandomState(7)
    cs = [torch.from_numpy(np.stack([rs.randint(0, params["num_embs"], size=f),
                                     np.full(f, rs.randint(0, params["num_spk_embs"]))], 1).astype(np.int64)).to(dev)
          for f in frames]
    zs = [torch.from_numpy(np.random.RandomState(100 + i).standard_normal(
        (1, params["in_channels"], (f - 1) // nf + 1)).astype(np.float32)).to(dev) for i, f in enumerate(frames)]

    def leg_hip():
        return m.inference_batch(cs, zs=zs)

    def leg_eager():
        return [orc(c, z[0].T) for c, z in zip(cs, zs)]

    legs = {"hip": leg_hip, "eager": leg_eager}
    times = {k: [] for k in legs}
    with torch.no_grad():
        for _ in range(args.warmup):
            outs = {k: fn() for k, fn in legs.items()}
        torch.cuda.synchronize(dev)
        diff = max(float((a - b).abs().max()) for a, b in zip(outs["hip"], outs["eager"]))
        del outs
        for _ in range(args.steps):
            for k, fn in legs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3)
        eng = m.engine()
        eng.set_timing(True)
        kinds = []
        for _ in range(3):
            leg_hip()
            kinds.append(eng.collect_timing())
        eng.set_timing(False)

    def stats(v):
        v = np.asarray(v)
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))

    samples = int(sum(frames)) * hop
    res = dict(config=args.config, utterances=len(frames), frames=int(sum(frames)), samples=samples, steps=args.steps,
               warmup=args.warmup, gain=args.gain, hip=stats(times["hip"]), eager=stats(times["eager"]),
               max_abs_diff_hip_vs_eager=diff,
               kernel_ms={k: float(np.median([d[k] for d in kinds])) for k in kinds[0]},
               device=torch.cuda.get_device_name(dev))
    res["hip_samples_per_s"] = samples / (res["hip"]["median_ms"] * 1e-3)
    res["eager_samples_per_s"] = samples / (res["eager"]["median_ms"] * 1e-3)
    res["eager_over_hip"] = res["eager"]["median_ms"] / res["hip"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
