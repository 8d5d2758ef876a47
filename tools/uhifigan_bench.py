#!/usr/bin/env python3
"""Time UHiFiGANGenerator (HIP excitation front end, strided and two-source transposed convs on the
conv-network executor) against torch eager on the same GPU.

Workload: uhifigan_v1 (24 kHz, hop 300) with seeded weights, 16 ragged utterances with
synthetic.libritts_lengths (80 to 1199 frames), fixed mel and excitation. Two legs, alternated step by
step in one process:
  hip    ``inference_batch``: the front-end launch and one pwg_cnet_run_ext over the whole batch;
  eager  the same module graph in torch fp32 on the same GPU, built from the drop-in's own parameter
         holders (input_conv, downsamples, hidden_conv, upsamples, output_conv and the residual
         blocks' Sequentials; eval mode, weight norm removed), utterance by utterance.
Each step is timed with a host clock around work that ends in a device synchronise; reported per leg:
median, min, max over the timed steps after the warm-up. A separate pass with per-launch HIP events
(pwg_cnet_set_timing) gives the executor's milliseconds per op, grouped as strided convs / transposed
convs / MRF / rest; the front end is timed with its own event pair. The two legs' outputs are compared.
The clocks are whatever the device runs at: no clock is pinned (recorded as ``clock_note``).

    python tools/uhifigan_bench.py --out profiles/uhifigan_v1/bench.json
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

from parallelwavegan_amd import UHiFiGANGenerator, configs, synthetic  # noqa: E402


def eager_block(blk, x):
    for d in range(len(blk.convs1)):
        t = blk.convs1[d](x)
        if blk.use_additional_convs:
            t = blk.convs2[d](t)
        x = t + x
    return x


def eager_forward(m, c, exc):
    """models/uhifigan.py:261-301 over the drop-in's torch modules: c (1, in, T), exc (1, 1, T * hop)."""
    nb = m.num_blocks

    def mrf(blocks, i, x):
        cs = 0.0
        for j in range(nb):
            cs = cs + eager_block(blocks[i * nb + j], x)
        return cs / nb

    h = m.input_conv(exc)
    skips = []
    for i in range(len(m.downsamples)):
        h = m.downsamples[i](mrf(m.downsamples_mrf, i, h))
        skips.append(h)
    skips.reverse()
    g = m.hidden_conv(c)
    for i in range(len(m.upsamples)):
        g = mrf(m.upsamples_mrf, i, m.upsamples[i](torch.cat((g, skips[i]), dim=1)))
    return m.output_conv(g)


def group_of(name):
    if name.startswith("downsamples."):
        return "strided_convs"
    if name.startswith("upsamples."):
        return "transposed_convs"
    if "_mrf." in name:
        return "mrf"
    return "rest"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="uhifigan_v1")
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gain", type=float, default=0.7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a ROCm GPU")
    dev = torch.device("cuda:0")
    params = configs.uhifigan_params(args.config)
    m = UHiFiGANGenerator(**configs.uhifigan_params(args.config))
    sd = synthetic.make_module_state_dict(m, seed=0, gain=args.gain)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.remove_weight_norm()
    m = m.eval().to(dev)
    hop = m.upsample_factor
    frames = [int(f) for f in synthetic.libritts_lengths(args.utts)]
    cs = [torch.from_numpy(synthetic.make_mel(f, params["in_channels"], seed=10 + i)).to(dev)
          for i, f in enumerate(frames)]
    es = [torch.from_numpy((0.5 * np.random.RandomState(100 + i).standard_normal(f * hop)).astype(np.float32)).to(dev)
          for i, f in enumerate(frames)]

    def leg_hip():
        return m.inference_batch(cs, es)

    def leg_eager():
        return [eager_forward(m, c.T[None], e[None, None])[0].T for c, e in zip(cs, es)]

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
        exc = torch.cat(es).contiguous()
        front = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            m._excite(exc, frames, dev)
            b.record()
            torch.cuda.synchronize(dev)
            front.append(a.elapsed_time(b))
        eng.set_timing(True)
        runs = []
        for _ in range(3):
            leg_hip()
            torch.cuda.synchronize(dev)
            g = {}
            for name, ms, _ in eng.collect_timing():
                g[group_of(name)] = g.get(group_of(name), 0.0) + ms
            runs.append(g)
        eng.set_timing(False)

    def stats(v):
        v = np.asarray(v)
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))

    op_ms = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    op_ms["front_end"] = float(np.median(front[1:]))
    total = sum(op_ms.values())
    samples = int(sum(frames)) * hop
    res = dict(config=args.config, utterances=len(frames), frames=int(sum(frames)), samples=samples, steps=args.steps,
               warmup=args.warmup, gain=args.gain, hip=stats(times["hip"]), eager=stats(times["eager"]),
               max_abs_diff_hip_vs_eager=diff, op_ms=op_ms, op_share={k: v / total for k, v in op_ms.items()},
               clock_note="device clocks not pinned; legs alternated step by step in one process",
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
