#!/usr/bin/env python3
"""Time the HIP sine generator (include/pwg_sine.h) on the UHiFiGAN benchmark batch.

Workload: uhifigan_v1 (24 kHz, hop 300), the 16 ragged utterances of tools/uhifigan_bench.py
(synthetic.libritts_lengths), a gliding f0 contour per utterance, tile layout, fixed noise draws.
Three legs, each timed with a HIP event pair around the calls on the current stream, alternated step
by step in one process:
  frames   one pwg_sine_frames call over the batch (what UHiFiGANGenerator.*_from_f0 issues);
  samples  one pwg_sine_samples call on the f0 already expanded to the sample rate;
  eager    a torch restatement of SineGen.forward (layers/sine.py: two fp32 cumulative sums) on the
           same GPU, utterance by utterance, with the same draws.
Reported per leg: median, min, max over the timed steps after the warm-up; the largest difference of
every leg from the frames leg; and the frames leg's share of one UHiFiGAN ``inference_batch`` step
(host clock around a synchronised call, as tools/uhifigan_bench.py measures it). No clock is pinned.

    python tools/sinegen_bench.py --out profiles/sinegen/bench.json
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

from parallelwavegan_amd import UHiFiGANGenerator, _lib, configs, sinegen, synthetic  # noqa: E402

SR, AMP, NSTD, THR = 24000.0, 0.1, 0.003, 0.0


def contour(n, seed):
    rs = np.random.RandomState(seed)
    f = np.clip(np.abs(300.0 + np.cumsum(rs.standard_normal(n)) * 12.0), 80.0, 900.0)
    f[np.repeat(rs.rand(n // 16 + 1) < 0.2, 16)[:n]] = 0.0
    return f.astype(np.float32)


def eager_sinegen(f0, n):
    """layers/sine.py:48-80, 111-146 for one channel: f0 (N,), n (N,) on the device."""
    rad = (f0 / SR) % 1
    over = torch.cumsum(rad, 0) % 1
    shift = torch.zeros_like(rad)
    shift[1:] = ((over[1:] - over[:-1]) < 0) * -1.0
    sines = torch.sin(torch.cumsum(rad + shift, 0) * 2 * np.pi) * AMP
    uv = (f0 > THR).float()
    return sines * uv + (uv * NSTD + (1 - uv) * AMP / 3) * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a ROCm GPU")
    dev = torch.device("cuda:0")
    params = configs.uhifigan_params("uhifigan_v1")
    m = UHiFiGANGenerator(**configs.uhifigan_params("uhifigan_v1"))
    sd = synthetic.make_module_state_dict(m, seed=0, gain=0.7)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.remove_weight_norm()
    m = m.eval().to(dev)
    hop = m.upsample_factor
    frames = [int(f) for f in synthetic.libritts_lengths(args.utts)]
    f0s = [contour(f, 200 + i) for i, f in enumerate(frames)]
    exts = [np.tile(f, hop) for f in f0s]
    rows = sum(frames) * hop
    f0_fr = torch.from_numpy(np.concatenate(f0s)).to(dev)
    f0_sm = torch.from_numpy(np.concatenate(exts)).to(dev)
    n = torch.randn(rows, device=dev)
    fstart = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)).to(dev)
    rstart = fstart * hop
    out_fr, out_sm = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    ext_dev = [torch.from_numpy(e).to(dev) for e in exts]
    n_dev = list(torch.split(n, [f * hop for f in frames]))

    def leg_frames():
        return sinegen.sine_call("pwg_sine_frames", dev, f0_fr, fstart, len(frames), sum(frames),
                                 (hop, _lib.PWG_SINE_LAYOUTS["tile"]), SR, 1, AMP, NSTD, THR, None, n, out_fr, None, None)

    def leg_samples():
        return sinegen.sine_call("pwg_sine_samples", dev, f0_sm, rstart, len(frames), rows, (), SR, 1, AMP, NSTD, THR,
                                 None, n, out_sm, None, None)

    eager_out = []

    def leg_eager():
        eager_out[:] = [eager_sinegen(f, z) for f, z in zip(ext_dev, n_dev)]

    legs = {"frames": leg_frames, "samples": leg_samples, "eager": leg_eager}
    times = {k: [] for k in legs}
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize(dev)
        for _ in range(args.steps):
            for k, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize(dev)
                times[k].append(a.elapsed_time(b))
        diff_samples = float((out_fr - out_sm).abs().max())
        diff_eager = float((out_fr - torch.cat(eager_out)).abs().max())
        # one UHiFiGAN step on the same batch, from f0
        cs = [torch.from_numpy(synthetic.make_mel(f, params["in_channels"], seed=10 + i)).to(dev)
              for i, f in enumerate(frames)]
        step = []
        for i in range(2 + 5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            m.inference_batch_from_f0(cs, f0s, SR, "tile", noises=n_dev)
            torch.cuda.synchronize(dev)
            if i >= 2:
                step.append((time.perf_counter() - t0) * 1e3)

    def stats(v):
        v = np.asarray(v)
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))

    res = dict(config="uhifigan_v1", utterances=len(frames), n_frames=int(sum(frames)), n_samples=rows, layout="tile",
               steps=args.steps, warmup=args.warmup, **{k: stats(v) for k, v in times.items()},
               max_abs_diff_samples_vs_frames=diff_samples, max_abs_diff_eager_vs_frames=diff_eager,
               uhifigan_step_from_f0=stats(step),
               clock_note="device clocks not pinned; legs alternated step by step in one process; each leg's time "
                          "includes its scratch and flag allocations",
               device=torch.cuda.get_device_name(dev))
    res["frames_share_of_step"] = res["frames"]["median_ms"] / res["uhifigan_step_from_f0"]["median_ms"]
    res["eager_over_frames"] = res["eager"]["median_ms"] / res["frames"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
