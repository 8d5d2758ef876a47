#!/usr/bin/env python3
"""Time the token front end of DiscreteSymbolHiFiGANGenerator against torch indexing.

Workload: ``inference_batch`` at dsym_hubert_v1 on 32 ragged utterances whose lengths are the
bench's RandomState(3) draw (synthetic.libritts_lengths), ids already on the device. Two legs,
alternated call by call in one process:
  hip    the drop-in: pwg_embed_rows writes the feature rows, then the HiFiGAN program;
  torch  the same program fed ``emb.weight[ids] + spk_emb.weight[g]`` built by torch indexing.
Each call is timed with a host clock around work that ends in a device synchronise. Reported per
leg: median, min, max, and the medians of the even and odd calls (their difference is the
run-to-run spread of the same code in the same session). The kernel's own time is a HIP event
pair around pwg_embed_rows alone. The two legs' outputs are compared bit for bit.

    python tools/dsym_frontend_bench.py --out profiles/dsym_frontend.json
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

from parallelwavegan_amd import DiscreteSymbolHiFiGANGenerator, _lib, configs, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dsym_hubert_v1")
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a ROCm GPU")
    dev = torch.device("cuda:0")
    _, params = configs.vocoder_params(args.config)
    m = DiscreteSymbolHiFiGANGenerator(**configs.vocoder_params(args.config)[1])
    m.remove_weight_norm()
    sd = synthetic.make_module_state_dict(m, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.eval().to(dev)
    frames = [int(f) for f in synthetic.libritts_lengths(args.utts)]
    rs = np.random.RandomState(7)
    has_spk = params["num_spk_embs"] > 0
    cs = []
    for f in frames:
        cols = [rs.randint(0, params["num_embs"], size=f)]
        if has_spk:
            cols.append(np.full(f, rs.randint(0, params["num_spk_embs"])))
        cs.append(torch.from_numpy(np.stack(cols, 1).astype(np.int64)).to(dev))
    eng = m.engine()
    frames_t = torch.tensor(frames, device=dev)

    def leg_hip():
        return m.inference_batch(cs)

    def leg_torch():
        ids = torch.cat([c[:, 0] for c in cs])
        feats = m.emb.weight[ids]
        if has_spk:
            g = torch.stack([c[0, 1] for c in cs])
            feats = feats + torch.repeat_interleave(m.spk_emb.weight[g], frames_t, dim=0)
        return eng.infer_rows(frames, feats.reshape(-1))

    legs = {"hip": leg_hip, "torch": leg_torch}
    times = {k: [] for k in legs}
    with torch.no_grad():
        for _ in range(args.warmup):
            outs = {k: fn() for k, fn in legs.items()}
        torch.cuda.synchronize(dev)
        same = all(torch.equal(a, b) for a, b in zip(outs["hip"], outs["torch"]))
        del outs
        for _ in range(args.steps):
            for k, fn in legs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3)
        # the kernel alone: the same arguments inference_batch passes
        emb, spk = m._tables
        ids = torch.cat([c[:, 0] for c in cs]).contiguous()
        g = torch.stack([c[0, 1] for c in cs]).contiguous() if has_spk else None
        row_start = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int64, device=dev)
        rows, dim = int(ids.numel()), params["in_channels"]
        feats = torch.empty(rows * dim, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L = _lib.load()
        kern = []
        for i in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.pwg_embed_rows(emb.data_ptr(), emb.shape[0], spk.data_ptr() if has_spk else None,
                                        spk.shape[0] if has_spk else 0, dim, ids.data_ptr(),
                                        g.data_ptr() if has_spk else None, row_start.data_ptr(), len(frames), rows,
                                        feats.data_ptr(), flag.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                kern.append(e0.elapsed_time(e1))
        assert int(flag.item()) == 0

    def stats(v):
        v = np.asarray(v)
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()),
                    median_even_ms=float(np.median(v[0::2])), median_odd_ms=float(np.median(v[1::2])), n=int(v.size))

    res = dict(config=args.config, utterances=len(frames), frames=int(sum(frames)), rows_bytes=rows * dim * 4,
               samples=int(sum(frames)) * m.upsample_factor, steps=args.steps, warmup=args.warmup,
               hip=stats(times["hip"]), torch=stats(times["torch"]), outputs_bit_identical=bool(same),
               embed_kernel_ms=stats(kern), device=torch.cuda.get_device_name(dev))
    res["spread_ms"] = max(abs(res[k]["median_even_ms"] - res[k]["median_odd_ms"]) for k in ("hip", "torch"))
    res["hip_minus_torch_ms"] = res["hip"]["median_ms"] - res["torch"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
