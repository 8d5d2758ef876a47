#!/usr/bin/env python3
"""Time the front end of DiscreteSymbolDurationGenerator against the same front end in torch eager ops.

Workload: ``inference_batch`` with PREDICTED durations at dsym_duration_v1 on 32 ragged token
sequences (a quarter of the bench's RandomState(3) lengths each, ids already on the device; the
predictor's output bias is set so that durations spread over roughly 0-6). Two legs, alternated
call by call in one process:
  hip    the drop-in: pwg_durpred_layer per layer, pwg_regulate_scan, pwg_regulate_rows, then the
         HiFiGAN program;
  torch  the same program fed by torch eager ops on the same GPU: embedding lookup, the predictor as
         a padded batch (conv1d -> relu -> layer_norm, masked between layers), exp / round / clamp,
         repeat_interleave.
Both legs read the per-utterance totals back once (the body cannot be planned without them). Each
call is timed with a host clock around work that ends in a device synchronise. Reported per leg:
median, min, max, and the medians of the even and odd calls (their difference is the run-to-run
spread of the same code in the same session). The front-end kernels' own time is a HIP event pair
around the predictor launches and around scan + gather. The legs' durations are compared exactly and,
where they agree, their outputs by max |difference|.

    python tools/dsym_variants_bench.py --out profiles/dsym_variants.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from parallelwavegan_amd import DiscreteSymbolDurationGenerator, _lib, configs, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dsym_duration_v1")
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--linear-bias", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a ROCm GPU")
    dev = torch.device("cuda:0")
    _, params = configs.vocoder_params(args.config)
    m = DiscreteSymbolDurationGenerator(**configs.vocoder_params(args.config)[1])
    m.remove_weight_norm()
    sd = synthetic.make_module_state_dict(m, seed=0)
    sd["duration_predictor.linear.bias"] = np.full(1, args.linear_bias, np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.eval().to(dev)
    counts = [max(1, int(f) // 4) for f in synthetic.libritts_lengths(args.utts)]
    rs = np.random.RandomState(7)
    cs = [torch.from_numpy(rs.randint(0, params["num_embs"] + 1, size=(t, 1)).astype(np.int64)).to(dev) for t in counts]
    eng = m.engine()
    dp, offset = m.duration_predictor, float(m.duration_predictor.offset)
    lens = torch.tensor(counts, device=dev)
    mask = (torch.arange(max(counts), device=dev)[None, :] < lens[:, None])  # (B, Tmax)

    def torch_front():
        ids = torch.cat([c[:, 0] for c in cs])
        rows = m.emb.weight[ids]
        h = torch.nn.utils.rnn.pad_sequence(torch.split(rows, counts), batch_first=True).transpose(1, 2)
        for seq in dp.conv:
            conv, norm = seq[0], seq[2]
            h = F.relu(F.conv1d(h, conv.weight, conv.bias, padding=1))
            h = F.layer_norm(h.transpose(1, 2), norm.normalized_shape, norm.weight, norm.bias, norm.eps).transpose(1, 2)
            h = h * mask[:, None, :]
        logd = F.linear(h.transpose(1, 2), dp.linear.weight, dp.linear.bias).squeeze(-1)
        ds = torch.clamp(torch.round(logd.exp() - offset), min=0).long() * mask
        totals = ds.sum(1)
        ds = torch.where((totals == 0)[:, None] & mask, torch.ones_like(ds), ds)
        flat = ds[mask]
        return rows, flat, ds.sum(1)

    def leg_hip():
        return m.inference_batch(cs)

    def leg_torch():
        rows, flat, totals = torch_front()
        frames = totals.tolist()  # the one read-back, as in the drop-in
        feats = torch.repeat_interleave(rows, flat, dim=0)
        return eng.infer_rows(frames, feats.reshape(-1))

    legs = {"hip": leg_hip, "torch": leg_torch}
    times = {k: [] for k in legs}
    with torch.no_grad():
        for _ in range(args.warmup):
            outs = {k: fn() for k, fn in legs.items()}
        torch.cuda.synchronize(dev)
        d_hip = torch.cat(m.predict_durations(cs))
        d_torch = torch_front()[1]
        mismatch = int((d_hip != d_torch).sum())
        diff = None
        if all(a.shape == b.shape for a, b in zip(outs["hip"], outs["torch"])):
            diff = max(float((a - b).abs().max()) for a, b in zip(outs["hip"], outs["torch"]))
        frames = [int(o.shape[0]) // m.upsample_factor for o in outs["hip"]]
        del outs
        for _ in range(args.steps):
            for k, fn in legs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3)
        # the kernels alone, with the arguments inference_batch passes
        _, _, rs_d, ids_d, _, _ = m._tokens_to_device([c[:, 0] for c in cs])
        n, tokens, dim = len(counts), sum(counts), params["in_channels"]
        stream = torch.cuda.current_stream(dev)
        L = _lib.load()
        os_d = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int64, device=dev)
        prefix = torch.empty(tokens, dtype=torch.int64, device=dev)
        totals = torch.empty(n, dtype=torch.int64, device=dev)
        feats = torch.empty(sum(frames) * dim, dtype=torch.float32, device=dev)
        k_pred, k_reg = [], []
        for i in range(args.warmup + args.steps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            _, dur = m._predict(ids_d, rs_d, n, tokens, stream)
            ev[1].record()
            _lib.check(L.pwg_regulate_scan(dur.data_ptr(), rs_d.data_ptr(), n, tokens, prefix.data_ptr(),
                                           totals.data_ptr(), m._flag.data_ptr(), stream.cuda_stream))
            _lib.check(L.pwg_regulate_rows(m._tables[0].data_ptr(), m.num_embs, dim, ids_d.data_ptr(), prefix.data_ptr(),
                                           totals.data_ptr(), rs_d.data_ptr(), os_d.data_ptr(), n, tokens, sum(frames),
                                           feats.data_ptr(), m._flag.data_ptr(), stream.cuda_stream))
            ev[2].record()
            ev[2].synchronize()
            if i >= args.warmup:
                k_pred.append(ev[0].elapsed_time(ev[1]))
                k_reg.append(ev[1].elapsed_time(ev[2]))
        assert int(m._flag.item()) == 0

    def stats(v):
        v = np.asarray(v)
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()),
                    median_even_ms=float(np.median(v[0::2])), median_odd_ms=float(np.median(v[1::2])), n=int(v.size))

    res = dict(config=args.config, utterances=n, tokens=tokens, frames=int(sum(frames)),
               samples=int(sum(frames)) * m.upsample_factor, steps=args.steps, warmup=args.warmup,
               hip=stats(times["hip"]), torch=stats(times["torch"]), durations_mismatching=mismatch,
               outputs_max_abs_diff=diff, predictor_kernels_ms=stats(k_pred), regulate_kernels_ms=stats(k_reg),
               device=torch.cuda.get_device_name(dev))
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
