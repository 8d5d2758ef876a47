#!/usr/bin/env python3
"""Time the HIP audio-conditioning kernels (include/pwg_wave.h) on the benchmark batch.

Workload: the 16 ragged utterances of tools/yin_bench.py (synthetic.libritts_lengths, frames x 300 samples,
3.69 M samples in all): an amplitude-modulated tone plus noise with a pause of a tenth of the utterance before
and after it. Settings: the silence trim at 2048 / 512 / 60 dB, the resampler at 48 kHz -> 24 kHz (1/2, 41
taps) and 44.1 kHz -> 24 kHz (80/147, 2941 taps) with the packed batch taken as the input at the higher rate,
and the fit to the mel length with a gain of 0.8 and the peak. Two legs per setting, each timed with a HIP
event pair around the calls on the current stream, alternated step by step in one process:
  engine   one pwg_*_run over the packed batch (the output allocation included);
  eager    torch fp32 on the same GPU, utterance by utterance. Trim: conv1d of the squares with a kernel of
           ones, maximum, threshold, first / last index by a masked min / max. Resample: one conv1d with
           `up` output channels (channel r holds the taps of outputs r mod up, placed in a common window)
           and stride `down`, then a transpose. Fit: slice, expand of the last sample, cat, multiply, abs max.
Reported per leg: median, min, max over the timed steps after the warm-up; per setting the agreement of the two
legs (bounds equal; largest resample difference; fit outputs equal). No clock is pinned.

    python tools/wave_bench.py --out profiles/wave/bench.json
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from parallelwavegan_amd import kaiser_lowpass_taps, synthetic  # noqa: E402
from parallelwavegan_amd.audio import ResamplePlan, TrimPlan, fit_run  # noqa: E402

TRIM = (2048, 512, 60.0)
RATES = {"48k_to_24k": (48000, 24000), "44k1_to_24k": (44100, 24000)}
HOP, FFT = 300, 2048


def eager_trim(x, fl, hop, factor, ones):
    p = fl // 2
    sq = torch.nn.functional.pad(x * x, (p, p))
    P = torch.nn.functional.conv1d(sq[None, None], ones, stride=hop)[0, 0] / fl
    n = P.numel()
    keep = torch.clamp(P, min=1e-10) > torch.clamp(P.max(), min=1e-10) * factor
    t = torch.arange(n, device=x.device)
    lo = torch.where(keep, t, n).min()
    hi = torch.where(keep, t, -1).max()
    return torch.stack([lo * hop, torch.clamp((hi + 1) * hop, max=x.numel())])


def eager_resample_weights(up, down, hf, device):
    """W (up, 1, S): row r holds hf[r down + half - s up] at s - s_min; with x padded by -s_min on the left,
    y[r + up j] = sum_s W[r][s - s_min] x[down j + s]. Returns (W, -s_min, S)."""
    half = len(hf) // 2
    s_min, s_max = -(half // up), ((up - 1) * down + half) // up
    W = np.zeros((up, s_max - s_min + 1), np.float32)
    for r in range(up):
        for s in range(s_min, s_max + 1):
            k = r * down + half - s * up
            if 0 <= k <= 2 * half:
                W[r, s - s_min] = hf[k]
    return torch.from_numpy(W[:, None, :]).to(device), -s_min, W.shape[1]


def eager_resample(x, up, down, W, left, S):
    T = x.numel()
    n_out = -(-T * up // down)
    J = -(-n_out // up)
    right = max(0, (J - 1) * down + S - (T + left))
    xp = torch.nn.functional.pad(x, (left, right))
    y = torch.nn.functional.conv1d(xp[None, None], W, stride=down)[0, :, :J]
    return y.t().reshape(-1)[:n_out]


def eager_fit(x, n, gain):
    T = x.numel()
    y = (x[:n] if n <= T else torch.cat([x, x[-1:].expand(n - T)])) * gain
    return y, y.abs().max()


def stats(v):
    v = np.asarray(v)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))


def speech_like(n, rs):
    t = np.arange(n)
    x = 1e-4 * rs.standard_normal(n)
    a, b = n // 10, n - n // 10
    x[a:b] += (0.5 * np.sin(2 * np.pi * 0.031 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.0007 * t)))[a:b]
    return x.astype(np.float32)


def time_legs(legs, steps, warmup, dev):
    times = {k: [] for k in legs}
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize(dev)
    for _ in range(steps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            times[k].append(a.elapsed_time(b))
    res = {k: stats(v) for k, v in times.items()}
    res["eager_over_engine"] = res["eager"]["median_ms"] / res["engine"]["median_ms"]
    return res


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
    frames = [int(f) for f in synthetic.libritts_lengths(args.utts)]
    lengths = [f * HOP for f in frames]
    rs = np.random.RandomState(5)
    waves = [torch.from_numpy(speech_like(n, rs)).to(dev) for n in lengths]
    packed = torch.cat(waves)
    res = dict(utterances=len(lengths), n_samples=int(sum(lengths)), steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(dev),
               clock_note="device clocks not pinned; legs alternated step by step in one process")
    out = {}
    with torch.no_grad():
        # ---- trim
        fl, hop, top_db = TRIM
        plan = TrimPlan(dev, fl, hop, top_db)
        factor = float(np.float32(10.0 ** (-top_db / 10.0)))
        ones = torch.ones(1, 1, fl, device=dev)

        def trim_engine():
            out["engine"] = plan.run(packed, lengths)[0]

        def trim_eager():
            out["eager"] = torch.stack([eager_trim(w, fl, hop, factor, ones) for w in waves])

        r = time_legs({"engine": trim_engine, "eager": trim_eager}, args.steps, args.warmup, dev)
        bounds = out["engine"].cpu().numpy()
        r.update(frame_length=fl, hop_length=hop, top_db=top_db, bounds_equal=bool(torch.equal(out["engine"], out["eager"])),
                 kept_share=float((bounds[:, 1] - bounds[:, 0]).sum() / sum(lengths)),
                 frames=int(sum(1 + n // hop for n in lengths)))
        res["trim"] = r

        # ---- resample
        for name, (src, dst) in RATES.items():
            g = int(np.gcd(src, dst))
            up, down = dst // g, src // g
            hf = kaiser_lowpass_taps(up, down).astype(np.float32)
            rplan = ResamplePlan(dev, up, down, hf)
            W, left, S = eager_resample_weights(up, down, hf, dev)

            def rs_engine():
                out["engine"] = rplan.run(packed, lengths)

            def rs_eager():
                out["eager"] = torch.cat([eager_resample(w, up, down, W, left, S) for w in waves])

            r = time_legs({"engine": rs_engine, "eager": rs_eager}, args.steps, args.warmup, dev)
            n_out = int(out["engine"].numel())
            macs = n_out * len(hf) / up
            r.update(up=up, down=down, taps=int(len(hf)), tile=rplan.tile, n_out=n_out,
                     max_abs_eager_vs_engine=float((out["engine"] - out["eager"]).abs().max()),
                     engine_gmacs_per_s=macs / r["engine"]["median_ms"] / 1e6)
            res[name] = r

        # ---- fit to the mel length, gain and peak
        outs = [(1 + n // HOP) * HOP for n in lengths]
        src = np.concatenate([[0], np.cumsum(lengths)[:-1]])

        def fit_engine():
            out["engine"] = fit_run(packed, src, lengths, outs, 0.8)

        def fit_eager():
            ys = [eager_fit(w, n, 0.8) for w, n in zip(waves, outs)]
            out["eager"] = (torch.cat([y for y, _ in ys]), torch.stack([p for _, p in ys]))

        r = time_legs({"engine": fit_engine, "eager": fit_eager}, args.steps, args.warmup, dev)
        r.update(gain=0.8, n_out=int(sum(outs)), outputs_equal=bool(torch.equal(out["engine"][0], out["eager"][0])),
                 peaks_equal=bool(torch.equal(out["engine"][1], out["eager"][1])))
        r["engine_gbytes_per_s"] = 8.0 * sum(outs) / r["engine"]["median_ms"] / 1e6
        res["fit"] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
