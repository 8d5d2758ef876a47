#!/usr/bin/env python3
"""Time the HIP YIN f0 estimator (include/pwg_yin.h) on the benchmark batch.

Workload: the 16 ragged utterances of tools/logmel_bench.py (synthetic.libritts_lengths), each of
frames x hop samples (a 150 Hz four-harmonic tone plus noise, so that voiced frames exist), at the LibriTTS
geometry the reference's f0_torchyin call gives (24 kHz, hop 300, frame_length = win_length 1200: tau_min 2,
tau_max 600, W = 1200) and at LJSpeech's (22.05 kHz, hop 256, win_length 1024: tau_max 512). Two legs per
setting, each timed with a HIP event pair around the calls on the current stream, alternated step by step
in one process:
  engine   one pwg_yin_run over the packed batch (the output allocation included);
  eager    torch fp32 on the same GPU, utterance by utterance: unfold + rfft / irfft (the difference
           function through the autocorrelation and cumulative energies) + cumsum + threshold and
           first-minimum search by argmax.
Reported per leg: median, min, max over the timed steps after the warm-up; the share of frames on which the
two legs give the same f0; and the engine leg's share of one UHiFiGAN step from f0 (uhifigan_v1 on the same
frame counts: host clock around a synchronised ``inference_batch_from_f0``). No clock is pinned.

    python tools/yin_bench.py --out profiles/yin/bench.json
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

from parallelwavegan_amd import UHiFiGANGenerator, YinF0Extractor, configs, synthetic  # noqa: E402

SETTINGS = {"libritts": (24000, 300, 1200), "ljspeech": (22050, 256, 1024)}


def eager_yin(x, fs, tau_min, tau_max, hop, threshold=0.1):
    """The estimator in torch eager fp32, d through rfft / irfft: (frames,) f0 in Hz."""
    W = 2 * tau_max
    fr = x.unfold(0, W, hop)
    spec = torch.fft.rfft(fr, 2 * W)
    r = torch.fft.irfft(spec * spec.conj(), 2 * W)[:, :tau_max]
    cs = torch.nn.functional.pad(torch.cumsum(fr * fr, 1), (1, 0))
    tau = torch.arange(tau_max, device=x.device)
    d = cs[:, W - tau] + (cs[:, W:W + 1] - cs[:, tau]) - 2.0 * r
    lag = torch.arange(1, tau_max, dtype=torch.float32, device=x.device)
    c = (d[:, 1:] * lag / torch.clamp(torch.cumsum(d[:, 1:], 1), min=1e-5))[:, tau_min:]
    # first True of a row by argmax over a weight that falls along the row: the maximum is unique (a plain
    # argmax over equal values may return any of them on the GPU)
    L = c.shape[1]
    fall = torch.arange(L, 0, -1, device=x.device)[None]
    below = c < threshold
    fb = (below * fall).argmax(1)                                    # 0 when no value is below the threshold
    rising = torch.cat([(c[:, 1:] - c[:, :-1]) >= 0, torch.ones_like(c[:, :1], dtype=torch.bool)], 1)
    k = ((rising & (torch.arange(L, device=x.device)[None] >= fb[:, None])) * fall).argmax(1) * (fb > 0)
    return torch.where(k > 0, float(fs) / (k + tau_min + 1).float(), torch.zeros_like(k, dtype=torch.float32))


def stats(v):
    v = np.asarray(v)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))


def tone(n, fs, rs):
    t = np.arange(n) / fs
    f = 150.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(f) / fs
    x = sum(a * np.sin(h * ph) for h, a in ((1, 0.3), (2, 0.15), (3, 0.1), (4, 0.05))) + 0.002 * rs.standard_normal(n)
    x[: n // 4] = 0.05 * rs.standard_normal(n // 4)
    return x.astype(np.float32)


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
    res = dict(utterances=len(frames), n_frames=int(sum(frames)), steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(dev),
               clock_note="device clocks not pinned; legs alternated step by step in one process")
    with torch.no_grad():
        for name, (sr, hop, win) in SETTINGS.items():
            ex = YinF0Extractor(sr, hop, frame_length=win, log=False)
            rs = np.random.RandomState(5)
            waves = [torch.from_numpy(tone(f * hop, sr, rs)).to(dev) for f in frames]
            packed, lengths = torch.cat(waves), [f * hop for f in frames]
            plan = ex.plan(dev)
            out = {}

            def leg_engine():
                out["engine"] = plan.run(packed, lengths)[0]

            def leg_eager():
                out["eager"] = torch.cat([eager_yin(w, sr, ex.tau_min, ex.tau_max, hop) for w in waves])

            legs = {"engine": leg_engine, "eager": leg_eager}
            times = {k: [] for k in legs}
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
            rows = int(out["engine"].shape[0])
            W = 2 * ex.tau_max
            terms = rows * sum(W - t for t in range(ex.tau_max))
            res[name] = dict(sampling_rate=sr, hop_size=hop, frame_length=win, tau_min=ex.tau_min, tau_max=ex.tau_max,
                             n_samples=int(sum(lengths)), rows=rows, workgroups=sum((plan.frames(t) + 7) // 8 for t in lengths),
                             **{k: stats(v) for k, v in times.items()},
                             voiced_share=float((out["engine"] > 0).float().mean()),
                             frames_equal_eager_vs_engine=float((out["engine"] == out["eager"]).float().mean()),
                             squared_differences=int(terms))
            med = res[name]["engine"]["median_ms"]
            res[name]["eager_over_engine"] = res[name]["eager"]["median_ms"] / med
            res[name]["engine_gterms_per_s"] = terms / med / 1e6

        # one UHiFiGAN step from f0 (uhifigan_v1) on the same frame counts
        params = configs.uhifigan_params("uhifigan_v1")
        m = UHiFiGANGenerator(**params)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_module_state_dict(m, seed=0).items()})
        m = m.eval().to(dev)
        cs = [torch.from_numpy(synthetic.make_mel(f, params["in_channels"], seed=10 + i)).to(dev) for i, f in enumerate(frames)]
        f0s = [torch.full((f,), 150.0, device=dev) for f in frames]
        step = []
        for i in range(2 + 5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            m.inference_batch_from_f0(cs, f0s, 24000, "tile")
            torch.cuda.synchronize(dev)
            if i >= 2:
                step.append((time.perf_counter() - t0) * 1e3)
    res["uhifigan_step_from_f0"] = stats(step)
    res["engine_share_of_uhifigan_step"] = res["libritts"]["engine"]["median_ms"] / res["uhifigan_step_from_f0"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
