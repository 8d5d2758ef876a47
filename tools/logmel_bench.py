#!/usr/bin/env python3
"""Time the HIP log-mel extractor (include/pwg_mel.h) on the benchmark batch.

Workload: the 16 ragged utterances of the README's PWG benchmark (synthetic.libritts_lengths), each
of frames x hop samples of seeded noise, at two recipe settings: LibriTTS (24 kHz, fft 2048, hop 300,
win 1200) and LJSpeech (22.05 kHz, fft 1024, hop 256, win 1024), 80 mels, 80-7600 Hz. Two legs per
setting, each timed with a HIP event pair around the calls on the current stream, alternated step by
step in one process:
  engine   one pwg_mel_run over the packed batch (the output allocation included);
  eager    torch on the same GPU, utterance by utterance: torch.stft (periodic Hann, reflect) + power +
           sqrt + matmul with the same mel matrix + clamp + log10 (losses/mel_loss.py without the clamp
           of the power, i.e. bin/preprocess.py's form).
Reported per leg: median, min, max over the timed steps after the warm-up; the largest difference between
the legs; and the engine leg's share of one libritts_v1 ParallelWaveGAN ``inference_batch`` step on the
same utterances (host clock around a synchronised call). No clock is pinned.

    python tools/logmel_bench.py --out profiles/logmel/bench.json
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

from parallelwavegan_amd import LogMelExtractor, ParallelWaveGANGenerator, configs, synthetic  # noqa: E402

SETTINGS = {"libritts": (24000, 2048, 300, 1200), "ljspeech": (22050, 1024, 256, 1024)}


def eager_logmel(x, n_fft, hop, win, window, melmat_t, eps=1e-10):
    st = torch.stft(x[None], n_fft, hop, win, window=window, center=True, return_complex=True)[0]
    amp = torch.sqrt(st.real ** 2 + st.imag ** 2).T
    return torch.log10(torch.clamp(amp @ melmat_t, min=eps))


def stats(v):
    v = np.asarray(v)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))


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
        for name, (sr, n_fft, hop, win) in SETTINGS.items():
            ex = LogMelExtractor(sr, n_fft, hop, win, 80, 80, 7600)
            rs = np.random.RandomState(5)
            waves = [torch.from_numpy((0.1 * rs.standard_normal(f * hop)).astype(np.float32)).to(dev) for f in frames]
            packed, lengths = torch.cat(waves), [f * hop for f in frames]
            plan = ex.plan(dev)
            window = torch.hann_window(win, device=dev)
            melmat_t = torch.from_numpy(ex.melmat.T.copy()).to(dev)
            out = {}

            def leg_engine():
                out["engine"] = plan.run(packed, lengths)

            def leg_eager():
                out["eager"] = torch.cat([eager_logmel(w, n_fft, hop, win, window, melmat_t) for w in waves])

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
            n_bins = n_fft // 2
            kp = (win + 7) // 8 * 8
            rows = int(out["engine"].shape[0])
            tiles = sum((1 + t // hop + 63) // 64 for t in lengths)
            res[name] = dict(sampling_rate=sr, fft_size=n_fft, hop_size=hop, win_length=win, n_samples=int(sum(lengths)),
                             rows=rows, workgroups=tiles, **{k: stats(v) for k, v in times.items()},
                             max_abs_diff_eager_vs_engine=float((out["engine"] - out["eager"]).abs().max()),
                             dft_gflop=2.0 * 2 * n_bins * kp * 64 * tiles / 1e9,
                             basis_l2_gbytes=4.0 * 2 * n_bins * kp * tiles / 1e9)
            res[name]["eager_over_engine"] = res[name]["eager"]["median_ms"] / res[name]["engine"]["median_ms"]

        # one ParallelWaveGAN step (libritts_v1) on the same utterances
        params = configs.generator_params("libritts_v1")
        sd = synthetic.make_state_dict(params, seed=0)
        m = ParallelWaveGANGenerator(**configs.generator_params("libritts_v1"))
        m.remove_weight_norm()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m = m.eval().to(dev)
        cs = [torch.from_numpy(synthetic.make_mel(f, 80, seed=10 + i)).to(dev) for i, f in enumerate(frames)]
        xs = [torch.randn(f * 300, 1, device=dev) for f in frames]
        step = []
        for i in range(2 + 5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            m.inference_batch(cs, xs)
            torch.cuda.synchronize(dev)
            if i >= 2:
                step.append((time.perf_counter() - t0) * 1e3)
    res["pwg_step"] = stats(step)
    res["engine_share_of_pwg_step"] = res["libritts"]["engine"]["median_ms"] / res["pwg_step"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
