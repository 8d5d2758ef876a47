#!/usr/bin/env python3
"""Time VQVAE (HIP first layer, grouped strided levels, code search and decoder front end; dense tail
and decoder on the conv-network executor) against torch eager on the same GPU.

Workload: vqvae_v3 (24 kHz, hop 64, local 2 -> 32 and global 128 x 128 conditioning) with seeded
weights, 16 ragged utterances of synthetic.libritts_lengths(16) * 100 + 7 i samples (0.3 to 5 s, no
multiples of the hop), wav -> codes -> wav. Two legs, alternated step by step in one process:
  hip    ``inference_batch`` over the whole batch;
  eager  the same graph in torch fp32 on the same GPU over the drop-in's own parameter holders (the
         encoder's Sequentials with F.conv1d(groups=...), the reference's addmm distance and torch.min,
         embedding / 1x1 conv / concatenation, the decoder's Sequential; eval mode, weight norm
         removed), utterance by utterance as the reference's decode loop runs them.
Each step is timed with a host clock around work that ends in a device synchronise, after warm-up steps
of both legs; reported per leg: median, min, max over the timed steps. A separate pass records one HIP
event at the end of every stage (VQVAE.stage_events) and gives the device milliseconds per stage: first
layer, each grouped level, dense tail (it includes the executor's range-status read, one host round
trip), search, decoder front end, decoder. The two legs' outputs are compared: waveforms on the
utterances whose codes agree, and the share of frames whose codes agree.
The clocks are whatever the device runs at: no clock is pinned (recorded as ``clock_note``).

    python tools/vqvae_bench.py --out profiles/vqvae_bench.json
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

from parallelwavegan_amd import VQVAE, configs, synthetic  # noqa: E402
from parallelwavegan_amd.melgan import ResidualStack  # noqa: E402


def eager_decoder(dec, h):
    for mod in dec.melgan:
        h = mod.stack(h) + mod.skip_layer(h) if isinstance(mod, ResidualStack) else mod(h)
    return h


def eager_forward(m, x, l, g):
    """models/vqvae.py:113-147 over the drop-in's torch modules: x (T,), l (T', num_local), g int."""
    h = x.view(1, 1, -1)
    for f in m.encoder.layers:
        h = f(h)
    z = h[0].T.contiguous()
    book = m.codebook.embedding.weight
    d = torch.addmm(torch.sum(book ** 2, dim=1) + torch.sum(z ** 2, dim=1, keepdim=True), z, book.t(), alpha=-2.0, beta=1.0)
    idx = torch.min(d, dim=1)[1]
    parts = [book[idx].T.unsqueeze(0)]
    if l is not None:
        parts.append(m.local_embed(l.T.unsqueeze(0)))
    if g is not None:
        parts.append(m.global_embed.weight[g].view(1, -1, 1).expand(-1, -1, idx.numel()))
    return eager_decoder(m.decoder, torch.cat(parts, dim=1))[0].T, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vqvae_v3")
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a ROCm GPU")
    dev = torch.device("cuda:0")
    params = configs.vqvae_params(args.config)
    m = VQVAE(**configs.vqvae_params(args.config))
    sd = synthetic.make_module_state_dict(m, seed=0)
    # a codebook where the encoder outputs are (tests/golden/make_golden_vqvae.py)
    n_layers = len(params["encoder_conf"]["downsample_scales"]) + 3
    sd["codebook.embedding.weight"] = (0.04 * sd["codebook.embedding.weight"]
                                       + sd[f"encoder.layers.{n_layers - 1}.bias"][None, :]).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.remove_weight_norm()
    m = m.eval().to(dev)
    hop = m.downsample_factor
    lens = [int(f) * 100 + 7 * i for i, f in enumerate(synthetic.libritts_lengths(args.utts))]
    frames = [-(-n // hop) for n in lens]
    rs = np.random.RandomState(1)
    xs = [torch.from_numpy((0.3 * rs.standard_normal(n)).astype(np.float32)).to(dev) for n in lens]
    ls = gs = None
    if params.get("num_local_embeds") is not None:
        ls = [torch.from_numpy(rs.standard_normal((f, params["num_local_embeds"])).astype(np.float32)).to(dev) for f in frames]
    if params.get("num_global_embeds") is not None:
        gs = [int(v) for v in rs.randint(params["num_global_embeds"], size=len(lens))]

    def leg_hip():
        return m.inference_batch(xs, ls, gs)

    def leg_eager():
        outs = [eager_forward(m, x, None if ls is None else ls[u], None if gs is None else gs[u]) for u, x in enumerate(xs)]
        return [o[0] for o in outs], [o[1] for o in outs]

    legs = {"hip": leg_hip, "eager": leg_eager}
    times = {k: [] for k in legs}
    with torch.no_grad():
        for _ in range(args.warmup):
            outs = {k: fn() for k, fn in legs.items()}
        torch.cuda.synchronize(dev)
        same = [bool(torch.equal(a, b)) for a, b in zip(outs["hip"][1], outs["eager"][1])]
        agree = sum(int((a == b).sum()) for a, b in zip(outs["hip"][1], outs["eager"][1])) / float(sum(frames))
        diffs = [float((a - b).abs().max()) for a, b, s in zip(outs["hip"][0], outs["eager"][0], same) if s]
        del outs
        for _ in range(args.steps):
            for k, fn in legs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3)
        runs = []
        for _ in range(4):
            m.stage_events = []
            leg_hip()
            torch.cuda.synchronize(dev)
            ev, m.stage_events = m.stage_events, None
            stage = {}
            for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
                if name not in ("begin", "decode_begin"):
                    stage[name] = a.elapsed_time(b)
            runs.append(stage)

    def stats(v):
        v = np.asarray(v)
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), n=int(v.size))

    stage_ms = {k: float(np.median([r[k] for r in runs[1:]])) for k in runs[0]}
    levels = sum(v for k, v in stage_ms.items() if k.startswith("level_"))
    samples = int(sum(lens))
    res = dict(config=args.config, utterances=len(lens), samples=samples, frames=int(sum(frames)), steps=args.steps,
               warmup=args.warmup, hip=stats(times["hip"]), eager=stats(times["eager"]),
               code_agreement_hip_vs_eager=agree, utterances_with_equal_codes=int(sum(same)),
               max_abs_diff_hip_vs_eager_on_those=max(diffs) if diffs else None,
               stage_ms=stage_ms, grouped_levels_ms=levels, grouped_levels_over_dense_tail=levels / stage_ms["dense_tail"],
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
