#!/usr/bin/env python3
"""Decode dumped features with the MI355X engine: the ``parallel-wavegan-decode`` CLI
(/root/reference/parallel_wavegan/bin/decode.py:31-268) for the accelerated generator types.

Same arguments for the mel-to-wave case (--dumpdir with ``*-feats.npy`` files, --outdir,
--checkpoint, --config, --normalize-before, --verbose) and the same outputs
(``{outdir}/{utt_id}_gen.wav``, PCM_16, and the mean per-utterance RTF in the log). Differences:
  * utterances are decoded in ragged BATCHES of up to --batch-frames mel frames per engine pass
    (the reference runs one utterance per call), by default sized from the free device memory;
    the logged RTF is per batch wall time / audio;
  * features are read lazily: lengths from the .npy headers, data per batch of the rank's shard;
  * under ``torch.distributed.run`` every rank decodes its LPT share of the utterances on its own
    GPU (sharding.decode_sharded) and writes its own wavs;
  * --scp (kaldiio) and hdf5 dumps are not available in this image: they raise;
  * --use-f0 (DiscreteSymbolF0Generator only; any other generator raises) reads ``*-f0.npy`` beside
    each ``*-feats.npy``, as the reference's npy branch does (bin/decode.py:185-252);
  * DiscreteSymbolDurationGenerator decodes in three steps: the durations of a batch of token
    sequences are predicted (predict_durations), the engine passes are then sized by the regulated
    frame counts instead of the token counts, and the tokens are decoded with ``ds=`` (host-resident
    durations: no further device-to-host traffic);
  * UHiFiGANGenerator reads ``*-excitation.npy`` beside each ``*-feats.npy`` (bin/decode.py:188-192 of
    the reference) and fails before any decoding when one is missing; ``*-f0.npy`` is read if present
    and otherwise ignored (the generator never uses f0, models/uhifigan.py:261-301). With
    --excitation-from-f0 {tile,hold} (an addition) no excitation dump is needed: ``*-f0.npy`` beside each
    ``*-feats.npy`` is padded (edge) or trimmed to the mel length (bin/preprocess.py:427-430 of the reference)
    and the excitation is generated on the GPU (UHiFiGANGenerator.inference_batch_from_f0) at
    ``sampling_rate_for_feats`` if the config has it, else ``sampling_rate``; ``tile`` is the layout the
    reference's preprocessing produces. --excitation-seed seeds the noise term's device draws;
  * VQVAE takes the reference's VQ-WAV2WAV branch (bin/decode.py:274-387) for ``format: npy`` dumps: it
    reads ``*-wave.npy`` (and ``*-local.npy`` / ``*-global.npy`` beside each when the config sets
    use_local_condition / use_global_condition), runs wav -> codes -> wav over ragged batches
    (VQVAE.inference_batch), writes ``<utt>_gen.wav`` and ``<outdir>/text`` with ``utt_id sym sym ...``
    per line. One process only;
  * DiscreteSymbolStyleMelGANGenerator reads (T, 2) [token id, speaker id] arrays from ``*-feats.npy`` like
    every token vocoder; --spk-id (an addition) replaces the speaker column, so that (T,) or (T, 1) id files
    decode too. It draws its noise on the device per batch.
"""

import argparse
import logging
import os
import sys
import time

import numpy as np
import torch


def engines_of(model):
    """The HIP engine(s) a drop-in module holds (PWG: one; MelGAN: one per PQMF setting)."""
    if hasattr(model, "_engines"):
        return [e[0] for e in model._engines.values()]
    return [model.engine()]


def batch_cost_model(model, device, frac=0.25, cap_gib=8.0, probe_frames=512, probe_utts=8):
    """Bytes of one engine pass as a function of (mel frames, utterances) and the budget they must
    fit: ``frac`` of the free device memory, at most ``cap_gib``. Per frame: the plan workspace of
    a one-utterance probe, plus the caller's mel input (4 B x input channels) and noise / output
    (4 B per audio sample and output channel, the noise for PWG only). Per utterance: what a probe
    of ``probe_utts`` equal utterances of the same total length adds over the one-utterance probe
    (segment gaps and tile padding). Channel counts and samples per frame come from the model."""
    eng = model.engine()
    if type(model).__name__ == "DiscreteSymbolStyleMelGANGenerator":
        # a trimmed TADE plan; per frame besides it: two int64 ids, the noise column's share, the audio out
        from parallelwavegan_amd._lib import PWG_SMG_PLAN_TRIM_NOISE as trim

        nf, hop = int(model.noise_upsample_factor), int(model.upsample_factor)
        each = probe_frames // probe_utts
        one = eng.plan([probe_frames], [(probe_frames - 1) // nf + 1], trim).workspace_bytes
        many = eng.plan([each] * probe_utts, [(each - 1) // nf + 1] * probe_utts, trim).workspace_bytes
        per_frame = one / probe_frames + 16 + 4 * model.in_channels / nf + 4 * hop * model.out_channels
        free, _ = torch.cuda.mem_get_info(device)
        return per_frame, max(0.0, (many - one) / (probe_utts - 1)), min(free * frac, cap_gib * (1 << 30))
    if hasattr(model, "aux_channels"):  # ParallelWaveGANGenerator: mel in, noise in, audio out
        in_ch, hop, out_ch, noise = model.aux_channels, model.upsample_factor, model.out_channels, 1
    else:  # MelGAN family: the program's input channels, output rate (PQMF included) and channels
        in_ch, hop, out_ch, noise = eng.program.channels[0], eng.hop, eng.out_channels, 0
    one = eng.plan([probe_frames]).workspace_bytes
    many = eng.plan([probe_frames // probe_utts] * probe_utts).workspace_bytes
    per_frame = one / probe_frames + 4 * in_ch + 4 * hop * (out_ch + noise)
    ext = getattr(getattr(eng, "program", None), "external", -1)
    if ext >= 0:  # UHiFiGAN: the excitation samples and the front end's rows (the external buffer)
        per_frame += 4 * eng.program.rate[ext] * (1 + eng.program.channels[ext])
    per_utt = max(0.0, (many - one) / (probe_utts - 1))
    free, _ = torch.cuda.mem_get_info(device)
    budget = min(free * frac, cap_gib * (1 << 30))
    return per_frame, per_utt, budget


def excitation_files(feats_files):
    """The ``*-excitation.npy`` file beside each ``*-feats.npy`` (UHiFiGANGenerator); raises
    FileNotFoundError naming the first utterances that lack one."""
    paths = [f[:-len("-feats.npy")] + "-excitation.npy" for f in feats_files]
    missing = [p for p in paths if not os.path.exists(p)]
    if missing:
        raise FileNotFoundError(f"UHiFiGANGenerator needs an excitation dump beside every feature file: "
                                f"{len(missing)} missing, first {missing[0]}")
    return paths


def f0_files(feats_files):
    """The ``*-f0.npy`` file beside each ``*-feats.npy`` (--excitation-from-f0); raises
    FileNotFoundError naming the first utterances that lack one."""
    paths = [f[:-len("-feats.npy")] + "-f0.npy" for f in feats_files]
    missing = [p for p in paths if not os.path.exists(p)]
    if missing:
        raise FileNotFoundError(f"--excitation-from-f0 needs an f0 dump beside every feature file: "
                                f"{len(missing)} missing, first {missing[0]}")
    return paths


def fit_f0(f0, frames):
    """f0 trimmed, or padded with its last value, to the mel length (bin/preprocess.py:427-430)."""
    f0 = np.ascontiguousarray(f0, np.float32).reshape(-1)
    if len(f0) >= frames:
        return f0[:frames]
    if len(f0) == 0:
        raise ValueError("an empty f0 contour cannot be padded")
    return np.pad(f0, (0, frames - len(f0)), mode="edge")


def vq_condition_files(wave_files, use_local, use_global):
    """The ``*-local.npy`` / ``*-global.npy`` files beside each ``*-wave.npy`` (None for a part the
    config does not use); raises FileNotFoundError naming the first missing one."""
    out = []
    for on, tag in ((use_local, "local"), (use_global, "global")):
        if not on:
            out.append(None)
            continue
        paths = [f[:-len("-wave.npy")] + f"-{tag}.npy" for f in wave_files]
        missing = [p for p in paths if not os.path.exists(p)]
        if missing:
            raise FileNotFoundError(f"use_{tag}_condition is set: VQVAE needs a {tag} dump beside every wave file: "
                                    f"{len(missing)} missing, first {missing[0]}")
        out.append(paths)
    return out


def decode_vq(args, config, model, device):
    """The VQ-WAV2WAV branch: every ``*-wave.npy`` of --dumpdir through VQVAE.inference_batch."""
    from parallelwavegan_amd.utils import find_files, log_rtf, write_pcm16_wav

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("VQVAE decoding is not sharded: run one process")
    files = find_files(args.dumpdir, "*-wave.npy")
    use_local, use_global = bool(config.get("use_local_condition")), bool(config.get("use_global_condition"))
    local_files, global_files = vq_condition_files(files, use_local, use_global)
    utt_ids = [os.path.basename(f).replace("-wave.npy", "") for f in files]
    lengths = [int(np.prod(np.load(f, mmap_mode="r", allow_pickle=False).shape)) for f in files]
    logging.info(f"The number of features to be decoded = {len(files)}.")
    hop = model.downsample_factor
    limit = args.batch_frames * hop if args.batch_frames is not None else 1 << 22  # samples per pass
    sr = config["sampling_rate"]
    model.remove_weight_norm()
    model = model.eval().to(device)
    batches, cur, n = [], [], 0
    for i, t in enumerate(lengths):
        if cur and n + t > limit:
            batches.append(cur)
            cur, n = [], 0
        cur.append(i)
        n += t
    if cur:
        batches.append(cur)
    total_rtf, done = 0.0, 0
    with open(os.path.join(config["outdir"], "text"), "w") as text:
        for batch in batches:
            xs = [np.ascontiguousarray(np.load(files[i], allow_pickle=False), np.float32).reshape(-1) for i in batch]
            ls = gs = None
            if use_local:
                ls = [np.ascontiguousarray(np.load(local_files[i], allow_pickle=False), np.float32) for i in batch]
            if use_global:
                gs = [int(np.asarray(np.load(global_files[i], allow_pickle=False)).reshape(-1)[0]) for i in batch]
            start = time.time()
            with torch.no_grad():
                ys, zs = model.inference_batch(xs, ls, gs)
                ys = [y.view(-1).cpu().numpy() for y in ys]
                zs = [z.view(-1).cpu().numpy() for z in zs]
            el = time.time() - start
            total_rtf += el / (sum(len(y) for y in ys) / sr) * len(ys)
            done += len(ys)
            for i, y, z in zip(batch, ys, zs):
                write_pcm16_wav(os.path.join(config["outdir"], f"{utt_ids[i]}_gen.wav"), y, sr)
                text.write(f"{utt_ids[i]} {' '.join(str(int(v)) for v in z)}\n")
    log_rtf(done, total_rtf)
    for eng in (model._tail, model.decoder.engine(False)):
        eng.release_workspace()
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description="Decode dumped features with the MI355X generator engine.")
    ap.add_argument("--scp", default=None, type=str)
    ap.add_argument("--dumpdir", default=None, type=str)
    ap.add_argument("--segments", default=None, type=str)
    ap.add_argument("--outdir", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--config", default=None, type=str)
    ap.add_argument("--normalize-before", default=False, action="store_true")
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--use-f0", default=False, action="store_true")
    ap.add_argument("--spk-id", type=int, default=None,
                    help="DiscreteSymbolStyleMelGANGenerator only: the speaker id of every utterance (replaces the "
                         "second column of the id files, which may then be (T,) or (T, 1))")
    ap.add_argument("--excitation-from-f0", choices=("tile", "hold"), default=None,
                    help="UHiFiGANGenerator only: generate the excitation on the GPU from *-f0.npy instead of reading "
                         "*-excitation.npy (tile: the contour repeated hop times, as the reference's preprocessing; "
                         "hold: every frame held for hop samples)")
    ap.add_argument("--excitation-seed", type=int, default=None,
                    help="with --excitation-from-f0: seed of the noise term's draws on the device")
    ap.add_argument("--batch-frames", type=int, default=None,
                    help="max mel frames per engine pass (ragged batch); default: sized from free device "
                         "memory (--batch-mem-frac of it, at most --batch-mem-gib)")
    ap.add_argument("--batch-mem-frac", type=float, default=0.25)
    ap.add_argument("--batch-mem-gib", type=float, default=8.0)
    args = ap.parse_args(argv)

    level = logging.DEBUG if args.verbose > 1 else (logging.INFO if args.verbose > 0 else logging.WARN)
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")

    from parallelwavegan_amd import sharding
    from parallelwavegan_amd.utils import find_files, load_model, log_rtf, read_config, write_pcm16_wav

    if args.scp is not None or args.segments is not None:
        raise NotImplementedError("--scp/--segments need kaldiio, which is not available; use --dumpdir (for a VQVAE: "
                                  "a --dumpdir of *-wave.npy files)")
    if args.dumpdir is None:
        raise ValueError("Please specify either --dumpdir or --feats-scp.")
    os.makedirs(args.outdir, exist_ok=True)
    cfg_path = args.config or os.path.join(os.path.dirname(args.checkpoint), "config.yml")
    config = read_config(cfg_path)
    config.update(vars(args))
    if config.get("format", "npy") != "npy":
        raise NotImplementedError("hdf5 dumps need h5py, which is not available; dump with format: npy")

    uhifigan = config.get("generator_type") == "UHiFiGANGenerator"
    if args.excitation_from_f0 is not None and not uhifigan:
        raise NotImplementedError(f"--excitation-from-f0 applies to a UHiFiGANGenerator (got "
                                  f"{config.get('generator_type')})")
    exc_files = exc_f0_files = None
    if uhifigan and args.excitation_from_f0 is not None:
        exc_f0_files = f0_files(find_files(args.dumpdir, "*-feats.npy"))
    elif uhifigan:
        exc_files = excitation_files(find_files(args.dumpdir, "*-feats.npy"))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0
    if world > 1:
        import torch.distributed as dist

        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        rank = dist.get_rank()
    if not torch.cuda.is_available():
        raise RuntimeError("the MI355X engine needs a ROCm GPU (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())

    model = load_model(args.checkpoint, config)
    if config.get("generator_type") == "VQVAE":
        if args.use_f0 or args.normalize_before:
            raise NotImplementedError("--use-f0 / --normalize-before do not apply to a VQVAE (it decodes waveforms)")
        return decode_vq(args, config, model, device)
    if args.normalize_before:
        assert hasattr(model, "mean"), "Feature stats are not registered."
        assert hasattr(model, "scale"), "Feature stats are not registered."
    from parallelwavegan_amd.dsym_variants import DiscreteSymbolDurationGenerator, DiscreteSymbolF0Generator

    if args.use_f0 and not (isinstance(model, DiscreteSymbolF0Generator) and model.use_f0):
        raise NotImplementedError(f"--use-f0 needs a DiscreteSymbolF0Generator with use_f0 (got "
                                  f"{type(model).__name__}); other f0 generators are not accelerated")
    if isinstance(model, DiscreteSymbolF0Generator) and model.use_f0 and not args.use_f0:
        raise ValueError("this generator was trained with use_f0: pass --use-f0 (and dump *-f0.npy files)")
    with_durations = isinstance(model, DiscreteSymbolDurationGenerator)
    smg_tokens = type(model).__name__ == "DiscreteSymbolStyleMelGANGenerator"
    if args.spk_id is not None and not smg_tokens:
        raise NotImplementedError(f"--spk-id applies to a DiscreteSymbolStyleMelGANGenerator (got {type(model).__name__})")
    model.remove_weight_norm()
    model = model.eval().to(device)

    files = find_files(args.dumpdir, "*-feats.npy")
    utt_ids = [os.path.basename(f).replace("-feats.npy", "") for f in files]
    # lengths from the .npy headers only (memory-mapped, nothing read); each rank loads the
    # features of its own shard, one batch at a time
    lengths = [int(np.load(f, mmap_mode="r", allow_pickle=False).shape[0]) for f in files]
    logging.info(f"The number of features to be decoded = {len(files)}.")
    sr = config["sampling_rate"]
    exc_sr = config.get("sampling_rate_for_feats") or sr
    if exc_f0_files is not None and args.excitation_seed is not None:
        torch.manual_seed(args.excitation_seed)
    if args.batch_frames is None:
        per_frame, per_utt, budget = batch_cost_model(model, device, args.batch_mem_frac, args.batch_mem_gib)
        logging.info(f"batch budget: {budget / 2**30:.2f} GiB, {per_frame:.0f} B per mel frame + {per_utt:.0f} B "
                     f"per utterance")

        def fits(nfr, nutt):
            return nfr * per_frame + nutt * per_utt <= budget
    else:
        def fits(nfr, nutt):
            return nfr <= args.batch_frames

    def load_feats(i):
        return torch.from_numpy(np.ascontiguousarray(np.load(files[i], allow_pickle=False), np.float32))

    def batches(idx, size):
        """``idx`` cut into consecutive runs that fit one engine pass; size[i]: frames of file i."""
        batch, nfr = [], 0
        for slot, i in enumerate(idx):
            if batch and not fits(nfr + size[i], len(batch) + 1):
                yield batch
                batch, nfr = [], 0
            batch.append((slot, i))
            nfr += size[i]
        if batch:
            yield batch

    def decode(idx):
        outs = [None] * len(idx)
        total_rtf, n = 0.0, 0
        size, durations, predict_time = lengths, {}, {}
        if with_durations:
            # step 1: predicted durations per batch of token sequences; step 2 (below): the engine
            # passes are sized by the regulated frame counts
            size = list(lengths)
            for batch in batches(idx, lengths):
                start = time.time()
                with torch.no_grad():
                    ds = model.predict_durations([load_feats(i) for _, i in batch])
                ds = [d.cpu().numpy() for d in ds]
                for (_, i), d in zip(batch, ds):
                    durations[i] = d
                    size[i] = int(d.sum()) or len(d)  # (all-zero durations count as all ones)
                    predict_time[i] = (time.time() - start) / len(batch)

        for batch in batches(idx, size):
            cs = [load_feats(i) for _, i in batch]
            kwargs = {}
            if args.use_f0:
                kwargs["f0s"] = [np.ascontiguousarray(np.load(files[i].replace("-feats.npy", "-f0.npy"),
                                                              allow_pickle=False), np.float32).reshape(-1)
                                 for _, i in batch]
            if with_durations:
                kwargs["ds"] = [durations[i] for _, i in batch]
            if smg_tokens and args.spk_id is not None:
                kwargs["g"] = args.spk_id
            if exc_f0_files is not None:
                f0s = [fit_f0(np.load(exc_f0_files[i], allow_pickle=False), lengths[i]) for _, i in batch]
            elif uhifigan:
                excs = [np.ascontiguousarray(np.load(exc_files[i], allow_pickle=False), np.float32).reshape(-1)
                        for _, i in batch]
                for _, i in batch:  # read like the reference does, never used by the generator
                    f0_path = files[i].replace("-feats.npy", "-f0.npy")
                    if os.path.exists(f0_path):
                        np.load(f0_path, allow_pickle=False)
            start = time.time()
            with torch.no_grad():
                if exc_f0_files is not None:
                    ys = model.inference_batch_from_f0(cs, f0s, exc_sr, args.excitation_from_f0)
                elif uhifigan:
                    ys = model.inference_batch(cs, excs)
                else:
                    ys = model.inference_batch(cs, normalize_before=args.normalize_before, **kwargs)
                ys = [y.view(-1).cpu().numpy() for y in ys]
            el = time.time() - start + sum(predict_time.get(i, 0.0) for _, i in batch)
            audio = sum(len(y) for y in ys) / sr
            total_rtf += el / audio * len(ys)
            n += len(ys)
            for (slot, i), y in zip(batch, ys):
                write_pcm16_wav(os.path.join(config["outdir"], f"{utt_ids[i]}_gen.wav"), y, sr)
                outs[slot] = len(y)
        log_rtf(n, total_rtf)
        return outs

    local = sharding.decode_sharded(lengths, decode)
    logging.info(f"rank {rank}: wrote {len(local)} utterances to {config['outdir']}")
    for eng in engines_of(model):
        eng.release_workspace()
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
