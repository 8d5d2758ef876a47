#!/usr/bin/env python3
"""Dump log-mel features of a directory of wavs with the MI355X engine: the mel branch of the
``parallel-wavegan-preprocess`` CLI (parallel_wavegan/bin/preprocess.py:348-405, 454-493) and, with
--stats, of ``parallel-wavegan-normalize`` (bin/normalize.py), for ``format: npy``.

    python -m parallelwavegan_amd.bin.preprocess --rootdir WAVS --dumpdir DUMP --config conf.yml [--stats stats.npy]
                                                 [--extract-f0-yin] [--condition-audio] [--resample-input]

Every ``*.wav`` under --rootdir (PCM16 mono, at the config's sampling_rate) gives ``<utt>-feats.npy``
((frames, num_mels) float32) and ``<utt>-wave.npy`` (the audio edge-padded by fft_size and cut to
frames * hop_size samples, float32): the files the decode CLI reads. With --stats the features are
``(logmel - mean) / scale``, as bin/normalize.py writes them. The utterances are extracted in ragged
batches of up to --batch-samples samples per kernel launch.

With --extract-f0-yin every utterance also gives ``<utt>-f0.npy``: the (frames,) float32 log-f0 contour of
the YIN estimator (parallelwavegan_amd.yin, the reference's f0_torchyin call of bin/preprocess.py:420-430
with frame_length = win_length), computed on the fitted audio of ``<utt>-wave.npy`` in the same ragged
batches and fitted to the mel length by a cut or a hold of the last value; 0 marks an unvoiced frame. No
``<utt>-excitation.npy`` is written: ``decode --excitation-from-f0 tile`` generates the excitation from
the f0 on the GPU, and the reference's dump of it holds random noise in any case. The flag is opt-in and
separate from the reference's --extract-f0 (its pyreaper path, not available here).

With --condition-audio the waveform steps of the reference run on the GPU (parallelwavegan_amd.audio,
include/pwg_wave.h), in its order (bin/preprocess.py:359-452): the silence trim (trim_silence,
trim_threshold_in_db, trim_frame_size, trim_hop_size), a resampled copy for the mel when the config has
sampling_rate_for_feats (the mel hop is hop_size * sampling_rate_for_feats // sampling_rate), the fit of the
audio to frames * hop_size, the YIN f0 on the fitted audio before the gain, the global_gain_scale, and the
clipping check: an utterance whose peak reaches 1.0 is skipped with the reference's warning. An utterance that
is too short for fft_size after the trim raises for that file by name. With --resample-input a wav at
another rate than the config's is resampled to sampling_rate first (an extension: the reference asserts). The
resampler is a polyphase Kaiser-windowed sinc (scipy.signal.resample_poly's default), not librosa's soxr.
Both flags are opt-in; without them the config keys and the other rate raise as before.

Not available, each raising with a message: --scp / --segments (kaldiio), hdf5 dumps, the config keys use_f0 /
use_f0_and_excitation (use --extract-f0-yin), a window other than hann, and, without --condition-audio,
silence trimming, resampling (sampling_rate_for_feats) and a global gain.
"""

import argparse
import logging
import os
import sys

import numpy as np


def _check_header(path, w):
    if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
        raise ValueError(f"{path}: only 16 bit PCM wavs are read (sample width {w.getsampwidth()} bytes)")
    if w.getnchannels() != 1:
        raise ValueError(f"{path} seems to be multi-channel signal.")


def wav_header(path):
    """(samples, sampling rate) of a PCM16 mono wav, from its header alone."""
    import wave

    with wave.open(path, "rb") as w:
        _check_header(path, w)
        return w.getnframes(), w.getframerate()


def read_wav(path):
    """(float32 samples in [-1, 1), sampling rate) of a PCM16 mono wav, scaled by 1 / 32768 as soundfile does."""
    import wave

    with wave.open(path, "rb") as w:
        _check_header(path, w)
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        return data.astype(np.float32) / 32768.0, w.getframerate()


def check_config(config, condition_audio=False):
    """Raise for what this CLI leaves out; condition_audio: the --condition-audio flag."""
    if config.get("format", "npy") != "npy":
        raise NotImplementedError("hdf5 dumps need h5py, which is not available; dump with format: npy")
    if not condition_audio:
        if config.get("trim_silence", False):
            raise NotImplementedError("trim_silence is applied with --condition-audio only; pass the flag, or trim "
                                      "beforehand and set trim_silence: false")
        if "sampling_rate_for_feats" in config:
            raise NotImplementedError("sampling_rate_for_feats needs resampling, which runs with --condition-audio only")
        if float(config.get("global_gain_scale", 1.0) or 0.0) not in (0.0, 1.0):
            raise NotImplementedError("global_gain_scale other than 1.0 is applied with --condition-audio only; pass "
                                      "the flag, or scale the wavs beforehand")
    if config.get("use_f0") or config.get("use_f0_and_excitation"):
        raise NotImplementedError("f0 / excitation extraction is not available; dump *-f0.npy with another tool")
    if config.get("window", "hann") != "hann":
        raise NotImplementedError(f"window {config['window']!r} is not accelerated (hann only)")


def fit_audio(audio, frames, fft_size, hop_size):
    """bin/preprocess.py:403-405: the audio edge-padded by fft_size and cut to frames * hop_size."""
    audio = np.pad(audio, (0, fft_size), mode="edge")[: frames * hop_size]
    assert len(audio) == frames * hop_size
    return audio


def main(argv=None):
    ap = argparse.ArgumentParser(description="Dump log-mel features with the MI355X engine.")
    ap.add_argument("--wav-scp", "--scp", default=None, type=str)
    ap.add_argument("--segments", default=None, type=str)
    ap.add_argument("--rootdir", default=None, type=str)
    ap.add_argument("--dumpdir", type=str, required=True)
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--stats", default=None, type=str, help="stats.npy ((2, num_mels): mean, scale): normalise")
    ap.add_argument("--batch-samples", type=int, default=1 << 23, help="max samples per kernel launch")
    ap.add_argument("--extract-f0-yin", action="store_true",
                    help="also write <utt>-f0.npy: the YIN log-f0 contour, fitted to the mel length")
    ap.add_argument("--condition-audio", action="store_true",
                    help="honour the config's trim_silence, sampling_rate_for_feats and global_gain_scale on the GPU")
    ap.add_argument("--resample-input", action="store_true",
                    help="resample a wav at another rate to the config's sampling_rate instead of refusing it")
    ap.add_argument("--verbose", type=int, default=1)
    args = ap.parse_args(argv)

    level = logging.DEBUG if args.verbose > 1 else (logging.INFO if args.verbose > 0 else logging.WARN)
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")

    from parallelwavegan_amd.logmel import LogMelExtractor
    from parallelwavegan_amd.utils import find_files, read_config

    if args.wav_scp is not None or args.segments is not None:
        raise NotImplementedError("--wav-scp/--scp/--segments need kaldiio, which is not available; use --rootdir")
    if args.rootdir is None:
        raise ValueError("Please specify --rootdir.")
    config = read_config(args.config)
    check_config(config, args.condition_audio)
    stats = None
    if args.stats is not None:
        if not args.stats.endswith(".npy"):
            raise NotImplementedError("hdf5 statistics need h5py, which is not available; use a stats.npy")
        stats = np.load(args.stats, allow_pickle=False)
    sr, fft_size, hop = config["sampling_rate"], config["fft_size"], config["hop_size"]
    # the rate and hop the features are taken at (bin/preprocess.py:369-387)
    sr_feats, hop_feats = sr, hop
    conditioner = None
    if args.condition_audio or args.resample_input:
        from parallelwavegan_amd.audio import AudioConditioner, resample_out_len

        # without --condition-audio check_config has refused every key but sampling_rate
        conditioner = AudioConditioner.from_config(config)
        if conditioner.sampling_rate_for_feats is not None:
            sr_feats = conditioner.sampling_rate_for_feats
            if hop * sr_feats % sr != 0:
                raise ValueError("hop_size must be int value. please check sampling_rate_for_feats is correct.")
            hop_feats = hop * sr_feats // sr
    extractor = LogMelExtractor.from_config(dict(config, sampling_rate=sr_feats, hop_size=hop_feats), stats=stats)
    f0_extractor = None
    if args.extract_f0_yin:
        from parallelwavegan_amd.yin import YinF0Extractor

        # raises for a geometry it cannot take, before any write; the reference passes the features' rate and
        # hop here (bin/preprocess.py:421-426)
        f0_extractor = YinF0Extractor.from_config(dict(config, sampling_rate=sr_feats, hop_size=hop_feats))

    files = find_files(args.rootdir, "*.wav")
    logging.info(f"The number of files = {len(files)}.")
    lengths, rates = [], []
    for f in files:  # headers only: every refusal comes before the first sample is read or file written
        n, fs = wav_header(f)
        if fs != sr:
            if not args.resample_input:
                raise ValueError(f"{f} seems to have a different sampling rate ({fs} Hz, the config says {sr} Hz); "
                                 "--resample-input resamples it.")
            conditioner.check_ratio(fs, sr)
            n = resample_out_len(n, sr, fs)
        if (n if sr_feats == sr else resample_out_len(n, sr_feats, sr)) <= fft_size // 2:
            raise ValueError(f"{f} has {n} samples: too short for fft_size {fft_size}")
        lengths.append(n)
        rates.append(fs)
    os.makedirs(args.dumpdir, exist_ok=True)
    written = []

    def save(i, audio, mel, f0):
        written.append(i)
        utt_id = os.path.splitext(os.path.basename(files[i]))[0]
        np.save(os.path.join(args.dumpdir, f"{utt_id}-wave.npy"), audio, allow_pickle=False)
        np.save(os.path.join(args.dumpdir, f"{utt_id}-feats.npy"), mel.cpu().numpy().astype(np.float32), allow_pickle=False)
        if f0 is not None:
            np.save(os.path.join(args.dumpdir, f"{utt_id}-f0.npy"), f0.cpu().numpy().astype(np.float32), allow_pickle=False)

    def flush_conditioned(batch):
        """One batch through the reference's order, the waveform staying on the GPU: (resample the input,)
        trim, (resample a copy for the mel,) mel, fit, f0 on the fitted audio, gain, clipping check."""
        audios = [read_wav(files[i])[0] for i in batch]
        for fs in sorted({rates[i] for i in batch} - {sr}):
            pos = [k for k, i in enumerate(batch) if rates[i] == fs]
            for k, y in zip(pos, conditioner.resample_batch([audios[k] for k in pos], fs, sr)):
                audios[k] = y
        if args.condition_audio and conditioner.trim_silence:
            audios, _ = conditioner.trim_batch(audios)
        feats_in = audios if sr_feats == sr else conditioner.resample_batch(audios, sr, sr_feats)
        for i, x in zip(batch, feats_in):
            if len(x) <= fft_size // 2:
                raise ValueError(f"{files[i]} has {len(x)} samples after conditioning: too short for fft_size {fft_size}")
        mels = extractor.extract_batch(feats_in)
        out_lengths = [len(mel) * hop for mel in mels]
        gain = conditioner.global_gain_scale if args.condition_audio else 1.0
        fitted, peaks = conditioner.fit_batch(audios, out_lengths, gain=gain)
        f0s = [None] * len(batch)
        if f0_extractor is not None:
            plain = fitted if gain == 1.0 else conditioner.fit_batch(audios, out_lengths, gain=1.0)[0]
            f0s = f0_extractor.extract_batch(plain, frames=[len(mel) for mel in mels])
        for i, audio, mel, f0, peak in zip(batch, fitted, mels, f0s, peaks.cpu().numpy()):
            if peak >= 1.0:
                utt_id = os.path.splitext(os.path.basename(files[i]))[0]
                logging.warning(f"{utt_id} causes clipping. it is better to re-consider global gain scale.")
                continue
            save(i, audio.cpu().numpy(), mel, f0)

    def flush(batch):
        """Load, extract and write one batch of file indices; only its samples are in memory."""
        if conditioner is not None:
            return flush_conditioned(batch)
        audios = [read_wav(files[i])[0] for i in batch]
        mels = extractor.extract_batch(audios)
        fitted = [fit_audio(audio, len(mel), fft_size, hop).astype(np.float32) for audio, mel in zip(audios, mels)]
        f0s = [None] * len(batch)
        if f0_extractor is not None:
            f0s = f0_extractor.extract_batch(fitted, frames=[len(mel) for mel in mels])
        for i, audio, mel, f0 in zip(batch, fitted, mels, f0s):
            save(i, audio, mel, f0)

    batch, n = [], 0
    for i, t in enumerate(lengths):
        if batch and n + t > args.batch_samples:
            flush(batch)
            batch, n = [], 0
        batch.append(i)
        n += t
    if batch:
        flush(batch)
    logging.info(f"wrote {len(written)} of {len(files)} utterances to {args.dumpdir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
