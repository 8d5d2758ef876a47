"""Drop-in ``DiscreteSymbolDurationGenerator`` and ``DiscreteSymbolF0Generator``: the token
vocoders of the reference's cvss_c/hubert_voc1 and opencpop/token_voc1 duration and f0 recipes
(parallel_wavegan/models/hifigan.py:1100-1487) on the MI355X engine.

Both keep the body of ``DiscreteSymbolHiFiGANGenerator`` (dsym.py): the conv-network program is what
hifigan.lower_hifigan emits, and only the front end that writes its buffer 0 differs
(include/pwg_embed.h, csrc/pwg_embed_ext.hip).

Duration class: the DurationPredictor (layers/duration_predictor.py) runs as one pwg_durpred_layer
launch per layer straight from the embedding table, the LengthRegulator
(layers/length_regulator.py) as pwg_regulate_scan + pwg_regulate_rows. The body can only be planned
once the regulated frame counts are known on the host: with caller-given host-resident durations
they are, and nothing comes back from the device; with predicted or device-resident durations ONE
copy of the per-utterance totals (8 bytes per utterance) is awaited before the plan is made.
Deviations from the reference: the all-zero -> all-ones rule is applied per utterance also inside
a batch (the reference applies it only when the whole batch sums to zero); ``g`` is ignored by
``inference`` (the reference builds the speaker column and then drops it again without a table).
Refused: ``num_spk_embs > 0`` (the reference class cannot run it: its predictor is built for
in_channels + spk_emb_dim inputs and fed in_channels), duration kernel sizes other than 3, more than
4 layers, channel counts that are no multiple of 16 or above 1024.

F0 class: pwg_embed_rows_f0 writes rows of in_channels + linear_channel floats: the token part
(``emb(ids) [+ spk_emb(g)]``, or the weighted sum over ``layer_num`` tables) and ``f0_embedding``.
Deviation from the reference: with ``use_f0=False`` ``inference`` ignores ``f0`` (the reference
raises AttributeError there, ``self.use_f0`` never being set). Refused: ``use_embedding_feats=True``,
``use_weight_sum`` with a speaker table (the reference crashes on it), ``layer_num > 16``,
``linear_channel`` no multiple of 16.
"""

import types

import numpy as np
import torch

from . import _lib
from .dsym import DiscreteSymbolHiFiGANGenerator, _as_ids
from .engine import fold_weight_norm
from .hifigan import lower_hifigan

MAX_TABLES = 16      # PWG_EMBED_MAX_TABLES (include/pwg_embed.h)
MAX_PREDICTOR_CH = 1024
MAX_PREDICTOR_LAYERS = 4


class DurationPredictor(torch.nn.Module):
    """Parameter holder with the layout of layers/duration_predictor.py:17-70."""

    def __init__(self, idim, n_layers=2, n_chans=384, kernel_size=3, dropout_rate=0.1, offset=1.0):
        super().__init__()
        self.offset = offset
        self.conv = torch.nn.ModuleList()
        for idx in range(n_layers):
            self.conv += [torch.nn.Sequential(
                torch.nn.Conv1d(idim if idx == 0 else n_chans, n_chans, kernel_size, stride=1,
                                padding=(kernel_size - 1) // 2),
                torch.nn.ReLU(),
                torch.nn.LayerNorm(n_chans, eps=1e-12),  # over channels (layers/layer_norm.py)
                torch.nn.Dropout(dropout_rate))]
        self.linear = torch.nn.Linear(n_chans, 1)


def plan_frame_limit(program):
    """The largest sum of frames pwg_cnet_plan_create accepts for ``program`` (every buffer's
    rows x leading dimension stays below 2^31)."""
    nb = len(program.channels)
    lim = []
    for b, (c, r) in enumerate(zip(program.channels, program.rate)):
        ld = c if b == nb - 1 else (c + 15) // 16 * 16
        lim.append((((1 << 31) // max(1, ld)) - 1) // r)
    return min(lim)


def _as_durations(d):
    d = _as_ids(d)
    if d.ndim != 1:
        raise ValueError("durations must be one-dimensional, one per token")
    return d


def _device_cat(parts, dev):
    return torch.cat([t if torch.is_tensor(t) and t.device == dev else torch.as_tensor(t, device=dev)
                      for t in parts])


class DiscreteSymbolDurationGenerator(DiscreteSymbolHiFiGANGenerator):
    """models/hifigan.py:1100-1295, executed on the MI355X conv-network engine."""

    _front_prefixes = ("emb.", "spk_emb.", "duration_predictor.")

    def __init__(self, in_channels=512, out_channels=1, channels=512, num_embs=100, num_spk_embs=128,
                 spk_emb_dim=128, concat_spk_emb=False, duration_layers=2, duration_chans=384,
                 duration_kernel_size=3, duration_offset=1.0, duration_dropout_rate=0.5, kernel_size=7,
                 upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], use_additional_convs=True, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_weight_norm=True):
        if num_spk_embs > 0:
            raise NotImplementedError(
                "DiscreteSymbolDurationGenerator with num_spk_embs > 0 is not supported: the reference class cannot "
                "run it either (its duration predictor is built for in_channels + spk_emb_dim inputs and is fed "
                "in_channels); every recipe sets num_spk_embs: 0")
        if duration_kernel_size != 3:
            raise NotImplementedError(f"duration_kernel_size {duration_kernel_size} is not accelerated (only 3)")
        if not 1 <= duration_layers <= MAX_PREDICTOR_LAYERS:
            raise NotImplementedError(f"duration_layers {duration_layers} is not accelerated (1 to "
                                      f"{MAX_PREDICTOR_LAYERS})")
        for what, ch in (("in_channels", in_channels), ("duration_chans", duration_chans)):
            if ch % 16 or not 16 <= ch <= MAX_PREDICTOR_CH:
                raise NotImplementedError(f"{what} {ch} is not accelerated by the duration predictor kernel (multiples "
                                          f"of 16 up to {MAX_PREDICTOR_CH})")
        super().__init__(in_channels=in_channels, out_channels=out_channels, channels=channels,
                         num_embs=num_embs + 1,  # for padding case (models/hifigan.py:1160)
                         num_spk_embs=num_spk_embs, spk_emb_dim=spk_emb_dim, concat_spk_emb=concat_spk_emb,
                         kernel_size=kernel_size, upsample_scales=upsample_scales,
                         upsample_kernel_sizes=upsample_kernel_sizes, resblock_kernel_sizes=resblock_kernel_sizes,
                         resblock_dilations=resblock_dilations, use_additional_convs=use_additional_convs, bias=bias,
                         nonlinear_activation=nonlinear_activation,
                         nonlinear_activation_params=nonlinear_activation_params, use_weight_norm=use_weight_norm)
        # (created after apply_weight_norm, as in the reference: its keys are plain)
        self.duration_predictor = DurationPredictor(in_channels, n_layers=duration_layers, n_chans=duration_chans,
                                                    kernel_size=duration_kernel_size,
                                                    dropout_rate=duration_dropout_rate, offset=duration_offset)
        self._dp = None  # per layer (w [3][cin][cout], bias, ln weight, ln bias), then (linear w, linear b)
        self._totals_host = None

    # ------------------------------------------------------------------ engine plumbing
    def _load_front(self, dev):
        super()._load_front(dev)
        sd = fold_weight_norm({k: v for k, v in self.state_dict().items() if k.startswith("duration_predictor.")})

        def t(key):
            return torch.from_numpy(np.ascontiguousarray(sd["duration_predictor." + key], np.float32)).to(dev)

        layers = []
        for i in range(len(self.duration_predictor.conv)):
            layers.append((t(f"conv.{i}.0.weight").permute(2, 1, 0).contiguous(), t(f"conv.{i}.0.bias"),
                           t(f"conv.{i}.2.weight"), t(f"conv.{i}.2.bias")))
        self._dp = (layers, t("linear.weight").reshape(-1).contiguous(), t("linear.bias"))

    def _predict(self, ids_d, rs_d, n, tokens, stream):
        """The predictor over the batch's ``tokens`` rows: (log durations fp32, durations int64)."""
        layers, lin_w, lin_b = self._dp
        dev = ids_d.device
        emb = self._tables[0]
        logdur = torch.empty(tokens, dtype=torch.float32, device=dev)
        dur = torch.empty(tokens, dtype=torch.int64, device=dev)
        L = _lib.load()
        x = None
        for i, (w, b, g, beta) in enumerate(layers):
            last = i == len(layers) - 1
            cin, cout = w.shape[1], w.shape[2]
            y = None if last else torch.empty(tokens * cout, dtype=torch.float32, device=dev)
            _lib.check(L.pwg_durpred_layer(
                x.data_ptr() if x is not None else None, emb.data_ptr() if x is None else None,
                self.num_embs if x is None else 0, ids_d.data_ptr() if x is None else None, cin, cout, 3,
                w.data_ptr(), b.data_ptr(), g.data_ptr(), beta.data_ptr(), lin_w.data_ptr() if last else None,
                lin_b.data_ptr() if last else None, float(self.duration_predictor.offset), rs_d.data_ptr(), n, tokens,
                y.data_ptr() if y is not None else None, logdur.data_ptr() if last else None,
                dur.data_ptr() if last else None, self._flag.data_ptr(), stream.cuda_stream))
            x = y
        return logdur, dur

    def _check_frames(self, totals, pad):
        """Per-utterance body frames from the regulated totals; ValueError before anything is
        allocated when one plan cannot hold the batch."""
        frames = [int(t) for t in totals]
        if pad:
            frames = [max(frames)] * len(frames)
        limit = plan_frame_limit(self._engine.program)
        run = 0
        for u, f in enumerate(frames):
            run += f
            if run > limit:
                raise ValueError(f"utterance {u} brings the batch to {run} regulated frames, more than one plan of "
                                 f"this generator can hold ({limit}); decode fewer utterances per call")
        return frames

    def _tokens_to_device(self, toks, extra_host=()):
        """One upload of row_start, ``extra_host`` int64 arrays and the host-resident token ids.
        Returns (engine, device, row_start tensor, ids tensor, [extra tensors])."""
        self._check_host(toks, None)  # before any GPU use
        eng = self.engine()
        dev = eng.device
        counts = [int(t.shape[0]) for t in toks]
        if min(counts) < 1:
            raise ValueError("every utterance needs at least one frame")
        n = len(counts)
        host = [np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)] + [np.asarray(e, np.int64) for e in extra_host]
        host_tok = all(isinstance(t, np.ndarray) for t in toks)
        if host_tok:
            host += toks
        up = self._upload(np.concatenate(host), dev)
        rs_d, o = up[:n + 1], n + 1
        extra = []
        for e in extra_host:
            extra.append(up[o:o + len(e)])
            o += len(e)
        ids_d = up[o:] if host_tok else _device_cat(toks, dev)
        return eng, dev, rs_d, ids_d, extra, counts

    def _run_regulated(self, toks, ds, pad=False, want_log=False):
        """toks / ds: per utterance a 1-D int64 ndarray (host) or long tensor (device); ds None:
        predicted. pad: every utterance gets the longest one's frames, the surplus rows being zeros
        (pad_list). Returns (engine outputs, log durations tensor or None)."""
        n = len(toks)
        host_ds = ds is not None and all(isinstance(d, np.ndarray) for d in ds)
        if ds is not None:
            for u, (t, d) in enumerate(zip(toks, ds)):
                if int(d.shape[0]) != int(t.shape[0]):
                    raise ValueError(f"utterance {u}: {int(d.shape[0])} durations for {int(t.shape[0])} tokens")
                if isinstance(d, np.ndarray) and d.size and (d.min() < 0 or d.max() >= 1 << 31):
                    raise ValueError(f"utterance {u}: a duration outside [0, 2^31)")
        extra, frames = [], None
        if host_ds:
            self._check_host(toks, None)  # before any GPU use
            self.engine()  # (the plan limit comes from its program)
            frames = self._check_frames([int(d.sum()) or len(d) for d in ds], pad)
            extra = [np.concatenate([[0], np.cumsum(frames)]), np.concatenate(ds)]
        eng, dev, rs_d, ids_d, extra_d, counts = self._tokens_to_device(toks, extra)
        tokens, dim = sum(counts), self.in_channels
        L = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            logdur = None
            if ds is None or want_log:
                logdur, dur = self._predict(ids_d, rs_d, n, tokens, stream)
            if host_ds:
                os_d, ds_d = extra_d
            else:
                ds_d = dur if ds is None else _device_cat(ds, dev)
            prefix = torch.empty(tokens, dtype=torch.int64, device=dev)
            totals = torch.empty(n, dtype=torch.int64, device=dev)
            _lib.check(L.pwg_regulate_scan(ds_d.data_ptr(), rs_d.data_ptr(), n, tokens, prefix.data_ptr(),
                                           totals.data_ptr(), self._flag.data_ptr(), stream.cuda_stream))
            if not host_ds:
                # the one device -> host copy of this path: the body cannot be planned before the
                # regulated frame counts are known (8 bytes per utterance, awaited here)
                if self._totals_host is None or self._totals_host.numel() < n:
                    self._totals_host = torch.empty(max(64, 2 * n), dtype=torch.int64).pin_memory()
                self._totals_host[:n].copy_(totals, non_blocking=True)
                stream.synchronize()
                self._stage_busy = False
                frames = self._check_frames(self._totals_host[:n].tolist(), pad)
                os_d = self._upload(np.concatenate([[0], np.cumsum(frames)]).astype(np.int64), dev)
            out_rows = sum(frames)
            feats = torch.empty(out_rows * dim, dtype=torch.float32, device=dev)
            _lib.check(L.pwg_regulate_rows(self._tables[0].data_ptr(), self.num_embs, dim, ids_d.data_ptr(),
                                           prefix.data_ptr(), totals.data_ptr(), rs_d.data_ptr(), os_d.data_ptr(), n,
                                           tokens, out_rows, feats.data_ptr(), self._flag.data_ptr(),
                                           stream.cuda_stream))
            self._flag_fetch(stream)
            outs = eng.infer_rows(frames, feats)
            self._flag_raise()
        return outs, logdur, counts

    # ------------------------------------------------------------------ reference API
    def _split_ids(self, cs):
        toks = []
        for c in cs:
            ids = _as_ids(c)
            if ids.ndim != 2:
                raise ValueError("c must be (T, 1)")
            if ids.shape[0] < 1:
                raise ValueError("every utterance needs at least one frame")
            toks.append(ids[:, 0])  # (without a speaker table the reference keeps column 0 only)
        return toks

    def predict_durations(self, cs):
        """``duration_predictor.inference`` over a ragged list of (T, 1) id arrays: one int64 device
        tensor of T durations per utterance (what ``inference`` regulates with when ``ds`` is None).
        Waits for the launches (the id check of device-resident ids is read back)."""
        toks = self._split_ids(cs)
        eng, dev, rs_d, ids_d, _, counts = self._tokens_to_device(toks)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _, dur = self._predict(ids_d, rs_d, len(toks), sum(counts), stream)
            self._flag_fetch(stream)
            self._flag_raise()
        return list(torch.split(dur, counts))

    def forward(self, c, ds):
        """models/hifigan.py:1190-1229: c (B, 1, T) ids, ds (B, T) durations -> (y (B, out_channels,
        max_b sum(ds[b]) * hop), log durations (B, T)); utterances with a smaller total are padded
        with zero feature rows, as the reference's pad_list does."""
        if not torch.is_tensor(c):
            c = torch.as_tensor(np.asarray(c))
        if c.dim() != 3:
            raise ValueError("forward expects c (B, 1, T)")
        assert c.size(1) == 1
        ids, d = _as_ids(c), _as_ids(ds)
        if d.ndim != 2 or d.shape[0] != ids.shape[0]:
            raise ValueError("forward expects ds (B, T)")
        B = ids.shape[0]
        outs, logdur, _ = self._run_regulated([ids[b, 0] for b in range(B)], [d[b] for b in range(B)], pad=True,
                                              want_log=True)
        return torch.stack([o.transpose(0, 1) for o in outs], 0), logdur.view(B, -1)

    def inference(self, c, g=None, ds=None, normalize_before=False):
        """models/hifigan.py:1231-1254: c (T, 1) -> (sum(ds) * hop, out_channels); ``ds`` None:
        predicted durations. ``g`` is ignored (no speaker table)."""
        return self.inference_batch([c], None if ds is None else [ds], normalize_before)[0]

    def inference_batch(self, cs, ds=None, normalize_before=False):
        """Ragged list form of ``inference``: ``ds`` is None (predicted) or one duration vector per
        utterance (then the predictor is skipped)."""
        assert not normalize_before, "No statistics are used."
        toks = self._split_ids(cs)
        if ds is not None:
            if len(ds) != len(toks):
                raise ValueError("ds needs one duration vector per utterance")
            ds = [_as_durations(d) for d in ds]
        return self._run_regulated(toks, ds)[0]


class DiscreteSymbolF0Generator(DiscreteSymbolHiFiGANGenerator):
    """models/hifigan.py:1298-1487, executed on the MI355X conv-network engine."""

    _front_prefixes = ("emb.", "spk_emb.", "f0_embedding.", "weights")

    def __init__(self, in_channels=512, out_channels=1, channels=512, linear_channel=256, num_embs=100,
                 num_spk_embs=128, spk_emb_dim=128, concat_spk_emb=False, kernel_size=7, upsample_scales=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], use_additional_convs=True, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_weight_norm=True, use_embedding_feats=False, use_weight_sum=False, layer_num=12,
                 use_fix_weight=False, use_f0=True):
        if use_embedding_feats:
            raise NotImplementedError("use_embedding_feats=True is not accelerated in DiscreteSymbolF0Generator")
        if use_weight_sum and num_spk_embs > 0:
            raise NotImplementedError("use_weight_sum with a speaker table is not supported (the reference's forward "
                                      "crashes on it: emb is then a ModuleList)")
        if use_weight_sum and not 1 <= layer_num <= MAX_TABLES:
            raise NotImplementedError(f"layer_num {layer_num} is not accelerated (1 to {MAX_TABLES} tables)")
        if use_f0 and (linear_channel % 16 or linear_channel < 16):
            raise NotImplementedError(f"linear_channel {linear_channel} is not accelerated (multiples of 16)")
        super().__init__(in_channels=in_channels, out_channels=out_channels, channels=channels, num_embs=num_embs,
                         num_spk_embs=num_spk_embs, spk_emb_dim=spk_emb_dim, concat_spk_emb=concat_spk_emb,
                         kernel_size=kernel_size, upsample_scales=upsample_scales,
                         upsample_kernel_sizes=upsample_kernel_sizes, resblock_kernel_sizes=resblock_kernel_sizes,
                         resblock_dilations=resblock_dilations, use_additional_convs=use_additional_convs, bias=bias,
                         nonlinear_activation=nonlinear_activation,
                         nonlinear_activation_params=nonlinear_activation_params, use_weight_norm=use_weight_norm)
        # the assignments below follow models/hifigan.py:1371-1401 one for one: the state dict's key
        # order depends on them
        self.use_f0 = use_f0 is True
        self.linear_channel = int(linear_channel) if self.use_f0 else 0
        if self.use_f0:
            self.f0_embedding = torch.nn.Linear(in_features=1, out_features=linear_channel)
        self.use_weight_sum = use_weight_sum is True
        if self.use_weight_sum:
            self.layer_num = layer_num
            self.use_fix_weight = use_fix_weight
            self.weights = torch.nn.Parameter(torch.ones(self.layer_num), requires_grad=use_fix_weight is not True)
            self.emb = torch.nn.ModuleList([torch.nn.Embedding(num_embeddings=num_embs, embedding_dim=in_channels)
                                            for _ in range(self.layer_num)])
        # rebuilt after weight norm: plain input_conv.weight / input_conv.bias
        self.input_conv = torch.nn.Conv1d(in_channels + self.linear_channel, channels, kernel_size, 1,
                                          padding=(kernel_size - 1) // 2)
        self.use_embedding_feats = False
        self._f0 = None  # (table weights or None, f0_embedding weight, bias) on the device

    # ------------------------------------------------------------------ lowering / engine plumbing
    def program(self):
        """The HiFiGAN body program; buffer 0 is in_channels + linear_channel wide."""
        return lower_hifigan(types.SimpleNamespace(
            in_channels=self.in_channels + self.linear_channel, out_channels=self.out_channels,
            input_conv=self.input_conv, num_upsamples=self.num_upsamples, upsamples=self.upsamples,
            num_blocks=self.num_blocks, blocks=self.blocks, output_conv=self.output_conv))

    def _load_front(self, dev):
        def f32(t):
            return t.detach().to(dev, torch.float32).contiguous()

        tw = None
        if self.use_weight_sum:
            emb = torch.stack([f32(e.weight) for e in self.emb]).contiguous()  # (L, num_embs, dim), back to back
            w = self.weights.detach().float()
            tw = f32(w if self.use_fix_weight else torch.nn.functional.softmax(w, dim=-1))
            spk = None
        else:
            emb = f32(self.emb.weight)
            spk = f32(self.spk_emb.weight) if self.num_spk_embs > 0 else None
        self._tables = (emb, spk)
        self._f0 = (tw, f32(self.f0_embedding.weight).reshape(-1), f32(self.f0_embedding.bias)) if self.use_f0 \
            else (tw, None, None)

    def _want_columns(self):
        return self.layer_num if self.use_weight_sum else super()._want_columns()

    def _check_host(self, toks, spks):
        for u, t in enumerate(toks):
            if isinstance(t, np.ndarray):
                bad = np.argwhere((t < 0) | (t >= self.num_embs))
                if bad.size:
                    raise IndexError(f"token id {int(t[tuple(bad[0])])} at frame {int(bad[0][0])} of utterance {u} is "
                                     f"out of range [0, {self.num_embs})")
        super()._check_host((), spks)

    def _run_f0(self, toks, spks, f0s):
        """toks: per utterance int64 ids, (T,) or with use_weight_sum (T, layer_num), ndarray or
        device tensor; spks as in the parent; f0s: per utterance (T,) float32 ndarray or device
        tensor, or None without use_f0."""
        if not self.use_f0 and not self.use_weight_sum:
            return self._run_tokens(toks, spks)
        self._check_host(toks, spks)  # before any GPU use
        frames = [int(t.shape[0]) for t in toks]
        if min(frames) < 1:
            raise ValueError("every utterance needs at least one frame")
        if self.use_f0:
            if f0s is None or len(f0s) != len(toks):
                raise ValueError("use_f0 is set: f0 is required, one vector per utterance")
            for u, (f, T) in enumerate(zip(f0s, frames)):
                if f.ndim != 1 or int(f.shape[0]) != T:
                    raise ValueError(f"utterance {u}: f0 of shape {tuple(f.shape)} for {T} frames (one value per "
                                     f"frame is needed)")
        eng = self.engine()
        dev = eng.device
        emb, spk = self._tables
        tw, lin_w, lin_b = self._f0
        n, rows, dim, lin = len(frames), sum(frames), self.in_channels, self.linear_channel
        host = [np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)]
        host_spk = spk is not None and not any(torch.is_tensor(g) for g in spks)
        if host_spk:
            host.append(np.asarray(spks, np.int64))
        host_tok = all(isinstance(t, np.ndarray) for t in toks)
        n_ids = rows * (self.layer_num if self.use_weight_sum else 1)
        if host_tok:
            host += [t.reshape(-1) for t in toks]
        host_f0 = self.use_f0 and all(isinstance(f, np.ndarray) for f in f0s)
        if host_f0:  # fp32 values ride in the int64 staging buffer, two to a word
            f = np.concatenate(f0s + [np.zeros(rows % 2, np.float32)]).astype(np.float32)
            host.append(f.view(np.int64))
        up = self._upload(np.concatenate(host), dev)  # one upload of everything host-resident
        rs_d, o = up[:n + 1], n + 1
        spk_d = None
        if host_spk:
            spk_d, o = up[o:o + n], o + n
        elif spk is not None:
            spk_d = torch.stack([g if torch.is_tensor(g) and g.device == dev and g.dim() == 0 else
                                 torch.as_tensor(g, device=dev).reshape(()) for g in spks])
        if host_tok:
            ids_d, o = up[o:o + n_ids], o + n_ids
        else:
            ids_d = _device_cat([t.reshape(-1) for t in toks], dev)
        f0_d = None
        if host_f0:
            f0_d = up[o:].view(torch.float32)
        elif self.use_f0:
            f0_d = _device_cat(f0s, dev).to(torch.float32).contiguous()
        feats = torch.empty(rows * (dim + lin), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _lib.check(_lib.load().pwg_embed_rows_f0(
                emb.data_ptr(), self.num_embs, self.layer_num if tw is not None else 1,
                tw.data_ptr() if tw is not None else None, spk.data_ptr() if spk is not None else None,
                self.num_spk_embs if spk is not None else 0, dim, lin, f0_d.data_ptr() if f0_d is not None else None,
                lin_w.data_ptr() if lin_w is not None else None, lin_b.data_ptr() if lin_b is not None else None,
                ids_d.data_ptr(), spk_d.data_ptr() if spk_d is not None else None, rs_d.data_ptr(), n, rows,
                feats.data_ptr(), self._flag.data_ptr(), stream.cuda_stream))
            self._flag_fetch(stream)
            outs = eng.infer_rows(frames, feats)
            self._flag_raise()
        return outs

    # ------------------------------------------------------------------ reference API
    @staticmethod
    def _as_f0(f):
        """(T,) float32: an ndarray for host-resident input, a tensor for a device tensor."""
        if torch.is_tensor(f):
            if f.device.type == "cpu":
                return np.ascontiguousarray(f.detach().numpy(), np.float32)
            return f.detach()
        return np.ascontiguousarray(np.asarray(f), np.float32)

    def forward(self, c, f0=None):
        """models/hifigan.py:1404-1463: c (B, 2, T), (B, 1, T) or with use_weight_sum (B, L, T) ids,
        f0 (B, 1, T) -> (B, out_channels, T * hop). With use_f0, f0 is required."""
        if not self.use_f0 and not self.use_weight_sum:
            return super().forward(c)
        if not torch.is_tensor(c):
            c = torch.as_tensor(np.asarray(c))
        if c.dim() != 3:
            raise ValueError("forward expects c (B, 2, T), (B, 1, T) or (B, L, T)")
        assert c.size(1) == self._want_columns()
        ids = _as_ids(c)
        B = ids.shape[0]
        f0s = None
        if self.use_f0:
            if f0 is None:
                raise ValueError("use_f0 is set: f0 (B, 1, T) is required")
            f = self._as_f0(f0)
            if f.ndim != 3 or f.shape[0] != B or f.shape[1] != 1:
                raise ValueError("forward expects f0 (B, 1, T)")
            f0s = [f[b, 0] for b in range(B)]
        spks = None
        if self.use_weight_sum:
            toks = [ids[b].T if isinstance(ids, np.ndarray) else ids[b].transpose(0, 1) for b in range(B)]
        else:
            toks = [ids[b, 0] for b in range(B)]
            if self.num_spk_embs > 0:
                spks = [ids[b, 1, 0] if torch.is_tensor(ids) else int(ids[b, 1, 0]) for b in range(B)]
        return torch.stack([o.transpose(0, 1) for o in self._run_f0(toks, spks, f0s)], 0)

    def inference(self, c, f0=None, g=None, normalize_before=False):
        """models/hifigan.py:1466-1487: c (T, 2), (T, 1) or (T, L) ids, f0 (T,) -> (T * hop,
        out_channels). Without use_f0, ``f0`` is ignored."""
        return self.inference_batch([c], None if f0 is None else [f0], g, normalize_before)[0]

    def inference_batch(self, cs, f0s=None, g=None, normalize_before=False):
        """Ragged list form of ``inference``: one f0 vector per utterance; ``g`` as in the parent."""
        assert not normalize_before, "No statistics are used."
        n = len(cs)
        if g is not None:
            assert self.num_spk_embs > 0
            if torch.is_tensor(g) and g.dim() == 0 or np.ndim(g) == 0:
                g = [g] * n
            if len(g) != n:
                raise ValueError("g needs one speaker id per utterance")
        if self.use_f0:
            if f0s is None or len(f0s) != n:
                raise ValueError("use_f0 is set: f0 is required, one vector per utterance")
            f0s = [self._as_f0(f) for f in f0s]
        else:
            f0s = None
        toks, spks = [], ([] if self.num_spk_embs > 0 else None)
        for u, c in enumerate(cs):
            ids = _as_ids(c)
            if ids.ndim != 2:
                raise ValueError("c must be (T, 2), (T, 1) or (T, L)")
            if g is None:
                assert ids.shape[1] == self._want_columns()
            if ids.shape[0] < 1:
                raise ValueError("every utterance needs at least one frame")
            toks.append(ids if self.use_weight_sum else ids[:, 0])
            if spks is not None:
                s = ids[0, 1] if g is None else g[u]
                spks.append(s.long() if torch.is_tensor(s) and s.device.type != "cpu" else int(s))
        return self._run_f0(toks, spks, f0s)
