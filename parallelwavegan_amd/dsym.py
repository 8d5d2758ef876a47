"""Drop-in ``DiscreteSymbolHiFiGANGenerator``: the token vocoder of the reference's hubert_voc1 /
token_voc1 recipes (parallel_wavegan/models/hifigan.py:867-1097) on the MI355X engine.

The body is a HiFiGAN v1 generator and runs as the same conv-network program as HiFiGANGenerator
(hifigan.lower_hifigan). The front end (models/hifigan.py:1008-1024) is ``emb(ids)`` plus, with a
speaker table, ``spk_emb(g)`` added to every frame of the utterance; here it is one launch of
pwg_embed_rows (include/pwg_embed.h) over the whole ragged batch, which writes the rows the program
reads as buffer 0. Same constructor arguments, defaults and state-dict keys as the reference class
(emb.weight, spk_emb.weight, input_conv.*, upsamples.*, blocks.*, output_conv.*).

Out-of-range ids (torch.nn.Embedding raises IndexError): host-resident inputs are checked before
upload; for device inputs the kernel never reads the table with such an id, writes the row as zeros
and sets a flag that is looked at after the forward's own status synchronisation.

Refused (NotImplementedError): concat_spk_emb=True, upsample kernel sizes other than twice the
scale, odd upsample scales.
"""

import numpy as np
import torch

from . import _lib, cnet
from .engine import WeightTracker, first_parameter
from .hifigan import HiFiGANGenerator, HiFiGANResidualBlock

BAD_TOKEN, BAD_SPEAKER, BAD_DURATION = 1, 2, 4  # include/pwg_embed.h


def _as_ids(x):
    """``x.long()`` of the reference (floats truncated): an int64 ndarray for host-resident input,
    a long tensor for a device tensor."""
    if torch.is_tensor(x):
        if x.device.type == "cpu":
            return x.detach().long().numpy()
        return x if x.dtype == torch.int64 and not x.requires_grad else x.detach().long()
    x = np.asarray(x)
    if x.dtype.kind == "f":
        x = np.trunc(x)
    return x.astype(np.int64)


class DiscreteSymbolHiFiGANGenerator(HiFiGANGenerator):
    """models/hifigan.py:867-1097, executed on the MI355X conv-network engine."""

    def __init__(self, in_channels=512, out_channels=1, channels=512, num_embs=100, num_spk_embs=128,
                 spk_emb_dim=128, concat_spk_emb=False, kernel_size=7, upsample_scales=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], use_additional_convs=True, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_weight_norm=True, use_embedding_feats=False):
        torch.nn.Module.__init__(self)
        self.num_embs = int(num_embs)
        self.num_spk_embs = int(num_spk_embs)
        self.use_embedding_feats = bool(use_embedding_feats)
        self.emb = torch.nn.Embedding(num_embeddings=num_embs, embedding_dim=in_channels)
        if self.num_spk_embs > 0:
            if concat_spk_emb:
                raise NotImplementedError("concat_spk_emb=True is not accelerated (the reference concatenates "
                                          "the speaker embedding along time; no recipe sets it)")
            self.spk_emb = torch.nn.Embedding(num_embeddings=num_spk_embs, embedding_dim=spk_emb_dim)
            self.concat_spk_emb = False
            assert in_channels == spk_emb_dim
        assert kernel_size % 2 == 1, "Kernal size must be odd number."
        assert len(upsample_scales) == len(upsample_kernel_sizes)
        assert len(resblock_dilations) == len(resblock_kernel_sizes)
        for s, k in zip(upsample_scales, upsample_kernel_sizes):
            if k != 2 * s:
                raise NotImplementedError(f"upsample kernel size {k} is not twice its scale {s}")
            if s % 2:
                raise NotImplementedError(f"odd upsample scale {s}: the reference's ConvTranspose1d then yields "
                                          f"T * {s} + 1 samples, which the executor's integer rates cannot express")
        self.num_upsamples = len(upsample_kernel_sizes)
        self.num_blocks = len(resblock_kernel_sizes)
        self.use_causal_conv = False
        self.in_channels, self.out_channels = in_channels, out_channels
        self.upsample_factor = int(np.prod(upsample_scales))
        act = getattr(torch.nn, nonlinear_activation)
        # (the reference passes ``bias`` to the residual blocks only: models/hifigan.py:940-987)
        self.input_conv = torch.nn.Conv1d(in_channels, channels, kernel_size, 1, padding=(kernel_size - 1) // 2)
        self.upsamples = torch.nn.ModuleList()
        self.blocks = torch.nn.ModuleList()
        for i in range(len(upsample_kernel_sizes)):
            k, s = upsample_kernel_sizes[i], upsample_scales[i]
            cout = channels // (2 ** (i + 1))
            self.upsamples += [torch.nn.Sequential(
                act(**nonlinear_activation_params),
                torch.nn.ConvTranspose1d(channels // (2 ** i), cout, k, s, padding=(k - s) // 2))]
            for j in range(len(resblock_kernel_sizes)):
                self.blocks += [HiFiGANResidualBlock(resblock_kernel_sizes[j], cout, resblock_dilations[j], bias,
                                                     use_additional_convs, nonlinear_activation,
                                                     nonlinear_activation_params)]
        self.output_conv = torch.nn.Sequential(
            torch.nn.LeakyReLU(),  # slope 0.01, as the reference (models/hifigan.py:976-988)
            torch.nn.Conv1d(channels // (2 ** (i + 1)), out_channels, kernel_size, 1, padding=(kernel_size - 1) // 2),
            torch.nn.Tanh(),
        )
        if use_weight_norm:
            self.apply_weight_norm()
        self.reset_parameters()
        self._engine = None
        self._weights = WeightTracker()
        self._sig = None
        self._tables = None  # (emb, spk_emb or None): fp32 device tensors, refreshed with the packed image
        self._flag = self._flag_host = self._flag_event = None
        self._stage = self._stage_np = None  # pinned staging of the per-call index upload
        self._stage_busy = False

    @property
    def feature_input(self):
        """models/hifigan.py:1021-1024: without a speaker table and with use_embedding_feats, ``c``
        already holds the in_channels features."""
        return self.num_spk_embs <= 0 and self.use_embedding_feats

    # ------------------------------------------------------------------ engine plumbing
    _front_prefixes = ("emb.", "spk_emb.")  # state-dict keys of the front end: not part of the body program

    def _load_front(self, dev):
        """The front end's fp32 device tensors, refreshed whenever the body's packed image is."""
        spk = self.spk_emb.weight.detach().to(dev, torch.float32).contiguous() if self.num_spk_embs > 0 else None
        self._tables = (self.emb.weight.detach().to(dev, torch.float32).contiguous(), spk)

    def _device(self):
        dev = first_parameter(self).device
        if dev.type != "cuda":
            raise RuntimeError("parallelwavegan_amd.DiscreteSymbolHiFiGANGenerator runs on a ROCm GPU only; move the "
                               "module with .to('cuda') (there is no CPU fallback)")
        return dev

    def engine(self):
        dev = self._device()
        if self._engine is None or self._engine.device != dev:
            self._engine = cnet.CnetEngine(self.program(), dev)
            self._weights.invalidate()
        if self._weights.changed(self):
            with torch.no_grad():
                state = {k: v for k, v in self.state_dict().items() if not k.startswith(self._front_prefixes)}
                self._engine.load_state_dict(state)
                self._load_front(dev)
            if self._flag is None or self._flag.device != dev:
                self._flag = torch.zeros(1, dtype=torch.int32, device=dev)
                self._flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
                self._flag_event = torch.cuda.Event()
                self._stage = self._stage_np = None
            self._weights.mark_packed()
        return self._engine

    # ------------------------------------------------------------------ token front end
    def _check_host(self, toks, spks):
        for u, t in enumerate(toks):
            if isinstance(t, np.ndarray):
                bad = np.flatnonzero((t < 0) | (t >= self.num_embs))
                if bad.size:
                    raise IndexError(f"token id {int(t[bad[0]])} at frame {int(bad[0])} of utterance {u} is out of "
                                     f"range [0, {self.num_embs})")
        for u, g in enumerate(spks or ()):
            if not torch.is_tensor(g) and not 0 <= g < self.num_spk_embs:
                raise IndexError(f"speaker id {g} of utterance {u} is out of range [0, {self.num_spk_embs})")

    def _upload(self, arr, dev):
        """int64 ndarray -> device tensor through a pinned staging buffer kept on the module, as an
        asynchronous copy on the current stream (a pageable copy blocks the host). The buffer is
        free again once the call's flag event, recorded behind the copy, has completed."""
        n = int(arr.size)
        if self._stage_busy:  # a call that raised between its upload and its event
            torch.cuda.current_stream(dev).synchronize()
        if self._stage is None or self._stage.numel() < n:
            self._stage = torch.empty(max(2 * n, 4096), dtype=torch.int64).pin_memory()
            self._stage_np = self._stage.numpy()
        self._stage_np[:n] = arr
        self._stage_busy = True
        return self._stage[:n].to(dev, non_blocking=True)

    def _run_tokens(self, toks, spks):
        """toks: per utterance a 1-D int64 ndarray (host) or long tensor (device); spks: per
        utterance an int (host) or a 0-dim long device tensor, or None without a speaker table.
        Returns the engine's per-utterance outputs (T * hop, out_channels)."""
        self._check_host(toks, spks)  # before any GPU use
        eng = self.engine()
        dev = eng.device
        emb, spk = self._tables
        frames = [int(t.shape[0]) for t in toks]
        if min(frames) < 1:
            raise ValueError("every utterance needs at least one frame")
        n, rows, dim = len(frames), sum(frames), self.in_channels
        row_start = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
        host = [row_start]
        host_spk = spk is not None and not any(torch.is_tensor(g) for g in spks)
        if host_spk:
            host.append(np.asarray(spks, np.int64))
        host_tok = all(isinstance(t, np.ndarray) for t in toks)
        if host_tok:
            host += toks
        up = self._upload(np.concatenate(host), dev)  # one upload of everything host-resident
        rs_d, o = up[:n + 1], n + 1
        spk_d = None
        if host_spk:
            spk_d, o = up[o:o + n], o + n
        elif spk is not None:
            spk_d = torch.stack([g if torch.is_tensor(g) and g.device == dev and g.dim() == 0 else
                                 torch.as_tensor(g, device=dev).reshape(()) for g in spks])
        if host_tok:
            ids_d = up[o:]
        else:
            ids_d = torch.cat([t if torch.is_tensor(t) and t.device == dev else torch.as_tensor(t, device=dev)
                               for t in toks])
        feats = torch.empty(rows * dim, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _lib.check(_lib.load().pwg_embed_rows(
                emb.data_ptr(), self.num_embs, spk.data_ptr() if spk is not None else None,
                self.num_spk_embs if spk is not None else 0, dim, ids_d.data_ptr(),
                spk_d.data_ptr() if spk_d is not None else None, rs_d.data_ptr(), n, rows, feats.data_ptr(),
                self._flag.data_ptr(), stream.cuda_stream))
            self._flag_fetch(stream)
            outs = eng.infer_rows(frames, feats)
            self._flag_raise()
        return outs

    def _flag_fetch(self, stream):
        """The flag travels to pinned memory on the same stream, ahead of the forward: by the time
        CnetEngine.run(check=True) has synchronised for its range status the copy has landed, and
        the success path pays no synchronisation of its own."""
        self._flag_host.copy_(self._flag, non_blocking=True)
        self._flag_event.record(stream)

    def _flag_raise(self):
        if not self._flag_event.query():  # (exact-fp32 mode: run() has no status to wait for)
            self._flag_event.synchronize()
        self._stage_busy = False
        bits = int(self._flag_host[0])
        if bits:
            self._flag.zero_()
            what = [w for b, w in ((BAD_TOKEN, f"a token id outside [0, {self.num_embs})"),
                                   (BAD_SPEAKER, f"a speaker id outside [0, {self.num_spk_embs})"),
                                   (BAD_DURATION, "a duration outside [0, 2^31)")) if bits & b]
            # (ids are IndexError as in torch.nn.Embedding; a bad duration alone is a ValueError)
            raise (IndexError if bits & (BAD_TOKEN | BAD_SPEAKER) else ValueError)("the batch holds " + " and ".join(what))

    def _want_columns(self):
        return 2 if self.num_spk_embs > 0 else 1

    # ------------------------------------------------------------------ reference API
    def forward(self, c):
        """models/hifigan.py:997-1035: c (B, 2, T) ids and speaker ids (the speaker of utterance b is
        c[b, 1, 0]), (B, 1, T) ids without a speaker table, or (B, in_channels, T) features with
        use_embedding_feats -> (B, out_channels, T * hop). Float ids are truncated (``.long()``)."""
        if self.feature_input:
            return HiFiGANGenerator.forward(self, c)
        if not torch.is_tensor(c):
            c = torch.as_tensor(np.asarray(c))
        if c.dim() != 3:
            raise ValueError("forward expects c (B, 2, T) or (B, 1, T)")
        assert c.size(1) == self._want_columns()
        ids = _as_ids(c)
        toks = [ids[b, 0] for b in range(ids.shape[0])]
        spks = None
        if self.num_spk_embs > 0:
            spks = [ids[b, 1, 0] if torch.is_tensor(ids) else int(ids[b, 1, 0]) for b in range(ids.shape[0])]
        return torch.stack([o.transpose(0, 1) for o in self._run_tokens(toks, spks)], 0)

    def inference(self, c, g=None, normalize_before=False):
        """models/hifigan.py:1076-1097: c (T, 2) or (T, 1) -> (T * hop, out_channels); ``g``
        overrides the speaker column."""
        return self.inference_batch([c], g, normalize_before)[0]

    def inference_batch(self, cs, g=None, normalize_before=False):
        """Ragged list form of ``inference`` (what bin/decode.py calls): ``g`` is None, one speaker
        id for every utterance, or one per utterance."""
        assert not normalize_before, "No statistics are used."
        if self.feature_input:
            return HiFiGANGenerator.inference_batch(self, cs, False)
        n = len(cs)
        if g is not None:
            assert self.num_spk_embs > 0  # (the reference builds (T, 2) and then asserts one column)
            if torch.is_tensor(g) and g.dim() == 0 or np.ndim(g) == 0:
                g = [g] * n
            if len(g) != n:
                raise ValueError("g needs one speaker id per utterance")
        toks, spks = [], ([] if self.num_spk_embs > 0 else None)
        for u, c in enumerate(cs):
            ids = _as_ids(c)
            if ids.ndim != 2:
                raise ValueError("c must be (T, 2) or (T, 1)")
            if g is None:
                assert ids.shape[1] == self._want_columns()
            if ids.shape[0] < 1:
                raise ValueError("every utterance needs at least one frame")
            toks.append(ids[:, 0])
            if spks is not None:
                s = ids[0, 1] if g is None else g[u]
                spks.append(s.long() if torch.is_tensor(s) and s.device.type != "cpu" else int(s))
        return self._run_tokens(toks, spks)
