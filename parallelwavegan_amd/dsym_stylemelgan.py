"""Drop-in ``DiscreteSymbolStyleMelGANGenerator``: the token vocoder of the reference's
egs/vctk/hubert_voc1/conf/style_melgan_hubert.v1.yaml (parallel_wavegan/models/style_melgan.py:364-602)
on the MI355X TADE kernels (include/pwg_smg.h).

Same constructor arguments, defaults, submodule names and state-dict keys as the reference class
(emb.weight, spk_emb.weight, then StyleMelGANGenerator's keys), so a reference checkpoint loads with
``strict=True``. The holders, the handle and the weight tracking are stylemelgan.py's. Two things differ
from StyleMelGANGenerator and are what pwg_smg_plan_create_ex / pwg_smg_run_tokens add:
  * the aux input is c = emb[ids] + spk_emb[g], the speaker read from the utterance's first frame
    (style_melgan.py:497-505). The first aux conv gathers it while it stages its input: no buffer of c and
    no embedding launch;
  * ``inference`` cuts the upsampled noise to the T frames (style_melgan.py:596-597) instead of padding c up
    to it: every tensor has exactly T rows per utterance, and so has every instance-norm statistic.

Out-of-range ids (torch.nn.Embedding raises IndexError): host-resident ids are checked before upload (a
ValueError naming the kind); ids already on the device are checked by the kernel, which never forms an
address from a bad one, stages zeros instead and sets a flag that ``pwg_smg_run_status`` turns into the same
ValueError. The module stays usable afterwards.

Refused: concat_spk_emb=True (NotImplementedError: the reference itself cannot run it, it concatenates the
speaker embedding along time and the first aux conv then fails on its channel count), everything
StyleMelGANGenerator refuses (same texts), a one-frame utterance (ValueError: InstanceNorm1d over one
element raises in the reference), normalize_before=True (AssertionError, as the reference).
"""

import numpy as np
import torch

from . import _lib
from .dsym import _as_ids
from .stylemelgan import StyleMelGANGenerator


class DiscreteSymbolStyleMelGANGenerator(StyleMelGANGenerator):
    """models/style_melgan.py:364-602, executed on the MI355X TADE kernels."""

    def __init__(self, in_channels=128, aux_channels=128, channels=64, out_channels=1, num_embs=100, num_spk_embs=128,
                 spk_emb_dim=128, concat_spk_emb=False, kernel_size=9, dilation=2, bias=True,
                 noise_upsample_scales=[11, 2, 2, 2], noise_upsample_activation="LeakyReLU",
                 noise_upsample_activation_params={"negative_slope": 0.2},
                 upsample_scales=[2, 2, 2, 2, 2, 2, 2, 2, 1], upsample_mode="nearest", gated_function="softmax",
                 use_weight_norm=True):
        if concat_spk_emb:
            raise NotImplementedError("concat_spk_emb=True is not accelerated: the reference itself cannot run it (it "
                                      "concatenates the speaker embedding along time, and the first aux conv then "
                                      "fails on its channel count)")
        assert aux_channels == spk_emb_dim
        super().__init__(in_channels, aux_channels, channels, out_channels, kernel_size, dilation, bias,
                         noise_upsample_scales, noise_upsample_activation, noise_upsample_activation_params,
                         upsample_scales, upsample_mode, gated_function, use_weight_norm)
        self.num_embs, self.num_spk_embs = int(num_embs), int(num_spk_embs)
        self.concat_spk_emb = False
        self.emb = torch.nn.Embedding(num_embeddings=num_embs, embedding_dim=aux_channels)
        self.spk_emb = torch.nn.Embedding(num_embeddings=num_spk_embs, embedding_dim=spk_emb_dim)
        # the reference registers the tables first: same state-dict order
        mods = self._modules
        items = [(k, mods[k]) for k in ("emb", "spk_emb")] + [(k, v) for k, v in mods.items() if k not in ("emb", "spk_emb")]
        mods.clear()
        mods.update(items)
        self._tables = None  # (emb, spk_emb) fp32 device tensors and the packed image they were read with

    def register_stats(self, stats):
        raise NotImplementedError("DiscreteSymbolStyleMelGANGenerator uses no feature statistics")

    def _device(self):
        dev = self.emb.weight.device
        if dev.type != "cuda":
            raise RuntimeError("parallelwavegan_amd.DiscreteSymbolStyleMelGANGenerator runs on a ROCm GPU only; move "
                               "the module with .to('cuda') (there is no CPU fallback)")
        return dev

    def engine(self):
        eng = super().engine()  # repacks when a parameter (the tables among them) changed
        if self._tables is None or self._tables[2] is not eng.packed:
            dev = eng.device
            self._tables = (self.emb.weight.detach().to(dev, torch.float32).contiguous(),
                            self.spk_emb.weight.detach().to(dev, torch.float32).contiguous(), eng.packed)
        return eng

    def _plan(self, eng, frames, noise_len):
        key = (tuple(frames), tuple(noise_len))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 16:
                self._plans.clear()
            plan = self._plans[key] = eng.plan(frames, noise_len, _lib.PWG_SMG_PLAN_TRIM_NOISE)
        return plan

    # ------------------------------------------------------------------ token front end
    def _check_host(self, toks, spks):
        for u, t in enumerate(toks):
            if isinstance(t, np.ndarray):
                bad = np.flatnonzero((t < 0) | (t >= self.num_embs))
                if bad.size:
                    raise ValueError(f"bad token id {int(t[bad[0]])} at frame {int(bad[0])} of utterance {u}: outside "
                                     f"[0, {self.num_embs})")
        for u, g in enumerate(spks):
            if not torch.is_tensor(g) and not 0 <= g < self.num_spk_embs:
                raise ValueError(f"bad speaker id {g} of utterance {u}: outside [0, {self.num_spk_embs})")

    def _run_tokens(self, toks, spks, zs, keep=None):
        """toks: per utterance a 1-D int64 ndarray (host) or long tensor (device); spks: per utterance an
        int or a 0-dim long device tensor; zs: per utterance (Lz, in_channels) or None (drawn here, Lz =
        (T - 1) // noise_upsample_factor + 1). Returns the per-utterance outputs (T * upsample_factor,
        out_channels). keep: a dict that receives the plan and the workspace (tests)."""
        frames = [int(t.shape[0]) for t in toks]
        if min(frames) < 2:
            raise ValueError("every utterance needs at least two frames (the reference's InstanceNorm1d raises on "
                             "one)")
        self._check_host(toks, spks)  # before any GPU use
        eng = self.engine()
        dev = eng.device
        emb, spk, _ = self._tables
        nf = int(self.noise_upsample_factor)
        if zs is None:
            zs = [torch.randn((f - 1) // nf + 1, self.in_channels, dtype=torch.float32, device=dev) for f in frames]
        else:
            zs = [self._rows(z, dev) for z in zs]
        if len(zs) != len(toks):
            raise ValueError("one noise tensor per utterance")
        for z in zs:
            if z.dim() != 2 or z.shape[1] != self.in_channels or z.shape[0] < 1:
                raise ValueError(f"z must be (Lz, {self.in_channels})")
        plan = self._plan(eng, frames, [int(z.shape[0]) for z in zs])
        hop = int(self.upsample_factor)
        with torch.cuda.device(dev):
            ids = torch.cat([torch.from_numpy(np.ascontiguousarray(t)).to(dev) if isinstance(t, np.ndarray)
                             else t.to(dev).reshape(-1) for t in toks]).contiguous()
            if any(torch.is_tensor(g) for g in spks):
                spk_ids = torch.stack([g.to(dev).reshape(()) if torch.is_tensor(g)
                                       else torch.tensor(int(g), dtype=torch.int64, device=dev) for g in spks])
            else:
                spk_ids = torch.tensor([int(g) for g in spks], dtype=torch.int64, device=dev)
            z_all = zs[0] if len(zs) == 1 else torch.cat(zs, 0)
            out = torch.empty(plan.out_rows, self.out_channels, dtype=torch.float32, device=dev)
            ws = eng.run_tokens(plan, emb, spk, ids, spk_ids.contiguous(), z_all, out, check=True)
        if keep is not None:
            keep.update(plan=plan, workspace=ws)
        outs, o = [], 0
        for f in frames:
            outs.append(out[o:o + f * hop])
            o += f * hop
        return outs

    # ------------------------------------------------------------------ reference API
    def forward(self, c, z=None):
        """models/style_melgan.py:486-519: c (B, 2, T) token ids and speaker ids (the speaker of utterance
        b is c[b, 1, 0]), z (B, in_channels, Lz) -> (B, out_channels, T * upsample_factor). T must equal
        Lz * noise_upsample_factor (the reference fails on the shape mismatch inside the first block); z=None
        draws Lz = 1 as the reference does. Float ids are truncated (``.long()``)."""
        if not torch.is_tensor(c):
            c = torch.as_tensor(np.asarray(c))
        if c.dim() != 3:
            raise ValueError("forward expects c (B, 2, T)")
        assert c.size(1) == 2
        if z is None:
            z = torch.randn(c.size(0), self.in_channels, 1, device=self._device())
        elif not torch.is_tensor(z):
            z = torch.from_numpy(np.asarray(z, np.float32))
        assert z.dim() == 3 and z.size(0) == c.size(0)
        assert c.size(2) == z.size(2) * int(self.noise_upsample_factor), \
            "c needs noise length * noise_upsample_factor frames"
        ids = _as_ids(c)
        toks = [ids[b, 0] for b in range(ids.shape[0])]
        spks = [ids[b, 1, 0] if torch.is_tensor(ids) else int(ids[b, 1, 0]) for b in range(ids.shape[0])]
        zs = [z[b].transpose(0, 1) for b in range(z.size(0))]
        return torch.stack([o.transpose(0, 1) for o in self._run_tokens(toks, spks, zs)], 0)

    def inference(self, c, g=None, normalize_before=False, z=None):
        """models/style_melgan.py:557-602: c (T, 2) [token id, speaker id], or (T, 1) / (T,) with ``g`` ->
        (T * upsample_factor, out_channels); ``g`` replaces the speaker column. ``z`` (1, in_channels, Lz) or
        (in_channels, Lz), Lz = (T - 1) // noise_upsample_factor + 1, makes a run reproducible (an extension;
        the reference always draws it)."""
        return self.inference_batch([c], g, None if z is None else [z], normalize_before)[0]

    def inference_batch(self, cs, g=None, zs=None, normalize_before=False):
        """Ragged list form of ``inference`` (what bin/decode.py calls): the whole batch is one trimmed plan,
        every utterance with its own speaker and its own instance-norm statistics. ``g``: None, one speaker
        id for every utterance, or one per utterance."""
        assert not normalize_before, "No statistics are used."
        n = len(cs)
        if g is not None:
            if torch.is_tensor(g) and g.dim() == 0 or not torch.is_tensor(g) and np.ndim(g) == 0:
                g = [g] * n
            if len(g) != n:
                raise ValueError("g needs one speaker id per utterance")
        toks, spks = [], []
        for u, c in enumerate(cs):
            ids = _as_ids(c)
            if ids.ndim == 1 and g is not None:
                ids = ids[:, None]
            if ids.ndim != 2:
                raise ValueError("c must be (T, 2), or (T, 1) / (T,) with g")
            if g is None:
                assert ids.shape[1] == 2
            if ids.shape[0] < 1:
                raise ValueError("every utterance needs at least one frame")
            toks.append(ids[:, 0])
            s = ids[0, 1] if g is None else g[u]
            spks.append(s.long() if torch.is_tensor(s) and s.device.type != "cpu" else int(s))
        if zs is not None:
            rows = []
            for z in zs:
                if not torch.is_tensor(z):
                    z = torch.from_numpy(np.asarray(z, np.float32))
                if z.dim() == 3:
                    assert z.size(0) == 1
                    z = z[0]
                rows.append(z.transpose(0, 1))
            zs = rows
        return self._run_tokens(toks, spks, zs)
