"""Drop-in ``VQVAE`` (waveform -> codes -> waveform) running on the MI355X kernels of include/pwg_vq.h
and the conv-network executor (include/pwg_cnet.h).

Mirrors the reference's parallel_wavegan.models.VQVAE (parallel_wavegan/models/vqvae.py:16-171): same
constructor arguments and defaults, sub-module names and state-dict keys (``encoder.layers.N...``,
``codebook.embedding.weight``, ``decoder.melgan...``, ``local_embed.*``, ``global_embed.weight``; with
``use_weight_norm`` the convs of all three parts carry weight_g / weight_v), ``encode(x)``,
``decode(indices, l, g)``, ``forward(x, l, g)`` (eval semantics, no gradients), ``remove_weight_norm``,
``apply_weight_norm``; plus the ragged ``encode_batch``, ``decode_batch`` and ``inference_batch``.

Data flow. Encode: the encoder is a MelGANDiscriminator (models/melgan.py:260-396) -- its first layer
(ReflectionPad1d + Conv1d(1 -> C) + LeakyReLU) is pwg_vq_wave_rows, every grouped strided level one
pwg_vq_gsconv over rows packed at their true lengths (an utterance of n rows leaves a level with
ceil(n / s) rows, the reference's floor((n - 1) / s) + 1), the two dense convs at the frame rate a
two-op program of the executor, and the codebook's arg-min pwg_vq_nearest. Decode: pwg_vq_decode_rows
writes the channel concatenation [codebook[idx] ; local_embed(l) ; global_embed[g]] as the input rows
of the decoder, the project's MelGANGenerator drop-in. Graph replay is off (a single chain gains
nothing from it). The torch modules only hold parameters; a CPU module raises.
"""

import copy
import ctypes
import logging

import numpy as np
import torch

from . import _lib, cnet
from .engine import WeightTracker, first_parameter, fold_weight_norm, forget_device
from .melgan import MelGANGenerator, _slope

DEFAULT_ENCODER_CONF = {"out_channels": 256, "downsample_scales": [4, 4, 2, 2], "max_downsample_channels": 1024}
DEFAULT_DECODER_CONF = {"in_channels": 256, "upsample_scales": [4, 4, 2, 2], "channels": 512, "stacks": 3}


class MelGANDiscriminatorHolder(torch.nn.Module):
    """Parameter holder with the layout of the reference's MelGANDiscriminator (models/melgan.py:
    260-396): layers[0] = [pad, Conv1d(in -> C, k0 * k1), act], one [grouped strided Conv1d, act] per
    downsample scale, [Conv1d(k0), act], Conv1d(k1)."""

    def __init__(self, in_channels=1, out_channels=1, kernel_sizes=[5, 3], channels=16, max_downsample_channels=1024,
                 bias=True, downsample_scales=[4, 4, 4, 4], nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, pad="ReflectionPad1d", pad_params={}):
        super().__init__()
        assert len(kernel_sizes) == 2
        assert kernel_sizes[0] % 2 == 1
        assert kernel_sizes[1] % 2 == 1
        if nonlinear_activation != "LeakyReLU":
            raise NotImplementedError(f"encoder nonlinear_activation={nonlinear_activation!r}: only LeakyReLU is accelerated")
        if pad != "ReflectionPad1d":
            raise NotImplementedError(f"encoder pad={pad!r}: only ReflectionPad1d is accelerated")
        if in_channels != 1:
            raise NotImplementedError(f"in_channels={in_channels}: the multi-band form is not accelerated")
        k_first = int(np.prod(kernel_sizes))
        if k_first > 31:
            raise NotImplementedError(f"kernel_sizes={list(kernel_sizes)}: their product (the first layer's kernel) "
                                      f"must not exceed 31")
        if channels < 16 or channels % 16:
            raise NotImplementedError(f"encoder channels={channels}: must be a multiple of 16")
        act = torch.nn.LeakyReLU
        self.layers = torch.nn.ModuleList()
        self.layers += [torch.nn.Sequential(torch.nn.ReflectionPad1d((k_first - 1) // 2, **pad_params),
                                            torch.nn.Conv1d(in_channels, channels, k_first, bias=bias),
                                            act(**nonlinear_activation_params))]
        in_chs = channels
        for s in downsample_scales:
            if not 2 <= s <= 4:
                raise NotImplementedError(f"downsample_scales: scales must be within 2..4, got {s}")
            out_chs = min(in_chs * s, max_downsample_channels)
            groups = in_chs // 4
            if out_chs % groups or out_chs // groups not in (4, 8, 16) or out_chs % 16:
                raise NotImplementedError(f"downsample level {in_chs} -> {out_chs}: outputs per group must be 4, 8 "
                                          f"or 16 (channels, downsample_scales, max_downsample_channels)")
            self.layers += [torch.nn.Sequential(
                torch.nn.Conv1d(in_chs, out_chs, kernel_size=s * 10 + 1, stride=s, padding=s * 5, groups=groups, bias=bias),
                act(**nonlinear_activation_params))]
            in_chs = out_chs
        out_chs = min(in_chs * 2, max_downsample_channels)
        self.layers += [torch.nn.Sequential(
            torch.nn.Conv1d(in_chs, out_chs, kernel_sizes[0], padding=(kernel_sizes[0] - 1) // 2, bias=bias),
            act(**nonlinear_activation_params))]
        self.layers += [torch.nn.Conv1d(out_chs, out_channels, kernel_sizes[1], padding=(kernel_sizes[1] - 1) // 2,
                                        bias=bias)]
        self.downsample_scales = tuple(int(s) for s in downsample_scales)
        self.out_channels = out_channels
        self.reset_parameters()

    def reset_parameters(self):
        """models/melgan.py:381-396: conv weights ~ N(0, 0.02)."""
        def _reset(m):
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)):
                m.weight.data.normal_(0.0, 0.02)
        self.apply(_reset)


class VQCodebook(torch.nn.Module):
    """layers/vector_quantize_codebook.py:17-30: the embedding table, uniform(+-1 / num_embeds)."""

    def __init__(self, num_embeds, embed_dim):
        super().__init__()
        self.embedding = torch.nn.Embedding(num_embeds, embed_dim)
        self.embedding.weight.data.uniform_(-1.0 / num_embeds, 1.0 / num_embeds)


def lower_encoder_tail(enc):
    """The two dense convs at the frame rate as a conv-network program: buffer 0 holds the last
    grouped level's rows, the last buffer ``out_channels`` (= embed_dim) channels, no tanh."""
    c5, a5 = enc.layers[-2][0], enc.layers[-2][1]
    c3 = enc.layers[-1]
    n = len(enc.layers)
    P = cnet.Program(c5.in_channels)
    h = P.buffer(c5.out_channels, 1)
    k5, k3 = f"layers.{n - 2}.0", f"layers.{n - 1}"
    P.conv(k5, h, c5.out_channels,
           [P.src(0, c5.in_channels, c5.kernel_size[0], 1, c5.padding[0], cnet.PAD_ZERO, 1.0, k5 + ".weight")],
           bias=k5 + ".bias" if c5.bias is not None else None)
    y = P.buffer(c3.out_channels, 1)
    P.conv(k3, y, c3.out_channels,
           [P.src(h, c5.out_channels, c3.kernel_size[0], 1, c3.padding[0], cnet.PAD_ZERO, _slope(a5), k3 + ".weight")],
           bias=k3 + ".bias" if c3.bias is not None else None)
    return P


class VQVAE(torch.nn.Module):
    """models/vqvae.py:16-171, executed on the MI355X kernels."""

    def __init__(self, in_channels=1, out_channels=1, num_embeds=512, embed_dim=256, num_local_embeds=None,
                 local_embed_dim=None, num_global_embeds=None, global_embed_dim=None,
                 encoder_type="MelGANDiscriminator", decoder_type="MelGANGenerator",
                 encoder_conf=DEFAULT_ENCODER_CONF, decoder_conf=DEFAULT_DECODER_CONF, use_weight_norm=True):
        super().__init__()
        if encoder_type != "MelGANDiscriminator":
            raise NotImplementedError(f"encoder_type={encoder_type!r}: only MelGANDiscriminator is accelerated")
        if decoder_type != "MelGANGenerator":
            raise NotImplementedError(f"decoder_type={decoder_type!r}: only MelGANGenerator is accelerated")
        if in_channels != 1:
            raise NotImplementedError(f"in_channels={in_channels}: the multi-band form is not accelerated")
        if out_channels != 1:
            raise NotImplementedError(f"out_channels={out_channels}: the multi-band form is not accelerated")
        if embed_dim < 16 or embed_dim % 16 or embed_dim > 1024:
            raise NotImplementedError(f"embed_dim={embed_dim}: must be a multiple of 16 up to 1024")
        # (the reference updates its default dicts in place; these are copies)
        encoder_conf = dict(copy.deepcopy(encoder_conf), in_channels=in_channels)
        decoder_conf = dict(copy.deepcopy(decoder_conf), out_channels=out_channels)
        self.local_dim = 0
        if num_local_embeds is not None:
            if local_embed_dim is not None:
                if local_embed_dim % 16:
                    raise NotImplementedError(f"local_embed_dim={local_embed_dim}: must be a multiple of 16")
                self.local_embed = torch.nn.Conv1d(num_local_embeds, local_embed_dim, 1)
                self.local_dim = int(local_embed_dim)
            else:
                if num_local_embeds % 16:
                    raise NotImplementedError(f"num_local_embeds={num_local_embeds}: without a projection the local "
                                              f"rows are copied and must be a multiple of 16 wide")
                self.local_embed = None
                self.local_dim = int(num_local_embeds)
        self.global_dim = 0
        if num_global_embeds is not None:
            if global_embed_dim is None or global_embed_dim % 16:
                raise NotImplementedError(f"global_embed_dim={global_embed_dim}: must be a multiple of 16")
            self.global_embed = torch.nn.Embedding(num_global_embeds, global_embed_dim)
            self.global_dim = int(global_embed_dim)
        self.num_local_embeds, self.num_global_embeds = num_local_embeds, num_global_embeds
        self.num_embeds, self.embed_dim = int(num_embeds), int(embed_dim)
        self.encoder = MelGANDiscriminatorHolder(**encoder_conf)
        self.codebook = VQCodebook(num_embeds=num_embeds, embed_dim=embed_dim)
        self.decoder = MelGANGenerator(**decoder_conf)
        self.decoder.program(False)  # (lowering refuses what the drop-in refuses: now, not at the first call)
        if self.encoder.out_channels != embed_dim:
            raise ValueError(f"encoder_conf out_channels={self.encoder.out_channels} must equal embed_dim={embed_dim}")
        want = self.embed_dim + self.local_dim + self.global_dim
        if self.decoder.in_channels != want:
            raise ValueError(f"decoder_conf in_channels={self.decoder.in_channels} must equal embed_dim + local + "
                             f"global dims = {want}")
        self.downsample_factor = int(np.prod(self.encoder.downsample_scales))
        self.upsample_factor = self.decoder.upsample_factor
        if use_weight_norm:
            self.remove_weight_norm()  # the decoder applied its own (models/vqvae.py:81-83)
            self.apply_weight_norm()
        self._tail = None      # CnetEngine of the encoder's dense tail
        self._front = None     # device weights of the HIP front ends
        self._weights = WeightTracker()
        self.stage_events = None  # a list: every stage appends (name, event recorded at its end)

    def _mark(self, name):
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    # ------------------------------------------------------------------ reference API
    def apply_weight_norm(self):
        def _apply(m):
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)):
                torch.nn.utils.weight_norm(m)
        self.apply(_apply)

    def remove_weight_norm(self):
        def _remove(m):
            try:
                torch.nn.utils.remove_weight_norm(m)
            except ValueError:
                return
        self.apply(_remove)

    # ------------------------------------------------------------------ engine plumbing
    def _device(self):
        dev = first_parameter(self).device
        if dev.type != "cuda":
            raise RuntimeError("parallelwavegan_amd.VQVAE runs on a ROCm GPU only; move the module with .to('cuda') "
                               "(there is no CPU fallback)")
        return dev

    def _apply(self, fn, *args, **kwargs):
        forget_device(self)
        if getattr(self, "_weights", None) is not None:
            self._weights.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def invalidate_weights(self):
        self._weights.invalidate()
        self.decoder.invalidate_weights()

    def _prepare(self):
        """Engines and device weights, re-packed when a parameter changed."""
        dev = self._device()
        if self._tail is None or self._tail.device != dev:
            self._tail = cnet.CnetEngine(lower_encoder_tail(self.encoder), dev)
            self._tail.set_graphs(False)
            self._weights.invalidate()
        if self._weights.changed(self):
            L = _lib.load()
            with torch.no_grad():
                enc = fold_weight_norm({k: v for k, v in self.encoder.state_dict().items()})
                self._tail.load_state_dict(enc)

                def up(a):
                    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

                c0 = self.encoder.layers[0][1]
                front = dict(w0=up(enc["layers.0.1.weight"].reshape(c0.out_channels, -1)),
                             b0=up(enc["layers.0.1.bias"]) if c0.bias is not None else None, levels=[])
                for i, s in enumerate(self.encoder.downsample_scales):
                    conv = self.encoder.layers[1 + i][0]
                    w = np.ascontiguousarray(enc[f"layers.{1 + i}.0.weight"], np.float32)
                    n = L.pwg_vq_gsconv_packed_count(conv.in_channels, conv.out_channels, s)
                    if n < 0:
                        raise NotImplementedError(f"grouped level {conv.in_channels} -> {conv.out_channels}, stride {s}")
                    packed = np.empty(n, np.float32)
                    _lib.check(L.pwg_vq_gsconv_pack(w.ctypes.data, conv.in_channels, conv.out_channels, s,
                                                    packed.ctypes.data))
                    front["levels"].append((up(packed), up(enc[f"layers.{1 + i}.0.bias"]) if conv.bias is not None else None,
                                            conv.in_channels, conv.out_channels, s, _slope(self.encoder.layers[1 + i][1])))
                book = self.codebook.embedding.weight.detach().to(dev, torch.float32).contiguous()
                front["book"] = book
                front["enorm"] = torch.empty(self.num_embeds, dtype=torch.float32, device=dev)
                with torch.cuda.device(dev):
                    _lib.check(L.pwg_vq_code_norms(book.data_ptr(), self.num_embeds, self.embed_dim,
                                                   front["enorm"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
                if getattr(self, "local_embed", None) is not None:
                    le = fold_weight_norm({"local_embed." + k: v for k, v in self.local_embed.state_dict().items()})
                    front["wl"] = up(le["local_embed.weight"].reshape(self.local_dim, -1))
                    front["bl"] = up(le["local_embed.bias"])
                if self.global_dim:
                    front["glob"] = self.global_embed.weight.detach().to(dev, torch.float32).contiguous()
                front["flag"] = torch.zeros(1, dtype=torch.int32, device=dev)
                self._front = front
            self._weights.mark_packed()
        eng = self.decoder.engine(False)
        eng.set_graphs(False)
        return dev

    @staticmethod
    def _starts(lengths, dev):
        starts = np.zeros(len(lengths) + 1, np.int64)
        np.cumsum(lengths, out=starts[1:])
        return starts, torch.from_numpy(starts).to(dev)

    def _encode_rows(self, xs, want_zq=False, keep=None):
        """Packed encoder output of a ragged batch: (z rows x embed_dim, idx rows int64, zq or None,
        frames per utterance)."""
        dev = self._prepare()
        L, F = _lib.load(), self._front
        xs = [torch.as_tensor(x, dtype=torch.float32).to(dev).reshape(-1) for x in xs]
        if not xs:
            raise ValueError("at least one utterance is required")
        enc = self.encoder
        k0 = enc.layers[0][1].kernel_size[0]
        lens = [int(x.numel()) for x in xs]
        for n in lens:
            if n < (k0 - 1) // 2 + 1:
                raise ValueError(f"an input of {n} samples is shorter than the {(k0 - 1) // 2 + 1} the encoder's "
                                 f"reflection padding needs")
        x = torch.cat(xs).contiguous() if len(xs) > 1 else xs[0].contiguous()
        host, rs = self._starts(lens, dev)
        rows, C = int(host[-1]), enc.layers[0][1].out_channels
        stream = torch.cuda.current_stream(dev).cuda_stream
        cur = torch.empty(rows * C, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            self._mark("begin")
            _lib.check(L.pwg_vq_wave_rows(x.data_ptr(), F["w0"].data_ptr(), F["b0"].data_ptr() if F["b0"] is not None else None,
                                          C, k0, ctypes.c_float(_slope(enc.layers[0][2])), rs.data_ptr(), host.ctypes.data,
                                          len(lens), rows, cur.data_ptr(), stream))
            self._mark("first_layer")
            if keep is not None:
                keep["levels"] = [(cur, list(lens))]
            for lvl, (wp, b, cin, cout, s, slope) in enumerate(F["levels"]):
                lens = [(n + s - 1) // s for n in lens]
                host_o, rs_o = self._starts(lens, dev)
                rows_o = int(host_o[-1])
                y = torch.empty(rows_o * cout, dtype=torch.float32, device=dev)
                _lib.check(L.pwg_vq_gsconv(cur.data_ptr(), rs.data_ptr(), rows, cin, wp.data_ptr(),
                                           b.data_ptr() if b is not None else None, cout, s, ctypes.c_float(slope),
                                           y.data_ptr(), rs_o.data_ptr(), rows_o, len(lens), stream))
                cur, rs, rows = y, rs_o, rows_o
                self._mark(f"level_{lvl + 1}")
                if keep is not None:
                    keep["levels"].append((cur, list(lens)))
            plan = self._tail.plan(lens)
            z = torch.empty(rows * self.embed_dim, dtype=torch.float32, device=dev)
            self._tail.run(plan, cur, z)
            self._mark("dense_tail")
            idx = torch.empty(rows, dtype=torch.int64, device=dev)
            zq = torch.empty(rows * self.embed_dim, dtype=torch.float32, device=dev) if want_zq else None
            F["flag"].zero_()
            _lib.check(L.pwg_vq_nearest(z.data_ptr(), rows, self.embed_dim, F["book"].data_ptr(), F["enorm"].data_ptr(),
                                        self.num_embeds, idx.data_ptr(), zq.data_ptr() if want_zq else None,
                                        F["flag"].data_ptr(), stream))
            self._mark("search")
        if int(F["flag"].item()) & _lib.PWG_VQ_BAD_INPUT:
            logging.warning("VQVAE.encode: the encoder output holds non-finite values; their frames get code 0")
        return z.view(rows, self.embed_dim), idx, (zq.view(rows, self.embed_dim) if want_zq else None), lens

    def _check_conditioning(self, ls, gs, n):
        has_l, has_g = self.num_local_embeds is not None, self.num_global_embeds is not None
        if (ls is not None) != has_l:
            raise ValueError("local conditioning: the model " + ("needs l" if has_l else "has no local_embed, but l was given"))
        if (gs is not None) != has_g:
            raise ValueError("global conditioning: the model " + ("needs g" if has_g else "has no global_embed, but g was given"))
        if ls is not None and len(ls) != n:
            raise ValueError("one local conditioning sequence per utterance is required")
        if gs is not None and len(gs) != n:
            raise ValueError("one global id per utterance is required")

    def _decode_rows(self, idx, frames, ls, gs):
        """The decoder over packed code rows: list of (T'_u * hop, 1)."""
        dev = self._prepare()
        L, F = _lib.load(), self._front
        self._check_conditioning(ls, gs, len(frames))
        rows = int(sum(frames))
        host, rs = self._starts(frames, dev)
        local = None
        if ls is not None:
            ls = [torch.as_tensor(l, dtype=torch.float32).to(dev) for l in ls]
            for l, f in zip(ls, frames):
                if l.dim() != 2 or l.size(0) != f or l.size(1) != self.num_local_embeds:
                    raise ValueError(f"l must be (T', {self.num_local_embeds}) with T' = {f} frames")
            local = torch.cat([l.reshape(-1) for l in ls]).contiguous()
        g_ids = None
        if gs is not None:
            g_ids = torch.as_tensor([int(g) for g in gs], dtype=torch.int64).to(dev)
        width = self.decoder.in_channels
        out = torch.empty(rows * width, dtype=torch.float32, device=dev)
        F["flag"].zero_()
        wl, bl, glob = F.get("wl"), F.get("bl"), F.get("glob")
        with torch.cuda.device(dev):
            self._mark("decode_begin")
            _lib.check(L.pwg_vq_decode_rows(
                F["book"].data_ptr(), self.num_embeds, self.embed_dim, idx.data_ptr(),
                local.data_ptr() if local is not None else None, self.num_local_embeds or 0,
                wl.data_ptr() if wl is not None and local is not None else None,
                bl.data_ptr() if bl is not None and local is not None else None, self.local_dim,
                glob.data_ptr() if glob is not None else None, self.num_global_embeds or 0, self.global_dim,
                g_ids.data_ptr() if g_ids is not None else None, rs.data_ptr(), len(frames), rows, out.data_ptr(),
                F["flag"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            self._mark("decode_front_end")
        flag = int(F["flag"].item())
        if flag & _lib.PWG_VQ_BAD_CODE:
            raise IndexError(f"a code index lies outside [0, {self.num_embeds})")
        if flag & _lib.PWG_VQ_BAD_GLOBAL:
            raise IndexError(f"a global id lies outside [0, {self.num_global_embeds})")
        ys = self.decoder.engine(False).infer_rows(list(frames), out)
        self._mark("decoder")
        return ys

    # ------------------------------------------------------------------ ragged batches
    def encode_batch(self, xs):
        """List of (T_u,) waveforms -> list of (T'_u,) int64 code sequences, T'_u = ceil(T_u / hop)."""
        _, idx, _, frames = self._encode_rows(list(xs))
        return list(torch.split(idx, frames))

    def decode_batch(self, idxs, ls=None, gs=None):
        """Lists of (T'_u,) codes, (T'_u, num_local_embeds) local rows and global ids -> list of
        (T'_u * hop, 1) waveforms."""
        dev = self._device()
        idxs = [torch.as_tensor(i, dtype=torch.int64).to(dev).reshape(-1) for i in idxs]
        if not idxs:
            raise ValueError("at least one utterance is required")
        frames = [int(i.numel()) for i in idxs]
        idx = torch.cat(idxs).contiguous() if len(idxs) > 1 else idxs[0].contiguous()
        return self._decode_rows(idx, frames, ls, gs)

    def inference_batch(self, xs, ls=None, gs=None):
        """wav -> codes -> wav over a ragged batch: (list of (T'_u * hop, 1), list of (T'_u,) codes)."""
        _, idx, _, frames = self._encode_rows(list(xs))
        ys = self._decode_rows(idx, frames, ls, gs)
        return ys, list(torch.split(idx, frames))

    # ------------------------------------------------------------------ reference forward paths
    def _check_x(self, x):
        if x.dim() != 3 or x.size(1) != 1:
            raise ValueError("expected x (B, 1, T)")

    @staticmethod
    def _local_rows(l, B):
        return None if l is None else [l[b].transpose(0, 1) for b in range(B)]

    def encode(self, x):
        """models/vqvae.py:113-125: x (B, 1, T) -> (B, T') int64."""
        self._check_x(x)
        B = x.size(0)
        _, idx, _, _ = self._encode_rows([x[b, 0] for b in range(B)])
        return idx.view(B, -1)

    def decode(self, indices, l=None, g=None):
        """models/vqvae.py:127-147: indices (B, T'), l (B, num_local_embeds, T'), g (B,) -> (B, 1, T' * hop)."""
        if indices.dim() != 2:
            raise ValueError("expected indices (B, T')")
        B = indices.size(0)
        ys = self.decode_batch([indices[b] for b in range(B)], self._local_rows(l, B),
                               None if g is None else [int(v) for v in g.reshape(-1)])
        return torch.stack([y.transpose(0, 1) for y in ys], 0)

    def forward(self, x, l=None, g=None):
        """models/vqvae.py:85-111 in eval: (x_bar (B, 1, T' * hop), z_e (B, embed_dim, T'), z_q (same))."""
        self._check_x(x)
        B = x.size(0)
        z, idx, zq, frames = self._encode_rows([x[b, 0] for b in range(B)], want_zq=True)
        ys = self._decode_rows(idx, frames, self._local_rows(l, B), None if g is None else [int(v) for v in g.reshape(-1)])
        x_bar = torch.stack([y.transpose(0, 1) for y in ys], 0)
        T = frames[0]
        return (x_bar, z.view(B, T, self.embed_dim).transpose(1, 2).contiguous(),
                zq.view(B, T, self.embed_dim).transpose(1, 2).contiguous())
