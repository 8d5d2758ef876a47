"""Drop-in ``UHiFiGANGenerator`` running on the MI355X conv-network executor (include/pwg_cnet.h).

Mirrors the reference's parallel_wavegan.models.UHiFiGANGenerator (parallel_wavegan/models/
uhifigan.py:19-387): same constructor arguments and defaults, sub-module names and state-dict keys
(input_conv.0, downsamples.i.0, downsamples_mrf.n, hidden_conv, upsamples.i.1, upsamples_mrf.n,
output_conv.1), ``forward(c, f0, excitation)``, ``inference(excitation, f0, c, normalize_before)``,
``remove_weight_norm``, ``apply_weight_norm``, ``reset_parameters``, ``register_stats``; plus
``inference_batch`` for ragged batches, and ``excitation_from_f0`` / ``inference_from_f0`` /
``inference_batch_from_f0``, which generate the excitation on the GPU from frame-rate f0 (the HIP sine
generator pwg_sine_frames, include/pwg_sine.h: what the reference's preprocessing computes on the CPU
with SineGen, bin/preprocess.py:420-442). Eval semantics: Dropout is the identity.

The network is a U-Net (models/uhifigan.py:273-301). The excitation signal at the sample rate goes
through input_conv (1 -> C; the HIP front end pwg_uhg_excite_rows, include/pwg_uhg.h, whose output is
the program's external buffer), then per level through a multi-receptive-field stage (the averaged
parallel residual blocks ``lower_mrf`` shares with HiFiGAN) and a strided conv C -> 2C down to the
next rate (PWG_CNET_SCONV). The mel goes through hidden_conv; every decoder level runs a
ConvTranspose1d over the channel concatenation of the decoder state and the encoder level of the
same rate (one two-source PWG_CNET_CONVT, no concatenated copy) and an MRF stage.

Quirks of the reference, reproduced: ``inference`` never normalises (normalize_before is accepted and
ignored, models/uhifigan.py:360-387), ``f0`` is never used, the last LeakyReLU has torch's default
slope 0.01.
"""

import ctypes
import logging

import numpy as np
import torch

from . import _lib, cnet
from .engine import WeightTracker, first_parameter, fold_weight_norm, forget_device
from .hifigan import HiFiGANResidualBlock, _conv_bias, _conv_src, lower_mrf
from .melgan import _slope


def lower_uhifigan(m):
    """The conv-network program of a UHiFiGAN body. Buffer 0 is the mel (rate 1); the external
    buffer holds input_conv's output at the sample rate (rate = hop). ``m.taps`` names the buffers
    a test can read back (pwg_cnet_plan_buffer)."""
    P = cnet.Program(m.in_channels)
    nb = m.num_blocks
    ch, rate = m.channels, m.upsample_factor
    cur = P.external_buffer(ch, rate)
    taps = dict(excite=cur, down_mrf=[], down=[], up=[], up_mrf=[])
    skips = []
    for i, s in enumerate(m.downsample_scales):
        acc = lower_mrf(P, m.downsamples_mrf, i * nb, nb, "downsamples_mrf", cur, ch, rate)
        conv, act = m.downsamples[i][0], m.downsamples[i][1]
        key = f"downsamples.{i}.0"
        rate //= s
        cur = P.buffer(2 * ch, rate)
        P.sconv(key, cur, 2 * ch, P.src(acc, ch, taps=conv.kernel_size[0], pad=conv.padding[0], weight=key + ".weight"),
                s, conv.padding[0], bias=key + ".bias" if conv.bias is not None else None,
                post_act=cnet.ACT_LRELU, post_slope=_slope(act))
        ch *= 2
        skips.append(cur)
        taps["down_mrf"].append(acc)
        taps["down"].append(cur)
    skips.reverse()
    hc = m.hidden_conv
    cur = P.buffer(ch, rate)
    taps["hidden"] = cur
    P.conv("hidden_conv", cur, ch,
           [P.src(0, m.in_channels, hc.kernel_size[0], 1, hc.padding[0], cnet.PAD_ZERO, 1.0, "hidden_conv.weight")],
           bias="hidden_conv.bias" if hc.bias is not None else None)
    for i, s in enumerate(m.upsample_scales):
        act, ct = m.upsamples[i][0], m.upsamples[i][1]
        key = f"upsamples.{i}.1"
        rate *= s
        up = P.buffer(ct.out_channels, rate)
        # torch.cat((hidden_mel, residual_results[i]), dim=1): the decoder state's rows come first
        P.convt(key, up, ct.out_channels, P.src(cur, ch, pre_slope=_slope(act), weight=key + ".weight"), s,
                ct.padding[0], ct.output_padding[0], bias=key + ".bias" if ct.bias is not None else None,
                src2=P.src(skips[i], ch, pre_slope=_slope(act)))
        ch = ct.out_channels
        cur = lower_mrf(P, m.upsamples_mrf, i * nb, nb, "upsamples_mrf", up, ch, rate)
        taps["up"].append(up)
        taps["up_mrf"].append(cur)
    out = P.buffer(m.out_channels, rate)
    P.conv("output_conv.1", out, m.out_channels, [_conv_src(P, cur, ch, m.output_conv, "output_conv")],
           bias=_conv_bias(m.output_conv, "output_conv"), post_act=cnet.ACT_TANH)
    m.taps = taps
    return P


class UHiFiGANGenerator(torch.nn.Module):
    """models/uhifigan.py:19-387, executed on the MI355X conv-network engine."""

    def __init__(self, in_channels=80, out_channels=1, channels=512, kernel_size=7, downsample_scales=(8, 8, 2, 2),
                 downsample_kernel_sizes=(16, 16, 4, 4), upsample_scales=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], dropout=0.3, use_additional_convs=True,
                 bias=True, nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_causal_conv=False, use_weight_norm=True):
        super().__init__()
        assert kernel_size % 2 == 1, "Kernel size must be odd number."
        assert len(upsample_scales) == len(upsample_kernel_sizes)
        assert len(resblock_dilations) == len(resblock_kernel_sizes)
        if use_causal_conv:
            # (the reference cannot build it either: CausalConv1d takes no padding / stride, TypeError)
            raise NotImplementedError("use_causal_conv=True: the causal UHiFiGAN is not accelerated")
        if nonlinear_activation != "LeakyReLU":
            raise NotImplementedError(f"nonlinear_activation={nonlinear_activation!r}: only LeakyReLU is accelerated")
        if out_channels != 1:
            raise NotImplementedError(f"out_channels={out_channels}: the excitation front end takes one channel")
        if list(downsample_scales) != list(reversed(list(upsample_scales))):
            # (the reference's torch.cat then fails on every input)
            raise NotImplementedError("downsample_scales must be upsample_scales reversed")
        if len(downsample_kernel_sizes) != len(downsample_scales):
            raise NotImplementedError("downsample_kernel_sizes must have one entry per downsample scale")
        for name, scales, kernels in (("downsample", downsample_scales, downsample_kernel_sizes),
                                      ("upsample", upsample_scales, upsample_kernel_sizes)):
            for s, k in zip(scales, kernels):
                if not 2 <= s <= 8:
                    raise NotImplementedError(f"{name}_scales: scales must be within 2..8, got {s}")
                if k != 2 * s:
                    raise NotImplementedError(f"{name}_kernel_sizes must be 2 * scale, got {k} for scale {s}")
        if channels % 16 or in_channels % 16:
            raise NotImplementedError("channels and in_channels must be multiples of 16")
        if kernel_size > 11:
            raise NotImplementedError("kernel_size: the excitation front end takes at most 11 taps")
        self.num_upsamples = len(upsample_kernel_sizes)
        self.num_blocks = len(resblock_kernel_sizes)
        self.use_causal_conv = False
        self.in_channels, self.out_channels, self.channels = in_channels, out_channels, channels
        self.downsample_scales = tuple(int(s) for s in downsample_scales)
        self.upsample_scales = tuple(int(s) for s in upsample_scales)
        self.upsample_factor = int(np.prod(upsample_scales))
        act = getattr(torch.nn, nonlinear_activation)
        pad = (kernel_size - 1) // 2
        self.downsamples = torch.nn.ModuleList()
        self.downsamples_mrf = torch.nn.ModuleList()
        self.upsamples = torch.nn.ModuleList()
        self.upsamples_mrf = torch.nn.ModuleList()
        self.input_conv = torch.nn.Sequential(
            torch.nn.Conv1d(out_channels, channels, kernel_size, bias=bias, padding=pad),
            act(**nonlinear_activation_params),
            torch.nn.Dropout(dropout),
        )
        ch = channels
        for i, s in enumerate(downsample_scales):
            for j in range(len(resblock_kernel_sizes)):
                self.downsamples_mrf += [HiFiGANResidualBlock(resblock_kernel_sizes[j], ch, resblock_dilations[j], bias,
                                                              use_additional_convs, nonlinear_activation,
                                                              nonlinear_activation_params, False)]
            self.downsamples += [torch.nn.Sequential(
                torch.nn.Conv1d(ch, ch * 2, downsample_kernel_sizes[i], stride=s, bias=bias, padding=s // 2 + s % 2),
                act(**nonlinear_activation_params),
                torch.nn.Dropout(dropout),
            )]
            ch *= 2
        self.hidden_conv = torch.nn.Conv1d(in_channels, ch, kernel_size, bias=bias, padding=pad)
        for i, s in enumerate(upsample_scales):
            self.upsamples += [torch.nn.Sequential(
                act(**nonlinear_activation_params),
                torch.nn.ConvTranspose1d(ch * 2, ch // 2, upsample_kernel_sizes[i], s, padding=s // 2 + s % 2,
                                         output_padding=s % 2, bias=bias),
            )]
            for j in range(len(resblock_kernel_sizes)):
                self.upsamples_mrf += [HiFiGANResidualBlock(resblock_kernel_sizes[j], ch // 2, resblock_dilations[j],
                                                            bias, use_additional_convs, nonlinear_activation,
                                                            nonlinear_activation_params, False)]
            ch //= 2
        self.output_conv = torch.nn.Sequential(
            torch.nn.LeakyReLU(),  # slope 0.01, as the reference (models/uhifigan.py:227-239)
            torch.nn.Conv1d(ch, out_channels, kernel_size, bias=bias, padding=pad),
            torch.nn.Tanh(),
        )
        if use_weight_norm:
            self.apply_weight_norm()
        self.reset_parameters()
        self._engine = None
        self._weights = WeightTracker()
        self._front = None  # (weight, bias or None) of input_conv.0 on the device, folded

    # ------------------------------------------------------------------ reference API
    def reset_parameters(self):
        """models/uhifigan.py:303-316: conv weights ~ N(0, 0.01)."""
        def _reset(m):
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)):
                m.weight.data.normal_(0.0, 0.01)
        self.apply(_reset)

    def remove_weight_norm(self):
        def _remove(m):
            try:
                torch.nn.utils.remove_weight_norm(m)
            except ValueError:
                return
        self.apply(_remove)

    def apply_weight_norm(self):
        def _apply(m):
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)):
                torch.nn.utils.weight_norm(m)
        self.apply(_apply)

    def register_stats(self, stats):
        """models/uhifigan.py:342-358 (.npy; .h5 needs h5py). The buffers are registered as in the
        reference; ``inference`` never applies them (see the module docstring)."""
        assert stats.endswith(".h5") or stats.endswith(".npy")
        if stats.endswith(".h5"):
            import h5py
            with h5py.File(stats, "r") as f:
                mean, scale = f["mean"][()].reshape(-1), f["scale"][()].reshape(-1)
        else:
            arr = np.load(stats)
            mean, scale = arr[0].reshape(-1), arr[1].reshape(-1)
        dev = first_parameter(self).device
        self.register_buffer("mean", torch.from_numpy(np.asarray(mean)).float().to(dev))
        self.register_buffer("scale", torch.from_numpy(np.asarray(scale)).float().to(dev))
        logging.info("Successfully registered stats as buffer.")

    # ------------------------------------------------------------------ lowering / engine plumbing
    def program(self):
        return lower_uhifigan(self)

    def _device(self):
        dev = first_parameter(self).device
        if dev.type != "cuda":
            raise RuntimeError("parallelwavegan_amd.UHiFiGANGenerator runs on a ROCm GPU only; move the module "
                               "with .to('cuda') (there is no CPU fallback)")
        return dev

    def _apply(self, fn, *args, **kwargs):
        forget_device(self)
        if getattr(self, "_weights", None) is not None:
            self._weights.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def invalidate_weights(self):
        self._weights.invalidate()

    def engine(self):
        dev = self._device()
        if self._engine is None or self._engine.device != dev:
            self._engine = cnet.CnetEngine(self.program(), dev)
            self._weights.invalidate()
        if self._weights.changed(self):
            with torch.no_grad():
                state = {k: v for k, v in self.state_dict().items() if k not in ("mean", "scale")}
                self._engine.load_state_dict(state)
                front = fold_weight_norm({k: v for k, v in state.items() if k.startswith("input_conv.0.")})
                w = torch.from_numpy(np.ascontiguousarray(front["input_conv.0.weight"], np.float32)).to(dev)
                b = front.get("input_conv.0.bias")
                if b is not None:
                    b = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev)
                self._front = (w.reshape(self.channels, -1).contiguous(), b)
            self._weights.mark_packed()
        return self._engine

    def _excite(self, exc, frames, dev):
        """input_conv over the packed excitation rows: the external buffer's rows (rows x channels)."""
        L = _lib.load()
        w, b = self._front
        hop = self.upsample_factor
        starts = np.zeros(len(frames) + 1, np.int64)
        np.cumsum([f * hop for f in frames], out=starts[1:])
        row_start = torch.from_numpy(starts).to(dev)
        rows = int(starts[-1])
        out = torch.empty(rows * self.channels, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(L.pwg_uhg_excite_rows(exc.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                             self.channels, w.shape[1], ctypes.c_float(_slope(self.input_conv[1])),
                                             row_start.data_ptr(), len(frames), rows, out.data_ptr(),
                                             stream.cuda_stream))
        return out, row_start

    def _run(self, cs, excs, keep=None):
        dev = self._device()
        if len(cs) != len(excs) or not cs:
            raise ValueError("one excitation per utterance is required")
        hop = self.upsample_factor
        cs = [torch.as_tensor(c, dtype=torch.float32).to(dev).contiguous() for c in cs]
        excs = [torch.as_tensor(e, dtype=torch.float32).to(dev).reshape(-1) for e in excs]
        for c, e in zip(cs, excs):
            if c.dim() != 2 or c.size(1) != self.in_channels:
                raise ValueError(f"c must be (T, {self.in_channels})")
            if e.numel() != c.size(0) * hop:
                raise ValueError(f"excitation has {e.numel()} samples, expected T * prod(upsample_scales) = "
                                 f"{c.size(0)} * {hop} = {c.size(0) * hop}")
        exc = torch.cat(excs).contiguous() if len(excs) > 1 else excs[0].contiguous()
        return self._run_packed(cs, exc, keep)

    def _run_packed(self, cs, exc, keep=None):
        """The body over device mels ``cs`` and the packed excitation rows of the whole batch."""
        dev = self._device()
        eng = self.engine()
        frames = [int(c.size(0)) for c in cs]
        mel = torch.cat([c.reshape(-1) for c in cs]) if len(cs) > 1 else cs[0].reshape(-1)
        ext, row_start = self._excite(exc, frames, dev)
        outs = eng.infer_rows(frames, mel, ext=ext)
        if keep is not None:
            plan = eng.plan(frames)
            keep.update(plan=plan, workspace=eng.workspace(plan.workspace_bytes), ext=ext, frames=frames)
        return outs

    # ------------------------------------------------------------------ forward paths
    def forward(self, c=None, f0=None, excitation=None):
        """models/uhifigan.py:261-301: c (B, in_channels, T), excitation (B, 1, T * hop) ->
        (B, out_channels, T * hop). ``f0`` is accepted and ignored, as in the reference."""
        if c is None or excitation is None:
            raise ValueError("forward needs c and excitation")
        if c.dim() != 3 or c.size(1) != self.in_channels:
            raise ValueError(f"forward expects c (B, {self.in_channels}, T)")
        if excitation.dim() != 3 or excitation.size(0) != c.size(0) or excitation.size(1) != 1:
            raise ValueError("forward expects excitation (B, 1, T * prod(upsample_scales))")
        outs = self._run([c[b].transpose(0, 1) for b in range(c.size(0))],
                         [excitation[b, 0] for b in range(c.size(0))])
        return torch.stack([o.transpose(0, 1) for o in outs], 0)

    def inference(self, excitation=None, f0=None, c=None, normalize_before=False):
        """models/uhifigan.py:360-387: c (T, in_channels), excitation (T * hop,) -> (T * hop, out_channels).
        ``normalize_before`` and ``f0`` are accepted and ignored, as in the reference."""
        if c is None or excitation is None:
            raise ValueError("inference needs excitation and c")
        return self._run([c], [excitation])[0]

    def inference_batch(self, cs, excitations):
        """Ragged batch: lists of (T_u, in_channels) and (T_u * hop,) -> list of (T_u * hop, out_channels);
        one plan for the batch."""
        return self._run(list(cs), list(excitations))

    # ------------------------------------------------------------------ excitation from f0
    @staticmethod
    def _check_sine_args(sampling_rate, layout):
        if layout not in _lib.PWG_SINE_LAYOUTS:
            raise ValueError(f"layout must be 'tile' or 'hold', got {layout!r}")
        if not sampling_rate > 0:
            raise ValueError(f"sampling_rate must be positive, got {sampling_rate}")

    def _sine_frames(self, f0s, sampling_rate, layout, noises, generator, dev):
        """One pwg_sine_frames launch over the ragged batch: the packed excitation rows (sum T_u * hop,)
        ``_excite`` reads, on the device, and the frames per utterance. SineGen's defaults, as the
        reference's preprocessing uses them: one channel, sine_amp 0.1, noise_std 0.003, threshold 0."""
        from . import sinegen

        f0s = [torch.as_tensor(f, dtype=torch.float32).to(dev).reshape(-1) for f in f0s]
        if not f0s:
            raise ValueError("one f0 contour per utterance is required")
        hop = self.upsample_factor
        frames = [int(f.numel()) for f in f0s]
        starts = np.zeros(len(frames) + 1, np.int64)
        np.cumsum(frames, out=starts[1:])
        rows = int(starts[-1]) * hop
        if noises is None:
            n = torch.randn(rows, device=dev, generator=generator)
        else:
            if len(noises) != len(f0s):
                raise ValueError("one noise signal per utterance is required")
            noises = [torch.as_tensor(z, dtype=torch.float32).to(dev).reshape(-1) for z in noises]
            for z, t in zip(noises, frames):
                if z.numel() != t * hop:
                    raise ValueError(f"noise has {z.numel()} samples, expected T * prod(upsample_scales) = {t * hop}")
            n = torch.cat(noises) if len(noises) > 1 else noises[0].contiguous()
        f0 = torch.cat(f0s) if len(f0s) > 1 else f0s[0].contiguous()
        exc = torch.empty(rows, dtype=torch.float32, device=dev)
        flag = sinegen.sine_call("pwg_sine_frames", dev, f0, torch.from_numpy(starts).to(dev), len(frames),
                                 int(starts[-1]), (hop, _lib.PWG_SINE_LAYOUTS[layout]), float(sampling_rate), 1, 0.1,
                                 0.003, 0.0, None, n, exc, None, None)
        sinegen.check_flag(flag)
        return exc, frames

    def excitation_from_f0(self, f0s, sampling_rate, layout="tile", noise=None, generator=None):
        """Frame-rate f0 contours (list of (T_u,)) -> list of (T_u * hop,) excitation signals on the
        device, what the reference dumps as ``*-excitation.npy``. layout "tile" repeats the whole
        contour hop times (ext[i] = f0[i % T], what the reference's preprocessing builds and shipped
        checkpoints were trained on), "hold" holds every frame for hop samples (ext[i] = f0[i // hop]).
        noise: list of (T_u * hop,) standard-normal draws; otherwise drawn on the device with
        ``generator`` (a stream that differs from CPU torch's)."""
        self._check_sine_args(sampling_rate, layout)
        exc, frames = self._sine_frames(list(f0s), sampling_rate, layout, noise, generator, self._device())
        return list(torch.split(exc, [t * self.upsample_factor for t in frames]))

    def inference_from_f0(self, f0, c, sampling_rate, layout="tile", noise=None):
        """``inference`` with the excitation generated from f0 (T,) on the GPU: c (T, in_channels) ->
        (T * hop, out_channels)."""
        return self.inference_batch_from_f0([c], [f0], sampling_rate, layout, None if noise is None else [noise])[0]

    def inference_batch_from_f0(self, cs, f0s, sampling_rate, layout="tile", noises=None):
        """``inference_batch`` with the excitations generated from the f0 contours: one pwg_sine_frames
        launch writes the packed rows the front end reads (no host round trip)."""
        self._check_sine_args(sampling_rate, layout)
        dev = self._device()
        cs, f0s = list(cs), list(f0s)
        if len(cs) != len(f0s) or not cs:
            raise ValueError("one f0 contour per utterance is required")
        cs = [torch.as_tensor(c, dtype=torch.float32).to(dev).contiguous() for c in cs]
        for c, f in zip(cs, f0s):
            if c.dim() != 2 or c.size(1) != self.in_channels:
                raise ValueError(f"c must be (T, {self.in_channels})")
            if int(np.prod(np.shape(f))) != c.size(0):
                raise ValueError(f"f0 has {int(np.prod(np.shape(f)))} frames, c has {c.size(0)}")
        exc, _ = self._sine_frames(f0s, sampling_rate, layout, noises, None, dev)
        return self._run_packed(cs, exc)
