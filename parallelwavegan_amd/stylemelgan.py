"""Drop-in ``StyleMelGANGenerator`` (parallel_wavegan/models/style_melgan.py:18-240 with the
TADEResBlock of layers/tade_res_block.py) on the MI355X TADE kernels (include/pwg_smg.h,
csrc/pwg_smg.hip).

Same constructor arguments, defaults, submodule names and state-dict keys as the reference class
(noise_upsample.{0,2,..}, blocks.i.tade{1,2}.aux_conv.0 / .gated_conv.0, blocks.i.gated_conv{1,2},
output_conv.0; weight_g / weight_v under weight norm), so a reference checkpoint loads with
``strict=True``. The modules only hold the parameters: the forward is one pwg_smg_run over the whole
(ragged) batch, every utterance with its own instance-norm statistics.

Refused (NotImplementedError): upsample_mode other than "nearest", a noise activation other than
LeakyReLU, channels not a multiple of 16 or above 64, aux_channels not a multiple of 16 or above 128,
even kernel sizes and kernel sizes above 11. There is no exact-fp32 mode: a run whose values leave the
fp16 pair range of the split-f16 conv kernels raises FloatingPointError.
"""

import ctypes
import logging

import numpy as np
import torch

from . import _lib
from .engine import WeightTracker, first_parameter, fold_weight_norm, forget_device


class TADELayer(torch.nn.Module):
    """Parameter holder of layers/tade_res_block.py:11-72 (the instance norm and the upsampling hold
    no state)."""

    def __init__(self, in_channels=64, aux_channels=80, kernel_size=9, bias=True, upsample_factor=2,
                 upsample_mode="nearest"):
        super().__init__()
        pad = (kernel_size - 1) // 2
        self.aux_conv = torch.nn.Sequential(
            torch.nn.Conv1d(aux_channels, in_channels, kernel_size, 1, bias=bias, padding=pad))
        self.gated_conv = torch.nn.Sequential(
            torch.nn.Conv1d(in_channels, in_channels * 2, kernel_size, 1, bias=bias, padding=pad))


class TADEResBlock(torch.nn.Module):
    """Parameter holder of layers/tade_res_block.py:75-160."""

    def __init__(self, in_channels=64, aux_channels=80, kernel_size=9, dilation=2, bias=True, upsample_factor=2,
                 upsample_mode="nearest", gated_function="softmax"):
        super().__init__()
        pad = (kernel_size - 1) // 2
        self.tade1 = TADELayer(in_channels, aux_channels, kernel_size, bias, 1, upsample_mode)
        self.gated_conv1 = torch.nn.Conv1d(in_channels, in_channels * 2, kernel_size, 1, bias=bias, padding=pad)
        self.tade2 = TADELayer(in_channels, in_channels, kernel_size, bias, upsample_factor, upsample_mode)
        self.gated_conv2 = torch.nn.Conv1d(in_channels, in_channels * 2, kernel_size, 1, bias=bias, dilation=dilation,
                                           padding=pad * dilation)
        if gated_function not in _lib.PWG_SMG_GATES:
            raise ValueError(f"{gated_function} is not supported.")


def make_smg_config(in_channels, aux_channels, channels, out_channels, kernel_size, dilation, bias,
                    noise_upsample_scales, noise_slope, upsample_scales, gated_function):
    cfg = _lib.PwgSmgConfig()
    cfg.in_channels, cfg.aux_channels, cfg.channels, cfg.out_channels = in_channels, aux_channels, channels, out_channels
    cfg.kernel_size, cfg.dilation, cfg.bias = kernel_size, dilation, int(bool(bias))
    cfg.gate = _lib.PWG_SMG_GATES[gated_function]
    cfg.noise_slope = float(noise_slope)
    if max(len(noise_upsample_scales), len(upsample_scales)) > _lib.PWG_SMG_MAX_SCALES:
        raise NotImplementedError(f"more than {_lib.PWG_SMG_MAX_SCALES} scales")
    cfg.num_noise_scales = len(noise_upsample_scales)
    for i, s in enumerate(noise_upsample_scales):
        cfg.noise_scales[i] = int(s)
    cfg.num_scales = len(upsample_scales)
    for i, s in enumerate(upsample_scales):
        cfg.upsample_scales[i] = int(s)
    return cfg


class SmgPlan:
    """pwg_smg_plan_*: the ragged batch's layout (host only). flags None: pwg_smg_plan_create; an int:
    pwg_smg_plan_create_ex (``_lib.PWG_SMG_PLAN_TRIM_NOISE``: the token class's trimmed layout)."""

    def __init__(self, handle, frames, noise_len, flags=None):
        self.handle = handle  # keeps the PwgSmg alive
        self.flags = flags
        self.frames = [int(f) for f in frames]
        self.noise_len = [int(n) for n in noise_len]
        n = len(self.frames)
        if n != len(self.noise_len):
            raise ValueError("frames and noise_len need one entry per utterance")
        ll = ctypes.c_longlong * n
        self._p = ctypes.c_void_p()
        self._lib = _lib.load()
        if flags is None:
            _lib.check(self._lib.pwg_smg_plan_create(handle._h, n, ll(*self.frames), ll(*self.noise_len),
                                                     ctypes.byref(self._p)))
        else:
            _lib.check(self._lib.pwg_smg_plan_create_ex(handle._h, n, ll(*self.frames), ll(*self.noise_len), int(flags),
                                                        ctypes.byref(self._p)))
        self.workspace_bytes = int(self._lib.pwg_smg_plan_workspace_bytes(self._p))
        self.out_rows = int(self._lib.pwg_smg_plan_out_rows(self._p))

    def tensor(self, block, which):
        """(offset_bytes, rows, ld) of a block's tensor in the workspace (pwg_smg_plan_tensor)."""
        off, rows, ld = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
        _lib.check(self._lib.pwg_smg_plan_tensor(self._p, block, which, ctypes.byref(off), ctypes.byref(rows),
                                                 ctypes.byref(ld)))
        return off.value, rows.value, ld.value

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.pwg_smg_plan_destroy(self._p)
            self._p = None


class SmgHandle:
    """pwg_smg_create and what hangs off it. device None: host only (counts, packing, plans)."""

    def __init__(self, cfg, conv_names, device=None):
        self._lib = _lib.load()
        self.cfg = cfg
        self.conv_names = list(conv_names)
        self.device = device
        self._h = ctypes.c_void_p()
        index = -1 if device is None else (device.index if device.index is not None else torch.cuda.current_device())
        _lib.check(self._lib.pwg_smg_create(ctypes.byref(cfg), index, ctypes.byref(self._h)))
        self.ref_weight_count = int(self._lib.pwg_smg_ref_weight_count(self._h))
        self.packed_weight_count = int(self._lib.pwg_smg_packed_weight_count(self._h))
        self.packed = None
        self._ws = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.pwg_smg_destroy(self._h)
            self._h = None

    def flatten_state_dict(self, state):
        """State dict (weight norm folded or not) -> the reference order of include/pwg_smg.h."""
        folded = fold_weight_norm(state)
        parts = []
        for name in self.conv_names:
            parts.append(np.ascontiguousarray(folded[name + ".weight"], np.float32).reshape(-1))
            if self.cfg.bias:
                parts.append(np.ascontiguousarray(folded[name + ".bias"], np.float32).reshape(-1))
        flat = np.concatenate(parts)
        if flat.size != self.ref_weight_count:
            raise ValueError(f"state dict holds {flat.size} weights, the generator {self.ref_weight_count}")
        return flat

    def pack(self, state):
        """Packed image (host ndarray); RangeError when a weight leaves the fp16 pair range."""
        flat = self.flatten_state_dict(state)
        packed = np.empty(self.packed_weight_count, np.float32)
        _lib.check(self._lib.pwg_smg_pack_weights(self._h, flat.ctypes.data, packed.ctypes.data))
        return packed

    def load_state_dict(self, state):
        self.packed = torch.from_numpy(self.pack(state)).to(self.device)

    def plan(self, frames, noise_len, flags=None):
        return SmgPlan(self, frames, noise_len, flags)

    def workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def release_workspace(self):
        self._ws = None

    def set_timing(self, on):
        _lib.check(self._lib.pwg_smg_set_timing(self._h, int(bool(on))))

    def collect_timing(self):
        ms = (ctypes.c_double * len(_lib.PWG_SMG_KINDS))()
        _lib.check(self._lib.pwg_smg_timing_collect(self._h, ms))
        return dict(zip(_lib.PWG_SMG_KINDS, ms))

    def run(self, plan, c, z, out, mean=None, scale=None, check=True):
        """c (sum frames, aux), z (sum noise_len, in_channels), out (plan.out_rows, out_channels):
        contiguous fp32 tensors on the device. Returns the workspace tensor."""
        ws = self.workspace(plan.workspace_bytes)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.pwg_smg_run(plan._p, self.packed.data_ptr(), c.data_ptr(),
                                         mean.data_ptr() if mean is not None else None,
                                         scale.data_ptr() if scale is not None else None, z.data_ptr(),
                                         out.data_ptr(), ws.data_ptr(), stream))
        if check:
            self._status(plan, ws, stream)
        return ws

    def _status(self, plan, ws, stream):
        rc = self._lib.pwg_smg_run_status(plan._p, ws.data_ptr(), stream)
        if rc == _lib.PWG_ERR_RANGE:
            msg = self._lib.pwg_last_error().decode(errors="replace")
            # (include/pwg_smg.h: an id outside its table, reported ahead of a non-finite sample)
            raise (ValueError if msg.startswith("bad ") else FloatingPointError)(msg)
        _lib.check(rc)

    def run_tokens(self, plan, emb, spk, ids, spk_ids, z, out, check=True):
        """pwg_smg_run_tokens on a trimmed plan. emb (num_embs, aux), spk (num_spk, aux): contiguous fp32;
        ids (sum frames,), spk_ids (n_utts,): contiguous int64; z, out as ``run``; all on the device.
        Returns the workspace tensor. An id outside its table raises ValueError."""
        for t, dt in ((emb, torch.float32), (spk, torch.float32), (ids, torch.int64), (spk_ids, torch.int64)):
            assert t.is_contiguous() and t.dtype == dt and t.device == self.packed.device
        assert ids.numel() == sum(plan.frames) and spk_ids.numel() == len(plan.frames)
        assert emb.shape[1] == spk.shape[1] == self.cfg.aux_channels
        ws = self.workspace(plan.workspace_bytes)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.pwg_smg_run_tokens(plan._p, self.packed.data_ptr(), emb.data_ptr(), emb.shape[0],
                                                spk.data_ptr(), spk.shape[0], ids.data_ptr(), spk_ids.data_ptr(),
                                                z.data_ptr(), out.data_ptr(), ws.data_ptr(), stream))
        if check:
            self._status(plan, ws, stream)
        return ws


def debug_stats(x, rows_per_utt):
    """pwg_smg_debug_stats: (mean, rstd), each (n_utts, channels), of the utterances stacked in the
    device tensor x (sum rows, channels)."""
    lib = _lib.load()
    n, ch = len(rows_per_utt), x.shape[1]
    assert x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == sum(rows_per_utt)
    nbytes = (16 * n + 2 * ch * (x.shape[0] // _lib.PWG_SMG_STATS_TILE + n + 1)) * 4 + 512
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    mean = torch.empty(n, ch, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    with torch.cuda.device(x.device):
        _lib.check(lib.pwg_smg_debug_stats(x.data_ptr(), ch, ch, (ctypes.c_longlong * n)(*rows_per_utt), n,
                                           mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(),
                                           torch.cuda.current_stream(x.device).cuda_stream))
        torch.cuda.current_stream(x.device).synchronize()
    return mean, rstd


class StyleMelGANGenerator(torch.nn.Module):
    """models/style_melgan.py:18-240, executed on the MI355X TADE kernels."""

    def __init__(self, in_channels=128, aux_channels=80, channels=64, out_channels=1, kernel_size=9, dilation=2,
                 bias=True, noise_upsample_scales=[11, 2, 2, 2], noise_upsample_activation="LeakyReLU",
                 noise_upsample_activation_params={"negative_slope": 0.2},
                 upsample_scales=[2, 2, 2, 2, 2, 2, 2, 2, 1], upsample_mode="nearest", gated_function="softmax",
                 use_weight_norm=True):
        super().__init__()
        if upsample_mode != "nearest":
            raise NotImplementedError(f"upsample_mode {upsample_mode!r}: only nearest-neighbour repetition is accelerated")
        if noise_upsample_activation != "LeakyReLU":
            raise NotImplementedError(f"noise_upsample_activation {noise_upsample_activation!r}: only LeakyReLU is accelerated")
        if channels % 16 or not 16 <= channels <= 64:
            raise NotImplementedError(f"channels {channels}: a multiple of 16 up to 64 is required")
        if aux_channels % 16 or not 16 <= aux_channels <= 128:
            raise NotImplementedError(f"aux_channels {aux_channels}: a multiple of 16 up to 128 is required")
        if kernel_size % 2 == 0 or not 1 <= kernel_size <= 11:
            raise NotImplementedError(f"kernel_size {kernel_size}: an odd size up to 11 is required")
        self.in_channels = in_channels
        self.aux_channels = aux_channels
        self.out_channels = out_channels
        noise_upsample = []
        in_chs = in_channels
        for s in noise_upsample_scales:
            noise_upsample += [
                torch.nn.ConvTranspose1d(in_chs, channels, s * 2, stride=s, padding=s // 2 + s % 2,
                                         output_padding=s % 2, bias=bias),
                getattr(torch.nn, noise_upsample_activation)(**noise_upsample_activation_params),
            ]
            in_chs = channels
        self.noise_upsample = torch.nn.Sequential(*noise_upsample)
        self.noise_upsample_factor = np.prod(noise_upsample_scales)
        self.blocks = torch.nn.ModuleList()
        aux_chs = aux_channels
        for s in upsample_scales:
            self.blocks += [TADEResBlock(channels, aux_chs, kernel_size, dilation, bias, s, upsample_mode, gated_function)]
            aux_chs = channels
        self.upsample_factor = np.prod(upsample_scales)
        self.output_conv = torch.nn.Sequential(
            torch.nn.Conv1d(channels, out_channels, kernel_size, 1, bias=bias, padding=(kernel_size - 1) // 2),
            torch.nn.Tanh(),
        )
        self._cfg = make_smg_config(in_channels, aux_channels, channels, out_channels, kernel_size, dilation, bias,
                                    list(noise_upsample_scales),
                                    dict(noise_upsample_activation_params).get("negative_slope", 0.01),
                                    list(upsample_scales), gated_function)
        self._conv_names = [f"noise_upsample.{2 * i}" for i in range(len(noise_upsample_scales))]
        for i in range(len(upsample_scales)):
            self._conv_names += [f"blocks.{i}.{n}" for n in ("tade1.aux_conv.0", "tade1.gated_conv.0", "gated_conv1",
                                                            "tade2.aux_conv.0", "tade2.gated_conv.0", "gated_conv2")]
        self._conv_names.append("output_conv.0")
        if use_weight_norm:
            self.apply_weight_norm()
        self.reset_parameters()
        self._engine = None
        self._weights = WeightTracker()
        self._plans = {}

    # ------------------------------------------------------------------ reference housekeeping
    def remove_weight_norm(self):
        """models/style_melgan.py:145-155."""
        def _remove(m):
            try:
                torch.nn.utils.remove_weight_norm(m)
            except ValueError:
                return
        self.apply(_remove)

    def apply_weight_norm(self):
        """models/style_melgan.py:157-167."""
        def _apply(m):
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)):
                torch.nn.utils.weight_norm(m)
        self.apply(_apply)

    def reset_parameters(self):
        """models/style_melgan.py:169-179: conv weights ~ N(0, 0.02)."""
        def _reset(m):
            if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)):
                m.weight.data.normal_(0.0, 0.02)
        self.apply(_reset)

    def register_stats(self, stats):
        """models/style_melgan.py:181-197 (.npy; .h5 needs h5py)."""
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

    def _apply(self, fn, *args, **kwargs):
        forget_device(self)
        self._weights.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def invalidate_weights(self):
        """After an in-place write through ``param.data`` (see engine.WeightTracker)."""
        self._weights.invalidate()

    # ------------------------------------------------------------------ engine plumbing
    def _device(self):
        dev = first_parameter(self).device
        if dev.type != "cuda":
            raise RuntimeError("parallelwavegan_amd.StyleMelGANGenerator runs on a ROCm GPU only; move the module "
                               "with .to('cuda') (there is no CPU fallback)")
        return dev

    def host_handle(self):
        """A host-only SmgHandle (weight counts, packing, plans) of this generator."""
        return SmgHandle(self._cfg, self._conv_names, None)

    def engine(self):
        dev = self._device()
        if self._engine is None or self._engine.device != dev:
            self._engine = SmgHandle(self._cfg, self._conv_names, dev)
            self._plans = {}
            self._weights.invalidate()
        if self._weights.changed(self):
            with torch.no_grad():
                state = {k: v for k, v in self.state_dict().items() if k not in ("mean", "scale")}
                self._engine.load_state_dict(state)
            self._weights.mark_packed()
        return self._engine

    def _plan(self, eng, frames, noise_len):
        key = (tuple(frames), tuple(noise_len))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 16:
                self._plans.clear()
            plan = self._plans[key] = eng.plan(frames, noise_len)
        return plan

    @staticmethod
    def _rows(x, dev):
        """array or tensor (rows, channels) -> contiguous fp32 device tensor."""
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), np.float32))
        return x.detach().to(dev, torch.float32).contiguous()

    def _run(self, cs, zs, normalize_before=False, keep=None):
        """cs: per utterance (T, aux); zs: per utterance (Lz, in_channels) or None (drawn here).
        Returns the per-utterance outputs (T * upsample_factor, out_channels). keep: a dict that
        receives the plan and the workspace (tests)."""
        eng = self.engine()
        dev = eng.device
        nf = int(self.noise_upsample_factor)
        cs = [self._rows(c, dev) for c in cs]
        for c in cs:
            if c.dim() != 2 or c.shape[1] != self.aux_channels:
                raise ValueError(f"c must be (T, {self.aux_channels})")
            if c.shape[0] < 1:
                raise ValueError("every utterance needs at least one frame")
        frames = [int(c.shape[0]) for c in cs]
        if zs is None:
            zs = [torch.randn((f - 1) // nf + 1, self.in_channels, dtype=torch.float32, device=dev) for f in frames]
        else:
            zs = [self._rows(z, dev) for z in zs]
        if len(zs) != len(cs):
            raise ValueError("one noise tensor per utterance")
        for z in zs:
            if z.dim() != 2 or z.shape[1] != self.in_channels or z.shape[0] < 1:
                raise ValueError(f"z must be (Lz, {self.in_channels})")
        noise_len = [int(z.shape[0]) for z in zs]
        plan = self._plan(eng, frames, noise_len)
        mean = scale = None
        if normalize_before:
            mean = self.mean.detach().to(dev, torch.float32).contiguous()
            scale = self.scale.detach().to(dev, torch.float32).contiguous()
        hop = int(self.upsample_factor)
        with torch.cuda.device(dev):
            c_all = cs[0] if len(cs) == 1 else torch.cat(cs, 0)
            z_all = zs[0] if len(zs) == 1 else torch.cat(zs, 0)
            out = torch.empty(plan.out_rows, self.out_channels, dtype=torch.float32, device=dev)
            ws = eng.run(plan, c_all, z_all, out, mean, scale, check=True)
        if keep is not None:
            keep.update(plan=plan, workspace=ws)
        outs, o = [], 0
        for f in frames:
            outs.append(out[o:o + f * hop])
            o += f * hop
        return outs

    # ------------------------------------------------------------------ reference API
    def forward(self, c, z=None):
        """models/style_melgan.py:123-143: c (B, aux_channels, Tc), z (B, in_channels, Lz) ->
        (B, out_channels, Tc * upsample_factor). Tc must equal Lz * noise_upsample_factor (the
        reference fails on the shape mismatch inside the first block); z=None draws Lz = 1 as the
        reference does."""
        dev = self._device()
        if not torch.is_tensor(c):
            c = torch.from_numpy(np.asarray(c, np.float32))
        if c.dim() != 3:
            raise ValueError("forward expects c (B, aux_channels, T)")
        if z is None:
            z = torch.randn(c.size(0), self.in_channels, 1, device=dev)
        elif not torch.is_tensor(z):
            z = torch.from_numpy(np.asarray(z, np.float32))
        assert z.dim() == 3 and z.size(0) == c.size(0)
        assert c.size(2) == z.size(2) * int(self.noise_upsample_factor), \
            "c needs noise length * noise_upsample_factor frames"
        cs = [c[b].transpose(0, 1) for b in range(c.size(0))]
        zs = [z[b].transpose(0, 1) for b in range(z.size(0))]
        return torch.stack([o.transpose(0, 1) for o in self._run(cs, zs)], 0)

    def inference(self, c, normalize_before=False, z=None):
        """models/style_melgan.py:199-240: c (T, aux_channels) -> (T * upsample_factor,
        out_channels). ``z`` (1, in_channels, Lz) or (in_channels, Lz), Lz = (T - 1) //
        noise_upsample_factor + 1, makes a run reproducible (an extension; the reference always
        draws it)."""
        return self.inference_batch([c], normalize_before, None if z is None else [z])[0]

    def inference_batch(self, cs, normalize_before=False, zs=None):
        """Ragged list form of ``inference``: the whole batch is one plan, every utterance keeps its
        own instance-norm statistics."""
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
        return self._run(list(cs), zs, normalize_before)
