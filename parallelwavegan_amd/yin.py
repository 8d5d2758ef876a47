"""YIN f0 estimation on the HIP kernel (include/pwg_yin.h): waveform in, the frame-rate f0 contour that
``UHiFiGANGenerator.inference_batch_from_f0``, the decode CLI's ``--excitation-from-f0`` and the f0-conditioned
token vocoders read out.

* ``yin_estimate``: the signature of ``torchyin.estimate`` (Hz, 0 where unvoiced).
* ``f0_torchyin``: drop-in for parallel_wavegan/bin/preprocess.py:f0_torchyin (ndarray in, log-f0 ndarray out).
* ``YinF0Extractor``: a ragged batch of waveforms to a list of contours, optionally fitted to given frame
  counts (the mel lengths) by a cut or an edge hold.

The estimator is defined in closed form in include/pwg_yin.h and DESIGN.md 3.11. The ``torchyin`` package
itself was not available to compare with: agreement with it is unverified.
"""

import ctypes

import numpy as np
import torch

from . import _lib

_NO_CPU = "YIN f0 extraction runs on a ROCm GPU only (there is no CPU fallback)"


def lag_bounds(sample_rate, pitch_min, pitch_max):
    """(tau_min, tau_max) = (int(sample_rate / pitch_max), int(sample_rate / pitch_min))."""
    if not pitch_min > 0 or not pitch_max > 0:
        raise ValueError("pitch_min and pitch_max must be positive")
    return int(sample_rate / pitch_max), int(sample_rate / pitch_min)


def _check_geometry(tau_min, tau_max, hop, threshold):
    """The plan's checks, raised before a device is needed."""
    if hop < 1:
        raise ValueError(f"hop must be >= 1, got {hop}")
    if tau_max - 1 - tau_min < 1:
        raise ValueError(f"no lag to search: tau_min = {tau_min}, tau_max = {tau_max} (pitch_min must be well below "
                         "pitch_max and the sampling rate)")
    if not (threshold > 0 and np.isfinite(threshold)):
        raise ValueError(f"threshold must be finite and positive, got {threshold}")
    if tau_max > _lib.PWG_YIN_MAX_TAU:
        raise NotImplementedError(f"tau_max = {tau_max} is above {_lib.PWG_YIN_MAX_TAU}: raise pitch_min")


class YinPlan:
    """A pwg_yin plan on one device."""

    def __init__(self, device, fs, tau_min, tau_max, hop, threshold=0.1, log_f0=False):
        L = _lib.load()
        self.device, self.tau_min, self.tau_max, self.hop = torch.device(device), int(tau_min), int(tau_max), int(hop)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.pwg_yin_plan_create(ctypes.c_float(fs), int(tau_min), int(tau_max), int(hop),
                                             ctypes.c_float(threshold), int(bool(log_f0)), ctypes.byref(h)))
        self._h, self._destroy = h, L.pwg_yin_plan_destroy

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def frames(self, n_samples):
        W = 2 * self.tau_max
        return 1 if n_samples < W else 1 + (int(n_samples) - W) // self.hop

    def run(self, wave, lengths, out_frames=None, want_tau=False, want_cmdf=False):
        """wave: packed fp32 device tensor of sum(lengths) samples -> (f0, tau or None, cmdf or None) device
        tensors of sum(rows) rows on the current stream; rows = out_frames, or each utterance's own frames."""
        L = _lib.load()
        n = len(lengths)
        starts = (ctypes.c_longlong * (n + 1))()
        for i, t in enumerate(lengths):
            starts[i + 1] = starts[i] + int(t)
        if out_frames is None:
            rows, frames_arg = sum(self.frames(int(t)) for t in lengths), None
        else:
            if len(out_frames) != n:
                raise ValueError("out_frames must hold one row count per utterance")
            rows, frames_arg = sum(int(r) for r in out_frames), (ctypes.c_longlong * n)(*[int(r) for r in out_frames])
        f0 = torch.empty(rows, dtype=torch.float32, device=self.device)
        tau = torch.empty(rows, dtype=torch.int32, device=self.device) if want_tau else None
        cmdf = (torch.empty(rows, self.tau_max - 1 - self.tau_min, dtype=torch.float32, device=self.device)
                if want_cmdf else None)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(L.pwg_yin_run(self._h, wave.data_ptr(), starts, n, frames_arg, f0.data_ptr(), ptr(tau), ptr(cmdf),
                                     rows, stream))
        return f0, tau, cmdf


class YinF0Extractor:
    """Waveforms to f0 contours on the GPU, over ragged batches: the reference's
    ``f0_torchyin(audio, sampling_rate, hop_size, frame_length)`` with the plan kept.

    frame_length: when given, pitch_min = sampling_rate / (frame_length / 2), as the reference sets it (the
    recipes pass win_length). log: natural log of the voiced values, zeros kept (what f0_torchyin returns)."""

    def __init__(self, sampling_rate, hop_size, frame_length=None, pitch_min=40, pitch_max=10000, threshold=0.1,
                 log=True):
        if frame_length is not None:
            pitch_min = sampling_rate / (frame_length / 2)
        self.sampling_rate, self.hop_size, self.frame_length = sampling_rate, int(hop_size), frame_length
        self.pitch_min, self.pitch_max, self.threshold, self.log = pitch_min, pitch_max, float(threshold), bool(log)
        self.tau_min, self.tau_max = lag_bounds(sampling_rate, pitch_min, pitch_max)
        _check_geometry(self.tau_min, self.tau_max, self.hop_size, self.threshold)
        self._plans = {}

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"] = {}  # C handles: a copy builds its own
        return state

    @classmethod
    def from_config(cls, config, **kwargs):
        """From a recipe's config dict: sampling_rate, hop_size and win_length (as frame_length), which is
        the reference's call in bin/preprocess.py:421-426."""
        return cls(config["sampling_rate"], config["hop_size"], frame_length=config["win_length"], **kwargs)

    def frames(self, n_samples):
        W = 2 * self.tau_max
        return 1 if n_samples < W else 1 + (int(n_samples) - W) // self.hop_size

    def plan(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._plans:
            self._plans[device] = YinPlan(device, self.sampling_rate, self.tau_min, self.tau_max, self.hop_size,
                                          self.threshold, self.log)
        return self._plans[device]

    def extract_batch(self, waves, frames=None, device=None):
        """waves: a list of (T_u,) or (T_u, 1) tensors or arrays -> a list of (frames_u,) device tensors, views
        of one buffer, from one launch sequence. frames: per utterance the rows wanted (the mel lengths): a
        longer contour is cut, a shorter one holds its last value; None gives each utterance's own frames."""
        if len(waves) == 0:
            return []
        flat = []
        for w in waves:
            w = torch.as_tensor(w) if not isinstance(w, torch.Tensor) else w.detach()
            if w.dim() == 2 and w.size(1) == 1:
                w = w.reshape(-1)
            if w.dim() != 1:
                raise ValueError("each waveform must be (T,) or (T, 1)")
            if w.numel() == 0:
                raise ValueError("an empty waveform has no frame")
            flat.append(w)
        if frames is not None:
            frames = [int(f) for f in frames]
            if len(frames) != len(flat) or min(frames) < 1:
                raise ValueError("frames must hold one count >= 1 per waveform")
        if device is None:
            on_gpu = [w.device for w in flat if w.device.type == "cuda"]
            if not on_gpu and not torch.cuda.is_available():
                raise RuntimeError(_NO_CPU)
            device = on_gpu[0] if on_gpu else torch.device("cuda", torch.cuda.current_device())
        plan = self.plan(device)
        lengths = [int(w.numel()) for w in flat]
        with torch.no_grad():
            if len(flat) == 1:
                packed = flat[0].to(device=plan.device, dtype=torch.float32).contiguous()
            else:
                packed = torch.cat([w.to(device=plan.device, dtype=torch.float32) for w in flat])
            f0, _, _ = plan.run(packed, lengths, frames)
        rows = frames if frames is not None else [self.frames(t) for t in lengths]
        return list(torch.split(f0, rows))

    def extract(self, wave, frames=None, device=None):
        return self.extract_batch([wave], None if frames is None else [frames], device)[0]


def yin_estimate(signal, sample_rate, pitch_min=20, pitch_max=20000, frame_stride=0.01, threshold=0.1):
    """``torchyin.estimate``'s signature on the HIP kernel: signal (T,) or (B, T) device tensor -> f0 in Hz,
    (frames,) or (B, frames), 0 where unvoiced. The hop is int(frame_stride * sample_rate)."""
    if not isinstance(signal, torch.Tensor):
        raise TypeError("signal must be a torch.Tensor")
    if signal.dim() not in (1, 2):
        raise ValueError("signal must be (T,) or (B, T)")
    if signal.device.type != "cuda":
        raise RuntimeError(_NO_CPU)
    tau_min, tau_max = lag_bounds(sample_rate, pitch_min, pitch_max)
    hop = int(frame_stride * sample_rate)
    _check_geometry(tau_min, tau_max, hop, threshold)
    x = signal.detach().to(torch.float32).contiguous()
    B, T = (1, x.numel()) if x.dim() == 1 else x.shape
    if T < 1:
        raise ValueError("an empty signal has no frame")
    plan = YinPlan(x.device, sample_rate, tau_min, tau_max, hop, threshold, False)
    with torch.no_grad():
        f0, _, _ = plan.run(x.view(-1), [T] * B)
    return f0 if signal.dim() == 1 else f0.view(B, -1)


def f0_torchyin(audio, sampling_rate, hop_size=256, frame_length=None, pitch_min=40, pitch_max=10000):
    """bin/preprocess.py:f0_torchyin on the GPU: audio (T,) ndarray -> log f0 (frames,) float32 ndarray,
    0 where unvoiced."""
    ex = YinF0Extractor(sampling_rate, hop_size, frame_length, pitch_min, pitch_max)
    return ex.extract(np.asarray(audio, np.float32)).cpu().numpy()
