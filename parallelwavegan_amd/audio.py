"""Audio conditioning on the HIP kernels (include/pwg_wave.h): what the reference's preprocess does to a
waveform before any feature is taken (parallel_wavegan/bin/preprocess.py:359-452).

* ``trim_silence``: ``librosa.effects.trim``'s call shape (ndarray in, ``(audio[start:end], [start, end])`` out).
* ``resample_poly`` / ``resample``: a polyphase rational resampler with ``scipy.signal.resample_poly``'s
  zero-padded form and its default Kaiser low-pass (``kaiser_lowpass_taps``).
* ``AudioConditioner``: ragged batches of trim, resample and fit (cut of a range, edge pad to a length, gain
  and clipping peak), built from a recipe's config.

The closed forms are in include/pwg_wave.h and DESIGN.md 3.12.
"""

import ctypes
import math

import numpy as np
import torch

from . import _lib

_NO_CPU = "audio conditioning runs on a ROCm GPU only (there is no CPU fallback)"


def kaiser_lowpass_taps(up, down, zeros=10, beta=5.0):
    """``scipy.signal.resample_poly``'s default filter, ``firwin(2 half + 1, 1 / max, window=("kaiser", beta))
    * up`` with ``half = zeros * max(up, down)``, restated in NumPy float64: (2 half + 1,) float64. up and
    down are reduced by their gcd first, as scipy does."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("up and down must be >= 1")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    mx = max(up, down)
    half = int(zeros) * mx
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = (1.0 / mx) * np.sinc(k / mx) * np.kaiser(2 * half + 1, beta)
    return h / h.sum() * up


def resample_out_len(n_samples, up, down):
    """ceil(n_samples up / down) with up / down reduced."""
    g = math.gcd(int(up), int(down))
    return -(-int(n_samples) * (int(up) // g) // (int(down) // g))


def trim_frames(n_samples, frame_length, hop_length):
    """1 + (T + 2 (fl // 2) - fl) // hop: the frames librosa's centred rms gives."""
    return 1 + (int(n_samples) + 2 * (frame_length // 2) - frame_length) // hop_length


def _starts(lengths):
    s = (ctypes.c_longlong * (len(lengths) + 1))()
    for i, t in enumerate(lengths):
        s[i + 1] = s[i] + int(t)
    return s


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class TrimPlan:
    """A pwg_trim plan on one device."""

    def __init__(self, device, frame_length, hop_length, top_db, pad_mode="constant"):
        if pad_mode not in _lib.PWG_TRIM_PAD_MODES:
            raise ValueError(f"pad_mode must be one of {sorted(_lib.PWG_TRIM_PAD_MODES)}, got {pad_mode!r}")
        L = _lib.load()
        self.device, self.frame_length, self.hop_length = torch.device(device), int(frame_length), int(hop_length)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.pwg_trim_plan_create(self.frame_length, self.hop_length, ctypes.c_float(top_db),
                                              _lib.PWG_TRIM_PAD_MODES[pad_mode], ctypes.byref(h)))
        self._h, self._destroy = h, L.pwg_trim_plan_destroy

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def run(self, wave, lengths, want_power=True):
        """wave: packed fp32 device tensor of sum(lengths) samples -> (bounds (n, 2) int64 device tensor,
        power (sum of frames,) fp32 device tensor or None) on the current stream."""
        L = _lib.load()
        n = len(lengths)
        rows = sum(trim_frames(t, self.frame_length, self.hop_length) for t in lengths)
        bounds = torch.empty(n, 2, dtype=torch.int64, device=self.device)
        power = torch.empty(rows, dtype=torch.float32, device=self.device) if want_power else None
        with torch.cuda.device(self.device):
            _lib.check(L.pwg_trim_run(self._h, wave.data_ptr(), _starts(lengths), n, bounds.data_ptr(),
                                      power.data_ptr() if want_power else None, rows, _stream(self.device)))
        return bounds, power


class ResamplePlan:
    """A pwg_resample plan on one device; taps default to ``kaiser_lowpass_taps(up, down)``."""

    def __init__(self, device, up, down, taps=None):
        L = _lib.load()
        g = math.gcd(int(up), int(down))
        self.device, self.up, self.down = torch.device(device), int(up) // g, int(down) // g
        taps = kaiser_lowpass_taps(up, down) if taps is None else taps
        taps = np.ascontiguousarray(taps, np.float32)
        if taps.ndim != 1:
            raise ValueError("taps must be one-dimensional")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.pwg_resample_plan_create(self.up, self.down, taps.ctypes.data, taps.size, ctypes.byref(h)))
        self._h, self._destroy = h, L.pwg_resample_plan_destroy
        self.tile = L.pwg_resample_plan_tile(h)

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def out_len(self, n_samples):
        return -(-int(n_samples) * self.up // self.down)

    def run(self, wave, lengths):
        """wave: packed fp32 device tensor of sum(lengths) samples -> the packed outputs on the current stream."""
        L = _lib.load()
        total = sum(self.out_len(t) for t in lengths)
        out = torch.empty(total, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pwg_resample_run(self._h, wave.data_ptr(), _starts(lengths), len(lengths), out.data_ptr(), total,
                                          _stream(self.device)))
        return out


def fit_run(wave, src_start, src_len, out_lengths, gain=1.0, want_peak=True):
    """pwg_wave_fit_run: per utterance out[i] = gain * wave[src_start + min(i, src_len - 1)], i < out_length.
    wave: fp32 device tensor -> (packed outputs, peaks (n,) fp32 or None) on the current stream."""
    L = _lib.load()
    n = len(out_lengths)
    if len(src_start) != n or len(src_len) != n:
        raise ValueError("src_start, src_len and out_lengths must hold one entry per utterance")
    for s, t in zip(src_start, src_len):
        if int(s) < 0 or int(t) < 1 or int(s) + int(t) > wave.numel():
            raise ValueError(f"the source range [{s}, {s} + {t}) is empty or outside the {wave.numel()} samples")
    arr = lambda v: (ctypes.c_longlong * len(v))(*[int(x) for x in v])  # noqa: E731
    ostart = _starts(out_lengths)
    out = torch.empty(int(ostart[n]), dtype=torch.float32, device=wave.device)
    peak = torch.empty(n, dtype=torch.float32, device=wave.device) if want_peak else None
    with torch.cuda.device(wave.device):
        _lib.check(L.pwg_wave_fit_run(wave.data_ptr(), arr(src_start), arr(src_len), out.data_ptr(), ostart, n,
                                      ctypes.c_float(gain), peak.data_ptr() if want_peak else None, _stream(wave.device)))
    return out, peak


def _flatten(waves):
    flat = []
    for w in waves:
        w = torch.as_tensor(w) if not isinstance(w, torch.Tensor) else w.detach()
        if w.dim() == 2 and w.size(1) == 1:
            w = w.reshape(-1)
        if w.dim() != 1:
            raise ValueError("each waveform must be (T,) or (T, 1)")
        if w.numel() == 0:
            raise ValueError("an empty waveform cannot be conditioned")
        flat.append(w)
    return flat


def _device_of(flat, device):
    if device is not None:
        device = torch.device(device)
    else:
        on_gpu = [w.device for w in flat if w.device.type == "cuda"]
        if not on_gpu and not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU)
        device = on_gpu[0] if on_gpu else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise RuntimeError(_NO_CPU)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _pack(flat, device):
    if len(flat) == 1:
        return flat[0].to(device=device, dtype=torch.float32).contiguous()
    return torch.cat([w.to(device=device, dtype=torch.float32) for w in flat])


class AudioConditioner:
    """The reference preprocess's waveform steps over ragged batches on the GPU: silence trim
    (``trim_batch``), resampling (``resample_batch``) and the fit to a length with the global gain and the
    clipping peak (``fit_batch``). Every method takes a list of (T,) or (T, 1) tensors or arrays and returns
    views of one device buffer."""

    def __init__(self, sampling_rate, trim_silence=False, trim_threshold_in_db=60, trim_frame_size=2048,
                 trim_hop_size=512, sampling_rate_for_feats=None, global_gain_scale=1.0, input_sampling_rate=None,
                 trim_pad_mode="constant"):
        self.sampling_rate = int(sampling_rate)
        self.trim_silence = bool(trim_silence)
        self.trim_threshold_in_db = float(trim_threshold_in_db)
        self.trim_frame_size, self.trim_hop_size = int(trim_frame_size), int(trim_hop_size)
        self.trim_pad_mode = trim_pad_mode
        self.sampling_rate_for_feats = None if sampling_rate_for_feats is None else int(sampling_rate_for_feats)
        self.global_gain_scale = float(global_gain_scale)
        self.input_sampling_rate = None if input_sampling_rate is None else int(input_sampling_rate)
        if self.trim_silence:
            if not (self.trim_threshold_in_db > 0 and np.isfinite(self.trim_threshold_in_db)):
                raise ValueError(f"trim_threshold_in_db must be finite and positive, got {trim_threshold_in_db}")
            if self.trim_frame_size < 1 or self.trim_hop_size < 1:
                raise ValueError("trim_frame_size and trim_hop_size must be >= 1")
            if trim_pad_mode not in _lib.PWG_TRIM_PAD_MODES:
                raise ValueError(f"trim_pad_mode must be one of {sorted(_lib.PWG_TRIM_PAD_MODES)}")
            if (_lib.PWG_TRIM_FRAME_TILE - 1) * self.trim_hop_size + self.trim_frame_size > _lib.PWG_TRIM_MAX_TILE_SPAN:
                raise NotImplementedError("the trim frame tile does not fit the LDS: lower trim_frame_size / trim_hop_size")
        for a, b in ((self.input_sampling_rate, self.sampling_rate), (self.sampling_rate, self.sampling_rate_for_feats)):
            if a is not None and b is not None:
                self.check_ratio(a, b)
        self._plans = {}

    @staticmethod
    def check_ratio(orig_sr, target_sr):
        if orig_sr < 1 or target_sr < 1:
            raise ValueError("sampling rates must be positive")
        g = math.gcd(int(orig_sr), int(target_sr))
        if max(orig_sr, target_sr) // g > _lib.PWG_RESAMPLE_MAX_RATE:
            raise NotImplementedError(f"resampling {orig_sr} -> {target_sr} Hz reduces to {target_sr // g}/{orig_sr // g}, "
                                      f"above {_lib.PWG_RESAMPLE_MAX_RATE}")

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"] = {}  # C handles and device memory: a copy builds its own
        return state

    @classmethod
    def from_config(cls, config, input_sampling_rate=None, **kwargs):
        """From a recipe's config dict: trim_silence, trim_threshold_in_db, trim_frame_size, trim_hop_size,
        sampling_rate, sampling_rate_for_feats and global_gain_scale (a scale that is not positive is not
        applied, as in bin/preprocess.py:445)."""
        gain = float(config.get("global_gain_scale", 1.0) or 0.0)
        return cls(config["sampling_rate"], trim_silence=config.get("trim_silence", False),
                   trim_threshold_in_db=config.get("trim_threshold_in_db", 60),
                   trim_frame_size=config.get("trim_frame_size", 2048), trim_hop_size=config.get("trim_hop_size", 512),
                   sampling_rate_for_feats=config.get("sampling_rate_for_feats"),
                   global_gain_scale=gain if gain > 0.0 else 1.0, input_sampling_rate=input_sampling_rate, **kwargs)

    def _plan(self, key, make):
        if key not in self._plans:
            self._plans[key] = make()
        return self._plans[key]

    def trim_plan(self, device):
        return self._plan(("trim", device), lambda: TrimPlan(device, self.trim_frame_size, self.trim_hop_size,
                                                             self.trim_threshold_in_db, self.trim_pad_mode))

    def resample_plan(self, device, orig_sr, target_sr):
        g = math.gcd(int(orig_sr), int(target_sr))
        up, down = int(target_sr) // g, int(orig_sr) // g
        return self._plan(("resample", device, up, down), lambda: ResamplePlan(device, up, down))

    def trim_batch(self, waves, device=None):
        """-> (views of the packed batch cut to the non-silent ranges, bounds ndarray (n, 2) int64). The
        bounds come back to the host here: the one synchronisation of the conditioning."""
        if len(waves) == 0:
            return [], np.zeros((0, 2), np.int64)
        flat = _flatten(waves)
        device = _device_of(flat, device)
        with torch.no_grad():
            packed = _pack(flat, device)
            lengths = [int(w.numel()) for w in flat]
            bounds, _ = self.trim_plan(device).run(packed, lengths)
            bounds = bounds.cpu().numpy()
        views, s0 = [], 0
        for t, (a, b) in zip(lengths, bounds):
            views.append(packed[s0 + int(a): s0 + int(b)])
            s0 += t
        return views, bounds

    def resample_batch(self, waves, orig_sr, target_sr, device=None):
        """-> the utterances at target_sr, ceil(T target_sr / orig_sr) samples each."""
        if len(waves) == 0:
            return []
        self.check_ratio(orig_sr, target_sr)
        flat = _flatten(waves)
        device = _device_of(flat, device)
        plan = self.resample_plan(device, orig_sr, target_sr)
        lengths = [int(w.numel()) for w in flat]
        with torch.no_grad():
            out = plan.run(_pack(flat, device), lengths)
        return list(torch.split(out, [plan.out_len(t) for t in lengths]))

    def fit_batch(self, waves, out_lengths, gain=None, device=None):
        """-> (views: each utterance edge-padded or cut to out_lengths[u] and scaled by gain (default: the
        global_gain_scale), peaks (n,) fp32 device tensor of max |out|)."""
        if len(waves) == 0:
            return [], torch.zeros(0)
        flat = _flatten(waves)
        out_lengths = [int(n) for n in out_lengths]
        if len(out_lengths) != len(flat) or min(out_lengths) < 1:
            raise ValueError("out_lengths must hold one length >= 1 per waveform")
        device = _device_of(flat, device)
        lengths = [int(w.numel()) for w in flat]
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        with torch.no_grad():
            out, peak = fit_run(_pack(flat, device), starts, lengths, out_lengths,
                                self.global_gain_scale if gain is None else gain)
        return list(torch.split(out, out_lengths)), peak


def _as_device_batch(x):
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    if x.device.type != "cuda":
        raise RuntimeError(_NO_CPU)
    x = x.detach().to(torch.float32).contiguous()
    B, T = (1, x.numel()) if x.dim() == 1 else x.shape
    if T < 1 or B < 1:
        raise ValueError("an empty signal cannot be resampled")
    return x, B, T


def resample_poly(x, up, down, taps=None):
    """``scipy.signal.resample_poly(x, up, down, axis=-1)`` on the HIP kernel: x (T,) or (B, T) device tensor ->
    (ceil(T up / down),) or (B, ...) fp32. taps: odd-length low-pass, default ``kaiser_lowpass_taps(up, down)``."""
    x, B, T = _as_device_batch(x)
    plan = ResamplePlan(x.device, up, down, taps)
    with torch.no_grad():
        out = plan.run(x.view(-1), [T] * B)
    return out if x.dim() == 1 else out.view(B, -1)


def resample(audio, orig_sr, target_sr):
    """The call shape of ``librosa.resample(audio, orig_sr=, target_sr=)`` in the reference: (T,) ndarray in,
    (ceil(T target_sr / orig_sr),) float32 ndarray out. The filter is the Kaiser-windowed sinc of
    ``kaiser_lowpass_taps`` (scipy's resample_poly default), NOT librosa's default soxr_hq: the soxr
    package was not available to compare with, so parity with it is unverified."""
    audio = np.asarray(audio, np.float32)
    if audio.ndim != 1:
        raise ValueError("audio must be (T,)")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU)
    AudioConditioner.check_ratio(int(orig_sr), int(target_sr))
    x = torch.from_numpy(audio).to(torch.device("cuda", torch.cuda.current_device()))
    return resample_poly(x, int(target_sr), int(orig_sr)).cpu().numpy()


def trim_silence(audio, top_db=60, frame_length=2048, hop_length=512, pad_mode="constant"):
    """``librosa.effects.trim(audio, top_db=, frame_length=, hop_length=)`` with ref=np.max on the HIP kernel:
    (T,) ndarray -> (audio[start:end], np.array([start, end])). pad_mode: "constant" (librosa >= 0.10) or
    "reflect" (older librosa's centred rms)."""
    audio = np.asarray(audio)
    if audio.ndim != 1:
        raise ValueError("audio must be (T,)")
    if audio.size == 0:
        raise ValueError("an empty waveform cannot be trimmed")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU)
    device = torch.device("cuda", torch.cuda.current_device())
    plan = TrimPlan(device, frame_length, hop_length, top_db, pad_mode)
    with torch.no_grad():
        bounds, _ = plan.run(torch.from_numpy(np.ascontiguousarray(audio, np.float32)).to(device), [audio.size])
    start, end = (int(v) for v in bounds.cpu().numpy()[0])
    return audio[start:end], np.array([start, end])
