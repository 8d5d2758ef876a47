"""Log-mel feature extraction on the HIP STFT + mel kernel (include/pwg_mel.h): waveform in, the
``(T', num_mels)`` features every mel-conditioned generator's ``inference_batch`` reads out.

* ``MelSpectrogram``: drop-in for parallel_wavegan/losses/mel_loss.py:MelSpectrogram (inference only:
  no gradient flows through the kernel).
* ``logmelfilterbank``: parallel_wavegan/bin/preprocess.py:logmelfilterbank.
* ``LogMelExtractor``: a ragged batch of waveforms to a list of feature tensors, optionally normalised
  with a ``stats.npy``-style mean / scale (bin/normalize.py).
* ``slaney_mel_basis``: librosa.filters.mel (Slaney scale, Slaney norm) restated in NumPy.

The window is the periodic Hann window, the padding reflect with ``center=True``: what every recipe uses.
"""

import ctypes

import numpy as np
import torch

from . import _lib


def slaney_mel_basis(sr, n_fft, n_mels, fmin=None, fmax=None):
    """librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) with its defaults (htk=False,
    norm="slaney"): (n_mels, 1 + n_fft // 2) float32, computed in float64."""
    fmin = 0.0 if fmin is None else float(fmin)
    fmax = sr / 2.0 if fmax is None else float(fmax)
    f_sp, min_log_hz, min_log_mel = 200.0 / 3.0, 1000.0, 15.0
    logstep = np.log(6.4) / 27.0

    def hz_to_mel(f):
        return f / f_sp if f < min_log_hz else min_log_mel + np.log(f / min_log_hz) / logstep

    mels = np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2)
    mel_f = np.where(mels < min_log_mel, mels * f_sp, min_log_hz * np.exp(logstep * (mels - min_log_mel)))
    fftfreq = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreq[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return w.astype(np.float32)


def _log_base_code(log_base):
    """The C-ABI's log_base argument: 10, 2, or 0 for the natural logarithm (None here)."""
    if log_base is None:
        return 0.0
    if log_base in (2.0, 10.0):
        return float(log_base)
    raise ValueError(f"log_base: {log_base} is not supported.")


def _split_stats(stats, num_mels):
    if stats is None:
        return None, None
    if isinstance(stats, (tuple, list)):
        mean, scale = stats
    else:
        stats = np.asarray(stats)
        if stats.ndim != 2 or stats.shape[0] != 2:
            raise ValueError("stats must be a (2, num_mels) array (mean, scale) or a (mean, scale) pair")
        mean, scale = stats[0], stats[1]
    mean = np.ascontiguousarray(np.asarray(mean, np.float32).reshape(-1))
    scale = np.ascontiguousarray(np.asarray(scale, np.float32).reshape(-1))
    if mean.shape != (num_mels,) or scale.shape != (num_mels,):
        raise ValueError(f"mean and scale must hold num_mels = {num_mels} values each")
    return mean, scale


class MelPlan:
    """A pwg_mel plan on one device: the windowed DFT basis and the mel matrix in fragment order."""

    def __init__(self, device, n_fft, win_length, hop, melmat, eps, log_base, amp_floor, mean=None, scale=None,
                 window=_lib.PWG_MEL_WINDOW_HANN):
        L = _lib.load()
        melmat = np.ascontiguousarray(melmat, np.float32)
        if melmat.ndim != 2:
            raise ValueError("melmat must be (num_mels, n_fft // 2 + 1)")
        self.device, self.hop, self.n_fft, self.num_mels = torch.device(device), int(hop), int(n_fft), melmat.shape[0]
        fp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.pwg_mel_plan_create(int(n_fft), int(win_length), int(hop), int(window), melmat.shape[0],
                                             fp(melmat), melmat.size, ctypes.c_float(eps), ctypes.c_float(log_base),
                                             int(amp_floor), fp(mean), fp(scale), ctypes.byref(h)))
        self._h, self._destroy = h, L.pwg_mel_plan_destroy

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def run(self, wave, lengths):
        """wave: packed fp32 device tensor of sum(lengths) samples -> (frames, num_mels) device tensor
        on the current stream."""
        L = _lib.load()
        starts = (ctypes.c_longlong * (len(lengths) + 1))()
        for i, t in enumerate(lengths):
            starts[i + 1] = starts[i] + int(t)
        rows = sum(1 + int(t) // self.hop for t in lengths)
        out = torch.empty(rows, self.num_mels, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(L.pwg_mel_run(self._h, wave.data_ptr(), starts, len(lengths), out.data_ptr(), rows, stream))
        return out


def _check_geometry(fft_size, win_length, hop_size, num_mels):
    """The plan's PWG_ERR_INVALID checks, raised before a device is needed."""
    if fft_size < 2 or fft_size % 2:
        raise ValueError(f"fft_size must be even and at least 2, got {fft_size}")
    if not 1 <= win_length <= fft_size:
        raise ValueError(f"win_length must be within 1..fft_size, got {win_length}")
    if hop_size < 1:
        raise ValueError(f"hop_size must be >= 1, got {hop_size}")
    if num_mels < 1:
        raise ValueError(f"num_mels must be >= 1, got {num_mels}")
    if num_mels > _lib.PWG_MEL_MAX_MELS:
        raise NotImplementedError(f"num_mels above {_lib.PWG_MEL_MAX_MELS} is not accelerated")


class LogMelExtractor:
    """Waveforms to (normalised) log-mel features on the GPU, over ragged batches.

    stats: a ``stats.npy``-style (2, num_mels) array [mean, scale] or a (mean, scale) pair; the output
    is then ``(logmel - mean) / scale`` (bin/normalize.py). melmat: a (num_mels, fft_size // 2 + 1)
    matrix to use instead of ``slaney_mel_basis``. amp_floor: clamp the power at eps before the square
    root (losses/mel_loss.py) instead of not at all (bin/preprocess.py, the default)."""

    def __init__(self, sampling_rate, fft_size=1024, hop_size=256, win_length=None, num_mels=80, fmin=None,
                 fmax=None, eps=1e-10, log_base=10.0, stats=None, melmat=None, amp_floor=False, window="hann"):
        if window != "hann":
            raise NotImplementedError(f"window {window!r} is not accelerated (hann only)")
        win_length = fft_size if win_length is None else win_length
        _check_geometry(fft_size, win_length, hop_size, num_mels)
        self.sampling_rate, self.fft_size, self.hop_size, self.win_length = sampling_rate, fft_size, hop_size, win_length
        self.num_mels, self.eps, self.log_base, self.amp_floor = num_mels, eps, log_base, bool(amp_floor)
        self._log_code = _log_base_code(log_base)
        if melmat is None:
            melmat = slaney_mel_basis(sampling_rate, fft_size, num_mels, fmin, fmax)
        melmat = np.ascontiguousarray(melmat, np.float32)
        if melmat.shape != (num_mels, fft_size // 2 + 1):
            raise ValueError(f"melmat must be ({num_mels}, {fft_size // 2 + 1}), got {tuple(melmat.shape)}")
        self.melmat = melmat
        self.mean, self.scale = _split_stats(stats, num_mels)
        self._plans = {}

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"] = {}  # C handles and device memory: a copy builds its own
        return state

    @classmethod
    def from_config(cls, config, stats=None, **kwargs):
        """From a recipe's config dict (sampling_rate, fft_size, hop_size, win_length, num_mels, fmin, fmax)."""
        if config.get("window", "hann") != "hann":
            raise NotImplementedError(f"window {config['window']!r} is not accelerated (hann only)")
        return cls(config["sampling_rate"], fft_size=config["fft_size"], hop_size=config["hop_size"],
                   win_length=config.get("win_length"), num_mels=config["num_mels"], fmin=config.get("fmin"),
                   fmax=config.get("fmax"), stats=stats, **kwargs)

    def frames(self, n_samples):
        return 1 + int(n_samples) // self.hop_size

    def plan(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("log-mel extraction runs on a ROCm GPU only (there is no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._plans:
            self._plans[device] = MelPlan(device, self.fft_size, self.win_length, self.hop_size, self.melmat, self.eps,
                                          self._log_code, self.amp_floor, self.mean, self.scale)
        return self._plans[device]

    def extract_batch(self, waves, device=None):
        """waves: a list of (T_u,) or (T_u, 1) tensors or arrays -> a list of (1 + T_u // hop, num_mels)
        device tensors, views of one buffer. Host arrays go to ``device`` (default: the current GPU)."""
        if len(waves) == 0:
            return []
        flat = []
        for w in waves:
            w = torch.as_tensor(w) if not isinstance(w, torch.Tensor) else w.detach()
            if w.dim() == 2 and w.size(1) == 1:
                w = w.reshape(-1)
            if w.dim() != 1:
                raise ValueError("each waveform must be (T,) or (T, 1)")
            flat.append(w)
        if device is None:
            on_gpu = [w.device for w in flat if w.device.type == "cuda"]
            if not on_gpu and not torch.cuda.is_available():
                raise RuntimeError("log-mel extraction runs on a ROCm GPU only (there is no CPU fallback)")
            device = on_gpu[0] if on_gpu else torch.device("cuda", torch.cuda.current_device())
        plan = self.plan(device)
        lengths = [int(w.numel()) for w in flat]
        short = [t for t in lengths if t <= self.fft_size // 2]
        if short:
            raise ValueError(f"a waveform of {short[0]} samples is too short: reflect padding needs more than "
                             f"fft_size // 2 = {self.fft_size // 2}")
        with torch.no_grad():
            if len(flat) == 1:
                packed = flat[0].to(device=plan.device, dtype=torch.float32).contiguous()
            else:
                packed = torch.cat([w.to(device=plan.device, dtype=torch.float32) for w in flat])
            out = plan.run(packed, lengths)
        rows = [self.frames(t) for t in lengths]
        return list(torch.split(out, rows))

    def extract(self, wave, device=None):
        return self.extract_batch([wave], device)[0]


class MelSpectrogram(torch.nn.Module):
    """losses/mel_loss.py:MelSpectrogram on the HIP kernel: ``forward(x (B, T) or (B, 1, T)) -> (B, num_mels,
    frames)``. Same constructor arguments, defaults, attributes and ``melmat`` buffer ((n_bins, num_mels))."""

    def __init__(self, fs=22050, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=80,
                 fmax=7600, center=True, normalized=False, onesided=True, eps=1e-10, log_base=10.0):
        super().__init__()
        self.fft_size = fft_size
        self.win_length = fft_size if win_length is None else win_length
        self.hop_size = hop_size
        self.center, self.normalized, self.onesided = center, normalized, onesided
        if window is not None and not hasattr(torch, f"{window}_window"):
            raise ValueError(f"{window} window is not implemented")
        if window != "hann":
            raise NotImplementedError(f"window {window!r} is not accelerated (hann only)")
        for name, value, want in (("center", center, True), ("normalized", normalized, False),
                                  ("onesided", onesided, True)):
            if bool(value) != want:
                raise NotImplementedError(f"{name}={value} is not accelerated")
        self.window = window
        self.eps = eps
        self.log_base = log_base
        self._log_code = _log_base_code(log_base)
        _check_geometry(fft_size, self.win_length, hop_size, num_mels)
        melmat = slaney_mel_basis(fs, fft_size, num_mels, fmin, fmax)
        self.register_buffer("melmat", torch.from_numpy(melmat.T.copy()).float())
        self._plans = {}

    def __getstate__(self):
        # the plans hold C handles and device memory: a copy or a pickle of the module builds its own
        state = self.__dict__.copy()
        state["_plans"] = {}
        return state

    def _plan(self, device):
        key = (device, self.melmat._version)
        if key not in self._plans:
            melmat = self.melmat.detach().cpu().numpy().T
            self._plans = {key: MelPlan(device, self.fft_size, self.win_length, self.hop_size, melmat, self.eps,
                                        self._log_code, True)}
        return self._plans[key]

    def forward(self, x):
        if x.dim() == 3:
            x = x.reshape(-1, x.size(2))
        if x.dim() != 2:
            raise ValueError("x must be (B, T) or (B, 1, T)")
        if x.device.type != "cuda":
            raise RuntimeError("parallelwavegan_amd.MelSpectrogram runs on a ROCm GPU only (there is no CPU fallback)")
        B, T = x.shape
        if T <= self.fft_size // 2:
            raise ValueError(f"T = {T} is too short: reflect padding needs more than fft_size // 2 = {self.fft_size // 2}")
        with torch.no_grad():
            out = self._plan(x.device).run(x.detach().to(torch.float32).contiguous().view(-1), [T] * B)
        return out.view(B, 1 + T // self.hop_size, -1).transpose(1, 2)


def logmelfilterbank(audio, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80,
                     fmin=None, fmax=None, eps=1e-10, log_base=10.0):
    """bin/preprocess.py:logmelfilterbank on the GPU: audio (T,) array or tensor -> (frames, num_mels); a
    NumPy array for an array, a device tensor for a tensor."""
    ex = LogMelExtractor(sampling_rate, fft_size, hop_size, win_length, num_mels, fmin, fmax, eps, log_base,
                         window=window)
    out = ex.extract(audio)
    return out if isinstance(audio, torch.Tensor) else out.cpu().numpy()
