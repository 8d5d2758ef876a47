"""MI355X-native Parallel WaveGAN generator inference engine.

Public surface (mirrors parallel_wavegan.models for the generator hot path):
  ParallelWaveGANGenerator  drop-in module, forward/inference run on HIP kernels
  Engine                    lower-level batch engine over the C-ABI (include/pwg.h)
  GraphedRun                one plan's forward captured as a HIP graph (pwg_graph_create) for
                            repeated shapes
  DiscreteSymbolHiFiGANGenerator  drop-in token vocoder (HIP embedding front end + HiFiGAN body)
  DiscreteSymbolDurationGenerator, DiscreteSymbolF0Generator
                            its duration- and f0-conditioned siblings (HIP duration predictor, length
                            regulator and f0 / weighted-sum front ends)
  StyleMelGANGenerator      drop-in StyleMelGAN generator on the TADE kernels (include/pwg_smg.h)
  DiscreteSymbolStyleMelGANGenerator
                            its token form: ids and a speaker id gathered in the first aux conv's staging, the
                            noise trimmed to the frames (pwg_smg_plan_create_ex, pwg_smg_run_tokens)
  UHiFiGANGenerator         drop-in U-Net HiFiGAN (mel + excitation): HIP excitation front end, strided
                            and two-source transposed convs on the conv-network executor
  SineGen                   drop-in sine excitation generator (layers/sine.py): f0 -> sine, uv, noise with
                            an exact 64-bit integer phase (include/pwg_sine.h); feeds UHiFiGANGenerator's
                            *_from_f0 methods
  VQVAE                     drop-in VQ-VAE (waveform -> codes -> waveform): HIP grouped strided encoder
                            levels, nearest-code search and decoder front end (include/pwg_vq.h)
  MelSpectrogram, logmelfilterbank, LogMelExtractor
                            waveform -> (normalised) log-mel features: the STFT as a windowed-DFT GEMM fused
                            with magnitude, mel projection, log and normalisation (include/pwg_mel.h)
  yin_estimate, f0_torchyin, YinF0Extractor
                            waveform -> frame-rate f0 contour: the YIN difference function in the direct form,
                            prefix sum and first-minimum search in one kernel (include/pwg_yin.h)
  trim_silence, resample, resample_poly, kaiser_lowpass_taps, AudioConditioner
                            the preprocess's waveform steps: silence trim, polyphase resampling, and the fit to
                            the feature length with the global gain and the clipping peak (include/pwg_wave.h)
"""

from .audio import AudioConditioner, kaiser_lowpass_taps, resample, resample_poly, trim_silence  # noqa: F401
from .engine import Engine, GraphedRun, HostHandle  # noqa: F401
from .dsym import DiscreteSymbolHiFiGANGenerator  # noqa: F401
from .dsym_stylemelgan import DiscreteSymbolStyleMelGANGenerator  # noqa: F401
from .dsym_variants import DiscreteSymbolDurationGenerator, DiscreteSymbolF0Generator  # noqa: F401
from .logmel import LogMelExtractor, MelSpectrogram, logmelfilterbank, slaney_mel_basis  # noqa: F401
from .models import ParallelWaveGANGenerator  # noqa: F401
from .sinegen import SineGen  # noqa: F401
from .stylemelgan import StyleMelGANGenerator  # noqa: F401
from .uhifigan import UHiFiGANGenerator  # noqa: F401
from .vqvae import VQVAE  # noqa: F401
from .yin import YinF0Extractor, f0_torchyin, yin_estimate  # noqa: F401

__version__ = "0.1.0"
