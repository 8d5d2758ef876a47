/*
 * pwg_mel.h — C-ABI of the log-mel feature extractor: a ragged batch of waveforms to the normalised
 * log-mel rows every mel-conditioned generator reads (parallel_wavegan/bin/preprocess.py:
 * logmelfilterbank and losses/mel_loss.py:MelSpectrogram; center = True, reflect padding, periodic
 * Hann window).
 *
 * Per frame t of an utterance x[0:T) and bin k in [0, n_fft / 2], all in fp32 on the device:
 *   re, im = sum_n x[t hop + n - n_fft / 2] w[n] (cos, -sin)(2 pi n k / n_fft)
 *   amp    = sqrt(max(re^2 + im^2, eps))   with amp_floor (MelSpectrogram.forward)
 *          = sqrt(re^2 + im^2)             without        (logmelfilterbank)
 *   mel[m] = max(eps, sum_k amp[k] melmat[m][k])
 *   out[m] = log_b(mel[m]), then (out - mean[m]) / scale[m] when the plan has statistics
 * w is the periodic Hann window of win_length taps, w[n] = 0.5 - 0.5 cos(2 pi (n - off) / win_length)
 * on n in [off, off + win_length), off = (n_fft - win_length) / 2, zero elsewhere (what torch.stft
 * and librosa.stft do). A sample index outside [0, T) mirrors at the utterance's own first / last
 * sample (reflect padding by n_fft / 2), never into a neighbour. An utterance gives 1 + T / hop frames.
 *
 * The STFT is a windowed-DFT GEMM on the exact-fp32 MFMA (k-ordered fp32 fma chains), fused with
 * the magnitude, the mel projection, the clamp, the log and the normalisation in ONE kernel: the
 * spectrogram never leaves the registers. The plan holds the windowed basis (built in float64 with
 * the angle reduced in integers, rounded once to fp32; only the win_length non-zero taps) and the
 * mel matrix in MFMA fragment order on the device.
 *
 * Conventions as in pwg_sine.h / pwg_embed.h: int status codes (pwg_last_error() gives the message),
 * argument checks (PWG_ERR_INVALID, then PWG_ERR_UNSUPPORTED) before any HIP call, no allocation and
 * no host synchronisation in pwg_mel_run, graph-capturable on `stream`, separate launches only and
 * every loop bounded by the arguments.
 *
 * The utterance boundaries are a HOST array: the checks this header promises before a launch (an
 * utterance too short to reflect, the row count) need them on the host, so the kernel receives each
 * utterance's offset and length by value and reads no boundary from device memory; a captured graph
 * therefore replays the boundaries it was captured with. Every sample index is clamped to the
 * utterance's [0, T) after the reflection. Non-finite samples are outside the contract: a NaN or
 * infinity spreads over the frames that cover it and nothing reports it.
 */
#ifndef PWG_MEL_H_
#define PWG_MEL_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PWG_MEL_FRAME_TILE = 64, /* consecutive frames of one utterance per workgroup */
  PWG_MEL_MAX_MELS = 128,
  PWG_MEL_WINDOW_HANN = 0  /* the only window */
};

/* Frames of an utterance of T samples: 1 + T / hop; -1 for T < 0 or hop < 1. */
PWG_API long long pwg_mel_frames(long long T, int hop);

/* melmat: HOST, num_mels x (n_fft / 2 + 1) fp32 row-major, melmat_count its element count.
 * log_base: 10, 2, or 0 for the natural logarithm. amp_floor: 0 or 1. mean, scale: HOST, num_mels
 * floats each, both or neither. The plan owns device copies on the current device; *plan is set on
 * PWG_OK only.
 * PWG_ERR_INVALID: a null melmat or plan, n_fft odd, below 2 or below win_length, win_length < 1,
 *   hop < 1, num_mels < 1, melmat_count != num_mels (n_fft / 2 + 1), eps negative or not finite,
 *   amp_floor not 0 / 1, only one of mean / scale.
 * PWG_ERR_UNSUPPORTED: a window other than PWG_MEL_WINDOW_HANN, a log base other than the three,
 *   num_mels > PWG_MEL_MAX_MELS, n_fft > 65536, or a geometry whose PWG_MEL_FRAME_TILE-frame
 *   sample span does not fit the LDS ((PWG_MEL_FRAME_TILE - 1) hop + win_length beyond ~31,000), or whose
 *   windowed basis (n_fft / 2 rounded up to 32, times win_length, times 2 floats) would exceed 1 GiB.
 * PWG_ERR_HIP: a HIP call failed, or the host ran out of memory (no exception leaves the call). */
PWG_API int pwg_mel_plan_create(int n_fft, int win_length, int hop, int window, int num_mels, const float* melmat,
                                long long melmat_count, float eps, float log_base, int amp_floor, const float* mean,
                                const float* scale, void** plan);
PWG_API void pwg_mel_plan_destroy(void* plan);

/* wave: DEVICE, packed fp32; utterance u is samples [sample_start[u], sample_start[u + 1]).
 * sample_start: HOST, n_utts + 1 entries, read during the call only. out: DEVICE, out_rows x
 * num_mels fp32, mel innermost, the utterances' frames back to back (utterance u's first row is the
 * sum of pwg_mel_frames of the utterances before it).
 * PWG_ERR_INVALID: a null argument, n_utts < 1, boundaries that are negative or decrease, an
 *   utterance of n_fft / 2 samples or fewer (torch.stft refuses it too), out_rows that is not the
 *   sum of the utterances' frames, a current device other than the one the plan was created on.
 * One launch per 64 utterances. */
PWG_API int pwg_mel_run(void* plan, const float* wave, const long long* sample_start, int n_utts, float* out,
                        long long out_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_MEL_H_ */
