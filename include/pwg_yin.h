/*
 * pwg_yin.h — C-ABI of the YIN f0 estimator: a ragged batch of waveforms to the frame-rate f0 contour
 * UHiFiGAN's excitation (pwg_sine.h) and the f0-conditioned token vocoders read (reference
 * parallel_wavegan/bin/preprocess.py:f0_torchyin; de Cheveigne & Kawahara 2002, eqs. 6 and 8).
 *
 * With W = 2 tau_max, an utterance x[0:T) has N = 1 + (T - W) / hop frames (one frame, zero-padded at
 * its end, when T < W); frame t covers x[t hop : t hop + W), no centring. Per frame, in fp32:
 *   d(tau) = sum_{j = 0}^{W - 1 - tau} (x[t hop + j] - x[t hop + j + tau])^2        tau = 0 .. tau_max - 1
 *   c(tau) = d(tau) tau / max(sum_{s = 1}^{tau} d(s), 1e-5)                          tau = 1 .. tau_max - 1
 * The searched sequence is c[k], k = 0 .. L - 1, tau = k + tau_min + 1, L = tau_max - 1 - tau_min.
 * fb is the smallest k with c[k] < threshold; with no such k, or with fb = 0, the frame is unvoiced
 * (k* = 0); otherwise k* is the smallest k >= fb with k = L - 1 or c[k + 1] - c[k] >= 0. The output is
 * f0 = fs / (k* + tau_min + 1) (an fp32 division) for k* > 0, else 0; with log_f0 the voiced values
 * are replaced by their natural logarithm and zeros stay 0.
 *
 * d is computed in the direct form: one fp32 fma chain per lag, j ascending (never through the
 * autocorrelation, whose energy terms cancel where the voicing decision is taken). The prefix sum is
 * taken in a fixed order too, so a frame's result does not depend on what else is in the batch.
 *
 * Conventions as in pwg_mel.h: int status codes (pwg_last_error() gives the message), argument checks
 * (PWG_ERR_INVALID, then PWG_ERR_UNSUPPORTED) before any HIP call, no allocation and no host
 * synchronisation in pwg_yin_run, graph-capturable on `stream`, separate launches only, every loop
 * bounded by the arguments, no workgroup waits on another. The utterance boundaries and row counts
 * are HOST arrays, passed to the kernel by value: a captured graph replays the ones it was captured
 * with. Every sample index is clamped to the utterance's [0, T); an utterance never reads a
 * neighbour's samples. Non-finite samples are outside the contract.
 */
#ifndef PWG_YIN_H_
#define PWG_YIN_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PWG_YIN_FRAME_TILE = 8,  /* consecutive frames of one utterance per workgroup */
  PWG_YIN_MAX_TAU = 1680   /* largest tau_max: 8 frames of 2 tau_max samples and their 8 x tau_max
                              differences are held in the 160 KiB LDS at once */
};

/* Frames of an utterance of T samples: 1 + (T - 2 tau_max) / hop, 1 for 0 < T < 2 tau_max; -1 for
 * T < 1, tau_max < 1 or hop < 1. */
PWG_API long long pwg_yin_frames(long long T, int tau_max, int hop);

/* fs: the sampling rate in Hz. log_f0: 0 (Hz) or 1 (natural log of the voiced values). The plan is
 * bound to the current device; *plan is set on PWG_OK only.
 * PWG_ERR_INVALID: a null plan, fs not finite or not positive, hop < 1, tau_min < 0,
 *   tau_max - 1 - tau_min < 1, a threshold that is not finite or not positive, log_f0 not 0 / 1.
 * PWG_ERR_UNSUPPORTED: tau_max > PWG_YIN_MAX_TAU (the frame tile would not fit the LDS). */
PWG_API int pwg_yin_plan_create(float fs, int tau_min, int tau_max, int hop, float threshold, int log_f0,
                                void** plan);
PWG_API void pwg_yin_plan_destroy(void* plan);

/* wave: DEVICE, packed fp32; utterance u is samples [sample_start[u], sample_start[u + 1]).
 * sample_start: HOST, n_utts + 1 entries. out_frames: HOST, n_utts row counts, or NULL for each
 * utterance's own frame count N. Rows beyond N hold frame N - 1's values (the edge pad); fewer rows
 * than N cut the contour. f0: DEVICE, out_rows fp32, the utterances' rows back to back. tau: DEVICE,
 * out_rows int32 k* (0 = unvoiced), or NULL. cmdf: DEVICE, out_rows x L fp32 c[k], or NULL.
 * PWG_ERR_INVALID: a null plan, wave, sample_start or f0, n_utts < 1, boundaries that are negative or
 *   decrease, an empty utterance, out_frames[u] < 1, out_rows that is not the sum of the row counts,
 *   a current device other than the plan's.
 * One launch per 64 utterances. */
PWG_API int pwg_yin_run(void* plan, const float* wave, const long long* sample_start, int n_utts,
                        const long long* out_frames, float* f0, int* tau, float* cmdf, long long out_rows,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_YIN_H_ */
