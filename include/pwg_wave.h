/*
 * pwg_wave.h — C-ABI of the audio conditioning the reference runs on a waveform before any feature is
 * taken (reference parallel_wavegan/bin/preprocess.py:359-452): silence trim, rational resampling, and the
 * fit to the feature length with the global gain and the clipping peak. Ragged batches throughout: a
 * packed fp32 buffer and HOST boundaries.
 *
 * 1. Silence trim (librosa.effects.trim in closed form). Utterance x[0:T), frame length fl, hop h,
 *    p = fl / 2 (integer division): n = 1 + (T + 2 p - fl) / h frames, frame t covers
 *    x[t h - p : t h - p + fl). An index outside [0, T) reads 0 in PWG_TRIM_PAD_ZERO (librosa >= 0.10) and
 *    mirrors at the utterance's own ends (period 2 (T - 1), the end samples not repeated) in
 *    PWG_TRIM_PAD_REFLECT (older librosa). P[t] = (sum x^2) / fl in fp32, in a fixed order: lane l of a
 *    wave adds the squares of the frame's samples l, l + 64, ... by fma, then a butterfly over the lanes.
 *    Frame t is non-silent iff max(1e-10, P[t]) > max(1e-10, max_t P[t]) * 10^(-top_db / 10), the factor
 *    computed in double and rounded once to fp32: amplitude_to_db(rms, ref=np.max, top_db=None) > -top_db
 *    without the logarithms. With top_db > 0 the loudest frame is non-silent, so the range is never
 *    empty and an all-zero utterance is kept whole. With a the first and b the last non-silent frame the
 *    bounds are [a h, min(T, (b + 1) h)).
 *
 * 2. Polyphase rational resampler (scipy.signal.resample_poly's zero-padded form). up and down are
 *    reduced by their gcd; odd-length taps hf[0 .. 2 half] come from the caller. n_out = ceil(T up / down),
 *      y[m] = sum_i x[i] hf[m down + half - i up],
 *      i = max(0, ceil((m down - half) / up)) .. min(T - 1, floor((m down + half) / up)),
 *    one fp32 fma chain per output, i ascending. up == down is a copy.
 *
 * 3. Fit, gain and peak: out_u[i] = gain * x[src_start_u + min(i, src_len_u - 1)] for i < out_len_u (the cut
 *    of a trimmed range, the reference's edge pad and cut to frames * hop, and audio *= global_gain_scale in
 *    one pass; the product is the plain fp32 one) and peak[u] = max_i |out_u[i]|, taken as an integer
 *    maximum over the bits of the non-negative floats: order-independent, so deterministic.
 *
 * Conventions as in pwg_mel.h and pwg_yin.h: int status codes (pwg_last_error() gives the message),
 * argument checks (PWG_ERR_INVALID, then PWG_ERR_UNSUPPORTED) before any HIP call, no allocation and no
 * host synchronisation in the *_run functions, graph-capturable on `stream`, separate launches only,
 * every loop bounded by the arguments, no workgroup waits on another. Boundaries are HOST arrays, passed
 * to the kernels by value: a captured graph replays the ones it was captured with. Every sample index is
 * clamped to its own utterance; an utterance never reads a neighbour's samples, and a result does not
 * depend on what else is in the batch. One launch of each kernel per 64 utterances. Non-finite samples
 * are outside the contract.
 */
#ifndef PWG_WAVE_H_
#define PWG_WAVE_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PWG_TRIM_PAD_ZERO = 0,
  PWG_TRIM_PAD_REFLECT = 1,
  PWG_TRIM_FRAME_TILE = 16,     /* consecutive frames of one utterance per workgroup of the power kernel */
  PWG_TRIM_MAX_TILE_SPAN = 36864, /* (FRAME_TILE - 1) hop + fl at most: the tile's samples are held in LDS */
  PWG_RESAMPLE_MAX_RATE = 640,  /* largest reduced up or down: covers 11.025 kHz -> 48 kHz */
  PWG_RESAMPLE_MAX_TAPS = 20 * 640 + 1,
  PWG_RESAMPLE_OUT_TILE = 1024  /* outputs of one utterance per workgroup (fewer where the tile's input
                                   span would not fit the LDS next to the taps: pwg_resample_plan_tile) */
};

/* ------------------------------------------------------------------------------------------- trim */

/* Frames of an utterance of T samples: 1 + (T + 2 (fl / 2) - fl) / hop; -1 for T < 1, fl < 1 or hop < 1. */
PWG_API long long pwg_trim_frames(long long T, int fl, int hop);

/* The plan is bound to the current device; *plan is set on PWG_OK only.
 * PWG_ERR_INVALID: a null plan, fl < 1, hop < 1, top_db not finite or <= 0, an unknown pad_mode.
 * PWG_ERR_UNSUPPORTED: (PWG_TRIM_FRAME_TILE - 1) hop + fl > PWG_TRIM_MAX_TILE_SPAN. */
PWG_API int pwg_trim_plan_create(int fl, int hop, float top_db, int pad_mode, void** plan);
PWG_API void pwg_trim_plan_destroy(void* plan);

/* wave: DEVICE, packed fp32; utterance u is samples [sample_start[u], sample_start[u + 1]).
 * sample_start: HOST, n_utts + 1 entries. bounds: DEVICE int64 [n_utts][2], (start, end) in samples of the
 * utterance. power: DEVICE, power_rows fp32, every utterance's P[t] back to back, or NULL (power_rows is
 * then ignored and the bounds kernel takes the powers from the samples itself, in the same order).
 * PWG_ERR_INVALID: a null plan, wave, sample_start or bounds, n_utts < 1, boundaries that are negative or
 *   decrease, an empty utterance, power_rows that is not the sum of the frame counts, a current device
 *   other than the plan's. */
PWG_API int pwg_trim_run(void* plan, const float* wave, const long long* sample_start, int n_utts,
                         long long* bounds, float* power, long long power_rows, void* stream);

/* --------------------------------------------------------------------------------------- resample */

/* ceil(T up / down); -1 for T < 1, up < 1 or down < 1. */
PWG_API long long pwg_resample_out_len(long long T, int up, int down);

/* taps: HOST fp32, tap_count = 2 half + 1 of them; copied to the device here (the plan is bound to the
 * current device; *plan is set on PWG_OK only).
 * PWG_ERR_INVALID: a null plan or taps, up < 1, down < 1, tap_count < 1 or even.
 * PWG_ERR_UNSUPPORTED: max(up, down) / gcd > PWG_RESAMPLE_MAX_RATE, tap_count > PWG_RESAMPLE_MAX_TAPS. */
PWG_API int pwg_resample_plan_create(int up, int down, const float* taps, int tap_count, void** plan);
PWG_API void pwg_resample_plan_destroy(void* plan);
/* Outputs per workgroup of this plan (PWG_RESAMPLE_OUT_TILE unless the LDS asks for fewer); -1 for null. */
PWG_API int pwg_resample_plan_tile(void* plan);

/* wave, sample_start: as pwg_trim_run. out: DEVICE, out_total fp32, the utterances' outputs back to back.
 * PWG_ERR_INVALID: a null plan, wave, sample_start or out, n_utts < 1, boundaries that are negative or
 *   decrease, an empty utterance, out_total that is not the sum of the output lengths, a current device
 *   other than the plan's. */
PWG_API int pwg_resample_run(void* plan, const float* wave, const long long* sample_start, int n_utts,
                             float* out, long long out_total, void* stream);

/* -------------------------------------------------------------------------------------------- fit */

/* wave: DEVICE fp32. src_start, src_len: HOST, n_utts entries each: utterance u reads
 * wave[src_start[u] .. src_start[u] + src_len[u]) and nothing else. out: DEVICE fp32; utterance u writes
 * out[out_start[u] .. out_start[u + 1]). out_start: HOST, n_utts + 1 entries. peak: DEVICE, n_utts fp32
 * (cleared inside the run), or NULL.
 * PWG_ERR_INVALID: a null wave, src_start, src_len, out or out_start, n_utts < 1, src_start[u] < 0,
 *   src_len[u] < 1, out boundaries that are negative or decrease, an empty output, a gain that is not
 *   finite. */
PWG_API int pwg_wave_fit_run(const float* wave, const long long* src_start, const long long* src_len, float* out,
                             const long long* out_start, int n_utts, float gain, float* peak, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_WAVE_H_ */
