/*
 * pwg_sine.h — C-ABI of the sine excitation generator (parallel_wavegan/layers/sine.py:SineGen,
 * flag_for_pulse = False), which turns f0 into the sample-rate excitation UHiFiGANGenerator reads
 * (pwg_uhg_excite_rows' x, include/pwg_uhg.h).
 *
 * The reference integrates the per-sample phase increment with fp32 cumulative sums. Here the
 * increment of every sample and channel is turned into a 64-bit fixed-point fraction of a cycle and
 * the phase is a wrapping uint64 sum: integer addition is associative, so every decomposition of the
 * sum gives the same bits, wrap-around at a full cycle is free, and there is no drift at any length.
 *
 * Per channel h in [0, dim), dim = harmonic_num + 1, everything in IEEE fp32:
 *   f_h   = f0 (h == 0), f0 * (h + 1) otherwise
 *   rad   = fmodf(f_h / sr, 1), plus 1 if negative            (torch's (f_h / sr) % 1)
 *   rad  += ini[u][h] on the first sample of utterance u only
 *   q     = floor(rad * 2^64) mod 2^64                        (uint64; rad lies in [0, 2])
 *   phase = sum of q over the utterance's samples up to and including this one, mod 2^64
 *   uv    = f0 > voiced_threshold                             (the fundamental only)
 *   noise = (uv ? noise_std : sine_amp / 3) * n
 *   sine  = sin(2 pi phase / 2^64) * sine_amp * uv + noise
 * A non-finite f0 (or one whose harmonic overflows fp32) counts as unvoiced with q = 0 and ORs
 * PWG_SINE_BAD_F0 into *flag. The phase reaches the sine's argument within 2^-26 of a cycle.
 *
 * Conventions as in pwg_embed.h: device pointers, int status codes (pwg_last_error() gives the
 * message), argument checks (PWG_ERR_INVALID, then PWG_ERR_UNSUPPORTED) before any HIP call, a
 * caller-zeroed int* flag, no allocation, no host synchronisation, graph-capturable on `stream`.
 * Separate launches only: no workgroup waits on another and every loop is bounded by the arguments.
 * Utterance boundaries read from device memory are clamped to the row range; utterance 0 owns the
 * rows before its start and the last utterance the rows after its end, and a row that garbage
 * boundaries leave outside its utterance is written as an unvoiced row of zero phase.
 */
#ifndef PWG_SINE_H_
#define PWG_SINE_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PWG_SINE_BAD_F0 = 1 };
enum { PWG_SINE_TILE = 0, PWG_SINE_HOLD = 1 };
enum { PWG_SINE_MAX_DIM = 8, PWG_SINE_SCAN_BLOCK = 1024 /* rows per workgroup of pwg_sine_samples */ };

/* Scratch bytes of pwg_sine_samples for `rows` samples in `n_utts` utterances, and of pwg_sine_frames
 * for `frames` frames (both for any dim up to PWG_SINE_MAX_DIM); -1 for negative arguments. The
 * scratch needs 8-byte alignment and no initialisation. */
PWG_API long long pwg_sine_scratch_bytes(long long rows, int n_utts);
PWG_API long long pwg_sine_frames_scratch_bytes(long long frames, int n_utts);

/* Sample-rate f0 (what SineGen.forward receives): f0 holds `rows` floats, utterance u is rows
 * [row_start[u], row_start[u + 1]) (n_utts + 1 int64 entries).
 *   ini: n_utts x dim floats or NULL (zeros); n: rows x dim standard-normal floats or NULL (no noise term)
 *   sine: rows x dim, dim innermost (the reference's (B, N, dim)); uv: rows or NULL; noise: rows x dim or NULL
 * Three launches: per-block totals of q, an exclusive scan of the block totals, and the final pass
 * (in-block scan; an utterance's phase is the running sum minus the sum before its first row, which
 * in wrapping arithmetic is exactly the sum restarted there).
 * dim outside 1..PWG_SINE_MAX_DIM or sr <= 0: PWG_ERR_UNSUPPORTED. rows == 0 is PWG_OK and launches nothing. */
PWG_API int pwg_sine_samples(const float* f0, const long long* row_start, int n_utts, long long rows, float sr,
                             int dim, float sine_amp, float noise_std, float voiced_threshold, const float* ini,
                             const float* n, float* sine, float* uv, float* noise, void* scratch,
                             long long scratch_bytes, int* flag, void* stream);

/* Frame-rate f0: `frames` floats, utterance u is frames [frame_start[u], frame_start[u + 1]) = T_u
 * frames and owns output rows [frame_start[u] * hop, frame_start[u + 1] * hop); rows = frames * hop.
 *   PWG_SINE_TILE: sample i of the utterance reads f0[i % T_u] (the contour tiled hop times: what the
 *                  reference's preprocessing builds), phase = (i / T_u) * S + P[i % T_u]
 *   PWG_SINE_HOLD: sample i reads f0[i / hop], phase = hop * (P[t] - q[t]) + (i % hop + 1) * q[t]
 * with P the inclusive prefix of q over the utterance's frames and S its total (wrapping uint64), and
 * ini folded into the first sample. Two launches: one scan per utterance over its frames, then a fully
 * parallel sample pass. Bit-identical to pwg_sine_samples on the expanded f0.
 * hop < 1, a layout other than the two, dim outside 1..PWG_SINE_MAX_DIM or sr <= 0: PWG_ERR_UNSUPPORTED.
 * frames == 0 is PWG_OK and launches nothing. */
PWG_API int pwg_sine_frames(const float* f0, const long long* frame_start, int n_utts, long long frames, int hop,
                            int layout, float sr, int dim, float sine_amp, float noise_std, float voiced_threshold,
                            const float* ini, const float* n, float* sine, float* uv, float* noise, void* scratch,
                            long long scratch_bytes, int* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_SINE_H_ */
