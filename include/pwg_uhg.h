/*
 * pwg_uhg.h — C-ABI of the excitation front end of UHiFiGANGenerator
 * (parallel_wavegan/models/uhifigan.py:78-89, 274: input_conv = Sequential(Conv1d(1 -> C, K),
 * LeakyReLU, Dropout) over the sample-rate excitation signal; Dropout is the identity in eval).
 *
 * One launch over a ragged batch writes the time-major feature rows the conv-network executor reads
 * as its external buffer (pwg_cnet_set_external / pwg_cnet_run_ext, include/pwg_cnet.h).
 *
 * Errors: int status codes as in pwg.h (pwg_last_error() gives the message).
 */
#ifndef PWG_UHG_H_
#define PWG_UHG_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[r][c] = LeakyReLU_slope( b[c] + sum_{k < K} w[c][k] * x[r - (K-1)/2 + k] )   for r in [0, rows)
 * where a tap outside the row's own utterance [row_start[u], row_start[u+1]) reads zero (Conv1d's
 * zero padding per utterance, never the neighbouring utterance's samples).
 * x: rows fp32 samples, utterances back to back; w: channels x K packed fp32 (torch's (C, 1, K));
 * b: channels floats or NULL; row_start: n_utts + 1 int64 entries (clamped to [0, rows]); out: rows x
 * channels packed fp32, 16-byte aligned. All pointers device. channels a multiple of 16 up to 1024, K
 * odd up to 11, else PWG_ERR_UNSUPPORTED. fp32 fma chain in tap order: fp32-class error.
 * One launch on `stream`, no host synchronisation, no allocation: graph-capturable. The argument
 * checks come before any HIP call; rows == 0 is PWG_OK and launches nothing. */
PWG_API int pwg_uhg_excite_rows(const float* x, const float* w, const float* b, int channels, int kernel_size,
                                float slope, const long long* row_start, int n_utts, long long rows, float* out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_UHG_H_ */
