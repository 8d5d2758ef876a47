/*
 * pwg_vq.h — C-ABI of the VQVAE kernels (parallel_wavegan/models/vqvae.py:16-171 of the reference):
 * the encoder's first layer and grouped strided levels (MelGANDiscriminator, models/melgan.py:304-335),
 * the nearest-code search (functions/vector_quantizer.py:32-52) and the decoder's input rows.
 *
 * Every entry point is a stand-alone launch over a ragged batch of time-major rows (rows x channels
 * packed fp32, utterances back to back, row_start: n_utts + 1 int64 entries). The dense tail of the
 * encoder and the decoder run on the conv-network executor (include/pwg_cnet.h), whose `mel`
 * argument is what pwg_vq_gsconv (encoder) and pwg_vq_decode_rows (decoder) write.
 *
 * Conventions: all pointers are device pointers unless named *_host. Argument checks come before
 * any HIP call: bad arguments return PWG_ERR_INVALID, shapes outside the kernels
 * PWG_ERR_UNSUPPORTED. One launch on `stream`, no host synchronisation, no allocation. Zero rows is
 * PWG_OK and launches nothing. Every id read from device memory is range-checked before an address
 * is formed from it; a bad id ORs a PWG_VQ_BAD_* bit into *flag and its row is written as zeros.
 * row_start entries are clamped to [0, rows] on the device: no read or write leaves the buffers
 * whatever the array holds.
 *
 * Errors: int status codes as in pwg.h (pwg_last_error() gives the message).
 */
#ifndef PWG_VQ_H_
#define PWG_VQ_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWG_VQ_BAD_CODE 1   /* pwg_vq_decode_rows: a code id outside [0, num_embeds) */
#define PWG_VQ_BAD_GLOBAL 2 /* pwg_vq_decode_rows: a global id outside [0, num_global) */
#define PWG_VQ_BAD_INPUT 4  /* pwg_vq_nearest: a row of z holds a non-finite value */

/* The encoder's first layer, ReflectionPad1d((K-1)/2) + Conv1d(1 -> channels, K) + LeakyReLU:
 *   out[r][c] = LeakyReLU_slope( b[c] + sum_{k < K} w[c][k] * x[reflect_u(r - (K-1)/2 + k)] )
 * reflect_u mirrors at the first and last sample of the row's own utterance, never into a
 * neighbour. x: rows samples; w: channels x K (torch's (C, 1, K)); b: channels floats or NULL;
 * out: rows x channels, 16-byte aligned. K odd up to 31, channels a multiple of 16 with
 * channels * (K + 1) <= 16384 (the weights live in LDS), else PWG_ERR_UNSUPPORTED.
 * row_start_host: a host copy of row_start; an utterance shorter than (K-1)/2 + 1 samples is
 * PWG_ERR_INVALID (torch's reflection pad raises there too). fp32 fma chain in tap order. */
PWG_API int pwg_vq_wave_rows(const float* x, const float* w, const float* b, int channels, int kernel_size,
                             float slope, const long long* row_start, const long long* row_start_host, int n_utts,
                             long long rows, float* out, void* stream);

/* Number of floats of pwg_vq_gsconv_pack's image, -1 for an unsupported shape. */
PWG_API long long pwg_vq_gsconv_packed_count(int in_channels, int out_channels, int stride);

/* Host -> host. w: torch's (out_channels, 4, 10 stride + 1) grouped weight; packed: the kernel's
 * image [group][tap][64], one 16x4 A fragment of v_mfma_f32_16x16x4_f32 per group and tap: element
 * l holds W[16 m + (l & 15)][l >> 4][tap] when output channel 16 m + (l & 15) belongs to the group
 * and 0 otherwise, m = group * (out_channels / groups) / 16. */
PWG_API int pwg_vq_gsconv_pack(const float* w_host, int in_channels, int out_channels, int stride,
                               float* packed_host);

/* One grouped strided level, Conv1d(in, out, 10 s + 1, stride s, padding 5 s, groups in / 4) + LeakyReLU:
 *   y[o, q] = LeakyReLU_slope( b[o] + sum_{i < 4, k < 10 s + 1} W[o, i, k] * x[4 g(o) + i, q s - 5 s + k] )
 * Taps outside the utterance's own input rows read zero. x: rows_in x in_channels with row_start_in;
 * y: rows_out x out_channels with row_start_out (an utterance of n input rows has ceil(n / s) output
 * rows; the caller lays row_start_out out so). w_packed: pwg_vq_gsconv_pack's image; b: out_channels
 * floats or NULL; slope 1.0: no activation. s in 2..4, in_channels a multiple of 16, out_channels /
 * (in_channels / 4) in {4, 8, 16}, out_channels a multiple of 16 up to 1024, else
 * PWG_ERR_UNSUPPORTED. x, y and w_packed 16-byte aligned. Exact fp32 on the f32 MFMA. */
PWG_API int pwg_vq_gsconv(const float* x, const long long* row_start_in, long long rows_in, int in_channels,
                          const float* w_packed, const float* b, int out_channels, int stride, float slope,
                          float* y, const long long* row_start_out, long long rows_out, int n_utts, void* stream);

/* enorm[k] = ||e_k||^2 of the num_embeds x dim codebook: run once per codebook upload (not per
 * search); pwg_vq_nearest takes the result. */
PWG_API int pwg_vq_code_norms(const float* codebook, int num_embeds, int dim, float* enorm, void* stream);

/* idx[r] = argmin_k ( ||z_r||^2 - 2 z_r . e_k + ||e_k||^2 ), the lowest k among exactly equal
 * distances. z: rows x dim; codebook: num_embeds x dim; enorm: pwg_vq_code_norms' output; idx: rows
 * int64; zq: NULL, or rows x dim receiving codebook[idx[r]]. dim a multiple of 16 up to 1024
 * (else PWG_ERR_UNSUPPORTED), num_embeds >= 1 of any size: columns at or beyond num_embeds never win.
 * A row whose squared norm is not finite (it holds a NaN or an infinity, or overflows fp32) gives
 * index 0 and ORs PWG_VQ_BAD_INPUT into *flag. The index written is always inside [0, num_embeds).
 * The dot products run on the f32 MFMA with fp32 accumulate. z, codebook and zq 16-byte aligned. */
PWG_API int pwg_vq_nearest(const float* z, long long rows, int dim, const float* codebook, const float* enorm,
                           int num_embeds, long long* idx, float* zq, int* flag, void* stream);

/* The decoder's input rows, pwg_cnet_run's `mel` argument of D + L + G channels:
 *   out[r][0 : D]         = codebook[idx[r]]
 *   out[r][D : D+L]       = w_local . local[r] + b_local   (Conv1d(num_local, L, 1); one fma per
 *                           local channel, in channel order), or local[r] copied when w_local is NULL
 *                           (then L == num_local)
 *   out[r][D+L : D+L+G]   = glob[g_ids[u(r)]]
 * Each part is optional: codebook NULL (D ignored), local NULL (L ignored), glob NULL (G ignored); at
 * least one is present. local: rows x num_local; w_local: L x num_local; b_local: L floats or NULL.
 * D, L and G multiples of 16. A code id outside [0, num_embeds) or a global id outside
 * [0, num_global) sets PWG_VQ_BAD_CODE / PWG_VQ_BAD_GLOBAL and the whole row is zeros. row_start and
 * n_utts are needed with glob only. */
PWG_API int pwg_vq_decode_rows(const float* codebook, int num_embeds, int D, const long long* idx,
                               const float* local, int num_local, const float* w_local, const float* b_local, int L,
                               const float* glob, int num_global, int G, const long long* g_ids,
                               const long long* row_start, int n_utts, long long rows, float* out, int* flag,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_VQ_H_ */
