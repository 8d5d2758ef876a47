/*
 * pwg_embed.h — C-ABI of the token front end of the discrete-symbol vocoders
 * (DiscreteSymbolHiFiGANGenerator, parallel_wavegan/models/hifigan.py:867-1097).
 *
 * The reference turns unit ids into the generator's input features with two torch.nn.Embedding
 * lookups (models/hifigan.py:1008-1024): c = emb(ids) and, with a speaker table, c += spk_emb(g)
 * broadcast over the utterance's frames (g read from the utterance's first frame). Here that is ONE
 * launch over a ragged batch which writes the time-major feature rows the conv-network executor
 * reads as buffer 0 (pwg_cnet_run's `mel`, include/pwg_cnet.h).
 *
 * Errors: int status codes as in pwg.h (pwg_last_error() gives the message).
 */
#ifndef PWG_EMBED_H_
#define PWG_EMBED_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Status bits the kernel ORs into *flag (which the caller zeroes): a row with such an id is written
 * as zeros and the table is not read for it. */
enum { PWG_EMBED_BAD_TOKEN = 1, PWG_EMBED_BAD_SPEAKER = 2 };

/* out[r][0:dim] = emb[ids[r]][0:dim] + (spk ? spk[spk_ids[u(r)]][0:dim] : 0)   for r in [0, rows)
 * u(r) = the utterance with row_start[u] <= r < row_start[u+1]  (row_start: n_utts + 1 entries)
 * all pointers device; out is rows x dim packed fp32 = exactly pwg_cnet_run's `mel` argument.
 *
 * emb: num_embs x dim, spk: num_spk x dim or NULL (then num_spk, spk_ids, row_start and n_utts are
 * not used), both packed fp32; dim a multiple of 16 (the executor's input rule); emb, spk and out
 * 16-byte aligned. One fp32 add per element: bit-identical to torch's emb[ids] + spk[g].
 * A token id outside [0, num_embs) or a speaker id outside [0, num_spk) is checked before any
 * address is formed from it: the row is written as zeros and PWG_EMBED_BAD_TOKEN / _BAD_SPEAKER is
 * ORed into *flag. u(r) stays inside [0, n_utts) whatever row_start holds.
 * One launch on `stream`, no host synchronisation, no allocation: graph-capturable. The argument
 * checks (PWG_ERR_INVALID) come before any HIP call; rows == 0 is PWG_OK and launches nothing. */
PWG_API int pwg_embed_rows(const float* emb, int num_embs, const float* spk, int num_spk, int dim,
                           const long long* ids, const long long* spk_ids, const long long* row_start,
                           int n_utts, long long rows, float* out, int* flag, void* stream);

/* ---- Front ends of DiscreteSymbolDurationGenerator and DiscreteSymbolF0Generator
 * (models/hifigan.py:1100-1487; parallelwavegan_amd/csrc/pwg_embed_ext.hip). The conventions of
 * pwg_embed_rows hold for all four: device pointers, the argument checks (PWG_ERR_INVALID, then
 * PWG_ERR_UNSUPPORTED for shapes outside the kernels) come before any HIP call, one launch on
 * `stream`, no host synchronisation, no allocation; every id, duration and offset read from device
 * memory is checked before an address is formed from it, and a bad one ORs its bit into *flag. */
enum { PWG_EMBED_BAD_DURATION = 4, PWG_EMBED_MAX_TABLES = 16 };

/* One layer of the reference's DurationPredictor (layers/duration_predictor.py:17-88) over a ragged
 * batch of `rows` token-rate rows (utterance u = rows [row_start[u], row_start[u+1])):
 *   h[r] = LayerNorm_channels(ReLU(Conv1d_k3(in)[r] + bias)) * ln_g + ln_b      (eps 1e-12)
 * with the conv's zero padding at each utterance's own ends. Input rows: x (rows x cin fp32), or,
 * with x NULL, emb[ids[r]] (emb: num_embs x cin; an id outside [0, num_embs) reads as a zero row and
 * sets PWG_EMBED_BAD_TOKEN). w is the conv weight repacked to [tap][cin][cout] (torch's
 * (cout, cin, 3) permuted (2, 1, 0)). y (rows x cout) receives h unless NULL. With lin_w (cout
 * floats) and lin_b (1 float) the Linear head runs too: logdur[r] = h[r] . lin_w + lin_b and
 * dur[r] = max(round_half_even(exp(logdur[r]) - offset), 0) as int64 (NaN -> 0, saturating at
 * INT32_MAX). The conv is fp32 throughout (f32-input MFMA, fp32 fma chains): fp32-class error.
 * cin, cout: multiples of 16 up to 1024 and kernel_size 3, else PWG_ERR_UNSUPPORTED. x, emb, w and
 * y 16-byte aligned. rows == 0 is PWG_OK and launches nothing. */
PWG_API int pwg_durpred_layer(const float* x, const float* emb, int num_embs, const long long* ids, int cin, int cout,
                              int kernel_size, const float* w, const float* bias, const float* ln_g,
                              const float* ln_b, const float* lin_w, const float* lin_b, float offset,
                              const long long* row_start, int n_utts, long long rows, float* y, float* logdur,
                              long long* dur, int* flag, void* stream);

/* Length regulator, step 1 (layers/length_regulator.py:71-98): per utterance u the exclusive prefix
 * sums prefix[t] (t in [row_start[u], row_start[u+1]), starting at 0 for each utterance) and the
 * total totals[u] of the int64 durations ds[0:tokens]. An utterance whose durations sum to zero
 * counts as all ones. A duration outside [0, INT32_MAX] sets PWG_EMBED_BAD_DURATION and counts as
 * 0. row_start entries are clamped to [0, tokens] and to be non-decreasing. */
PWG_API int pwg_regulate_scan(const long long* ds, const long long* row_start, int n_utts, long long tokens,
                              long long* prefix, long long* totals, int* flag, void* stream);

/* Length regulator, step 2: out[r][0:dim] = emb[ids[src(r)]][0:dim] for r in [0, out_rows), where
 * utterance u owns output rows [out_start[u], out_start[u+1]) (n_utts + 1 entries), the row's
 * position in it is p = r - out_start[u], and src(r) is the token of u with prefix <= p < prefix +
 * duration. Rows with p >= totals[u] (an utterance given more output rows than its total: the
 * reference's pad_list padding) are zeros. prefix and totals as pwg_regulate_scan wrote them.
 * Bit-identical to torch.repeat_interleave(emb[ids], ds, 0). dim a multiple of 16; emb and out
 * 16-byte aligned. A token id outside [0, num_embs) gives a zero row and PWG_EMBED_BAD_TOKEN.
 * out_rows == 0 is PWG_OK and launches nothing. */
PWG_API int pwg_regulate_rows(const float* emb, int num_embs, int dim, const long long* ids, const long long* prefix,
                              const long long* totals, const long long* row_start, const long long* out_start,
                              int n_utts, long long tokens, long long out_rows, float* out, int* flag, void* stream);

/* pwg_embed_rows with rows of dim + lin floats (models/hifigan.py:1404-1455):
 *   out[r][0:dim]         = emb[ids[r]] + (spk ? spk[spk_ids[u(r)]] : 0)          (table_weights NULL;
 *                           bit-identical to pwg_embed_rows), or
 *                         = sum_l table_weights[l] * emb_l[ids[r * n_tables + l]]  (n_tables tables of
 *                           num_embs x dim packed back to back, ids (rows, n_tables) row-major, one fma
 *                           per table in table order; the weights already normalised by the host)
 *   out[r][dim:dim + lin] = f0[r] * lin_w + lin_b     (torch.nn.Linear(1, lin); lin_w, lin_b: lin floats)
 * lin is a multiple of 16 (0: no f0 columns; f0, lin_w and lin_b then unused). A row with a bad id
 * is zeros over all dim + lin columns. n_tables > PWG_EMBED_MAX_TABLES and a weighted sum with a
 * speaker table are PWG_ERR_UNSUPPORTED. emb, spk, lin_w, lin_b and out 16-byte aligned. */
PWG_API int pwg_embed_rows_f0(const float* emb, int num_embs, int n_tables, const float* table_weights,
                              const float* spk, int num_spk, int dim, int lin, const float* f0, const float* lin_w,
                              const float* lin_b, const long long* ids, const long long* spk_ids,
                              const long long* row_start, int n_utts, long long rows, float* out, int* flag,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_EMBED_H_ */
