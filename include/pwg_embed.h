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

#ifdef __cplusplus
}
#endif
#endif /* PWG_EMBED_H_ */
