// Token front end of the discrete-symbol vocoders (include/pwg_embed.h): the ragged embedding
// gather out[r] = emb[ids[r]] + spk[spk_ids[u(r)]] that writes the conv-network executor's input
// rows (models/hifigan.py:1008-1024 of the reference: emb(c_idx) + spk_emb(g_idx[:, 0, 0])).
//
// A pure gather: 4 dim bytes per row go out, the tables (100 x 512, 1025 x 768 floats) stay in L2.
// One wave takes EMB_ROWS consecutive rows; everything about a row (its token id, its utterance,
// the speaker id, the bounds verdict) is wave-uniform and lives in scalar registers, the lanes only
// move 16-byte vectors: lane l copies floats [4 l, 4 l + 4) + 256 j of the row, so a wave instruction
// covers 1 KiB contiguous. The utterance of a wave's first row comes from one binary search over
// row_start; the following rows only step forward.

#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/pwg_embed.h"
#include "pwg_internal.h"

namespace {

constexpr int EMB_WAVES = 4;  // waves per workgroup
constexpr int EMB_ROWS = 4;   // consecutive rows per wave

struct EmbedArgs {
  const float* emb;
  const float* spk;  // null: no speaker table
  const long long* ids;
  const long long* spk_ids;
  const long long* row_start;
  float* out;
  int* flag;
  long long rows;
  int num_embs, num_spk, dim, n_utts;
};

__global__ __launch_bounds__(64 * EMB_WAVES) void pwg_embed_rows_kernel(EmbedArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r0 = ((long long)blockIdx.x * EMB_WAVES + wave) * EMB_ROWS;
  if (r0 >= a.rows) return;
  const int nvec = a.dim >> 2;
  int u = 0;
  if (a.spk != nullptr) {
    // the last u in [0, n_utts) with row_start[u] <= r0 (u = 0 if none: the result never leaves
    // the speaker-id array, whatever the table holds)
    int lo = 0, hi = a.n_utts - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.row_start[mid] <= r0) lo = mid; else hi = mid - 1;
    }
    u = lo;
  }
  const long long r1 = r0 + EMB_ROWS < a.rows ? r0 + EMB_ROWS : a.rows;
  for (long long r = r0; r < r1; ++r) {
    const long long id = a.ids[r];
    int bad = (id < 0 || id >= a.num_embs) ? PWG_EMBED_BAD_TOKEN : 0;
    long long g = 0;
    if (a.spk != nullptr) {
      while (u + 1 < a.n_utts && a.row_start[u + 1] <= r) ++u;
      g = a.spk_ids[u];
      if (g < 0 || g >= a.num_spk) bad |= PWG_EMBED_BAD_SPEAKER;
    }
    float4* o = reinterpret_cast<float4*>(a.out + r * a.dim);
    if (bad) {  // no address is formed from an id that failed its check
      for (int v = lane; v < nvec; v += 64) o[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane == 0) __hip_atomic_fetch_or(a.flag, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    const float4* e = reinterpret_cast<const float4*>(a.emb + id * a.dim);
    if (a.spk != nullptr) {
      const float4* s = reinterpret_cast<const float4*>(a.spk + g * a.dim);
      for (int v = lane; v < nvec; v += 64) {
        const float4 x = e[v], y = s[v];
        o[v] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
      }
    } else {
      for (int v = lane; v < nvec; v += 64) o[v] = e[v];
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int pwg_embed_rows(const float* emb, int num_embs, const float* spk, int num_spk, int dim,
                              const long long* ids, const long long* spk_ids, const long long* row_start,
                              int n_utts, long long rows, float* out, int* flag, void* stream) {
  using pwg::set_error;
  if (!emb || !ids || !out || !flag) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: emb, ids, out and flag must not be null");
  if (num_embs < 1) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: num_embs must be >= 1");
  if (dim < 16 || dim % 16) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: dim must be a positive multiple of 16");
  if (rows < 0) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: rows must be >= 0");
  if (spk) {
    if (!spk_ids || !row_start) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: a speaker table needs spk_ids and row_start");
    if (num_spk < 1 || n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: a speaker table needs num_spk >= 1 and n_utts >= 1");
  } else if (num_spk < 0 || n_utts < 0) {
    return set_error(PWG_ERR_INVALID, "pwg_embed_rows: num_spk and n_utts must be >= 0");
  }
  if (!aligned16(emb) || !aligned16(spk) || !aligned16(out)) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: emb, spk and out must be 16-byte aligned");
  constexpr long long per_wg = (long long)EMB_WAVES * EMB_ROWS;
  const long long n_wg = (rows + per_wg - 1) / per_wg;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_embed_rows: too many rows for one launch");
  if (rows == 0) return PWG_OK;
  EmbedArgs a;
  a.emb = emb; a.spk = spk; a.ids = ids; a.spk_ids = spk ? spk_ids : nullptr; a.row_start = spk ? row_start : nullptr;
  a.out = out; a.flag = flag; a.rows = rows;
  a.num_embs = num_embs; a.num_spk = spk ? num_spk : 0; a.dim = dim; a.n_utts = spk ? n_utts : 0;
  hipLaunchKernelGGL(pwg_embed_rows_kernel, dim3((unsigned)n_wg), dim3(64 * EMB_WAVES), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(PWG_ERR_HIP, hipGetErrorString(e));
  return PWG_OK;
}
