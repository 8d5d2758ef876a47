// Front ends of the duration- and f0-conditioned token vocoders (include/pwg_embed.h; reference
// models/hifigan.py:1100-1487, layers/duration_predictor.py, layers/length_regulator.py):
//
//   pwg_durpred_layer   one DurationPredictor layer over a ragged batch of token-rate rows:
//                       Conv1d(k = 3, same padding) -> ReLU -> LayerNorm over channels, and on the
//                       last layer the Linear head with the log duration and the integer duration.
//   pwg_regulate_scan   per-utterance exclusive prefix sums and totals of the durations.
//   pwg_regulate_rows   the length-regulated gather out[r] = emb[ids[src(r)]].
//   pwg_embed_rows_f0   pwg_embed_rows with rows of dim + lin floats: a weighted sum of L tables
//                       in the token columns and f0[r] * W + b in the last lin columns.
//
// The predictor's convolution runs on the f32-input MFMA (v_mfma_f32_16x16x4_f32: an fp32 fma chain
// per output, no reduced-precision operand anywhere): the integer duration is round(exp(x) - offset),
// and an operand error of 1e-3 moves x across a rounding edge on about one token in a hundred, which
// changes the output length. A workgroup owns DP_ROWS = 16 consecutive rows and ALL output channels, so
// LayerNorm and the head read the conv result from LDS and nothing goes through HBM twice. Output
// tile of a wave: M = 16 rows x N = 16 channels per accumulator, K = 3 cin walked 4 at a time; the
// k steps alternate between DP_KCH accumulators per tile (independent MFMAs back to back), and every
// DP_FLUSH steps the accumulators are folded into a running total and restarted: an fma chain is
// then 32 products long instead of 3 cin, which keeps the log duration within about 1e-6 of a
// float64 evaluation at cin = 1024 (a single chain: 4e-6). The zero padding of the
// conv is applied per utterance: a tap that would read a row of the neighbouring utterance (or
// outside the batch) contributes zero.
//
// The two gathers follow pwg_embed_rows (pwg_embed.hip): one wave per EXT_ROWS consecutive output
// rows, everything about a row wave-uniform, lanes move 16-byte vectors.

#include <hip/hip_runtime.h>

#include <climits>
#include <string>

#include "../../include/pwg_embed.h"
#include "pwg_internal.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DP_MT = 1;       // MFMA M tiles (16 rows each) per workgroup
constexpr int DP_ROWS = 16 * DP_MT;  // rows (tokens) per workgroup
constexpr int DP_WAVES = 8;    // waves per workgroup; wave w owns channel tiles w, w + 8, ...
constexpr int DP_MAX_NT = 8;   // channel tiles per wave: cout <= 16 * DP_WAVES * DP_MAX_NT = 1024
constexpr int DP_KCH = 2;      // accumulators per tile the k steps alternate between
constexpr int DP_FLUSH = 8;    // MFMAs per accumulator (32 products) between folds into the running total
constexpr int DP_MAX_CH = 16 * DP_WAVES * DP_MAX_NT;
constexpr int DP_PAD = 4;      // LDS row padding in floats: 16 rows x 4 k land in 64 distinct banks

constexpr int EXT_WAVES = 4;   // gathers: waves per workgroup
constexpr int EXT_ROWS = 4;    // consecutive rows per wave
constexpr int SCAN_THREADS = 256;

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The last u in [0, n) with start[u] <= r (0 if none): never leaves [0, n) whatever start holds.
__device__ inline int last_le(const long long* start, int n, long long r) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ inline float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------ duration predictor layer
struct DurPredArgs {
  const float* x;        // rows x cin, or null: rows gathered from emb by ids
  const float* emb;
  const long long* ids;
  const float* w;        // [3][cin][cout]
  const float* bias;
  const float* ln_g;
  const float* ln_b;
  const float* lin_w;    // null: no head
  const float* lin_b;
  const long long* row_start;
  float* y;              // rows x cout, or null
  float* logdur;
  long long* dur;
  int* flag;
  long long rows;
  int num_embs, cin, cout, n_utts;
  float offset;
};

// The conv of one wave: NT channel tiles x DP_MT row tiles, K = 3 cin. Per pass 16 input channels:
// the 2 DP_KCH weight fragments of every tile and the A values are loaded first, then the MFMAs
// run (k order per accumulator: ascending). Every DP_FLUSH MFMAs per accumulator the chains are
// folded into the running total and restarted (blocked summation).
template <int NT>
__device__ __forceinline__ void durpred_conv(const DurPredArgs& a, const float* xrow, int xs_ld, const float* wcol,
                                             const bool (&tap_ok)[DP_MT][3], f32x4 (&tot)[DP_MT][DP_MAX_NT]) {
  f32x4 acc[DP_KCH][DP_MT][NT], sum[DP_MT][NT];
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      sum[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DP_KCH; ++c) acc[c][mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  auto fold = [&]() {
#pragma unroll
    for (int mt = 0; mt < DP_MT; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        f32x4 s = acc[0][mt][j];
#pragma unroll
        for (int c = 1; c < DP_KCH; ++c) s += acc[c][mt][j];
        sum[mt][j] += s;
#pragma unroll
        for (int c = 0; c < DP_KCH; ++c) acc[c][mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };
  int step = 0;
  for (int tap = 0; tap < 3; ++tap) {
    bool ok[DP_MT];
#pragma unroll
    for (int mt = 0; mt < DP_MT; ++mt) ok[mt] = tap == 0 ? tap_ok[mt][0] : (tap == 1 ? tap_ok[mt][1] : tap_ok[mt][2]);
    const float* xt = xrow + tap * xs_ld;
    const float* wt = wcol + (size_t)tap * a.cin * a.cout;
    for (int ci = 0; ci < a.cin; ci += 16) {
      float av[2][DP_KCH][DP_MT], b[2][DP_KCH][NT];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < DP_KCH; ++c) {
          const int k0 = ci + 8 * h + 4 * c;
#pragma unroll
          for (int j = 0; j < NT; ++j) b[h][c][j] = wt[(size_t)k0 * a.cout + j * DP_WAVES * 16];
#pragma unroll
          for (int mt = 0; mt < DP_MT; ++mt) {
            const float xv = xt[mt * 16 * xs_ld + k0];
            av[h][c][mt] = ok[mt] ? xv : 0.f;
          }
        }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < DP_KCH; ++c)
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int mt = 0; mt < DP_MT; ++mt)
              acc[c][mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h][c][mt], b[h][c][j], acc[c][mt][j], 0, 0, 0);
      if (++step == DP_FLUSH / 2) {
        step = 0;
        fold();
      }
    }
  }
  fold();
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) tot[mt][j] = sum[mt][j];
}

__global__ __launch_bounds__(64 * DP_WAVES) void pwg_durpred_layer_kernel(DurPredArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r0 = (long long)blockIdx.x * DP_ROWS;
  const int xs_ld = a.cin + DP_PAD, os_ld = a.cout + DP_PAD;

  // stage rows r0 - 1 .. r0 + DP_ROWS (the tile and one row either side); rows outside the batch
  // and rows whose id failed its check are zeros
  const int nvec = a.cin >> 2;
  for (int s = wave; s < DP_ROWS + 2; s += DP_WAVES) {
    const long long r = r0 - 1 + s;
    const float4* src = nullptr;
    if (r >= 0 && r < a.rows) {
      if (a.x != nullptr) {
        src = reinterpret_cast<const float4*>(a.x + r * a.cin);
      } else {
        const long long id = a.ids[r];
        if (id < 0 || id >= a.num_embs) {  // no address is formed from an id that failed its check
          if (lane == 0) __hip_atomic_fetch_or(a.flag, PWG_EMBED_BAD_TOKEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          src = reinterpret_cast<const float4*>(a.emb + id * a.cin);
        }
      }
    }
    float4* dst = reinterpret_cast<float4*>(lds + s * xs_ld);
    if (src != nullptr) {
      for (int v = lane; v < nvec; v += 64) dst[v] = src[v];
    } else {
      for (int v = lane; v < nvec; v += 64) dst[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  // A operand: lane l holds x[row l & 15][k = l >> 4] of each M tile; which taps of that row exist
  const int m = lane & 15, kq = lane >> 4;
  bool tap_ok[DP_MT][3];
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt) {
    const long long r = r0 + mt * 16 + m;
    tap_ok[mt][0] = tap_ok[mt][1] = tap_ok[mt][2] = false;
    if (r < a.rows) {
      const int u = last_le(a.row_start, a.n_utts, r);
      tap_ok[mt][0] = r > a.row_start[u];
      tap_ok[mt][1] = true;
      tap_ok[mt][2] = r + 1 < a.row_start[u + 1] && r + 1 < a.rows;
    }
  }
  __syncthreads();

  const int nt_total = a.cout >> 4;
  const int ntw = wave < nt_total ? (nt_total - wave + DP_WAVES - 1) / DP_WAVES : 0;
  f32x4 tot[DP_MT][DP_MAX_NT];
#pragma unroll
  for (int mt = 0; mt < DP_MT; ++mt)
#pragma unroll
    for (int j = 0; j < DP_MAX_NT; ++j) tot[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xrow = lds + m * xs_ld + kq;
  // B operand: lane l holds w[k = l >> 4][channel l & 15] of the tile
  const float* wcol = a.w + (size_t)kq * a.cout + wave * 16 + m;
  switch (ntw) {  // the tile count as a compile-time constant: a straight-line K loop
    case 1: durpred_conv<1>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 2: durpred_conv<2>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 3: durpred_conv<3>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 4: durpred_conv<4>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 5: durpred_conv<5>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 6: durpred_conv<6>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 7: durpred_conv<7>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    case 8: durpred_conv<8>(a, xrow, xs_ld, wcol, tap_ok, tot); break;
    default: break;
  }
  __syncthreads();  // every wave is done with the staged rows: the conv result takes their place

  // C/D: lane l holds channel l & 15 of rows 4 (l >> 4) + reg of each M tile
#pragma unroll
  for (int j = 0; j < DP_MAX_NT; ++j) {
    if (j < ntw) {
      const int col = (wave + j * DP_WAVES) * 16 + m;
      const float b = a.bias[col];
#pragma unroll
      for (int mt = 0; mt < DP_MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float v = tot[mt][j][reg] + b;
          lds[(mt * 16 + kq * 4 + reg) * os_ld + col] = v < 0.f ? 0.f : v;  // ReLU (a NaN stays a NaN)
        }
    }
  }
  __syncthreads();

  // LayerNorm over channels (two passes over the LDS row, biased variance, eps 1e-12) and the head
  const float inv_c = 1.f / (float)a.cout;
  for (int rr = 0; rr < DP_ROWS / DP_WAVES; ++rr) {
    const int row = wave * (DP_ROWS / DP_WAVES) + rr;
    const long long gr = r0 + row;
    if (gr >= a.rows) continue;
    const float* o = lds + row * os_ld;
    float s = 0.f;
    for (int c = lane; c < a.cout; c += 64) s += o[c];
    const float mean = wave_sum(s) * inv_c;
    float q = 0.f;
    for (int c = lane; c < a.cout; c += 64) {
      const float d = o[c] - mean;
      q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) * inv_c + 1e-12f);
    float h = 0.f;
    for (int c = lane; c < a.cout; c += 64) {
      const float v = (o[c] - mean) * rstd * a.ln_g[c] + a.ln_b[c];
      if (a.y != nullptr) a.y[gr * a.cout + c] = v;
      if (a.lin_w != nullptr) h = fmaf(v, a.lin_w[c], h);
    }
    if (a.lin_w != nullptr) {
      h = wave_sum(h) + a.lin_b[0];
      if (lane == 0) {
        a.logdur[gr] = h;
        // clamp(round(exp(x) - offset), min = 0).long(): half to even, NaN -> 0, saturating
        const float d = rintf(expf(h) - a.offset);
        a.dur[gr] = !(d > 0.f) ? 0LL : (d >= 2147483648.f ? (long long)INT_MAX : (long long)d);
      }
    }
  }
}

// ------------------------------------------------------------------ length regulator
struct ScanArgs {
  const long long* ds;
  const long long* row_start;
  long long* prefix;
  long long* totals;
  int* flag;
  long long tokens;
};

__device__ inline long long checked_duration(long long d, int* bad) {
  if (d < 0 || d > INT_MAX) {
    *bad = 1;
    return 0;
  }
  return d;
}

// One workgroup per utterance: the total (and with it the all-zero -> all-ones rule), then an
// exclusive scan in chunks of SCAN_THREADS with a running carry.
__global__ __launch_bounds__(SCAN_THREADS) void pwg_regulate_scan_kernel(ScanArgs a) {
  __shared__ long long part[SCAN_THREADS];
  const int tid = threadIdx.x;
  const int u = blockIdx.x;
  const long long b = clampll(a.row_start[u], 0, a.tokens);
  const long long e = clampll(a.row_start[u + 1], b, a.tokens);
  long long s = 0;
  int bad = 0;
  for (long long t = b + tid; t < e; t += SCAN_THREADS) s += checked_duration(a.ds[t], &bad);
  if (bad) __hip_atomic_fetch_or(a.flag, PWG_EMBED_BAD_DURATION, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  part[tid] = s;
  __syncthreads();
  for (int o = SCAN_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  const long long total = part[0];
  __syncthreads();
  const bool ones = total == 0;
  long long carry = 0;
  for (long long base = b; base < e; base += SCAN_THREADS) {
    const long long t = base + tid;
    int ignore = 0;
    const long long d = t < e ? (ones ? 1 : checked_duration(a.ds[t], &ignore)) : 0;
    part[tid] = d;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {  // inclusive scan
      const long long add = tid >= o ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (t < e) a.prefix[t] = carry + part[tid] - d;
    carry += part[SCAN_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) a.totals[u] = ones ? e - b : total;
}

struct RegulateArgs {
  const float* emb;
  const long long* ids;
  const long long* prefix;
  const long long* totals;
  const long long* row_start;
  const long long* out_start;
  float* out;
  int* flag;
  long long tokens, out_rows;
  int num_embs, dim, n_utts;
};

__global__ __launch_bounds__(64 * EXT_WAVES) void pwg_regulate_rows_kernel(RegulateArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r0 = ((long long)blockIdx.x * EXT_WAVES + wave) * EXT_ROWS;
  if (r0 >= a.out_rows) return;
  const int nvec = a.dim >> 2;
  int u = last_le(a.out_start, a.n_utts, r0);
  const long long r1 = r0 + EXT_ROWS < a.out_rows ? r0 + EXT_ROWS : a.out_rows;
  for (long long r = r0; r < r1; ++r) {
    while (u + 1 < a.n_utts && a.out_start[u + 1] <= r) ++u;
    const long long local = r - a.out_start[u];
    const long long tb = clampll(a.row_start[u], 0, a.tokens);
    const long long te = clampll(a.row_start[u + 1], tb, a.tokens);
    float4* o = reinterpret_cast<float4*>(a.out + r * a.dim);
    const float4* e = nullptr;
    if (local >= 0 && local < a.totals[u] && tb < te) {
      // the last token of the utterance whose exclusive prefix sum is <= local: among tokens with
      // equal sums (zero durations) that is the one the row belongs to; the search never leaves
      // [tb, te) whatever prefix holds
      long long lo = tb, hi = te - 1;
      while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (a.prefix[mid] <= local) lo = mid; else hi = mid - 1;
      }
      const long long id = a.ids[lo];
      if (id < 0 || id >= a.num_embs) {  // no address is formed from an id that failed its check
        if (lane == 0) __hip_atomic_fetch_or(a.flag, PWG_EMBED_BAD_TOKEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        e = reinterpret_cast<const float4*>(a.emb + id * a.dim);
      }
    }
    if (e != nullptr) {
      for (int v = lane; v < nvec; v += 64) o[v] = e[v];
    } else {  // padding past the utterance's total, or a bad id
      for (int v = lane; v < nvec; v += 64) o[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

// ------------------------------------------------------------------ f0 / weighted-sum front end
struct EmbedF0Args {
  const float* emb;
  const float* tw;   // null: one table, copied as it is
  const float* spk;
  const long long* ids;
  const long long* spk_ids;
  const long long* row_start;
  const float* f0;
  const float* lin_w;
  const float* lin_b;
  float* out;
  int* flag;
  long long rows;
  int num_embs, num_spk, dim, lin, n_tables, n_utts;
};

__global__ __launch_bounds__(64 * EXT_WAVES) void pwg_embed_rows_f0_kernel(EmbedF0Args a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r0 = ((long long)blockIdx.x * EXT_WAVES + wave) * EXT_ROWS;
  if (r0 >= a.rows) return;
  const int nvec = a.dim >> 2, lvec = a.lin >> 2, ld = a.dim + a.lin;
  const int L = a.tw != nullptr ? a.n_tables : 1;
  int u = a.spk != nullptr ? last_le(a.row_start, a.n_utts, r0) : 0;
  const long long r1 = r0 + EXT_ROWS < a.rows ? r0 + EXT_ROWS : a.rows;
  for (long long r = r0; r < r1; ++r) {
    int bad = 0;
    for (int l = 0; l < L; ++l) {
      const long long id = a.ids[r * L + l];
      if (id < 0 || id >= a.num_embs) bad = PWG_EMBED_BAD_TOKEN;
    }
    long long g = 0;
    if (a.spk != nullptr) {
      while (u + 1 < a.n_utts && a.row_start[u + 1] <= r) ++u;
      g = a.spk_ids[u];
      if (g < 0 || g >= a.num_spk) bad |= PWG_EMBED_BAD_SPEAKER;
    }
    float4* o = reinterpret_cast<float4*>(a.out + r * ld);
    if (bad) {  // no address is formed from an id that failed its check
      for (int v = lane; v < nvec + lvec; v += 64) o[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane == 0) __hip_atomic_fetch_or(a.flag, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    if (a.tw != nullptr) {  // sum_l w[l] * emb_l[ids[r][l]], one fma per table in table order
      for (int v = lane; v < nvec; v += 64) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int l = 0; l < L; ++l) {
          const float wl = a.tw[l];
          const float4 x = reinterpret_cast<const float4*>(a.emb + ((long long)l * a.num_embs + a.ids[r * L + l]) * a.dim)[v];
          s = make_float4(fmaf(wl, x.x, s.x), fmaf(wl, x.y, s.y), fmaf(wl, x.z, s.z), fmaf(wl, x.w, s.w));
        }
        o[v] = s;
      }
    } else {
      const float4* e = reinterpret_cast<const float4*>(a.emb + a.ids[r] * a.dim);
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
    if (lvec > 0) {  // Linear(1, lin): f0[r] * W + b
      const float f = a.f0[r];
      const float4* W = reinterpret_cast<const float4*>(a.lin_w);
      const float4* B = reinterpret_cast<const float4*>(a.lin_b);
      for (int v = lane; v < lvec; v += 64) {
        const float4 w = W[v], b = B[v];
        o[nvec + v] = make_float4(fmaf(f, w.x, b.x), fmaf(f, w.y, b.y), fmaf(f, w.z, b.z), fmaf(f, w.w, b.w));
      }
    }
  }
}

int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pwg::set_error(PWG_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  return PWG_OK;
}

}  // namespace

extern "C" int pwg_durpred_layer(const float* x, const float* emb, int num_embs, const long long* ids, int cin, int cout,
                                 int kernel_size, const float* w, const float* bias, const float* ln_g,
                                 const float* ln_b, const float* lin_w, const float* lin_b, float offset,
                                 const long long* row_start, int n_utts, long long rows, float* y, float* logdur,
                                 long long* dur, int* flag, void* stream) {
  using pwg::set_error;
  if (!w || !bias || !ln_g || !ln_b || !row_start || !flag)
    return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: w, bias, ln_g, ln_b, row_start and flag must not be null");
  if (x && (emb || ids)) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: give either x or emb and ids, not both");
  if (!x && (!emb || !ids)) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: without x, emb and ids must not be null");
  if (!x && num_embs < 1) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: num_embs must be >= 1");
  if (lin_w ? (!lin_b || !logdur || !dur) : (lin_b || logdur || dur))
    return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: the head needs lin_w, lin_b, logdur and dur together");
  if (!y && !lin_w) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: neither y nor the head is asked for");
  if (cin < 16 || cin % 16 || cout < 16 || cout % 16)
    return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: cin and cout must be positive multiples of 16");
  if (kernel_size < 1 || kernel_size % 2 == 0) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: kernel_size must be odd and >= 1");
  if (rows < 0 || n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: rows must be >= 0 and n_utts >= 1");
  if (!aligned16(x) || !aligned16(emb) || !aligned16(w) || !aligned16(y))
    return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: x, emb, w and y must be 16-byte aligned");
  const long long n_wg = (rows + DP_ROWS - 1) / DP_ROWS;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_durpred_layer: too many rows for one launch");
  if (kernel_size != 3) return set_error(PWG_ERR_UNSUPPORTED, "pwg_durpred_layer: only kernel_size 3 is supported");
  if (cin > DP_MAX_CH || cout > DP_MAX_CH) return set_error(PWG_ERR_UNSUPPORTED, "pwg_durpred_layer: cin and cout above 1024 are not supported");
  if (rows == 0) return PWG_OK;
  DurPredArgs a;
  a.x = x; a.emb = x ? nullptr : emb; a.ids = x ? nullptr : ids; a.w = w; a.bias = bias; a.ln_g = ln_g; a.ln_b = ln_b;
  a.lin_w = lin_w; a.lin_b = lin_b; a.row_start = row_start; a.y = y; a.logdur = logdur; a.dur = dur; a.flag = flag;
  a.rows = rows; a.num_embs = x ? 0 : num_embs; a.cin = cin; a.cout = cout; a.n_utts = n_utts; a.offset = offset;
  const int xs = (DP_ROWS + 2) * (cin + DP_PAD), os = DP_ROWS * (cout + DP_PAD);
  const size_t lds = sizeof(float) * (size_t)(xs > os ? xs : os);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pwg_durpred_layer_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_error(PWG_ERR_HIP, (std::string("pwg_durpred_layer: ") + hipGetErrorString(e)).c_str());
  }
  hipLaunchKernelGGL(pwg_durpred_layer_kernel, dim3((unsigned)n_wg), dim3(64 * DP_WAVES), lds, (hipStream_t)stream, a);
  return launched("pwg_durpred_layer");
}

extern "C" int pwg_regulate_scan(const long long* ds, const long long* row_start, int n_utts, long long tokens,
                                 long long* prefix, long long* totals, int* flag, void* stream) {
  using pwg::set_error;
  if (!ds || !row_start || !prefix || !totals || !flag)
    return set_error(PWG_ERR_INVALID, "pwg_regulate_scan: ds, row_start, prefix, totals and flag must not be null");
  if (n_utts < 1 || tokens < 0) return set_error(PWG_ERR_INVALID, "pwg_regulate_scan: n_utts must be >= 1 and tokens >= 0");
  ScanArgs a;
  a.ds = ds; a.row_start = row_start; a.prefix = prefix; a.totals = totals; a.flag = flag; a.tokens = tokens;
  hipLaunchKernelGGL(pwg_regulate_scan_kernel, dim3((unsigned)n_utts), dim3(SCAN_THREADS), 0, (hipStream_t)stream, a);
  return launched("pwg_regulate_scan");
}

extern "C" int pwg_regulate_rows(const float* emb, int num_embs, int dim, const long long* ids, const long long* prefix,
                                 const long long* totals, const long long* row_start, const long long* out_start,
                                 int n_utts, long long tokens, long long out_rows, float* out, int* flag, void* stream) {
  using pwg::set_error;
  if (!emb || !ids || !prefix || !totals || !row_start || !out_start || !out || !flag)
    return set_error(PWG_ERR_INVALID, "pwg_regulate_rows: no pointer may be null");
  if (num_embs < 1) return set_error(PWG_ERR_INVALID, "pwg_regulate_rows: num_embs must be >= 1");
  if (dim < 16 || dim % 16) return set_error(PWG_ERR_INVALID, "pwg_regulate_rows: dim must be a positive multiple of 16");
  if (n_utts < 1 || tokens < 0 || out_rows < 0)
    return set_error(PWG_ERR_INVALID, "pwg_regulate_rows: n_utts must be >= 1, tokens and out_rows >= 0");
  if (!aligned16(emb) || !aligned16(out)) return set_error(PWG_ERR_INVALID, "pwg_regulate_rows: emb and out must be 16-byte aligned");
  constexpr long long per_wg = (long long)EXT_WAVES * EXT_ROWS;
  const long long n_wg = (out_rows + per_wg - 1) / per_wg;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_regulate_rows: too many rows for one launch");
  if (out_rows == 0) return PWG_OK;
  RegulateArgs a;
  a.emb = emb; a.ids = ids; a.prefix = prefix; a.totals = totals; a.row_start = row_start; a.out_start = out_start;
  a.out = out; a.flag = flag; a.tokens = tokens; a.out_rows = out_rows; a.num_embs = num_embs; a.dim = dim; a.n_utts = n_utts;
  hipLaunchKernelGGL(pwg_regulate_rows_kernel, dim3((unsigned)n_wg), dim3(64 * EXT_WAVES), 0, (hipStream_t)stream, a);
  return launched("pwg_regulate_rows");
}

extern "C" int pwg_embed_rows_f0(const float* emb, int num_embs, int n_tables, const float* table_weights,
                                 const float* spk, int num_spk, int dim, int lin, const float* f0, const float* lin_w,
                                 const float* lin_b, const long long* ids, const long long* spk_ids,
                                 const long long* row_start, int n_utts, long long rows, float* out, int* flag,
                                 void* stream) {
  using pwg::set_error;
  if (!emb || !ids || !out || !flag) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: emb, ids, out and flag must not be null");
  if (num_embs < 1) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: num_embs must be >= 1");
  if (dim < 16 || dim % 16) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: dim must be a positive multiple of 16");
  if (lin < 0 || lin % 16) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: lin must be a non-negative multiple of 16");
  if (lin > 0 && (!f0 || !lin_w || !lin_b)) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: lin > 0 needs f0, lin_w and lin_b");
  if (rows < 0) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: rows must be >= 0");
  if (table_weights ? n_tables < 1 : (n_tables != 0 && n_tables != 1))
    return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: n_tables must be >= 1 with table_weights and 0 or 1 without");
  if (spk) {
    if (!spk_ids || !row_start) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: a speaker table needs spk_ids and row_start");
    if (num_spk < 1 || n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: a speaker table needs num_spk >= 1 and n_utts >= 1");
  } else if (num_spk < 0 || n_utts < 0) {
    return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: num_spk and n_utts must be >= 0");
  }
  if (!aligned16(emb) || !aligned16(spk) || !aligned16(out) || (lin > 0 && (!aligned16(lin_w) || !aligned16(lin_b))))
    return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: emb, spk, lin_w, lin_b and out must be 16-byte aligned");
  constexpr long long per_wg = (long long)EXT_WAVES * EXT_ROWS;
  const long long n_wg = (rows + per_wg - 1) / per_wg;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_embed_rows_f0: too many rows for one launch");
  if (table_weights && n_tables > PWG_EMBED_MAX_TABLES) return set_error(PWG_ERR_UNSUPPORTED, "pwg_embed_rows_f0: more than 16 tables are not supported");
  if (table_weights && spk) return set_error(PWG_ERR_UNSUPPORTED, "pwg_embed_rows_f0: a weighted sum with a speaker table is not supported");
  if (rows == 0) return PWG_OK;
  EmbedF0Args a;
  a.emb = emb; a.tw = table_weights; a.spk = spk; a.ids = ids; a.spk_ids = spk ? spk_ids : nullptr;
  a.row_start = spk ? row_start : nullptr; a.f0 = f0; a.lin_w = lin_w; a.lin_b = lin_b; a.out = out; a.flag = flag;
  a.rows = rows; a.num_embs = num_embs; a.num_spk = spk ? num_spk : 0; a.dim = dim; a.lin = lin;
  a.n_tables = table_weights ? n_tables : 1; a.n_utts = spk ? n_utts : 0;
  hipLaunchKernelGGL(pwg_embed_rows_f0_kernel, dim3((unsigned)n_wg), dim3(64 * EXT_WAVES), 0, (hipStream_t)stream, a);
  return launched("pwg_embed_rows_f0");
}
