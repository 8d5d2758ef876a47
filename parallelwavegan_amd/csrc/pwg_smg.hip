// StyleMelGAN generator path (include/pwg_smg.h): the noise upsampling, the TADE
// residual blocks and the output conv of parallel_wavegan/models/style_melgan.py:18-240 and
// layers/tade_res_block.py, for a ragged batch of utterances.
//
// Tensors are time-major (rows, channels) fp32; utterance u of a tensor at rate r (rows per noise-
// upsampled row) starts at row p0[u] * r, where p0 is the prefix sum of n0 = noise_len * noise_factor.
// Every kernel takes a 2-D grid (tile or element block, utterance): a tile never spans two utterances,
// and blocks past an utterance's end leave at once.
// In a trimmed plan (PWG_SMG_PLAN_TRIM_NOISE, the token class of style_melgan.py:364-602) n0 = frames
// instead: the last noise layer keeps rows t < frames only and everything after it has exactly
// `frames` rows per utterance at rate 1.
//
// smg_conv_kernel<MT, NT, EPI>: a K-tap "same" conv as an MFMA GEMM, out[o][t] = sum_{tap, ci}
// W[o][ci][tap] * in[(t + (tap - K/2) * dil) / up][ci], zero outside the utterance's own rows.
//   * fp32 operands as fp16 hi+lo pairs, three v_mfma_f32_16x16x32_f16 per product (hi*hi, hi*lo,
//     lo*hi), fp32 accumulate. The weights are the A operand (rows = output channels, MT 16-row
//     m-tiles), packed on the host into fragment order; the input is the B operand (columns = time).
//   * The reduction runs over 16-channel chunks q = tap * cs + cb (cs = cin / 16); one MFMA (k = 32)
//     takes chunks 2 s and 2 s + 1: lanes 0-31 hold chunk 2 s, lanes 32-63 chunk 2 s + 1, 8 channels
//     per 16-lane group. An odd chunk count is padded with zero weights.
//   * A workgroup of 4 waves makes 64 * NT output rows. It first stages the rows it reads
//     (64 NT + (K - 1) dil of them, already upsampled, clamped, normalised and zero-padded) into LDS as
//     fp16 hi and lo planes, each element split once; a wave then reads its B fragments with
//     16-byte LDS reads at row (column + tap * dil).
//     smg_conv_kernel<MT, NT, EPI_PLAIN, true> is the plain conv with another staging: a row is
//     emb[ids[row]] + spk[spk_ids[utterance]], gathered while it is split into the planes.
//   * Accumulator layout (16x16 tiles): lane l, register i of m-tile m holds channel 16 m + 4 (l >> 4)
//     + i of column l & 15. The three epilogues pair m-tile m with m-tile m + MT/2 in registers.
//
// Statistics (InstanceNorm1d: biased variance over the utterance's rows, per channel): the gate
// epilogue leaves its tile in LDS and one thread per channel and 64 rows computes their (mean, M2) in
// two passes in a fixed order; smg_finalise_kernel merges an utterance's tile partials in tile order with
// Chan's formula in fp64. No floating-point atomics: the result depends on the utterance's rows only.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pwg_embed.h"
#include "../../include/pwg_smg.h"
#include "pwg_internal.h"

namespace {

using pwg::set_error;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int EPI_PLAIN = 0, EPI_MODULATE = 1, EPI_GATE = 2;
constexpr int STATS_TILE = PWG_SMG_STATS_TILE;
constexpr float IN_EPS = 1e-5f;  // torch.nn.InstanceNorm1d's default
constexpr int LDS_LIMIT = 64 * 1024;

struct SmgUtt {
  long long p0;  // prefix sum of n0
  long long f0;  // prefix sum of frames
  long long z0;  // prefix sum of noise_len
  int n0;        // rows at rate 1: noise_len * noise_factor, or frames in a trimmed plan
  int frames;
  int noise_len;
  int pad_;
};

// ------------------------------------------------------------------ the utterance table
// The plan's table reaches the workspace as kernel arguments, TABLE_CHUNK utterances per launch (as the
// PWG plan descriptors do): no copy from pageable host memory, which the runtime may make wait on the
// host for earlier work of the stream. The first launch also zeroes the run's flag.
constexpr int TABLE_CHUNK = 64;  // 64 x 40 bytes of kernel arguments

struct TableArgs {
  SmgUtt* dst;
  int* flag;  // null: none
  int first, count;
  SmgUtt utt[TABLE_CHUNK];
};

__global__ __launch_bounds__(TABLE_CHUNK) void smg_table_kernel(TableArgs a) {
  if ((int)threadIdx.x < a.count) a.dst[a.first + threadIdx.x] = a.utt[threadIdx.x];
  if (a.flag && a.first == 0 && threadIdx.x == 0) *a.flag = 0;
}

// ------------------------------------------------------------------ noise upsampling
// ConvTranspose1d(kernel 2 s, stride s, padding p = s/2 + s%2, output_padding s%2) + LeakyReLU:
// L rows -> exactly L s rows. Output row t takes input rows l1 = (t + p) / s (tap (t + p) % s) and
// l1 - 1 (tap + s). One thread per output element, channels summed in order.
struct NoiseArgs {
  const SmgUtt* utt;
  const float* in;
  const float* w;  // [2 s][cin][cout]
  const float* bias;
  float* out;
  int cin, cout, s, p, f_in;  // f_in: input rows per noise column
  float slope;
  int trim;  // the last layer of a trimmed plan: rows t < n0 only, written at row p0 + t
};

__global__ __launch_bounds__(256) void smg_noise_kernel(NoiseArgs a) {
  const SmgUtt ut = a.utt[blockIdx.y];
  const long long L = (long long)ut.noise_len * a.f_in;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= L * a.s * a.cout) return;
  const long long t = e / a.cout;
  if (a.trim && t >= ut.n0) return;
  const int o = (int)(e - t * a.cout);
  const long long l1 = (t + a.p) / a.s;
  const int k1 = (int)((t + a.p) - l1 * a.s);
  const float* in0 = a.in + ut.z0 * a.f_in * a.cin;
  float acc = a.bias[o];
  if (l1 < L) {
    const float* x = in0 + l1 * a.cin;
    const float* w = a.w + (size_t)k1 * a.cin * a.cout + o;
    for (int i = 0; i < a.cin; ++i) acc = fmaf(x[i], w[(size_t)i * a.cout], acc);
  }
  if (l1 >= 1) {
    const float* x = in0 + (l1 - 1) * a.cin;
    const float* w = a.w + (size_t)(k1 + a.s) * a.cin * a.cout + o;
    for (int i = 0; i < a.cin; ++i) acc = fmaf(x[i], w[(size_t)i * a.cout], acc);
  }
  const long long row0 = a.trim ? ut.p0 : ut.z0 * a.f_in * a.s;
  a.out[(row0 + t) * a.cout + o] = acc >= 0.f ? acc : acc * a.slope;
}

// ------------------------------------------------------------------ statistics
// (mean, M2) of `cnt` values base[r * stride], r in order: two passes, fixed order.
__device__ inline float2 tile_moments(const float* base, long long stride, int cnt) {
  float s = 0.f;
  for (int r = 0; r < cnt; ++r) s += base[r * stride];
  const float mean = s / (float)cnt;
  float m2 = 0.f;
  for (int r = 0; r < cnt; ++r) {
    const float d = base[r * stride] - mean;
    m2 = fmaf(d, d, m2);
  }
  return make_float2(mean, m2);
}

// first partial slot of utterance u for tiles of `tile` rows at `rate`: the sum over earlier
// utterances of ceil(n0 rate / tile) is at most floor(p0 rate / tile) + u
__device__ inline long long tile_base(const SmgUtt& ut, int u, int rate, int tile) {
  return ut.p0 * rate / tile + u;
}

struct StatsArgs {
  const SmgUtt* utt;
  const float* x;
  float2* partial;
  int ld, C, rate;
};

__global__ void smg_stats_kernel(StatsArgs a) {
  const int u = blockIdx.y;
  const SmgUtt ut = a.utt[u];
  const long long rows = (long long)ut.n0 * a.rate;
  const long long t0 = (long long)blockIdx.x * STATS_TILE;
  const int ch = threadIdx.x;
  if (t0 >= rows || ch >= a.C) return;
  const int cnt = (int)(rows - t0 < STATS_TILE ? rows - t0 : STATS_TILE);
  a.partial[(tile_base(ut, u, a.rate, STATS_TILE) + blockIdx.x) * a.C + ch] =
      tile_moments(a.x + (ut.p0 * a.rate + t0) * a.ld + ch, a.ld, cnt);
}

struct FinaliseArgs {
  const SmgUtt* utt;
  const float2* partial;
  float* stats;     // interleaved (mean, rstd) per (utterance, channel), or
  float* mean_out;  // separate tables when stats is null
  float* rstd_out;
  int C, rate, tile;
};

__device__ inline void chan_merge(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
  if (nb == 0.0) return;
  const double nn = n + nb, d = mb - mean;
  mean += d * nb / nn;
  m2 += m2b + d * d * n * nb / nn;
  n = nn;
}

// One workgroup per utterance; S = 1024 / C segments of consecutive tiles, each merged in tile order
// by one thread per channel, then the segments in order.
__global__ __launch_bounds__(1024) void smg_finalise_kernel(FinaliseArgs a) {
  __shared__ double sh[1024 * 3];
  const int u = blockIdx.x;
  const SmgUtt ut = a.utt[u];
  const long long rows = (long long)ut.n0 * a.rate;
  const long long ntiles = (rows + a.tile - 1) / a.tile;
  const long long base = tile_base(ut, u, a.rate, a.tile);
  const int S = 1024 / a.C;
  const int seg = threadIdx.x / a.C, ch = threadIdx.x - seg * a.C;
  if (seg < S) {
    const long long per = (ntiles + S - 1) / S;
    const long long i0 = seg * per, i1 = i0 + per < ntiles ? i0 + per : ntiles;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (long long i = i0; i < i1; ++i) {
      const long long left = rows - i * a.tile;
      const float2 p = a.partial[(base + i) * a.C + ch];
      chan_merge(n, mean, m2, (double)(left < a.tile ? left : a.tile), (double)p.x, (double)p.y);
    }
    sh[threadIdx.x * 3 + 0] = n;
    sh[threadIdx.x * 3 + 1] = mean;
    sh[threadIdx.x * 3 + 2] = m2;
  }
  __syncthreads();
  if (seg == 0) {
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int s = 0; s < S; ++s) {
      const int i = (s * a.C + ch) * 3;
      chan_merge(n, mean, m2, sh[i], sh[i + 1], sh[i + 2]);
    }
    const float rstd = (float)(1.0 / sqrt(m2 / n + (double)IN_EPS));
    const long long o = (long long)u * a.C + ch;
    if (a.stats) {
      a.stats[2 * o] = (float)mean;
      a.stats[2 * o + 1] = rstd;
    } else {
      a.mean_out[o] = (float)mean;
      a.rstd_out[o] = rstd;
    }
  }
}

// ------------------------------------------------------------------ the conv
struct ConvArgs {
  const SmgUtt* utt;
  const float* in;     // rows x cin
  const float4* w;     // fragments [step][MT][hi, lo][lane] of 8 halves
  const float* bias;   // 16 MT
  float* out;          // rows x C (C = 16 MT plain, 8 MT modulate / gate)
  const float* mean;   // first aux conv: (c - mean) / scale on read, or null
  const float* scale;
  const float* x;      // modulate: the normalised tensor, rows / xu x C; gate: the residual or null
  const float* stats;  // modulate: (mean, rstd) of x per (utterance, channel)
  float2* partial;     // gate: tile partials of what it stores
  int cin, cs, K, dil, up, rate, in_is_c, xu, gate;
};

__device__ inline void split4(const float4 v, _Float16* hi, _Float16* lo) {
  const float f[4] = {v.x, v.y, v.z, v.w};
  f16x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = (_Float16)f[i];
    l[i] = (_Float16)(f[i] - (float)h[i]);
  }
  *reinterpret_cast<f16x4*>(hi) = h;
  *reinterpret_cast<f16x4*>(lo) = l;
}

// The token front end of the first aux conv (style_melgan.py:497-505): the staged row is
// emb[ids[f0 + row]] + spk[spk_ids[u]], one fp32 add per element as pwg_embed_rows makes it. Every id
// is checked before an address is formed from it; a bad one ORs its PWG_EMBED_* bit, shifted by
// PWG_SMG_FLAG_EMBED_SHIFT, into the run's flag.
struct TokArgs {
  const float* emb;          // num_embs x cin
  const float* spk;          // num_spk x cin
  const long long* ids;      // sum frames
  const long long* spk_ids;  // n_utts
  int* flag;
  int num_embs, num_spk;
};

struct NoTokArgs {};

template <int MT, int NT, int EPI, bool TOK = false>
__global__ __launch_bounds__(256) void smg_conv_kernel(ConvArgs a, std::conditional_t<TOK, TokArgs, NoTokArgs> tok) {
  [[maybe_unused]] const auto* tk = &tok;
  extern __shared__ __attribute__((aligned(16))) unsigned char smg_smem[];
  constexpr int ROWS = 64 * NT;
  constexpr int CM = MT / 2;                         // m-tiles of one half (modulate, gate)
  constexpr int C = EPI == EPI_PLAIN ? 16 * MT : 8 * MT;  // channels stored
  const int u = blockIdx.y;
  const SmgUtt ut = a.utt[u];
  const long long rows = (long long)ut.n0 * a.rate;
  const long long t0 = (long long)blockIdx.x * ROWS;
  if (t0 >= rows) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int halo = (a.K >> 1) * a.dil;
  const int nrow = ROWS + 2 * halo;
  const int SH = a.cin + 8;  // halves per staged row: 16 bytes of padding
  _Float16* s_hi = reinterpret_cast<_Float16*>(smg_smem);
  _Float16* s_lo = s_hi + (size_t)nrow * SH;

  {  // stage rows [t0 - halo, t0 + ROWS + halo) of the (virtual, upsampled) input
    const int c4n = a.cin >> 2;
    const long long in_row0 = a.in_is_c ? ut.f0 : ut.p0 * (a.rate / a.up);
    long long sid = 0;
    bool spk_ok = false;
    if constexpr (TOK) {
      sid = tk->spk_ids[u];
      spk_ok = sid >= 0 && sid < tk->num_spk;
      if (!spk_ok) {
        sid = 0;  // never an address
        if (threadIdx.x == 0)
          __hip_atomic_fetch_or(tk->flag, PWG_EMBED_BAD_SPEAKER << PWG_SMG_FLAG_EMBED_SHIFT, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    for (int idx = threadIdx.x; idx < nrow * c4n; idx += 256) {
      const int r = idx / c4n, c4 = idx - r * c4n;
      const long long tv = t0 - halo + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (TOK) {
        if (tv >= 0 && tv < rows) {
          long long pr = tv / a.up;
          if (pr > ut.frames - 1) pr = ut.frames - 1;
          const long long id = tk->ids[in_row0 + pr];
          if (id >= 0 && id < tk->num_embs) {
            v = *reinterpret_cast<const float4*>(tk->emb + id * a.cin + 4 * c4);
            if (spk_ok) {
              const float4 g = *reinterpret_cast<const float4*>(tk->spk + sid * a.cin + 4 * c4);
              v = make_float4(v.x + g.x, v.y + g.y, v.z + g.z, v.w + g.w);
            }
          } else if (c4 == 0) {  // the row stays zero
            __hip_atomic_fetch_or(tk->flag, PWG_EMBED_BAD_TOKEN << PWG_SMG_FLAG_EMBED_SHIFT, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      } else if (tv >= 0 && tv < rows) {
        long long pr = tv / a.up;
        if (a.in_is_c && pr > ut.frames - 1) pr = ut.frames - 1;  // replicate pad
        v = *reinterpret_cast<const float4*>(a.in + (in_row0 + pr) * a.cin + 4 * c4);
        if (a.mean) {
          const float4 m = *reinterpret_cast<const float4*>(a.mean + 4 * c4);
          const float4 s = *reinterpret_cast<const float4*>(a.scale + 4 * c4);
          v = make_float4((v.x - m.x) / s.x, (v.y - m.y) / s.y, (v.z - m.z) / s.z, (v.w - m.w) / s.w);
        }
      }
      split4(v, s_hi + (size_t)r * SH + 4 * c4, s_lo + (size_t)r * SH + 4 * c4);
    }
  }
  __syncthreads();

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4;
  const int col0 = wave * 16 * NT + (lane & 15);
  const int nq = a.K * a.cs;
  const int nsteps = (nq + 1) >> 1;
  for (int s = 0; s < nsteps; ++s) {
    int q = 2 * s + (g >> 1);
    if (q >= nq) q = nq - 1;  // the padding chunk: its weights are zero
    const int tap = q / a.cs, cb = q - tap * a.cs;
    const int off = tap * a.dil * SH + cb * 16 + (g & 1) * 8;
    f16x8 bh[NT], bl[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int o = (col0 + 16 * n) * SH + off;
      bh[n] = *reinterpret_cast<const f16x8*>(s_hi + o);
      bl[n] = *reinterpret_cast<const f16x8*>(s_lo + o);
    }
    const float4* w = a.w + (size_t)s * MT * 128 + lane;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const f16x8 ah = __builtin_bit_cast(f16x8, w[m * 128]);
      const f16x8 al = __builtin_bit_cast(f16x8, w[m * 128 + 64]);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[n], acc[m][n], 0, 0, 0);
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[n], acc[m][n], 0, 0, 0);
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[n], acc[m][n], 0, 0, 0);
      }
    }
  }

  const long long out_row0 = ut.p0 * a.rate;
  if constexpr (EPI == EPI_PLAIN) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const long long tv = t0 + col0 + 16 * n;
      if (tv >= rows) continue;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int ch = 16 * m + 4 * g;
        const float4 b = *reinterpret_cast<const float4*>(a.bias + ch);
        const f32x4 v = acc[m][n];
        *reinterpret_cast<float4*>(a.out + (out_row0 + tv) * C + ch) =
            make_float4(v[0] + b.x, v[1] + b.y, v[2] + b.z, v[3] + b.w);
      }
    }
  } else if constexpr (EPI == EPI_MODULATE) {
    const long long x_row0 = ut.p0 * (a.rate / a.xu);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const long long tv = t0 + col0 + 16 * n;
      if (tv >= rows) continue;
#pragma unroll
      for (int m = 0; m < CM; ++m) {
        const int ch = 16 * m + 4 * g;
        const float4 b1 = *reinterpret_cast<const float4*>(a.bias + ch);
        const float4 b2 = *reinterpret_cast<const float4*>(a.bias + C + ch);
        const float4 xv = *reinterpret_cast<const float4*>(a.x + (x_row0 + tv / a.xu) * C + ch);
        const float4 st0 = *reinterpret_cast<const float4*>(a.stats + ((size_t)u * C + ch) * 2);
        const float4 st1 = *reinterpret_cast<const float4*>(a.stats + ((size_t)u * C + ch) * 2 + 4);
        const f32x4 p = acc[m][n], q = acc[m + CM][n];
        float4 y;
        y.x = (p[0] + b1.x) * ((xv.x - st0.x) * st0.y) + (q[0] + b2.x);
        y.y = (p[1] + b1.y) * ((xv.y - st0.z) * st0.w) + (q[1] + b2.y);
        y.z = (p[2] + b1.z) * ((xv.z - st1.x) * st1.y) + (q[2] + b2.z);
        y.w = (p[3] + b1.w) * ((xv.w - st1.z) * st1.w) + (q[3] + b2.w);
        *reinterpret_cast<float4*>(a.out + (out_row0 + tv) * C + ch) = y;
      }
    }
  } else {
    constexpr int SS = C + 4;  // floats per row of the statistics tile
    float* stage = reinterpret_cast<float*>(smg_smem);
    const long long x_row0 = ut.p0 * (a.rate / a.xu);
    __syncthreads();  // every wave is done with the staged input: the tile takes its place
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int col = col0 + 16 * n;
      const long long tv = t0 + col;
      float ga[CM][4];
#pragma unroll
      for (int m = 0; m < CM; ++m) {
        const float4 b1 = *reinterpret_cast<const float4*>(a.bias + 16 * m + 4 * g);
        ga[m][0] = acc[m][n][0] + b1.x;
        ga[m][1] = acc[m][n][1] + b1.y;
        ga[m][2] = acc[m][n][2] + b1.z;
        ga[m][3] = acc[m][n][3] + b1.w;
      }
      if (a.gate == PWG_SMG_GATE_SOFTMAX) {
        // a column's C channels: CM m-tiles x 4 registers here, and the other three 16-lane groups
        float mx = ga[0][0];
#pragma unroll
        for (int m = 0; m < CM; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) mx = fmaxf(mx, ga[m][i]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < CM; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            ga[m][i] = expf(ga[m][i] - mx);
            sum += ga[m][i];
          }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.f / sum;
#pragma unroll
        for (int m = 0; m < CM; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) ga[m][i] *= inv;
      } else {
#pragma unroll
        for (int m = 0; m < CM; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) ga[m][i] = 1.f / (1.f + expf(-ga[m][i]));
      }
      if (tv < rows) {
#pragma unroll
        for (int m = 0; m < CM; ++m) {
          const int ch = 16 * m + 4 * g;
          const float4 b2 = *reinterpret_cast<const float4*>(a.bias + C + ch);
          float4 y;
          y.x = ga[m][0] * tanhf(acc[m + CM][n][0] + b2.x);
          y.y = ga[m][1] * tanhf(acc[m + CM][n][1] + b2.y);
          y.z = ga[m][2] * tanhf(acc[m + CM][n][2] + b2.z);
          y.w = ga[m][3] * tanhf(acc[m + CM][n][3] + b2.w);
          if (a.x) {
            const float4 r = *reinterpret_cast<const float4*>(a.x + (x_row0 + tv / a.xu) * C + ch);
            y = make_float4(r.x + y.x, r.y + y.y, r.z + y.z, r.w + y.w);
          }
          *reinterpret_cast<float4*>(a.out + (out_row0 + tv) * C + ch) = y;
          *reinterpret_cast<float4*>(stage + col * SS + ch) = y;
        }
      }
    }
    __syncthreads();
    // partials are per 64 rows whatever NT is: an utterance's statistics do not depend on the tile
    // size, which follows the longest utterance of the batch
    if ((int)threadIdx.x < C * NT) {
      const int sub = threadIdx.x / C, ch = threadIdx.x - sub * C;
      const long long left = rows - t0 - 64 * sub;
      if (left > 0)
        a.partial[(tile_base(ut, u, a.rate, 64) + blockIdx.x * NT + sub) * C + ch] =
            tile_moments(stage + 64 * sub * SS + ch, SS, (int)(left < 64 ? left : 64));
    }
  }
}

// ------------------------------------------------------------------ output conv + tanh
struct OutArgs {
  const SmgUtt* utt;
  const float* x;  // rows x C at rate hop
  const float* w;  // [K][C][oc]
  const float* bias;
  float* out;
  int* flag;
  int C, oc, K, hop;
};

__global__ __launch_bounds__(256) void smg_output_kernel(OutArgs a) {
  const SmgUtt ut = a.utt[blockIdx.y];
  const long long rows = (long long)ut.n0 * a.hop;      // what the conv sees
  const long long keep = (long long)ut.frames * a.hop;  // what is kept
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= keep * a.oc) return;
  const long long t = e / a.oc;
  const int o = (int)(e - t * a.oc);
  float acc = a.bias[o];
  for (int k = 0; k < a.K; ++k) {
    const long long tv = t + k - (a.K >> 1);
    if (tv < 0 || tv >= rows) continue;
    const float4* x = reinterpret_cast<const float4*>(a.x + (ut.p0 * a.hop + tv) * a.C);
    const float* w = a.w + (size_t)k * a.C * a.oc + o;
    for (int c4 = 0; c4 < a.C >> 2; ++c4) {  // channels in order, four per load
      const float4 v = x[c4];
      acc = fmaf(v.x, w[(size_t)(4 * c4) * a.oc], acc);
      acc = fmaf(v.y, w[(size_t)(4 * c4 + 1) * a.oc], acc);
      acc = fmaf(v.z, w[(size_t)(4 * c4 + 2) * a.oc], acc);
      acc = fmaf(v.w, w[(size_t)(4 * c4 + 3) * a.oc], acc);
    }
  }
  const float y = tanhf(acc);
  a.out[(ut.f0 * a.hop + t) * a.oc + o] = y;
  if (!(fabsf(y) <= 1.f)) __hip_atomic_fetch_or(a.flag, PWG_SMG_FLAG_NONFINITE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ host side
struct ConvSpec {
  int cin, cout, K;
  long long ref_w, ref_b;     // offsets in the reference order (ref_b < 0: none)
  long long pk_w, pk_b;       // offsets in the packed image (floats)
  int mt, cs, nsteps;         // fragment convs only
};

inline long long align64(long long n) { return (n + 63) / 64 * 64; }

uint16_t half_bits(float v) {
  const _Float16 h = (_Float16)v;
  uint16_t b;
  std::memcpy(&b, &h, 2);
  return b;
}

float half_value(uint16_t b) {
  _Float16 h;
  std::memcpy(&h, &b, 2);
  return (float)h;
}

}  // namespace

struct PwgSmg {
  PwgSmgConfig cfg;
  int device;
  int nblocks, noise_factor, hop;
  std::vector<ConvSpec> noise;  // transposed convs
  std::vector<ConvSpec> convs;  // 6 per block
  ConvSpec outc;
  long long ref_total, packed_total;
  bool timing = false;
  struct Span { int kind; hipEvent_t e0, e1; };
  std::vector<Span> spans;
};

struct PwgSmgPlan {
  const PwgSmg* g;
  int n_utts;
  bool trim;  // PWG_SMG_PLAN_TRIM_NOISE
  std::vector<SmgUtt> utts;
  long long tot_n0, tot_frames, tot_z, max_n0, max_frames, max_z;
  // workspace offsets in bytes
  long long ws_utt, ws_flag, ws_partial, ws_noise[2], ws_c1, ws_cab[2], ws_y, ws_x1, ws_bytes;
  std::vector<long long> ws_x;      // nblocks + 1
  std::vector<long long> ws_stats;  // 2 per block, + 1
  std::vector<int> rate;            // nblocks + 1
};

namespace {

int conv_lds_bytes(int cin, int K, int dil, int nt, int epi, int C) {
  const int in = (64 * nt + (K - 1) * dil) * (cin + 8) * 2 * 2;
  const int st = epi == EPI_GATE ? 64 * nt * (C + 4) * 4 : 0;
  return in > st ? in : st;
}

template <int MT, int NT, int EPI>
hipError_t launch_conv_inst(const ConvArgs& a, dim3 grid, int lds, hipStream_t s) {
  auto kfn = smg_conv_kernel<MT, NT, EPI>;
  const hipError_t e = pwg::allow_lds(reinterpret_cast<const void*>(kfn), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kfn, grid, dim3(256), (size_t)lds, s, a, NoTokArgs{});
  return hipGetLastError();
}

template <int MT, int EPI>
hipError_t launch_conv_nt(const ConvArgs& a, int nt, dim3 grid, int lds, hipStream_t s) {
  return nt == 2 ? launch_conv_inst<MT, 2, EPI>(a, grid, lds, s) : launch_conv_inst<MT, 1, EPI>(a, grid, lds, s);
}

template <int MT, int NT>
hipError_t launch_tok_inst(const ConvArgs& a, const TokArgs& tk, dim3 grid, int lds, hipStream_t s) {
  auto kfn = smg_conv_kernel<MT, NT, EPI_PLAIN, true>;
  const hipError_t e = pwg::allow_lds(reinterpret_cast<const void*>(kfn), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kfn, grid, dim3(256), (size_t)lds, s, a, tk);
  return hipGetLastError();
}

template <int MT>
hipError_t launch_tok_nt(const ConvArgs& a, const TokArgs& tk, int nt, dim3 grid, int lds, hipStream_t s) {
  return nt == 2 ? launch_tok_inst<MT, 2>(a, tk, grid, lds, s) : launch_tok_inst<MT, 1>(a, tk, grid, lds, s);
}

// mt: 16-row m-tiles of the conv's output (C / 16 plain, 2 C / 16 modulate and gate); tk: the token
// staging of the first aux conv (plain only), or null
hipError_t launch_conv(const ConvArgs& a, const TokArgs* tk, int mt, int nt, int epi, dim3 grid, int lds,
                       hipStream_t s) {
  if (tk) {
    if (epi != EPI_PLAIN) return hipErrorInvalidValue;
    switch (mt) {
      case 1: return launch_tok_nt<1>(a, *tk, nt, grid, lds, s);
      case 2: return launch_tok_nt<2>(a, *tk, nt, grid, lds, s);
      case 3: return launch_tok_nt<3>(a, *tk, nt, grid, lds, s);
      case 4: return launch_tok_nt<4>(a, *tk, nt, grid, lds, s);
    }
    return hipErrorInvalidValue;
  }
  if (epi == EPI_PLAIN) {
    switch (mt) {
      case 1: return launch_conv_nt<1, EPI_PLAIN>(a, nt, grid, lds, s);
      case 2: return launch_conv_nt<2, EPI_PLAIN>(a, nt, grid, lds, s);
      case 3: return launch_conv_nt<3, EPI_PLAIN>(a, nt, grid, lds, s);
      case 4: return launch_conv_nt<4, EPI_PLAIN>(a, nt, grid, lds, s);
    }
  } else if (epi == EPI_MODULATE) {
    switch (mt) {
      case 2: return launch_conv_nt<2, EPI_MODULATE>(a, nt, grid, lds, s);
      case 4: return launch_conv_nt<4, EPI_MODULATE>(a, nt, grid, lds, s);
      case 6: return launch_conv_nt<6, EPI_MODULATE>(a, nt, grid, lds, s);
      case 8: return launch_conv_nt<8, EPI_MODULATE>(a, nt, grid, lds, s);
    }
  } else {
    switch (mt) {
      case 2: return launch_conv_nt<2, EPI_GATE>(a, nt, grid, lds, s);
      case 4: return launch_conv_nt<4, EPI_GATE>(a, nt, grid, lds, s);
      case 6: return launch_conv_nt<6, EPI_GATE>(a, nt, grid, lds, s);
      case 8: return launch_conv_nt<8, EPI_GATE>(a, nt, grid, lds, s);
    }
  }
  return hipErrorInvalidValue;
}

int hipf(hipError_t e, const char* what) {
  const std::string m = std::string(what) + ": " + hipGetErrorString(e);
  return set_error(PWG_ERR_HIP, m.c_str());
}

// 64 NT rows per workgroup: 128 where some utterance has more than 64 rows and the staged input fits
int pick_nt(long long max_rows, int cin, int K, int dil, int epi, int C) {
  if (max_rows > 64 && conv_lds_bytes(cin, K, dil, 2, epi, C) <= LDS_LIMIT) return 2;
  return 1;
}

hipError_t upload_table(const std::vector<SmgUtt>& utts, SmgUtt* dst, int* flag, hipStream_t s) {
  const int n = (int)utts.size();
  for (int first = 0; first < n; first += TABLE_CHUNK) {
    TableArgs a;
    a.dst = dst; a.flag = flag; a.first = first;
    a.count = n - first < TABLE_CHUNK ? n - first : TABLE_CHUNK;
    std::memcpy(a.utt, utts.data() + first, sizeof(SmgUtt) * a.count);
    if (a.count < TABLE_CHUNK) std::memset(a.utt + a.count, 0, sizeof(SmgUtt) * (TABLE_CHUNK - a.count));
    hipLaunchKernelGGL(smg_table_kernel, dim3(1), dim3(TABLE_CHUNK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// pwg_smg_run / pwg_smg_debug_stats launch on the current device: refuse another one
int check_device(int want, const char* who) {
  int cur = -1;
  const hipError_t e = hipGetDevice(&cur);
  if (e != hipSuccess) return set_error(PWG_ERR_HIP, hipGetErrorString(e));
  if (cur != want) {
    const std::string m = std::string(who) + ": the handle was created for device " + std::to_string(want) +
                          " but device " + std::to_string(cur) + " is current";
    return set_error(PWG_ERR_INVALID, m.c_str());
  }
  return PWG_OK;
}

struct Runner {
  PwgSmg* g;
  hipStream_t s;
  int rc = PWG_OK;
  void begin(int kind) {
    if (!g || !g->timing || rc != PWG_OK) return;
    PwgSmg::Span sp;
    sp.kind = kind;
    if (hipEventCreate(&sp.e0) != hipSuccess) return;
    if (hipEventCreate(&sp.e1) != hipSuccess) {
      (void)hipEventDestroy(sp.e0);
      return;
    }
    (void)hipEventRecord(sp.e0, s);
    g->spans.push_back(sp);
    open = true;
  }
  void end(hipError_t e, const char* what) {
    if (open) (void)hipEventRecord(g->spans.back().e1, s);
    open = false;
    if (e != hipSuccess && rc == PWG_OK) rc = hipf(e, what);
  }
  bool open = false;
};

void run_stats(Runner& r, const SmgUtt* utt, int n_utts, long long max_n0, const float* x, int ld, int C, int rate,
               float2* partial, float* stats, float* mean_out, float* rstd_out) {
  if (r.rc != PWG_OK) return;
  StatsArgs sa{utt, x, partial, ld, C, rate};
  const long long tiles = (max_n0 * rate + STATS_TILE - 1) / STATS_TILE;
  r.begin(PWG_SMG_KIND_STATS);
  hipLaunchKernelGGL(smg_stats_kernel, dim3((unsigned)tiles, (unsigned)n_utts), dim3((unsigned)((C + 63) / 64 * 64)), 0,
                     r.s, sa);
  r.end(hipGetLastError(), "statistics kernel");
  if (r.rc != PWG_OK) return;
  FinaliseArgs fa{utt, partial, stats, mean_out, rstd_out, C, rate, STATS_TILE};
  r.begin(PWG_SMG_KIND_FINALISE);
  hipLaunchKernelGGL(smg_finalise_kernel, dim3((unsigned)n_utts), dim3(1024), 0, r.s, fa);
  r.end(hipGetLastError(), "statistics finalise kernel");
}

}  // namespace

extern "C" {

int pwg_smg_create(const PwgSmgConfig* c, int device, PwgSmg** out) {
  if (!c || !out) return set_error(PWG_ERR_INVALID, "pwg_smg_create: null argument");
  *out = nullptr;
  if (c->in_channels < 1 || c->out_channels < 1 || c->dilation < 1)
    return set_error(PWG_ERR_INVALID, "pwg_smg_create: in_channels, out_channels and dilation must be >= 1");
  if (c->channels < 16 || c->channels % 16 || c->channels > 64)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_smg_create: channels must be a multiple of 16 and at most 64");
  if (c->aux_channels < 16 || c->aux_channels % 16 || c->aux_channels > 128)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_smg_create: aux_channels must be a multiple of 16 and at most 128");
  if (c->kernel_size < 1 || c->kernel_size % 2 == 0 || c->kernel_size > 11)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_smg_create: kernel_size must be odd and at most 11");
  if (c->gate != PWG_SMG_GATE_SOFTMAX && c->gate != PWG_SMG_GATE_SIGMOID)
    return set_error(PWG_ERR_INVALID, "pwg_smg_create: unknown gate function");
  if (c->num_noise_scales < 1 || c->num_noise_scales > PWG_SMG_MAX_SCALES || c->num_scales < 1 ||
      c->num_scales > PWG_SMG_MAX_SCALES)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_smg_create: 1 to 16 noise scales and upsample scales");
  long long nf = 1, hop = 1;
  for (int i = 0; i < c->num_noise_scales; ++i) {
    if (c->noise_scales[i] < 1) return set_error(PWG_ERR_INVALID, "pwg_smg_create: noise scales must be >= 1");
    nf *= c->noise_scales[i];
  }
  for (int i = 0; i < c->num_scales; ++i) {
    if (c->upsample_scales[i] < 1) return set_error(PWG_ERR_INVALID, "pwg_smg_create: upsample scales must be >= 1");
    hop *= c->upsample_scales[i];
  }
  if (nf > (1 << 20) || hop > (1 << 20)) return set_error(PWG_ERR_UNSUPPORTED, "pwg_smg_create: scale product too large");
  const int C = c->channels, K = c->kernel_size;
  if (conv_lds_bytes(c->aux_channels, K, 1, 1, EPI_PLAIN, C) > LDS_LIMIT ||
      conv_lds_bytes(C, K, c->dilation, 1, EPI_GATE, C) > LDS_LIMIT)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_smg_create: the dilated taps of one tile do not fit the 64 KiB of LDS");
  if (device >= 0) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) return set_error(PWG_ERR_HIP, "pwg_smg_create: no such device");
  }
  PwgSmg* g = new PwgSmg();
  g->cfg = *c;
  g->device = device;
  g->nblocks = c->num_scales;
  g->noise_factor = (int)nf;
  g->hop = (int)hop;
  long long ref = 0, pk = 0;
  const bool bias = c->bias != 0;
  int cin = c->in_channels;
  for (int i = 0; i < c->num_noise_scales; ++i) {
    ConvSpec s{};
    s.cin = cin; s.cout = C; s.K = 2 * c->noise_scales[i];
    const long long n = (long long)s.cin * s.cout * s.K;
    s.ref_w = ref; ref += n;
    s.ref_b = bias ? ref : -1; if (bias) ref += s.cout;
    s.pk_w = pk; pk += align64(n);
    s.pk_b = pk; pk += align64(s.cout);
    g->noise.push_back(s);
    cin = C;
  }
  int aux = c->aux_channels;
  for (int b = 0; b < g->nblocks; ++b) {
    const int cins[6] = {aux, C, C, C, C, C};
    const int couts[6] = {C, 2 * C, 2 * C, C, 2 * C, 2 * C};
    for (int j = 0; j < 6; ++j) {
      ConvSpec s{};
      s.cin = cins[j]; s.cout = couts[j]; s.K = K;
      const long long n = (long long)s.cin * s.cout * s.K;
      s.ref_w = ref; ref += n;
      s.ref_b = bias ? ref : -1; if (bias) ref += s.cout;
      s.mt = s.cout / 16; s.cs = s.cin / 16; s.nsteps = (K * s.cs + 1) / 2;
      s.pk_w = pk; pk += (long long)s.nsteps * s.mt * 2 * 64 * 4;
      s.pk_b = pk; pk += align64(s.cout);
      g->convs.push_back(s);
    }
    aux = C;
  }
  {
    ConvSpec s{};
    s.cin = C; s.cout = c->out_channels; s.K = K;
    const long long n = (long long)s.cin * s.cout * s.K;
    s.ref_w = ref; ref += n;
    s.ref_b = bias ? ref : -1; if (bias) ref += s.cout;
    s.pk_w = pk; pk += align64(n);
    s.pk_b = pk; pk += align64(s.cout);
    g->outc = s;
  }
  g->ref_total = ref;
  g->packed_total = pk;
  *out = g;
  return PWG_OK;
}

void pwg_smg_destroy(PwgSmg* g) {
  if (!g) return;
  for (auto& sp : g->spans) {
    (void)hipEventDestroy(sp.e0);
    (void)hipEventDestroy(sp.e1);
  }
  delete g;
}

long long pwg_smg_ref_weight_count(const PwgSmg* g) { return g ? g->ref_total : -1; }
long long pwg_smg_packed_weight_count(const PwgSmg* g) { return g ? g->packed_total : -1; }

int pwg_smg_pack_weights(const PwgSmg* g, const float* ref, float* packed) {
  if (!g || !ref || !packed) return set_error(PWG_ERR_INVALID, "pwg_smg_pack_weights: null argument");
  std::memset(packed, 0, sizeof(float) * (size_t)g->packed_total);
  long long overflow = 0;
  auto put_bias = [&](const ConvSpec& s) {
    if (s.ref_b >= 0) std::memcpy(packed + s.pk_b, ref + s.ref_b, sizeof(float) * s.cout);
  };
  for (const ConvSpec& s : g->noise) {  // torch (cin, cout, k) -> [k][cin][cout]
    for (int i = 0; i < s.cin; ++i)
      for (int o = 0; o < s.cout; ++o)
        for (int k = 0; k < s.K; ++k)
          packed[s.pk_w + ((long long)k * s.cin + i) * s.cout + o] = ref[s.ref_w + ((long long)i * s.cout + o) * s.K + k];
    put_bias(s);
  }
  for (const ConvSpec& s : g->convs) {  // torch (cout, cin, k) -> fragments
    uint16_t* dst = reinterpret_cast<uint16_t*>(packed + s.pk_w);
    const int nq = s.K * s.cs;
    for (int st = 0; st < s.nsteps; ++st)
      for (int m = 0; m < s.mt; ++m)
        for (int lane = 0; lane < 64; ++lane) {
          const int o = 16 * m + (lane & 15), gq = lane >> 4;
          const int q = 2 * st + (gq >> 1);
          uint16_t* hi = dst + (((size_t)st * s.mt + m) * 2 * 64 + lane) * 8;
          uint16_t* lo = hi + 64 * 8;
          for (int j = 0; j < 8; ++j) {
            float v = 0.f;
            if (q < nq) {
              const int tap = q / s.cs, ci = (q % s.cs) * 16 + (gq & 1) * 8 + j;
              v = ref[s.ref_w + ((long long)o * s.cin + ci) * s.K + tap];
            }
            const uint16_t h = half_bits(v);
            if ((h & 0x7c00u) == 0x7c00u) ++overflow;
            hi[j] = h;
            lo[j] = half_bits(v - half_value(h));
          }
        }
    put_bias(s);
  }
  {
    const ConvSpec& s = g->outc;  // torch (oc, C, k) -> [k][C][oc]
    for (int o = 0; o < s.cout; ++o)
      for (int i = 0; i < s.cin; ++i)
        for (int k = 0; k < s.K; ++k)
          packed[s.pk_w + ((long long)k * s.cin + i) * s.cout + o] = ref[s.ref_w + ((long long)o * s.cin + i) * s.K + k];
    put_bias(s);
  }
  if (overflow) {
    const std::string m = std::to_string(overflow) +
                          " weight(s) beyond the fp16 pair range (|w| >= 65520 or not finite): this path has no "
                          "exact-fp32 mode";
    return set_error(PWG_ERR_RANGE, m.c_str());
  }
  return PWG_OK;
}

int pwg_smg_plan_create(const PwgSmg* g, int n_utts, const long long* frames, const long long* noise_len,
                        PwgSmgPlan** out) {
  return pwg_smg_plan_create_ex(g, n_utts, frames, noise_len, 0, out);
}

int pwg_smg_plan_create_ex(const PwgSmg* g, int n_utts, const long long* frames, const long long* noise_len, int flags,
                           PwgSmgPlan** out) {
  if (!g || !frames || !noise_len || !out) return set_error(PWG_ERR_INVALID, "pwg_smg_plan_create: null argument");
  *out = nullptr;
  if (flags & ~PWG_SMG_PLAN_TRIM_NOISE) return set_error(PWG_ERR_INVALID, "pwg_smg_plan_create_ex: unknown flags");
  if (n_utts < 1 || n_utts > 65535) return set_error(PWG_ERR_INVALID, "pwg_smg_plan_create: 1 to 65535 utterances");
  const bool trim = (flags & PWG_SMG_PLAN_TRIM_NOISE) != 0;
  PwgSmgPlan* p = new PwgSmgPlan();
  p->g = g;
  p->n_utts = n_utts;
  p->trim = trim;
  long long p0 = 0, f0 = 0, z0 = 0, mn = 0, mf = 0, mz = 0;
  for (int u = 0; u < n_utts; ++u) {
    const long long cover = noise_len[u] * g->noise_factor;
    const long long n0 = trim ? frames[u] : cover;
    const char* err = nullptr;
    if (frames[u] < 1) err = "pwg_smg_plan_create: every utterance needs at least one frame";
    else if (trim && frames[u] < 2)
      err = "pwg_smg_plan_create_ex: a trimmed plan needs at least two frames per utterance (instance norm over one "
            "row is undefined; the reference raises)";
    else if (noise_len[u] < 1 || cover < frames[u])
      err = "pwg_smg_plan_create: noise_len * noise_upsample_factor must cover the utterance's frames";
    else if (cover * g->hop > (1LL << 30)) err = "pwg_smg_plan_create: utterance too long";
    if (err) {
      delete p;
      return set_error(PWG_ERR_INVALID, err);
    }
    SmgUtt ut{p0, f0, z0, (int)n0, (int)frames[u], (int)noise_len[u], 0};
    p->utts.push_back(ut);
    p0 += n0; f0 += frames[u]; z0 += noise_len[u];
    mn = n0 > mn ? n0 : mn; mf = frames[u] > mf ? frames[u] : mf; mz = noise_len[u] > mz ? noise_len[u] : mz;
  }
  p->tot_n0 = p0; p->tot_frames = f0; p->tot_z = z0; p->max_n0 = mn; p->max_frames = mf; p->max_z = mz;
  const int C = g->cfg.channels;
  p->rate.push_back(1);
  for (int b = 0; b < g->nblocks; ++b) p->rate.push_back(p->rate.back() * g->cfg.upsample_scales[b]);
  long long o = 0;
  auto take = [&](long long bytes) { const long long at = o; o += (bytes + 255) / 256 * 256; return at; };
  p->ws_utt = take((long long)sizeof(SmgUtt) * n_utts);
  p->ws_flag = take(256);
  const long long big = p0 * g->hop * C * 4;  // one tensor at the final rate
  p->ws_partial = take((p0 * g->hop / 64 + n_utts + 1) * C * 8);
  // the noise layers before the last: noise_len * (product of all but the last scale) rows each, which is
  // at most p0 rows only while p0 == tot_z * noise_factor
  const long long mid_rows = trim ? z0 * (g->noise_factor / g->cfg.noise_scales[g->cfg.num_noise_scales - 1]) : p0;
  p->ws_noise[0] = take(mid_rows * C * 4);
  p->ws_noise[1] = take(mid_rows * C * 4);
  for (int b = 0; b <= g->nblocks; ++b) p->ws_x.push_back(take(p0 * p->rate[b] * C * 4));
  for (int i = 0; i <= 2 * g->nblocks; ++i) p->ws_stats.push_back(take((long long)n_utts * C * 8));
  p->ws_c1 = take(big);
  p->ws_cab[0] = take(big);
  p->ws_cab[1] = take(big);
  p->ws_y = take(big);
  p->ws_x1 = take(big);
  p->ws_bytes = o;
  *out = p;
  return PWG_OK;
}

void pwg_smg_plan_destroy(PwgSmgPlan* p) { delete p; }
long long pwg_smg_plan_workspace_bytes(const PwgSmgPlan* p) { return p ? p->ws_bytes : -1; }
long long pwg_smg_plan_out_rows(const PwgSmgPlan* p) { return p ? p->tot_frames * p->g->hop : -1; }

int pwg_smg_plan_tensor(const PwgSmgPlan* p, int block, int which, long long* offset_bytes, long long* rows, int* ld) {
  if (!p || !offset_bytes || !rows || !ld) return set_error(PWG_ERR_INVALID, "pwg_smg_plan_tensor: null argument");
  if (block < 0 || block >= p->g->nblocks) return set_error(PWG_ERR_INVALID, "pwg_smg_plan_tensor: no such block");
  const int C = p->g->cfg.channels;
  switch (which) {
    case PWG_SMG_BLOCK_X_IN:
    case PWG_SMG_BLOCK_X_OUT: {
      const int b = block + (which == PWG_SMG_BLOCK_X_OUT);
      *offset_bytes = p->ws_x[b]; *rows = p->tot_n0 * p->rate[b]; *ld = C;
      return PWG_OK;
    }
    case PWG_SMG_BLOCK_STATS_IN:
    case PWG_SMG_BLOCK_STATS_MID:
      *offset_bytes = p->ws_stats[2 * block + (which == PWG_SMG_BLOCK_STATS_MID)]; *rows = p->n_utts; *ld = 2 * C;
      return PWG_OK;
  }
  return set_error(PWG_ERR_INVALID, "pwg_smg_plan_tensor: no such tensor");
}

// The launches of pwg_smg_run (c, with mean and scale or without) and of pwg_smg_run_tokens (tok; its flag
// pointer is filled in here). The callers have checked their arguments.
static int run_launches(const PwgSmgPlan* p, const float* packed, const float* c, const float* mean, const float* scale,
                        const TokArgs* tok, const float* z, float* out, void* workspace, void* stream) {
  PwgSmg* g = const_cast<PwgSmg*>(p->g);
  const PwgSmgConfig& cf = g->cfg;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  auto F = [&](long long off) { return reinterpret_cast<float*>(ws + off); };
  const SmgUtt* utt = reinterpret_cast<const SmgUtt*>(ws + p->ws_utt);
  int* flag = reinterpret_cast<int*>(ws + p->ws_flag);
  float2* partial = reinterpret_cast<float2*>(ws + p->ws_partial);
  const int C = cf.channels, K = cf.kernel_size, n = p->n_utts;
  const hipError_t e = upload_table(p->utts, reinterpret_cast<SmgUtt*>(ws + p->ws_utt), flag, s);
  if (e != hipSuccess) return hipf(e, "pwg_smg_run: plan upload");
  Runner r{g, s};
  TokArgs tk{};
  if (tok) {
    tk = *tok;
    tk.flag = flag;
  }

  // noise upsampling: z -> x0
  const float* nin = z;
  int f_in = 1;
  for (size_t i = 0; i < g->noise.size() && r.rc == PWG_OK; ++i) {
    const ConvSpec& cs = g->noise[i];
    const int sc = cf.noise_scales[i];
    const bool last = i + 1 == g->noise.size();
    float* nout = last ? F(p->ws_x[0]) : F(p->ws_noise[i & 1]);
    const int trim = last && p->trim;
    NoiseArgs a{utt, nin, packed + cs.pk_w, packed + cs.pk_b, nout, cs.cin, cs.cout, sc, sc / 2 + sc % 2, f_in, cf.noise_slope,
                trim};
    const long long elems = (trim ? p->max_n0 : p->max_z * f_in * sc) * cs.cout;
    r.begin(PWG_SMG_KIND_NOISE);
    hipLaunchKernelGGL(smg_noise_kernel, dim3((unsigned)((elems + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
    r.end(hipGetLastError(), "noise upsampling kernel");
    nin = nout;
    f_in *= sc;
  }
  run_stats(r, utt, n, p->max_n0, F(p->ws_x[0]), C, C, 1, partial, F(p->ws_stats[0]), nullptr, nullptr);

  auto conv = [&](const ConvSpec& cs, int kind, int epi, const float* in, float* o, int dil, int up, int rate,
                  bool in_is_c, const float* x, int xu, const float* stats) {
    if (r.rc != PWG_OK) return 0;
    const long long max_rows = p->max_n0 * rate;
    const int nt = pick_nt(max_rows, cs.cin, K, dil, epi, C);
    ConvArgs a{};
    a.utt = utt; a.in = in; a.w = reinterpret_cast<const float4*>(packed + cs.pk_w); a.bias = packed + cs.pk_b;
    a.out = o; a.mean = in_is_c ? mean : nullptr; a.scale = in_is_c ? scale : nullptr;
    a.x = x; a.stats = stats; a.partial = partial;
    a.cin = cs.cin; a.cs = cs.cs; a.K = K; a.dil = dil; a.up = up; a.rate = rate; a.in_is_c = in_is_c; a.xu = xu;
    a.gate = cf.gate;
    const int rows = 64 * nt;
    r.begin(kind);
    r.end(launch_conv(a, in_is_c && tok ? &tk : nullptr, cs.mt, nt, epi, dim3((unsigned)((max_rows + rows - 1) / rows), (unsigned)n),
                      conv_lds_bytes(cs.cin, K, dil, nt, epi, C), s),
          "conv kernel");
    return 64;  // rows per statistics partial
  };
  auto finalise = [&](int rate, int tile, float* stats) {
    if (r.rc != PWG_OK) return;
    FinaliseArgs fa{utt, partial, stats, nullptr, nullptr, C, rate, tile};
    r.begin(PWG_SMG_KIND_FINALISE);
    hipLaunchKernelGGL(smg_finalise_kernel, dim3((unsigned)n), dim3(1024), 0, s, fa);
    r.end(hipGetLastError(), "statistics finalise kernel");
  };

  const float* cin = c;
  for (int b = 0; b < g->nblocks; ++b) {
    const ConvSpec* cv = &g->convs[6 * b];
    const int rt = p->rate[b], sc = cf.upsample_scales[b], ro = rt * sc;
    float* c1 = F(p->ws_c1);
    float* c2 = F(p->ws_cab[b & 1]);
    float* y = F(p->ws_y);
    float* x1 = F(p->ws_x1);
    const float* xin = F(p->ws_x[b]);
    float* xout = F(p->ws_x[b + 1]);
    conv(cv[0], PWG_SMG_KIND_AUX_CONV, EPI_PLAIN, cin, c1, 1, 1, rt, b == 0, nullptr, 1, nullptr);
    conv(cv[1], PWG_SMG_KIND_MODULATE_CONV, EPI_MODULATE, c1, y, 1, 1, rt, false, xin, 1, F(p->ws_stats[2 * b]));
    int tile = conv(cv[2], PWG_SMG_KIND_GATE_CONV, EPI_GATE, y, x1, 1, 1, rt, false, nullptr, 1, nullptr);
    finalise(rt, tile, F(p->ws_stats[2 * b + 1]));
    conv(cv[3], PWG_SMG_KIND_AUX_CONV, EPI_PLAIN, c1, c2, 1, sc, ro, false, nullptr, 1, nullptr);
    conv(cv[4], PWG_SMG_KIND_MODULATE_CONV, EPI_MODULATE, c2, y, 1, 1, ro, false, x1, sc, F(p->ws_stats[2 * b + 1]));
    tile = conv(cv[5], PWG_SMG_KIND_GATE_CONV, EPI_GATE, y, xout, cf.dilation, 1, ro, false, xin, sc, nullptr);
    if (b + 1 < g->nblocks) finalise(ro, tile, F(p->ws_stats[2 * b + 2]));  // nothing normalises the last x
    cin = c2;
  }
  if (r.rc == PWG_OK) {
    OutArgs a{utt, F(p->ws_x[g->nblocks]), packed + g->outc.pk_w, packed + g->outc.pk_b, out, flag, C, cf.out_channels, K, g->hop};
    const long long elems = p->max_frames * g->hop * cf.out_channels;
    r.begin(PWG_SMG_KIND_OUTPUT);
    hipLaunchKernelGGL(smg_output_kernel, dim3((unsigned)((elems + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
    r.end(hipGetLastError(), "output kernel");
  }
  return r.rc;
}

int pwg_smg_run(const PwgSmgPlan* p, const float* packed, const float* c, const float* mean, const float* scale,
                const float* z, float* out, void* workspace, void* stream) {
  if (!p || !packed || !c || !z || !out || !workspace) return set_error(PWG_ERR_INVALID, "pwg_smg_run: null argument");
  if ((mean == nullptr) != (scale == nullptr)) return set_error(PWG_ERR_INVALID, "pwg_smg_run: mean and scale go together");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return set_error(PWG_ERR_INVALID, "pwg_smg_run: workspace must be 256-byte aligned");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(mean) |
       reinterpret_cast<uintptr_t>(scale)) & 15)
    return set_error(PWG_ERR_INVALID, "pwg_smg_run: packed, c, mean and scale must be 16-byte aligned");
  if (p->g->device < 0) return set_error(PWG_ERR_INVALID, "pwg_smg_run: a host-only handle cannot run");
  if (const int rc = check_device(p->g->device, "pwg_smg_run")) return rc;
  return run_launches(p, packed, c, mean, scale, nullptr, z, out, workspace, stream);
}

int pwg_smg_run_tokens(const PwgSmgPlan* p, const float* packed, const float* emb, int num_embs, const float* spk,
                       int num_spk, const long long* ids, const long long* spk_ids, const float* z, float* out,
                       void* workspace, void* stream) {
  if (!p || !packed || !emb || !spk || !ids || !spk_ids || !z || !out || !workspace)
    return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: null argument");
  if (num_embs < 1 || num_spk < 1) return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: empty embedding table");
  if (reinterpret_cast<uintptr_t>(workspace) & 255)
    return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: workspace must be 256-byte aligned");
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(emb) | reinterpret_cast<uintptr_t>(spk)) & 15)
    return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: packed, emb and spk must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(spk_ids)) & 7)
    return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: ids and spk_ids must be 8-byte aligned");
  if (!p->trim)
    return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: the plan was not created with PWG_SMG_PLAN_TRIM_NOISE");
  if (p->g->device < 0) return set_error(PWG_ERR_INVALID, "pwg_smg_run_tokens: a host-only handle cannot run");
  if (const int rc = check_device(p->g->device, "pwg_smg_run_tokens")) return rc;
  const TokArgs tok{emb, spk, ids, spk_ids, nullptr, num_embs, num_spk};
  return run_launches(p, packed, nullptr, nullptr, nullptr, &tok, z, out, workspace, stream);
}

int pwg_smg_run_status(const PwgSmgPlan* p, void* workspace, void* stream) {
  if (!p || !workspace) return set_error(PWG_ERR_INVALID, "pwg_smg_run_status: null argument");
  int flag = 0;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(&flag, static_cast<char*>(workspace) + p->ws_flag, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hipf(e, "pwg_smg_run_status");
  if (flag & ~PWG_SMG_FLAG_NONFINITE) {
    const int bits = flag >> PWG_SMG_FLAG_EMBED_SHIFT;
    const bool tokb = bits & PWG_EMBED_BAD_TOKEN, spkb = bits & PWG_EMBED_BAD_SPEAKER;
    return set_error(PWG_ERR_RANGE, tokb && spkb ? "bad token id and bad speaker id: ids outside [0, num_embs) and [0, num_spk) "
                                                   "were read as zero rows"
                                    : tokb       ? "bad token id: an id outside [0, num_embs) was read as a zero row"
                                                 : "bad speaker id: an id outside [0, num_spk) contributed zero");
  }
  if (flag != 0)
    return set_error(PWG_ERR_RANGE,
                     "non-finite StyleMelGAN output: a value left the fp16 pair range of the split-f16 conv kernels "
                     "upstream (|v| >= 65520), or the input is not finite; this path has no exact-fp32 mode");
  return PWG_OK;
}

int pwg_smg_debug_stats(const float* x, int ld, int channels, const long long* rows_per_utt, int n_utts, float* mean_out,
                        float* rstd_out, void* workspace, void* stream) {
  if (!x || !rows_per_utt || !mean_out || !rstd_out || !workspace)
    return set_error(PWG_ERR_INVALID, "pwg_smg_debug_stats: null argument");
  if (channels < 1 || channels > 1024 || ld < channels || n_utts < 1 || n_utts > 65535)
    return set_error(PWG_ERR_INVALID, "pwg_smg_debug_stats: 1 <= channels <= min(ld, 1024), 1 to 65535 utterances");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return set_error(PWG_ERR_INVALID, "pwg_smg_debug_stats: workspace must be 256-byte aligned");
  std::vector<SmgUtt> utts;
  long long p0 = 0, mx = 0;
  for (int u = 0; u < n_utts; ++u) {
    const long long rws = rows_per_utt[u];
    if (rws < 1 || rws > (1LL << 30)) return set_error(PWG_ERR_INVALID, "pwg_smg_debug_stats: rows out of range");
    utts.push_back(SmgUtt{p0, 0, 0, (int)rws, 0, 0, 0});
    p0 += rws;
    mx = rws > mx ? rws : mx;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const long long tab = ((long long)sizeof(SmgUtt) * n_utts + 255) / 256 * 256;
  const hipError_t e = upload_table(utts, reinterpret_cast<SmgUtt*>(ws), nullptr, s);
  if (e != hipSuccess) return hipf(e, "pwg_smg_debug_stats: table upload");
  Runner r{nullptr, s};
  run_stats(r, reinterpret_cast<const SmgUtt*>(ws), n_utts, mx, x, ld, channels, 1, reinterpret_cast<float2*>(ws + tab),
            nullptr, mean_out, rstd_out);
  return r.rc;
}

int pwg_smg_set_timing(PwgSmg* g, int on) {
  if (!g) return set_error(PWG_ERR_INVALID, "pwg_smg_set_timing: null handle");
  g->timing = on != 0;
  return PWG_OK;
}

int pwg_smg_timing_collect(PwgSmg* g, double* ms) {
  if (!g || !ms) return set_error(PWG_ERR_INVALID, "pwg_smg_timing_collect: null argument");
  for (int k = 0; k < PWG_SMG_KINDS; ++k) ms[k] = 0.0;
  int rc = PWG_OK;
  for (auto& sp : g->spans) {
    float t = 0.f;
    hipError_t e = hipEventSynchronize(sp.e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, sp.e0, sp.e1);
    if (e != hipSuccess && rc == PWG_OK) rc = hipf(e, "pwg_smg_timing_collect");
    ms[sp.kind] += t;
    (void)hipEventDestroy(sp.e0);
    (void)hipEventDestroy(sp.e1);
  }
  g->spans.clear();
  return rc;
}

}  // extern "C"
