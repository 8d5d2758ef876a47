// The VQVAE kernels (include/pwg_vq.h; parallel_wavegan/models/vqvae.py:16-171 of the reference):
//
//  * pwg_vq_wave_kernel: the encoder's first layer, ReflectionPad1d + Conv1d(1 -> C, K <= 31) +
//    LeakyReLU over the sample-rate signal. K C FMAs per sample on the VALU in tap order, weights in
//    LDS, one 16-byte store per thread (the layout of pwg_uhg_excite_kernel, pwg_uconv.hip). A tap
//    outside the utterance mirrors at the utterance's own first / last sample.
//
//  * pwg_vq_gsconv_kernel<S>: one grouped strided level of MelGANDiscriminator, Conv1d(in, out,
//    10 S + 1, stride S, padding 5 S, groups in / 4). A group has 4 input channels: they are the K = 4
//    of v_mfma_f32_16x16x4_f32, one MFMA per (group, tap, 16 output columns), so none of the zero
//    blocks of the dense-equivalent weight is multiplied. A workgroup (4 waves) takes GS_COLS = 64
//    output columns of one utterance and one 16-channel input block; wave w owns group w of the
//    block and all four 16-column tiles (four independent accumulators). The input span of the
//    column tile (73 S + 1 rows x 64 bytes) is staged in LDS once and reused over the 10 S + 1 taps.
//    LDS row r lives at 64 r + 16 (r / S) bytes (the pitch of pwg_uconv_sconv_kernel): the 16 lanes of
//    one k read rows S apart, 4 (4 S + 1) words apart -- 36, 52, 68 words for S = 2, 3, 4, all
//    distinct multiples of 4 modulo the 64 banks -- and the four k of a column are consecutive words,
//    so the 64 4-byte reads of a wave fall on 64 distinct banks.
//    M = 16 holds one group of 16 outputs, two of 8 or four of 4: the A fragment of a group has zeros
//    in the rows of the other groups of its m-tile (pwg_vq_gsconv_pack), and a wave stores only its
//    own group's rows. Exact fp32.
//
//  * pwg_vq_nearest_kernel: the nearest-code search. A workgroup takes 16 rows of z; its 4 waves
//    share the 16-code column tiles round robin. z . e^T runs on the 16x16x4 f32 MFMA (lane (k, j)
//    reads 4 consecutive floats of its row / code per 16-float step: four MFMAs), the distance is
//    (||e||^2 + ||z||^2) - 2 z.e in fp32 (the reference's addmm), every lane keeps its running best
//    in ascending code order with a strict <, and the 16 lanes, then the 4 waves, are merged by
//    (distance, index): the lowest index among equal distances wins.
//
//  * pwg_vq_decode_kernel: the decoder's input rows [codebook[idx] ; local projection ; global row],
//    one wave per row as pwg_embed_rows_kernel (pwg_embed.hip).

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <string>

#include "../../include/pwg_vq.h"
#include "pwg_internal.h"

namespace pwg {
namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------
constexpr int WV_MAX_K = 31;
constexpr int WV_MAX_LDS_FLOATS = 16384;  // channels * (K + 1): 64 KiB of LDS

struct WaveArgs {
  const float* x;
  const float* w;
  const float* b;
  const long long* row_start;
  float* out;
  long long rows;
  int n_utts, C, K;
  float slope;
};

__global__ void __launch_bounds__(256) pwg_vq_wave_kernel(const WaveArgs a) {
  extern __shared__ __attribute__((aligned(16))) float wv_w[];  // [C][K] weights, then [C] biases
  const int nw = a.C * a.K;
  for (int i = threadIdx.x; i < nw; i += 256) wv_w[i] = a.w[i];
  for (int i = threadIdx.x; i < a.C; i += 256) wv_w[nw + i] = a.b ? a.b[i] : 0.f;
  __syncthreads();
  const int vpr = a.C >> 2;  // 16-byte vectors per row
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long r = idx / vpr;
  const int v = (int)(idx - r * vpr);
  if (r >= a.rows) return;
  // the last u in [0, n_utts) with row_start[u] <= r (u = 0 if none)
  int lo = 0, hi = a.n_utts - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.row_start[mid] <= r) lo = mid; else hi = mid - 1;
  }
  long long t0 = clampll(a.row_start[lo], 0, r);
  long long t1 = clampll(a.row_start[lo + 1], r + 1, a.rows);
  const long long len = t1 - t0;  // >= 1: the row itself
  const int pad = (a.K - 1) >> 1;
  float xs[WV_MAX_K];
#pragma unroll
  for (int k = 0; k < WV_MAX_K; ++k) {
    long long p = r - t0 - pad + k;
    if (p < 0) p = -p;
    if (p >= len) p = 2 * (len - 1) - p;
    p = clampll(p, 0, len - 1);  // (an utterance shorter than the host check saw: stay inside it)
    xs[k] = k < a.K ? a.x[t0 + p] : 0.f;
  }
  float o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int ch = 4 * v + c;
    float acc = wv_w[nw + ch];
#pragma unroll
    for (int k = 0; k < WV_MAX_K; ++k)
      if (k < a.K) acc = __builtin_fmaf(wv_w[ch * a.K + k], xs[k], acc);
    o[c] = acc > 0.f ? acc : acc * a.slope;
  }
  *reinterpret_cast<float4*>(a.out + r * a.C + 4 * v) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------
constexpr int GS_COLS = 64;
constexpr int GS_THREADS = 256;

struct GsArgs {
  const float* x;
  const long long* rs_in;
  const float* w;
  const float* b;
  float* y;
  const long long* rs_out;
  long long rows_in, rows_out;
  int n_utts, Cin, Cout, opg;
  float slope;
};

__host__ __device__ constexpr int gs_span(int s) { return (GS_COLS - 1) * s + 10 * s + 1; }
__host__ __device__ constexpr int gs_lds(int s) { return gs_span(s) * 64 + (gs_span(s) / s + 1) * 16; }

template <int S>
__global__ void __launch_bounds__(GS_THREADS) pwg_vq_gsconv_kernel(const GsArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char gs_x[gs_lds(S)];
  constexpr int K = 10 * S + 1;
  constexpr int SPAN = gs_span(S);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int kk = lane >> 4, j = lane & 15;
  // this workgroup's utterance and column tile: utterance u has ceil(len_out / GS_COLS) tiles
  long long t = blockIdx.x, o0 = 0, len_out = 0;
  int u = 0;
  for (; u < a.n_utts; ++u) {
    o0 = clampll(a.rs_out[u], 0, a.rows_out);
    const long long o1 = clampll(a.rs_out[u + 1], o0, a.rows_out);
    len_out = o1 - o0;
    const long long nt = (len_out + GS_COLS - 1) / GS_COLS;
    if (t < nt) break;
    t -= nt;
  }
  if (u >= a.n_utts) return;  // (the grid is an upper bound of the tile count)
  const long long in0 = clampll(a.rs_in[u], 0, a.rows_in);
  const long long len_in = clampll(a.rs_in[u + 1], in0, a.rows_in) - in0;
  const long long q0 = t * GS_COLS;
  const long long r_first = q0 * S - 5 * S;  // utterance row of LDS row 0
  const int cb = blockIdx.y;

  // the span's rows of channel block cb; rows outside the utterance read zero (never a neighbour's)
  for (int it = threadIdx.x; it < SPAN * 4; it += GS_THREADS) {
    const int row = it >> 2, qd = it & 3;
    const long long r = r_first + row;
    f32x4v v = {0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < len_in) v = *reinterpret_cast<const f32x4v*>(a.x + (size_t)(in0 + r) * a.Cin + cb * 16 + qd * 4);
    *reinterpret_cast<f32x4v*>(gs_x + row * 64 + (row / S) * 16 + qd * 16) = v;
  }
  __syncthreads();

  const int g = cb * 4 + wave;  // < Cin / 4: Cin is a multiple of 16
  const float* const wp = a.w + (size_t)g * K * 64 + lane;
  f32x4v acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
  // lane (kk, j) of column tile n reads channel 4 wave + kk of LDS row (16 n + j) S + k
  const unsigned char* const bp = gs_x + j * (S * 64 + 16) + (4 * wave + kk) * 4;
  float av = wp[0];
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    const float an = k + 1 < K ? wp[(k + 1) * 64] : 0.f;
    const unsigned char* const bk = bp + k * 64 + (k / S) * 16;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const float bv = *reinterpret_cast<const float*>(bk + n * 16 * (S * 64 + 16));
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[n], 0, 0, 0);
    }
    av = an;
  }

  // accumulator register i of lane (kk, j): m-tile row 4 kk + i, column j. The group's rows in its
  // m-tile are [slot, slot + opg); the other rows belong to other waves' groups.
  const int first = g * a.opg;
  const int slot = first & 15;
  const int i0 = 4 * kk;
  if (i0 < slot || i0 >= slot + a.opg) return;
  const int o = (first & ~15) + i0;
  f32x4v bb = {0.f, 0.f, 0.f, 0.f};
  if (a.b) bb = *reinterpret_cast<const f32x4v*>(a.b + o);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const long long q = q0 + n * 16 + j;
    if (q >= len_out) continue;
    f32x4v v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = acc[n][i] + bb[i];
      v[i] = s > 0.f ? s : s * a.slope;
    }
    *reinterpret_cast<f32x4v*>(a.y + (size_t)(o0 + q) * a.Cout + o) = v;
  }
}

bool gs_shape_ok(int cin, int cout, int s) {
  if (s < 2 || s > 4 || cin < 16 || cin % 16 || cout < 16 || cout % 16 || cout > 1024) return false;
  const int groups = cin / 4;
  if (cout % groups) return false;
  const int opg = cout / groups;
  return opg == 4 || opg == 8 || opg == 16;
}

// ---------------------------------------------------------------------------------------------
struct NormArgs {
  const float* e;
  float* en;
  int N, D;
};

__global__ void __launch_bounds__(256) pwg_vq_code_norms_kernel(const NormArgs a) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.N) return;
  float s = 0.f;
  for (int d = lane; d < a.D; d += 64) {
    const float v = a.e[(size_t)k * a.D + d];
    s = __builtin_fmaf(v, v, s);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) a.en[k] = s;
}

struct NnArgs {
  const float* z;
  const float* e;
  const float* en;
  long long* idx;
  float* zq;
  int* flag;
  long long rows;
  int D, N;
};

constexpr int NN_ROWS = 16;

__global__ void __launch_bounds__(256) pwg_vq_nearest_kernel(const NnArgs a) {
  __shared__ float nn_d[4][NN_ROWS];
  __shared__ int nn_i[4][NN_ROWS];
  __shared__ int nn_best[NN_ROWS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int kk = lane >> 4, j = lane & 15;
  const long long r0 = (long long)blockIdx.x * NN_ROWS;
  const bool zin = r0 + j < a.rows;
  const float* const zp = a.z + (size_t)(zin ? r0 + j : 0) * a.D + 4 * kk;

  // ||z_j||^2: every lane sums the 4-float pieces it also feeds the MFMAs, the four k lanes of a row add up
  float zn = 0.f;
  if (zin) {
    for (int d0 = 0; d0 < a.D; d0 += 16) {
      const f32x4v v = *reinterpret_cast<const f32x4v*>(zp + d0);
#pragma unroll
      for (int i = 0; i < 4; ++i) zn = __builtin_fmaf(v[i], v[i], zn);
    }
  }
  zn += __shfl_xor(zn, 16);
  zn += __shfl_xor(zn, 32);  // every lane with this j now holds ||z_j||^2
  float znr[4];              // ... and the norms of its accumulator rows 4 kk + i
#pragma unroll
  for (int i = 0; i < 4; ++i) znr[i] = __shfl(zn, 4 * kk + i);

  float bd[4];
  int bi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { bd[i] = INFINITY; bi[i] = 0; }
  const int n_tiles = (a.N + 15) >> 4;
  for (int ct = wave; ct < n_tiles; ct += 4) {
    const int c = ct * 16 + j;
    const bool cin = c < a.N;  // code columns at or beyond N read nothing and never win
    const float* const ep = a.e + (size_t)(cin ? c : 0) * a.D + 4 * kk;
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < a.D; d0 += 16) {
      f32x4v zv = {0.f, 0.f, 0.f, 0.f}, ev = {0.f, 0.f, 0.f, 0.f};
      if (zin) zv = *reinterpret_cast<const f32x4v*>(zp + d0);
      if (cin) ev = *reinterpret_cast<const f32x4v*>(ep + d0);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[i], ev[i], acc, 0, 0, 0);
    }
    if (cin) {
      const float en = a.en[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = __builtin_fmaf(-2.f, acc[i], en + znr[i]);
        if (d < bd[i]) { bd[i] = d; bi[i] = c; }
      }
    }
  }
  // the 16 code lanes of a row, then the 4 waves: smallest (distance, index)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const float od = __shfl_xor(bd[i], off);
      const int oi = __shfl_xor(bi[i], off);
      if (od < bd[i] || (od == bd[i] && oi < bi[i])) { bd[i] = od; bi[i] = oi; }
    }
    if (j == 0) { nn_d[wave][4 * kk + i] = bd[i]; nn_i[wave][4 * kk + i] = bi[i]; }
  }
  __syncthreads();
  if (threadIdx.x < NN_ROWS) {  // wave 0, lane j = threadIdx.x: zn is this row's norm
    float d = nn_d[0][threadIdx.x];
    int best = nn_i[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float od = nn_d[w][threadIdx.x];
      const int oi = nn_i[w][threadIdx.x];
      if (od < d || (od == d && oi < best)) { d = od; best = oi; }
    }
    if (zin) {
      if (!(fabsf(zn) <= FLT_MAX)) {
        best = 0;
        __hip_atomic_fetch_or(a.flag, PWG_VQ_BAD_INPUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      a.idx[r0 + threadIdx.x] = best;
    }
    nn_best[threadIdx.x] = best;  // inside [0, N) by construction
  }
  if (a.zq == nullptr) return;
  __syncthreads();
  const int vpr = a.D >> 2;
  for (int it = threadIdx.x; it < NN_ROWS * vpr; it += 256) {
    const int row = it / vpr, v = it - row * vpr;
    if (r0 + row >= a.rows) break;
    reinterpret_cast<f32x4v*>(a.zq + (size_t)(r0 + row) * a.D)[v] =
        reinterpret_cast<const f32x4v*>(a.e + (size_t)nn_best[row] * a.D)[v];
  }
}

// ---------------------------------------------------------------------------------------------
constexpr int DEC_WAVES = 4;  // waves per workgroup
constexpr int DEC_ROWS = 4;   // consecutive rows per wave

struct DecArgs {
  const float* e;
  const long long* idx;
  const float* local;
  const float* wl;
  const float* bl;
  const float* glob;
  const long long* g_ids;
  const long long* row_start;
  float* out;
  int* flag;
  long long rows;
  int N, D, nl, L, NG, G, n_utts;
};

__global__ void __launch_bounds__(64 * DEC_WAVES) pwg_vq_decode_kernel(const DecArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long r0 = ((long long)blockIdx.x * DEC_WAVES + wave) * DEC_ROWS;
  if (r0 >= a.rows) return;
  const int width = a.D + a.L + a.G;
  int u = 0;
  if (a.glob != nullptr) {  // the last u in [0, n_utts) with row_start[u] <= r0 (u = 0 if none)
    int lo = 0, hi = a.n_utts - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.row_start[mid] <= r0) lo = mid; else hi = mid - 1;
    }
    u = lo;
  }
  const long long r1 = r0 + DEC_ROWS < a.rows ? r0 + DEC_ROWS : a.rows;
  for (long long r = r0; r < r1; ++r) {
    int bad = 0;
    long long id = 0, g = 0;
    if (a.e != nullptr) {
      id = a.idx[r];
      if (id < 0 || id >= a.N) bad |= PWG_VQ_BAD_CODE;
    }
    if (a.glob != nullptr) {
      while (u + 1 < a.n_utts && a.row_start[u + 1] <= r) ++u;
      g = a.g_ids[u];
      if (g < 0 || g >= a.NG) bad |= PWG_VQ_BAD_GLOBAL;
    }
    float* const o = a.out + r * width;
    if (bad) {  // no address is formed from an id that failed its check
      for (int v = lane; v < (width >> 2); v += 64) reinterpret_cast<float4*>(o)[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane == 0) __hip_atomic_fetch_or(a.flag, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    if (a.e != nullptr) {
      const float4* const e = reinterpret_cast<const float4*>(a.e + id * a.D);
      for (int v = lane; v < (a.D >> 2); v += 64) reinterpret_cast<float4*>(o)[v] = e[v];
    }
    if (a.local != nullptr) {
      const float* const l = a.local + r * a.nl;
      for (int c = lane; c < a.L; c += 64) {
        float acc;
        if (a.wl != nullptr) {
          acc = a.bl ? a.bl[c] : 0.f;
          for (int i = 0; i < a.nl; ++i) acc = __builtin_fmaf(a.wl[c * a.nl + i], l[i], acc);
        } else {
          acc = l[c];
        }
        o[a.D + c] = acc;
      }
    }
    if (a.glob != nullptr) {
      const float4* const s = reinterpret_cast<const float4*>(a.glob + g * a.G);
      float4* const og = reinterpret_cast<float4*>(o + a.D + a.L);
      for (int v = lane; v < (a.G >> 2); v += 64) og[v] = s[v];
    }
  }
}

int launch_status(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(PWG_ERR_HIP, (std::string(who) + ": " + hipGetErrorString(e)).c_str());
  return PWG_OK;
}

}  // namespace
}  // namespace pwg

using pwg::set_error;

extern "C" int pwg_vq_wave_rows(const float* x, const float* w, const float* b, int channels, int kernel_size,
                                float slope, const long long* row_start, const long long* row_start_host,
                                int n_utts, long long rows, float* out, void* stream) {
  if (!x || !w || !row_start || !row_start_host || !out)
    return set_error(PWG_ERR_INVALID, "pwg_vq_wave_rows: x, w, row_start, row_start_host and out must not be null");
  if (n_utts < 1 || rows < 0) return set_error(PWG_ERR_INVALID, "pwg_vq_wave_rows: n_utts must be >= 1 and rows >= 0");
  if (kernel_size < 1 || kernel_size % 2 == 0 || kernel_size > pwg::WV_MAX_K)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_wave_rows: kernel_size must be odd and at most 31");
  if (channels < 16 || channels % 16 || (long long)channels * (kernel_size + 1) > pwg::WV_MAX_LDS_FLOATS)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_wave_rows: channels must be a multiple of 16 with channels * (kernel_size + 1) <= 16384");
  if (!pwg::aligned16(out)) return set_error(PWG_ERR_INVALID, "pwg_vq_wave_rows: out must be 16-byte aligned");
  if (rows == 0) return PWG_OK;
  const int pad = (kernel_size - 1) / 2;
  if (row_start_host[0] != 0 || row_start_host[n_utts] != rows)
    return set_error(PWG_ERR_INVALID, "pwg_vq_wave_rows: row_start must run from 0 to rows");
  for (int u = 0; u < n_utts; ++u)
    if (row_start_host[u + 1] - row_start_host[u] < pad + 1)
      return set_error(PWG_ERR_INVALID, "pwg_vq_wave_rows: an utterance is shorter than (kernel_size - 1) / 2 + 1 samples (reflection padding needs them)");
  const long long n_wg = (rows * (channels / 4) + 255) / 256;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_vq_wave_rows: too many rows for one launch");
  pwg::WaveArgs a;
  a.x = x; a.w = w; a.b = b; a.row_start = row_start; a.out = out; a.rows = rows;
  a.n_utts = n_utts; a.C = channels; a.K = kernel_size; a.slope = slope;
  const size_t lds = (size_t)(channels * kernel_size + channels) * sizeof(float);
  hipLaunchKernelGGL(pwg::pwg_vq_wave_kernel, dim3((unsigned)n_wg), dim3(256), lds, (hipStream_t)stream, a);
  return pwg::launch_status("pwg_vq_wave_rows");
}

extern "C" long long pwg_vq_gsconv_packed_count(int in_channels, int out_channels, int stride) {
  if (!pwg::gs_shape_ok(in_channels, out_channels, stride)) return -1;
  return (long long)(in_channels / 4) * (10 * stride + 1) * 64;
}

extern "C" int pwg_vq_gsconv_pack(const float* w_host, int in_channels, int out_channels, int stride,
                                  float* packed_host) {
  if (!w_host || !packed_host) return set_error(PWG_ERR_INVALID, "pwg_vq_gsconv_pack: w and packed must not be null");
  if (!pwg::gs_shape_ok(in_channels, out_channels, stride))
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_gsconv_pack: stride 2..4, in_channels a multiple of 16, 4, 8 or 16 outputs per group, out_channels a multiple of 16 up to 1024");
  const int groups = in_channels / 4, opg = out_channels / groups, K = 10 * stride + 1;
  for (int g = 0; g < groups; ++g) {
    const int mbase = (g * opg) & ~15;
    for (int k = 0; k < K; ++k) {
      float* const f = packed_host + ((size_t)g * K + k) * 64;
      for (int l = 0; l < 64; ++l) {
        const int o = mbase + (l & 15), i = l >> 4;
        f[l] = (o / opg == g) ? w_host[((size_t)o * 4 + i) * K + k] : 0.f;
      }
    }
  }
  return PWG_OK;
}

extern "C" int pwg_vq_gsconv(const float* x, const long long* row_start_in, long long rows_in, int in_channels,
                             const float* w_packed, const float* b, int out_channels, int stride, float slope,
                             float* y, const long long* row_start_out, long long rows_out, int n_utts,
                             void* stream) {
  if (!x || !row_start_in || !w_packed || !y || !row_start_out)
    return set_error(PWG_ERR_INVALID, "pwg_vq_gsconv: x, row_start_in, w_packed, y and row_start_out must not be null");
  if (n_utts < 1 || rows_in < 0 || rows_out < 0)
    return set_error(PWG_ERR_INVALID, "pwg_vq_gsconv: n_utts must be >= 1, rows_in and rows_out >= 0");
  if (!pwg::gs_shape_ok(in_channels, out_channels, stride))
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_gsconv: stride 2..4, in_channels a multiple of 16, 4, 8 or 16 outputs per group, out_channels a multiple of 16 up to 1024");
  if (!pwg::aligned16(x) || !pwg::aligned16(y) || !pwg::aligned16(w_packed) || !pwg::aligned16(b))
    return set_error(PWG_ERR_INVALID, "pwg_vq_gsconv: x, y, w_packed and b must be 16-byte aligned");
  // sum_u ceil(len_u / GS_COLS) <= rows_out / GS_COLS + n_utts
  const long long n_wg = rows_out / pwg::GS_COLS + n_utts;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_vq_gsconv: too many rows for one launch");
  if (rows_out == 0) return PWG_OK;
  pwg::GsArgs a;
  a.x = x; a.rs_in = row_start_in; a.w = w_packed; a.b = b; a.y = y; a.rs_out = row_start_out;
  a.rows_in = rows_in; a.rows_out = rows_out; a.n_utts = n_utts; a.Cin = in_channels; a.Cout = out_channels;
  a.opg = out_channels / (in_channels / 4); a.slope = slope;
  const dim3 grid((unsigned)n_wg, (unsigned)(in_channels / 16));
  hipStream_t s = (hipStream_t)stream;
  if (stride == 2) hipLaunchKernelGGL(pwg::pwg_vq_gsconv_kernel<2>, grid, dim3(pwg::GS_THREADS), 0, s, a);
  else if (stride == 3) hipLaunchKernelGGL(pwg::pwg_vq_gsconv_kernel<3>, grid, dim3(pwg::GS_THREADS), 0, s, a);
  else hipLaunchKernelGGL(pwg::pwg_vq_gsconv_kernel<4>, grid, dim3(pwg::GS_THREADS), 0, s, a);
  return pwg::launch_status("pwg_vq_gsconv");
}

extern "C" int pwg_vq_code_norms(const float* codebook, int num_embeds, int dim, float* enorm, void* stream) {
  if (!codebook || !enorm) return set_error(PWG_ERR_INVALID, "pwg_vq_code_norms: codebook and enorm must not be null");
  if (num_embeds < 1) return set_error(PWG_ERR_INVALID, "pwg_vq_code_norms: num_embeds must be >= 1");
  if (dim < 16 || dim % 16 || dim > 1024)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_code_norms: dim must be a multiple of 16 up to 1024");
  pwg::NormArgs a;
  a.e = codebook; a.en = enorm; a.N = num_embeds; a.D = dim;
  hipLaunchKernelGGL(pwg::pwg_vq_code_norms_kernel, dim3((unsigned)((num_embeds + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return pwg::launch_status("pwg_vq_code_norms");
}

extern "C" int pwg_vq_nearest(const float* z, long long rows, int dim, const float* codebook, const float* enorm,
                              int num_embeds, long long* idx, float* zq, int* flag, void* stream) {
  if (!z || !codebook || !enorm || !idx || !flag)
    return set_error(PWG_ERR_INVALID, "pwg_vq_nearest: z, codebook, enorm, idx and flag must not be null");
  if (rows < 0 || num_embeds < 1) return set_error(PWG_ERR_INVALID, "pwg_vq_nearest: rows must be >= 0 and num_embeds >= 1");
  if (dim < 16 || dim % 16 || dim > 1024)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_nearest: dim must be a multiple of 16 up to 1024");
  if (!pwg::aligned16(z) || !pwg::aligned16(codebook) || !pwg::aligned16(zq))
    return set_error(PWG_ERR_INVALID, "pwg_vq_nearest: z, codebook and zq must be 16-byte aligned");
  const long long n_wg = (rows + pwg::NN_ROWS - 1) / pwg::NN_ROWS;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_vq_nearest: too many rows for one launch");
  if (rows == 0) return PWG_OK;
  pwg::NnArgs a;
  a.z = z; a.e = codebook; a.en = enorm; a.idx = idx; a.zq = zq; a.flag = flag; a.rows = rows; a.D = dim; a.N = num_embeds;
  hipLaunchKernelGGL(pwg::pwg_vq_nearest_kernel, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)stream, a);
  return pwg::launch_status("pwg_vq_nearest");
}

extern "C" int pwg_vq_decode_rows(const float* codebook, int num_embeds, int D, const long long* idx,
                                  const float* local, int num_local, const float* w_local, const float* b_local,
                                  int L, const float* glob, int num_global, int G, const long long* g_ids,
                                  const long long* row_start, int n_utts, long long rows, float* out, int* flag,
                                  void* stream) {
  if (!out || !flag) return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: out and flag must not be null");
  if (!codebook && !local && !glob) return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: at least one of codebook, local and glob is needed");
  if (rows < 0) return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: rows must be >= 0");
  if (codebook) {
    if (!idx || num_embeds < 1) return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: a codebook needs idx and num_embeds >= 1");
    if (D < 16 || D % 16) return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_decode_rows: D must be a positive multiple of 16");
  } else {
    D = 0;
  }
  if (local) {
    if (num_local < 1) return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: local rows need num_local >= 1");
    if (!w_local && (b_local || L != num_local))
      return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: without w_local the rows are copied: L must equal num_local and b_local be null");
    if (L < 16 || L % 16) return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_decode_rows: L must be a positive multiple of 16");
  } else {
    L = 0;
  }
  if (glob) {
    if (!g_ids || !row_start || num_global < 1 || n_utts < 1)
      return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: a global table needs g_ids, row_start, num_global >= 1 and n_utts >= 1");
    if (G < 16 || G % 16) return set_error(PWG_ERR_UNSUPPORTED, "pwg_vq_decode_rows: G must be a positive multiple of 16");
  } else {
    G = 0;
  }
  if (!pwg::aligned16(codebook) || !pwg::aligned16(glob) || !pwg::aligned16(out))
    return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: codebook, glob and out must be 16-byte aligned");
  constexpr long long per_wg = (long long)pwg::DEC_WAVES * pwg::DEC_ROWS;
  const long long n_wg = (rows + per_wg - 1) / per_wg;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_vq_decode_rows: too many rows for one launch");
  if (rows == 0) return PWG_OK;
  pwg::DecArgs a;
  a.e = codebook; a.idx = idx; a.local = local; a.wl = local ? w_local : nullptr; a.bl = local ? b_local : nullptr;
  a.glob = glob; a.g_ids = g_ids; a.row_start = row_start; a.out = out; a.flag = flag; a.rows = rows;
  a.N = num_embeds; a.D = D; a.nl = num_local; a.L = L; a.NG = num_global; a.G = G; a.n_utts = glob ? n_utts : 0;
  hipLaunchKernelGGL(pwg::pwg_vq_decode_kernel, dim3((unsigned)n_wg), dim3(64 * pwg::DEC_WAVES), 0,
                     (hipStream_t)stream, a);
  return pwg::launch_status("pwg_vq_decode_rows");
}
