// UHiFiGAN's encoder kernels (parallel_wavegan/models/uhifigan.py:78-153, 274-283 of the reference):
//
//  * pwg_uconv_sconv_kernel: the strided Conv1d(C -> 2C, kernel 2s, stride s, padding s//2 + s%2) of
//    `downsamples[i]` as an op of the conv-network executor (PWG_CNET_SCONV, include/pwg_cnet.h),
//      y[o, q] = post(b[o] + sum_{i, k} W[o, i, k] x[i, q s - p + k]),
//    over the executor's time-major [rows][ld] fp32 buffers, zero taps outside the utterance.
//    A workgroup (4 waves) takes SCONV_COLS = 64 output columns of one utterance and up to 4 m-tiles
//    (128 output rows): wave w owns column tile w & 1 and the m-tile pair w >> 1. Per 16-channel block
//    the input span (64 s + s rows) is staged once in LDS -- pre-activated and, in split-f16 mode,
//    split into fp16 hi / lo pairs -- and the 2s taps run as MFMAs whose B operand is LDS row
//    c s + k of the lane's column c. The next block's rows are loaded into registers under the MFMAs.
//    LDS row r lives at 64 r + 16 (r / s) bytes: the lanes of a wave read rows s apart, i.e.
//    16 (4s + 1) bytes apart -- an odd number of 16-byte units for every s, even ones included, so
//    the 16-byte reads of consecutive lanes fall on distinct bank groups.
//    Two numeric modes (template flag): three 32x32x16 f16 products hi.hi, hi.lo, lo.hi with fp32
//    accumulate, the executor's split-f16 scheme, or exact fp32 on the 32x32x2 f32 MFMA. The A
//    fragments are the executor's own images ([chunk][m-tile][2][64][4], chunk = block K + tap).
//
//  * pwg_uhg_excite_kernel: the excitation front end (include/pwg_uhg.h), Conv1d(1 -> C, K) +
//    LeakyReLU over the sample-rate signal. K C FMAs per sample on the VALU (padding one input
//    channel to an MFMA K of 16 would read 16x the bytes); weights in LDS, one 16-byte store per
//    thread, consecutive threads consecutive addresses.

#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/pwg_cnet.h"
#include "../../include/pwg_uhg.h"
#include "pwg_internal.h"

namespace pwg {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_STRIDE = 8;
// 16-byte quads of the staged span per thread: (64 s + s) rows x 4 quads over 256 threads
constexpr int SC_QUADS = ((SCONV_COLS + 1) * SC_MAX_STRIDE * 4 + SC_THREADS - 1) / SC_THREADS;

__device__ __forceinline__ int sc_row_addr(int row, int grp) { return row * 64 + grp * 16; }

template <bool SPLIT>
__global__ void __launch_bounds__(SC_THREADS) pwg_uconv_sconv_kernel(const SconvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hh = lane >> 5, cl = lane & 31;
  const int2 blk = a.blocks[blockIdx.x];
  const int u = blk.x, q0 = blk.y;
  const int2 sx = *reinterpret_cast<const int2*>(a.seg_x + 2 * u);
  const int2 sy = *reinterpret_cast<const int2*>(a.seg_y + 2 * u);
  const int s = a.stride, K = 2 * s;
  const int span = SCONV_COLS * s + s;
  const int n_quads = span * 4;
  const int r_first = q0 * s - a.padding;  // utterance row of LDS row 0
  const int ct = wave & 1;
  const int m_base = blockIdx.y * 4 + (wave >> 1) * 2;
  const bool live0 = m_base < a.mt_total, live1 = m_base + 1 < a.mt_total;

  f32x16 acc[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  // the span's rows of channel block cb: rows outside the utterance read zero (never a neighbour's)
  f32x4v raw[SC_QUADS];
  auto gload = [&](int cb) {
#pragma unroll
    for (int i = 0; i < SC_QUADS; ++i) {
      const int it = threadIdx.x + SC_THREADS * i;
      const int row = it >> 2, qd = it & 3;
      const int r = r_first + row;
      f32x4v v = {0.f, 0.f, 0.f, 0.f};
      if (it < n_quads && r >= 0 && r < sx.y)
        v = *reinterpret_cast<const f32x4v*>(a.x + (size_t)(sx.x + r) * a.ld_x + cb * 16 + qd * 4);
      raw[i] = v;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < SC_QUADS; ++i) {
      const int it = threadIdx.x + SC_THREADS * i;
      if (it >= n_quads) continue;
      const int row = it >> 2, qd = it & 3;
      f32x4v v = raw[i];
      if (a.slope != 1.f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope;
      }
      unsigned char* const d = sc_lds + sc_row_addr(row, row / s);
      if constexpr (SPLIT) {
        u32x2v hi, lo;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const _Float16 h0 = (_Float16)v[2 * e], h1 = (_Float16)v[2 * e + 1];
          hi[e] = __builtin_bit_cast(unsigned, f16x2v{h0, h1});
          lo[e] = __builtin_bit_cast(unsigned, f16x2v{(_Float16)(v[2 * e] - (float)h0), (_Float16)(v[2 * e + 1] - (float)h1)});
        }
        *reinterpret_cast<u32x2v*>(d + qd * 8) = hi;
        *reinterpret_cast<u32x2v*>(d + 32 + qd * 8) = lo;
      } else {
        *reinterpret_cast<f32x4v*>(d + qd * 16) = v;
      }
    }
  };

  const int col = ct * 32 + cl;  // this lane's column in the block
  gload(0);
  for (int cb = 0; cb < a.cs; ++cb) {
    lstore();
    __syncthreads();
    if (cb + 1 < a.cs) gload(cb + 1);
    if (live0) {
      for (int k = 0; k < K; ++k) {
        const unsigned char* const b = sc_lds + sc_row_addr(col * s + k, col + (k >= s ? 1 : 0));
        const float* const wp = a.w + ((size_t)(cb * K + k) * a.mt_total + m_base) * 512;
        if constexpr (SPLIT) {
          const u32x4v bh = *reinterpret_cast<const u32x4v*>(b + 16 * hh);
          const u32x4v bl = *reinterpret_cast<const u32x4v*>(b + 32 + 16 * hh);
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            if (m == 1 && !live1) break;
            const u32x4v* const wa = reinterpret_cast<const u32x4v*>(wp + m * 512) + lane;
            const u32x4v ah = wa[0], al = wa[64];
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, ah), __builtin_bit_cast(f16x8v, bh),
                                                            acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, ah), __builtin_bit_cast(f16x8v, bl),
                                                            acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, al), __builtin_bit_cast(f16x8v, bh),
                                                            acc[m], 0, 0, 0);
          }
        } else {
          const f32x4v b0 = *reinterpret_cast<const f32x4v*>(b + 32 * hh);
          const f32x4v b1 = *reinterpret_cast<const f32x4v*>(b + 32 * hh + 16);
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            if (m == 1 && !live1) break;
            const f32x4v* const wa = reinterpret_cast<const f32x4v*>(wp + m * 512) + lane;
            const f32x4v a0 = wa[0], a1 = wa[64];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc[m], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b1[e], acc[m], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  const int q = q0 + col;
  if (q >= sy.y || !live0) return;
  float* const yrow = a.y + (size_t)(sy.x + q) * a.ld_y;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (m == 1 && !live1) break;
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
      const int row = 32 * (m_base + m) + 8 * j4 + 4 * hh;
      if (row >= a.ld_y) continue;
      f32x4v v = {0.f, 0.f, 0.f, 0.f};  // padding channels are written as zeros: later ops read whole chunks
      if (row < a.M) {
        const f32x4v bb = *reinterpret_cast<const f32x4v*>(a.bias + row);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float t = acc[m][4 * j4 + i] + bb[i];
          if (a.post_act == PWG_ACT_LRELU) t = t > 0.f ? t : t * a.post_slope;
          else if (a.post_act == PWG_ACT_TANH) t = tanhf(t);
          v[i] = row + i < a.M ? t : 0.f;
        }
      }
      *reinterpret_cast<f32x4v*>(yrow + row) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
constexpr int EX_MAX_K = 11, EX_MAX_C = 1024;

struct ExciteArgs {
  const float* x;
  const float* w;
  const float* b;
  const long long* row_start;
  float* out;
  long long rows;
  int n_utts, C, K;
  float slope;
};

__global__ void __launch_bounds__(256) pwg_uhg_excite_kernel(const ExciteArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ex_w[];  // [C][K] weights, then [C] biases
  const int nw = a.C * a.K;
  for (int i = threadIdx.x; i < nw; i += 256) ex_w[i] = a.w[i];
  for (int i = threadIdx.x; i < a.C; i += 256) ex_w[nw + i] = a.b ? a.b[i] : 0.f;
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
  long long t0 = a.row_start[lo], t1 = a.row_start[lo + 1];
  t0 = t0 < 0 ? 0 : t0;
  t1 = t1 > a.rows ? a.rows : t1;
  const int pad = (a.K - 1) >> 1;
  float xs[EX_MAX_K];
#pragma unroll
  for (int k = 0; k < EX_MAX_K; ++k) {
    const long long t = r - pad + k;
    xs[k] = (k < a.K && t >= t0 && t < t1) ? a.x[t] : 0.f;
  }
  float o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int ch = 4 * v + c;
    float acc = ex_w[nw + ch];
#pragma unroll
    for (int k = 0; k < EX_MAX_K; ++k)
      if (k < a.K) acc = __builtin_fmaf(ex_w[ch * a.K + k], xs[k], acc);
    o[c] = acc > 0.f ? acc : acc * a.slope;
  }
  *reinterpret_cast<float4*>(a.out + r * a.C + 4 * v) = make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace

int sconv_lds(int stride) {
  const int span = SCONV_COLS * stride + stride;
  return span * 64 + (span / stride + 1) * 16;
}

hipError_t launch_sconv(const SconvArgs& a, bool split, hipStream_t s) {
  if (a.n_blocks < 1) return hipSuccess;
  const dim3 grid((unsigned)a.n_blocks, (unsigned)((a.mt_total + 3) / 4));
  const size_t lds = (size_t)sconv_lds(a.stride);
  if (split) hipLaunchKernelGGL(pwg_uconv_sconv_kernel<true>, grid, dim3(SC_THREADS), lds, s, a);
  else hipLaunchKernelGGL(pwg_uconv_sconv_kernel<false>, grid, dim3(SC_THREADS), lds, s, a);
  return hipGetLastError();
}

}  // namespace pwg

extern "C" int pwg_uhg_excite_rows(const float* x, const float* w, const float* b, int channels, int kernel_size,
                                   float slope, const long long* row_start, int n_utts, long long rows, float* out,
                                   void* stream) {
  using pwg::set_error;
  if (!x || !w || !row_start || !out) return set_error(PWG_ERR_INVALID, "pwg_uhg_excite_rows: x, w, row_start and out must not be null");
  if (n_utts < 1 || rows < 0) return set_error(PWG_ERR_INVALID, "pwg_uhg_excite_rows: n_utts must be >= 1 and rows >= 0");
  if (channels < 16 || channels % 16 || channels > pwg::EX_MAX_C)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_uhg_excite_rows: channels must be a multiple of 16 up to 1024");
  if (kernel_size < 1 || kernel_size % 2 == 0 || kernel_size > pwg::EX_MAX_K)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_uhg_excite_rows: kernel_size must be odd and at most 11");
  if (reinterpret_cast<uintptr_t>(out) & 15) return set_error(PWG_ERR_INVALID, "pwg_uhg_excite_rows: out must be 16-byte aligned");
  const long long n_wg = (rows * (channels / 4) + 255) / 256;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_uhg_excite_rows: too many rows for one launch");
  if (rows == 0) return PWG_OK;
  pwg::ExciteArgs a;
  a.x = x; a.w = w; a.b = b; a.row_start = row_start; a.out = out; a.rows = rows;
  a.n_utts = n_utts; a.C = channels; a.K = kernel_size; a.slope = slope;
  const size_t lds = (size_t)(channels * kernel_size + channels) * sizeof(float);
  hipLaunchKernelGGL(pwg::pwg_uhg_excite_kernel, dim3((unsigned)n_wg), dim3(256), lds, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(PWG_ERR_HIP, hipGetErrorString(e));
  return PWG_OK;
}
