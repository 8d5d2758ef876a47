// Sine excitation generator (include/pwg_sine.h; reference layers/sine.py:SineGen without
// flag_for_pulse, and the f0 expansion of bin/preprocess.py:431-436).
//
// The phase is a wrapping uint64 sum of per-sample increments q = floor(rad * 2^64): exact, so any
// parallel decomposition gives the same bits, and the segmented (per utterance) sum is the plain
// running sum over all rows minus its value before the utterance's first row.
//
//   pwg_sine_samples   sample-rate f0, three launches:
//     sine_totals_kernel   workgroup b < n_blocks: the total of q over its SINE_BLOCK rows; workgroup
//                          n_blocks + u: for utterance u the sum of q from the start of the block its
//                          first row lies in up to that row, and the first sample's ini correction
//     sine_scan_kernel     one workgroup: exclusive scan of the block totals, in place
//     sine_final_kernel    in-block inclusive scan + the block's prefix - the utterance's base -> phase
//                          -> sine, uv, noise
//   pwg_sine_frames    frame-rate f0, two launches:
//     sine_frame_scan_kernel   one workgroup per utterance: inclusive prefix P over its frames, total S
//     sine_frame_final_kernel  every sample from P, S and its own frame's q in closed form
//
// A thread of the two final kernels owns 4 consecutive rows x dim channels = dim float4 stores.
// Built without fast-math: q must be bit-identical to torch's fp32 (f / sr) % 1, which needs the
// IEEE-rounded division (__fdiv_rn), fmodf, and no contraction of a * b + c into an fma.

#include <hip/hip_runtime.h>

#include <climits>
#include <string>

#include "../../include/pwg_sine.h"
#include "pwg_internal.h"

#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;

constexpr int SINE_THREADS = 256;
constexpr int SINE_RPT = 4;  // rows per thread
constexpr int SINE_BLOCK = SINE_THREADS * SINE_RPT;
constexpr int SINE_WAVES = SINE_THREADS / 64;
static_assert(SINE_BLOCK == PWG_SINE_SCAN_BLOCK, "the header names the scan's block size");

__device__ inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The last u in [0, n) with start[u] <= r (0 if none): never leaves [0, n) whatever start holds.
__device__ inline int last_le(const long long* start, int n, long long r) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Items [b, e) of utterance u out of N: utterance 0 owns what lies before its start, the last
// utterance what lies after its end; b <= e and both inside [0, N] whatever start holds.
struct Seg {
  long long b, e;
};
__device__ inline Seg seg_of(const long long* start, int n, int u, long long N) {
  Seg s;
  s.b = u == 0 ? 0 : clampll(start[u], 0, N);
  s.e = u == n - 1 ? N : clampll(start[u + 1], s.b, N);
  return s;
}

__device__ inline bool finite_f(float v) { return fabsf(v) < __builtin_huge_valf(); }  // false for a NaN too

// torch's (f_h / sr) % 1 in fp32: fmod, then + 1 where the remainder is negative (which can round to 1).
__device__ inline float rad_of(float f0, int h, float sr) {
  const float f = h == 0 ? f0 : f0 * (float)(h + 1);
  float r = fmodf(__fdiv_rn(f, sr), 1.0f);
  if (r < 0.f) r += 1.0f;
  return r;
}

// floor(rad * 2^64) mod 2^64 for rad in [0, 2]: the fraction times 2^64 is an exact fp32 product below 2^64.
__device__ inline u64 q_of_rad(float rad) {
  if (!finite_f(rad)) return 0;
  const float fr = rad - floorf(rad);
  return (u64)(fr * 18446744073709551616.0f);
}

__device__ inline u64 q_of(float f0, int h, float sr, int* bad) {
  const float r = rad_of(f0, h, sr);
  if (!finite_f(f0) || !finite_f(r)) {
    *bad = 1;
    return 0;
  }
  return q_of_rad(r);
}

// What ini adds to the utterance's first increment: q(rad + ini) - q(rad), the add in fp32.
__device__ inline u64 ini_delta(float f0, int h, float sr, float ini) {
  const float r = rad_of(f0, h, sr);
  if (!finite_f(f0) || !finite_f(r)) return 0;
  return q_of_rad(r + ini) - q_of_rad(r);
}

// sin(2 pi phase / 2^64): the phase as a signed fraction in [-1/2, 1/2) of a cycle, folded into
// [-1/4, 1/4] by sin(pi - x) = sin(x) in integers, then one int64 -> fp32 rounding (2^-26 of a cycle
// at the most) and sinpif of twice the fraction.
__device__ inline float phase_sin(u64 phase) {
  long long s = (long long)phase;
  constexpr long long quarter = 1LL << 62;
  if (s > quarter || s < -quarter) s = (long long)(0x8000000000000000ULL - (u64)s);
  return sinpif((float)s * 0x1p-63f);
}

struct Amp {
  float sine_amp, noise_std, third, threshold;  // third = sine_amp / 3 in fp32
};

__device__ inline bool voiced_of(float f0, const Amp& a) { return finite_f(f0) && f0 > a.threshold; }

__device__ inline void emit(u64 phase, bool voiced, float nv, const Amp& a, float* sine, float* noise) {
  const float z = (voiced ? a.noise_std : a.third) * nv;
  *noise = z;
  *sine = (phase_sin(phase) * a.sine_amp) * (voiced ? 1.f : 0.f) + z;
}

__device__ inline u64 wave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the workgroup; every thread gets it. `part` holds SINE_WAVES entries.
__device__ inline u64 block_sum(u64 v, u64* part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 s = 0;
  for (int w = 0; w < SINE_WAVES; ++w) s += part[w];
  return s;
}

// Inclusive scan over the workgroup's threads (thread order); `part` holds SINE_WAVES entries.
__device__ inline u64 block_scan(u64 v, u64* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  __syncthreads();
  if (lane == 63) part[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += part[w];
  return v;
}

// Stores 4 rows x DIM floats at p + r0 * DIM: DIM float4s when all 4 rows exist and p is aligned.
template <int DIM>
__device__ inline void store_rows(float* p, long long r0, long long rows, bool vec, const float (&v)[SINE_RPT * DIM]) {
  if (vec) {
    float4* o = reinterpret_cast<float4*>(p + r0 * DIM);
#pragma unroll
    for (int j = 0; j < DIM; ++j) o[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < SINE_RPT; ++k)
      if (r0 + k < rows) {
#pragma unroll
        for (int h = 0; h < DIM; ++h) p[(r0 + k) * DIM + h] = v[k * DIM + h];
      }
  }
}

template <int DIM>
__device__ inline void load_rows(const float* p, long long r0, long long rows, bool vec, float (&v)[SINE_RPT * DIM]) {
#pragma unroll
  for (int e = 0; e < SINE_RPT * DIM; ++e) v[e] = 0.f;
  if (p == nullptr) return;
  if (vec) {
    const float4* s = reinterpret_cast<const float4*>(p + r0 * DIM);
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      const float4 x = s[j];
      v[4 * j] = x.x; v[4 * j + 1] = x.y; v[4 * j + 2] = x.z; v[4 * j + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < SINE_RPT; ++k)
      if (r0 + k < rows) {
#pragma unroll
        for (int h = 0; h < DIM; ++h) v[k * DIM + h] = p[(r0 + k) * DIM + h];
      }
  }
}

__device__ inline bool aligned16_dev(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------ sample-rate f0
struct SampleArgs {
  const float* f0;
  const long long* row_start;
  const float* ini;
  const float* n;
  float* sine;
  float* uv;
  float* noise;
  u64* block_prefix;  // n_blocks x dim: block totals, then their exclusive scan
  u64* partial;       // n_utts x dim: sum of q from the start of the first row's block to the first row
  u64* delta;         // n_utts x dim: ini's correction of the first increment
  int* flag;
  long long rows, n_blocks;
  int n_utts, dim;
  float sr;
  Amp amp;
};

template <int DIM>
__global__ __launch_bounds__(SINE_THREADS) void sine_totals_kernel(SampleArgs a) {
  __shared__ u64 part[SINE_WAVES];
  const int tid = threadIdx.x;
  long long lo, hi;       // rows summed
  u64* dst;
  if (blockIdx.x < a.n_blocks) {
    lo = (long long)blockIdx.x * SINE_BLOCK;
    hi = lo + SINE_BLOCK < a.rows ? lo + SINE_BLOCK : a.rows;
    dst = a.block_prefix + (long long)blockIdx.x * DIM;
  } else {
    const int u = (int)(blockIdx.x - a.n_blocks);
    const Seg s = seg_of(a.row_start, a.n_utts, u, a.rows);
    lo = s.b / SINE_BLOCK * SINE_BLOCK;
    hi = s.b;
    dst = a.partial + (long long)u * DIM;
    if (tid < DIM) {
      const float ini = a.ini != nullptr ? a.ini[(long long)u * DIM + tid] : 0.f;
      a.delta[(long long)u * DIM + tid] = s.b < s.e ? ini_delta(a.f0[s.b], tid, a.sr, ini) : 0;
    }
  }
  u64 sum[DIM];
#pragma unroll
  for (int h = 0; h < DIM; ++h) sum[h] = 0;
  int bad = 0;
  for (long long r = lo + tid; r < hi; r += SINE_THREADS) {
    const float f = a.f0[r];
#pragma unroll
    for (int h = 0; h < DIM; ++h) sum[h] += q_of(f, h, a.sr, &bad);
  }
  if (bad && blockIdx.x < a.n_blocks) __hip_atomic_fetch_or(a.flag, PWG_SINE_BAD_F0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int h = 0; h < DIM; ++h) {
    const u64 t = block_sum(sum[h], part);
    if (tid == 0) dst[h] = t;
  }
}

// Exclusive scan, in place, of `count` rows of `dim` values: one workgroup, chunks of SINE_THREADS
// with a running carry.
__global__ __launch_bounds__(SINE_THREADS) void sine_scan_kernel(u64* v, long long count, int dim) {
  __shared__ u64 part[SINE_WAVES];
  const int tid = threadIdx.x;
  for (int h = 0; h < dim; ++h) {
    u64 carry = 0;
    for (long long base = 0; base < count; base += SINE_THREADS) {
      const long long i = base + tid;
      const u64 x = i < count ? v[i * dim + h] : 0;
      const u64 inc = block_scan(x, part);
      if (i < count) v[i * dim + h] = carry + inc - x;
      carry += part[0] + part[1] + part[2] + part[3];
      static_assert(SINE_WAVES == 4, "the carry sums four wave totals");
    }
  }
}

template <int DIM>
__global__ __launch_bounds__(SINE_THREADS) void sine_final_kernel(SampleArgs a) {
  __shared__ u64 part[SINE_WAVES];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * SINE_BLOCK + (long long)tid * SINE_RPT;
  float f[SINE_RPT];
#pragma unroll
  for (int k = 0; k < SINE_RPT; ++k) f[k] = r0 + k < a.rows ? a.f0[r0 + k] : 0.f;

  // G[k][h]: the running sum of q over all rows up to and including row r0 + k
  u64 G[SINE_RPT][DIM];
  int ignore = 0;
#pragma unroll
  for (int h = 0; h < DIM; ++h) {
    u64 run = 0;
#pragma unroll
    for (int k = 0; k < SINE_RPT; ++k) {
      run += r0 + k < a.rows ? q_of(f[k], h, a.sr, &ignore) : 0;
      G[k][h] = run;
    }
    const u64 before = block_scan(run, part) - run + a.block_prefix[(long long)blockIdx.x * DIM + h];
#pragma unroll
    for (int k = 0; k < SINE_RPT; ++k) G[k][h] += before;
  }
  if (r0 >= a.rows) return;

  const bool full = r0 + SINE_RPT <= a.rows;
  float nv[SINE_RPT * DIM], sv[SINE_RPT * DIM], zv[SINE_RPT * DIM], uvv[SINE_RPT];
  load_rows<DIM>(a.n, r0, a.rows, full && aligned16_dev(a.n), nv);
  int u = last_le(a.row_start, a.n_utts, r0);
#pragma unroll
  for (int k = 0; k < SINE_RPT; ++k) {
    const long long r = r0 + k;
    while (u + 1 < a.n_utts && a.row_start[u + 1] <= r) ++u;
    const Seg s = seg_of(a.row_start, a.n_utts, u, a.rows);
    const bool in = r >= s.b && r < s.e;  // false only where the boundaries are not sorted
    const bool voiced = in && voiced_of(f[k], a.amp);
    uvv[k] = voiced ? 1.f : 0.f;
    const long long blk = s.b / SINE_BLOCK;
#pragma unroll
    for (int h = 0; h < DIM; ++h) {
      u64 phase = 0;
      if (in) phase = G[k][h] - (a.block_prefix[blk * DIM + h] + a.partial[(long long)u * DIM + h]) + a.delta[(long long)u * DIM + h];
      emit(phase, voiced, nv[k * DIM + h], a.amp, &sv[k * DIM + h], &zv[k * DIM + h]);
    }
  }
  store_rows<DIM>(a.sine, r0, a.rows, full && aligned16_dev(a.sine), sv);
  if (a.noise != nullptr) store_rows<DIM>(a.noise, r0, a.rows, full && aligned16_dev(a.noise), zv);
  if (a.uv != nullptr) store_rows<1>(a.uv, r0, a.rows, full && aligned16_dev(a.uv), uvv);
}

// ------------------------------------------------------------------ frame-rate f0
struct FrameArgs {
  const float* f0;
  const long long* frame_start;
  const float* ini;
  const float* n;
  float* sine;
  float* uv;
  float* noise;
  u64* prefix;  // frames x dim: inclusive prefix of q within the utterance
  u64* total;   // n_utts x dim
  u64* delta;   // n_utts x dim
  int* flag;
  long long frames, rows;
  int n_utts, dim, hop, layout;
  float sr;
  Amp amp;
};

__global__ __launch_bounds__(SINE_THREADS) void sine_frame_scan_kernel(FrameArgs a) {
  __shared__ u64 part[SINE_WAVES];
  const int tid = threadIdx.x;
  const int u = blockIdx.x;
  const Seg s = seg_of(a.frame_start, a.n_utts, u, a.frames);
  int bad = 0;
  for (int h = 0; h < a.dim; ++h) {
    u64 carry = 0;
    for (long long base = s.b; base < s.e; base += SINE_THREADS) {
      const long long t = base + tid;
      const u64 x = t < s.e ? q_of(a.f0[t], h, a.sr, &bad) : 0;
      const u64 inc = block_scan(x, part);
      if (t < s.e) a.prefix[t * a.dim + h] = carry + inc;
      carry += part[0] + part[1] + part[2] + part[3];
    }
    if (tid == 0) {
      a.total[(long long)u * a.dim + h] = carry;
      const float ini = a.ini != nullptr ? a.ini[(long long)u * a.dim + h] : 0.f;
      a.delta[(long long)u * a.dim + h] = s.b < s.e ? ini_delta(a.f0[s.b], h, a.sr, ini) : 0;
    }
  }
  if (bad) __hip_atomic_fetch_or(a.flag, PWG_SINE_BAD_F0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int DIM>
__global__ __launch_bounds__(SINE_THREADS) void sine_frame_final_kernel(FrameArgs a) {
  const long long r0 = ((long long)blockIdx.x * SINE_THREADS + threadIdx.x) * SINE_RPT;
  if (r0 >= a.rows) return;
  const bool full = r0 + SINE_RPT <= a.rows;
  float nv[SINE_RPT * DIM], sv[SINE_RPT * DIM], zv[SINE_RPT * DIM], uvv[SINE_RPT];
  load_rows<DIM>(a.n, r0, a.rows, full && aligned16_dev(a.n), nv);
  const long long hop = a.hop;
  int u = last_le(a.frame_start, a.n_utts, r0 / hop);
  int ignore = 0;
#pragma unroll
  for (int k = 0; k < SINE_RPT; ++k) {
    const long long r = r0 + k < a.rows ? r0 + k : a.rows - 1;
    const long long fr = r / hop;
    while (u + 1 < a.n_utts && a.frame_start[u + 1] <= fr) ++u;
    const Seg s = seg_of(a.frame_start, a.n_utts, u, a.frames);
    const long long T = s.e - s.b;
    const bool in = fr >= s.b && fr < s.e;  // false only where the boundaries are not sorted
    const long long i = r - s.b * hop;      // the sample's index within the utterance
    long long t = 0;
    u64 rep = 0;                            // tile: full passes over the contour before this sample
    if (in) {
      if (a.layout == PWG_SINE_TILE) {
        rep = (u64)(i / T);
        t = i % T;
      } else {
        t = fr - s.b;
        rep = (u64)(i - t * hop);           // hold: the sample's position within its frame
      }
    }
    const float f = in ? a.f0[s.b + t] : 0.f;
    const bool voiced = in && voiced_of(f, a.amp);
    uvv[k] = voiced ? 1.f : 0.f;
#pragma unroll
    for (int h = 0; h < DIM; ++h) {
      u64 phase = 0;
      if (in) {
        const u64 P = a.prefix[(s.b + t) * DIM + h];
        const u64 d = a.delta[(long long)u * DIM + h];
        if (a.layout == PWG_SINE_TILE) {
          phase = rep * a.total[(long long)u * DIM + h] + P + d;
        } else {
          const u64 q = q_of(f, h, a.sr, &ignore);
          phase = (u64)hop * (P - q) + (rep + 1) * q + d;
        }
      }
      emit(phase, voiced, nv[k * DIM + h], a.amp, &sv[k * DIM + h], &zv[k * DIM + h]);
    }
  }
  store_rows<DIM>(a.sine, r0, a.rows, full && aligned16_dev(a.sine), sv);
  if (a.noise != nullptr) store_rows<DIM>(a.noise, r0, a.rows, full && aligned16_dev(a.noise), zv);
  if (a.uv != nullptr) store_rows<1>(a.uv, r0, a.rows, full && aligned16_dev(a.uv), uvv);
}

int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pwg::set_error(PWG_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  return PWG_OK;
}

template <template <int> class K, typename A>
void dispatch_dim(int dim, unsigned grid, hipStream_t st, const A& a) {
  switch (dim) {
    case 1: K<1>::launch(grid, st, a); break;
    case 2: K<2>::launch(grid, st, a); break;
    case 3: K<3>::launch(grid, st, a); break;
    case 4: K<4>::launch(grid, st, a); break;
    case 5: K<5>::launch(grid, st, a); break;
    case 6: K<6>::launch(grid, st, a); break;
    case 7: K<7>::launch(grid, st, a); break;
    default: K<8>::launch(grid, st, a); break;
  }
}

template <int DIM>
struct Totals {
  static void launch(unsigned grid, hipStream_t st, const SampleArgs& a) {
    hipLaunchKernelGGL(sine_totals_kernel<DIM>, dim3(grid), dim3(SINE_THREADS), 0, st, a);
  }
};
template <int DIM>
struct Final {
  static void launch(unsigned grid, hipStream_t st, const SampleArgs& a) {
    hipLaunchKernelGGL(sine_final_kernel<DIM>, dim3(grid), dim3(SINE_THREADS), 0, st, a);
  }
};
template <int DIM>
struct FrameFinal {
  static void launch(unsigned grid, hipStream_t st, const FrameArgs& a) {
    hipLaunchKernelGGL(sine_frame_final_kernel<DIM>, dim3(grid), dim3(SINE_THREADS), 0, st, a);
  }
};

constexpr long long SLOT = 8LL * PWG_SINE_MAX_DIM;  // scratch bytes per item at the largest dim
constexpr long long MAX_ITEMS = LLONG_MAX / 1024;   // rows * dim * 8 and the scratch sizes stay in range

// The checks both entry points share; 0 or the status to return.
int check_common(const char* fn, const float* f0, const long long* start, int n_utts, long long items,
                 const float* sine, const void* scratch, const int* flag) {
  using pwg::set_error;
  const std::string p = std::string(fn) + ": ";
  if (!f0 || !start || !sine || !scratch || !flag)
    return set_error(PWG_ERR_INVALID, (p + "f0, the utterance starts, sine, scratch and flag must not be null").c_str());
  if (n_utts < 1 || items < 0) return set_error(PWG_ERR_INVALID, (p + "n_utts must be >= 1 and the length >= 0").c_str());
  if (items > MAX_ITEMS) return set_error(PWG_ERR_INVALID, (p + "too many rows for one call").c_str());
  if (reinterpret_cast<uintptr_t>(scratch) & 7) return set_error(PWG_ERR_INVALID, (p + "scratch must be 8-byte aligned").c_str());
  return PWG_OK;
}

int check_shape(const char* fn, float sr, int dim) {
  using pwg::set_error;
  const std::string p = std::string(fn) + ": ";
  if (dim < 1 || dim > PWG_SINE_MAX_DIM) return set_error(PWG_ERR_UNSUPPORTED, (p + "dim (harmonic_num + 1) must be within 1..8").c_str());
  if (!(sr > 0.f) || !(sr < __builtin_huge_valf())) return set_error(PWG_ERR_UNSUPPORTED, (p + "sr must be positive and finite").c_str());
  return PWG_OK;
}

Amp make_amp(float sine_amp, float noise_std, float threshold) {
  Amp a;
  a.sine_amp = sine_amp;
  a.noise_std = noise_std;
  a.third = sine_amp / 3.0f;  // host fp32 division: IEEE
  a.threshold = threshold;
  return a;
}

}  // namespace

extern "C" long long pwg_sine_scratch_bytes(long long rows, int n_utts) {
  if (rows < 0 || n_utts < 0 || rows > MAX_ITEMS) return -1;
  return SLOT * ((rows + SINE_BLOCK - 1) / SINE_BLOCK + 2LL * n_utts);
}

extern "C" long long pwg_sine_frames_scratch_bytes(long long frames, int n_utts) {
  if (frames < 0 || n_utts < 0 || frames > MAX_ITEMS / SLOT) return -1;
  return SLOT * (frames + 2LL * n_utts);
}

extern "C" int pwg_sine_samples(const float* f0, const long long* row_start, int n_utts, long long rows, float sr,
                                int dim, float sine_amp, float noise_std, float voiced_threshold, const float* ini,
                                const float* n, float* sine, float* uv, float* noise, void* scratch,
                                long long scratch_bytes, int* flag, void* stream) {
  using pwg::set_error;
  int rc = check_common("pwg_sine_samples", f0, row_start, n_utts, rows, sine, scratch, flag);
  if (rc != PWG_OK) return rc;
  if (scratch_bytes < pwg_sine_scratch_bytes(rows, n_utts))
    return set_error(PWG_ERR_INVALID, "pwg_sine_samples: scratch is smaller than pwg_sine_scratch_bytes(rows, n_utts)");
  const long long n_blocks = (rows + SINE_BLOCK - 1) / SINE_BLOCK;
  if (n_blocks + n_utts > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_sine_samples: too many rows for one launch");
  rc = check_shape("pwg_sine_samples", sr, dim);
  if (rc != PWG_OK) return rc;
  if (rows == 0) return PWG_OK;
  SampleArgs a;
  a.f0 = f0; a.row_start = row_start; a.ini = ini; a.n = n; a.sine = sine; a.uv = uv; a.noise = noise;
  a.block_prefix = static_cast<u64*>(scratch);
  a.partial = a.block_prefix + n_blocks * PWG_SINE_MAX_DIM;
  a.delta = a.partial + (long long)n_utts * PWG_SINE_MAX_DIM;
  a.flag = flag; a.rows = rows; a.n_blocks = n_blocks; a.n_utts = n_utts; a.dim = dim; a.sr = sr;
  a.amp = make_amp(sine_amp, noise_std, voiced_threshold);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dim<Totals>(dim, (unsigned)(n_blocks + n_utts), st, a);
  rc = launched("pwg_sine_samples");
  if (rc != PWG_OK) return rc;
  hipLaunchKernelGGL(sine_scan_kernel, dim3(1), dim3(SINE_THREADS), 0, st, a.block_prefix, n_blocks, dim);
  rc = launched("pwg_sine_samples");
  if (rc != PWG_OK) return rc;
  dispatch_dim<Final>(dim, (unsigned)n_blocks, st, a);
  return launched("pwg_sine_samples");
}

extern "C" int pwg_sine_frames(const float* f0, const long long* frame_start, int n_utts, long long frames, int hop,
                               int layout, float sr, int dim, float sine_amp, float noise_std, float voiced_threshold,
                               const float* ini, const float* n, float* sine, float* uv, float* noise, void* scratch,
                               long long scratch_bytes, int* flag, void* stream) {
  using pwg::set_error;
  int rc = check_common("pwg_sine_frames", f0, frame_start, n_utts, frames, sine, scratch, flag);
  if (rc != PWG_OK) return rc;
  const long long need = pwg_sine_frames_scratch_bytes(frames, n_utts);
  if (need < 0 || scratch_bytes < need)
    return set_error(PWG_ERR_INVALID, "pwg_sine_frames: scratch is smaller than pwg_sine_frames_scratch_bytes(frames, n_utts)");
  if (hop < 1) return set_error(PWG_ERR_UNSUPPORTED, "pwg_sine_frames: hop must be >= 1");
  if (layout != PWG_SINE_TILE && layout != PWG_SINE_HOLD)
    return set_error(PWG_ERR_UNSUPPORTED, "pwg_sine_frames: layout must be PWG_SINE_TILE or PWG_SINE_HOLD");
  rc = check_shape("pwg_sine_frames", sr, dim);
  if (rc != PWG_OK) return rc;
  if (frames > MAX_ITEMS / hop) return set_error(PWG_ERR_INVALID, "pwg_sine_frames: too many rows for one call");
  const long long rows = frames * hop;
  constexpr long long per_wg = SINE_BLOCK;
  const long long n_wg = (rows + per_wg - 1) / per_wg;
  if (n_wg > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_sine_frames: too many rows for one launch");
  if (frames == 0) return PWG_OK;
  FrameArgs a;
  a.f0 = f0; a.frame_start = frame_start; a.ini = ini; a.n = n; a.sine = sine; a.uv = uv; a.noise = noise;
  a.prefix = static_cast<u64*>(scratch);
  a.total = a.prefix + frames * PWG_SINE_MAX_DIM;
  a.delta = a.total + (long long)n_utts * PWG_SINE_MAX_DIM;
  a.flag = flag; a.frames = frames; a.rows = rows; a.n_utts = n_utts; a.dim = dim; a.hop = hop; a.layout = layout;
  a.sr = sr;
  a.amp = make_amp(sine_amp, noise_std, voiced_threshold);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sine_frame_scan_kernel, dim3((unsigned)n_utts), dim3(SINE_THREADS), 0, st, a);
  rc = launched("pwg_sine_frames");
  if (rc != PWG_OK) return rc;
  dispatch_dim<FrameFinal>(dim, (unsigned)n_wg, st, a);
  return launched("pwg_sine_frames");
}
