// Audio conditioning (include/pwg_wave.h; reference bin/preprocess.py:359-452): silence trim, polyphase
// resampling, and the fit to the feature length with the global gain and the clipping peak.
//
//  * trim_power_kernel: a workgroup of 4 waves owns TRIM_TILE = 16 consecutive frames of one utterance and
//    stages their (TRIM_TILE - 1) hop + fl samples in LDS once, padded by the mode's rule (zero, or the
//    mirror at the utterance's own ends), so HBM sees each sample once per tile. One wave per frame: lane l
//    adds the squares of samples l, l + 64, ... (consecutive lanes on consecutive banks) by fma, then a
//    fixed butterfly. The rows go to `power`.
//  * trim_bounds_kernel: one workgroup per utterance. Pass 1 takes the maximum of the utterance's rows
//    (a maximum is exact in any order), pass 2 the first and last row above the threshold. Without a
//    `power` buffer each wave takes its frames' powers from the samples itself, in the same order.
//  * resample_kernel: a workgroup owns a tile of outputs of one utterance; the taps, stored phase-major
//    (phase f = k mod up at row f, pitch odd so that the rows of a 32-lane group start on different
//    banks), and the tile's input span sit in LDS. A thread's output is one fma chain, inputs ascending,
//    its taps contiguous (descending).
//  * fit_kernel: the gather with the edge hold, the gain, and per workgroup of 4096 outputs one integer
//    atomic maximum on the bits of |out| (order-independent).
//
// Built without fast-math and with contraction off: every product and sum is the one written.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/pwg_wave.h"
#include "pwg_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVE_CHUNK = 64;  // utterances per launch
constexpr int LDS_LIMIT = 160 * 1024;
constexpr long long MAX_T = 1LL << 40;

int hip_error(const char* fn, hipError_t e) {
  return pwg::set_error(PWG_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
}

// The checks every run makes of its packed boundaries; they read nothing of a plan.
int check_starts(const char* fn, const long long* sample_start, int n_utts) {
  using pwg::set_error;
  const std::string f(fn);
  if (sample_start[0] < 0) return set_error(PWG_ERR_INVALID, (f + ": sample_start must not be negative").c_str());
  for (int u = 0; u < n_utts; ++u) {
    const long long T = sample_start[u + 1] - sample_start[u];
    if (T < 0 || sample_start[u + 1] > MAX_T)
      return set_error(PWG_ERR_INVALID, (f + ": sample_start must not decrease (or exceed 2^40)").c_str());
    if (T == 0) return set_error(PWG_ERR_INVALID, (f + ": utterance " + std::to_string(u) + " is empty").c_str());
  }
  return PWG_OK;
}

int check_device(const char* fn, int plan_device) {
  int device = -1;
  const hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return hip_error(fn, e);
  if (device != plan_device)
    return pwg::set_error(PWG_ERR_INVALID, (std::string(fn) + ": the plan lives on device " + std::to_string(plan_device) +
                                            " but the current device is " + std::to_string(device)).c_str());
  return PWG_OK;
}

// ------------------------------------------------------------------------------------------------ trim

constexpr int TRIM_TILE = 16;
constexpr int TRIM_THREADS = 256;
constexpr int BOUNDS_THREADS = 1024;
static_assert(TRIM_TILE == PWG_TRIM_FRAME_TILE, "the header names the frame tile");
static_assert(PWG_TRIM_MAX_TILE_SPAN * 4 <= LDS_LIMIT, "the tile's samples are held in LDS");

struct TrimUtt {
  long long s0;    // first sample in wave
  long long T;     // samples
  long long n;     // frames
  long long row0;  // first row in power
};

struct TrimArgs {
  const float* wave;
  float* power;       // nullable
  long long* bounds;  // the launch's first utterance
  int fl, hop, p, reflect;
  float factor;
  TrimUtt utts[WAVE_CHUNK];
};

// x[i] of an utterance of T samples under the pad rule; i in [-p, T + p)
__device__ __forceinline__ float padded_sample(const float* x, long long T, long long i, int reflect) {
  if (i >= 0 && i < T) return x[i];
  if (!reflect) return 0.f;
  if (T == 1) return x[0];
  const long long period = 2 * (T - 1);
  long long m = i % period;
  if (m < 0) m += period;
  return x[m < T ? m : period - m];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(TRIM_THREADS) void trim_power_kernel(TrimArgs a) {
  extern __shared__ float smem[];
  const TrimUtt u = a.utts[blockIdx.y];
  const long long t0 = (long long)blockIdx.x * TRIM_TILE;
  if (t0 >= u.n) return;
  const int nf = u.n - t0 < TRIM_TILE ? (int)(u.n - t0) : TRIM_TILE;
  const int tid = threadIdx.x;
  const float* x = a.wave + u.s0;
  const int span = (nf - 1) * a.hop + a.fl;
  const long long i0 = t0 * a.hop - a.p;
  for (int m = tid; m < span; m += TRIM_THREADS) smem[m] = padded_sample(x, u.T, i0 + m, a.reflect);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int f = wave; f < nf; f += TRIM_THREADS / 64) {
    const float* xf = smem + f * a.hop;
    float s = 0.f;
    for (int j = lane; j < a.fl; j += 64) s = fmaf(xf[j], xf[j], s);
    s = wave_sum(s);
    if (lane == 0) a.power[u.row0 + t0 + f] = __fdiv_rn(s, (float)a.fl);
  }
}

// P[t] straight from the samples, by one wave, in trim_power_kernel's order
__device__ __forceinline__ float frame_power(const float* x, long long T, long long t, const TrimArgs& a, int lane) {
  const long long i0 = t * a.hop - a.p;
  float s = 0.f;
  for (int j = lane; j < a.fl; j += 64) {
    const float v = padded_sample(x, T, i0 + j, a.reflect);
    s = fmaf(v, v, s);
  }
  return __fdiv_rn(wave_sum(s), (float)a.fl);
}

__global__ __launch_bounds__(BOUNDS_THREADS) void trim_bounds_kernel(TrimArgs a) {
  __shared__ float s_max[BOUNDS_THREADS / 64];
  __shared__ long long s_lo[BOUNDS_THREADS / 64], s_hi[BOUNDS_THREADS / 64];
  const TrimUtt u = a.utts[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = BOUNDS_THREADS / 64;
  const float* x = a.wave + u.s0;
  const float* rows = a.power != nullptr ? a.power + u.row0 : nullptr;

  float mx = 0.f;  // powers are non-negative
  if (rows != nullptr) {
    for (long long t = tid; t < u.n; t += BOUNDS_THREADS) mx = fmaxf(mx, rows[t]);
  } else {
    for (long long t = wave; t < u.n; t += NW) mx = fmaxf(mx, frame_power(x, u.T, t, a, lane));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if (lane == 0) s_max[wave] = mx;
  __syncthreads();
  mx = s_max[0];
  for (int w = 1; w < NW; ++w) mx = fmaxf(mx, s_max[w]);
  const float thr = fmaxf(1e-10f, mx) * a.factor;

  long long lo = LLONG_MAX, hi = -1;
  if (rows != nullptr) {
    for (long long t = tid; t < u.n; t += BOUNDS_THREADS)
      if (fmaxf(1e-10f, rows[t]) > thr) {
        lo = t < lo ? t : lo;
        hi = t;
      }
  } else {
    for (long long t = wave; t < u.n; t += NW)
      if (fmaxf(1e-10f, frame_power(x, u.T, t, a, lane)) > thr) {
        lo = t < lo ? t : lo;
        hi = t;
      }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NW; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    // with a factor below 1 the loudest frame passes; the whole utterance otherwise (a factor that rounded to 1)
    if (hi < 0) {
      lo = 0;
      hi = u.n - 1;
    }
    const long long end = (hi + 1) * a.hop;
    a.bounds[2 * blockIdx.x] = lo * a.hop < u.T ? lo * a.hop : u.T;
    a.bounds[2 * blockIdx.x + 1] = end < u.T ? end : u.T;
  }
}

struct TrimPlan {
  int fl, hop, p, reflect, device;
  float factor;
};

long long trim_frames_of(long long T, int fl, int hop) { return 1 + (T + 2LL * (fl / 2) - fl) / hop; }

// --------------------------------------------------------------------------------------------- resample

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;
static_assert(RS_TILE == PWG_RESAMPLE_OUT_TILE, "the header names the output tile");

struct RsUtt {
  long long s0;     // first sample in wave
  long long T;      // samples
  long long o0;     // first output
  long long n_out;  // outputs
};

struct RsArgs {
  const float* wave;
  const float* taps;  // phase-major image [up][pitch]
  float* out;
  int up, down, half, pitch, tile;
  RsUtt utts[WAVE_CHUNK];
};

__host__ __device__ inline long long floor_div(long long a, long long b) {  // b > 0
  const long long q = a / b;
  return a % b < 0 ? q - 1 : q;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsArgs a) {
  extern __shared__ float smem[];
  const RsUtt u = a.utts[blockIdx.y];
  const long long m0 = (long long)blockIdx.x * a.tile;
  if (m0 >= u.n_out) return;
  const int nm = u.n_out - m0 < a.tile ? (int)(u.n_out - m0) : a.tile;
  const int tid = threadIdx.x;
  const int n_img = a.up * a.pitch;
  float* tp = smem;          // [up][pitch]
  float* xs = smem + n_img;  // the tile's input span
  // inputs of outputs m0 .. m0 + nm - 1, clamped to the utterance
  long long i_lo = -floor_div(-(m0 * a.down - a.half), a.up);
  long long i_hi = floor_div((m0 + nm - 1) * a.down + a.half, a.up);
  if (i_lo < 0) i_lo = 0;
  if (i_hi > u.T - 1) i_hi = u.T - 1;
  const int n_x = i_hi >= i_lo ? (int)(i_hi - i_lo + 1) : 0;
  pwg::stage_lds(tp, a.taps, n_img, tid, RS_THREADS);
  const float* x = a.wave + u.s0 + i_lo;
  for (int i = tid; i < n_x; i += RS_THREADS) xs[i] = x[i];
  __syncthreads();
  for (int r = tid; r < nm; r += RS_THREADS) {
    const long long m = m0 + r;
    const long long c = floor_div(m * a.down + a.half, a.up);  // tap q = c - i of phase f
    const int f = (int)(m * a.down + a.half - c * a.up);
    long long lo = -floor_div(-(m * a.down - a.half), a.up);
    long long hi = c;
    if (lo < 0) lo = 0;
    if (hi > u.T - 1) hi = u.T - 1;
    const float* xp = xs + (lo - i_lo);
    const float* hp = tp + f * a.pitch + (int)(c - lo);
    const int n = (int)(hi - lo + 1);
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc = fmaf(xp[i], hp[-i], acc);
    a.out[u.o0 + m] = acc;
  }
}

struct RsPlan {
  int up, down, half, pitch, tile, lds, device;
  float* taps;  // device, [up][pitch]; null for up == down
};

long long rs_out_len(long long T, int up, int down) { return (T * up + down - 1) / down; }

// inputs a tile of `tile` outputs can span (an upper bound)
long long rs_span(long long tile, int up, int down, int half) { return ((tile - 1) * down + 2LL * half) / up + 2; }

int gcd_of(int a, int b) {
  while (b != 0) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// -------------------------------------------------------------------------------------------------- fit

constexpr int FIT_THREADS = 256;
constexpr int FIT_PER_THREAD = 16;

struct FitUtt {
  long long s0;    // first source sample
  long long len;   // source samples
  long long o0;    // first output
  long long olen;  // outputs
};

struct FitArgs {
  const float* wave;
  float* out;
  unsigned* peak;  // the launch's first utterance; nullable
  float gain;
  FitUtt utts[WAVE_CHUNK];
};

__global__ __launch_bounds__(FIT_THREADS) void fit_kernel(FitArgs a) {
  __shared__ unsigned s_pk[FIT_THREADS / 64];
  const FitUtt u = a.utts[blockIdx.y];
  const long long b0 = (long long)blockIdx.x * (FIT_THREADS * FIT_PER_THREAD);
  if (b0 >= u.olen) return;
  const float* x = a.wave + u.s0;
  float* y = a.out + u.o0;
  unsigned pk = 0;
#pragma unroll
  for (int k = 0; k < FIT_PER_THREAD; ++k) {
    const long long i = b0 + k * FIT_THREADS + threadIdx.x;
    if (i < u.olen) {
      const float v = a.gain * x[i < u.len ? i : u.len - 1];
      y[i] = v;
      const unsigned bits = __float_as_uint(fabsf(v));
      pk = bits > pk ? bits : pk;
    }
  }
  if (a.peak != nullptr) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned o = __shfl_xor(pk, off);
      pk = o > pk ? o : pk;
    }
    // one atomic per workgroup: they all land on the utterance's one word
    if ((threadIdx.x & 63) == 0) s_pk[threadIdx.x >> 6] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < FIT_THREADS / 64; ++w) pk = s_pk[w] > pk ? s_pk[w] : pk;
      if (pk != 0) atomicMax(a.peak + blockIdx.y, pk);
    }
  }
}

}  // namespace

// ================================================================================================ trim

extern "C" long long pwg_trim_frames(long long T, int fl, int hop) {
  if (T < 1 || fl < 1 || hop < 1) return -1;
  return trim_frames_of(T, fl, hop);
}

extern "C" int pwg_trim_plan_create(int fl, int hop, float top_db, int pad_mode, void** plan) {
  using pwg::set_error;
  auto bad = [&](int code, const char* msg) {
    return set_error(code, (std::string("pwg_trim_plan_create: ") + msg).c_str());
  };
  if (!plan) return bad(PWG_ERR_INVALID, "plan must not be null");
  if (fl < 1) return bad(PWG_ERR_INVALID, "fl must be >= 1");
  if (hop < 1) return bad(PWG_ERR_INVALID, "hop must be >= 1");
  if (!(top_db > 0.f) || !(top_db < __builtin_huge_valf()))
    return bad(PWG_ERR_INVALID, "top_db must be finite and positive");
  if (pad_mode != PWG_TRIM_PAD_ZERO && pad_mode != PWG_TRIM_PAD_REFLECT)
    return bad(PWG_ERR_INVALID, "pad_mode must be PWG_TRIM_PAD_ZERO or PWG_TRIM_PAD_REFLECT");
  if ((long long)(TRIM_TILE - 1) * hop + fl > PWG_TRIM_MAX_TILE_SPAN)
    return bad(PWG_ERR_UNSUPPORTED, "(PWG_TRIM_FRAME_TILE - 1) hop + fl above PWG_TRIM_MAX_TILE_SPAN: the frame tile does not fit the LDS");
  TrimPlan p;
  p.fl = fl; p.hop = hop; p.p = fl / 2; p.reflect = pad_mode == PWG_TRIM_PAD_REFLECT;
  p.factor = (float)std::pow(10.0, -(double)top_db / 10.0);
  hipError_t e = hipGetDevice(&p.device);
  if (e == hipSuccess)
    e = pwg::allow_lds(reinterpret_cast<const void*>(trim_power_kernel), 4 * PWG_TRIM_MAX_TILE_SPAN);
  if (e != hipSuccess) return hip_error("pwg_trim_plan_create", e);
  TrimPlan* out = new (std::nothrow) TrimPlan(p);
  if (out == nullptr) return set_error(PWG_ERR_HIP, "pwg_trim_plan_create: out of host memory");
  *plan = out;
  return PWG_OK;
}

extern "C" void pwg_trim_plan_destroy(void* plan) { delete static_cast<TrimPlan*>(plan); }

extern "C" int pwg_trim_run(void* plan, const float* wave, const long long* sample_start, int n_utts,
                            long long* bounds, float* power, long long power_rows, void* stream) {
  using pwg::set_error;
  if (!plan || !wave || !sample_start || !bounds)
    return set_error(PWG_ERR_INVALID, "pwg_trim_run: plan, wave, sample_start and bounds must not be null");
  if (n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_trim_run: n_utts must be >= 1");
  int rc = check_starts("pwg_trim_run", sample_start, n_utts);
  if (rc != PWG_OK) return rc;
  const TrimPlan* p = static_cast<const TrimPlan*>(plan);
  if (power != nullptr) {
    long long rows = 0;
    for (int u = 0; u < n_utts; ++u) rows += trim_frames_of(sample_start[u + 1] - sample_start[u], p->fl, p->hop);
    if (rows != power_rows)
      return set_error(PWG_ERR_INVALID, ("pwg_trim_run: power_rows is " + std::to_string(power_rows) +
                                         " but the frame counts sum to " + std::to_string(rows)).c_str());
  }
  rc = check_device("pwg_trim_run", p->device);
  if (rc != PWG_OK) return rc;
  const int lds = 4 * ((TRIM_TILE - 1) * p->hop + p->fl);
  hipError_t e = pwg::allow_lds(reinterpret_cast<const void*>(trim_power_kernel), lds);
  if (e != hipSuccess) return hip_error("pwg_trim_run", e);
  TrimArgs a;
  a.wave = wave; a.power = power;
  a.fl = p->fl; a.hop = p->hop; a.p = p->p; a.reflect = p->reflect; a.factor = p->factor;
  long long row0 = 0;
  for (int u0 = 0; u0 < n_utts; u0 += WAVE_CHUNK) {
    const int n = n_utts - u0 < WAVE_CHUNK ? n_utts - u0 : WAVE_CHUNK;
    long long max_tiles = 0;
    std::memset(a.utts, 0, sizeof(a.utts));
    for (int i = 0; i < n; ++i) {
      TrimUtt& d = a.utts[i];
      d.s0 = sample_start[u0 + i];
      d.T = sample_start[u0 + i + 1] - d.s0;
      d.n = trim_frames_of(d.T, p->fl, p->hop);
      d.row0 = row0;
      row0 += d.n;
      const long long tiles = (d.n + TRIM_TILE - 1) / TRIM_TILE;
      if (tiles > max_tiles) max_tiles = tiles;
    }
    if (max_tiles > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_trim_run: too many frames for one launch");
    a.bounds = bounds + 2LL * u0;
    if (power != nullptr) {
      hipLaunchKernelGGL(trim_power_kernel, dim3((unsigned)max_tiles, (unsigned)n), dim3(TRIM_THREADS), lds,
                         (hipStream_t)stream, a);
      e = hipGetLastError();
      if (e != hipSuccess) return hip_error("pwg_trim_run", e);
    }
    hipLaunchKernelGGL(trim_bounds_kernel, dim3((unsigned)n), dim3(BOUNDS_THREADS), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_error("pwg_trim_run", e);
  }
  return PWG_OK;
}

// ============================================================================================ resample

extern "C" long long pwg_resample_out_len(long long T, int up, int down) {
  if (T < 1 || up < 1 || down < 1 || T > MAX_T) return -1;
  const int g = gcd_of(up, down);
  return rs_out_len(T, up / g, down / g);
}

extern "C" int pwg_resample_plan_create(int up, int down, const float* taps, int tap_count, void** plan) {
  using pwg::set_error;
  auto bad = [&](int code, const char* msg) {
    return set_error(code, (std::string("pwg_resample_plan_create: ") + msg).c_str());
  };
  if (!plan || !taps) return bad(PWG_ERR_INVALID, "plan and taps must not be null");
  if (up < 1 || down < 1) return bad(PWG_ERR_INVALID, "up and down must be >= 1");
  if (tap_count < 1 || tap_count % 2 == 0) return bad(PWG_ERR_INVALID, "tap_count must be odd and >= 1");
  const int g = gcd_of(up, down);
  up /= g;
  down /= g;
  if (up > PWG_RESAMPLE_MAX_RATE || down > PWG_RESAMPLE_MAX_RATE)
    return bad(PWG_ERR_UNSUPPORTED, "the reduced up or down is above PWG_RESAMPLE_MAX_RATE");
  if (tap_count > PWG_RESAMPLE_MAX_TAPS) return bad(PWG_ERR_UNSUPPORTED, "tap_count above PWG_RESAMPLE_MAX_TAPS");
  RsPlan p;
  p.up = up; p.down = down; p.half = tap_count / 2; p.taps = nullptr;
  const int q = (tap_count + up - 1) / up;
  p.pitch = q | 1;
  const long long n_img = (long long)up * p.pitch;
  // the largest tile whose input span fits next to the taps; one output always does
  const long long room = LDS_LIMIT / 4 - n_img;
  long long tile = RS_TILE;
  if (rs_span(tile, up, down, p.half) > room) tile = 1 + ((room - 2) * up - 2LL * p.half) / down;
  if (tile < 1 || rs_span(tile, up, down, p.half) > room)
    return bad(PWG_ERR_UNSUPPORTED, "the taps and one output's inputs do not fit the LDS");
  p.tile = (int)tile;
  p.lds = (int)(4 * (n_img + rs_span(tile, up, down, p.half)));
  hipError_t e = hipGetDevice(&p.device);
  if (e != hipSuccess) return hip_error("pwg_resample_plan_create", e);
  if (up != down) {
    std::vector<float> img((size_t)n_img, 0.f);
    for (int k = 0; k < tap_count; ++k) img[(size_t)(k % up) * p.pitch + k / up] = taps[k];
    e = pwg::allow_lds(reinterpret_cast<const void*>(resample_kernel), p.lds);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p.taps), sizeof(float) * n_img);
    if (e == hipSuccess) {
      e = hipMemcpy(p.taps, img.data(), sizeof(float) * n_img, hipMemcpyHostToDevice);
      if (e != hipSuccess) (void)hipFree(p.taps);
    }
    if (e != hipSuccess) return hip_error("pwg_resample_plan_create", e);
  }
  RsPlan* out = new (std::nothrow) RsPlan(p);
  if (out == nullptr) {
    if (p.taps != nullptr) (void)hipFree(p.taps);
    return set_error(PWG_ERR_HIP, "pwg_resample_plan_create: out of host memory");
  }
  *plan = out;
  return PWG_OK;
}

extern "C" void pwg_resample_plan_destroy(void* plan) {
  RsPlan* p = static_cast<RsPlan*>(plan);
  if (p == nullptr) return;
  if (p->taps != nullptr) (void)hipFree(p->taps);
  delete p;
}

extern "C" int pwg_resample_plan_tile(void* plan) { return plan ? static_cast<const RsPlan*>(plan)->tile : -1; }

extern "C" int pwg_resample_run(void* plan, const float* wave, const long long* sample_start, int n_utts,
                                float* out, long long out_total, void* stream) {
  using pwg::set_error;
  if (!plan || !wave || !sample_start || !out)
    return set_error(PWG_ERR_INVALID, "pwg_resample_run: plan, wave, sample_start and out must not be null");
  if (n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_resample_run: n_utts must be >= 1");
  int rc = check_starts("pwg_resample_run", sample_start, n_utts);
  if (rc != PWG_OK) return rc;
  const RsPlan* p = static_cast<const RsPlan*>(plan);
  long long total = 0;
  for (int u = 0; u < n_utts; ++u) total += rs_out_len(sample_start[u + 1] - sample_start[u], p->up, p->down);
  if (total != out_total)
    return set_error(PWG_ERR_INVALID, ("pwg_resample_run: out_total is " + std::to_string(out_total) +
                                       " but the output lengths sum to " + std::to_string(total)).c_str());
  rc = check_device("pwg_resample_run", p->device);
  if (rc != PWG_OK) return rc;
  hipError_t e;
  if (p->up == p->down) {
    e = hipMemcpyAsync(out, wave + sample_start[0], sizeof(float) * (size_t)total, hipMemcpyDeviceToDevice,
                       (hipStream_t)stream);
    return e == hipSuccess ? PWG_OK : hip_error("pwg_resample_run", e);
  }
  e = pwg::allow_lds(reinterpret_cast<const void*>(resample_kernel), p->lds);
  if (e != hipSuccess) return hip_error("pwg_resample_run", e);
  RsArgs a;
  a.wave = wave; a.taps = p->taps; a.out = out;
  a.up = p->up; a.down = p->down; a.half = p->half; a.pitch = p->pitch; a.tile = p->tile;
  long long o0 = 0;
  for (int u0 = 0; u0 < n_utts; u0 += WAVE_CHUNK) {
    const int n = n_utts - u0 < WAVE_CHUNK ? n_utts - u0 : WAVE_CHUNK;
    long long max_tiles = 0;
    std::memset(a.utts, 0, sizeof(a.utts));
    for (int i = 0; i < n; ++i) {
      RsUtt& d = a.utts[i];
      d.s0 = sample_start[u0 + i];
      d.T = sample_start[u0 + i + 1] - d.s0;
      d.n_out = rs_out_len(d.T, p->up, p->down);
      d.o0 = o0;
      o0 += d.n_out;
      const long long tiles = (d.n_out + p->tile - 1) / p->tile;
      if (tiles > max_tiles) max_tiles = tiles;
    }
    if (max_tiles > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_resample_run: too many outputs for one launch");
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)max_tiles, (unsigned)n), dim3(RS_THREADS), p->lds,
                       (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_error("pwg_resample_run", e);
  }
  return PWG_OK;
}

// ================================================================================================= fit

extern "C" int pwg_wave_fit_run(const float* wave, const long long* src_start, const long long* src_len, float* out,
                                const long long* out_start, int n_utts, float gain, float* peak, void* stream) {
  using pwg::set_error;
  if (!wave || !src_start || !src_len || !out || !out_start)
    return set_error(PWG_ERR_INVALID, "pwg_wave_fit_run: wave, src_start, src_len, out and out_start must not be null");
  if (n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_wave_fit_run: n_utts must be >= 1");
  if (out_start[0] < 0) return set_error(PWG_ERR_INVALID, "pwg_wave_fit_run: out_start must not be negative");
  for (int u = 0; u < n_utts; ++u) {
    if (src_start[u] < 0 || src_start[u] > MAX_T)
      return set_error(PWG_ERR_INVALID, ("pwg_wave_fit_run: src_start[" + std::to_string(u) + "] must be >= 0").c_str());
    if (src_len[u] < 1 || src_len[u] > MAX_T)
      return set_error(PWG_ERR_INVALID, ("pwg_wave_fit_run: src_len[" + std::to_string(u) + "] must be >= 1").c_str());
    const long long n = out_start[u + 1] - out_start[u];
    if (n < 0 || out_start[u + 1] > MAX_T)
      return set_error(PWG_ERR_INVALID, "pwg_wave_fit_run: out_start must not decrease (or exceed 2^40)");
    if (n == 0)
      return set_error(PWG_ERR_INVALID, ("pwg_wave_fit_run: output " + std::to_string(u) + " is empty").c_str());
  }
  if (!(gain == gain) || gain == __builtin_huge_valf() || gain == -__builtin_huge_valf())
    return set_error(PWG_ERR_INVALID, "pwg_wave_fit_run: gain must be finite");
  hipError_t e;
  if (peak != nullptr) {
    e = hipMemsetAsync(peak, 0, sizeof(float) * (size_t)n_utts, (hipStream_t)stream);
    if (e != hipSuccess) return hip_error("pwg_wave_fit_run", e);
  }
  FitArgs a;
  a.wave = wave; a.out = out; a.gain = gain;
  constexpr long long PER_BLOCK = FIT_THREADS * FIT_PER_THREAD;
  for (int u0 = 0; u0 < n_utts; u0 += WAVE_CHUNK) {
    const int n = n_utts - u0 < WAVE_CHUNK ? n_utts - u0 : WAVE_CHUNK;
    long long max_blocks = 0;
    std::memset(a.utts, 0, sizeof(a.utts));
    for (int i = 0; i < n; ++i) {
      FitUtt& d = a.utts[i];
      d.s0 = src_start[u0 + i];
      d.len = src_len[u0 + i];
      d.o0 = out_start[u0 + i];
      d.olen = out_start[u0 + i + 1] - d.o0;
      const long long blocks = (d.olen + PER_BLOCK - 1) / PER_BLOCK;
      if (blocks > max_blocks) max_blocks = blocks;
    }
    if (max_blocks > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_wave_fit_run: too many samples for one launch");
    a.peak = peak != nullptr ? reinterpret_cast<unsigned*>(peak) + u0 : nullptr;
    hipLaunchKernelGGL(fit_kernel, dim3((unsigned)max_blocks, (unsigned)n), dim3(FIT_THREADS), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_error("pwg_wave_fit_run", e);
  }
  return PWG_OK;
}
