// YIN f0 estimation (include/pwg_yin.h; reference bin/preprocess.py:f0_torchyin). One kernel, two phases:
//
//  * A workgroup owns YIN_TILE = 8 consecutive frames of one utterance and stages each frame's
//    W = 2 tau_max samples as a row of its own in LDS (zero past the utterance's end). The row pitch
//    is 4 (mod 32) words and a lag run is YIN_RUN = 15 lags, so the 8 frames x 4 runs of a 32-lane
//    group sit on 32 different banks whatever the hop is (4 f + 15 p mod 32 is injective there).
//  * Phase 1, the difference function in the direct form. A thread owns a run of 15 consecutive lags
//    of one frame: it keeps x[j + tau0 .. j + tau0 + 14] in registers and slides that window like an
//    FIR, so a step costs two LDS reads (x[j], one new window sample) for 15 subtract + fma pairs.
//    Each lag is ONE fp32 fma chain, j ascending. A run at lag tau0 takes W - tau0 steps, so a
//    thread takes run q and then run n_runs - 1 - q: every thread does the same work, and the 8
//    frames of one run pair share a wave's lanes, which keeps the lanes of a wave within a few
//    steps of each other. d stays in LDS.
//  * Phase 2, one wave per frame: the lanes sum contiguous chunks of d, an in-wave scan (fixed order)
//    gives each chunk's offset, a second pass turns d into c in place; then two first-hit searches
//    (threshold, local minimum), each a per-lane scan and a wave minimum. The wave that owns an
//    utterance's last frame also writes the rows held beyond it.
//
// Built without fast-math and with contraction off: the subtract is rounded, the square-and-add is one
// explicit fma, the divisions are the IEEE ones, the logarithm is taken in double and rounded once.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "../../include/pwg_yin.h"
#include "pwg_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int YIN_TILE = 8;
constexpr int YIN_RUN = 15;
constexpr int YIN_MAX_THREADS = 512;
constexpr int YIN_CHUNK = 64;  // utterances per launch
constexpr int YIN_LDS_LIMIT = 160 * 1024;
static_assert(YIN_TILE == PWG_YIN_FRAME_TILE, "the header names the frame tile");

struct YinUtt {
  long long s0;    // first sample in wave
  long long T;     // samples
  long long N;     // frames the utterance has
  long long rows;  // rows to write (beyond N: frame N - 1 held; fewer: cut)
  long long row0;  // first output row
};

struct YinArgs {
  const float* wave;
  float* f0;
  int* tau;     // nullable
  float* cmdf;  // nullable
  int tau_min, tau_max, hop, pitch, n_runs, n_pairs, log_f0;
  float fs, threshold;
  YinUtt utts[YIN_CHUNK];
};

// the row pitch of a staged frame: at least W + YIN_RUN + 1 words and 4 (mod 32)
__host__ __device__ inline int yin_pitch(int tau_max) { return (2 * tau_max + YIN_RUN + 1 + 27) / 32 * 32 + 4; }

// d(tau0 .. tau0 + 14) of the frame at xf into df (lags below tau_max only)
__device__ __forceinline__ void lag_run(const float* xf, float* df, int tau0, int W, int tau_max) {
  float w[YIN_RUN], acc[YIN_RUN];
#pragma unroll
  for (int r = 0; r < YIN_RUN; ++r) {
    w[r] = xf[tau0 + r];
    acc[r] = 0.f;
  }
  // steps [0, n_full): every lag of the run is inside the frame (j + tau0 + 14 <= W - 1)
  const int n_full = W - tau0 - YIN_RUN + 1;
  int j = 0;
  for (; j + YIN_RUN <= n_full; j += YIN_RUN) {
    const float* a = xf + j;
    const float* b = xf + j + tau0 + YIN_RUN;
#pragma unroll
    for (int s = 0; s < YIN_RUN; ++s) {
      const float x0 = a[s];
#pragma unroll
      for (int r = 0; r < YIN_RUN; ++r) {
        const float dd = x0 - w[(s + r) % YIN_RUN];  // slot (s + r) % 15 holds x[j + s + tau0 + r]
        acc[r] = fmaf(dd, dd, acc[r]);
      }
      w[s] = b[s];
    }
  }
  // the rest of each chain, straight from LDS: fewer than 2 x 15 steps per lag
#pragma unroll
  for (int r = 0; r < YIN_RUN; ++r) {
    float s = acc[r];
    const int tau = tau0 + r;
    for (int i = j; i < W - tau; ++i) {
      const float dd = xf[i] - xf[i + tau];
      s = fmaf(dd, dd, s);
    }
    if (tau < tau_max) df[tau] = s;
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(YIN_MAX_THREADS) void yin_kernel(YinArgs a) {
  extern __shared__ float smem[];
  const YinUtt u = a.utts[blockIdx.y];
  const long long n_calc = u.N < u.rows ? u.N : u.rows;
  const long long t0 = (long long)blockIdx.x * YIN_TILE;
  if (t0 >= n_calc) return;
  const int nf = n_calc - t0 < YIN_TILE ? (int)(n_calc - t0) : YIN_TILE;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int tau_max = a.tau_max, W = 2 * tau_max, P = a.pitch;
  float* xs = smem;                 // [YIN_TILE][P]
  float* d = smem + YIN_TILE * P;   // [YIN_TILE][tau_max]

  {
    const float* x = a.wave + u.s0;
    for (int f = 0; f < nf; ++f) {
      const long long p0 = (t0 + f) * a.hop;
      for (int m = tid; m < P; m += nthr) {
        const long long p = p0 + m;
        const float v = x[p < u.T ? p : u.T - 1];
        xs[f * P + m] = p < u.T ? v : 0.f;
      }
    }
  }
  __syncthreads();

  // phase 1: task = (run pair p, frame f), the frame on the fastest lanes
  const int n_tasks = a.n_pairs * YIN_TILE;
  for (int task = tid; task < n_tasks; task += nthr) {
    const int f = task % YIN_TILE, p = task / YIN_TILE;
    if (f >= nf) continue;
    const int q2 = a.n_runs - 1 - p;
    lag_run(xs + f * P, d + f * tau_max, p * YIN_RUN, W, tau_max);
    if (q2 != p) lag_run(xs + f * P, d + f * tau_max, q2 * YIN_RUN, W, tau_max);
  }
  __syncthreads();

  // phase 2: frame f of the tile on wave f % n_waves; every wave makes the same number of rounds
  const int lane = tid & 63, wave = tid >> 6, n_waves = nthr >> 6;
  const int L = tau_max - 1 - a.tau_min;
  const int chunk = (tau_max - 1 + 63) / 64;
  const int lo = 1 + lane * chunk < tau_max ? 1 + lane * chunk : tau_max;
  const int hi = lo + chunk < tau_max ? lo + chunk : tau_max;
  for (int f0 = 0; f0 < YIN_TILE; f0 += n_waves) {
    const int f = f0 + wave;
    const bool live = f < nf;
    float* df = d + (live ? f : 0) * tau_max;
    if (live) {
      float sum = 0.f;
      for (int t = lo; t < hi; ++t) sum += df[t];
      float incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
      }
      float run = __shfl_up(incl, 1);
      if (lane == 0) run = 0.f;
      for (int t = lo; t < hi; ++t) {
        const float dt = df[t];
        run += dt;
        df[t] = __fdiv_rn(dt * (float)t, fmaxf(run, 1e-5f));
      }
    }
    __syncthreads();
    if (live) {
      const int first = lo > a.tau_min + 1 ? lo : a.tau_min + 1;
      int hit = INT_MAX;
      for (int t = first; t < hi; ++t)
        if (df[t] < a.threshold) {
          hit = t;
          break;
        }
      const int fb = wave_min(hit);  // as a lag; INT_MAX: none
      int ks = 0;
      if (fb != INT_MAX && fb != a.tau_min + 1) {
        int best = INT_MAX;
        for (int t = lo > fb ? lo : fb; t < hi; ++t)
          if (t == tau_max - 1 || df[t + 1] - df[t] >= 0.f) {
            best = t;
            break;
          }
        ks = wave_min(best) - a.tau_min - 1;
      }
      float v = 0.f;
      if (ks > 0) {
        v = __fdiv_rn(a.fs, (float)(ks + a.tau_min + 1));
        if (a.log_f0) v = (float)log((double)v);  // logf is 2 ulp off; one double log per frame costs nothing
      }
      // this frame's row, and the rows held beyond the utterance's last frame
      const long long t = t0 + f;
      const long long r_end = t == u.N - 1 ? u.rows : t + 1;
      for (long long r = t; r < r_end; ++r) {
        const long long row = u.row0 + r;
        if (lane == 0) {
          a.f0[row] = v;
          if (a.tau != nullptr) a.tau[row] = ks;
        }
        if (a.cmdf != nullptr)
          for (int k = lane; k < L; k += 64) a.cmdf[row * L + k] = df[k + a.tau_min + 1];
      }
    }
  }
}

struct YinPlan {
  float fs, threshold;
  int tau_min, tau_max, hop, log_f0, pitch, n_runs, n_pairs, threads, lds, device;
};

int hip_error(const char* fn, hipError_t e) {
  return pwg::set_error(PWG_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
}

long long frames_of(long long T, int tau_max, int hop) {
  const long long W = 2LL * tau_max;
  return T < W ? 1 : 1 + (T - W) / hop;
}

}  // namespace

extern "C" long long pwg_yin_frames(long long T, int tau_max, int hop) {
  if (T < 1 || tau_max < 1 || hop < 1) return -1;
  return frames_of(T, tau_max, hop);
}

extern "C" int pwg_yin_plan_create(float fs, int tau_min, int tau_max, int hop, float threshold, int log_f0,
                                   void** plan) {
  using pwg::set_error;
  auto bad = [&](int code, const char* msg) {
    return set_error(code, (std::string("pwg_yin_plan_create: ") + msg).c_str());
  };
  const float inf = __builtin_huge_valf();
  if (!plan) return bad(PWG_ERR_INVALID, "plan must not be null");
  if (!(fs > 0.f) || !(fs < inf)) return bad(PWG_ERR_INVALID, "fs must be finite and positive");
  if (hop < 1) return bad(PWG_ERR_INVALID, "hop must be >= 1");
  if (tau_min < 0) return bad(PWG_ERR_INVALID, "tau_min must be >= 0");
  if ((long long)tau_max - 1 - tau_min < 1)
    return bad(PWG_ERR_INVALID, "tau_max - 1 - tau_min must be >= 1 (no lag to search)");
  if (!(threshold > 0.f) || !(threshold < inf)) return bad(PWG_ERR_INVALID, "threshold must be finite and positive");
  if (log_f0 != 0 && log_f0 != 1) return bad(PWG_ERR_INVALID, "log_f0 must be 0 or 1");
  if (tau_max > PWG_YIN_MAX_TAU)
    return bad(PWG_ERR_UNSUPPORTED, "tau_max above PWG_YIN_MAX_TAU: the frame tile does not fit the LDS");
  YinPlan p;
  p.fs = fs; p.threshold = threshold; p.tau_min = tau_min; p.tau_max = tau_max; p.hop = hop; p.log_f0 = log_f0;
  p.pitch = yin_pitch(tau_max);
  p.n_runs = (tau_max + YIN_RUN - 1) / YIN_RUN;
  p.n_pairs = (p.n_runs + 1) / 2;
  const int tasks = p.n_pairs * YIN_TILE;
  const int rounds = (tasks + YIN_MAX_THREADS - 1) / YIN_MAX_THREADS;
  p.threads = ((tasks + rounds - 1) / rounds + 63) / 64 * 64;
  p.lds = 4 * YIN_TILE * (p.pitch + tau_max);
  if (p.lds > YIN_LDS_LIMIT) return bad(PWG_ERR_UNSUPPORTED, "the frame tile does not fit the LDS");
  hipError_t e = hipGetDevice(&p.device);
  if (e == hipSuccess) e = pwg::allow_lds(reinterpret_cast<const void*>(yin_kernel), p.lds);
  if (e != hipSuccess) return hip_error("pwg_yin_plan_create", e);
  YinPlan* out = new (std::nothrow) YinPlan(p);
  if (out == nullptr) return set_error(PWG_ERR_HIP, "pwg_yin_plan_create: out of host memory");
  *plan = out;
  return PWG_OK;
}

extern "C" void pwg_yin_plan_destroy(void* plan) { delete static_cast<YinPlan*>(plan); }

extern "C" int pwg_yin_run(void* plan, const float* wave, const long long* sample_start, int n_utts,
                           const long long* out_frames, float* f0, int* tau, float* cmdf, long long out_rows,
                           void* stream) {
  using pwg::set_error;
  if (!plan || !wave || !sample_start || !f0)
    return set_error(PWG_ERR_INVALID, "pwg_yin_run: plan, wave, sample_start and f0 must not be null");
  if (n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_yin_run: n_utts must be >= 1");
  constexpr long long MAX_T = 1LL << 40;
  // the boundaries and the row counts first: these checks read nothing of the plan
  if (sample_start[0] < 0) return set_error(PWG_ERR_INVALID, "pwg_yin_run: sample_start must not be negative");
  for (int u = 0; u < n_utts; ++u) {
    const long long T = sample_start[u + 1] - sample_start[u];
    if (T < 0 || sample_start[u + 1] > MAX_T)
      return set_error(PWG_ERR_INVALID, "pwg_yin_run: sample_start must not decrease (or exceed 2^40)");
    if (T == 0)
      return set_error(PWG_ERR_INVALID, ("pwg_yin_run: utterance " + std::to_string(u) + " is empty").c_str());
    if (out_frames != nullptr && (out_frames[u] < 1 || out_frames[u] > MAX_T))
      return set_error(PWG_ERR_INVALID, ("pwg_yin_run: out_frames[" + std::to_string(u) + "] must be >= 1").c_str());
  }
  const YinPlan* p = static_cast<const YinPlan*>(plan);
  long long rows = 0;
  for (int u = 0; u < n_utts; ++u)
    rows += out_frames != nullptr ? out_frames[u]
                                  : frames_of(sample_start[u + 1] - sample_start[u], p->tau_max, p->hop);
  if (rows != out_rows)
    return set_error(PWG_ERR_INVALID, ("pwg_yin_run: out_rows is " + std::to_string(out_rows) +
                                       " but the row counts sum to " + std::to_string(rows)).c_str());

  int device = -1;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return hip_error("pwg_yin_run", e);
  if (device != p->device)
    return set_error(PWG_ERR_INVALID, ("pwg_yin_run: the plan lives on device " + std::to_string(p->device) +
                                       " but the current device is " + std::to_string(device)).c_str());
  YinArgs a;
  a.wave = wave; a.f0 = f0; a.tau = tau; a.cmdf = cmdf;
  a.tau_min = p->tau_min; a.tau_max = p->tau_max; a.hop = p->hop; a.pitch = p->pitch; a.n_runs = p->n_runs;
  a.n_pairs = p->n_pairs; a.log_f0 = p->log_f0; a.fs = p->fs; a.threshold = p->threshold;
  e = pwg::allow_lds(reinterpret_cast<const void*>(yin_kernel), p->lds);
  if (e != hipSuccess) return hip_error("pwg_yin_run", e);
  long long row0 = 0;
  for (int u0 = 0; u0 < n_utts; u0 += YIN_CHUNK) {
    const int n = n_utts - u0 < YIN_CHUNK ? n_utts - u0 : YIN_CHUNK;
    long long max_tiles = 0;
    std::memset(a.utts, 0, sizeof(a.utts));
    for (int i = 0; i < n; ++i) {
      YinUtt& d = a.utts[i];
      d.s0 = sample_start[u0 + i];
      d.T = sample_start[u0 + i + 1] - d.s0;
      d.N = frames_of(d.T, p->tau_max, p->hop);
      d.rows = out_frames != nullptr ? out_frames[u0 + i] : d.N;
      d.row0 = row0;
      row0 += d.rows;
      const long long calc = d.N < d.rows ? d.N : d.rows;
      const long long tiles = (calc + YIN_TILE - 1) / YIN_TILE;
      if (tiles > max_tiles) max_tiles = tiles;
    }
    if (max_tiles > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_yin_run: too many frames for one launch");
    hipLaunchKernelGGL(yin_kernel, dim3((unsigned)max_tiles, (unsigned)n), dim3(p->threads), p->lds,
                       (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_error("pwg_yin_run", e);
  }
  return PWG_OK;
}
