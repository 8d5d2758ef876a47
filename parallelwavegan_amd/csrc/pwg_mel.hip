// Log-mel feature extraction (include/pwg_mel.h; reference bin/preprocess.py:logmelfilterbank and
// losses/mel_loss.py:MelSpectrogram): STFT as a windowed-DFT GEMM on the exact-fp32 MFMA, fused with
// magnitude, mel projection, clamp, log and normalisation. One kernel, mel_kernel<MT>:
//
//  * A workgroup (4 waves) owns MEL_TILE = 64 consecutive frames of one utterance. It stages the
//    sample span those frames cover, (64 - 1) hop + K floats (K = win_length rounded up to 8), into
//    LDS once, reflection resolved while staging. Span sample i lives at word i + (i / hop) pad with
//    pad = 1 for an even hop: the B fragment of v_mfma_f32_32x32x2_f32 has one frame per lane, so
//    lanes read words hop + pad apart, and an odd stride spreads 32 lanes over 32 banks (a bare
//    hop of 256 would put them all on one).
//  * The bins [0, n_fft / 2) are cut into tiles of 32; wave w takes tiles w, w + 4, ... For a tile
//    it runs the K loop with four accumulators: cos and sin x frames [0, 32) and [32, 64). The A
//    fragments (basis rows) stream from L2 as one float4 per lane and trig per four k-steps, read a
//    group ahead; the two B reads of a step serve both trigs. The Nyquist bin rides in the sine
//    slot of bin 0, whose own sine is zero, so n_fft / 2 + 1 bins cost n_fft / 2 rows.
//  * C of the DFT has the frame on the lane and the bins of the tile in the 16 registers, register
//    r of lane half h holding bin (r & 3) + 8 (r >> 2) + 4 h. That is exactly the B operand of a
//    32x32x2 step whose two k are those two bins, so after the magnitude the amplitudes go into the
//    mel GEMM from the registers, without LDS: 16 steps per (bin tile, 32 mels, 32 frames), the mel
//    matrix packed in that k order. Mel-row tiles whose weights are all zero on a bin tile (most:
//    a filter is a narrow triangle) are skipped by a host-built mask.
//  * The four waves' mel sums meet in LDS in wave order (fixed order: the same bits whatever the
//    batch), the Nyquist column is added, and 256 threads clamp, log, normalise and store rows.
//
// Built without fast-math; sqrtf, log10f, log2f, logf and the division are the precise ones.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pwg_mel.h"
#include "pwg_internal.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4v = __attribute__((ext_vector_type(4))) float;

constexpr int MEL_TILE = 64;
constexpr int MEL_THREADS = 256;
constexpr int MEL_WAVES = MEL_THREADS / 64;
constexpr int MEL_RED_PITCH = MEL_TILE + 1;  // floats per mel row of the reduction image
constexpr int MEL_CHUNK = 64;                // utterances per launch
constexpr int MEL_LDS_LIMIT = 160 * 1024;
constexpr long long MEL_BASIS_LIMIT = 1LL << 28;  // floats of the fragment-ordered basis (1 GiB)
static_assert(MEL_TILE == PWG_MEL_FRAME_TILE, "the header names the frame tile");

struct MelUtt {
  long long s0;    // first sample in wave
  long long T;     // samples
  long long row0;  // first output row
};

struct MelArgs {
  const float* wave;
  float* out;
  const float* basis;          // [n_bt][nk4][cos, sin][64 lanes][4]
  const float* melfrag;        // [n_bt][MT][4][64 lanes][4]
  const unsigned char* mask;   // [n_bt]: bit m set when mel-row tile m has a weight on the bin tile
  const float* nyq;            // [num_mels]: the Nyquist column of melmat
  const float* mean;           // nullable
  const float* scale;
  int half, off, hop, pad, nk4, n_bt, num_mels, span, log_kind, amp_floor;
  float eps;
  MelUtt utts[MEL_CHUNK];
};

template <int MT>
__global__ __launch_bounds__(MEL_THREADS) void mel_kernel(MelArgs a) {
  extern __shared__ float smem[];
  const MelUtt u = a.utts[blockIdx.y];
  const long long frames = 1 + u.T / a.hop;
  const long long t0 = (long long)blockIdx.x * MEL_TILE;
  if (t0 >= frames) return;
  const int nf = frames - t0 < MEL_TILE ? (int)(frames - t0) : MEL_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hop = a.hop, pad = a.pad;

  float* xs = smem;                                     // the staged span
  float* red = smem + (a.span + a.span / hop * pad + pad + 3) / 4 * 4;  // [MT * 32][MEL_RED_PITCH]
  float* nyq_amp = red + MT * 32 * MEL_RED_PITCH;       // [MEL_TILE]

  // span sample i is utterance sample t0 hop - n_fft / 2 + off + i, mirrored once and clamped
  {
    const long long p0 = t0 * hop - a.half + a.off;
    const float* x = a.wave + u.s0;
    for (int i = tid; i < a.span; i += MEL_THREADS) {
      long long p = p0 + i;
      if (p < 0) p = -p;
      if (p >= u.T) p = 2 * (u.T - 1) - p;
      p = p < 0 ? 0 : (p >= u.T ? u.T - 1 : p);
      xs[i + i / hop * pad] = x[p];
    }
  }
  __syncthreads();

  const int j = lane & 31, h = lane >> 5;
  const int pitch = hop + pad;
  const float* const b0 = xs + j * pitch;
  const float* const b1 = xs + (j + 32) * pitch;

  f32x16 mel[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) mel[m][f][r] = 0.f;
  float nq0 = 0.f, nq1 = 0.f;

  for (int bt = wave; bt < a.n_bt; bt += MEL_WAVES) {
    f32x16 c0, c1, s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) c0[r] = c1[r] = s0[r] = s1[r] = 0.f;
    const f32x4v* bp = reinterpret_cast<const f32x4v*>(a.basis) + (long long)bt * a.nk4 * 128 + lane;
    // tap n = 2 step + h sits at word o = n + (n / hop) pad of a frame's row; rem = n % hop
    int rem = h, o = h;
    while (rem >= hop) {
      rem -= hop;
      o += pad;
    }
    f32x4v ac = bp[0], as = bp[64];
    for (int g = 0; g < a.nk4; ++g) {
      const int gn = g + 1 < a.nk4 ? g + 1 : g;
      const f32x4v nc = bp[gn * 128], ns = bp[gn * 128 + 64];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float x0 = b0[o], x1 = b1[o];
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[q], x0, c0, 0, 0, 0);
        s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(as[q], x0, s0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[q], x1, c1, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(as[q], x1, s1, 0, 0, 0);
        rem += 2;
        o += 2;
        while (rem >= hop) {
          rem -= hop;
          o += pad;
        }
      }
      ac = nc;
      as = ns;
    }

    // magnitude, in place in c0 / c1; bin 0's sine slot is the Nyquist bin
    const bool dc = bt == 0 && h == 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float p0 = c0[r] * c0[r] + s0[r] * s0[r];
      float p1 = c1[r] * c1[r] + s1[r] * s1[r];
      if (r == 0 && dc) {
        float q0 = s0[0] * s0[0], q1 = s1[0] * s1[0];
        p0 = c0[0] * c0[0];
        p1 = c1[0] * c1[0];
        if (a.amp_floor) {
          q0 = fmaxf(q0, a.eps);
          q1 = fmaxf(q1, a.eps);
        }
        nq0 = sqrtf(q0);
        nq1 = sqrtf(q1);
      }
      if (a.amp_floor) {
        p0 = fmaxf(p0, a.eps);
        p1 = fmaxf(p1, a.eps);
      }
      c0[r] = sqrtf(p0);
      c1[r] = sqrtf(p1);
    }

    const unsigned msk = a.mask[bt];
    const f32x4v* mp = reinterpret_cast<const f32x4v*>(a.melfrag) + (long long)bt * MT * 256 + lane;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (msk & (1u << m)) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x4v w = mp[(m * 4 + r4) * 64];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            mel[m][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q], c0[4 * r4 + q], mel[m][0], 0, 0, 0);
            mel[m][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q], c1[4 * r4 + q], mel[m][1], 0, 0, 0);
          }
        }
      }
    }
  }

  // the waves' sums meet in wave order; a wave that had no bin tile holds zeros
  if (wave == 0 && h == 0) {
    nyq_amp[j] = nq0;
    nyq_amp[j + 32] = nq1;
  }
  for (int w = 0; w < MEL_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* d = red + (m * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * MEL_RED_PITCH + f * 32 + j;
            *d = w == 0 ? mel[m][f][r] : *d + mel[m][f][r];
          }
    }
    __syncthreads();
  }

  const int total = nf * a.num_mels;
  float* const orow = a.out + (u.row0 + t0) * a.num_mels;
  for (int e = tid; e < total; e += MEL_THREADS) {
    const int t = e / a.num_mels, m = e - t * a.num_mels;
    float v = red[m * MEL_RED_PITCH + t] + nyq_amp[t] * a.nyq[m];
    v = fmaxf(v, a.eps);
    v = a.log_kind == 0 ? log10f(v) : (a.log_kind == 1 ? log2f(v) : logf(v));
    if (a.mean != nullptr) v = __fdiv_rn(v - a.mean[m], a.scale[m]);
    orow[e] = v;
  }
}

struct MelPlan {
  int n_fft, win, hop, num_mels, mt, off, pad, kp, nk4, n_bt, span, lds, log_kind, amp_floor;
  float eps;
  int device;
  float* d_basis = nullptr;
  float* d_melfrag = nullptr;
  unsigned char* d_mask = nullptr;
  float* d_nyq = nullptr;
  float* d_mean = nullptr;
  float* d_scale = nullptr;
};

const void* kernel_of(int mt) {
  switch (mt) {
    case 1: return reinterpret_cast<const void*>(mel_kernel<1>);
    case 2: return reinterpret_cast<const void*>(mel_kernel<2>);
    case 3: return reinterpret_cast<const void*>(mel_kernel<3>);
    default: return reinterpret_cast<const void*>(mel_kernel<4>);
  }
}

void launch(int mt, dim3 grid, int lds, hipStream_t st, const MelArgs& a) {
  switch (mt) {
    case 1: hipLaunchKernelGGL(mel_kernel<1>, grid, dim3(MEL_THREADS), lds, st, a); break;
    case 2: hipLaunchKernelGGL(mel_kernel<2>, grid, dim3(MEL_THREADS), lds, st, a); break;
    case 3: hipLaunchKernelGGL(mel_kernel<3>, grid, dim3(MEL_THREADS), lds, st, a); break;
    default: hipLaunchKernelGGL(mel_kernel<4>, grid, dim3(MEL_THREADS), lds, st, a); break;
  }
}

int hip_error(const char* fn, hipError_t e) {
  return pwg::set_error(PWG_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
}

template <typename T>
hipError_t upload(T** dst, const std::vector<T>& src) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

int plan_build(int n_fft, int win_length, int hop, int num_mels, const float* melmat, float eps, int log_kind,
               int amp_floor, const float* mean, const float* scale, void** plan);

void free_plan(MelPlan* p) {
  if (p == nullptr) return;
  for (void* d : {(void*)p->d_basis, (void*)p->d_melfrag, (void*)p->d_mask, (void*)p->d_nyq, (void*)p->d_mean,
                  (void*)p->d_scale})
    if (d != nullptr) (void)hipFree(d);
  delete p;
}

}  // namespace

extern "C" long long pwg_mel_frames(long long T, int hop) {
  if (T < 0 || hop < 1) return -1;
  return 1 + T / hop;
}

extern "C" int pwg_mel_plan_create(int n_fft, int win_length, int hop, int window, int num_mels, const float* melmat,
                                   long long melmat_count, float eps, float log_base, int amp_floor,
                                   const float* mean, const float* scale, void** plan) {
  using pwg::set_error;
  const char* fn = "pwg_mel_plan_create: ";
  auto bad = [&](int code, const char* msg) { return set_error(code, (std::string(fn) + msg).c_str()); };
  if (!melmat || !plan) return bad(PWG_ERR_INVALID, "melmat and plan must not be null");
  if (n_fft < 2 || (n_fft & 1)) return bad(PWG_ERR_INVALID, "n_fft must be even and at least 2");
  if (win_length < 1 || win_length > n_fft) return bad(PWG_ERR_INVALID, "win_length must be within 1..n_fft");
  if (hop < 1) return bad(PWG_ERR_INVALID, "hop must be >= 1");
  if (num_mels < 1) return bad(PWG_ERR_INVALID, "num_mels must be >= 1");
  if (melmat_count != (long long)num_mels * (n_fft / 2 + 1))
    return bad(PWG_ERR_INVALID, "melmat must hold num_mels x (n_fft / 2 + 1) values");
  if (!(eps >= 0.f) || !(eps < __builtin_huge_valf())) return bad(PWG_ERR_INVALID, "eps must be finite and >= 0");
  if (amp_floor != 0 && amp_floor != 1) return bad(PWG_ERR_INVALID, "amp_floor must be 0 or 1");
  if ((mean == nullptr) != (scale == nullptr)) return bad(PWG_ERR_INVALID, "mean and scale come together");
  if (window != PWG_MEL_WINDOW_HANN) return bad(PWG_ERR_UNSUPPORTED, "the Hann window is the only one");
  int log_kind;
  if (log_base == 10.f) log_kind = 0;
  else if (log_base == 2.f) log_kind = 1;
  else if (log_base == 0.f) log_kind = 2;
  else return bad(PWG_ERR_UNSUPPORTED, "log_base must be 10, 2 or 0 (natural)");
  if (num_mels > PWG_MEL_MAX_MELS) return bad(PWG_ERR_UNSUPPORTED, "num_mels above PWG_MEL_MAX_MELS");
  if (n_fft > 65536) return bad(PWG_ERR_UNSUPPORTED, "n_fft above 65536");
  // the fragment-ordered basis: ceil(n_fft / 64) bin tiles x win_length rounded up to 8, cos and sin
  const long long basis_floats = (long long)((n_fft / 2 + 31) / 32) * ((win_length + 7) / 8) * 512;
  if (basis_floats > MEL_BASIS_LIMIT) return bad(PWG_ERR_UNSUPPORTED, "the windowed basis would exceed 1 GiB");
  return plan_build(n_fft, win_length, hop, num_mels, melmat, eps, log_kind, amp_floor, mean, scale, plan);
}

namespace {

// Everything of pwg_mel_plan_create after the checks; throws std::bad_alloc where the host is out of memory.
int plan_build_unguarded(int n_fft, int win_length, int hop, int num_mels, const float* melmat, float eps, int log_kind,
                         int amp_floor, const float* mean, const float* scale, void** plan) {
  using pwg::set_error;
  auto bad = [&](int code, const char* msg) {
    return set_error(code, (std::string("pwg_mel_plan_create: ") + msg).c_str());
  };
  std::unique_ptr<MelPlan, void (*)(MelPlan*)> holder(new MelPlan, free_plan);
  MelPlan* p = holder.get();
  p->n_fft = n_fft; p->win = win_length; p->hop = hop; p->num_mels = num_mels;
  p->mt = (num_mels + 31) / 32;
  p->off = (n_fft - win_length) / 2;
  p->pad = (hop & 1) ? 0 : 1;
  p->kp = (win_length + 7) / 8 * 8;
  p->nk4 = p->kp / 8;
  const int half = n_fft / 2;
  p->n_bt = (half + 31) / 32;
  p->eps = eps; p->log_kind = log_kind; p->amp_floor = amp_floor;
  const long long span = (long long)(MEL_TILE - 1) * hop + p->kp;
  const long long xs_words = (span + span / hop * p->pad + p->pad + 3) / 4 * 4;
  const long long lds = 4 * (xs_words + (long long)p->mt * 32 * MEL_RED_PITCH + MEL_TILE);
  if (lds > MEL_LDS_LIMIT) return bad(PWG_ERR_UNSUPPORTED, "the sample span of a frame tile does not fit the LDS");
  p->span = (int)span;
  p->lds = (int)lds;

  // the windowed basis: float64, the angle reduced in integers, one rounding to fp32
  std::vector<double> ct(n_fft), st(n_fft), w(p->kp, 0.0);
  const double two_pi = 6.283185307179586476925286766559;
  for (int i = 0; i < n_fft; ++i) {
    ct[i] = std::cos(two_pi * i / n_fft);
    st[i] = std::sin(two_pi * i / n_fft);
  }
  for (int i = 0; i < win_length; ++i) w[i] = 0.5 - 0.5 * std::cos(two_pi * i / win_length);
  std::vector<float> basis((size_t)p->n_bt * p->nk4 * 512, 0.f);
  for (int bt = 0; bt < p->n_bt; ++bt)
    for (int g = 0; g < p->nk4; ++g)
      for (int l = 0; l < 64; ++l)
        for (int q = 0; q < 4; ++q) {
          const int tap = 2 * (4 * g + q) + (l >> 5), bin = bt * 32 + (l & 31);
          if (tap >= win_length || bin >= half) continue;
          const long long n = p->off + tap;
          const int ang = (int)(n * bin % n_fft);
          const size_t base = (((size_t)bt * p->nk4 + g) * 2 * 64 + l) * 4 + q;
          basis[base] = (float)(w[tap] * ct[ang]);
          // bin 0 has no sine: its slot carries the Nyquist bin, cos(pi n)
          basis[base + 256] = bin == 0 ? (float)((n & 1) ? -w[tap] : w[tap]) : (float)(-w[tap] * st[ang]);
        }
  const int n_bins = half + 1;
  std::vector<float> melfrag((size_t)p->n_bt * p->mt * 1024, 0.f);
  std::vector<unsigned char> mask(p->n_bt, 0);
  for (int bt = 0; bt < p->n_bt; ++bt)
    for (int m = 0; m < p->mt; ++m)
      for (int r = 0; r < 16; ++r)
        for (int l = 0; l < 64; ++l) {
          const int row = m * 32 + (l & 31), bin = bt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
          if (row >= num_mels || bin >= half) continue;
          const float v = melmat[(size_t)row * n_bins + bin];
          melfrag[((((size_t)bt * p->mt + m) * 4 + (r >> 2)) * 64 + l) * 4 + (r & 3)] = v;
          if (v != 0.f) mask[bt] |= (unsigned char)(1u << m);
        }
  std::vector<float> nyq(num_mels);
  for (int m = 0; m < num_mels; ++m) nyq[m] = melmat[(size_t)m * n_bins + half];

  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess) e = upload(&p->d_basis, basis);
  if (e == hipSuccess) e = upload(&p->d_melfrag, melfrag);
  if (e == hipSuccess) e = upload(&p->d_mask, mask);
  if (e == hipSuccess) e = upload(&p->d_nyq, nyq);
  if (e == hipSuccess && mean != nullptr) {
    e = upload(&p->d_mean, std::vector<float>(mean, mean + num_mels));
    if (e == hipSuccess) e = upload(&p->d_scale, std::vector<float>(scale, scale + num_mels));
  }
  if (e == hipSuccess) e = pwg::allow_lds(kernel_of(p->mt), p->lds);
  if (e != hipSuccess) return hip_error("pwg_mel_plan_create", e);
  *plan = holder.release();
  return PWG_OK;
}

int plan_build(int n_fft, int win_length, int hop, int num_mels, const float* melmat, float eps, int log_kind,
               int amp_floor, const float* mean, const float* scale, void** plan) {
  try {
    return plan_build_unguarded(n_fft, win_length, hop, num_mels, melmat, eps, log_kind, amp_floor, mean, scale, plan);
  } catch (const std::exception& ex) {  // no exception crosses the C ABI
    return pwg::set_error(PWG_ERR_HIP, (std::string("pwg_mel_plan_create: out of host memory (") + ex.what() + ")").c_str());
  }
}

}  // namespace

extern "C" void pwg_mel_plan_destroy(void* plan) { free_plan(static_cast<MelPlan*>(plan)); }

extern "C" int pwg_mel_run(void* plan, const float* wave, const long long* sample_start, int n_utts, float* out,
                           long long out_rows, void* stream) {
  using pwg::set_error;
  if (!plan || !wave || !sample_start || !out)
    return set_error(PWG_ERR_INVALID, "pwg_mel_run: plan, wave, sample_start and out must not be null");
  if (n_utts < 1) return set_error(PWG_ERR_INVALID, "pwg_mel_run: n_utts must be >= 1");
  const MelPlan* p = static_cast<const MelPlan*>(plan);
  constexpr long long MAX_T = 1LL << 40;
  if (sample_start[0] < 0) return set_error(PWG_ERR_INVALID, "pwg_mel_run: sample_start must not be negative");
  long long rows = 0;
  for (int u = 0; u < n_utts; ++u) {
    const long long T = sample_start[u + 1] - sample_start[u];
    if (T < 0 || sample_start[u + 1] > MAX_T)
      return set_error(PWG_ERR_INVALID, "pwg_mel_run: sample_start must not decrease (or exceed 2^40)");
    if (T <= p->n_fft / 2)
      return set_error(PWG_ERR_INVALID, ("pwg_mel_run: utterance " + std::to_string(u) + " has " + std::to_string(T) +
                                         " samples; reflect padding needs more than n_fft / 2 = " +
                                         std::to_string(p->n_fft / 2)).c_str());
    rows += 1 + T / p->hop;
  }
  if (rows != out_rows)
    return set_error(PWG_ERR_INVALID, ("pwg_mel_run: out_rows is " + std::to_string(out_rows) + " but the utterances give " +
                                       std::to_string(rows) + " frames").c_str());

  int device = -1;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return hip_error("pwg_mel_run", e);
  if (device != p->device)
    return set_error(PWG_ERR_INVALID, ("pwg_mel_run: the plan lives on device " + std::to_string(p->device) +
                                       " but the current device is " + std::to_string(device)).c_str());
  MelArgs a;
  a.wave = wave; a.out = out; a.basis = p->d_basis; a.melfrag = p->d_melfrag; a.mask = p->d_mask; a.nyq = p->d_nyq;
  a.mean = p->d_mean; a.scale = p->d_scale;
  a.half = p->n_fft / 2; a.off = p->off; a.hop = p->hop; a.pad = p->pad; a.nk4 = p->nk4; a.n_bt = p->n_bt;
  a.num_mels = p->num_mels; a.span = p->span; a.log_kind = p->log_kind; a.amp_floor = p->amp_floor; a.eps = p->eps;
  e = pwg::allow_lds(kernel_of(p->mt), p->lds);
  if (e != hipSuccess) return hip_error("pwg_mel_run", e);
  long long row0 = 0;
  for (int u0 = 0; u0 < n_utts; u0 += MEL_CHUNK) {
    const int n = n_utts - u0 < MEL_CHUNK ? n_utts - u0 : MEL_CHUNK;
    long long max_tiles = 0;
    std::memset(a.utts, 0, sizeof(a.utts));
    for (int i = 0; i < n; ++i) {
      const long long T = sample_start[u0 + i + 1] - sample_start[u0 + i];
      const long long frames = 1 + T / p->hop;
      a.utts[i].s0 = sample_start[u0 + i];
      a.utts[i].T = T;
      a.utts[i].row0 = row0;
      row0 += frames;
      const long long tiles = (frames + MEL_TILE - 1) / MEL_TILE;
      if (tiles > max_tiles) max_tiles = tiles;
    }
    if (max_tiles > INT_MAX) return set_error(PWG_ERR_INVALID, "pwg_mel_run: too many frames for one launch");
    launch(p->mt, dim3((unsigned)max_tiles, (unsigned)n), p->lds, (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_error("pwg_mel_run", e);
  }
  return PWG_OK;
}
