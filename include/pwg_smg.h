/*
 * pwg_smg.h — C-ABI of the StyleMelGAN generator path
 * (StyleMelGANGenerator, parallel_wavegan/models/style_melgan.py:18-240; TADEResBlock,
 * parallel_wavegan/layers/tade_res_block.py).
 *
 * The network does not fit the conv-network executor (pwg_cnet.h): every TADE layer normalises its
 * input over the utterance's whole time axis (InstanceNorm1d), the aux path is upsampled by
 * nearest-neighbour repetition, and a block's outputs are softmax-over-channels(xa) * tanh(xb).
 * It runs on kernels of its own (parallelwavegan_amd/csrc/pwg_smg.hip).
 *
 * Conventions as in pwg_cnet.h: int status codes (pwg.h; pwg_last_error() gives the message), an
 * opaque stream (hipStream_t), host-only plan creation, a caller-owned workspace, and no allocation
 * or host synchronisation in pwg_smg_run. All tensors are time-major: (rows, channels) packed fp32.
 */
#ifndef PWG_SMG_H_
#define PWG_SMG_H_

#include "pwg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWG_SMG_MAX_SCALES 16
/* rows per tile of the stand-alone statistics pass (pwg_smg_debug_stats, the noise stage) */
#define PWG_SMG_STATS_TILE 128

enum { PWG_SMG_GATE_SOFTMAX = 0, PWG_SMG_GATE_SIGMOID = 1 };

/* which tensor of a block pwg_smg_plan_tensor locates */
enum {
  PWG_SMG_BLOCK_X_IN = 0,     /* the block's input x: rows x channels */
  PWG_SMG_BLOCK_X_OUT = 1,    /* its output x: rows * scale x channels */
  PWG_SMG_BLOCK_STATS_IN = 2, /* (mean, rstd) of x_in: n_utts x channels x 2 */
  PWG_SMG_BLOCK_STATS_MID = 3 /* (mean, rstd) of the first gate's output x1: n_utts x channels x 2 */
};

/* kernel kinds of the per-launch timing (pwg_smg_timing_collect) */
enum {
  PWG_SMG_KIND_NOISE = 0,
  PWG_SMG_KIND_STATS = 1,
  PWG_SMG_KIND_AUX_CONV = 2,
  PWG_SMG_KIND_MODULATE_CONV = 3,
  PWG_SMG_KIND_GATE_CONV = 4,
  PWG_SMG_KIND_FINALISE = 5,
  PWG_SMG_KIND_OUTPUT = 6,
  PWG_SMG_KINDS = 7
};

/* pwg_smg_plan_create_ex flags */
enum {
  /* The layout of DiscreteSymbolStyleMelGANGenerator.inference (style_melgan.py:588-600): the upsampled
   * noise is cut to the utterance's frames (x = noise_up[:, :, :T]) instead of the aux frames being
   * padded up to it, so every tensor has exactly frames[u] rows per utterance at rate 1 and every
   * instance-norm statistic is taken over them. */
  PWG_SMG_PLAN_TRIM_NOISE = 1
};

/* Bits of the run's flag word (pwg_smg_run_status): a non-finite sample from the output kernel, and the
 * PWG_EMBED_BAD_* bits of pwg_embed.h shifted left by PWG_SMG_FLAG_EMBED_SHIFT from the token staging. */
enum { PWG_SMG_FLAG_NONFINITE = 1, PWG_SMG_FLAG_EMBED_SHIFT = 8 };

typedef struct PwgSmgConfig {
  int in_channels;  /* noise channels */
  int aux_channels; /* multiple of 16, <= 128 */
  int channels;     /* multiple of 16, <= 64 */
  int out_channels;
  int kernel_size; /* odd, <= 11 */
  int dilation;    /* of each block's second gated conv */
  int bias;        /* 0: the convs have no bias (and the reference order holds none) */
  int gate;        /* PWG_SMG_GATE_* */
  float noise_slope; /* LeakyReLU slope of the noise upsampling */
  int num_noise_scales;
  int noise_scales[PWG_SMG_MAX_SCALES];
  int num_scales;
  int upsample_scales[PWG_SMG_MAX_SCALES];
} PwgSmgConfig;

typedef struct PwgSmg PwgSmg;
typedef struct PwgSmgPlan PwgSmgPlan;

/* device >= 0: the device the handle runs on; the caller makes it current (hipSetDevice) around
 * pwg_smg_run, which returns PWG_ERR_INVALID when another device is current. device -1: a host-only
 * handle (counts, packing and plans work, pwg_smg_run is refused). PWG_ERR_UNSUPPORTED for a shape
 * outside the kernels. */
PWG_API int pwg_smg_create(const PwgSmgConfig* cfg, int device, PwgSmg** out);
PWG_API void pwg_smg_destroy(PwgSmg* g);

/* Reference order = state-dict order with weight norm folded: per conv `weight` then (bias != 0)
 * `bias`; convs in module order noise_upsample.{0,2,..}, blocks.i.{tade1.aux_conv.0,
 * tade1.gated_conv.0, gated_conv1, tade2.aux_conv.0, tade2.gated_conv.0, gated_conv2},
 * output_conv.0; each tensor in torch's own element order. */
PWG_API long long pwg_smg_ref_weight_count(const PwgSmg* g);
PWG_API long long pwg_smg_packed_weight_count(const PwgSmg* g);
/* Both host pointers. PWG_ERR_RANGE if a conv weight does not fit an fp16 hi+lo pair
 * (|w| >= 65520 or not finite). */
PWG_API int pwg_smg_pack_weights(const PwgSmg* g, const float* ref_host, float* packed_host);

/* frames[u] >= 1 aux frames and noise_len[u] noise columns per utterance;
 * noise_len[u] * noise_factor >= frames[u] is required (the aux frames are replicate-padded up to
 * it, style_melgan.py:230-231). */
PWG_API int pwg_smg_plan_create(const PwgSmg* g, int n_utts, const long long* frames, const long long* noise_len,
                                PwgSmgPlan** out);
/* flags = 0: exactly pwg_smg_plan_create. PWG_SMG_PLAN_TRIM_NOISE: utterance u owns frames[u] rows at
 * rate 1 (row prefix(frames)[u] * rate of every tensor); frames[u] >= 2 is required (InstanceNorm1d over
 * one row raises in the reference) and noise_len[u] * noise_factor >= frames[u] still holds: the last
 * noise layer keeps its first frames[u] rows. Unknown flags are PWG_ERR_INVALID. pwg_smg_plan_tensor and
 * pwg_smg_plan_out_rows report the trimmed layout. */
PWG_API int pwg_smg_plan_create_ex(const PwgSmg* g, int n_utts, const long long* frames, const long long* noise_len,
                                   int flags, PwgSmgPlan** out);
PWG_API void pwg_smg_plan_destroy(PwgSmgPlan* p);
PWG_API long long pwg_smg_plan_workspace_bytes(const PwgSmgPlan* p);
/* output rows of the whole batch: sum of frames[u] * prod(upsample_scales) */
PWG_API long long pwg_smg_plan_out_rows(const PwgSmgPlan* p);

/* All device pointers. c: the utterances' aux frames back to back, (sum frames) x aux_channels;
 * mean, scale: aux_channels each or both NULL ((c - mean) / scale is applied on read);
 * z: per utterance (noise_len, in_channels), rows back to back; out: pwg_smg_plan_out_rows x
 * out_channels; workspace: pwg_smg_plan_workspace_bytes, 256-byte aligned.
 * Launches only: the plan's utterance table travels as kernel arguments (64 utterances per launch of
 * a one-workgroup kernel, which also zeroes the run's flag), so the call makes no host-to-device copy,
 * allocates nothing and does not synchronise (with timing off, below). */
PWG_API int pwg_smg_run(const PwgSmgPlan* p, const float* packed, const float* c, const float* mean,
                        const float* scale, const float* z, float* out, void* workspace, void* stream);
/* The token form (DiscreteSymbolStyleMelGANGenerator, style_melgan.py:364-602) on a plan made with
 * PWG_SMG_PLAN_TRIM_NOISE: the aux input is c[r] = emb[ids[r]] + spk[spk_ids[u(r)]], gathered where the first
 * aux conv stages its input (one fp32 add per element, as pwg_embed_rows; no (rows, aux_channels) buffer and
 * no launch of its own). All device pointers. emb: num_embs x aux_channels, spk: num_spk x aux_channels,
 * packed fp32, 16-byte aligned; ids: int64, the utterances' token ids back to back (sum frames); spk_ids:
 * int64, one per utterance; the rest as pwg_smg_run. Every id is checked before an address is formed from
 * it: a token id outside [0, num_embs) is staged as a zero row and sets PWG_EMBED_BAD_TOKEN <<
 * PWG_SMG_FLAG_EMBED_SHIFT in the run's flag; a speaker id outside [0, num_spk) contributes zero and sets
 * PWG_EMBED_BAD_SPEAKER << PWG_SMG_FLAG_EMBED_SHIFT. Launches only, as pwg_smg_run. The argument checks
 * (PWG_ERR_INVALID: null pointers, alignment, a plan without PWG_SMG_PLAN_TRIM_NOISE, a host-only handle,
 * another current device) come before any launch. */
PWG_API int pwg_smg_run_tokens(const PwgSmgPlan* p, const float* packed, const float* emb, int num_embs,
                               const float* spk, int num_spk, const long long* ids, const long long* spk_ids,
                               const float* z, float* out, void* workspace, void* stream);
/* Synchronises the stream and reads the run's flag: PWG_ERR_RANGE if a non-finite sample was stored
 * (a value left the fp16 pair range upstream, or the input was not finite), or, after pwg_smg_run_tokens, if
 * an id was out of range (the message starts with "bad token id" or "bad speaker id"; ids are reported
 * first). */
PWG_API int pwg_smg_run_status(const PwgSmgPlan* p, void* workspace, void* stream);

/* Where a block's tensors lie in the workspace after pwg_smg_run (tests compare block by block).
 * rows counts the whole batch (utterance u starts at row prefix(noise_len * noise_factor)[u] * rate, or
 * prefix(frames)[u] * rate in a trimmed plan);
 * for the statistics tables rows = n_utts and ld = 2 * channels. */
PWG_API int pwg_smg_plan_tensor(const PwgSmgPlan* p, int block, int which, long long* offset_bytes,
                                long long* rows, int* ld);

/* The partial-statistics and finalise kernels on a caller's buffer: x holds the utterances' rows back
 * to back (row stride ld floats, channels <= min(ld, 1024)); mean_out, rstd_out: n_utts x channels.
 * workspace: (16 * n_utts + 2 * channels * (sum(rows) / PWG_SMG_STATS_TILE + n_utts + 1)) * 4 + 512
 * bytes, device. rows_per_utt is a host array, read before the call returns. Launches on the current
 * device. */
PWG_API int pwg_smg_debug_stats(const float* x, int ld, int channels, const long long* rows_per_utt, int n_utts,
                                float* mean_out, float* rstd_out, void* workspace, void* stream);

/* on != 0: pwg_smg_run brackets every launch with HIP events. For measurement passes only: such a run
 * allocates (two events per launch, kept on the handle until collected) and is not thread-safe: the
 * runs of one handle's plans, and pwg_smg_timing_collect, must then come from one thread at a time.
 * pwg_smg_timing_collect synchronises the events and adds each launch's milliseconds to
 * ms[PWG_SMG_KINDS], then destroys them. */
PWG_API int pwg_smg_set_timing(PwgSmg* g, int on);
PWG_API int pwg_smg_timing_collect(PwgSmg* g, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* PWG_SMG_H_ */
