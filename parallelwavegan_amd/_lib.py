"""ctypes binding of the engine's C-ABI (include/pwg.h) and its in-tree build.

The shared library is built IN-TREE (parallelwavegan_amd/lib/libpwg_hip.so) by ``build()``
with hipcc for gfx950 so it travels with the repository snapshot. There is no fallback: if the
library is missing, ``load()`` raises, and so does every GPU entry point that needs it.

``torch`` must be imported before the library is loaded: torch ships its own
libamdhip64.so.7 and the dynamic loader then resolves our NEEDED entry to that same runtime
(one HIP runtime per process, so torch device pointers and streams are valid here).
"""

import ctypes
import os
import subprocess
import threading

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.environ.get("PWG_LIB_PATH") or os.path.join(LIB_DIR, "libpwg_hip.so")
CSRC = [
    os.path.join(PKG_DIR, "csrc", "pwg_kernels.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_capi.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_cnet.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_split.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_split16.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_rccl.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_mstack.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_rstack.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_embed.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_embed_ext.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_smg.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_uconv.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_vq.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_sine.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_mel.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_yin.hip"),
    os.path.join(PKG_DIR, "csrc", "pwg_wave.hip"),
]
HEADERS = [
    os.path.join(REPO_DIR, "include", "pwg.h"),
    os.path.join(REPO_DIR, "include", "pwg_cnet.h"),
    os.path.join(REPO_DIR, "include", "pwg_embed.h"),
    os.path.join(REPO_DIR, "include", "pwg_mel.h"),
    os.path.join(REPO_DIR, "include", "pwg_sine.h"),
    os.path.join(REPO_DIR, "include", "pwg_smg.h"),
    os.path.join(REPO_DIR, "include", "pwg_uhg.h"),
    os.path.join(REPO_DIR, "include", "pwg_vq.h"),
    os.path.join(REPO_DIR, "include", "pwg_wave.h"),
    os.path.join(REPO_DIR, "include", "pwg_yin.h"),
    os.path.join(PKG_DIR, "csrc", "pwg_internal.h"),
]
OFFLOAD_ARCH = "gfx950"

PWG_OK = 0
PWG_ERR_INVALID = 1
PWG_ERR_ASSERT = 2
PWG_ERR_HIP = 3
PWG_ERR_UNSUPPORTED = 4
PWG_ERR_RANGE = 5
PWG_ERR_RERUN = 6
PWG_RCCL_UNIQUE_ID_BYTES = 128

PWG_LAYOUT_INFERENCE = 0
PWG_LAYOUT_FORWARD = 1

KERNEL_BUCKETS = ("conv_in", "upsample", "first_conv", "residual_layer", "head")
PWG_MAX_SCALES = 8

# Every symbol include/*.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "pwg_abi_version",
    "pwg_last_error",
    "pwg_create",
    "pwg_destroy",
    "pwg_receptive_field_size",
    "pwg_upsample_factor",
    "pwg_ref_weight_count",
    "pwg_packed_weight_count",
    "pwg_pack_weights",
    "pwg_plan_create",
    "pwg_plan_destroy",
    "pwg_plan_total_samples",
    "pwg_plan_padded_samples",
    "pwg_plan_workspace_bytes",
    "pwg_run",
    "pwg_run_status",
    "pwg_graph_create",
    "pwg_graph_launch",
    "pwg_graph_destroy",
    "pwg_set_option",
    "pwg_get_option",
    "pwg_fragment_ahead_launches",
    "pwg_set_timing",
    "pwg_release_stream",
    "pwg_timing_collect",
    "pwg_timing_span",
    "pwg_rccl_unique_id",
    "pwg_rccl_comm_create",
    "pwg_rccl_comm_destroy",
    "pwg_broadcast_weights",
    # include/pwg_cnet.h: conv-network executor (MelGAN family)
    "pwg_cnet_abi_version",
    "pwg_cnet_create",
    "pwg_cnet_destroy",
    "pwg_cnet_packed_weight_count",
    "pwg_cnet_pack_weights",
    "pwg_cnet_plan_create",
    "pwg_cnet_plan_destroy",
    "pwg_cnet_plan_image",
    "pwg_cnet_plan_rows",
    "pwg_cnet_plan_workspace_bytes",
    "pwg_cnet_plan_buffer",
    "pwg_cnet_run",
    "pwg_cnet_set_external",
    "pwg_cnet_run_ext",
    "pwg_cnet_run_status",
    "pwg_cnet_plan_schedule",
    "pwg_cnet_set_option",
    "pwg_cnet_set_timing",
    "pwg_cnet_timing_collect",
    "pwg_cnet_timing_span",
    "pwg_cnet_release_stream",
    "pwg_rstack_debug_launches",
    "pwg_rstack_debug_probe",
    # include/pwg_embed.h: token front end of the discrete-symbol vocoders
    "pwg_embed_rows",
    # ... and of the duration- and f0-conditioned ones (csrc/pwg_embed_ext.hip)
    "pwg_durpred_layer",
    "pwg_regulate_scan",
    "pwg_regulate_rows",
    "pwg_embed_rows_f0",
    # include/pwg_uhg.h: UHiFiGAN's excitation front end (csrc/pwg_uconv.hip)
    "pwg_uhg_excite_rows",
    # include/pwg_sine.h: sine excitation from f0 (csrc/pwg_sine.hip)
    "pwg_sine_scratch_bytes",
    "pwg_sine_frames_scratch_bytes",
    "pwg_sine_samples",
    "pwg_sine_frames",
    # include/pwg_mel.h: log-mel feature extraction (csrc/pwg_mel.hip)
    "pwg_mel_frames",
    "pwg_mel_plan_create",
    "pwg_mel_plan_destroy",
    "pwg_mel_run",
    # include/pwg_yin.h: YIN f0 estimation (csrc/pwg_yin.hip)
    "pwg_yin_frames",
    "pwg_yin_plan_create",
    "pwg_yin_plan_destroy",
    "pwg_yin_run",
    # include/pwg_wave.h: silence trim, polyphase resampling, fit / gain / peak (csrc/pwg_wave.hip)
    "pwg_trim_frames",
    "pwg_trim_plan_create",
    "pwg_trim_plan_destroy",
    "pwg_trim_run",
    "pwg_resample_out_len",
    "pwg_resample_plan_create",
    "pwg_resample_plan_destroy",
    "pwg_resample_plan_tile",
    "pwg_resample_run",
    "pwg_wave_fit_run",
    # include/pwg_vq.h: VQVAE's encoder front end, grouped strided levels, code search and decoder rows
    # (csrc/pwg_vq.hip)
    "pwg_vq_wave_rows",
    "pwg_vq_gsconv_packed_count",
    "pwg_vq_gsconv_pack",
    "pwg_vq_gsconv",
    "pwg_vq_code_norms",
    "pwg_vq_nearest",
    "pwg_vq_decode_rows",
    # include/pwg_smg.h: StyleMelGAN generator path
    "pwg_smg_create",
    "pwg_smg_destroy",
    "pwg_smg_ref_weight_count",
    "pwg_smg_packed_weight_count",
    "pwg_smg_pack_weights",
    "pwg_smg_plan_create",
    "pwg_smg_plan_create_ex",
    "pwg_smg_plan_destroy",
    "pwg_smg_plan_workspace_bytes",
    "pwg_smg_plan_out_rows",
    "pwg_smg_run",
    "pwg_smg_run_tokens",
    "pwg_smg_run_status",
    "pwg_smg_plan_tensor",
    "pwg_smg_debug_stats",
    "pwg_smg_set_timing",
    "pwg_smg_timing_collect",
)

PWG_OPT_LAYER_KERNEL = 0
PWG_OPT_WAVES_PER_WG = 1
PWG_OPT_WG_PER_CU = 2
PWG_OPT_FUSE_FIRST_CONV = 3
PWG_OPT_PIPELINE = 4
PWG_OPT_HALF_BLOCKS = 5
PWG_OPT_SYNC = 6
PWG_OPT_SYNC_ABORT = 7
PWG_OPT_SYNC_TIMEOUT = 8
PWG_OPT_FRAGMENT_AHEAD = 9
PWG_OPT_SKIP_AHEAD = 10


PWG_VQ_BAD_CODE, PWG_VQ_BAD_GLOBAL, PWG_VQ_BAD_INPUT = 1, 2, 4

PWG_SINE_BAD_F0 = 1
PWG_SINE_LAYOUTS = {"tile": 0, "hold": 1}
PWG_SINE_MAX_DIM = 8
PWG_SINE_SCAN_BLOCK = 1024

PWG_MEL_FRAME_TILE = 64
PWG_MEL_MAX_MELS = 128
PWG_MEL_WINDOW_HANN = 0

PWG_YIN_FRAME_TILE = 8
PWG_YIN_MAX_TAU = 1680

PWG_TRIM_PAD_MODES = {"constant": 0, "reflect": 1}
PWG_TRIM_FRAME_TILE = 16
PWG_TRIM_MAX_TILE_SPAN = 36864
PWG_RESAMPLE_MAX_RATE = 640
PWG_RESAMPLE_MAX_TAPS = 20 * 640 + 1
PWG_RESAMPLE_OUT_TILE = 1024

PWG_SMG_MAX_SCALES = 16
PWG_SMG_STATS_TILE = 128
PWG_SMG_GATES = {"softmax": 0, "sigmoid": 1}
PWG_SMG_X_IN, PWG_SMG_X_OUT, PWG_SMG_STATS_IN, PWG_SMG_STATS_MID = range(4)
PWG_SMG_PLAN_TRIM_NOISE = 1
PWG_SMG_KINDS = ("noise", "stats", "aux_conv", "modulate_conv", "gate_conv", "finalise", "output")


class PwgSmgConfig(ctypes.Structure):
    _fields_ = [
        ("in_channels", ctypes.c_int),
        ("aux_channels", ctypes.c_int),
        ("channels", ctypes.c_int),
        ("out_channels", ctypes.c_int),
        ("kernel_size", ctypes.c_int),
        ("dilation", ctypes.c_int),
        ("bias", ctypes.c_int),
        ("gate", ctypes.c_int),
        ("noise_slope", ctypes.c_float),
        ("num_noise_scales", ctypes.c_int),
        ("noise_scales", ctypes.c_int * PWG_SMG_MAX_SCALES),
        ("num_scales", ctypes.c_int),
        ("upsample_scales", ctypes.c_int * PWG_SMG_MAX_SCALES),
    ]


class PwgConfig(ctypes.Structure):
    _fields_ = [
        ("in_channels", ctypes.c_int),
        ("out_channels", ctypes.c_int),
        ("kernel_size", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("stacks", ctypes.c_int),
        ("residual_channels", ctypes.c_int),
        ("gate_channels", ctypes.c_int),
        ("skip_channels", ctypes.c_int),
        ("aux_channels", ctypes.c_int),
        ("aux_context_window", ctypes.c_int),
        ("use_causal_conv", ctypes.c_int),
        ("use_conv_in", ctypes.c_int),
        ("num_scales", ctypes.c_int),
        ("upsample_scales", ctypes.c_int * PWG_MAX_SCALES),
        ("interpolate_mode", ctypes.c_int),
    ]


def _needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in CSRC + HEADERS)


def _compile_cmd(hipcc, extra_flags):
    return [
        hipcc,
        f"--offload-arch={OFFLOAD_ARCH}",
        "-O3",
        "-std=c++17",
        "-fPIC",
        "-fvisibility=hidden",
        "-mcode-object-version=5",
        # keep the work-queue atomic a plain per-lane op: the optimizer's wave-reduction form
        # waits for the returned value right after issue, which defeats the claim-ahead
        "-mllvm",
        "-amdgpu-atomic-optimizer-strategy=None",
        "-Wall",
    ] + list(extra_flags)


def build(force=False, verbose=False, extra_flags=(), out_path=None, jobs=None, link_flags=()):
    """Compile the HIP kernels + C-ABI into parallelwavegan_amd/lib/libpwg_hip.so (gfx950): one
    hipcc -c per source in parallel (objects under build/<variant>/, rebuilt when a source or
    header is newer), then one link. extra_flags/out_path build A/B measurement variants (e.g.
    -DPWG_STORE_SC1=0) elsewhere."""
    from concurrent.futures import ThreadPoolExecutor

    target = out_path or LIB_PATH
    if not force and out_path is None and (os.environ.get("PWG_NO_BUILD") == "1" or not _needs_build()):
        return LIB_PATH
    os.makedirs(os.path.dirname(target), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    variant = os.path.splitext(os.path.basename(target))[0]
    objdir = os.path.join(REPO_DIR, "build", variant)
    os.makedirs(objdir, exist_ok=True)
    base = _compile_cmd(hipcc, extra_flags)
    stamp = os.path.join(objdir, "flags.txt")
    flags_txt = " ".join(base)
    stale_flags = not os.path.exists(stamp) or open(stamp).read() != flags_txt
    newest_header = max(os.path.getmtime(h) for h in HEADERS)

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if (not force and not stale_flags and os.path.exists(obj)
                and os.path.getmtime(obj) >= max(os.path.getmtime(src), newest_header)):
            return obj, ""
        tmp = obj + ".tmp.%d" % os.getpid()
        cmd = base + ["-c", "-o", tmp, src]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
        os.replace(tmp, obj)
        return obj, res.stdout + res.stderr

    n = jobs or min(len(CSRC), max(1, int(os.environ.get("MAX_JOBS", os.cpu_count() or 1))))
    with ThreadPoolExecutor(max_workers=n) as ex:
        results = list(ex.map(compile_one, CSRC))
    with open(stamp, "w") as f:
        f.write(flags_txt)
    tmp = target + ".tmp.%d" % os.getpid()
    cmd = ([hipcc, f"--offload-arch={OFFLOAD_ARCH}", "-shared", "-fPIC", "-o", tmp] + [o for o, _ in results]
           + list(link_flags) + ["-ldl"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    if verbose:
        for _, log in results:
            if log:
                print(log)
    os.replace(tmp, target)
    return target


# Host-side sanitizer build: the C-ABI's host code (config checks, weight
# packing, PWG and conv-network plan builders) under AddressSanitizer + UndefinedBehaviorSanitizer,
# with every uninitialised automatic variable filled with a 0xAA pattern (a field that is never
# assigned then holds a large, deterministic garbage value instead of whatever the stack held,
# which is how an uninitialised OpPhase field once produced a garbage block list and a GPU fault).
# Device code is built unoptimised (-O0: 1 min instead of 3; it never runs) and unsanitised (each
# -fsanitize= only after -Xarch_host): this library is for the host-only tests in this container
# (tests/test_host_sanitized.py), never for a GPU run.
SANITIZE_FLAGS = ["-O1", "-g", "-Xarch_device", "-O0"] + [f for x in ("-fsanitize=address", "-fsanitize=undefined", "-fno-omit-frame-pointer",
                                               "-ftrivial-auto-var-init=pattern") for f in ("-Xarch_host", x)]
SANITIZE_LINK = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-shared-libsan"]
SANITIZED_LIB_PATH = os.path.join(REPO_DIR, "build", "sanitized", "libpwg_hip_asan.so")


SANITIZED_SOURCES = ("pwg_capi.hip", "pwg_cnet.hip")  # the host plan builders; the others are launchers


def build_host_sanitized(force=False):
    """Build SANITIZED_LIB_PATH: pwg_capi.hip and pwg_cnet.hip (config checks, packing, plan
    builders) compiled with SANITIZE_FLAGS, linked with the product build's objects of the other
    sources (kernels and their launchers; build() first). Returns the library path."""
    from concurrent.futures import ThreadPoolExecutor

    build()
    objdir = os.path.dirname(SANITIZED_LIB_PATH)
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = _compile_cmd(hipcc, SANITIZE_FLAGS)
    newest = max(os.path.getmtime(f) for f in CSRC + HEADERS)
    if not force and os.path.exists(SANITIZED_LIB_PATH) and os.path.getmtime(SANITIZED_LIB_PATH) >= newest:
        return SANITIZED_LIB_PATH

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        res = subprocess.run(base + ["-c", "-o", obj, src], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc (sanitized) failed:\n" + res.stdout + res.stderr)
        return obj

    srcs = [c for c in CSRC if os.path.basename(c) in SANITIZED_SOURCES]
    with ThreadPoolExecutor(max_workers=len(srcs)) as ex:
        objs = list(ex.map(compile_one, srcs))
    product = os.path.join(REPO_DIR, "build", os.path.splitext(os.path.basename(LIB_PATH))[0])
    objs += [os.path.join(product, os.path.basename(c) + ".o") for c in CSRC if os.path.basename(c) not in SANITIZED_SOURCES]
    cmd = ([hipcc, f"--offload-arch={OFFLOAD_ARCH}", "-shared", "-fPIC", "-o", SANITIZED_LIB_PATH] + objs
           + SANITIZE_LINK + ["-ldl"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link (sanitized) failed:\n" + res.stdout + res.stderr)
    return SANITIZED_LIB_PATH


def sanitizer_runtime():
    """The ASan runtime to LD_PRELOAD into an uninstrumented python (None if absent)."""
    import glob

    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    return hits[-1] if hits else None


_lib = None
_lock = threading.Lock()


def load():
    """Load the built library (raises if it is missing: no CPU fallback exists)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            )
        import torch  # noqa: F401  (bind our NEEDED libamdhip64.so.7 to torch's HIP runtime)

        lib = ctypes.CDLL(LIB_PATH)
        vp = ctypes.c_void_p
        ll = ctypes.c_longlong
        lib.pwg_abi_version.restype = ctypes.c_int
        lib.pwg_last_error.restype = ctypes.c_char_p
        lib.pwg_create.argtypes = [ctypes.POINTER(PwgConfig), ctypes.c_int, ctypes.POINTER(vp)]
        lib.pwg_destroy.argtypes = [vp]
        lib.pwg_destroy.restype = None
        for name in ("pwg_receptive_field_size", "pwg_upsample_factor", "pwg_ref_weight_count",
                     "pwg_packed_weight_count"):
            getattr(lib, name).argtypes = [vp]
            getattr(lib, name).restype = ll
        lib.pwg_pack_weights.argtypes = [vp, vp, vp]
        lib.pwg_plan_create.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ll), ctypes.c_int, ctypes.POINTER(vp)]
        lib.pwg_plan_destroy.argtypes = [vp]
        lib.pwg_plan_destroy.restype = None
        for name in ("pwg_plan_total_samples", "pwg_plan_padded_samples", "pwg_plan_workspace_bytes"):
            getattr(lib, name).argtypes = [vp]
            getattr(lib, name).restype = ll
        lib.pwg_run.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pwg_run_status.argtypes = [vp, vp, vp]
        lib.pwg_graph_create.argtypes = [vp] * 9 + [ctypes.POINTER(vp)]
        lib.pwg_graph_launch.argtypes = [vp, vp]
        lib.pwg_graph_destroy.argtypes = [vp]
        lib.pwg_graph_destroy.restype = None
        lib.pwg_get_option.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ll)]
        lib.pwg_fragment_ahead_launches.argtypes = [vp, ctypes.POINTER(ll)]
        lib.pwg_rccl_unique_id.argtypes = [vp]
        lib.pwg_rccl_comm_create.argtypes = [ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        lib.pwg_rccl_comm_destroy.argtypes = [vp]
        lib.pwg_broadcast_weights.argtypes = [vp, vp, ctypes.c_int, vp, vp]
        lib.pwg_set_timing.argtypes = [vp, ctypes.c_int]
        lib.pwg_release_stream.argtypes = [vp, vp]
        lib.pwg_set_option.argtypes = [vp, ctypes.c_int, ctypes.c_longlong]
        lib.pwg_timing_collect.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ll)]
        lib.pwg_timing_span.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        lib.pwg_embed_rows.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int, ll,
                                       vp, vp, vp]
        ci = ctypes.c_int
        lib.pwg_durpred_layer.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, ctypes.c_float, vp, ci, ll,
                                          vp, vp, vp, vp, vp]
        lib.pwg_regulate_scan.argtypes = [vp, vp, ci, ll, vp, vp, vp, vp]
        lib.pwg_regulate_rows.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, ll, ll, vp, vp, vp]
        lib.pwg_embed_rows_f0.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, ll, vp, vp, vp]
        lib.pwg_uhg_excite_rows.argtypes = [vp, vp, vp, ci, ci, ctypes.c_float, vp, ci, ll, vp, vp]
        cf = ctypes.c_float
        lib.pwg_sine_scratch_bytes.argtypes = [ll, ci]
        lib.pwg_sine_scratch_bytes.restype = ll
        lib.pwg_sine_frames_scratch_bytes.argtypes = [ll, ci]
        lib.pwg_sine_frames_scratch_bytes.restype = ll
        lib.pwg_sine_samples.argtypes = [vp, vp, ci, ll, cf, ci, cf, cf, cf, vp, vp, vp, vp, vp, vp, ll, vp, vp]
        lib.pwg_sine_frames.argtypes = [vp, vp, ci, ll, ci, ci, cf, ci, cf, cf, cf, vp, vp, vp, vp, vp, vp, ll, vp, vp]
        lib.pwg_mel_frames.argtypes = [ll, ci]
        lib.pwg_mel_frames.restype = ll
        lib.pwg_mel_plan_create.argtypes = [ci, ci, ci, ci, ci, vp, ll, cf, cf, ci, vp, vp, ctypes.POINTER(vp)]
        lib.pwg_mel_plan_destroy.argtypes = [vp]
        lib.pwg_mel_plan_destroy.restype = None
        lib.pwg_mel_run.argtypes = [vp, vp, ctypes.POINTER(ll), ci, vp, ll, vp]
        lib.pwg_yin_frames.argtypes = [ll, ci, ci]
        lib.pwg_yin_frames.restype = ll
        lib.pwg_yin_plan_create.argtypes = [cf, ci, ci, ci, cf, ci, ctypes.POINTER(vp)]
        lib.pwg_yin_plan_destroy.argtypes = [vp]
        lib.pwg_yin_plan_destroy.restype = None
        lib.pwg_yin_run.argtypes = [vp, vp, ctypes.POINTER(ll), ci, ctypes.POINTER(ll), vp, vp, vp, ll, vp]
        lib.pwg_trim_frames.argtypes = [ll, ci, ci]
        lib.pwg_trim_frames.restype = ll
        lib.pwg_trim_plan_create.argtypes = [ci, ci, cf, ci, ctypes.POINTER(vp)]
        lib.pwg_trim_plan_destroy.argtypes = [vp]
        lib.pwg_trim_plan_destroy.restype = None
        lib.pwg_trim_run.argtypes = [vp, vp, ctypes.POINTER(ll), ci, vp, vp, ll, vp]
        lib.pwg_resample_out_len.argtypes = [ll, ci, ci]
        lib.pwg_resample_out_len.restype = ll
        lib.pwg_resample_plan_create.argtypes = [ci, ci, vp, ci, ctypes.POINTER(vp)]
        lib.pwg_resample_plan_destroy.argtypes = [vp]
        lib.pwg_resample_plan_destroy.restype = None
        lib.pwg_resample_plan_tile.argtypes = [vp]
        lib.pwg_resample_run.argtypes = [vp, vp, ctypes.POINTER(ll), ci, vp, ll, vp]
        lib.pwg_wave_fit_run.argtypes = [vp, ctypes.POINTER(ll), ctypes.POINTER(ll), vp, ctypes.POINTER(ll), ci, cf, vp, vp]
        lib.pwg_vq_wave_rows.argtypes = [vp, vp, vp, ci, ci, cf, vp, vp, ci, ll, vp, vp]
        lib.pwg_vq_gsconv_packed_count.argtypes = [ci, ci, ci]
        lib.pwg_vq_gsconv_packed_count.restype = ll
        lib.pwg_vq_gsconv_pack.argtypes = [vp, ci, ci, ci, vp]
        lib.pwg_vq_gsconv.argtypes = [vp, vp, ll, ci, vp, vp, ci, ci, cf, vp, vp, ll, ci, vp]
        lib.pwg_vq_code_norms.argtypes = [vp, ci, ci, vp, vp]
        lib.pwg_vq_nearest.argtypes = [vp, ll, ci, vp, vp, ci, vp, vp, vp, vp]
        lib.pwg_vq_decode_rows.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, ci, vp, ci, ci, vp, vp, ci, ll, vp, vp, vp]
        lib.pwg_smg_create.argtypes = [ctypes.POINTER(PwgSmgConfig), ctypes.c_int, ctypes.POINTER(vp)]
        lib.pwg_smg_destroy.argtypes = [vp]
        lib.pwg_smg_destroy.restype = None
        lib.pwg_smg_plan_destroy.argtypes = [vp]
        lib.pwg_smg_plan_destroy.restype = None
        for name in ("pwg_smg_ref_weight_count", "pwg_smg_packed_weight_count", "pwg_smg_plan_workspace_bytes",
                     "pwg_smg_plan_out_rows"):
            getattr(lib, name).argtypes = [vp]
            getattr(lib, name).restype = ll
        lib.pwg_smg_pack_weights.argtypes = [vp, vp, vp]
        lib.pwg_smg_plan_create.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.POINTER(vp)]
        lib.pwg_smg_plan_create_ex.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.c_int,
                                               ctypes.POINTER(vp)]
        lib.pwg_smg_run.argtypes = [vp] * 9
        lib.pwg_smg_run_tokens.argtypes = [vp, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        lib.pwg_smg_run_status.argtypes = [vp, vp, vp]
        lib.pwg_smg_plan_tensor.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ll), ctypes.POINTER(ll),
                                            ctypes.POINTER(ctypes.c_int)]
        lib.pwg_smg_debug_stats.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ll), ctypes.c_int, vp, vp, vp, vp]
        lib.pwg_smg_set_timing.argtypes = [vp, ctypes.c_int]
        lib.pwg_smg_timing_collect.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        if lib.pwg_abi_version() != 2:
            raise RuntimeError("libpwg_hip ABI version mismatch")
        _lib = lib
        return lib


class RangeError(ArithmeticError):
    """PWG_ERR_RANGE: a value left the fp16 pair range of the split-f16 kernels."""


class RerunError(RuntimeError):
    """PWG_ERR_RERUN: a grid-synchronised or layer-pipelined forward did not complete (the GPU was
    shared, or a bounded wait gave up); its output is invalid and the run must be redone on the
    per-layer launches."""


_ERRORS = {
    PWG_ERR_RANGE: RangeError,
    PWG_ERR_RERUN: RerunError,
    PWG_ERR_INVALID: ValueError,
    PWG_ERR_ASSERT: AssertionError,
    PWG_ERR_HIP: RuntimeError,
    PWG_ERR_UNSUPPORTED: NotImplementedError,
}


def check(rc):
    """Raise the reference's exception type for a non-zero status (include/pwg.h)."""
    if rc == PWG_OK:
        return
    msg = load().pwg_last_error().decode(errors="replace")
    raise _ERRORS.get(rc, RuntimeError)(msg)
