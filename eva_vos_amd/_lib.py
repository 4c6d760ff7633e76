"""ctypes binding of libstcn_hip.so (C ABI declared in include/stcn_hip.h).

The HIP library is the product: there is no CPU / PyTorch fallback.  If the shared object is missing
the import fails loudly (build it with ``python -c 'import __graft_entry__ as g; g.build()'`` or
``make -C eva_vos_amd/csrc``)."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64; loading them
#               before libstcn_hip.so makes the process use ONE HIP runtime, whatever the import order)

_HERE = os.path.dirname(os.path.abspath(__file__))
# STCN_LIB: another build of the same library (measurement aid: tools/gpu_ab_trace.sh compares two builds on one GPU box)
LIB_PATH = os.environ.get("STCN_LIB") or os.path.join(_HERE, "libstcn_hip.so")

RESET_KEEP_FRAMES = 1          # STCN_RESET_KEEP_FRAMES (stcn_engine_reset_ex)
K_CLASSES = ("conv", "conv_reduce", "memread", "elementwise", "conv_n1", "other", "wino_input", "fusion_conv", "attention")


class WeightDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class EngineOpts(C.Structure):
    """stcn_engine_opts: a negative field = not given (environment variable / default)."""
    _fields_ = [(n, C.c_int32) for n in ("lookahead", "decode_batch", "key_batch", "fuse_side")]


# the int32 of an engine plan in the order of include/stcn_hip.h (STCN_ENGINE_PLAN_INTS of them); stcn_engine_get_plan appends bank_cap
ENGINE_PLAN_FIELDS = ("n_slots", "lookahead", "lookahead_req", "group", "key_batch", "fuse_side", "dual_sweep", "bank_lo", "bank_initial",
                      "main_key_batch", "main_group", "has_side", "side_key_batch", "side_group", "second_key_batch", "second_group")


class ModelOpts(C.Structure):
    """stcn_model_opts: a non-positive field = not given (top_k: 50; km: the plain read)."""
    _fields_ = [("top_k", C.c_int32), ("km", C.c_float)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("frames", "key_miss", "value_enc", "fused", "bank_fwd", "bank_bwd")]


# name -> (restype, argtypes); kept in one table so tests can check every declared symbol is exported
_P, _I, _L, _F, _D = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
PROTOTYPES = {
    "stcn_last_error": (C.c_char_p, []),
    "stcn_version": (C.c_char_p, []),
    "stcn_model_create": (_I, [_I, C.POINTER(WeightDesc), _I, C.POINTER(WeightDesc), _I, C.POINTER(_P)]),
    "stcn_model_create_ex": (_I, [_I, C.POINTER(WeightDesc), _I, C.POINTER(WeightDesc), _I, C.POINTER(ModelOpts), C.POINTER(_P)]),
    "stcn_model_get_top_k": (_I, [_P, C.POINTER(C.c_int32)]),
    "stcn_model_get_km": (_I, [_P, C.POINTER(C.c_float)]),
    "stcn_model_destroy": (_I, [_P]),
    "stcn_fusion_model_create": (_I, [_I, C.POINTER(WeightDesc), _I, C.POINTER(_P)]),
    "stcn_stage_create": (_I, [_P, _I, _I, _I, _P, C.POINTER(_P)]),
    "stcn_stage_destroy": (_I, [_P]),
    "stcn_stage_encode_key": (_I, [_P] * 7),
    "stcn_stage_encode_value": (_I, [_P, _P, _P, _P, _I, _P]),
    "stcn_stage_segment": (_I, [_P, _P, _L, _P, _L, _L, _I, _I, _P, _P, _P, _P, _P]),
    "stcn_stage_attention": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "stcn_stage_fusion": (_I, [_P, _P, _P, _P, _P, _F, _F, _P]),
    "stcn_aggregate_wbg": (_I, [_P, _P, _I, _L, _I, _I, _P]),
    "stcn_test_transpose": (_I, [_P, _P, _P, _I, _I, _I, _L, _L, _I]),
    "stcn_engine_create": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, C.POINTER(_P)]),
    "stcn_engine_create_ex": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, C.POINTER(EngineOpts), C.POINTER(_P)]),
    "stcn_engine_get_opts": (_I, [_P, C.POINTER(EngineOpts)]),
    "stcn_engine_get_plan": (_I, [_P, C.POINTER(C.c_int32), _I]),
    "stcn_test_engine_plan": (_I, [_I, _I, _I, _I, C.POINTER(EngineOpts), C.POINTER(C.c_int32), _I]),
    "stcn_engine_destroy": (_I, [_P]),
    "stcn_engine_reset": (_I, [_P]),
    "stcn_engine_reset_ex": (_I, [_P, C.c_uint32, C.POINTER(C.c_int32)]),
    "stcn_engine_clone": (_I, [_P, _P, _P, _P, C.POINTER(_P)]),
    "stcn_interact": (_I, [_P, _P, _I, _I, _I]),
    "stcn_engine_set_undo": (_I, [_P, _I]),
    "stcn_engine_undo": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stcn_engine_get_undo": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "stcn_get_stats": (_I, [_P, C.POINTER(Stats)]),
    "stcn_get_key_frames": (_I, [_P, C.POINTER(C.c_int64)]),
    "stcn_frame_gram_scratch": (_I, [_I, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "stcn_frame_sq_distances": (_I, [_P, _P, _I, C.c_int64, C.c_int64, _P, _P]),
    "stcn_engine_frame_distances": (_I, [_P, _P]),
    "stcn_engine_frame_features": (_I, [_P, _I, _P]),
    "stcn_get_flops": (_I, [_P, C.POINTER(_D)]),
    "stcn_last_conv_path": (C.c_char_p, []),
    "stcn_test_conv_trace": (_I, [_I]),
    "stcn_test_conv_trace_get": (C.c_char_p, []),
    "stcn_test_conv": (_I, [_P, _P, _P, _P, _P, _P] + [_I] * 11),
    "stcn_test_conv_ex": (_I, [_P, _P, _P, _P, _P, _P] + [_I] * 11 + [_P, _I, _L, _L, _L, _I, _L]),
    "stcn_test_conv_path": (_I, [_I] * 9 + [C.c_char_p, _I]),
    "stcn_test_conv_plan": (_I, [_I] * 9 + [C.POINTER(C.c_int32), _I, C.POINTER(_D)]),
    "stcn_test_sweep_plan": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int32), _I, C.POINTER(C.c_int32)]),
    "stcn_test_encode_key": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "stcn_test_encode_value": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "stcn_test_memory_read": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "stcn_test_memory_read_k": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "stcn_test_memory_read_km": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "stcn_bench_memory_read": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, C.POINTER(_F), C.POINTER(C.c_int32)]),
    "stcn_bench_memory_read_k": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, C.POINTER(_F), C.POINTER(C.c_int32)]),
    "stcn_bench_memory_read_km": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P, C.POINTER(_F), C.POINTER(C.c_int32)]),
    "stcn_memread_plan": (_I, [_I, _I, C.POINTER(C.c_int32)]),
    "stcn_attention_plan": (_I, [_I, C.POINTER(C.c_int32)]),
    "stcn_memread_scratch": (_I, [_I, C.POINTER(C.c_int64)]),
    "stcn_test_kernel": (_I, [C.c_char_p, _P, C.POINTER(_P), _I, C.POINTER(C.c_int64), _I, C.POINTER(_D), _I]),
    "stcn_test_fail_at": (_I, [_I]),
    "stcn_test_side_delay_us": (_I, [_I]),
    "stcn_test_decode": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "stcn_test_attention": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "stcn_test_attention_ex": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "stcn_test_fusion": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _I, _I, _P]),
    "stcn_metrics_jf_counts": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "stcn_metrics_j_counts": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "stcn_metrics_round": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P]),
    "stcn_metrics_trial": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P]),
    "stcn_metrics_objects_scratch": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int64)]),
    "stcn_metrics_objects_jf_counts": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "stcn_metrics_objects_j_counts": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "stcn_metrics_objects_round": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P, _P]),
    "stcn_metrics_round_typed": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P]),
    "stcn_robot_scratch": (_I, [_I, _I, C.POINTER(C.c_int64)]),
    "stcn_robot_click": (_I, [_P, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P]),
    "stcn_robot_bbox": (_I, [_P, _P, _I, _I, _P]),
    "stcn_robot_best_mask": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "stcn_masks_resize_nearest": (_I, [_P, _P, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "stcn_frames_to_rgb8": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "stcn_prob_upsample_argmax": (_I, [_P, _P] + [_I] * 12 + [_P]),
    "stcn_frames_downsample_aa": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "stcn_bench_conv": (_I, [_P] + [_I] * 11 + [C.POINTER(_F), C.POINTER(_D)]),
    "stcn_bench_mfma_rate": (_I, [_P, _I, C.POINTER(_F), C.POINTER(_F)]),
    "stcn_pool_release": (_I, []),
    "stcn_pool_stats": (_I, [C.POINTER(C.c_int64)] * 3),
    "stcn_engine_set_profiling": (_I, [_P, _I]),
    "stcn_get_kernel_ms": (_I, [_P, C.POINTER(_F), C.POINTER(C.c_int32)]),
    "stcn_get_kernel_flops": (_I, [_P, C.POINTER(_D)]),
    "stcn_get_kernel_bytes": (_I, [_P, C.POINTER(_D)]),
    "stcn_get_kernel_exec_flops": (_I, [_P, C.POINTER(_D)]),
    "stcn_get_conv_regimes": (_I, [_P, C.POINTER(_D)]),
}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP engine has not been built (run __graft_entry__.build() "
                "or `make -C eva_vos_amd/csrc`).  There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = res, args
    return _lib


def check(rc: int, what: str = "stcn") -> None:
    if rc != 0:
        msg = lib().stcn_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def src_hash() -> str:
    """The source hash the LOADED library was built from (csrc/Makefile: sha256 of the sorted *.hip / *.cpp / *.h of csrc + the C-ABI header +
    the extra flags, 12 hex digits) - captures under profiles/ are stamped with it, bench.py compares it with theirs."""
    import re
    m = re.search(r"src ([0-9a-f]{12})", lib().stcn_version().decode())
    return m.group(1) if m else "unknown"


def tree_hash(extra: str = "") -> str:
    """The same hash computed from the sources in the tree (what a fresh `make` would stamp): differs from src_hash() when the .so is stale."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(os.path.basename(f) for pat in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(csrc, pat)))
    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(csrc, f), "rb").read())
    h.update(open(os.path.join(_HERE, "..", "include", "stcn_hip.h"), "rb").read())
    h.update((extra + "\n").encode())
    return h.hexdigest()[:12]
