"""CPU: the stage API (the reference's PropagationNetwork.encode_key / encode_value / segment_with_query / get_attention, FusionNet.forward,
aggregate_wbg) - its C exports, the argument checks that run before any device call, and the Python entry points without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from eva_vos_amd import _lib
from eva_vos_amd.params import FusionNet, PropagationNetwork

STAGE_SYMBOLS = ["stcn_stage_create", "stcn_stage_destroy", "stcn_stage_encode_key", "stcn_stage_encode_value", "stcn_stage_segment",
                 "stcn_stage_attention", "stcn_stage_fusion", "stcn_aggregate_wbg", "stcn_fusion_model_create"]
E_INVALID = -1


def err():
    return _lib.lib().stcn_last_error().decode()


def test_every_stage_symbol_is_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "stcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for n in STAGE_SYMBOLS + ["stcn_test_transpose"]:
        assert re.search(r"\b" + n + r"\s*\(", src), f"include/stcn_hip.h does not declare {n}"
        assert n in _lib.PROTOTYPES, f"the ctypes table lacks {n}"
        assert hasattr(lib, n), f"libstcn_hip.so lacks {n}"


def test_invalid_arguments_are_refused_before_any_device_call():
    """Each refusal names what it refused, so a NULL context cannot stand in for the check under test."""
    lib = _lib.lib()
    h = C.c_void_p()
    one = C.c_void_p(16)                 # a non-null pointer that is never followed: every call below fails its checks first
    assert lib.stcn_stage_create(None, 128, 160, 1, None, C.byref(h)) == E_INVALID and "null" in err()
    assert lib.stcn_stage_create(None, 100, 160, 1, None, C.byref(h)) == E_INVALID and "nh=100" in err()
    assert lib.stcn_stage_create(None, 128, 150, 1, None, C.byref(h)) == E_INVALID and "nw=150" in err()
    assert lib.stcn_stage_create(None, 128, 160, 0, None, C.byref(h)) == E_INVALID and "max_objects=0" in err()
    assert lib.stcn_stage_create(None, 128, 160, 33, None, C.byref(h)) == E_INVALID and "max_objects=33" in err()
    assert h.value is None
    assert lib.stcn_stage_destroy(None) == 0
    for k in (0, 33):
        assert lib.stcn_stage_encode_value(None, one, one, one, k, one) == E_INVALID and f"k={k}" in err()
        assert lib.stcn_stage_segment(None, one, 80, one, 80, 0, 1, k, one, one, one, one, one) == E_INVALID and f"k={k}" in err()
        assert lib.stcn_aggregate_wbg(None, one, k, 100, 1, 0, one) == E_INVALID and f"k={k}" in err()
    assert lib.stcn_stage_segment(None, one, 80, one, 80, 0, 0, 1, one, one, one, one, one) == E_INVALID and "T=0" in err()
    for b in (0, 34):
        assert lib.stcn_stage_attention(None, one, one, one, one, b, one) == E_INVALID and f"b={b}" in err()
    # null contexts and null tensors
    assert lib.stcn_stage_encode_key(None, one, one, one, one, one, one) == E_INVALID and "null" in err()
    assert lib.stcn_stage_encode_value(None, one, one, one, 1, one) == E_INVALID and "null" in err()
    assert lib.stcn_stage_segment(None, one, 80, one, 80, 0, 1, 1, one, one, one, one, one) == E_INVALID and "null" in err()
    assert lib.stcn_stage_attention(None, one, one, one, one, 2, one) == E_INVALID and "null" in err()
    assert lib.stcn_stage_fusion(None, one, one, one, one, 0.5, 0.5, one) == E_INVALID and "null" in err()
    assert lib.stcn_aggregate_wbg(None, None, 1, 100, 1, 0, one) == E_INVALID and "null" in err()
    assert lib.stcn_aggregate_wbg(None, one, 1, 100, 1, 0, None) == E_INVALID
    assert lib.stcn_aggregate_wbg(None, one, 1, 0, 1, 0, one) == E_INVALID and "npix=0" in err()
    assert lib.stcn_fusion_model_create(0, None, 0, C.byref(h)) == E_INVALID and "null" in err()
    assert lib.stcn_test_transpose(None, one, one, 1, 8, 6, 8, 0, 1) == E_INVALID          # C % 4
    assert lib.stcn_test_transpose(None, one, one, 1, 8, 4, 7, 0, 1) == E_INVALID          # ld < R


def test_the_six_python_entry_points_exist():
    for n in ("encode_key", "encode_value", "segment_with_query", "get_attention"):
        assert callable(getattr(PropagationNetwork, n)), n
    assert list(inspect.signature(FusionNet.forward).parameters) == ["self", "im", "seg1", "seg2", "attn", "time"]
    from mivos.model.aggregate import aggregate_wbg
    from eva_vos_amd import stages
    assert aggregate_wbg is stages.aggregate_wbg
    import mivos.model.fusion_net
    import mivos.model.propagation.prop_net
    assert mivos.model.propagation.prop_net.PropagationNetwork is PropagationNetwork and mivos.model.fusion_net.FusionNet is FusionNet


def test_the_training_forward_still_raises():
    with pytest.raises(RuntimeError):
        PropagationNetwork()(torch.zeros(1))


def test_host_tensors_are_refused_and_nothing_falls_back_to_the_cpu():
    """Without a GPU every entry point raises the RuntimeError InferenceCore raises; with one, tensors in host memory are a ValueError."""
    from mivos.model.aggregate import aggregate_wbg
    p, f = PropagationNetwork(), FusionNet()
    z = torch.zeros
    calls = [lambda: p.encode_key(z(1, 3, 32, 32)),
             lambda: p.encode_value(z(1, 3, 32, 32), z(1, 1024, 2, 2), z(1, 1, 32, 32)),
             lambda: p.segment_with_query(z(1, 64, 1, 2, 2), z(1, 512, 1, 2, 2), z(1, 512, 4, 4), z(1, 256, 8, 8), z(1, 64, 2, 2), z(1, 512, 2, 2)),
             lambda: p.get_attention(z(1, 64, 1, 2, 2), z(2, 1, 32, 32), z(2, 1, 32, 32), z(1, 64, 2, 2)),
             lambda: f(z(1, 3, 32, 32), z(1, 1, 32, 32), z(1, 1, 32, 32), z(1, 2, 32, 32), z(1, 2)),
             lambda: aggregate_wbg(z(1, 1, 32, 32), keep_bg=True)]
    for c in calls:
        with pytest.raises(ValueError if torch.cuda.is_available() else RuntimeError, match="no CPU fallback"):
            c()
