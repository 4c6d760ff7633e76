"""CPU: the conv planners are pure host code - the kernel family and plan of every CONVS case of test_gpu_kernels.py, without a device
(stcn_test_conv_path sets up what stcn_test_conv sets up, plans and launches nothing)."""
import ctypes as C

import pytest

from test_gpu_kernels import CONVS, PATHS


def conv_path(B, H, W, Cin, Cout, K, s, flags, splitk):
    from eva_vos_amd import _lib
    out = C.create_string_buffer(96)
    _lib.check(_lib.lib().stcn_test_conv_path(B, H, W, Cin, Cout, K, s, flags, splitk, out, len(out)), "stcn_test_conv_path")
    return out.value.decode()


@pytest.mark.parametrize("B,H,W,Cin,Cout,K,s,flags,splitk,path", [c + (p,) for c, p in zip(CONVS, PATHS) if c[4] > 1])
def test_planned_path_of_every_conv_case(B, H, W, Cin, Cout, K, s, flags, splitk, path, monkeypatch):
    # the settings of the default variant of test_conv_matches_fp64_reference (read when the hook makes its workspace)
    monkeypatch.setenv("STCN_WINO_MIN_CIN", "64")
    monkeypatch.setenv("STCN_FUSION_CONV12", "1")
    ran = conv_path(B, H, W, Cin, Cout, K, s, flags, splitk)
    print(ran)
    assert ran.startswith(path), (ran, path)
