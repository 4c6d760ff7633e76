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


# ---------------------------------------------------------------------------------------------- the plan in numbers
FIELDS = ("family splitk ppw tail n_in n_gemm reduce TH TW Mt Mt_pad KB kb_per_split "
          "mb tiles_m tiles_n grid full_wg pieces per chunks tm_per_chunk tile_big rem_full rem_split rem_per chain").split()
WINO4, WINO2 = 2, 3


def conv_plan(B, H, W, Cin, Cout, K, s, flags, splitk):
    """the numeric plan (stcn_test_conv_plan) as a dict, v_floats and fl_exec included"""
    from eva_vos_amd import _lib
    iv, dv = (C.c_int32 * len(FIELDS))(), (C.c_double * 2)()
    _lib.check(_lib.lib().stcn_test_conv_plan(B, H, W, Cin, Cout, K, s, flags, splitk, iv, len(iv), dv), "stcn_test_conv_plan")
    d = dict(zip(FIELDS, iv))
    d["v_floats"], d["fl_exec"] = dv[0], dv[1]
    return d


# every stride-1 3x3 layer shape (Cin, Cout) of the model at 1/4, 1/8 and 1/16 scale of 480x864
LAYERS = {4: [(64, 64), (256, 256)],
          8: [(128, 128), (512, 512), (512, 256), (256, 256)],
          16: [(256, 256), (1024, 64), (1024, 512), (512, 512), (256, 512)]}
BATCHES = sorted(set(range(1, 9)) | {5 * k for k in range(1, 9)})
SWEEP = [(B, 480 // sc, 864 // sc, cin, cout, 3, 1, fl, 0)
         for sc, layers in LAYERS.items() for cin, cout in layers for B in BATCHES for fl in (0, 4)]
WINO_CONVS = [c for c, p in zip(CONVS, PATHS) if p.startswith("wino")]


def check_winograd_plan(case, pl):
    """what must hold between the numbers of a Winograd plan, whichever launch it describes"""
    B, H, W, Cin, Cout, K, s, flags, splitk = case
    edge, positions = (4, 36) if pl["family"] == WINO4 else (2, 16)
    assert pl["TH"] == -(-H // edge) and pl["TW"] == -(-W // edge) and pl["Mt"] == B * pl["TH"] * pl["TW"] and pl["KB"] == Cin // 8
    assert pl["Mt"] <= pl["Mt_pad"] < pl["Mt"] + 64 and pl["Mt_pad"] % 64 == 0
    assert pl["v_floats"] == positions * Cin * pl["Mt_pad"]
    if pl["family"] == WINO4:
        assert pl["n_in"] == pl["n_gemm"] == pl["chunks"]
        assert pl["reduce"] == (pl["pieces"] > 1)
        pieces, per = pl["pieces"], pl["per"]
        assert pl["mb"] in (1, 2) and pl["tiles_m"] * 32 * pl["mb"] == pl["Mt_pad"] and pl["tiles_n"] * 32 == Cout
        if pl["mb"] == 1:
            assert pl["grid"] == pl["full_wg"] + (pl["tiles_m"] * pl["tiles_n"] - pl["full_wg"]) * pieces
        else:
            assert pieces == 1 and pl["grid"] == pl["tiles_m"] * pl["tiles_n"]
        assert pieces <= 8
        # the chunk slices [c * tm_per_chunk, min(tiles_m, (c + 1) * tm_per_chunk)) cover [0, tiles_m) exactly once
        slices = [(c * pl["tm_per_chunk"], min(pl["tiles_m"], (c + 1) * pl["tm_per_chunk"])) for c in range(pl["chunks"])]
        assert slices[0][0] == 0 and slices[-1][1] == pl["tiles_m"]
        assert all(lo < hi for lo, hi in slices) and all(a[1] == b[0] for a, b in zip(slices, slices[1:]))
        assert pl["chunks"] == 1 or pl["mb"] == 2
    else:
        assert pl["n_in"] == pl["n_gemm"] == 1
        assert pl["reduce"] == (pl["splitk"] > 1)
        assert pl["ppw"] in (1, 2)
        pieces, per = pl["splitk"], pl["kb_per_split"]
    assert per * (pieces - 1) < pl["KB"] <= per * pieces           # no K range is empty, together they cover K


@pytest.mark.parametrize("case", WINO_CONVS, ids=lambda c: "-".join(map(str, c)))
def test_the_numbers_of_every_winograd_conv_case_agree(case, monkeypatch):
    monkeypatch.setenv("STCN_WINO_MIN_CIN", "64")
    pl = conv_plan(*case)
    print(pl)
    assert pl["family"] in (WINO4, WINO2)
    check_winograd_plan(case, pl)


@pytest.mark.parametrize("chunk_mb", [None, "0", "1", "8"])
def test_the_numbers_of_the_model_layer_plans_agree(chunk_mb, monkeypatch):
    """every stride-1 3x3 layer shape of the model, as an F(2x2) layer (flags 0) and as an F(4x4) one (flags 4), over one to eight frames
    and the decode groups of one to eight objects; under small V slices the big launches are chunked"""
    if chunk_mb is not None:
        monkeypatch.setenv("STCN_WINO4_CHUNK_MB", chunk_mb)
    seen = {WINO4: 0, WINO2: 0}
    chunked = tail = small = split2 = 0
    for case in SWEEP:
        pl = conv_plan(*case)
        if pl["family"] not in seen:
            continue                        # 64-channel layers in small launches: the direct kernel
        assert case[3] >= 128 or case[7] & 4 or pl["Mt"] >= 16384, (case, pl)
        seen[pl["family"]] += 1
        try:
            check_winograd_plan(case, pl)
        except AssertionError as ex:
            raise AssertionError((case, pl)) from ex
        chunked += pl["chunks"] > 1
        tail += pl["family"] == WINO4 and pl["pieces"] > 1 and pl["full_wg"] > 0
        small += pl["family"] == WINO4 and pl["pieces"] > 1 and pl["full_wg"] == 0
        split2 += pl["family"] == WINO2 and pl["splitk"] > 1
    print(seen, chunked, tail, small, split2)
    # the sweep reaches every kind of launch the checks above distinguish
    assert seen[WINO4] >= 150 and seen[WINO2] >= 100 and tail and small and split2
    assert (chunked > 0) == (chunk_mb != "0")


def test_conv_plan_rejects_bad_arguments():
    from eva_vos_amd import _lib
    lib = _lib.lib()
    iv, dv = (C.c_int32 * len(FIELDS))(), (C.c_double * 2)()
    assert lib.stcn_test_conv_plan(1, 30, 54, 256, 256, 3, 1, 0, 0, iv, len(iv) - 1, dv) != 0
    assert lib.stcn_test_conv_plan(1, 30, 54, 256, 256, 3, 1, 0, 0, None, len(iv), dv) != 0
    assert lib.stcn_test_conv_plan(1, 30, 54, 256, 256, 3, 1, 0, 0, iv, len(iv), None) != 0
    assert lib.stcn_test_conv_plan(1, 30, 54, 6, 256, 3, 1, 0, 0, iv, len(iv), dv) != 0
