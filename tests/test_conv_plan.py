"""CPU: the conv planners are pure host code - the kernel family and plan of every CONVS case of test_gpu_kernels.py, without a device
(stcn_test_conv_path sets up what stcn_test_conv sets up, plans and launches nothing)."""
import ctypes as C

import pytest

from large_extents import ENGINE_CONVS, LARGE_CONVS, REFUSED_CONV, conv_peak_gb, periodic_check
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


# ---------------------------------------------------------------------------------------------- operands of gigabytes
E_INVALID = -1
IMG = 17 * 23                 # pixels of the ragged image of the large cases
F22_TILES, F44_TILES = 9 * 12, 5 * 6         # Winograd tiles of one such image


def refused(case):
    from eva_vos_amd import _lib
    out = C.create_string_buffer(96)
    rc = _lib.lib().stcn_test_conv_path(*case, out, len(out))
    return rc == E_INVALID and "2 GiB" in _lib.lib().stcn_last_error().decode()


def affine_out(case):
    """the optional 28th number of stcn_test_conv_plan"""
    from eva_vos_amd import _lib
    iv, dv = (C.c_int32 * (len(FIELDS) + 1))(), (C.c_double * 2)()
    _lib.check(_lib.lib().stcn_test_conv_plan(*case, iv, len(iv), dv), "stcn_test_conv_plan")
    return iv[len(FIELDS)]


@pytest.mark.parametrize("name,case,residual,path,peak_gb", LARGE_CONVS + ENGINE_CONVS, ids=[c[0] for c in LARGE_CONVS + ENGINE_CONVS])
def test_planned_path_of_every_large_extent_case(name, case, residual, path, peak_gb):
    """What test_gpu_large_extents.py runs, planned without a device (256 CUs assumed, the MI355X value)."""
    ran = conv_path(*case)
    print(ran)
    assert ran.startswith(path), (ran, path)
    # the peak the case states in its id is the one its shape gives (operands, the hook's Winograd workspace, the fp64 chunks of the check)
    peak = conv_peak_gb(case, residual)
    assert abs(peak - peak_gb) <= 0.1 and peak < 16, (peak, peak_gb)


def test_an_input_of_2_gib_is_refused_by_the_planner():
    assert refused(REFUSED_CONV)
    assert refused(REFUSED_CONV[:5] + (1, 1, 2, 0))


def test_input_boundary_at_2_pow_31_bytes():
    """256 channels: 400 384 bytes per image, 5363 images are 2^31 - 224 256 bytes, 5364 are beyond."""
    per = IMG * 256 * 4
    B = (1 << 31) // per
    assert B * per < 1 << 31 <= (B + 1) * per and B == 5363
    assert conv_path(B, 17, 23, 256, 64, 3, 1, 2, 0).startswith("direct ")             # V of either Winograd form is beyond 4 GiB here
    assert conv_path(B, 17, 23, 256, 64, 1, 1, 2, 0).startswith("direct_pointwise")
    assert refused((B + 1, 17, 23, 256, 64, 3, 1, 2, 0)) and refused((B + 1, 17, 23, 256, 64, 1, 1, 2, 0))


def test_winograd_boundaries_at_v_of_2_pow_32_bytes():
    """wino_extents_ok: V of positions * Cin * Mt_pad * 4 bytes must stay BELOW 2^32.  256 channels: F(2x2) 16 384 bytes per padded tile, the
    last batch whose 108 tiles per image pad (to 64) to fewer than 262 144 tiles is 2426; F(4x4) 36 864 bytes per padded tile (30 per image,
    padded to 128), the last batch is 3882.  One image more and the conv runs direct (V of the other form is larger still)."""
    pad = lambda n, u: -(-n // u) * u
    b2 = max(B for B in range(2400, 2440) if 16 * 256 * 4 * pad(B * F22_TILES, 64) < 1 << 32)
    b4 = max(B for B in range(3860, 3900) if 36 * 256 * 4 * pad(B * F44_TILES, 128) < 1 << 32)
    assert (b2, b4) == (2426, 3882)
    assert 16 * 256 * 4 * pad((b2 + 1) * F22_TILES, 64) == 1 << 32                      # exactly 2^32: declined
    lo, hi = conv_plan(b2, 17, 23, 256, 64, 3, 1, 2, 0), conv_plan(b2 + 1, 17, 23, 256, 64, 3, 1, 2, 0)
    assert lo["family"] == WINO2 and lo["v_floats"] * 4 < 1 << 32 and hi["family"] == 4
    assert conv_path(b2 + 1, 17, 23, 256, 64, 3, 1, 2, 0).startswith("direct ")
    lo, hi = conv_plan(b4, 17, 23, 256, 64, 3, 1, 6, 0), conv_plan(b4 + 1, 17, 23, 256, 64, 3, 1, 6, 0)
    assert lo["family"] == WINO4 and lo["v_floats"] * 4 < 1 << 32 and hi["family"] == 4
    check_winograd_plan((b4, 17, 23, 256, 64, 3, 1, 6, 0), lo)
    assert conv_path(b4 + 1, 17, 23, 256, 64, 3, 1, 6, 0).startswith("direct ")


def test_dense_output_boundary_at_2_pow_32_bytes():
    """affine_out (descriptor stores, one address add per row) while (M + 128) * N * 4 < 2^32; beyond, the epilogue with 64-bit addresses.
    64 -> 512 pointwise: 5363 images give M + 128 = 2 097 061 < 2^21, 5364 give 2 097 452."""
    B = max(b for b in range(5300, 5400) if (b * IMG + 128) * 512 * 4 < 1 << 32)
    assert B == 5363
    for b, want, path in ((B, 1, "direct_pointwise_chain"), (B + 1, 0, "direct_pointwise ")):        # the chain kernel needs the dense output
        case = (b, 17, 23, 64, 512, 1, 1, 2, 0)
        assert conv_path(*case).startswith(path) and affine_out(case) == want, (case, want, path)
    assert affine_out((5600, 17, 23, 64, 256, 3, 1, 3, 0)) == 1 and affine_out((5600, 17, 23, 64, 512, 1, 1, 2, 0)) == 0


def test_chain_guard_boundary_at_2_pow_31_bytes():
    """pw_chain_tiles: with N % 64 != 0 the chain kernel is taken only while (M + 64) * N * 4 < 2^31 (lanes of columns >= N add row offsets to
    the 0x80000000 sentinel).  N = 160: 8581 images are below, 8582 beyond; N = 256 has no such lane and keeps the chain."""
    B = max(b for b in range(8500, 8700) if (b * IMG + 64) * 160 * 4 < 1 << 31)
    assert B == 8581
    assert conv_path(B, 17, 23, 64, 160, 1, 1, 2, 0).startswith("direct_pointwise_chain") and conv_plan(B, 17, 23, 64, 160, 1, 1, 2, 0)["chain"] > 0
    assert conv_path(B + 1, 17, 23, 64, 160, 1, 1, 2, 0).startswith("direct_pointwise ") and conv_plan(B + 1, 17, 23, 64, 160, 1, 1, 2, 0)["chain"] == 0
    assert conv_path(B + 1, 17, 23, 64, 256, 1, 1, 2, 0).startswith("direct_pointwise_chain")


def test_a_forced_split_k_never_sees_more_output_than_its_slabs_hold():
    """conv_plan drops a split of more than ws_floats (the hooks: 16 Mi) slab floats: splitk = 2 holds for M * N <= 8 Mi (83 images of
    64 -> 256), one image more runs unsplit - so conv_reduce_kernel cannot be given an output of gigabytes through the hook."""
    assert 2 * 83 * IMG * 256 <= 16 << 20 < 2 * 84 * IMG * 256
    assert conv_path(83, 17, 23, 64, 256, 3, 1, 3, 2).startswith("direct splitk=2")
    assert conv_path(84, 17, 23, 64, 256, 3, 1, 3, 2).startswith("direct splitk=1")
    assert conv_path(5600, 17, 23, 64, 256, 3, 1, 3, 2).startswith("direct splitk=1")


# the checker of test_gpu_large_extents.py on small NumPy arrays: what a 32-bit offset slip does to a periodic batch must be reported
def periodic_output(B, dense, period, seed=3):
    import numpy as np
    import torch
    exp = np.random.RandomState(seed).randn(period, dense)
    y = np.concatenate([exp[b % period] for b in range(B)]).astype(np.float32)
    return y, torch.from_numpy(exp.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("period", [3, 6])
def test_periodic_checker_passes_a_correct_output_in_whole_and_ragged_chunks(period):
    import torch
    for B, chunk in ((12, 1 << 26), (13, 500), (7, 1)):
        y, exp = periodic_output(B, 40, period)
        assert periodic_check(torch.from_numpy(y), exp, chunk) == (0.0, 0)


@pytest.mark.parametrize("shift_bytes", [1 << 31, 1 << 32])
@pytest.mark.parametrize("period", [3, 6])
def test_periodic_checker_reports_a_write_displaced_by_a_wrapped_offset(shift_bytes, period):
    """A tile of 64 values whose stores went shift_bytes away (modulo the small buffer: only the phase against the period matters, and a
    period of 3 images never divides a power of two): NaN where it belonged, wrong values where it landed."""
    import numpy as np
    import torch
    B, dense = 24, 40
    good, exp = periodic_output(B, dense, period)
    assert (shift_bytes // 4) % (period * dense) != 0
    y = good.copy()
    src = np.arange(300, 364)
    y[src] = np.nan                                              # the output was NaN before the call ...
    y[(src + shift_bytes // 4) % y.size] = good[src]             # ... and the tile's values went elsewhere
    err, bad = periodic_check(torch.from_numpy(y), exp, 200)
    assert bad == 64 and err > 1e-3, (err, bad)
    y = good.copy()
    y[(src + shift_bytes // 4) % y.size] = good[src]             # the same slip in a second write of the tile: values alone
    err, bad = periodic_check(torch.from_numpy(y), exp, 200)
    assert bad == 0 and err > 1e-3, (err, bad)


def test_periodic_checker_reports_a_dropped_tile():
    import numpy as np
    import torch
    y, exp = periodic_output(24, 40, 3)
    y[-32:] = np.nan                                             # the last tile of the last element was never stored
    assert periodic_check(torch.from_numpy(y), exp, 200) == (0.0, 32)
