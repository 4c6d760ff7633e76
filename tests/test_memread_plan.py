"""CPU: the launch plan and the scratch layout of the top-k memory read are pure host code (memread_plan / memread_scratch_floats, through
stcn_memread_plan / stcn_memread_scratch) - checked against what the kernels need in closed form, not against a copy of the planner.

What the kernels need of a plan for N bank rows and Q queries (memread.hip):
  * threshold_kernel takes at most 512 group maxima per query, pass 1 writes 64 per chunk: nc1 * 64 <= 512;
  * merge_readout_kernel stages the lists of at most 32 chunks per query: nc2 <= 32;
  * the chunks of a pass cover its steps, and none is empty (an empty pass-1 chunk would hand 64 maxima of -inf to the threshold);
  * the ns sampled steps of pass 1, every ss-th one, reach the end of the bank: ns * ss >= steps;
and of the scratch, which depends on Q alone and so must hold for every N:
  * gmax holds pass 1's maxima [Q][nc1 * 64] and, later in the same read, the selection of a read of several objects (indices and weights
    [Q][50] each);
  * cand_v / cand_i hold pass 2's lists [nc2][Q][50], cand_n their lengths [nc2][Q], tau one threshold per query."""
import ctypes as C

import pytest

NS = (50, 63, 64, 65, 1620, 32_400, 168_480, 2_000_000)
QS = (1, 16, 63, 64, 65, 97, 333, 1531, 1620, 8100, 12_960, 65_536, 65_537, 259_200)
TOPK = 50       # STCN_MAX_TOP_K: the stride of every candidate list


def plan(N, Q):
    from eva_vos_amd import _lib
    pl = (C.c_int32 * 7)()
    _lib.check(_lib.lib().stcn_memread_plan(N, Q, pl), "stcn_memread_plan")
    return dict(zip(("steps", "ss", "ns", "nc1", "spc1", "nc2", "spc2"), pl))


def scratch(Q):
    from eva_vos_amd import _lib
    sz = (C.c_int64 * 5)()
    _lib.check(_lib.lib().stcn_memread_scratch(Q, sz), "stcn_memread_scratch")
    return dict(zip(("cand_v", "cand_i", "cand_n", "gmax", "tau"), sz))


def check_plan_and_scratch(p, s, N, Q):
    """The inequalities above for one plan p and one scratch s (also run by hand on the sizes the scratch had before it was single-sourced)"""
    at = (N, Q, p, s)
    assert p["steps"] == -(-N // 64) and p["ss"] >= 1, at
    assert p["nc1"] * 64 <= 512 and 1 <= p["nc1"] <= 8 and 1 <= p["nc2"] <= 32, at
    for steps, nc, spc in ((p["ns"], p["nc1"], p["spc1"]), (p["steps"], p["nc2"], p["spc2"])):
        assert spc * nc >= steps, at                    # the chunks cover the steps ...
        assert spc * (nc - 1) < steps, at               # ... and the last one is not empty (the others are full)
    assert p["ns"] * p["ss"] >= p["steps"] and (p["ns"] - 1) * p["ss"] < p["steps"], at
    assert p["nc1"] * Q * 64 <= s["gmax"], at
    assert p["nc2"] * Q <= s["cand_n"], at
    assert p["nc2"] * Q * TOPK <= s["cand_v"] == s["cand_i"], at
    assert 2 * Q * TOPK <= s["gmax"], at
    assert s["tau"] >= Q, at


@pytest.mark.parametrize("Q", QS)
def test_every_plan_fits_the_kernels_and_the_scratch(Q):
    s = scratch(Q)
    for N in NS:
        check_plan_and_scratch(plan(N, Q), s, N, Q)


def test_the_sweep_meets_every_branch_of_the_plan():
    """sample strides 1, 4 and 8 (2 takes a bank of 96 .. 191 steps: N = 8100 beside the sweep), single- and multi-chunk passes, both chunk
    caps, and the query counts at which `resident / qblocks` reaches 1 and then 0 (one chunk either way)"""
    plans = [plan(N, Q) for N in NS for Q in QS]
    assert {p["ss"] for p in plans} == {1, 4, 8} and plan(8100, 97)["ss"] == 2
    check_plan_and_scratch(plan(8100, 97), scratch(97), 8100, 97)
    assert {1, 8} <= {p["nc1"] for p in plans} and {1, 32} <= {p["nc2"] for p in plans}
    assert plan(2_000_000, 65_536)["nc1"] == 1 and plan(2_000_000, 65_537)["nc1"] == 1


def test_scratch_of_the_shapes_the_engine_runs_is_what_it_always_was():
    """Up to a decode group of 8 frames at 480p (Q = 12 960) - and as long as 2 * Q * 50 <= 64 * pairs - the five sizes are the layout the
    engine and the hooks each spelled out before: pairs = 65536 + Q + 64 (chunk, query) lists; pairs * 50, pairs * 50, pairs, pairs * 64, Q."""
    for Q in (1, 80, 333, 1531, 1620, 8100, 12_960, 65_537):
        pairs = 65536 + Q + 64
        assert scratch(Q) == dict(cand_v=pairs * 50, cand_i=pairs * 50, cand_n=pairs, gmax=pairs * 64, tau=Q), Q


def test_gmax_grows_with_the_selection_of_a_large_read():
    """a 4K decode group: the selection of a read of several objects no longer fits 64 * pairs floats"""
    Q = 259_200
    assert scratch(Q)["gmax"] == 2 * Q * 50 > 64 * (65536 + Q + 64)


def test_memread_exports_reject_bad_arguments():
    from eva_vos_amd import _lib
    lib = _lib.lib()
    sz, pl = (C.c_int64 * 5)(), (C.c_int32 * 7)()
    assert lib.stcn_memread_scratch(0, sz) != 0 and lib.stcn_memread_scratch(16, None) != 0
    assert lib.stcn_memread_plan(0, 16, pl) != 0 and lib.stcn_memread_plan(64, 0, pl) != 0 and lib.stcn_memread_plan(64, 16, None) != 0
