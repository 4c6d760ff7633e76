"""The simulated user without a GPU: the host restatement against the reference's own robot (tests/golden/robot_clicks.npz, written by
tools/gen_golden_robot.py), the C ABI's new rows, and its refusals - all of them before a device call."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from eva_vos_amd import _lib, annotate, eval_driver, metrics, robots

GOLD = load_golden("robot_clicks")
CASES = sorted({k.rsplit(".", 1)[0] for k in GOLD})
NEW = ["stcn_robot_scratch", "stcn_robot_click", "stcn_robot_bbox", "stcn_robot_best_mask", "stcn_metrics_round_typed"]


def case(name):
    iou = float(GOLD[f"{name}.iou"])
    return GOLD[f"{name}.pred"], GOLD[f"{name}.gt"], int(GOLD[f"{name}.mode"]), None if np.isnan(iou) else iou


def test_the_fixture_holds_every_case_at_both_sizes():
    kinds = {n.rsplit("_", 1)[0] for n in CASES}
    assert len(CASES) == 2 * len(kinds) and {n.rsplit("_", 1)[1] for n in CASES} == {"48x64", "37x53"}
    for must in ("blob", "crossing", "spiral", "diagonal", "equal_fp", "equal_fp_fn", "ring", "border", "equal", "empty_pred", "median_even",
                 "median_odd", "l_shape", "two_clicks"):
        assert must in kinds


@pytest.mark.parametrize("name", CASES)
def test_the_host_restatement_equals_the_reference_robot(name):
    pred, gt, mode, iou = case(name)
    robot = robots.HostClickRobot()
    clicks, labels = robot.middle_click(gt) if mode == robots.MIDDLE else robot.interact(pred, gt, iou)
    assert clicks.tolist() == GOLD[f"{name}.clicks"].tolist() and labels.tolist() == GOLD[f"{name}.labels"].tolist()


def test_the_fixtures_reach_the_branches_they_are_named_for():
    rec = lambda n: robots.host_click_record(*case(n))[0]      # noqa: E731
    for size in ("48x64", "37x53"):
        assert rec(f"ring_{size}")[robots.MOVED] == 1 and rec(f"l_shape_{size}")[robots.MOVED] == 1 and rec(f"l_shape_middle_{size}")[robots.MOVED] == 1
        assert rec(f"diagonal_{size}")[[robots.FN_SIZE, robots.FN_COUNT]].tolist() == [18, 2]
        r = rec(f"equal_fp_fn_{size}")
        assert r[robots.FP_SIZE] == r[robots.FN_SIZE] and r[robots.CLASS] == 1 and r[robots.LABEL0] == 0
        assert rec(f"equal_fp_{size}")[robots.FP_COUNT] == 2
        assert rec(f"two_clicks_{size}")[robots.N_CLICKS] == 2 and rec(f"two_clicks_high_iou_{size}")[robots.N_CLICKS] == 1
        assert rec(f"equal_{size}")[robots.CLASS] == 0
    # the ring's centroid has more than one nearest object pixel: the first in raster order is taken
    pred, gt, _, _ = case("ring_48x64")
    ys, xs = np.nonzero(gt)
    d2 = (xs - 32) ** 2 + (ys - 24) ** 2
    assert (d2 == d2.min()).sum() > 1 and rec("ring_48x64")[[robots.X0, robots.Y0]].tolist() == [xs[d2.argmin()], ys[d2.argmin()]]


def test_an_empty_object_has_no_click_and_no_box():
    z = np.zeros((9, 11), np.uint8)
    rec, comp = robots.host_click_record(z, z)
    assert rec.tolist() == [0] * robots.RECORD_INTS and not comp.any()
    with pytest.raises(ValueError):
        robots.HostClickRobot().middle_click(z)
    assert robots.host_bbox(z).tolist() == [0] * 5
    with pytest.raises(ValueError):
        robots.HostBboxRobot().interact(z)
    z[2:5, 3:9] = 1
    assert robots.HostBboxRobot().interact(z).tolist() == [[3.0, 2.0, 8.0, 4.0]]


def test_a_frame_of_one_row_one_column_or_one_pixel_is_a_frame():
    """A 2-D mask is taken as it is; only a mask with more dimensions loses those of extent one."""
    row = np.zeros((1, 9), np.uint8)
    row[0, 2:7] = 1
    for gt, click, box in ((row, [4, 0], [1, 2, 0, 6, 0]), (row.T.copy(), [0, 4], [1, 0, 2, 0, 6])):
        rec, comp = robots.host_click_record(np.zeros_like(gt), gt)
        assert comp.shape == gt.shape and np.array_equal(comp, gt)
        assert rec[:robots.MOVED + 1].tolist() == [1, click[0], click[1], 1, 0, 0, 0, 2, 0, 5, 0, 1, 0]
        assert robots.host_click_record(None, gt, robots.MIDDLE)[0][:4].tolist() == [1, click[0], click[1], 1]
        assert robots.host_bbox(gt).tolist() == box
        clicks, labels = robots.HostClickRobot().interact(np.zeros_like(gt), gt)
        assert clicks.tolist() == [click] and labels.tolist() == [1]
        # the reference's [1,1,H,W] of the same frame, and a stack of candidates [M,1,H,W]
        assert robots.host_click_record(np.zeros_like(gt)[None, None], gt[None, None])[0].tolist() == rec.tolist()
        half = gt.copy()
        half.reshape(-1)[2:4] = 0
        iou, idx, counts = robots.host_best_mask(np.stack([half, gt, half])[:, None], gt)
        assert (idx, iou) == (1, 1.0) and counts.tolist() == [[3, 5], [5, 5], [3, 5]]
        assert robots.host_best_mask([half], gt[None])[2].tolist() == [[3, 5]]
    one = np.ones((1, 1), np.uint8)
    assert robots.host_click_record(0 * one, one)[0][:robots.MOVED + 1].tolist() == [1, 0, 0, 1, 0, 0, 0, 2, 0, 1, 0, 1, 0]
    assert robots.host_click_record(one, 0 * one)[0][:robots.MOVED + 1].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0]
    assert robots.host_click_record(one, one)[0][:4].tolist() == [1, 0, 0, 1] and robots.host_click_record(one[None, None], one[None])[1].shape == (1, 1)
    assert robots.host_bbox(one).tolist() == [1, 0, 0, 0, 0] and robots.host_bbox(0 * one).tolist() == [0] * 5
    assert robots.host_best_mask([one, 0 * one], one)[:2] == (1.0, 0)
    assert robots.scratch_bytes(1, 1) == 256 + 16 + 8              # the header, two histogram words rounded to 16 bytes, a parent and a size


def test_every_shape_accepted_before_keeps_its_meaning():
    m = np.arange(12).reshape(3, 4) % 3 == 0
    for shape in ((3, 4), (1, 3, 4), (1, 1, 3, 4), (3, 4, 1), (1, 3, 1, 4), (3, 1, 4)):
        assert np.array_equal(robots._as_bool(m.reshape(shape)), m)
        assert robots._frame_shape(shape) == (3, 4)
    for shape, hw in (((1, 4), (1, 4)), ((4, 1), (4, 1)), ((1, 1), (1, 1)), ((1, 1, 1, 4), (1, 4)), ((1, 1, 4, 1), (4, 1)), ((1, 1, 1, 1), (1, 1))):
        assert robots._frame_shape(shape) == hw
    for shape in ((4,), (), (2, 3, 4), (2, 1, 3, 4), (4, 1, 1)):
        assert robots._frame_shape(shape) is None
        with pytest.raises(AssertionError):
            robots._as_bool(np.zeros(shape))


@pytest.mark.parametrize("name", NEW)
def test_the_new_symbols_are_declared_and_exported(name):
    assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)


def test_the_prototypes_have_the_headers_arguments():
    P, I, D = C.c_void_p, C.c_int, C.c_double
    assert _lib.PROTOTYPES["stcn_robot_scratch"] == (I, [I, I, C.POINTER(C.c_int64)])
    assert _lib.PROTOTYPES["stcn_robot_click"] == (I, [P, P, P, I, I, I, I, D, P, P, P])
    assert _lib.PROTOTYPES["stcn_robot_bbox"] == (I, [P, P, I, I, P])
    assert _lib.PROTOTYPES["stcn_robot_best_mask"] == (I, [P, P, P, I, I, I, P])
    assert len(_lib.PROTOTYPES["stcn_metrics_round_typed"][1]) == len(_lib.PROTOTYPES["stcn_metrics_round"][1]) + 1
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "stcn_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
    for name, value in (("N_CLICKS", 0), ("CLASS", 7), ("FP_SIZE", 8), ("FN_COUNT", 11), ("MOVED", 12), ("RECORD_INTS", 16)):
        assert getattr(robots, name) == value and f"#define STCN_ROBOT_{name}" in header


def test_the_scratch_size_needs_no_gpu():
    # the header, the two histograms, and a parent and a size word per pixel
    for H, W in ((48, 64), (37, 53), (480, 854), (1, 1 << 24), (4096, 4096)):
        n = robots.scratch_bytes(H, W)
        assert n >= 8 * H * W + 4 * (H + W) and n <= 8 * H * W + 4 * (H + W) + 512 and n % 8 == 0


def _refused(rc, *needles):
    assert rc == -1                                            # STCN_E_INVALID
    msg = _lib.lib().stcn_last_error().decode()
    for n in needles:
        assert n in msg, msg


BUF = (C.c_uint8 * 64)()
PTR = C.cast(BUF, C.c_void_p)           # never dereferenced: every call below is refused on the host


@pytest.mark.parametrize("H,W", [(0, 5), (5, 0), (-1, 4), (4097, 4096), (1, (1 << 24) + 1), (1 << 16, 1 << 16)])
def test_every_call_refuses_a_frame_outside_1_to_2_pow_24_pixels(H, W):
    lib = _lib.lib()
    n = C.c_int64(-7)
    _refused(lib.stcn_robot_scratch(H, W, C.byref(n)), "stcn_robot_scratch", "bad frame")
    assert n.value == -7
    _refused(lib.stcn_robot_click(None, PTR, PTR, H, W, 0, 0, 0.0, PTR, PTR, None), "stcn_robot_click", "bad frame")
    _refused(lib.stcn_robot_bbox(None, PTR, H, W, PTR), "stcn_robot_bbox", "bad frame")
    _refused(lib.stcn_robot_best_mask(None, PTR, PTR, 3, H, W, PTR), "stcn_robot_best_mask", "bad frame")


def test_null_pointers_and_bad_modes_are_refused_before_a_device_call():
    lib = _lib.lib()
    _refused(lib.stcn_robot_scratch(4, 4, None), "stcn_robot_scratch", "null")
    for hole in range(4):
        a = [PTR] * 4
        a[hole] = None
        _refused(lib.stcn_robot_click(None, a[0], a[1], 8, 8, 0, 0, 0.0, a[2], a[3], None), "stcn_robot_click", "null")
    _refused(lib.stcn_robot_click(None, None, None, 8, 8, 1, 0, 0.0, PTR, PTR, None), "stcn_robot_click", "null")      # the middle click reads gt
    _refused(lib.stcn_robot_click(None, PTR, PTR, 8, 8, 2, 0, 0.0, PTR, PTR, None), "stcn_robot_click", "mode 2")
    _refused(lib.stcn_robot_click(None, PTR, PTR, 8, 8, 0, 0, 0.0, C.c_void_p(PTR.value + 4), PTR, None), "stcn_robot_click", "aligned")
    _refused(lib.stcn_robot_bbox(None, None, 8, 8, PTR), "stcn_robot_bbox", "null")
    _refused(lib.stcn_robot_bbox(None, PTR, 8, 8, None), "stcn_robot_bbox", "null")
    for hole in range(3):
        a = [PTR] * 3
        a[hole] = None
        _refused(lib.stcn_robot_best_mask(None, a[0], a[1], 3, 8, 8, a[2]), "stcn_robot_best_mask", "null")
    for M in (0, -1, 9):
        _refused(lib.stcn_robot_best_mask(None, PTR, PTR, M, 8, 8, PTR), "stcn_robot_best_mask", f"M = {M}")


def _typed(**kw):
    a = {n: PTR for n in ("masks", "gt", "type", "annot", "noobj", "gen", "scratch", "counts", "quality", "select")}
    a.update(nh=64, nw=64, lh=7, lw=2, T=4, H=50, W=60, t0=0, t1=3, j_only=0)
    a.update(kw)
    return _lib.lib().stcn_metrics_round_typed(None, a["masks"], a["nh"], a["nw"], a["lh"], a["lw"], a["gt"], a["type"], a["annot"], a["noobj"], a["T"],
                                               a["H"], a["W"], a["t0"], a["t1"], a["j_only"], 20.0, a["gen"], a["scratch"], a["counts"], a["quality"],
                                               a["select"])


@pytest.mark.parametrize("name", ["masks", "gt", "type", "annot", "noobj", "gen", "scratch", "counts", "quality", "select"])
def test_the_typed_round_refuses_null_pointers(name):
    _refused(_typed(**{name: None}), "stcn_metrics_round_typed", "null")


def test_the_typed_round_keeps_the_rounds_other_refusals():
    _refused(_typed(t0=3, t1=2), "stcn_metrics_round_typed", "[3, 2)")
    _refused(_typed(nh=40), "stcn_metrics_round_typed", "crop")
    _refused(_typed(H=1), "stcn_metrics_round_typed", "bad shape")


# ------------------------------------------------------------------------------------------------ the driver's new names
def test_the_typed_policies_stand_beside_the_mask_policies():
    assert eval_driver.TYPED_POLICIES == ("rand_type", "rand_rand", "oracle_oracle")
    assert not set(eval_driver.TYPED_POLICIES) & set(eval_driver.POLICIES)
    assert eval_driver.POLICIES == ("oracle_mask", "rand_mask", "qnet_mask", "upper_bound_mask", "l2_mask")


def test_typed_policies_refuse_what_they_cannot_run_before_touching_the_engine():
    s = {"num_frames": 4, "object_ids": [0, 1], "num_objects": 2}
    with pytest.raises(ValueError, match="one annotation type"):
        eval_driver.run_typed_policy("rand_type", None, s, 3, None, ["click", "mask"])
    with pytest.raises(ValueError, match="more than one"):
        eval_driver.run_typed_policy("rand_rand", None, s, 3, None, ["mask"])
    with pytest.raises(AttributeError):
        eval_driver.run_typed_policy("oracle_oracle", None, s, 3, None, ["scribble", "mask"])
    with pytest.raises(ValueError, match="one-object policy"):
        eval_driver.run_typed_policy("oracle_oracle", None, s, 3, None, ["3clicks", "mask"])
    with pytest.raises(ValueError, match="multi-object sessions support"):
        eval_driver.run("", "", "", None, None, "rand_type", multi_object=True, annotator="component", annotation_types=["click"])
    with pytest.raises(ValueError, match="unknown annotator"):
        eval_driver.make_annotator("sam")


def test_the_component_predictor_answers_prompts_by_its_rules():
    gt = np.zeros((20, 30), np.uint8)
    gt[5:12, 6:20] = 1
    p = annotate.ComponentPredictor()
    p.set_target(gt)
    p.set_image(None)
    masks, scores, logits = p.predict(click_coords=np.array([[10, 8]]), click_labels=np.array([1]))      # a positive click on the object: all of it
    assert masks.shape == (3, 1, 20, 30) and logits.shape == (3, 20, 30) and scores.tolist() == pytest.approx([0.9, 0.8, 0.7])
    m = masks[:, 0].numpy()
    assert m[0].sum() == 5 * 12 and m[1].sum() == 9 * 16 and m[2].sum() == 11 * 18 and not any(np.array_equal(v, gt != 0) for v in m)
    assert np.array_equal(logits > 0, m) and set(np.unique(logits).tolist()) == {-4.0, 4.0}
    # from its own dilated answer, a negative click on the surplus ring removes it; a click elsewhere changes nothing
    again, _, _ = p.predict(click_coords=np.array([[10, 8], [5, 4], [28, 18]]), click_labels=np.array([1, 0, 0]), mask_input=logits[1][None])
    assert again[0, 0].numpy().sum() == 5 * 12
    box, _, _ = p.predict(bbox=np.array([[6.0, 5.0, 19.0, 11.0]]))
    assert box[0, 0].numpy().sum() == 5 * 12 and box[1, 0].numpy().sum() == 9 * 16
    p.reset_image()
    with pytest.raises(AssertionError):
        p.predict()


def test_the_host_annotator_runs_the_references_loops_over_the_stand_in():
    import torch
    gt = torch.zeros((40, 50), dtype=torch.uint8)
    gt[8:25, 10:34] = 1
    mivos = torch.zeros((1, 40, 50), dtype=torch.bool)
    mivos[0, 10:30, 12:40] = True
    a = annotate.PromptAnnotator.on_host(annotate.ComponentPredictor())
    mask, cost, iou, logits, clicks, labels, bbox = a.annotate("mask", gt)
    assert cost == 80 and iou == 1 and mask is gt
    assert a.annotate("3clicks", torch.zeros_like(gt))[1:3] == (3, 20)
    mask, cost, iou, logits, clicks, labels, bbox = a.annotate("3clicks", gt, None, mivos, None)
    assert cost == 3 * 1.5 + 1 and mask.shape == (1, 40, 50) and 0.5 < iou < 1 and bbox is None and len(clicks) == len(labels) >= 3
    prev = dict(sam_logits=logits, click_coords=clicks, click_labels=labels, bbox=None)
    again = a.annotate("click", gt, None, mask, prev)
    assert len(again[4]) == len(clicks) + 1 and again[1] == 1.5 + 1
    mask, cost, iou, logits, clicks, labels, bbox = a.annotate("bbox", gt)
    assert cost == 7 and bbox.tolist() == [[10.0, 8.0, 33.0, 24.0]] and clicks is None
    assert metrics._current_types(5, [0, 3, 3, 1], [1, 2, 1, 2]).tolist() == [1, 2, 0, 1, 0]
