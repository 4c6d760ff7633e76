"""The device robots (csrc/robot.hip) on the cases of tests/robot_cases.py: links across tile seams and corners that are the only tie of a
component, frames of one row, one column, one pixel, sizes above 2^16, coordinate sums and squared distances above 2^32, 2^24 pixels, and
the middle click's order statistic with more than one histogram entry per thread.  Every comparison is exact - records, components and
counts are integers, the IoU is compared by its fp32 bits; the yardstick is the host restatement (eva_vos_amd.robots.host_*), which
tests/test_robot_api.py holds to the reference's robot and tests/test_robot_cases.py to what each case is named for."""
import numpy as np
import pytest
import torch

import robot_cases as rc
from eva_vos_amd import robots

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(a.copy()).to(DEV)                   # (the cases are read-only arrays)


def device_run(robot, name):
    """(record as a list, component or None) of one device call; the component plane starts as sevens, so every pixel has to be written."""
    pred, gt, mode, iou = rc.get(name)
    g = to_dev(gt)
    if mode == robots.MIDDLE:
        return robot.middle_click_device(g).cpu().tolist(), None
    comp = torch.full(g.shape, 7, dtype=torch.uint8, device=DEV)
    rec = robot.interact_device(to_dev(pred), g, iou, component=comp)
    return rec.cpu().tolist(), comp.cpu().numpy()


def check_case(robot, name):
    want, want_comp = rc.host(name)
    for visit in range(2):                                      # the second call reuses the first one's scratch
        got, got_comp = device_run(robot, name)
        assert got == want, (name, visit)
        if got_comp is not None:
            assert np.array_equal(got_comp, want_comp), (name, visit)


@pytest.mark.parametrize("name", rc.names("seam"))
def test_links_across_tile_seams_and_corners(name):
    check_case(robots.ClickRobot(), name)


def test_thin_and_tiny_frames_on_one_robot():
    robot = robots.ClickRobot()                                 # one robot: a scratch per frame size, each used by three cases twice
    for name in rc.names("thin"):
        check_case(robot, name)


@pytest.mark.parametrize("name", rc.names("line"))
def test_lines_of_2_pow_17_and_2_pow_18_pixels(name):
    check_case(robots.ClickRobot(), name)


@pytest.mark.parametrize("name", rc.names("middle"))
def test_middle_clicks_with_several_histogram_entries_per_thread(name):
    check_case(robots.ClickRobot(), name)


def test_2_pow_24_pixels_equal_squares_with_first_pixels_above_2_pow_23():
    check_case(robots.ClickRobot(), "big_squares")


def test_2_pow_24_pixels_the_last_pixel_is_a_component():
    check_case(robots.ClickRobot(), "big_last_pixel")


def test_2_pow_24_pixels_both_coordinate_sums_above_2_pow_32():
    check_case(robots.ClickRobot(), "big_rectangle")


# ------------------------------------------------------------------------------------------------ box and best mask at the extents
MASKS = ["one_pixel_pred0_gt1", "one_pixel_pred0_gt0", "noise_1x70", "noise_70x1", "noise_2x65", "runs_33x33", "row_2p17_false_positive",
         "column_2p17_false_positive", "row_2p18_two_runs", "column_2p18_two_runs_tied", "big_squares", "big_last_pixel", "big_rectangle"]


@pytest.mark.parametrize("name", MASKS)
def test_the_box_of_thin_and_2_pow_24_pixel_masks(name):
    robot = robots.BboxRobot()
    pred, gt, _, _ = rc.get(name)
    for mask in (gt, pred, pred | gt):
        assert robot.interact_device(to_dev(mask)).cpu().tolist() == robots.host_bbox(mask).tolist()
    if name == "row_2p18_two_runs":
        assert robots.host_bbox(gt).tolist() == [1, 0, 0, (1 << 18) - 1, 0]            # a coordinate above 65535


def candidates(target, M):
    """M candidates: the target moved along both axes by different amounts - no two alike, the closest neither first nor last for M > 1 -
    and, second to last of eight, an empty one."""
    H, W = target.shape
    step_y, step_x = (0 if H == 1 else 37 if H > 256 else 1), (0 if W == 1 else 11 if W > 256 else 1)
    out = [np.roll(target, (k * step_y, k * step_x), (0, 1)) for k in (5, 3, 8, 1, 6, 2, 7, 4)[:M]]
    if M == 8:
        out[6] = np.zeros_like(target)
    return np.stack(out)


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("name", ["one_pixel_pred0_gt1", "noise_1x70", "noise_70x1", "noise_2x65", "row_2p17_false_positive", "column_2p18_two_runs",
                                  "big_rectangle"])
def test_best_mask_counts_and_fp32_iou_of_thin_and_2_pow_24_pixel_masks(name, M):
    pred, gt, _, _ = rc.get(name)
    target = pred if name == "row_2p17_false_positive" else gt          # the long run: counts of 2^17 - 1
    cands = candidates(target, M)
    iou, idx, counts = robots.host_best_mask(list(cands), target)
    t = to_dev(target)
    out = robots.best_mask_device(to_dev(cands), t).cpu().numpy()
    assert out[2:2 + 2 * M].reshape(-1, 2).tolist() == counts.tolist()
    assert int(out[0]) == idx
    assert out[1:2].view(np.float32)[0].tobytes() == np.float32(iou).tobytes()
    # the reference's shapes: candidates [M,1,H,W], target [1,1,H,W]
    assert robots.best_mask(to_dev(cands)[:, None].bool(), t[None, None].bool()) == (iou, idx)


def test_the_reference_style_calls_take_a_frame_of_one_row_and_of_one_column():
    robot, host, box = robots.ClickRobot(), robots.HostClickRobot(), robots.BboxRobot()
    for name in ("runs_1x70", "runs_70x1", "noise_1x70", "noise_70x1", "one_pixel_pred0_gt1"):
        pred, gt, _, iou = rc.get(name)
        p, g = to_dev(pred), to_dev(gt)
        want = host.interact(pred, gt, iou)
        for a, b in ((p, g), (p[None, None].bool(), g[None, None].float())):           # [1,W] as it is, and the reference's [1,1,1,W]
            clicks, labels = robot.interact(a, b, iou)
            assert clicks.tolist() == want[0].tolist() and labels.tolist() == want[1].tolist()
        assert robot.middle_click(g)[0].tolist() == host.middle_click(gt)[0].tolist()
        assert box.interact(g[None, None]).tolist() == robots.HostBboxRobot().interact(gt).tolist()


# ------------------------------------------------------------------------------------------------ the scratch is what the kernels write
SENTINEL = 0xA5
TAIL = 1 << 16


@pytest.mark.parametrize("name", ["one_pixel_pred0_gt1", "noise_37x53", "row_2p17_false_positive", "big_squares"])
def test_the_kernels_write_nothing_behind_the_scratch_they_ask_for(name):
    if name == "noise_37x53":                                   # odd H + W: the histograms end off a 16-byte boundary
        pred, gt, mode, iou = rc.noise(37, 53, 31)
        want = robots.host_click_record(pred, gt, mode, iou)[0].tolist()
    else:
        (pred, gt, mode, iou), want = rc.get(name), rc.host(name)[0]
    H, W = gt.shape
    need = robots.scratch_bytes(H, W)
    assert need == 256 + (4 * (H + W) + 15) // 16 * 16 + 8 * H * W
    big = torch.full((need + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    robot = robots.ClickRobot()
    p, g = to_dev(pred), to_dev(gt)
    robot._scratch[(H, W, g.device)] = big[:need]
    assert robot._scratch_for(H, W, g.device).data_ptr() == big.data_ptr()
    rec = robot.interact_device(p, g, iou).cpu().tolist()
    mid = robot.middle_click_device(g).cpu().tolist()
    assert bool((big[need:] == SENTINEL).all())
    assert not bool((big[:need] == SENTINEL).all())              # the calls did use this scratch
    assert rec == want
    assert mid == robots.host_click_record(None, gt, robots.MIDDLE)[0].tolist()
