"""The device robots (csrc/robot.hip behind stcn_robot_*) against the host restatement (eva_vos_amd.robots.host_*), which
tests/test_robot_api.py holds to the reference's own robot.  Every comparison is exact: records, components, counts, fp32 bits."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from eva_vos_amd import robots, synth

pytestmark = pytest.mark.gpu

GOLD = load_golden("robot_clicks")
CASES = sorted({k.rsplit(".", 1)[0] for k in GOLD})


def fixture_case(name):
    iou = float(GOLD[f"{name}.iou"])
    return GOLD[f"{name}.pred"], GOLD[f"{name}.gt"], int(GOLD[f"{name}.mode"]), None if np.isnan(iou) else iou


def noise_case(p, seed):
    g = np.random.default_rng(seed)
    return (g.random((64, 96)) < p).astype(np.uint8), (g.random((64, 96)) < p).astype(np.uint8), robots.INTERACT, None


def ellipse_case():
    m = synth.synthetic_mask(6, 480, 854, 1)[0, :, 0].numpy().astype(np.uint8)      # moving ellipses: frames 1 and 4 overlap partly
    return m[1], m[4], robots.INTERACT, None


OTHER = {"noise_0.5": lambda: noise_case(0.5, 11), "noise_0.1": lambda: noise_case(0.1, 12), "noise_0.1_iou": lambda: noise_case(0.1, 14)[:3] + (0.05,),
         "ellipses_480x854": ellipse_case}


def get_case(name):
    return OTHER[name]() if name in OTHER else fixture_case(name)


def device_record(robot, pred, gt, mode, iou, with_component=True):
    dev = torch.device("cuda:0")
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    comp = torch.full(g.shape, 7, dtype=torch.uint8, device=dev) if with_component and mode == robots.INTERACT else None
    rec = robot.middle_click_device(g) if mode == robots.MIDDLE else robot.interact_device(p, g, iou, component=comp)
    return rec.cpu().numpy(), None if comp is None else comp.cpu().numpy()


@pytest.mark.parametrize("name", CASES + sorted(OTHER))
def test_the_device_record_and_component_equal_the_host_restatement(name):
    pred, gt, mode, iou = get_case(name)
    want, want_comp = robots.host_click_record(pred, gt, mode, iou)
    got, got_comp = device_record(robots.ClickRobot(), pred, gt, mode, iou)
    assert got.tolist() == want.tolist()
    if got_comp is not None:
        assert np.array_equal(got_comp, want_comp)


def test_the_noise_masks_reach_ties_and_every_field():
    recs = [robots.host_click_record(*get_case(n))[0] for n in ("noise_0.5", "noise_0.1", "noise_0.1_iou")]
    assert all(r[robots.FP_COUNT] > 50 and r[robots.FN_COUNT] > 50 for r in recs[1:])
    assert recs[2][robots.N_CLICKS] == 2 and recs[2][robots.MOVED] == 1
    seen = np.stack(recs + [robots.host_click_record(*get_case(n))[0] for n in CASES]).any(0)
    assert seen[:robots.MOVED + 1].all()
    from scipy import ndimage
    pred, gt, _, _ = get_case("noise_0.1")
    sizes = np.bincount(ndimage.label(pred & ~gt & 1, structure=np.ones((3, 3), int))[0].ravel())[1:]
    assert (sizes == sizes.max()).sum() >= 1 and len(sizes) - len(set(sizes.tolist())) > 10      # many components of equal size


def test_the_reference_style_calls_return_the_references_values():
    dev = torch.device("cuda:0")
    robot, host = robots.ClickRobot(), robots.HostClickRobot()
    for name in ("blob_48x64", "two_clicks_37x53", "ring_48x64"):
        pred, gt, mode, iou = fixture_case(name)
        # the reference hands [1,1,H,W] tensors (bool or float) to its robot
        clicks, labels = robot.interact(torch.from_numpy(pred).to(dev)[None, None].bool(), torch.from_numpy(gt).to(dev)[None, None].float(), iou)
        assert clicks.tolist() == GOLD[f"{name}.clicks"].tolist() and labels.tolist() == GOLD[f"{name}.labels"].tolist()
        assert clicks.dtype == host.interact(pred, gt, iou)[0].dtype and clicks.shape == (len(labels), 2)
    pred, gt, _, _ = fixture_case("l_shape_middle_37x53")
    clicks, labels = robot.middle_click(torch.from_numpy(gt).to(dev))
    assert clicks.tolist() == GOLD["l_shape_middle_37x53.clicks"].tolist() and labels.tolist() == [1]
    with pytest.raises(ValueError):
        robot.middle_click(torch.zeros((20, 30), dtype=torch.uint8, device=dev))


def test_repeated_calls_on_one_stream_with_reused_scratch_give_identical_records():
    robot = robots.ClickRobot()
    names = ["noise_0.1", "spiral_48x64", "equal_48x64", "noise_0.5", "ring_48x64", "median_odd_48x64", "noise_0.1"]      # 64x96 and 48x64 scratch, reused
    first = [device_record(robot, *get_case(n))[0] for n in names]
    # enqueue everything again without a host wait in between, then read
    dev = torch.device("cuda:0")
    recs = []
    for n in names * 2:
        pred, gt, mode, iou = get_case(n)
        g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        recs.append(robot.middle_click_device(g) if mode == robots.MIDDLE else robot.interact_device(p, g, iou))
    got = torch.stack(recs).cpu().numpy()
    for i, n in enumerate(names * 2):
        assert got[i].tolist() == first[i % len(names)].tolist(), n
        assert got[i].tolist() == robots.host_click_record(*get_case(n))[0].tolist()


def test_bbox_is_the_min_and_max_of_the_object_and_an_empty_mask_is_reported():
    dev = torch.device("cuda:0")
    robot = robots.BboxRobot()
    for name in CASES + sorted(OTHER):
        _, gt, _, _ = get_case(name)
        assert robot.interact_device(torch.from_numpy(gt).to(dev)).cpu().numpy().tolist() == robots.host_bbox(gt).tolist(), name
    one = np.zeros((37, 53), np.uint8)
    one[36, 52] = 1
    assert robot.interact(torch.from_numpy(one).to(dev)[None, None]).tolist() == [[52.0, 36.0, 52.0, 36.0]]
    empty = torch.zeros((37, 53), dtype=torch.uint8, device=dev)
    assert robot.interact_device(empty).cpu().numpy().tolist() == [0, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        robot.interact(empty)


def test_best_mask_counts_fp32_iou_and_first_maximum():
    dev = torch.device("cuda:0")
    g = np.random.default_rng(5)
    target = np.zeros((37, 53), np.uint8)
    target[5:30, 8:40] = 1
    noisy = lambda p: (target ^ (g.random(target.shape) < p)).astype(np.uint8)      # noqa: E731
    a, b = noisy(0.2), noisy(0.05)
    sets = {
        "three": [a, b, noisy(0.4)],
        "duplicates": [a, b, b.copy(), a, b.copy()],                              # the first of the equal best wins
        "eight": [noisy(p) for p in (0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.02, 0.3)],
        "one_empty": [np.zeros_like(target)],
        "exact": [noisy(0.3), target.copy()],
    }
    for name, cands in sets.items():
        iou, idx, counts = robots.host_best_mask(cands, target)
        out = robots.best_mask_device(torch.from_numpy(np.stack(cands)).to(dev), torch.from_numpy(target).to(dev)).cpu().numpy()
        assert out[2:2 + 2 * len(cands)].reshape(-1, 2).tolist() == counts.tolist(), name
        assert int(out[0]) == idx, name
        assert out[1:2].view(np.float32)[0].tobytes() == np.float32(iou).tobytes(), name
        assert robots.best_mask(torch.from_numpy(np.stack(cands)).to(dev)[:, None].bool(), torch.from_numpy(target).to(dev)[None, None].bool()) == (iou, idx)
    assert robots.host_best_mask(sets["duplicates"], target)[1] == 1
    # both empty: (0 + 1e-6) / (0 + 1e-6) = 1, the reference's smoothing
    z = torch.zeros((1, 37, 53), dtype=torch.uint8, device=dev)
    assert robots.best_mask(z, z[0]) == (1.0, 0)
    # a large frame: counts beyond 2^16 per wave and block
    big_t = synth.synthetic_mask(6, 480, 854, 1)[0, :, 0].numpy().astype(np.uint8)
    iou, idx, counts = robots.host_best_mask([big_t[0], big_t[3], big_t[2]], big_t[2 + 1])
    out = robots.best_mask_device(torch.from_numpy(big_t[[0, 3, 2]].copy()).to(dev), torch.from_numpy(big_t[3]).to(dev)).cpu().numpy()
    assert out[2:8].reshape(-1, 2).tolist() == counts.tolist() and int(out[0]) == idx == 1
    assert out[1:2].view(np.float32)[0].tobytes() == np.float32(iou).tobytes()
