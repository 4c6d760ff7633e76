"""Click fixtures captured from the REAL reference robot (build container only) -> tests/golden/robot_clicks.npz.

The reference's ``robots/click_robot.py`` imports ``skimage.measure.label``, which the build container does not have.  This tool defines the
stand-in itself, on ``scipy.ndimage.label`` with a structure of ones (= ``connectivity=2``), and imports the reference's ``ClickRobot``
under it.  What the stand-in ASSUMES of skimage: components are numbered in raster order of their first pixels (true of scipy; DESIGN.md
section 7 says so).  Everything else - the bincount / argmax selection, the centroids, the nearest-pixel fallback, the tie between the two
regions, the iou branch, the middle click - is the reference's own code running.

Per case ``<name>``: ``.pred`` / ``.gt`` uint8 [H,W], ``.mode`` (0 = interact, 1 = middle_click), ``.iou`` (NaN = not given),
``.clicks`` int64 [n,2] and ``.labels`` int64 [n] as the reference returned them.  tests/test_robot_api.py holds the host restatement to
them; tests/test_gpu_robot.py holds the device robot to the host restatement on the same masks.

Run:  python tools/gen_golden_robot.py --reference=<checkout of the reference>
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _rect(m, y0, y1, x0, x1, v=1):
    m[max(y0, 0):y1, max(x0, 0):x1] = v


def _spiral(H, W):
    """A one-pixel-wide rectangular spiral with one-pixel gaps: one component whose pixels are a single long path."""
    m = np.zeros((H, W), np.uint8)
    y0, y1, x0, x1 = 1, H - 2, 1, W - 2
    y, x = y0, x0
    while y1 - y0 >= 2 and x1 - x0 >= 2:
        m[y0, x0:x1 + 1] = 1                       # top, left to right
        m[y0:y1 + 1, x1] = 1                       # right, down
        m[y1, x0 + 2:x1 + 1] = 1                   # bottom, back to x0 + 2
        m[y0 + 2:y1 + 1, x0 + 2] = 1               # up to the next ring's start
        y0, y1, x0, x1 = y0 + 2, y1 - 2, x0 + 2, x1 - 2
        if y1 >= y0 and x1 >= x0:
            m[y0, x0] = 1
    return m


def cases(H, W):
    """name -> (pred, gt, mode, iou) at H x W.  48 x 64 and 37 x 53 divide no 32 x 32 tile."""
    z = lambda: np.zeros((H, W), np.uint8)         # noqa: E731
    out = {}
    cy, cx = H // 2, W // 2

    gt, pr = z(), z()                              # one blob each, shifted: a false positive and a false negative of different sizes
    _rect(gt, 8, 26, 10, 34); _rect(pr, 12, 31, 16, 38)
    out["blob"] = (pr, gt, 0, None)

    gt = z()                                       # a cross through the whole frame: one component over every tile border
    gt[cy - 1:cy + 1, :] = 1; gt[:, cx - 1:cx + 1] = 1
    out["crossing"] = (z(), gt, 0, None)

    out["spiral"] = (z(), _spiral(H, W), 0, None)  # worst case for label propagation
    out["spiral_fp"] = (_spiral(H, W), z(), 0, None)

    gt = z()                                       # two squares that touch at a corner only (18 pixels together) beside one of 12
    _rect(gt, 5, 8, 5, 8); _rect(gt, 8, 11, 8, 11); _rect(gt, 20, 23, 30, 34)
    out["diagonal"] = (z(), gt, 0, None)

    gt, pr = z(), z()                              # two equal false-positive squares: the raster-first wins
    _rect(gt, 14, 24, 20, 32); pr[:] = gt
    _rect(pr, 4, 8, 40, 44); _rect(pr, 28, 32, 4, 8)
    out["equal_fp"] = (pr, gt, 0, None)

    gt, pr = z(), z()                              # equal largest false positive and false negative: the negative click wins
    _rect(gt, 14, 24, 20, 32); pr[:] = gt
    _rect(gt, 3, 7, 3, 7); _rect(pr, 28, 32, 40, 44)
    out["equal_fp_fn"] = (pr, gt, 0, None)

    yy, xx = np.mgrid[:H, :W]                       # a ring: the centroid falls into the hole, several object pixels are equally near
    d2 = (yy - cy) ** 2 + (xx - cx) ** 2
    out["ring"] = (z(), ((d2 >= 36) & (d2 <= 81)).astype(np.uint8), 0, None)

    gt = z()                                       # components on the frame border and in its corners
    _rect(gt, 0, 4, W - 7, W); _rect(gt, H - 3, H, 0, 5)
    out["border"] = (z(), gt, 0, None)

    gt = z(); _rect(gt, 9, 20, 11, 30)             # no error: the middle click (11 x 19 pixels: odd)
    out["equal"] = (gt.copy(), gt, 0, None)
    out["empty_pred"] = (z(), gt.copy(), 0, None)
    gt = z(); _rect(gt, 10, 14, 20, 26)            # 4 x 6: an even count, the medians are means of two values
    out["median_even"] = (gt.copy(), gt, 0, None)
    gt = z(); _rect(gt, 10, 13, 20, 25)
    out["median_odd"] = (gt.copy(), gt, 1, None)

    gt = z()                                       # an L turned by 45 degrees: the medians meet between its arms, outside the object
    for k in range(13):
        gt[cy + k:cy + k + 2, 6 + k] = 1; gt[cy - k - 1:cy - k + 1, 6 + k] = 1
    out["l_shape"] = (gt.copy(), gt, 0, None)
    out["l_shape_middle"] = (z(), gt.copy(), 1, None)

    gt, pr = z(), z()                              # the mask sits on another object: iou < 0.1 gives the negative and the positive click
    _rect(gt, 5, 15, 5, 20); _rect(pr, 20, 34, 30, 50)
    out["two_clicks"] = (pr, gt, 0, 0.0)
    out["two_clicks_high_iou"] = (pr.copy(), gt.copy(), 0, 0.5)
    return out


def all_cases():
    out = {}
    for H, W in ((48, 64), (37, 53)):
        for name, c in cases(H, W).items():
            out[f"{name}_{H}x{W}"] = c
    return out


def import_reference_robot(reference):
    from scipy import ndimage

    def label(mask, connectivity=2, return_num=False):
        assert connectivity == 2 and mask.ndim == 2
        lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
        return (lab, n) if return_num else lab

    skimage, measure = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    measure.label, skimage.measure = label, measure
    sys.modules["skimage"], sys.modules["skimage.measure"] = skimage, measure
    sys.path.insert(0, reference)
    from robots.click_robot import ClickRobot
    assert os.path.abspath(reference) in os.path.abspath(sys.modules["robots.click_robot"].__file__)
    return ClickRobot()


def main():
    import torch
    ref = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--reference=")] or [os.environ.get("EVA_VOS_REFERENCE", "")]
    if not ref[0] or not os.path.isdir(ref[0]):
        sys.exit("give the checkout of the reference: --reference=PATH (or EVA_VOS_REFERENCE)")
    robot = import_reference_robot(ref[0])
    out = {}
    for name, (pred, gt, mode, iou) in all_cases().items():
        g, p = torch.from_numpy(gt)[None, None], torch.from_numpy(pred)[None, None]
        clicks, labels = robot.middle_click(g) if mode == 1 else robot.interact(p, g, iou)
        out[f"{name}.pred"], out[f"{name}.gt"] = pred, gt
        out[f"{name}.mode"], out[f"{name}.iou"] = np.array(mode), np.array(np.nan if iou is None else iou)
        out[f"{name}.clicks"], out[f"{name}.labels"] = np.asarray(clicks, np.int64).reshape(-1, 2), np.asarray(labels, np.int64).reshape(-1)
        print(name, out[f"{name}.clicks"].tolist(), out[f"{name}.labels"].tolist(), flush=True)
    path = os.path.join(GOLD, "robot_clicks.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(all_cases())} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
