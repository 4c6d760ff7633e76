"""Stored-image fixtures captured from the REAL reference helpers (build container only) -> tests/golden/annot_export.npz.

Runs the reference's own ``tens2image`` and ``im_normalize`` (datasets/helpers.py:4-17) and the ``* 255 -> uint8`` step of its driver
(generate_annotation_dataset.py:170-172) over a handful of small fp32 frames.  ``datasets/helpers.py`` is loaded by its path - the package's
``__init__`` pulls in the whole training stack - and it imports ``matplotlib.pyplot`` for its plotting helpers, which the build container may
not have: an empty stand-in module is registered then; nothing of it runs.

Per case ``<name>``: ``.frame`` fp32 [1,3,H,W] as the driver hands it over (``images[:, frame]``), ``.rgb8`` uint8 [H,W,3] as the reference
stored it.  Frames are at least 2 x 2: ``tens2image`` squeezes, so the reference itself has no HWC image for H = 1 or W = 1.
tests/test_annot_dataset_api.py holds ``annot_driver.frames_to_rgb8_host`` to them, tests/test_gpu_annot_dataset.py the kernel.

Run:  python tools/gen_golden_annot.py --reference=<checkout of the reference>
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def cases():
    """name -> fp32 [1,3,H,W].  Philox streams, so the frames do not depend on the NumPy version's legacy generator."""
    g = np.random.Generator(np.random.Philox(key=[23, 256]))
    out = {}
    out["random"] = g.normal(0, 1.2, (1, 3, 13, 17)).astype(np.float32)                       # what an ImageNet-normalised frame looks like
    out["random_odd"] = g.uniform(-2.2, 2.7, (1, 3, 7, 9)).astype(np.float32)
    out["constant"] = np.full((1, 3, 6, 5), 0.375, np.float32)                                # max - min = 0: the divisor is 1e-8, all zero
    spike = np.full((1, 3, 5, 7), -1.5, np.float32)                                           # a single pixel above a constant frame
    spike[0, 1, 2, 3] = 2.25
    out["single_pixel"] = spike
    out["all_negative"] = (-g.uniform(0.5, 3.0, (1, 3, 8, 6))).astype(np.float32)
    split = g.uniform(-1, 1, (1, 3, 6, 10)).astype(np.float32)                                # min in the last channel, max in the first
    split[0, 2, 5, 9], split[0, 0, 0, 0] = -4.0, 5.0
    out["min_max_channels"] = split
    tiny = (g.uniform(0, 1, (1, 3, 4, 4)) * 3e-9).astype(np.float32)                          # a range below 1e-8: the floor of the divisor
    out["tiny_range"] = tiny
    steps = (np.arange(3 * 16 * 16, dtype=np.float32).reshape(1, 3, 16, 16) / 767 * 2 - 1)    # a ramp: every byte value is met near its edge
    out["ramp"] = steps.astype(np.float32)
    return out


def import_reference_helpers(reference):
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mpl, plt = types.ModuleType("matplotlib"), types.ModuleType("matplotlib.pyplot")
        mpl.pyplot = plt
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, plt
    path = os.path.join(reference, "datasets", "helpers.py")
    spec = importlib.util.spec_from_file_location("reference_datasets_helpers", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.abspath(reference) in os.path.abspath(mod.__file__)
    return mod


def main():
    import torch
    ref = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--reference=")] or [os.environ.get("EVA_VOS_REFERENCE", "")]
    if not ref[0] or not os.path.isdir(ref[0]):
        sys.exit("give the checkout of the reference: --reference=PATH (or EVA_VOS_REFERENCE)")
    helpers = import_reference_helpers(ref[0])
    out = {}
    for name, frame in cases().items():
        rgb_frame = torch.from_numpy(frame.copy())                                            # deepcopy(images[:, frame]).cpu()
        rgb_img = helpers.im_normalize(helpers.tens2image(rgb_frame))
        canvas = (rgb_img * 255).astype(np.uint8)
        assert canvas.shape == frame.shape[2:] + (3,), (name, canvas.shape)
        out[f"{name}.frame"], out[f"{name}.rgb8"] = frame, canvas
        print(name, frame.shape, "min", float(frame.min()), "max", float(frame.max()), "bytes", int(canvas.min()), "..", int(canvas.max()), flush=True)
    path = os.path.join(GOLD, "annot_export.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(cases())} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
