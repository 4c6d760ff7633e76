"""The annotation-type dataset driver on the GPU: the export kernel (stcn_frames_to_rgb8 behind annot_driver.frames_to_rgb8) against the NumPy
statement of what the reference stores, byte for byte, at the smallest shapes where it can go wrong, and the driver end to end through
``annot_driver.run`` against ``eval_driver.run_typed_policy('oracle_oracle', metric='j')`` on the same samples."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from eva_vos_amd import _lib, annot_driver, eval_driver, fq_driver, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "annot_export.npz")
CANARY = 64


def _clip(T, H, W, seed):
    g = np.random.Generator(np.random.Philox(key=[seed, 256]))
    return g.normal(0, 1.2, (T, 3, H, W)).astype(np.float32)


def _check(clip, frames=None):
    got = annot_driver.frames_to_rgb8(torch.from_numpy(clip).cuda(), frames)
    ref = annot_driver.frames_to_rgb8_host(clip, frames)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == ref.shape
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    return ref


def _raw(clip_dev, frames_dev, n, scratch, out):
    T, _, H, W = clip_dev.shape
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    return _lib.lib().stcn_frames_to_rgb8(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(clip_dev), T, H, W, ptr(frames_dev), n, ptr(scratch), ptr(out))


# ------------------------------------------------------------------------------------------------ the kernel
# (T, H, W).  Pass 1 reads a frame as up to 3 head floats, float4s from its first 16-byte boundary, up to 3 tail floats; a wave takes 256
# floats of the body per load, a workgroup 4096.  3 * H * W is a multiple of 3, so the frames of a clip start at every offset mod 4 and the
# body of a later frame is N - head: with N = 258 frame 1 has a body of exactly one wave (256), with N = 4098 of exactly one workgroup
# (4096), with N = 8193 frame 1 has 8190 = two workgroups - 2 and frame 3 exactly two (8192); N = 4095 / 4101 and 8190 / 8196 lie on either side.
# W = 5, 7, 9: the tails of pass 2's runs of four pixels and rows that start at every alignment.
SHAPES = [(1, 1, 1), (2, 1, 3), (2, 5, 5), (3, 5, 7), (2, 3, 9), (4, 5, 17), (4, 2, 43), (4, 15, 91), (4, 2, 683), (4, 1, 1367), (4, 30, 91), (4, 1, 2731),
          (2, 4, 683)]


@pytest.mark.parametrize("T,H,W", SHAPES)
def test_the_kernel_equals_the_host_restatement_at_small_and_seam_shapes(T, H, W):
    _check(_clip(T, H, W, seed=T * H * W))
    _check(_clip(T, H, W, seed=7)[::-1].copy(), [T - 1])


def test_a_constant_frame_is_all_zero_and_a_clip_of_them_too():
    clip = np.full((2, 3, 6, 5), 0.375, np.float32)
    clip[1] = -2.5
    assert int(_check(clip).max()) == 0


# where the minimum and the maximum sit in the flattened [3,H,W] frame (negative: from the end): first / last element, different channels, the
# scalar tail and head of a frame that starts off a 16-byte boundary
EXTREMA = [(0, -1), (-1, 0), (0, 1), (-2, -1), (-3, -2), (40, 2 * 35 + 1), (2 * 35 + 34, 3), (1, -1)]


@pytest.mark.parametrize("i_min,i_max", EXTREMA)
def test_the_extrema_are_found_wherever_they_sit(i_min, i_max):
    T, H, W = 3, 5, 7                                            # N = 105: frames start at offsets 0, 1, 2 mod 4
    g = np.random.Generator(np.random.Philox(key=[i_min % 97, i_max % 89]))
    clip = g.uniform(-1, 1, (T, 3, H, W)).astype(np.float32)
    flat = clip.reshape(T, -1)
    flat[:, i_min], flat[:, i_max] = -5.0, 7.0
    ref = _check(clip).reshape(T, -1, 3)
    n = H * W
    pix = lambda i: ((i % (3 * n)) % n, (i % (3 * n)) // n)      # noqa: E731   flat index -> (pixel, channel)
    assert all(ref[t][pix(i_max)] == 255 and ref[t][pix(i_min)] == 0 for t in range(T))


def test_all_negative_values_and_the_exact_255():
    clip = -np.abs(_clip(2, 6, 10, seed=5)) - 0.5
    ref = _check(clip)
    assert int(ref.min()) == 0 and int(ref.max()) == 255
    for t in range(2):                                           # the maximum pixel comes out as exactly 255: (max - min) / (max - min) * 255
        hwc = clip[t].transpose(1, 2, 0)
        assert (ref[t][hwc == hwc.max()] == 255).all() and (ref[t][hwc == hwc.min()] == 0).all()


def test_frames_with_repeats_descending_and_none():
    clip = _clip(4, 6, 7, seed=11)
    for frames in ([3, 1, 1, 0], [3, 2, 1, 0], [2], [1, 2], None, [0, 0, 0]):
        ref = _check(clip, frames)
        assert len(ref) == (4 if frames is None else len(frames))


def test_no_frames_is_a_no_op():
    clip = torch.from_numpy(_clip(2, 4, 4, seed=1)).cuda()
    out = annot_driver.frames_to_rgb8(clip, [])
    assert tuple(out.shape) == (0, 4, 4, 3) and out.dtype == torch.uint8
    buf = torch.full((CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = torch.full((CANARY // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _raw(clip, None, 0, scratch, buf) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()) and bool((scratch == 0x5A5A5A5A).all())


@pytest.mark.parametrize("T,H,W,frames", [(3, 6, 7, [2, 0, 2, 1]), (2, 8, 8, None), (1, 5, 9, None)])
def test_a_misaligned_output_and_the_canaries_behind_out_and_scratch(T, H, W, frames):
    clip = _clip(T, H, W, seed=3)
    n = T if frames is None else len(frames)
    size = n * H * W * 3
    for shift in (0, 1, 2, 3):
        buf = torch.full((shift + size + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        scratch = torch.full((2 * n + CANARY // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        idx = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
        assert _raw(torch.from_numpy(clip).cuda(), idx, n, scratch, buf[shift:]) == 0
        torch.cuda.synchronize()
        ref = annot_driver.frames_to_rgb8_host(clip, frames)
        assert torch.equal(buf[shift:shift + size].cpu(), torch.from_numpy(ref).flatten()), shift
        assert bool((buf[:shift] == 0xA5).all()) and bool((buf[shift + size:] == 0xA5).all()) and bool((scratch[2 * n:] == 0x5A5A5A5A).all()), shift


def test_a_480p_clip_of_three_frames():
    clip = synth.synthetic_clip(3, 480, 854)[0].numpy()
    ref = _check(clip)
    assert ref.shape == (3, 480, 854, 3) and int(ref.min()) == 0 and int(ref.max()) == 255
    _check(clip, [2, 0])


def test_the_golden_cases_through_the_kernel():
    g = np.load(GOLD)
    names = sorted({k.split(".")[0] for k in g.files})
    assert len(names) >= 5
    for name in names:
        got = annot_driver.frames_to_rgb8(torch.from_numpy(g[f"{name}.frame"]).cuda())
        assert torch.equal(got[0].cpu(), torch.from_numpy(g[f"{name}.rgb8"])), name


def test_a_frame_outside_the_clip_is_refused_by_the_wrapper_and_zeros_from_the_kernel():
    clip = _clip(3, 6, 7, seed=9)
    dev = torch.from_numpy(clip).cuda()
    for frames in ([3], [-1, 0], [0, 1, 7]):
        with pytest.raises(ValueError, match="frames"):
            annot_driver.frames_to_rgb8(dev, frames)
    frames = [1, 3, -1, 2]                                        # the C entry reads nothing of frames 3 and -1 and writes zeros for them
    out = torch.full((4, 6, 7, 3), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = torch.empty((4, 2), dtype=torch.int32, device="cuda")
    assert _raw(dev, torch.tensor(frames, dtype=torch.int32, device="cuda"), 4, scratch, out) == 0
    ref = annot_driver.frames_to_rgb8_host(clip, [1, 2])
    assert torch.equal(out[[0, 3]].cpu(), torch.from_numpy(ref)) and int(out[[1, 2]].max()) == 0


# ------------------------------------------------------------------------------------------------ the driver
def _files(out):
    return {os.path.join(sub, f): open(os.path.join(out, sub, f), "rb").read() for sub in ("Images", "Masks", "SAM_Embeddings") for f in sorted(os.listdir(os.path.join(out, sub)))}


def test_the_driver_end_to_end_against_the_oracle_oracle_session(nets, tmp_path):
    """2 videos, two objects in one of them, 8 frames, 4 rounds, the ``nets`` fixture.  Frames of 112 x 128, not 96 x 112: the fixture's networks
    read top_k = 50 rows of the memory bank and the engine refuses a frame with fewer 1/16-scale positions than that (96 x 112 has 42;
    112 x 128, with 56, is what test_gpu_eva_vos runs its driver on)."""
    from mivos.inference_core import InferenceCore
    root, rounds = str(tmp_path / "db"), 4
    imset = fq_driver.make_synthetic_tree(root, {"v0": (8, 112, 128, 2), "v1": (8, 112, 128, 1)})
    outs = [str(tmp_path / f"annot_{lanes}") for lanes in (1, 2)]
    stats = {}
    for lanes, out in zip((1, 2), outs):
        rows = annot_driver.run(root, imset, out, nets[0], nets[1], rounds=rounds, annotator="component", lanes=lanes, stats=stats if lanes == 1 else None)
    csvs = [open(os.path.join(out, "synthetic.csv"), "rb").read() for out in outs]
    assert csvs[0] == csvs[1] and _files(outs[0]) == _files(outs[1])                 # rows and files do not depend on the lanes
    with open(os.path.join(outs[0], "synthetic.csv"), newline="") as f:
        lines = list(csv.DictReader(f))
    print(lines, stats)
    assert list(lines[0]) == annot_driver.csv_header() and len(lines) == len(rows) == 3 * (rounds - 1)
    ids = [ln["id"] for ln in lines]
    assert [ln["video_name"] for ln in lines] == [n for n in ("v0__1", "v0__2", "v1__1") for _ in range(rounds - 1)]
    assert [int(ln["round"]) for ln in lines] == list(range(2, rounds + 1)) * 3
    for sub, ext in (("Images", ".png"), ("Masks", ".png"), ("SAM_Embeddings", ".npy")):
        assert sorted(os.listdir(os.path.join(outs[0], sub))) == sorted(i + ext for i in ids)
    ds = fq_driver.ClipDataset(root, imset)
    for i in range(len(ds)):
        sample = ds[i]
        mine = [ln for ln in lines if ln["video_name"] == sample["name"]]
        proc = InferenceCore(nets[0], nets[1], sample["rgb"].cuda(), 1)
        ref = eval_driver.run_typed_policy("oracle_oracle", proc, sample, rounds, eval_driver.make_annotator("component"), ["3clicks", "mask"], metric="j")
        assert [int(ln["frame_num"]) for ln in mine] == ref["annotated_frames"][1:] and [ln["selected_annotation"] for ln in mine] == ref["annotations_actions"][1:]
        cost = np.zeros(sample["num_frames"])
        cost[0] = 80
        for k, ln in enumerate(mine):
            frame, r = int(ln["frame_num"]), int(ln["round"])
            assert ln["id"] == f"{sample['name']}_{r}_frame_{frame}"
            assert float(ln["init_iou"]) == float(ref["round_metrics"][k][frame])                # the quality after round r - 1, to the bit
            data = ref["action_data"][k]
            assert float(ln["3clicks_iou"]) == float(data["3clicks"]["iou"]) and float(ln["mask_iou"]) == float(data["mask"]["iou"]) == 1.0
            cost[frame] += ref["annotation_times"][k + 1]
            assert float(ln["frame_cost"]) == cost[frame] and float(ln["video_cost"]) == cost.sum()
            image = np.asarray(Image.open(os.path.join(outs[0], "Images", ln["id"] + ".png")))
            assert np.array_equal(image, annot_driver.frames_to_rgb8_host(sample["rgb"][0], [frame])[0])
            mask = np.asarray(Image.open(os.path.join(outs[0], "Masks", ln["id"] + ".png")))
            assert mask.ndim == 2 and mask.dtype == np.uint8 and set(np.unique(mask).tolist()) <= {0, 255}
            if ln["selected_annotation"] == "mask":
                assert np.array_equal(mask, (sample["gt"][0, frame, 0].numpy() > 0.5).astype(np.uint8) * 255)
            emb = np.load(os.path.join(outs[0], "SAM_Embeddings", ln["id"] + ".npy"))
            assert emb.shape == (256, 64, 64) and emb.dtype == np.float32 and np.isfinite(emb).all()
