"""Annotation-type dataset generation on the HIP engine: the AnnotDB the reference's ``AnnotTypeDB`` reads to train the annotation-type agent.

Own counterpart of the reference driver ``generate_annotation_dataset.py:79-182``: per (video, object) an ``oracle_oracle`` session over
``['3clicks', 'mask']`` scored by J - round 1 is the mask of frame 0, every later round annotates the worst frame with the action of the best
reward (``eval_driver.oracle_action``) - and per round r > 1 one CSV row plus three files: the frame as an 8-bit RGB image, the evaluated mask
of the frame after the round, the segmenter's image embedding.  The session is ``sessions.annotation_session`` with the two stop-rule details
of this loop (:108-110: the quality rule at every round, no ``not_avail_frames`` skip); dataset, ranks, lanes and the PNG writers are
``fq_driver``'s, annotators ``eval_driver``'s.

Differences by design:

* the images are made on the device: ONE ``stcn_frames_to_rgb8`` call per session turns the frames of all its rows into uint8 [n,H,W,3]
  (per-frame min / max, normalise, x 255, truncate, HWC - ``im_normalize(tens2image(.))`` byte for byte); a quarter of the fp32 bytes crosses
  PCIe, once per session, into pinned memory, and host threads encode the PNGs while the GPU runs the next session;
* J per frame, the click robot and the best-of-three stay on the device, as in ``eval_driver``;
* the embedding is asked of the annotator AFTER the action, as the reference does, but for the frame of the row: where the action set no image
  (only 'mask' was tried, or the frame has no object) the reference stores whatever an earlier frame left in the predictor; here the frame is
  set then (``PromptAnnotator.image_embedding(reuse=True)``: no second encoder pass where the action did set it);
* rows are gathered once at the end (fixed-width fp32 rows; the fp64 values travel as four 16-bit pieces each, so the CSV prints them exactly).

Kept quirk: ``Masks/<id>.png`` is the EVALUATED mask of the frame after the round (``gen_masks[frame]`` after ``eval_processor_metric``,
generate_annotation_dataset.py:144,163): the ground truth for a 'mask' action, the annotator's mask otherwise - not the propagated mask the
action was chosen on.

Usage:  python -m eva_vos_amd.annot_driver --root data/MOSE --imset data/MOSE/ImageSets/subset_train_1.txt --out AnnotDB
        (multi-GPU: python -m torch.distributed.run --nproc-per-node N -m eva_vos_amd.annot_driver ...)
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import os
import threading
import time

import numpy as np
import torch

from . import _lib
from .eval_driver import ANNOTATORS, ARGUMENTS, _one_object_session, make_annotator, oracle_action
from .fq_driver import ClipDataset, add_stats, gather_sorted, lane_cores, load_networks, rank_samples, report_and_leave, run_lanes, write_png
from .sessions import SessionPolicy, annotation_session

DEFAULT_TYPES = ("3clicks", "mask")                             # generate_annotation_dataset.py:78
COLUMNS = ("id", "frame_cost", "video_cost", "selected_annotation", "frame_num", "round", "video_name", "init_iou")     # :64-77, then <type>_iou


def csv_header(annotation_types=DEFAULT_TYPES) -> list:
    """The reference's columns, in its order (generate_annotation_dataset.py:64-77)."""
    return list(COLUMNS) + [f"{t}_iou" for t in annotation_types]


# ------------------------------------------------------------------------------------------------ frames as stored images
def _frame_list(frames, T: int, who: str) -> list:
    frames = list(range(T)) if frames is None else [int(f) for f in frames]
    if frames and (min(frames) < 0 or max(frames) >= T):
        raise ValueError(f"{who}: frames {frames} of a clip of {T}")
    return frames


def frames_to_rgb8_host(clip, frames=None) -> np.ndarray:
    """The NumPy statement of what the reference stores of a frame (datasets/helpers.py:4-17, generate_annotation_dataset.py:170-174):
    ``(im_normalize(tens2image(frame)) * 255).astype(uint8)`` - the minimum and maximum over the whole [3,H,W] frame, (x - min) /
    max(max - min, 1e-8) * 255 in fp32, truncated, HWC.  clip: fp32 [T,3,H,W] (array or tensor) -> uint8 [n,H,W,3]."""
    a = clip.detach().cpu().numpy() if hasattr(clip, "detach") else np.asarray(clip)
    if a.dtype != np.float32 or a.ndim != 4 or a.shape[1] != 3:
        raise ValueError(f"frames_to_rgb8_host takes float32 [T,3,H,W], got {a.dtype} {a.shape}")
    frames = _frame_list(frames, a.shape[0], "frames_to_rgb8_host")
    out = np.empty((len(frames),) + a.shape[2:] + (3,), np.uint8)
    for i, f in enumerate(frames):
        im = a[f].transpose((1, 2, 0))
        lo = im.min()
        d = max(np.float32(im.max() - lo), np.float32(1e-8))
        out[i] = ((im - lo) / d * np.float32(255)).astype(np.uint8)
    return out


def frames_to_rgb8(clip: torch.Tensor, frames=None) -> torch.Tensor:
    """clip: fp32 [T,3,H,W] on the device (finite values) -> uint8 [n,H,W,3] on that device, equal to ``frames_to_rgb8_host`` byte for byte.
    ``frames``: the frames to take, in order, repeats allowed (None: all T); an index outside the clip raises ValueError.  One C call
    (``stcn_frames_to_rgb8``: three launches for all n frames) on the current stream, no sync; torch allocates the output and the scratch."""
    if clip.dtype != torch.float32 or clip.dim() != 4 or clip.shape[1] != 3 or not clip.is_cuda:
        raise ValueError(f"frames_to_rgb8 takes float32 [T,3,H,W] on the device, got {clip.dtype} {tuple(clip.shape)} on {clip.device}")
    clip = clip.contiguous()
    T, _, H, W = (int(v) for v in clip.shape)
    frames = _frame_list(frames, T, "frames_to_rgb8")
    n = len(frames)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=clip.device)
    if n == 0:
        return out
    idx = None
    if frames == list(range(frames[0], frames[0] + n)):            # a run of frames: a view, no index upload
        clip, T = clip[frames[0]:frames[0] + n], n
    else:
        idx = torch.tensor(frames, dtype=torch.int32).to(clip.device, non_blocking=True)
    scratch = torch.empty((n, 2), dtype=torch.int32, device=clip.device)
    with torch.cuda.device(clip.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().stcn_frames_to_rgb8(stream, C.c_void_p(clip.data_ptr()), T, H, W, C.c_void_p(idx.data_ptr()) if idx is not None else None, n,
                                                  C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr())), "stcn_frames_to_rgb8")
    return out


# ------------------------------------------------------------------------------------------------ the session
def run_annotation_dataset(processor, sample, rounds: int, annotator, annotation_types=DEFAULT_TYPES, stats: dict = None, scorer=None) -> dict:
    """One sample through the session of generate_annotation_dataset.py:89-178: ``oracle_oracle`` over ``annotation_types``, metric J, with
    ``stop_when_perfect`` and without the ``not_avail_frames`` skip.  ``annotator``: an ``annotate.PromptAnnotator`` whose predictor gives an
    image embedding; ``scorer``: another evaluation with ``TypedRoundScorer``'s interface.  A per-video sample is refused.
    Returns dict(rows, masks, embeddings, frames, annotated_frames, annotations_actions, annotation_times, round_metrics):
    ``rows``: one dict per round r > 1 that ran, keyed by ``csv_header(annotation_types)`` - ``frame_cost`` / ``video_cost`` the seconds spent
    on the frame / the video so far, ``init_iou`` the previous round's quality at the frame (from the scorer's rows, fetched once, at the
    end), ``<type>_iou`` what ``oracle_action`` measured for the type (NaN for a box it skipped);
    ``masks``: uint8 [n,H,W] on the device, row i's frame as the round evaluated it (copied out of the round's ``gen``: the scorer reuses it);
    ``embeddings``: [n,256,64,64] on the device, the annotator's embedding of row i's frame after the action (None when n = 0);
    ``frames``: row i's frame, for the export of the images (``frames_to_rgb8``)."""
    from .annotate import check_annotation_types
    types_ = check_annotation_types(annotation_types)
    T, gt, images, scorer = _one_object_session("annot_driver", processor, sample, rounds, "j", scorer)
    empty = scorer.empty_host
    data, embeddings, masks = [], [], []

    def action(frame, gen, frame_annots):
        g, im = gt[frame, 0], images[frame]
        out = oracle_action(annotator, types_, g, gen[frame][None].to(torch.bool), im, frame_annots, empty=bool(empty[frame]))
        data.append(out[-1])
        e = annotator.image_embedding(im, g, reuse=True)         # as the annotator stands after the action (:120)
        embeddings.append(e.reshape(e.shape[-3:]))
        return out[:-1]

    def choose_frame(worst, types, gen, frames):
        if len(frames) > 1:                                        # a round r > 1: its frame as it was evaluated (:163)
            masks.append(gen[frames[-1]].clone())
        return worst

    session = SessionPolicy(lambda f: gt[f][None], choose_frame, action=action, stop_at_T=False, stop_when_perfect=True, check_available=False)
    ses = annotation_session(processor, scorer, T, rounds, session, {} if stats is None else stats)
    q = scorer.qualities() if ses["costs"] else None
    name = sample["name"]
    frame_cost, rows = np.zeros(T), []
    for i, (frame, cost, act) in enumerate(zip(ses["frames"], ses["costs"], ses["actions"])):
        frame_cost[frame] += cost
        if i == 0:
            continue
        r = i + 1                                                  # rounds are skipped at the end of a session only
        row = dict(id=f"{name}_{r}_frame_{frame}", frame_cost=float(frame_cost[frame]), video_cost=float(frame_cost.sum()), selected_annotation=act,
                   frame_num=int(frame), round=r, video_name=name, init_iou=float(q[i - 1][frame]))
        for t in types_:
            row[f"{t}_iou"] = float(data[i - 1][t]["iou"]) if t in data[i - 1] else float("nan")
        rows.append(row)
    n = len(rows)
    return dict(rows=rows, masks=torch.stack(masks[:n]) if n else torch.zeros((0,) + tuple(gt.shape[-2:]), dtype=torch.uint8, device=gt.device),
                embeddings=torch.stack(embeddings[:n]) if n else None, frames=[row["frame_num"] for row in rows],
                annotated_frames=ses["frames"], annotations_actions=ses["actions"], annotation_times=ses["costs"],
                round_metrics=[q[i].copy() for i in range(len(ses["costs"]))], propagated_frames=ses["propagated_frames"])


# ------------------------------------------------------------------------------------------------ output
def _pack64(x: float) -> np.ndarray:
    """An fp64 value as four fp32 numbers - its 16-bit pieces, each exact in fp32 - for the fixed-width fp32 rows the ranks gather."""
    return np.array([x], np.float64).view(np.uint16).astype(np.float32)


def _unpack64(v) -> float:
    return float(np.asarray(v, np.float32).astype(np.uint16).view(np.float64)[0])


def _export(res: dict, clip: torch.Tensor, out: str, writers):
    """The files of a session's rows: ONE ``frames_to_rgb8`` call for the images, masks x 255, the embeddings; one copy each into pinned
    memory on the current stream, then a writer thread waits for the copies (an event) and writes ``Images/<id>.png`` (RGB), ``Masks/<id>.png``
    (2-D, 0 / 255) and ``SAM_Embeddings/<id>.npy``.  Returns the writer's future, or None for a session without rows."""
    ids = [row["id"] for row in res["rows"]]
    if not ids:
        return None
    dev = [frames_to_rgb8(clip, res["frames"]), res["masks"] * 255, res["embeddings"].float().contiguous()]
    host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in dev]
    for h, t in zip(host, dev):
        h.copy_(t, non_blocking=True)
    ready = torch.cuda.Event(blocking=True)
    ready.record()
    images, masks, embeddings = (h.numpy() for h in host)

    def write():
        ready.synchronize()
        for i, sid in enumerate(ids):
            write_png(os.path.join(out, "Images", f"{sid}.png"), images[i])
            write_png(os.path.join(out, "Masks", f"{sid}.png"), masks[i])
            np.save(os.path.join(out, "SAM_Embeddings", f"{sid}.npy"), embeddings[i])

    return writers.submit(write)


def run(root: str, imset: str, out: str, prop_net, fuse_net, rounds: int = 10, annotator="component", annotation_types=DEFAULT_TYPES, lanes: int = 2,
        seed: int = 0, device: str = "cuda", share_frames: bool = True, stats: dict = None):
    """Process this rank's share of the samples (`lanes` videos in flight) and write ``out/Images``, ``out/Masks``, ``out/SAM_Embeddings`` and -
    rank 0 - ``out/<imset>.csv`` with ``csv_header(annotation_types)``, rows in sample order and then round order; rows and files do not
    depend on the number of lanes or ranks.  Returns the gathered rows on every rank (fp32: sample id, round, frame, frame_cost, video_cost,
    the action's index in ``annotation_types``, then init_iou and one IoU per type as four 16-bit pieces each).
    ``annotator``: a factory of one ``PromptAnnotator`` per lane thread, or the name of a built-in ('component'); ``seed``: the session draws
    nothing - accepted so that the drivers share their arguments; ``share_frames``, ``stats``: as ``eval_driver.run``."""
    from concurrent.futures import ThreadPoolExecutor

    from mivos.inference_core import InferenceCore

    from .annotate import check_annotation_types
    if annotator is None:
        raise ValueError(f"annot_driver needs annotator=...: {ARGUMENTS['annotator']}")
    if isinstance(annotator, str) and annotator not in ANNOTATORS:
        make_annotator(annotator)                                  # raises what eval_driver raises for the name
    types_ = check_annotation_types(annotation_types)
    ds = ClipDataset(root, imset)
    rank, mine = rank_samples(ds, share_frames)
    cores = lane_cores(InferenceCore, prop_net, fuse_net, lanes, share_frames)
    width = 6 + 4 * (1 + len(types_))
    for sub in ("Images", "Masks", "SAM_Embeddings"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    writers = ThreadPoolExecutor(8)                                # zlib releases the GIL: the encoders run beside the lanes
    pending, lane = [], threading.local()

    def work(i, sample):
        t_c = time.perf_counter()
        proc = cores.core_for(sample)
        t_s = time.perf_counter()
        if not hasattr(lane, "annotator"):                         # one per lane thread
            lane.annotator = make_annotator(annotator) if isinstance(annotator, str) else annotator()
        res = run_annotation_dataset(proc, sample, rounds, lane.annotator, types_)
        cores.done(proc)
        pending.append(_export(res, sample["rgb"][0], out, writers))
        add_stats(stats, dict(create_s=t_s - t_c, session_s=time.perf_counter() - t_s, propagated_frames=res["propagated_frames"],
                              interactions=len(res["annotation_times"])))
        rows = []
        for row in res["rows"]:
            v = np.empty(width, np.float32)
            v[:6] = (i, row["round"], row["frame_num"], row["frame_cost"], row["video_cost"], types_.index(row["selected_annotation"]))
            for j, key in enumerate(["init_iou"] + [f"{t}_iou" for t in types_]):
                v[6 + 4 * j:10 + 4 * j] = _pack64(row[key])
            rows.append(v)
        return rows

    rows = run_lanes(root, imset, mine, lanes, work, device, stats, share_frames=share_frames, lane_done=cores.release)
    cores.add_to(stats)
    t_p = time.perf_counter()
    for f in pending:
        if f is not None:
            f.result()                                             # surface write errors; every file is on disk before the CSV
    if stats is not None:
        stats["wait_writers_s"] = round(time.perf_counter() - t_p, 4)
    writers.shutdown()
    allrows, ordered = gather_sorted(rows, width)
    if rank == 0:
        imset_str = os.path.splitext(os.path.basename(imset))[0]
        with open(os.path.join(out, f"{imset_str}.csv"), "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(csv_header(types_))
            for row in ordered:
                name, r, frame = ds.name(int(row[0])), int(row[1]), int(row[2])
                wr.writerow([f"{name}_{r}_frame_{frame}", float(row[3]), float(row[4]), types_[int(row[5])], frame, r, name]
                            + [_unpack64(row[6 + 4 * j:10 + 4 * j]) for j in range(1 + len(types_))])
    return allrows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--imset", required=True)
    ap.add_argument("--out", default="AnnotDB")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--annotator", default="component", choices=ANNOTATORS, help="the segmenter behind clicks and boxes: 'component' is a deterministic "
                    "stand-in that knows the ground truth (NOT a segmenter); a real SAM controller is passed to annot_driver.run(annotator=...)")
    ap.add_argument("--annotation-types", nargs="+", default=list(DEFAULT_TYPES), metavar="TYPE", help="'click', 'bbox', 'mask' or '<N>clicks'")
    ap.add_argument("--lanes", type=int, default=2, help="videos in flight per GPU")
    ap.add_argument("--seed", type=int, default=0, help="accepted for symmetry with eval_driver: the oracle session draws nothing")
    ap.add_argument("--no-share-frames", action="store_true", help="a fresh engine and a fresh upload of the clip for every object of a video "
                    "(default: the sessions of a video's objects share one engine and its frame features; same output)")
    ap.add_argument("--prop-weights", default="./model_weights/mivos/stcn_yt_vos.pth")
    ap.add_argument("--fusion-weights", default="./model_weights/mivos/fusion_stcn_yt_vos.pth")
    ap.add_argument("--synthetic-weights", action="store_true", help="use the deterministic recipe (no checkpoints)")
    ap.add_argument("--top-k", type=int, default=50, help="rows of the memory bank each query reads, 1..50 (PropagationNetwork(top_k=...): 20 for STCN checkpoints, 50 for MiVOS)")
    ap.add_argument("--km", type=float, default=None, metavar="SIGMA", help="kernelized memory read: standard deviation (1/16-scale positions) of the Gaussian "
                    "around each memory row's best query; default: the plain read")
    a = ap.parse_args()
    prop, fuse = load_networks(a)
    rows = run(a.root, a.imset, a.out, prop, fuse, a.rounds, a.annotator, a.annotation_types, a.lanes, a.seed, share_frames=not a.no_share_frames)
    report_and_leave(f"{len(rows)} rows -> {os.path.join(a.out, os.path.splitext(os.path.basename(a.imset))[0] + '.csv')}")


if __name__ == "__main__":
    main()
