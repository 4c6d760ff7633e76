"""Frame-quality dataset generation on the HIP engine, sharded over the GPUs of one node (BASELINE config 4).

Own counterpart of the reference driver ``generate_fq_dataset.py:60-86`` and what it calls - the clip loader
``datasets/annotation_dataset.py:80-132`` (one sample per (video, object), ImageNet normalisation
``datasets/range_transform.py:3-6``), the oracle policy ``interactions/mask.py:113-156`` (8 rounds: annotate
the worst frame by J with its ground-truth mask; ``oracle_rounds``, a record for the session loop of ``eva_vos_amd/sessions.py``) and
the writer ``util/fq_dataset.py:50-91`` (224x224 nearest-resized masks as PNG + a CSV of
``state_name, ious, selected_frame``).  Differences by design:

* samples are assigned to ranks with an LPT schedule over their frame counts instead of ``--min-idx/--max-idx``;
  propagation has no collective; ONE gather of fixed-width rows at the end (RCCL over xGMI), rank 0 writes the CSV;
* a decoded clip is cached per video and reused for all its objects (the reference re-decodes it per object);
* so are its device copy and the engine with the frame features it has computed: the sessions of a video's objects run one after the other
  on one ``InferenceCore`` re-targeted with ``reset(keep_frame_features=True)``, videos are dealt whole to ranks and lanes - same rows and
  files (``--no-share-frames``: a fresh engine and upload per sample);
* J is computed on the GPU from the engine's mask tensor (``stcn_metrics_jf_counts``), only counts cross PCIe;
* the 224x224 PNG states are encoded and written by host threads while the GPU propagates the next round.
* two samples are in flight per GPU (host thread + HIP stream each, ``--lanes``): +9..17 % rounds/s;

Usage:  python -m eva_vos_amd.fq_driver --root data/MOSE --imset data/MOSE/ImageSets/subset_train_4.txt --out FQ_DB
        (multi-GPU: python -m torch.distributed.run --nproc-per-node N -m eva_vos_amd.fq_driver ...)
"""
from __future__ import annotations

import argparse
import csv
import os
import time
from typing import Dict, List

import numpy as np
import torch
from PIL import Image

from . import metrics, shard
from .sessions import NO_OBJECT, SessionPolicy, annotation_session, frame_quality  # noqa: F401  (frame_quality: callers find it here too)

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


# ------------------------------------------------------------------------------------------------ data
_DECODE_POOL = None
_DECODE_LOCK = __import__("threading").Lock()


class _DecodeProcs:
    """A pool of image-decode worker PROCESSES (eva_vos_amd/_decode_worker.py: NumPy + Pillow only) fed over pipes; the pixels come back
    through shared memory.  Threads would do the decoding itself just as well (Pillow releases the interpreter lock inside its codecs) but
    they take that lock thousands of times per video around the codec calls - and the lanes that drive the GPU share it (round 6:
    building one InferenceCore, 0.9 ms of Python, took 30-60 ms beside 16 decode threads)."""

    def __init__(self, n: int):
        import atexit
        import queue
        import subprocess
        import sys
        from concurrent.futures import ThreadPoolExecutor
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        self.idle = queue.Queue()
        self.procs = [subprocess.Popen([sys.executable, "-m", "eva_vos_amd._decode_worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                       text=True, bufsize=1, cwd=root, env=env) for _ in range(n)]
        for p_ in self.procs:
            self.idle.put(p_)
        self.waiters = ThreadPoolExecutor(n, thread_name_prefix="stcn-decode-wait")      # threads that only block on a worker's pipe
        atexit.register(self.close)

    def close(self):
        for p_ in self.procs:
            try:
                p_.stdin.close()
            except OSError:
                pass
        self.procs = []

    def _call(self, req: dict):
        import json
        p_ = self.idle.get()
        try:
            p_.stdin.write(json.dumps(req) + "\n")
            p_.stdin.flush()
            ans = p_.stdout.readline()
        finally:
            self.idle.put(p_)
        if not ans.startswith("ok"):
            raise RuntimeError(f"image-decode worker: {ans.strip() or 'died'}")

    def decode(self, jpgs, pngs, H: int, W: int):
        """uint8 [T,H,W,3] frames and [T,H,W] label maps of one video (either list may be None), decoded by the workers in chunks."""
        from multiprocessing import shared_memory
        T = len(jpgs if jpgs is not None else pngs)
        rgb = shared_memory.SharedMemory(create=True, size=T * H * W * 3) if jpgs is not None else None
        lab = shared_memory.SharedMemory(create=True, size=T * H * W) if pngs is not None else None
        try:
            step = max(1, -(-T // (2 * len(self.procs))))
            futs = []
            for f0 in range(0, T, step):
                frames = [[t, jpgs[t] if jpgs is not None else None, pngs[t] if pngs is not None else None] for t in range(f0, min(T, f0 + step))]
                futs.append(self.waiters.submit(self._call, {"rgb": rgb.name if rgb else None, "lab": lab.name if lab else None, "shape": [T, H, W], "frames": frames}))
            for f in futs:
                f.result()
            u8 = np.ndarray((T, H, W, 3), np.uint8, buffer=rgb.buf).copy() if rgb else None
            lb = np.ndarray((T, H, W), np.uint8, buffer=lab.buf).copy() if lab else None
            return u8, lb
        finally:
            for m in (rgb, lab):
                if m is not None:
                    m.close()
                    m.unlink()


def decode_pool():
    """The process-wide image-decode pool shared by every lane's loader (what matters is that the NEXT sample of every lane is ready when
    the lane asks for it, not who decodes it).  STCN_DECODE_PROCS worker processes (default min(8, host cores / 4); see _DecodeProcs);
    STCN_DECODE_PROCS=0: a pool of STCN_DECODE_THREADS threads instead (default min(16, cores / 2); 0 = decode inline)."""
    global _DECODE_POOL
    cores = os.cpu_count() or 2
    n_proc = int(os.environ.get("STCN_DECODE_PROCS", min(8, max(1, cores // 4))))
    n_thr = int(os.environ.get("STCN_DECODE_THREADS", min(16, max(1, cores // 2))))
    if n_proc <= 0 and n_thr <= 0:
        return None
    with _DECODE_LOCK:
        if _DECODE_POOL is None:
            if n_proc > 0 and os.path.isdir("/dev/shm"):
                try:
                    _DECODE_POOL = _DecodeProcs(n_proc)
                except OSError:
                    _DECODE_POOL = None
            if _DECODE_POOL is None and n_thr > 0:
                from concurrent.futures import ThreadPoolExecutor
                _DECODE_POOL = ThreadPoolExecutor(n_thr, thread_name_prefix="stcn-decode")
        return _DECODE_POOL


class ClipDataset:
    """DAVIS/MOSE directory layout: JPEGImages/480p/<video>/%05d.jpg, Annotations/480p/<video>/%05d.png
    (palette index = object id).  One sample per (video, object), named ``<video>__<obj>``.

    ``per_video=True`` is the view of the multi-object sessions: one sample per video that has an object, named ``<video>``, with the
    label map itself as ``gt`` (uint8 [1,T,1,H,W]), ``num_objects`` = k (the largest label of the first frame, as the per-object view
    counts them) and ``object_ids`` = the k sample ids the per-object view gives its objects.  Same decoded clip cache."""

    def __init__(self, root: str, imset: str, resolution: str = "480p", per_video: bool = False):
        self.image_dir = os.path.join(root, "JPEGImages", resolution)
        self.mask_dir = os.path.join(root, "Annotations", resolution)
        self.per_video = per_video
        self.samples: List[tuple] = []          # (video, object id, frames); per_video: (video, number of objects, frames)
        self.object_names: List[str] = []       # per-object sample id -> <video>__<obj>, in either view
        self.first_object_id: List[int] = []    # per_video: the per-object sample id of object 1 of sample i
        for line in open(imset):
            v = line.strip()
            if not v:
                continue
            first = np.array(Image.open(os.path.join(self.mask_dir, v, "00000.png")).convert("P"))
            n = len(os.listdir(os.path.join(self.image_dir, v)))
            k = int(first.max())
            if per_video and k > 0:
                self.samples.append((v, k, n))
                self.first_object_id.append(len(self.object_names))
            for obj in range(1, k + 1):
                if not per_video:
                    self.samples.append((v, obj, n))
                self.object_names.append(f"{v}__{obj}")
        self._cache: Dict[str, tuple] = {}

    def __len__(self):
        return len(self.samples)

    def name(self, i):
        v, o, _ = self.samples[i]
        return v if self.per_video else f"{v}__{o}"

    def _clip(self, video: str, n: int):
        """Decoded once per video (samples of a video are adjacent): the frames as uint8 [T,H,W,3] - pinned when a GPU is there, so
        that the prefetcher can upload the BYTES (a quarter of the fp32 clip) and normalise on the device - and the label maps.
        Round 6: the frames of a video are decoded by a SHARED pool of host threads (PIL releases the GIL while it decodes): one thread
        per lane took ~150 ms per 40-frame 480p video, more than the GPU needs for its eight rounds - the lanes waited for their loaders."""
        if video not in self._cache:
            self._cache.clear()                  # keep one decoded clip

            def frame(f):
                return np.asarray(Image.open(os.path.join(self.image_dir, video, f"{f:05d}.jpg")).convert("RGB"))

            def label(f):
                return np.array(Image.open(os.path.join(self.mask_dir, video, f"{f:05d}.png")).convert("P"), dtype=np.uint8)

            pool = decode_pool()
            if isinstance(pool, _DecodeProcs):
                w_, h_ = Image.open(os.path.join(self.image_dir, video, "00000.jpg")).size        # header only
                u8, lab = pool.decode([os.path.join(self.image_dir, video, f"{f:05d}.jpg") for f in range(n)],
                                      [os.path.join(self.mask_dir, video, f"{f:05d}.png") for f in range(n)], h_, w_)
            elif pool is None:
                u8, lab = np.stack([frame(f) for f in range(n)]), np.stack([label(f) for f in range(n)])
            else:
                fr, lb = [pool.submit(frame, f) for f in range(n)], [pool.submit(label, f) for f in range(n)]
                u8, lab = np.stack([x.result() for x in fr]), np.stack([x.result() for x in lb])
            u8 = torch.from_numpy(np.ascontiguousarray(u8))
            if torch.cuda.is_available():
                u8 = u8.pin_memory()
            self._cache[video] = [u8, torch.from_numpy(lab), None]
        return self._cache[video]

    @staticmethod
    def normalize_host(u8: torch.Tensor) -> torch.Tensor:
        """ToTensor + ImageNet normalisation on the host, [T,H,W,3] uint8 -> [T,3,H,W] float32 (datasets/range_transform.py:3-6)."""
        rgb = u8.numpy().astype(np.float32) / 255.0
        return torch.from_numpy(np.ascontiguousarray(((rgb - MEAN) / STD).transpose(0, 3, 1, 2)))

    @staticmethod
    def normalize_lut() -> np.ndarray:
        """The 3 x 256 values normalize_host can produce: a byte has 256 values per channel, so the host arithmetic evaluated on them IS the
        whole function - a table look-up on the device is bit-identical to the host path by construction (no GPU division in between)."""
        b = np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1)                    # [256, 3]: byte value in every channel
        return np.ascontiguousarray(((b.astype(np.float32) / 255.0 - MEAN) / STD).T)  # [3, 256] float32, the expression of normalize_host

    @staticmethod
    def normalize_device(u8: torch.Tensor) -> torch.Tensor:
        """normalize_host on the device the bytes were uploaded to: per channel a 256-entry table look-up (one gather pass instead of four
        host passes over 200 MB).  Bit-identical to normalize_host (tests/test_gpu_driver_golden.py asserts equality, not closeness)."""
        lut = torch.from_numpy(ClipDataset.normalize_lut()).to(u8.device)
        out = torch.empty((u8.shape[0], 3) + tuple(u8.shape[1:3]), dtype=torch.float32, device=u8.device)
        for c in range(3):
            out[:, c] = torch.nn.functional.embedding(u8[..., c].to(torch.int32), lut[c].view(256, 1)).squeeze(-1)
        return out

    def _meta(self, i):
        v, obj, n = self.samples[i]
        entry = self._clip(v, n)
        if self.per_video:                                         # obj is the number of objects here
            first = self.first_object_id[i]
            return entry, {"gt": entry[1][None, :, None], "name": v, "video": v, "num_frames": n, "num_objects": obj,
                           "object_ids": list(range(first, first + obj))}
        gt = (entry[1] == obj).float()[None, :, None]              # [1,T,1,H,W], no bg channel (reference layout)
        return entry, {"gt": gt, "name": self.name(i), "video": v, "num_frames": n}

    def __getitem__(self, i):
        entry, sample = self._meta(i)
        if entry[2] is None:
            entry[2] = self.normalize_host(entry[0])               # host users (CPU tests, reference-style loops): normalised once per video
        sample["rgb"] = entry[2][None]
        return sample

    def raw(self, i):
        """The sample with its frames as uint8 [T,H,W,3] (``rgb_u8``) instead of the normalised float clip: for the prefetcher."""
        entry, sample = self._meta(i)
        sample["rgb_u8"] = entry[0]
        return sample


def prefetched(ds: "ClipDataset", indices, device: str = "cuda", timing: dict = None, share_frames: bool = True):
    """Yield (i, sample) for i in indices with sample['rgb'] already on `device`.  The NEXT sample is decoded on a
    host thread (PIL releases the GIL) into pinned memory as BYTES, copied H2D and normalised on a side stream while the caller
    propagates the current one (round 4: the host used to normalise in four NumPy passes over 200 MB per clip and upload fp32) - the reference decodes and uploads synchronously between samples (generate_fq_dataset.py:60-63).
    ``share_frames``: a sample of the video the previous one belonged to (its next object) gets the device clip of that one - the same
    tensor, neither uploaded nor normalised again."""
    from concurrent.futures import ThreadPoolExecutor
    on_gpu = torch.cuda.is_available() and str(device).startswith("cuda")
    side = torch.cuda.Stream() if on_gpu else None
    last = {}                                                     # the clip of the loader's previous sample: video, rgb, _ready, _host

    def load(i):
        if not on_gpu:
            return dict(ds[i])
        sample = dict(ds.raw(i))
        host = sample.pop("rgb_u8")                               # pinned uint8 [T,H,W,3]: a quarter of the fp32 clip crosses PCIe
        if share_frames and last.get("video") == sample["video"]:
            sample.update(rgb=last["rgb"], _ready=last["_ready"], _host=last["_host"])
            return sample
        with torch.cuda.stream(side):
            sample["rgb"] = ds.normalize_device(host.to(device, non_blocking=True))[None]      # normalised on the device, on the side stream
            ev = torch.cuda.Event()
            ev.record(side)
        sample["_ready"], sample["_host"] = ev, host              # keep the pinned buffer alive until the copy is done
        last.clear()
        if share_frames:
            last.update(video=sample["video"], rgb=sample["rgb"], _ready=ev, _host=host)
        return sample

    indices = list(indices)
    with ThreadPoolExecutor(1) as pool:
        fut = pool.submit(load, indices[0]) if indices else None
        for n, i in enumerate(indices):
            t_w = time.perf_counter()
            sample = fut.result()
            if timing is not None:                                # how long the lane stood waiting for its loader (decode + upload not hidden)
                timing["wait_input_s"] = timing.get("wait_input_s", 0.0) + time.perf_counter() - t_w
            fut = pool.submit(load, indices[n + 1]) if n + 1 < len(indices) else None
            if on_gpu:
                torch.cuda.current_stream().wait_event(sample.pop("_ready"))
                sample["rgb"].record_stream(torch.cuda.current_stream())
                sample.pop("_host")
            yield i, sample


_STATS_LOCK = __import__("threading").Lock()


def lane_engine_options(lanes: int):
    """Engine tunables for `lanes` videos in flight per GPU: the engines' own side streams (key-encoder look-ahead, FusionNet of
    rounds >= 2) help ONE video in flight (+6..8 %); with several lanes the videos already fill each other's gaps and eight
    streams only contend (second interactions -3 %).  Given to InferenceCore explicitly - the process environment is not touched
    (an STCN_LOOKAHEAD set by the user still wins)."""
    return {"lookahead": 0} if lanes > 1 and "STCN_LOOKAHEAD" not in os.environ else None


class LaneCores:
    """The InferenceCore of every lane thread, kept while the lane's consecutive samples belong to one video.  Per-object mode: one
    annotation session per (video, object), as the reference runs them (interactions/eval.py:92-99) - but what the engine caches per
    frame does not depend on the object, so the next object of the video gets the SAME core, re-targeted with
    ``reset(keep_frame_features=True)``: no second engine, no second pass of the key encoder over the clip.  A new core is built only
    when the video changes (the old one is dropped first: its device memory serves the new one).  ``share_frames=False``: a fresh core
    per sample, the reference's protocol to the letter (A/B runs).  ``make(sample)`` constructs a core.
    ``engines_created`` / ``key_frames_encoded`` count over all lanes (``done(core)`` adds a finished session's key-encoder frames)."""

    def __init__(self, make, share_frames: bool = True):
        import threading
        self.make, self.share_frames = make, share_frames
        self.local, self.lock = threading.local(), threading.Lock()
        self.engines_created = self.key_frames_encoded = 0

    def core_for(self, sample):
        tl = self.local
        if self.share_frames and getattr(tl, "core", None) is not None and tl.video == sample["video"]:
            tl.core.reset(keep_frame_features=True)
            return tl.core
        tl.core = None
        core = self.make(sample)
        with self.lock:
            self.engines_created += 1
        if self.share_frames:
            tl.core, tl.video = core, sample["video"]
        return core

    def done(self, core):
        with self.lock:
            self.key_frames_encoded += int(core.key_frames_encoded)

    def release(self):
        """The calling lane has no more samples: its core goes now, not when the last lane ends."""
        self.local.core = None

    def add_to(self, stats: dict):
        add_stats(stats, {k_: getattr(self, k_) for k_ in ("engines_created", "key_frames_encoded")})


def run_lanes(root: str, imset: str, mine, lanes: int, work, device: str = "cuda", stats: dict = None, per_video: bool = False,
              share_frames: bool = True, lane_done=None):
    """Process the samples `mine` on `lanes` host threads, each with its own HIP stream, clip loader and prefetcher
    (samples are independent; two videos in flight fill each other's kernel tails, as bench.py's lanes do).
    work(i, sample) -> list of rows; returns all rows.  Chunks are contiguous so that the objects of one video stay
    with one loader (per-video decode cache).  ``per_video``: the indices are those of ``ClipDataset(..., per_video=True)``.
    ``share_frames`` (per-object samples): the chunks are cut between videos wherever there are at least as many videos as lanes, at about
    equal frame counts (shard.chunk_bounds) - the objects of a video then meet one lane, one device clip and one engine (LaneCores) - and
    the prefetcher uploads a clip once per video.  ``lane_done()``, if given, is called on every lane's thread after its last sample."""
    from concurrent.futures import ThreadPoolExecutor
    mine = list(mine)
    lanes = max(1, min(lanes, len(mine)))
    on_gpu = torch.cuda.is_available() and str(device).startswith("cuda")
    dev_index = torch.cuda.current_device() if on_gpu else None
    if share_frames and not per_video and lanes > 1:
        samples = ClipDataset(root, imset).samples
        bounds = shard.chunk_bounds([samples[i][0] for i in mine], lanes, [samples[i][2] for i in mine])
    else:
        bounds = [len(mine) * l // lanes for l in range(lanes + 1)]

    def lane(l):
        ds = ClipDataset(root, imset, per_video=per_video)
        rows = []
        if on_gpu:
            torch.cuda.set_device(dev_index)
            ctx = torch.cuda.stream(torch.cuda.Stream())
        else:
            import contextlib
            ctx = contextlib.nullcontext()
        timing = {} if stats is not None else None
        t_lane = time.perf_counter()
        with ctx:
            try:
                for i, sample in prefetched(ds, mine[bounds[l]:bounds[l + 1]], device, timing, share_frames and not per_video):
                    t_s = time.perf_counter()
                    rows += work(i, sample)
                    if timing is not None:
                        timing["work_s"] = timing.get("work_s", 0.0) + time.perf_counter() - t_s
                if on_gpu:
                    torch.cuda.current_stream().synchronize()
            finally:
                if lane_done is not None:
                    lane_done()
        if stats is not None:                                      # host-side account of the lane: where its wall time went
            timing["lane_s"] = time.perf_counter() - t_lane
            with _STATS_LOCK:
                stats.setdefault("lanes", []).append({k_: round(v_, 4) for k_, v_ in timing.items()})
        return rows

    if lanes == 1:
        return lane(0)
    with ThreadPoolExecutor(lanes) as ex:
        return [r for part in ex.map(lane, range(lanes)) for r in part]


def rank_samples(ds: "ClipDataset", share_frames: bool, multi_object: bool = False):
    """(this process's rank, the sorted samples of `ds` that are its share): an LPT schedule over the ranks by frame count.
    ``share_frames``: videos are dealt whole - the objects of a video share an engine; else samples are dealt one by one (adjacent objects still
    share a decode), a per-video sample of the multi-object mode weighing frames x objects."""
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)
    if share_frames:
        parts = shard.lpt_assign_grouped([s[2] for s in ds.samples], [s[0] for s in ds.samples], world)
    else:
        parts = shard.lpt_assign([s[2] * (s[1] if multi_object else 1) for s in ds.samples], world)
    return rank, sorted(parts[rank])


def lane_cores(core_class, prop_net, fuse_net, lanes: int, share_frames: bool, multi_object: bool = False) -> LaneCores:
    """The LaneCores of a driver run: ``core_class`` (InferenceCore, as the caller sees it) over the sample's clip, with all the objects of a
    per-video sample or with one."""
    return LaneCores(lambda sample: core_class(prop_net, fuse_net, sample["rgb"], sample["num_objects"] if multi_object else 1,
                                               engine_options=lane_engine_options(lanes)), share_frames)


def add_stats(stats: dict, more: dict) -> None:
    """Add a session's counters and seconds to the run's `stats` (None: nothing is kept); the lanes share the dict."""
    if stats is not None:
        with _STATS_LOCK:
            for k_, v_ in more.items():
                stats[k_] = stats.get(k_, 0) + v_


def gather_sorted(rows: list, width: int):
    """The one collective of a run: every rank's rows, gathered on every rank (shard.gather_rows) - and the same rows in the order the CSV
    lists them, by sample id and round."""
    allrows = shard.gather_rows(np.stack(rows) if rows else np.zeros((0, width), np.float32), width)
    return allrows, allrows[np.lexsort((allrows[:, 1], allrows[:, 0]))]


def make_synthetic_tree(root: str, videos: Dict[str, tuple], seed: int = 0) -> str:
    """Write a tiny DAVIS-layout dataset (for tests / smoke runs).  videos: name -> (T, H, W, n_objects)."""
    from . import synth
    names = []
    for vi, (name, (T, H, W, k)) in enumerate(videos.items()):
        os.makedirs(os.path.join(root, "JPEGImages", "480p", name), exist_ok=True)
        os.makedirs(os.path.join(root, "Annotations", "480p", name), exist_ok=True)
        img = synth.synthetic_clip(T, H, W, seed=seed + vi)[0].numpy()
        msk = synth.synthetic_mask(T, H, W, k, seed=seed + vi)[:, :, 0].numpy()
        for t in range(T):
            rgb = np.clip((img[t].transpose(1, 2, 0) * STD + MEAN) * 255, 0, 255).astype(np.uint8)
            Image.fromarray(rgb).save(os.path.join(root, "JPEGImages", "480p", name, f"{t:05d}.jpg"), quality=95)
            lab = np.zeros((H, W), np.uint8)
            for o in range(k):
                lab[msk[o, t] > 0.5] = o + 1
            pim = Image.fromarray(lab, mode="P")
            pim.putpalette([0, 0, 0, 255, 0, 0, 0, 255, 0, 0, 0, 255] + [0] * (256 * 3 - 12))
            pim.save(os.path.join(root, "Annotations", "480p", name, f"{t:05d}.png"))
        names.append(name)
    os.makedirs(os.path.join(root, "ImageSets"), exist_ok=True)
    imset = os.path.join(root, "ImageSets", "synthetic.txt")
    open(imset, "w").write("\n".join(names) + "\n")
    return imset


# ------------------------------------------------------------------------------------------------ policy
def oracle_rounds(processor, sample, rounds: int = 8, stats: dict = None):
    """The oracle annotation policy of the FQ dataset (interactions/mask.py:113-156): annotate the worst frame by J with its ground-truth
    mask.  `stats` (optional dict, one per caller thread): see sessions.annotation_session.
    Round 6: the evaluation of a round stays on the device (metrics.RoundScorer: compose + J counts + fp64 quality + arg-min in one enqueue);
    one int per round crosses PCIe, the per-frame J rows of all rounds are fetched once at the end.  Same values, same selection as
    sessions.frame_quality + numpy.argmin (tests/test_gpu_driver_golden.py).  Returns ([(selected frame, quality[T]) per round], gens)."""
    gt = sample["gt"][0].to(processor.prob.device)              # [T,1,H,W]
    scorer = metrics.RoundScorer(gt[:, 0], "j", max_rounds=max(rounds, 1), no_object=NO_OBJECT)
    policy = SessionPolicy(mask_of=lambda f: gt[f][None], choose_frame=lambda worst, types, gen, frames: worst, keep_gen=True)
    ses = annotation_session(processor, scorer, sample["num_frames"], rounds, policy, stats)
    q = scorer.qualities()
    return [(w, q[i]) for i, w in enumerate(ses["chosen"][1:])], ses["gens"]


# ------------------------------------------------------------------------------------------------ output
def write_png(path: str, a: np.ndarray, level: int = 1) -> None:
    """8-bit grayscale [H,W] or RGB [H,W,3] PNG, written with zlib directly: the writer threads of a run encode ~3 000 small images,
    and PIL's encoder holds the GIL while it works - the lanes that drive the GPU then wait for the interpreter (fq_driver: 52 rounds/s
    without output, 28 with it through PIL).  ``zlib.compress`` / ``zlib.crc32`` release the GIL on buffers of this size, so the
    encoding really runs beside the lanes.  Filter type 0 on every scanline; any PNG reader decodes the same pixels."""
    import struct
    import zlib
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape[:2]
    ctype = 2 if a.ndim == 3 else 0
    raw = np.empty((h, 1 + w * (3 if ctype == 2 else 1)), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = a.reshape(h, -1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + chunk(b"IEND", b""))


def _write_frames(dev8: torch.Tensor, out_dir: str, pool=None):
    """uint8 frames [T,H,W] or [T,H,W,3] -> out_dir/%05d.png.  With `pool` (a ThreadPoolExecutor) the PNG encoding + file writes happen on
    host threads while the GPU propagates the next round (zlib and file I/O release the GIL); returns the future, or None when done inline.
    Round 6: with a pool the download does not stop the lane either - the frames go to pinned memory asynchronously and the WRITER thread
    waits for the copy (an event), not the thread that drives the GPU."""
    if pool is None or not dev8.is_cuda:
        frames, ready = dev8.cpu().numpy(), None
    else:
        host = torch.empty(dev8.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(dev8, non_blocking=True)
        ready = torch.cuda.Event(blocking=True)
        ready.record()
        dev8.record_stream(torch.cuda.current_stream())
        frames = host.numpy()

    def write():
        if ready is not None:
            ready.synchronize()
        os.makedirs(out_dir, exist_ok=True)
        for t, m in enumerate(frames):
            write_png(os.path.join(out_dir, f"{t:05d}.png"), m)

    if pool is None:
        write()
        return None
    return pool.submit(write)


def save_state_masks(gen: torch.Tensor, out_dir: str, pool=None):
    """224x224 nearest-neighbour PNGs like util/fq_dataset.py:64-84 (mask_to_224).  The resize runs on the device; `pool` and the return
    value: see _write_frames."""
    small = torch.nn.functional.interpolate(gen[:, None].float(), size=(224, 224), mode="nearest")[:, 0]
    return _write_frames((small * 255).to(torch.uint8), out_dir, pool)


def save_rgb_frames(rgb: torch.Tensor, out_dir: str, pool=None):
    """RGBFrames/224/<video>/%05d.png like util/fq_dataset.py:26-47 (``save_frames``): each normalised frame is resized to
    224x224 (bicubic, antialias), min-max normalised PER FRAME (``im_normalize``) and written as 8-bit RGB - the inputs of
    the reference's QNet training set.  rgb: [T,3,H,W] float (ImageNet-normalised, host or device); the resize runs where
    the tensor lives, the PNG encoding on `pool` threads when given (_write_frames)."""
    small = torch.nn.functional.interpolate(rgb.float(), size=(224, 224), mode="bicubic", align_corners=False, antialias=True)
    lo = small.amin((1, 2, 3), keepdim=True)
    hi = small.amax((1, 2, 3), keepdim=True)
    return _write_frames(((small - lo) / (hi - lo).clamp_min(1e-8) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous(), out_dir, pool)


def run(root: str, imset: str, out: str, prop_net, fuse_net, rounds: int = 8, save_masks: bool = True,
        device: str = "cuda", lanes: int = 2, stats: dict = None, share_frames: bool = True, working_size=None):
    """Process this rank's share of the samples (`lanes` videos in flight); returns the gathered rows on every rank
    (rows: sample id, round, selected frame, T, then T per-frame J values padded with NaN).
    `stats` (optional dict): this rank's `propagated_frames` (frames the engines visited), `interactions`, `key_frames_encoded` (frames
    that went through the key encoder) and `engines_created` are added to it.
    `share_frames`: the sessions of a video's objects run one after the other on ONE engine that keeps the clip and its frame features
    between them (LaneCores) - videos, not samples, are dealt to ranks and lanes.  Same rows, same files; False: a fresh engine and a
    fresh upload per sample, samples dealt one by one.
    `working_size` (an int; None: the clip's own size, as before): the engines propagate on the clip brought down to that shorter side, J is
    computed on the masks brought back to the clip's own size (working_size.ScaledInferenceCore takes InferenceCore's place); the 224 x 224
    frames and states are made from own-size data as before."""
    import functools
    from concurrent.futures import ThreadPoolExecutor

    from mivos.inference_core import InferenceCore

    from .working_size import ScaledInferenceCore, check_working_size
    core_class = InferenceCore if check_working_size(working_size) is None else functools.partial(ScaledInferenceCore, working_size=working_size)
    ds = ClipDataset(root, imset)
    rank, mine = rank_samples(ds, share_frames)
    cores = lane_cores(core_class, prop_net, fuse_net, lanes, share_frames)
    width = 4 + max(s[2] for s in ds.samples)
    writers = ThreadPoolExecutor(8) if save_masks else None           # zlib releases the GIL: the encoders really run beside the lanes
    pending = []

    saved_rgb = set()
    rgb_lock = __import__("threading").Lock()

    def work(i, sample):
        rows = []
        if save_masks:                                     # once per video (generate_fq_dataset.py:77-80)
            with rgb_lock:
                first = sample["video"] not in saved_rgb
                saved_rgb.add(sample["video"])
            if first:
                pending.append(save_rgb_frames(sample["rgb"][0], os.path.join(out, "RGBFrames", "224", sample["video"]), writers))
        t_c = time.perf_counter()
        proc = cores.core_for(sample)
        mine_stats = {"create_s": time.perf_counter() - t_c} if stats is not None else None
        t_c = time.perf_counter()
        states, gens = oracle_rounds(proc, sample, rounds, mine_stats)
        cores.done(proc)
        if stats is not None:
            add_stats(stats, dict(mine_stats, session_s=time.perf_counter() - t_c))
        sid = 1
        for r, ((worst, q), gen) in enumerate(zip(states, gens)):
            if float(q[worst]) == NO_OBJECT:
                continue                                   # util/fq_dataset.py:55: no-object states are not saved
            row = np.full(width, np.nan, np.float32)
            row[:4] = (i, sid, worst, len(q))
            row[4:4 + len(q)] = q
            rows.append(row)
            if save_masks:
                pending.append(save_state_masks(gen, os.path.join(out, "Annotations", "224", f"{sample['name']}_round_{sid}"), writers))
            sid += 1
        return rows

    rows = run_lanes(root, imset, mine, lanes, work, device, stats, share_frames=share_frames, lane_done=cores.release)
    cores.add_to(stats)
    t_p = time.perf_counter()
    for f in pending:
        f.result()                                         # surface write errors; all PNGs are on disk before the CSV
    if stats is not None:
        stats["wait_writers_s"] = round(time.perf_counter() - t_p, 4)
    if writers is not None:
        writers.shutdown()
    allrows, ordered = gather_sorted(rows, width)
    if rank == 0:
        os.makedirs(out, exist_ok=True)
        # res_<imset>.csv, columns as generate_fq_dataset.py:48-52,85-86 (the ious cell holds the per-frame list)
        imset_str = os.path.splitext(os.path.basename(imset))[0]
        with open(os.path.join(out, f"res_{imset_str}.csv"), "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(["state_name", "ious", "selected_frame"])
            for row in ordered:
                n = int(row[3])
                wr.writerow([f"{ds.name(int(row[0]))}_round_{int(row[1])}", [float(v) for v in row[4:4 + n]], int(row[2])])
    return allrows


def load_networks(a):
    """The start of either driver's main(): gradients off, this process bound to its GPU and joined to the process group (one process per GPU;
    RCCL unless STCN_DIST_BACKEND says otherwise), and the two networks, in eval mode, with the weights the command line `a` names."""
    from . import synth
    from .params import FusionNet, PropagationNetwork
    torch.set_grad_enabled(False)
    shard.init_from_env()
    prop, fuse = PropagationNetwork(top_k=a.top_k, km=a.km), FusionNet()
    for net, path in ((prop, a.prop_weights), (fuse, a.fusion_weights)):
        net.load_state_dict(synth.recipe_state_dict(net) if a.synthetic_weights else torch.load(path, map_location="cpu"))
    return prop.eval(), fuse.eval()


def report_and_leave(message: str) -> None:
    """The end of it: rank 0 says where the output is, the process group is left."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_rank() == 0:
        print(message)
    if dist.is_initialized():
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--imset", required=True)
    ap.add_argument("--out", default="FQ_DB")
    ap.add_argument("--prop-weights", default="./model_weights/mivos/stcn_yt_vos.pth")
    ap.add_argument("--fusion-weights", default="./model_weights/mivos/fusion_stcn_yt_vos.pth")
    ap.add_argument("--synthetic-weights", action="store_true", help="use the deterministic recipe (no checkpoints)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--lanes", type=int, default=2, help="videos in flight per GPU")
    ap.add_argument("--no-share-frames", action="store_true", help="a fresh engine and a fresh upload of the clip for every object of a video "
                    "(default: the sessions of a video's objects share one engine and its frame features; same output)")
    ap.add_argument("--top-k", type=int, default=50, help="rows of the memory bank each query reads, 1..50 (PropagationNetwork(top_k=...): 20 for STCN checkpoints, 50 for MiVOS)")
    ap.add_argument("--km", type=float, default=None, metavar="SIGMA", help="kernelized memory read: standard deviation (1/16-scale positions) of the Gaussian "
                    "around each memory row's best query (prop_model.memory.km of the reference, e.g. 5.6); default: the plain read")
    ap.add_argument("--working-size", type=int, default=None, metavar="N", help="propagate on the clip resized so that its shorter side is N (antialiased bicubic, "
                    "e.g. 480; clips that are no larger keep their size) and score the masks brought back to the clip's own size; default: the clip's own size")
    a = ap.parse_args()
    if a.working_size is not None and a.working_size < 1:
        ap.error(f"--working-size {a.working_size}: the length of the shorter side, at least 1")
    prop, fuse = load_networks(a)
    rows = run(a.root, a.imset, a.out, prop, fuse, a.rounds, lanes=a.lanes, share_frames=not a.no_share_frames, working_size=a.working_size)
    report_and_leave(f"{len(rows)} states -> {os.path.join(a.out, 'res_' + os.path.splitext(os.path.basename(a.imset))[0] + '.csv')}")


if __name__ == "__main__":
    main()
