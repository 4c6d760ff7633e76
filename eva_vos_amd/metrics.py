"""J (region IoU), F (boundary F-measure) and J&F for binary masks - own NumPy/SciPy implementation of
the measures the reference's callers compute per frame after every interaction
(interactions/metrics.py:24-34 ``get_j_and_f``, :38-97 boundary map, :100-160 ``f_measure``;
interactions/eval.py:27-81).  Caller-side code, integer-exact."""
from __future__ import annotations

import numpy as np
from scipy import ndimage


def jaccard(gt: np.ndarray, pred: np.ndarray) -> float:
    gt, pred = np.asarray(gt, bool), np.asarray(pred, bool)
    union = (gt | pred).sum()
    return 0.0 if union == 0 else float((gt & pred).sum() / union)


def boundary_map(seg: np.ndarray) -> np.ndarray:
    """1-pixel boundary, offset half a pixel towards the origin (the classic seg2bmap at equal size)."""
    seg = np.asarray(seg, bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1], s[:-1, :], se[:-1, :-1] = seg[:, 1:], seg[1:, :], seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def _disk(r: int) -> np.ndarray:
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) <= r * r


def f_measure(gt: np.ndarray, pred: np.ndarray, bound_th: float = 0.008) -> float:
    gt, pred = np.asarray(gt, bool), np.asarray(pred, bool)
    r = int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(gt.shape)))
    fb, gb = boundary_map(pred), boundary_map(gt)
    se = _disk(r)
    n_fg, n_gt = int(fb.sum()), int(gb.sum())
    if n_fg == 0 and n_gt > 0:
        p, rc = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        p, rc = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        p, rc = 1.0, 1.0
    else:
        p = float((fb & ndimage.binary_dilation(gb, se)).sum() / n_fg)
        rc = float((gb & ndimage.binary_dilation(fb, se)).sum() / n_gt)
    return 0.0 if p + rc == 0 else 2 * p * rc / (p + rc)


def j_and_f(gt: np.ndarray, pred: np.ndarray) -> float:
    return 0.5 * jaccard(gt, pred) + 0.5 * f_measure(gt, pred)


def sequence_scores(gt: np.ndarray, pred: np.ndarray, every: int = 1) -> np.ndarray:
    """[T,H,W] masks -> rows (frame, J, F, J&F) for frames 0, every, 2*every, ..."""
    rows = []
    for t in range(0, gt.shape[0], every):
        j, f = jaccard(gt[t], pred[t]), f_measure(gt[t], pred[t])
        rows.append((t, j, f, 0.5 * (j + f)))
    return np.asarray(rows, np.float32)


# ------------------------------------------------------------------------------------------------ GPU path
def _scores_from_counts(c: np.ndarray) -> np.ndarray:
    """[T,6] integer counts -> rows (J, F, J&F) with the reference's special cases (metrics.py:141-158)."""
    out = np.zeros((c.shape[0], 3), np.float64)
    for t, (inter, union, n_gt, n_fg, gt_m, fg_m) in enumerate(c.tolist()):
        j = 0.0 if union == 0 else inter / union
        if n_fg == 0 and n_gt > 0:
            p, r = 1.0, 0.0
        elif n_fg > 0 and n_gt == 0:
            p, r = 0.0, 1.0
        elif n_fg == 0 and n_gt == 0:
            p, r = 1.0, 1.0
        else:
            p, r = fg_m / n_fg, gt_m / n_gt
        f = 0.0 if p + r == 0 else 2 * p * r / (p + r)
        out[t] = (j, f, 0.5 * (j + f))
    return out


def label_counts(gt: np.ndarray, gen: np.ndarray, num_objects: int) -> np.ndarray:
    """Label maps [T,H,W] (0 = background, o in 1..k = object o, a label above k = background) -> int64 [k,T,6]: per object and frame
    the six integers of ``stcn_metrics_jf_counts`` on the binary masks ``gt == o`` and ``gen == o`` (host: NumPy / SciPy)."""
    gt, gen = np.asarray(gt), np.asarray(gen)
    T, H, W = gt.shape
    se = _disk(int(np.ceil(0.008 * np.linalg.norm((H, W)))))
    c = np.zeros((num_objects, T, 6), np.int64)
    for o in range(1, num_objects + 1):
        for t in range(T):
            g, p = gt[t] == o, gen[t] == o
            gb, fb = boundary_map(g), boundary_map(p)
            c[o - 1, t] = ((g & p).sum(), (g | p).sum(), gb.sum(), fb.sum(),
                           (gb & ndimage.binary_dilation(fb, se)).sum() if fb.any() else 0,
                           (fb & ndimage.binary_dilation(gb, se)).sum() if gb.any() else 0)
    return c


def label_round_quality(gt: np.ndarray, gen: np.ndarray, num_objects: int, metric: str = "j_and_f", no_object: float = 20.0, counts=None):
    """The evaluation of one round of a k-object session, restated on the host - the yardstick of ``stcn_metrics_objects_round``.
    gt, gen: label maps [T,H,W] (gen = the evaluated map: ground truth on annotated frames, the engine's labels elsewhere).
    Returns (q [k,T], Q [T], selection), float64:
    q[o][t] = J (``metric == "j"``) or J&F of object o + 1 in frame t from its counts as ``_scores_from_counts`` computes them, ``no_object``
    where ``gt == o + 1`` is empty in frame t;  Q[t] = the mean of q[.][t] over the objects present in the ground truth of frame t - added
    in ascending o, then divided by their number - or ``no_object`` when there is none;  selection = ``numpy.argmin(Q)``.
    ``counts`` (optional [k,T,6]): use these instead of counting on the host."""
    gt = np.asarray(gt)
    k, T = int(num_objects), gt.shape[0]
    c = label_counts(gt, gen, k) if counts is None else np.asarray(counts)
    col = 0 if metric == "j" else 2
    q = np.full((k, T), float(no_object), np.float64)
    Q = np.full(T, float(no_object), np.float64)
    present = np.stack([(gt == o).reshape(T, -1).any(1) for o in range(1, k + 1)])
    for o in range(k):
        q[o, present[o]] = _scores_from_counts(c[o])[present[o], col]
    for t in range(T):
        s, n = 0.0, 0
        for o in range(k):
            if present[o, t]:
                s, n = s + float(q[o, t]), n + 1
        if n:
            Q[t] = s / n
    return q, Q, int(np.argmin(Q))


def _check_num_objects(k) -> int:
    k = int(k)
    if not 1 <= k <= 32:
        raise ValueError(f"num_objects = {k}: the library is built for 1..32 objects (STCN_MAX_OBJECTS)")
    return k


def _ptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import ctypes as C

    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _objects_scratch(k: int, T: int, H: int, W: int, device):
    """The boundary scratch of the k-object metric calls, sized by the library (``stcn_metrics_objects_scratch``) and by nothing else."""
    import ctypes as C

    import torch

    from . import _lib
    n = C.c_int64()
    _lib.check(_lib.lib().stcn_metrics_objects_scratch(k, T, H, W, C.byref(n)), "stcn_metrics_objects_scratch")
    return torch.empty((int(n.value),), dtype=torch.uint8, device=device)


def _boundary_scratch(k, T: int, H: int, W: int, device):
    """A byte per pixel for binary masks (k None), ``_objects_scratch`` for label maps."""
    import torch
    return torch.empty((T * H * W,), dtype=torch.uint8, device=device) if k is None else _objects_scratch(k, T, H, W, device)


def _scores_gpu(gt, pred, k, j_only: bool):
    """The counts of the binary masks (k None: ``stcn_metrics_j[f]_counts``) or of the label maps of k objects
    (``stcn_metrics_objects_j[f]_counts``) gt, pred - uint8 [T,H,W], contiguous, on one cuda device - downloaded (only the integers cross
    PCIe) and turned into rows (J, F, J&F) per frame, float64 [T,3] or [k,T,3]; ``j_only``: columns 1 and 2 are NaN."""
    import torch

    from . import _lib
    assert gt.is_cuda and pred.is_cuda and gt.shape == pred.shape and gt.dim() == 3 and gt.dtype == pred.dtype == torch.uint8
    T, H, W = gt.shape
    name = f"stcn_metrics_{'' if k is None else 'objects_'}{'j' if j_only else 'jf'}_counts"
    with torch.cuda.device(gt.device):
        counts = torch.empty((T, 6) if k is None else (k, T, 6), dtype=torch.int32, device=gt.device)
        scratch = () if j_only else (_boundary_scratch(k, T, H, W, gt.device),)
        _lib.check(getattr(_lib.lib(), name)(_stream(), _ptr(gt), _ptr(pred), *(() if k is None else (k,)), T, H, W, _ptr(counts),
                                             *map(_ptr, scratch)), name)
        c = counts.cpu().numpy()
    if j_only:
        out = np.full(c.shape[:-1] + (3,), np.nan)
        out[..., 0] = np.where(c[..., 1] > 0, c[..., 0] / np.maximum(c[..., 1], 1), 0.0)
        return out
    return _scores_from_counts(c) if k is None else np.stack([_scores_from_counts(c[o]) for o in range(k)])


def sequence_scores_gpu(gt, pred, j_only: bool = False):
    """J, F, J&F per frame on the GPU (HIP kernels behind ``stcn_metrics_jf_counts``).
    gt, pred: torch uint8/bool tensors [T,H,W] on the same cuda device (non-zero = object).
    Returns float64 [T,3]; only the 6*T integer counts cross PCIe.  ``j_only``: the region measure alone (``stcn_metrics_j_counts``:
    no boundary maps, no disk matching) - column 0 is J, columns 1 and 2 are NaN."""
    import torch
    return _scores_gpu((gt != 0).to(torch.uint8).contiguous(), (pred != 0).to(torch.uint8).contiguous(), None, j_only)


def sequence_scores_objects_gpu(gt, pred, num_objects: int, j_only: bool = False):
    """``sequence_scores_gpu`` for label maps of ``num_objects`` objects: gt, pred uint8 [T,H,W] on the same cuda device (0 = background,
    o = object o, a label above ``num_objects`` = background).  Returns float64 [k,T,3] - rows (J, F, J&F) of object o + 1 as
    ``sequence_scores_gpu(gt == o + 1, pred == o + 1)`` returns them - from ONE pass over the pixels (``stcn_metrics_objects_jf_counts``;
    ``j_only``: ``stcn_metrics_objects_j_counts``, columns 1 and 2 NaN)."""
    return _scores_gpu(gt.contiguous(), pred.contiguous(), _check_num_objects(num_objects), j_only)


class RoundScorer:
    """The per-round evaluation of an annotation session, kept on the device (``stcn_metrics_round``): after every ``interact()`` the
    reference's loops compute per-frame J or J&F of the propagated masks against the ground truth (annotated frames counting with their
    ground truth, the NO_OBJECT token for frames without the object: interactions/eval.py:27-81) and the oracle policy takes the arg-min
    (interactions/mask.py:130-133).  Here one C call enqueues compose + counts + fp64 quality + arg-min on the engine's stream; only the
    selected frame (4 bytes) crosses PCIe per round - the host waits for it on a BLOCKING event (it sleeps instead of spinning a core) -
    and the quality rows of all rounds are fetched together at the end of the session (``qualities()``).  Bit-identical to the host path
    (``sequence_scores_gpu`` + NumPy), which the tests assert.

    ``num_objects=k`` scores a MULTI-OBJECT session (``stcn_metrics_objects_round``): ``gt_thw`` is a uint8 label map (0 = background,
    o in 1..k = object o, a label above k = background), ``processor`` an engine built with ``num_objects=k``, ``gen`` the evaluated label map.
    The frame quality is the mean of the per-object qualities over the objects present in the frame's ground truth (``label_round_quality``
    is the host restatement, bit-identical); ``object_qualities()`` returns the per-object rows.  Still one enqueue sequence - its length does
    not depend on k - and one 4-byte download per round."""

    def __init__(self, gt_thw, metric: str = "j", max_rounds: int = 64, no_object: float = 20.0, num_objects=None):
        import torch

        from . import _lib
        assert gt_thw.is_cuda and gt_thw.dim() == 3
        self.metric, self.no_object = metric, float(no_object)
        self.dev = gt_thw.device
        self.T, self.H, self.W = T, H, W = tuple(int(v) for v in gt_thw.shape)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.dev)      # noqa: E731
        # binary masks or label maps: decided here, once - the entry point, what it takes between `annotated` and T (``_which``) and
        # where the per-object rows of round r go (``_object_rows``); score() is the same for both
        if num_objects is None:
            self.k, self.object_quality = None, None
            self.gt = (gt_thw > 0.5 if gt_thw.is_floating_point() else gt_thw != 0).to(torch.uint8).contiguous()
            empty = self.gt.flatten(1).sum(1) == 0
            self.noobj = empty.to(torch.uint8).contiguous()
            self.counts = new((T, 6), torch.int32)
            self._entry, self._which, self._object_rows = "stcn_metrics_round", (_ptr(self.noobj),), lambda r: ()
        else:
            self.k = _check_num_objects(num_objects)
            assert gt_thw.dtype == torch.uint8, "a label map is uint8"
            self.gt = torch.where(gt_thw > self.k, torch.zeros_like(gt_thw), gt_thw).contiguous()      # objects that appear later: background
            present = torch.stack([(self.gt == o).flatten(1).any(1) for o in range(1, self.k + 1)])     # [k,T], once per sample
            self.present = present.to(torch.uint8).contiguous()
            self.present_host = present.cpu().numpy()                 # ONE sync per sample
            empty = ~present.any(0)                                   # frames without any object carry the NO_OBJECT token
            self.noobj = empty.to(torch.uint8).contiguous()
            self.object_quality = new((max_rounds, self.k, T), torch.float64)
            self.counts = new((self.k, T, 6), torch.int32)
            self._entry, self._which = "stcn_metrics_objects_round", (_ptr(self.present), self.k)
            self._object_rows = lambda r: (_ptr(self.object_quality[r]),)
        self._enqueue = getattr(_lib.lib(), self._entry)
        self.empty_host = empty.cpu().numpy()                         # ONE sync per sample: which frames carry the NO_OBJECT token
        self.annotated = torch.zeros(T, dtype=torch.uint8, device=self.dev)
        self.flags_host = torch.zeros(T, dtype=torch.uint8).pin_memory()
        self.scratch = None if metric == "j" else _boundary_scratch(self.k, T, H, W, self.dev)
        self.quality = new((max_rounds, T), torch.float64)
        self.select = new((max_rounds,), torch.int32)
        self.select_host = torch.empty((max_rounds,), dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event(blocking=True)
        self.rounds = 0
        self._scored = frozenset()

    def _fill_flags(self, frames, types):
        """What ``annotated`` on the device says of every frame: 1 = annotated (its ground truth is evaluated)."""
        if types is not None:
            raise ValueError("RoundScorer: annotation types are scored by TypedRoundScorer")
        self.flags_host[sorted(set(frames))] = 1

    def score(self, processor, annotated_frames, keep_gen: bool = True, incremental: bool = True, types=None):
        """Enqueue the evaluation of the round just propagated by ``processor`` and return (selected frame, gen): gen = uint8 [T,H,W] on the
        device (the evaluated masks; a fresh tensor when keep_gen, else a scratch that the next round overwrites).  ``annotated_frames``:
        every frame annotated so far, the one annotated in THIS round last.  ``incremental``: from the second round on only the frames the
        round can have changed - between the neighbouring annotated frames of the new one - are composed and counted again (the masks of the
        others are what they were: the engine only rewrites the probabilities of the frames it visits)."""
        import torch

        from . import _lib
        r = self.rounds
        if r >= self.quality.shape[0]:
            raise RuntimeError("RoundScorer: more rounds than max_rounds")
        lw, uw, lh, uh = processor.pad
        frames = [int(f) for f in annotated_frames]
        cur, others = frames[-1], set(frames[:-1]) - {frames[-1]}
        t0, t1 = 0, self.T
        if incremental and r > 0:
            t0 = max([f for f in others if f < cur] + [-1]) + 1
            t1 = min([f for f in others if f > cur] + [self.T])
        with torch.cuda.device(self.dev):
            self.flags_host.zero_()                                   # (the previous round's copy is done: every round ends in a wait)
            self._fill_flags(frames, types)
            self.annotated.copy_(self.flags_host, non_blocking=True)  # T bytes H2D from pinned memory
            prev = getattr(self, "_gen", None)
            if prev is None:
                gen = torch.empty((self.T, self.H, self.W), dtype=torch.uint8, device=self.dev)
                t0, t1 = 0, self.T
            elif keep_gen:
                gen = prev.clone() if (t0, t1) != (0, self.T) else torch.empty_like(prev)      # the frames outside [t0, t1) carry over
            else:
                gen = prev
            self._gen = gen
            _lib.check(self._enqueue(
                _stream(), _ptr(processor.masks), processor.nh, processor.nw, lh, lw, _ptr(self.gt), _ptr(self.annotated), *self._which,
                self.T, self.H, self.W, t0, t1, 1 if self.metric == "j" else 0, self.no_object, _ptr(gen), _ptr(self.scratch), _ptr(self.counts),
                *self._object_rows(r), _ptr(self.quality[r]), _ptr(self.select[r:r + 1])), self._entry)
            self.select_host[r:r + 1].copy_(self.select[r:r + 1], non_blocking=True)
            self.event.record()
            self.event.synchronize()                                  # blocking wait: the lane's host thread sleeps until the round is done
        self.rounds = r + 1
        self._scored = frozenset(frames)                             # what `annotated` and `counts` on the device describe: score_trial builds on it
        return int(self.select_host[r]), gen

    def score_trial(self, processor, annotated_frames, candidate: int, row: int) -> None:
        """Enqueue the evaluation of a TRIAL (``stcn_metrics_trial``; binary sessions): ``processor`` has just tried ``interact`` on frame
        ``candidate`` on top of the round scored last, whose annotated frames are ``annotated_frames``, and will take it back
        (``InferenceCore.undo``).  Row ``row`` of the trial table receives the per-frame quality a real round with that annotation would get,
        to the bit: the frames the trial can have changed - between the annotated neighbours of ``candidate`` - are composed and counted into
        scratch, the others take the counts of the last round.  No host wait; ``rounds``, ``counts``, the evaluated masks and ``annotated``
        stay what they were, so the next ``score()`` is that of a scorer that ran no trial.  The table holds T rows (``max_trials``)."""
        import torch

        from . import _lib
        if self.k is not None or self._entry != "stcn_metrics_round":
            raise RuntimeError("RoundScorer.score_trial: trials are scored for one-object (binary) sessions of mask annotations only")
        frames, cand, row = frozenset(int(f) for f in annotated_frames), int(candidate), int(row)
        if self.rounds == 0 or frames != self._scored:
            raise RuntimeError("RoundScorer.score_trial: a trial builds on the round scored last; annotated_frames are not that round's")
        if not 0 <= cand < self.T:
            raise ValueError(f"RoundScorer.score_trial: candidate frame {cand} outside [0, {self.T})")
        with torch.cuda.device(self.dev):
            if getattr(self, "trial_quality", None) is None:
                self.max_trials = self.T
                self.trial_quality = torch.empty((self.max_trials, self.T), dtype=torch.float64, device=self.dev)
                self.trial_host = torch.empty((self.max_trials, self.T), dtype=torch.float64).pin_memory()
                self._trial_gen = torch.empty((self.T * self.H * self.W,), dtype=torch.uint8, device=self.dev)
                self._trial_counts = torch.empty((self.T, 6), dtype=torch.int32, device=self.dev)
            if not 0 <= row < self.max_trials:
                raise RuntimeError(f"RoundScorer.score_trial: row {row} outside the trial table of {self.max_trials} rows")
            t0 = max([f for f in frames if f < cand] + [-1]) + 1
            t1 = min([f for f in frames if f > cand] + [self.T])
            lw, uw, lh, uh = processor.pad
            # the boundary map is scratch of a single call in score() too: trials share it
            _lib.check(_lib.lib().stcn_metrics_trial(
                _stream(), _ptr(processor.masks), processor.nh, processor.nw, lh, lw, _ptr(self.gt), _ptr(self.annotated), _ptr(self.noobj), cand,
                self.T, self.H, self.W, t0, t1, 1 if self.metric == "j" else 0, self.no_object, _ptr(self.counts), _ptr(self._trial_gen),
                _ptr(self.scratch), _ptr(self._trial_counts), _ptr(self.trial_quality[row])), "stcn_metrics_trial")

    def trial_rows(self, n: int):
        """float64 [n, T]: rows 0 .. n - 1 of the trial table - ONE device-to-host copy into pinned memory and one blocking-event wait (the
        host thread sleeps until every trial enqueued so far is done)."""
        import torch
        n = int(n)
        if n < 0 or n > getattr(self, "max_trials", 0):
            raise RuntimeError(f"RoundScorer.trial_rows: {n} rows asked of a trial table of {getattr(self, 'max_trials', 0)}")
        if n == 0:
            return np.zeros((0, self.T), np.float64)
        with torch.cuda.device(self.dev):
            self.trial_host[:n].copy_(self.trial_quality[:n], non_blocking=True)
            self.event.record()
            self.event.synchronize()
        return self.trial_host[:n].numpy().copy()

    def qualities(self):
        """float64 [rounds, T]: the per-frame quality of every round scored so far (one D2H copy)."""
        return self.quality[: self.rounds].cpu().numpy()

    def object_qualities(self):
        """float64 [rounds, k, T]: the per-object quality of every round of a multi-object session scored so far (one D2H copy)."""
        if self.object_quality is None:
            raise RuntimeError("RoundScorer.object_qualities: a one-object scorer (num_objects=None) has the rows of qualities() only")
        return self.object_quality[: self.rounds].cpu().numpy()


def _current_types(T: int, frames, types) -> np.ndarray:
    """uint8 [T]: the type of every frame after the annotations ``frames`` (with repeats) of the types ``types``: the last one counts."""
    frames, types = [int(f) for f in frames], [int(t) for t in types]
    if len(frames) != len(types) or any(t not in (1, 2) for t in types):
        raise ValueError("one type, 1 (mask) or 2 (clicks / box), per annotated frame")
    cur = np.zeros(T, np.uint8)
    for f, t in zip(frames, types):
        cur[f] = t
    return cur


class TypedRoundScorer(RoundScorer):
    """``RoundScorer`` for sessions that mix masks with cheaper annotations (``stcn_metrics_round_typed``; interactions/eval.py:57-64): a
    frame annotated with a mask (type 1) is evaluated with its ground truth, a frame annotated with clicks or a box (type 2) with the
    annotator's imperfect mask, which ``set_annotation`` stores in a device buffer the scorer owns.  One-object sessions only.
    ``score(processor, frames, types=...)`` takes every annotation so far, in order and WITH repeats - a type-2 frame stays selectable
    until it gets a mask - and the type of each; the type of a frame is that of its last annotation.  The frames a round can have changed are
    those between the annotated neighbours of the frame just (re)annotated, plus that frame (its evaluated mask changes with its type)."""

    def __init__(self, gt_thw, metric: str = "j", max_rounds: int = 64, no_object: float = 20.0):
        import torch
        super().__init__(gt_thw, metric, max_rounds, no_object)
        self.annot = torch.zeros((self.T, self.H, self.W), dtype=torch.uint8, device=self.dev)
        self._entry = "stcn_metrics_round_typed"
        from . import _lib
        self._enqueue = getattr(_lib.lib(), self._entry)
        self._which = (_ptr(self.annot), _ptr(self.noobj))

    def set_annotation(self, frame: int, mask) -> None:
        """The annotator's mask of a type-2 frame ([H,W], any dtype, on the scorer's device; non-zero = object): a device copy, no sync."""
        import torch
        m = mask.reshape(self.H, self.W)
        self.annot[int(frame)].copy_(m if m.dtype == torch.uint8 else (m > 0.5 if m.is_floating_point() else m != 0))

    def _fill_flags(self, frames, types):
        if types is None:
            raise ValueError("TypedRoundScorer.score: give the type of every annotation (types=...)")
        self.flags_host.copy_(__import__("torch").from_numpy(_current_types(self.T, frames, types)))


class HostTypedScorer:
    """The typed evaluation restated on the host - the yardstick of ``TypedRoundScorer`` and the scoring of the host route that
    tools/click_robot_cost.py measures against: every round downloads the engine's masks, composes the evaluated masks in NumPy
    (interactions/eval.py:57-64), counts with ``label_counts`` (NumPy / SciPy) and scores with ``_scores_from_counts``.  Same interface,
    same values to the bit, every frame recounted in every round."""

    def __init__(self, gt_thw, metric: str = "j", max_rounds: int = 64, no_object: float = 20.0):
        g = gt_thw.detach().cpu().numpy()
        self.gt = (g > 0.5 if g.dtype.kind == "f" else g != 0).astype(np.uint8)
        self.T, self.H, self.W = self.gt.shape
        self.dev = gt_thw.device
        self.metric, self.no_object = metric, float(no_object)
        self.empty_host = self.gt.reshape(self.T, -1).sum(1) == 0
        self.annot = np.zeros_like(self.gt)
        self.rows, self.gens = [], []
        self.rounds = 0

    def set_annotation(self, frame: int, mask) -> None:
        m = mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask)
        self.annot[int(frame)] = (m.reshape(self.H, self.W) != 0)

    def score(self, processor, annotated_frames, keep_gen: bool = True, incremental: bool = True, types=None):
        import torch
        cur = _current_types(self.T, annotated_frames, types)
        lw, uw, lh, uh = processor.pad
        seg = (processor.masks[:, 0, lh:processor.nh - uh, lw:processor.nw - uw] > 0).cpu().numpy().astype(np.uint8)
        gen = np.where(cur[:, None, None] == 1, self.gt, np.where(cur[:, None, None] == 2, self.annot, seg)).astype(np.uint8)
        c = label_counts(self.gt, gen, 1)[0]
        if self.metric == "j":
            q = np.array([0.0 if u == 0 else i / u for i, u in c[:, :2].tolist()], np.float64)
        else:
            q = _scores_from_counts(c)[:, 2].copy()
        q[self.empty_host] = self.no_object
        self.rows.append(q)
        self.counts = c
        self.rounds += 1
        return int(np.argmin(q)), torch.from_numpy(gen).to(self.dev)

    def qualities(self):
        return np.stack(self.rows) if self.rows else np.zeros((0, self.T), np.float64)
