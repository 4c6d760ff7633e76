"""Cases for the click robot (csrc/robot.hip) at the places its labelling and its arithmetic can go wrong, and a host restatement of the
pixel pairs its two labelling kernels visit.  Host only (NumPy / SciPy): tests/test_robot_cases.py checks that every case does what it is
named for, tests/test_gpu_robot_extents.py runs them on the device against ``robots.host_click_record``.

A case is ``(pred, gt, mode, iou)`` as ``robots.host_click_record`` takes it.  The error map of a pair of masks is three-valued:
0 = agree, 1 = false positive, 2 = false negative; pixels join only inside a class."""
import functools
from typing import Callable, NamedTuple

import numpy as np

from eva_vos_amd import robots

TILE = 32       # robot.hip: TILE_W = TILE_H

SEAM_KINDS = ("W_seam", "N_seam", "NW_vseam", "NW_hseam", "NW_corner", "NE_vseam", "NE_hseam", "NE_corner")
KINDS = ("W_in", "N_in", "NW_in", "NE_in") + SEAM_KINDS


def error_map(pred, gt) -> np.ndarray:
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    return np.where(p == g, 0, np.where(p, 1, 2)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the links of the labelling, by kind
def _pairs(cls, dy, dx, where):
    """[k,2] linear indices (pixel, its neighbour at (y + dy, x + dx)) over the pixels of ``where`` whose neighbour is inside the frame and
    of the same non-zero class."""
    W = cls.shape[1]
    y, x = np.nonzero(where & (cls != 0))
    ny, nx = y + dy, x + dx
    ok = (ny >= 0) & (nx >= 0) & (nx < W)
    y, x, ny, nx = y[ok], x[ok], ny[ok], nx[ok]
    same = cls[ny, nx] == cls[y, x]
    return np.stack([y[same] * W + x[same], ny[same] * W + nx[same]], 1).astype(np.int64)


def _local(cls):
    H, W = cls.shape
    ly, lx = np.meshgrid(np.arange(H) % TILE, np.arange(W) % TILE, indexing="ij")
    return ly, lx


def link_edges(cls) -> dict:
    """Every same-class pair (pixel, its W / N / NW / NE neighbour) of a three-valued error map, keyed by where the pair lies relative to
    the 32 x 32 tiles of the labelling: inside one tile, across a vertical seam (the pixel is in the first - for NE the last - column of its
    tile), across a horizontal seam (first row), or across a tile corner (both)."""
    cls = np.asarray(cls)
    ly, lx = _local(cls)
    top, left, right = ly == 0, lx == 0, lx == TILE - 1
    return {
        "W_in": _pairs(cls, 0, -1, ~left), "W_seam": _pairs(cls, 0, -1, left),
        "N_in": _pairs(cls, -1, 0, ~top), "N_seam": _pairs(cls, -1, 0, top),
        "NW_in": _pairs(cls, -1, -1, ~left & ~top), "NW_vseam": _pairs(cls, -1, -1, left & ~top),
        "NW_hseam": _pairs(cls, -1, -1, ~left & top), "NW_corner": _pairs(cls, -1, -1, left & top),
        "NE_in": _pairs(cls, -1, 1, ~right & ~top), "NE_vseam": _pairs(cls, -1, 1, right & ~top),
        "NE_hseam": _pairs(cls, -1, 1, ~right & top), "NE_corner": _pairs(cls, -1, 1, right & top),
    }


def kernel_edges(cls) -> np.ndarray:
    """The pairs the two kernels join, [k,2], restated from robot.hip.
    ccl_tile_kernel, inside a tile: W when lx > 0; with ly > 0, N when the north pixel is of the same class, otherwise NW (lx > 0) and
    NE (lx < 31) - a north neighbour of the same class joins its own W and E neighbours itself.
    ccl_merge_kernel, across tiles: W when lx == 0; with y > 0, north of the same class (in this tile or not): N when ly == 0 and nothing
    else; otherwise NW when lx == 0 or ly == 0, NE when lx == 31 or ly == 0."""
    cls = np.asarray(cls)
    H, W = cls.shape
    ly, lx = _local(cls)
    north = np.zeros((H, W), bool)
    north[1:] = (cls[1:] == cls[:-1]) & (cls[1:] != 0)
    tile = [_pairs(cls, 0, -1, lx > 0),
            _pairs(cls, -1, 0, (ly > 0) & north),
            _pairs(cls, -1, -1, (ly > 0) & ~north & (lx > 0)),
            _pairs(cls, -1, 1, (ly > 0) & ~north & (lx < TILE - 1))]
    merge = [_pairs(cls, 0, -1, lx == 0),
             _pairs(cls, -1, 0, north & (ly == 0)),
             _pairs(cls, -1, -1, ~north & ((lx == 0) | (ly == 0))),
             _pairs(cls, -1, 1, ~north & ((lx == TILE - 1) | (ly == 0)))]
    return np.concatenate(tile + merge)


def label_from_edges(cls, edges):
    """(components, labels [H,W] int64: 0 where the class is 0, else 1 + the rank of the component's first pixel in raster order - the
    numbering of scipy.ndimage.label)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    cls = np.asarray(cls)
    n = cls.size
    graph = coo_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    on = np.flatnonzero(cls.ravel() != 0)
    lab = np.zeros(n, np.int64)
    if on.size:
        _, first, inv = np.unique(comp[on], return_index=True, return_inverse=True)      # first: the first pixel of each component
        lab[on] = np.argsort(np.argsort(first))[inv] + 1
    return int(lab.max()), lab.reshape(cls.shape)


def _edges_without(cls, kind):
    return np.concatenate([e for k, e in link_edges(cls).items() if k != kind])


def components_without(cls, kind=None) -> int:
    """Components of both error classes together when the links of one kind are left out (None: all links)."""
    return label_from_edges(cls, _edges_without(cls, kind))[0]


def record_without(case, kind):
    """The host record of a case whose labelling has lost the links of one kind: ``robots.host_click_record`` with its labelling step
    replaced (the selection, the centroid and the fallback stay the host's own)."""
    def largest(region):
        cls = region.astype(np.uint8)
        n, lab = label_from_edges(cls, _edges_without(cls, kind))
        if n == 0:
            return 0, 0, None
        sizes = np.bincount(lab.ravel())[1:]
        return n, int(sizes.max()), lab == int(np.argmax(sizes)) + 1
    pred, gt, mode, iou = case
    saved = robots._largest_component
    robots._largest_component = largest
    try:
        return robots.host_click_record(pred, gt, mode, iou)[0]
    finally:
        robots._largest_component = saved


# ------------------------------------------------------------------------------------------------ builders
def _as_class(shape, mask, cls):
    """false negative (2): the object is `mask` and nothing is predicted; false positive (1): `mask` is predicted and there is no object."""
    m, z = mask.astype(np.uint8), np.zeros(shape, np.uint8)
    return (z, m) if cls == 2 else (m, z)


def _interact(pred, gt, iou=None):
    return pred, gt, robots.INTERACT, iou


def diagonal_blocks(H, W, cy, cx, direction, cls):
    """A 4x4 and a 3x5 block that touch only in one diagonal pixel pair at (cy, cx): NW - the pair (cy, cx) / (cy - 1, cx - 1);
    NE - the pair (cy, cx - 1) / (cy - 1, cx)."""
    m = np.zeros((H, W), bool)
    if direction == "NW":
        m[cy - 4:cy, cx - 4:cx] = True
        m[cy:cy + 3, cx:cx + 5] = True
    else:
        m[cy:cy + 4, cx - 4:cx] = True
        m[cy - 3:cy, cx:cx + 5] = True
    return _interact(*_as_class((H, W), m, cls))


def bridge(axis):
    """Two blocks joined by a one-pixel line that crosses the seam between tiles 0 and 1 straight on: axis 1 a W link, axis 0 an N link."""
    m = np.zeros((64, 64), bool)
    m[10:14, 26:30] = m[9:15, 34:38] = True
    m[12, 30:34] = True
    return _interact(*_as_class((64, 64), m.T.copy() if axis == 0 else m, 2))


def staircase(direction):
    """Single pixels along a diagonal of a 130 x 131 frame, through three tile corners: every pixel hangs on its neighbour by one link."""
    m = np.zeros((130, 131), bool)
    k = np.arange(2, 126)
    m[k, k if direction == "NW" else 127 - k] = True        # NW: (32,32) (64,64) (96,96); NE: (32,95) (64,63) (96,31)
    return _interact(*_as_class(m.shape, m, 2))


def serpentine():
    """256 x 256: the even rows full, on the odd rows one end pixel, alternating - one component of 32896 pixels that crosses each of the
    seven vertical seams on 128 rows; its parent chains are as long as the rows."""
    m = np.zeros((256, 256), bool)
    m[0::2] = True
    m[1::4, 255] = True
    m[3::4, 0] = True
    return _interact(*_as_class(m.shape, m, 2))


def chessboard():
    """17 x 17 squares around the tile corner (32, 32), the two error classes alternating: the four straight neighbours of a pixel are of
    the other class, the diagonal ones of its own - two interleaved components (145 and 144 pixels) that hold together by diagonals alone."""
    pred, gt = np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8)
    y, x = np.mgrid[24:41, 24:41]
    even = (y + x) % 2 == 0
    pred[y[even], x[even]] = 1
    gt[y[~even], x[~even]] = 1
    return _interact(pred, gt, 0.0)


def stripes():
    """Columns of the two error classes alternating around the tile corner (32, 32): every diagonal neighbour is of the OTHER class and
    must not join - nine false-positive and eight false-negative columns, each one component."""
    pred, gt = np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8)
    for x in range(24, 41):
        (pred if x % 2 == 0 else gt)[24:41, x] = 1
    return _interact(pred, gt, 0.0)


def noise(H, W, seed, mode=robots.INTERACT, p=0.5):
    g = np.random.default_rng(seed)
    return (g.random((H, W)) < p).astype(np.uint8), (g.random((H, W)) < p).astype(np.uint8), mode, None


def runs(H, W):
    """One run of pixels in raster order per mask: the false negative [n/5, n/2), agreement [n/2, 4n/5), the false positive [4n/5, 9n/10)."""
    n = H * W
    pred, gt = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    gt[n // 5:4 * n // 5] = 1
    pred[n // 2:9 * n // 10] = 1
    return _interact(pred.reshape(H, W), gt.reshape(H, W), 0.0)


def one_by_one(p, g):
    return _interact(np.full((1, 1), p, np.uint8), np.full((1, 1), g, np.uint8), 0.0)


def _line(n, axis, values):
    return values.reshape((1, n) if axis == 1 else (n, 1))


def line_all_false_negative(n, axis):
    return _interact(_line(n, axis, np.zeros(n, np.uint8)), _line(n, axis, np.ones(n, np.uint8)))


def line_false_positive_far_object(n, axis):
    """Everything but the last pixel is predicted, the object is the last pixel alone: two clicks, the second at the far end."""
    pred, gt = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    pred[-1], gt[-1] = 0, 1
    return _interact(_line(n, axis, pred), _line(n, axis, gt), 0.0)


def line_two_runs(n, axis, tied, mode):
    """The object in two runs of 1000 pixels at the two ends of a line of n = 2^18: the median falls on the background half-way, more than
    2^16 pixels (d^2 > 2^32) from both.  Not tied: the runs are [0, 1000) and [n - 1000, n), the median (n - 1) / 2 is cut to n / 2 - 1, so
    the first run is nearer by one.  Tied: the second run one pixel earlier, the median exactly n / 2 - 1: the first in raster order wins."""
    gt = np.zeros(n, np.uint8)
    gt[:1000] = 1
    if tied:
        gt[n - 1001:n - 1] = 1
    else:
        gt[n - 1000:] = 1
    g = _line(n, axis, gt)
    return (g.copy() if mode == robots.INTERACT else np.zeros_like(g)), g, mode, None


BIG = 4096


def big_squares():
    """2^24 pixels: two 4x4 false negatives whose first pixels lie above 2^23 (equal: the first in raster order is taken), a smaller one near
    the top, and a 4x4 false positive (equal to them: the false positive is clicked, the false negative goes along at iou 0)."""
    pred, gt = np.zeros((BIG, BIG), np.uint8), np.zeros((BIG, BIG), np.uint8)
    gt[4090:4094, 10:14] = gt[4090:4094, 3000:3004] = 1
    gt[5:7, 100:103] = 1
    pred[4080:4084, 2000:2004] = 1
    return _interact(pred, gt, 0.0)


def big_last_pixel():
    """The false positive is the very last pixel (its root 2^24 - 1: the low bits of its key are all zero), the false negative one pixel."""
    pred, gt = np.zeros((BIG, BIG), np.uint8), np.zeros((BIG, BIG), np.uint8)
    pred[BIG - 1, BIG - 1] = 1
    gt[2048, 7] = 1
    return _interact(pred, gt, 0.0)


def big_rectangle():
    """A filled 1200 x 1200 false negative in the bottom-right corner: 1.44M pixels on 38 x 38 tiles, both coordinate sums about 5.0e9."""
    pred, gt = np.zeros((BIG, BIG), np.uint8), np.zeros((BIG, BIG), np.uint8)
    gt[BIG - 1200:, BIG - 1200:] = 1
    return _interact(pred, gt)


def middle_noise(H, W, odd, mode):
    """pred == gt, a sparse object (2 % of the pixels) with an odd or an even number of pixels: no error, the middle click."""
    gt = (np.random.default_rng(H * 1000 + W).random((H, W)) < 0.02).astype(np.uint8)
    if int(gt.sum()) % 2 != int(odd):
        gt[H // 2, W // 2] ^= 1
    return (gt.copy() if mode == robots.INTERACT else np.zeros_like(gt)), gt, mode, None


def middle_block(H, W, even, mode):
    """A filled block whose medians lie ON it (the click does not move) in the LAST histogram entry of a thread of the order statistic
    (entry % chunk == chunk - 1 with chunk = ceil(length / 256)); `even`: one row and one column more, so that the two middle pixels lie
    in two rows and two columns, the second in the next thread's first entry."""
    gt = np.zeros((H, W), np.uint8)
    cy, cx = (v // 2 + 5 - (v // 2 + 5 + 1) % ((v + 255) // 256) for v in (H, W))
    gt[cy - 7:cy + 8 + even, cx - 9:cx + 10 + even] = 1
    return (gt.copy() if mode == robots.INTERACT else np.zeros_like(gt)), gt, mode, None


def middle_l_shape(H, W, mode):
    """An L turned by 45 degrees (two diagonal arms, three pixels thick, that open to the right), off the centre of the frame: the medians
    meet between the arms, on the background, and the click moves to the nearest object pixel."""
    gt = np.zeros((H, W), np.uint8)
    arm, cy, x0 = min(H, W) // 3, H // 2 + 7, W // 2
    for k in range(arm):
        gt[cy + k:cy + k + 3, x0 + k] = 1
        gt[cy - k - 3:cy - k, x0 + k] = 1
    return (gt.copy() if mode == robots.INTERACT else np.zeros_like(gt)), gt, mode, None


# ------------------------------------------------------------------------------------------------ the table
class Case(NamedTuple):
    group: str                      # seam, thin, line, big, middle
    build: Callable
    decisive: tuple = ()            # seam kinds whose loss changes the components and the record
    claims: tuple = ()              # sum>2^32, size>=2^16, d2>2^32, tie, moved, empty


CASES = {}


def _add(name, group, build, decisive=(), claims=()):
    assert name not in CASES
    CASES[name] = Case(group, build, tuple(decisive), tuple(claims))


for _d in ("NW", "NE"):
    for _cls, _tag in ((2, "fn"), (1, "fp")):
        _add(f"corner_{_d}_{_tag}_64x64", "seam", functools.partial(diagonal_blocks, 64, 64, 32, 32, _d, _cls), [f"{_d}_corner"])
    _add(f"corner_{_d}_fn_70x101", "seam", functools.partial(diagonal_blocks, 70, 101, 64, 64 if _d == "NW" else 96, _d, 2), [f"{_d}_corner"])
    _add(f"corner_{_d}_fp_70x101", "seam", functools.partial(diagonal_blocks, 70, 101, 32, 96 if _d == "NW" else 64, _d, 1), [f"{_d}_corner"])
    _add(f"vseam_{_d}_64x64", "seam", functools.partial(diagonal_blocks, 64, 64, 43, 32, _d, 2), [f"{_d}_vseam"])
    _add(f"hseam_{_d}_64x64", "seam", functools.partial(diagonal_blocks, 64, 64, 32, 45, _d, 1), [f"{_d}_hseam"])
    _add(f"staircase_{_d}_130x131", "seam", functools.partial(staircase, _d), [f"{_d}_corner"])
_add("bridge_W_64x64", "seam", functools.partial(bridge, 1), ["W_seam"])
_add("bridge_N_64x64", "seam", functools.partial(bridge, 0), ["N_seam"])
_add("serpentine_256x256", "seam", serpentine, ["W_seam"])
_add("chessboard_64x64", "seam", chessboard)
_add("stripes_64x64", "seam", stripes, ["N_seam"])

for _p in (0, 1):
    for _g in (0, 1):
        _add(f"one_pixel_pred{_p}_gt{_g}", "thin", functools.partial(one_by_one, _p, _g), claims=["empty"] if (_p, _g) == (0, 0) else [])
for _i, (_H, _W) in enumerate(((1, 70), (70, 1), (2, 65), (31, 31), (32, 32), (33, 33))):
    _add(f"noise_{_H}x{_W}", "thin", functools.partial(noise, _H, _W, 100 + _i))
    _add(f"noise_middle_{_H}x{_W}", "thin", functools.partial(noise, _H, _W, 200 + _i, robots.MIDDLE, 0.3))
    _add(f"runs_{_H}x{_W}", "thin", functools.partial(runs, _H, _W))

for _axis, _tag in ((1, "row"), (0, "column")):
    _add(f"{_tag}_2p17_false_negative", "line", functools.partial(line_all_false_negative, 1 << 17, _axis), claims=["size>=2^16", "sum>2^32"])
    _add(f"{_tag}_2p17_false_positive", "line", functools.partial(line_false_positive_far_object, 1 << 17, _axis), claims=["size>=2^16", "sum>2^32"])
    _add(f"{_tag}_2p18_two_runs", "line", functools.partial(line_two_runs, 1 << 18, _axis, False, robots.MIDDLE), claims=["d2>2^32", "moved"])
    _add(f"{_tag}_2p18_two_runs_tied", "line", functools.partial(line_two_runs, 1 << 18, _axis, True, robots.MIDDLE), claims=["d2>2^32", "moved", "tie"])
    _add(f"{_tag}_2p18_two_runs_tied_interact", "line", functools.partial(line_two_runs, 1 << 18, _axis, True, robots.INTERACT),
         claims=["d2>2^32", "moved", "tie"])

_add("big_squares", "big", big_squares)
_add("big_last_pixel", "big", big_last_pixel)
_add("big_rectangle", "big", big_rectangle, claims=["size>=2^16", "sum>2^32"])

for _H, _W in ((255, 257), (256, 256), (257, 255), (511, 513), (480, 854)):
    _add(f"middle_odd_{_H}x{_W}", "middle", functools.partial(middle_noise, _H, _W, True, robots.INTERACT))
    _add(f"middle_even_{_H}x{_W}", "middle", functools.partial(middle_noise, _H, _W, False, robots.MIDDLE))
    _add(f"middle_block_odd_{_H}x{_W}", "middle", functools.partial(middle_block, _H, _W, 0, robots.MIDDLE))
    _add(f"middle_block_even_{_H}x{_W}", "middle", functools.partial(middle_block, _H, _W, 1, robots.INTERACT))
for _H, _W in ((257, 255), (511, 513), (480, 854)):
    _add(f"middle_l_shape_{_H}x{_W}", "middle", functools.partial(middle_l_shape, _H, _W, robots.INTERACT), claims=["moved"])
    _add(f"middle_l_shape_mode_{_H}x{_W}", "middle", functools.partial(middle_l_shape, _H, _W, robots.MIDDLE), claims=["moved"])


def names(group):
    return [n for n, c in CASES.items() if c.group == group]


@functools.lru_cache(maxsize=None)
def get(name):
    """(pred, gt, mode, iou) of a case, built once; the arrays are read-only."""
    pred, gt, mode, iou = CASES[name].build()
    for a in (pred, gt):
        a.setflags(write=False)
    return pred, gt, mode, iou


@functools.lru_cache(maxsize=None)
def host(name):
    """(record as a list, component) of the host restatement, computed once per process."""
    rec, comp = robots.host_click_record(*get(name))
    comp.setflags(write=False)
    return rec.tolist(), comp
