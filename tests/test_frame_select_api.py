"""CPU: the frame-distance entry points (csrc/frame_select.hip behind stcn_frame_* / stcn_engine_frame_*) - symbols, host-side refusals,
the launch plan - and the host half of the l2_mask policy (eva_vos_amd.frame_select.farthest_frame, eval_driver)."""
import ctypes as C

import numpy as np
import pytest

from eva_vos_amd import _lib, eval_driver, frame_select

NAMES = ("stcn_frame_gram_scratch", "stcn_frame_sq_distances", "stcn_engine_frame_distances", "stcn_engine_frame_features")


def test_the_four_symbols_are_exported_and_declared():
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert _lib.PROTOTYPES["stcn_frame_sq_distances"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p])
    assert _lib.PROTOTYPES["stcn_engine_frame_features"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])


def test_every_refusal_happens_on_the_host_and_names_the_value():
    """Host pointers that are never dereferenced (16: aligned, non-null): each bad argument returns STCN_E_INVALID with its value in the message."""
    lib = _lib.lib()
    one = C.c_void_p(16)

    def refused(*args):
        assert lib.stcn_frame_sq_distances(None, *args) == -1, args
        return lib.stcn_last_error().decode()

    assert "null" in refused(None, 5, 64, 64, one, one)
    assert "null" in refused(one, 5, 64, 64, None, one)
    assert "null" in refused(one, 5, 64, 64, one, None)
    assert "T=0 " in refused(one, 0, 64, 64, one, one)
    assert "T=107 " in refused(one, 107, 64, 64, one, one) and "106" in lib.stcn_last_error().decode()
    assert "T=-3 " in refused(one, -3, 64, 64, one, one)
    assert "K=0 " in refused(one, 5, 0, 64, one, one)
    assert "K=2 " in refused(one, 5, 2, 64, one, one)
    assert "K=62 " in refused(one, 5, 62, 64, one, one)
    assert "stride=60 " in refused(one, 5, 64, 60, one, one) and "K=64" in lib.stcn_last_error().decode()
    assert "stride=66 " in refused(one, 5, 64, 66, one, one)
    assert "16-byte aligned" in refused(C.c_void_p(20), 5, 64, 64, one, one)
    for fn in (lib.stcn_engine_frame_distances, lambda e, p: lib.stcn_engine_frame_features(e, 0, p)):
        assert fn(None, one) == -1 and b"null" in lib.stcn_last_error()
    assert lib.stcn_frame_gram_scratch(107, 64, None, None) == -1 and b"T=107" in lib.stcn_last_error()
    assert lib.stcn_frame_gram_scratch(5, 6, None, None) == -1 and b"K=6" in lib.stcn_last_error()
    assert lib.stcn_frame_gram_scratch(5, 64, None, None) == 0            # either out pointer may be null


@pytest.mark.parametrize("T", [1, 16, 17, 106])
@pytest.mark.parametrize("K", [4, 252, 4100, 1658880])
def test_plan_covers_k_and_sizes_the_scratch(T, K):
    nbytes, slices = frame_select.gram_plan(T, K)
    nt = (T + 15) // 16
    pairs = nt * (nt + 1) // 2
    assert slices >= 1 and nbytes == slices * pairs * 2048
    # the slice length is not exported; it follows from the plan's rule (whole k-steps of 32, as few per slice as the slice budget allows):
    # the slices must cover K and the last one must not be empty
    steps = -(-K // 32)
    per = -(-steps // min(steps, 512))
    length = per * 32
    assert slices == -(-steps // per) and slices <= 512
    assert slices * length >= K and (slices - 1) * length < K


def test_plan_refuses_107_frames():
    with pytest.raises(RuntimeError, match="T=107"):
        frame_select.gram_plan(107, 4100)


def _farthest_loop(dist, annotated):
    """get_frame_l2 / get_min_l2_dist written out (interactions/policies.py:21-36,69-88) on a distance matrix."""
    best, frame = -np.inf, -1
    for i in range(dist.shape[0]):
        lo = np.inf
        for a in annotated:
            if dist[i, a] < lo:
                lo = dist[i, a]
        if lo > best:
            best, frame = lo, i
    return frame


def test_farthest_frame_is_the_reference_rule():
    rng = np.random.default_rng(3)
    for T in (2, 5, 12, 40):
        x = rng.normal(size=(T, 7))
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
        for n in (1, 2, T // 2 + 1):
            ann = rng.choice(T, size=min(n, T), replace=False).tolist()
            got = frame_select.farthest_frame(d, ann)
            assert got == _farthest_loop(d, ann) and (got not in ann or len(ann) == T)
        assert frame_select.farthest_frame(d, list(range(T))) == 0 == _farthest_loop(d, list(range(T)))       # all annotated: every minimum is 0
        assert frame_select.farthest_frame(d, [T - 1]) == int(np.argmax(d[:, T - 1]))                         # a single annotated frame
    # an exact tie: frames 1 and 3 are equally far from frame 0, frame 2 is nearer - the first index wins (strict >)
    d = np.array([[0., 4., 1., 4.], [4., 0., 9., 16.], [1., 9., 0., 9.], [4., 16., 9., 0.]])
    assert frame_select.farthest_frame(d, [0]) == 1 == _farthest_loop(d, [0])
    assert frame_select.farthest_frame(d, [0, 0]) == 1                                                          # a re-annotated frame counts once
    assert frame_select.farthest_frame(d[::-1, ::-1].copy(), [3]) == 0


def test_l2_mask_is_a_policy_of_both_modes():
    assert "l2_mask" in eval_driver.POLICIES and "l2_mask" in eval_driver.MULTI_OBJECT_POLICIES


def test_l2_mask_refuses_a_clip_longer_than_the_key_cache_before_it_touches_the_processor():
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the processor was touched ({name})")

    sample = {"num_frames": 107, "name": "long__1", "video": "long"}
    with pytest.raises(ValueError, match="106"):
        eval_driver.run_policy("l2_mask", Untouchable(), sample, 3)
    with pytest.raises(ValueError, match="106"):
        eval_driver.run_policy("l2_mask", Untouchable(), dict(sample, num_objects=2), 3, multi_object=True)
