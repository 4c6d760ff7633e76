"""CPU: the schedule of a sweep is pure host code (plan_sweep, through stcn_test_sweep_plan) - checked against the rule in closed form,
not against a copy of the planner's loop.

The span = |closest - idx| - 1 frames of a sweep sit at distances 1 .. span from idx.  A frame goes into the memory bank when it is not the
sweep's last and lies mem_freq frames from the last inserted one (from idx at first): exactly the distances d with d % mem_freq == 0 and
d < span.  Every inserting distance ends a segment, and so does span; inside a segment the groups are consecutive chunks of `cap` frames,
the last one holding the remainder; a group inserts exactly when it ends at an inserting distance."""
import ctypes as C

import pytest

MEM_FREQS = (1, 2, 3, 5, 7, 12, 50)
CAPS = tuple(range(1, 9))
SPANS = tuple(range(0, 61))


def sweep_plan(idx, closest, mem_freq, cap):
    """[(first frame in sweep order, lowest frame, frames, inserts)] of the sweep"""
    from eva_vos_amd import _lib
    lib = _lib.lib()
    count = C.c_int32(-1)
    _lib.check(lib.stcn_test_sweep_plan(idx, closest, mem_freq, cap, None, 0, C.byref(count)), "stcn_test_sweep_plan")
    n = count.value
    out = (C.c_int32 * (4 * max(n, 1)))()
    _lib.check(lib.stcn_test_sweep_plan(idx, closest, mem_freq, cap, out, n, C.byref(count)), "stcn_test_sweep_plan")
    assert count.value == n
    return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


def expected_groups(span, mem_freq, cap):
    """[(first distance, frames, inserts)] from the closed form"""
    inserting = [d for d in range(1, span + 1) if d % mem_freq == 0 and d < span]
    ends = inserting + ([span] if span > 0 else [])
    groups, start = [], 1
    for end in ends:                                     # segment: distances start .. end
        n = end - start + 1
        sizes = [cap] * (n // cap) + ([n % cap] if n % cap else [])
        for i, g in enumerate(sizes):
            groups.append((start, g, end in inserting and i == len(sizes) - 1))
            start += g
    return groups


def check_sweep(idx, closest, mem_freq, cap):
    span, step = abs(closest - idx) - 1, 1 if closest > idx else -1
    got = sweep_plan(idx, closest, mem_freq, cap)
    want = expected_groups(span, mem_freq, cap)
    assert [(abs(first - idx), G, bool(ins)) for first, _, G, ins in got] == want, (idx, closest, mem_freq, cap)
    # the groups partition the distances 1 .. span in order
    assert [d for first, _, G, _ in got for d in range(abs(first - idx), abs(first - idx) + G)] == list(range(1, span + 1))
    for first, t_lo, G, ins in got:
        frames = [first + j * step for j in range(G)]
        assert 1 <= G <= cap and t_lo == min(frames), (idx, closest, mem_freq, cap)
        assert all(min(idx, closest) < t < max(idx, closest) for t in frames)
        assert bool(ins) == (abs(frames[-1] - idx) % mem_freq == 0 and abs(frames[-1] - idx) < span)
    # the bank slots a sweep reserves for its temporaries (span // mem_freq + 1) always hold what it inserts
    assert sum(ins for *_, ins in got) <= span // mem_freq


@pytest.mark.parametrize("mem_freq", MEM_FREQS)
@pytest.mark.parametrize("forward", (True, False), ids=("forward", "backward"))
def test_sweep_plan_follows_the_insertion_rule(mem_freq, forward):
    for span in SPANS:
        for cap in CAPS:
            idx = 3 if forward else span + 4                 # backward sweeps end at frame 3 too (closest = 3: an interacted frame)
            check_sweep(idx, idx + span + 1 if forward else idx - span - 1, mem_freq, cap)


@pytest.mark.parametrize("T,mem_freq,idx", [(30, 12, 17), (9, 50, 0), (3, 5, 1), (2, 1, 0)])
def test_sweep_plan_of_the_large_mem_freq_and_tiny_clip_shapes(T, mem_freq, idx):
    """the first-interaction sweeps of test_decode_groups_with_large_mem_freq_and_tiny_clips: to both ends of the clip, at every cap the
    engine can resolve (min(mem_freq, 8) and below)"""
    for cap in range(1, min(mem_freq, 8) + 1):
        check_sweep(idx, T, mem_freq, cap)
        check_sweep(idx, -1, mem_freq, cap)


def test_sweep_plan_rejects_bad_arguments():
    from eva_vos_amd import _lib
    lib = _lib.lib()
    count = C.c_int32(0)
    assert lib.stcn_test_sweep_plan(0, 5, 0, 1, None, 0, C.byref(count)) != 0
    assert lib.stcn_test_sweep_plan(0, 5, 1, 0, None, 0, C.byref(count)) != 0
    assert lib.stcn_test_sweep_plan(0, 5, 1, 1, None, 2, C.byref(count)) != 0
    assert lib.stcn_test_sweep_plan(0, 5, 1, 1, None, 0, None) != 0
