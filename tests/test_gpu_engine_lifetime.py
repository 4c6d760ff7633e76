"""GPU: whatever an engine or a stage context takes from the device pool in its life goes back when it is destroyed.  The pool counts the
buffers it has handed out (stcn_pool_stats); every case takes that count as its baseline, lives through the paths that allocate, retire,
reuse and release - bank growth behind in-flight copies, journal entries dropped and reused, undo, clones, failures at both points of an
interaction, the frame-distance scratch, a stage context whose staging grows - drops everything, and must be back at the baseline: the
same number of buffers, the same bytes.  Engine cases run with the side stream, the second sweep and its workspace (lookahead 2) and with
none of them (lookahead 0)."""
import copy
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from eva_vos_amd import _lib, stages, synth

pytestmark = pytest.mark.gpu

T, H, W = 14, 128, 160                       # h16 * w16 = 80 >= top_k
OPTIONS = [{"lookahead": 2}, {"lookahead": 0}]
CYCLE = (0, 9, 4, 12, 6)


def pool_live():
    """(buffers, bytes) the pool has handed out, once every dropped object is finalized and the device idle."""
    gc.collect()
    torch.cuda.synchronize()
    n, b, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().stcn_pool_stats(C.byref(n), C.byref(b), C.byref(c)), "stcn_pool_stats")
    assert n.value >= 0 and b.value >= 0 and c.value >= 0
    return n.value, b.value


def _clip(k):
    return synth.synthetic_clip(T, H, W, seed=31).cuda(), synth.synthetic_mask(T, H, W, k, seed=32).cuda()


def _core(nets, img, k, options, depth):
    from mivos.inference_core import InferenceCore
    core = InferenceCore(nets[0], nets[1], img, k, mem_freq=5, engine_options=dict(options))
    core.set_undo_depth(depth)
    return core


def whole_life(nets, options, k):
    """Returns (core, clone) after the last interaction of each (tools and one-off comparisons of two builds call this too)."""
    img, msk = _clip(k)

    def go(core, f):
        if k == 1:
            core.interact(msk[:, f], f, download=False)
        else:                                  # scribble mode: background + k planes
            core.interact(torch.cat([1 - msk[:, f].sum(0, keepdim=True).clamp(0, 1), msk[:, f]], 0), f, scribble=True, download=False)

    core = _core(nets, img, k, options, depth=2)
    alive = pool_live()
    for i in range(18):                        # 18 certain slots: the 16-slot first generation of the bank is outgrown and retired
        go(core, CYCLE[i % len(CYCLE)])
    assert core.undo_state()["depth"] == 2 and core.undo_state()["entries"] == 2, "16 entries were dropped, their buffers retired or reused"
    core.undo(download=False)
    core.undo(download=False)
    clone = copy.deepcopy(core)
    go(core, 7)
    go(clone, 2)
    assert core.frame_distances().shape == (T, T)
    assert pool_live()[1] > alive[1], "a larger bank, a journal and a clone are alive"
    return core, clone


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: f"lookahead{o['lookahead']}")
def test_a_whole_engine_life_returns_every_buffer(nets, options, k):
    base = pool_live()
    core, clone = whole_life(nets, options, k)
    assert core.interacted == set(CYCLE) | {7} and clone.interacted == set(CYCLE) | {2}
    assert pool_live()[0] > base[0], "the pool's statistics see the engines"
    del core, clone
    assert pool_live() == base


@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: f"lookahead{o['lookahead']}")
def test_eighteen_interactions_outgrow_the_first_bank_generation(nets, options):
    """What the whole-life case rests on, shown on a core WITHOUT a journal: nothing but bank_reserve allocates after its construction (no
    frame distances are asked for), so the pool hands out more bytes only when the bank grows - and the 18 interactions of the whole-life
    case make it grow.  A 19th collects the retired generation (its event has fired: the device was idle), so the same number of buffers
    is out as at the start."""
    base = pool_live()
    img, msk = _clip(1)
    core = _core(nets, img, 1, options, depth=0)
    start = pool_live()
    for i in range(9):                         # as many certain slots as fit whatever the options: lookahead 2 keeps 4 + 2 slots for its sweeps
        core.interact(msk[:, CYCLE[i % len(CYCLE)]], CYCLE[i % len(CYCLE)], download=False)
    assert pool_live() == start, "9 certain slots fit the first generation of 16"
    for i in range(9, 18):
        core.interact(msk[:, CYCLE[i % len(CYCLE)]], CYCLE[i % len(CYCLE)], download=False)
    torch.cuda.synchronize()
    core.interact(msk[:, 7], 7, download=False)
    grown = pool_live()
    assert grown[1] > start[1] and grown[0] == start[0], (start, grown)
    del core
    assert pool_live() == base


@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: f"lookahead{o['lookahead']}")
def test_failure_paths_return_every_buffer(nets, options):
    base = pool_live()
    img, msk = _clip(1)
    core = _core(nets, img, 1, options, depth=1)
    core.interact(msk[:, 2], 2, download=False)
    _lib.check(_lib.lib().stcn_test_fail_at(-1))
    try:
        with pytest.raises(RuntimeError, match="bank_reserve"):
            core.interact(msk[:, 9], 9, download=False)
        core.interact(msk[:, 9], 9, download=False)                  # refused in its reservation: the engine stayed usable
        _lib.check(_lib.lib().stcn_test_fail_at(25))
        with pytest.raises(RuntimeError, match="injected fault"):
            core.interact(msk[:, 5], 5, download=False)
    finally:
        _lib.check(_lib.lib().stcn_test_fail_at(0))
    assert core.interacted == {2, 9} and core.undo_state()["entries"] == 0
    with pytest.raises(RuntimeError, match="failed state"):
        core.interact(msk[:, 5], 5, download=False)
    clone = copy.deepcopy(core)
    with pytest.raises(RuntimeError, match="failed state"):
        clone.interact(msk[:, 5], 5, download=False)
    core.reset()
    core.interact(msk[:, 5], 5, download=False)
    assert core.interacted == {5} and core.stats()["frames"] == T - 1
    del core, clone
    assert pool_live() == base


def test_a_clone_reserves_the_bank_of_its_source_and_continues_the_session(weights, nets, monkeypatch):
    """A clone's bank has its source's capacity - not that capacity plus the slots in front of the certain ones once more, which doubled
    it per generation of clones - and the clone carries the session on exactly as its source does.  T = 9 at mem_freq 1 with the dual
    sweep: 8 + 2 slots in front (bank_lo), 9 behind for a whole-clip sweep, 8 certain ones = 27, so a bank of 32."""
    from eva_vos_amd.params import PropagationNetwork
    from mivos.inference_core import InferenceCore
    for name in ("STCN_LOOKAHEAD", "STCN_DUAL_SWEEP"):
        monkeypatch.delenv(name, raising=False)
    prop = PropagationNetwork(top_k=16)          # 64 x 64 pixels: 16 bank rows per frame
    prop.load_state_dict(weights[0], strict=True)
    n, s = 9, 64
    img, msk = synth.synthetic_clip(n, s, s, seed=31).cuda(), synth.synthetic_mask(n, s, s, 1, seed=32).cuda()
    src = InferenceCore(prop.eval(), nets[1], img, 1, mem_freq=1, engine_options={"lookahead": 2})
    plan = src.engine_plan()
    assert (plan["dual_sweep"], plan["bank_lo"], plan["bank_initial"], plan["bank_cap"]) == (1, 10, 27, 32)
    src.interact(msk[:, 2], 2, download=False)
    clone = copy.deepcopy(src)
    assert clone.engine_plan() == plan
    grandchild = copy.deepcopy(clone)
    assert grandchild.engine_plan() == plan
    for f in (6, 4):
        assert np.array_equal(clone.interact(msk[:, f], f), src.interact(msk[:, f], f))
        assert torch.equal(clone.prob, src.prob)
    assert clone.engine_plan() == src.engine_plan() == plan, "three certain slots: nobody had to grow"


def test_a_stage_context_returns_every_buffer(nets):
    """A stage context has no engine options: one case.  The contexts live in the model object (an LRU the stage calls fill); the ones other
    tests left there are destroyed before the baseline is taken, ours afterwards."""
    prop = nets[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    model = stages._prop_model(prop, dev)

    stages._destroy_contexts(model)
    base = pool_live()
    g = torch.Generator(device="cuda").manual_seed(7)
    h, w = H // 16, W // 16

    def rnd(*shape):
        return torch.randn(shape, generator=g, device="cuda")

    q = rnd(1, 512, 2 * h, 2 * w), rnd(1, 256, 4 * h, 4 * w), rnd(1, 64, h, w), rnd(1, 512, h, w)
    sizes = []
    for frames in (1, 3):                      # the staging of one frame, then grown to three
        prob = stages.segment_with_query(prop, rnd(1, 64, frames, h, w), rnd(1, 512, frames, h, w), *q)
        assert prob.shape == (1, 1, H, W) and bool(torch.isfinite(prob).all())
        sizes.append(pool_live())
    assert sizes[0][0] > base[0] and sizes[1][0] == sizes[0][0] and sizes[1][1] > sizes[0][1], (base, sizes)
    assert stages._destroy_contexts(model) == 1
    assert pool_live() == base
