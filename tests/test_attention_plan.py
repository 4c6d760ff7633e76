"""CPU: the launch plan of the fusion attention read is pure host code (attention_plan, through stcn_attention_plan) - restated here and
checked, for every frame of 1 .. 40000 positions, against what the kernels need of it (memread.hip):
  * colmax_pass_kernel writes 16 group maxima per (chunk, query) into a scratch that is [256][hw] wherever it is allocated (the hook, the
    stage context, the engine), and attention_pass_kernel reads NCeff * 16 of them: NCeff * 16 <= 256;
  * attention_finalize_kernel sums the partial sums of NCeff chunks of a scratch sized for 16: NCeff <= 16;
  * the chunks of spc steps cover the steps, and none is empty - an empty chunk would hand 16 maxima of -inf on (harmless) and a partial
    sum that nobody wrote to the finalize (not harmless).
The shapes of test_gpu_attention.py are pinned to the regime each was chosen for, so that a change of the plan cannot silently move a case."""
import ctypes as C

import pytest

# (h16, w16) of test_gpu_attention.py -> what the plan is at that shape: steps, qblocks, NC, spc, NCeff
SHAPES = {
    (1, 1): (1, 1, 1, 1, 1), (1, 3): (1, 1, 1, 1, 1), (3, 5): (1, 1, 1, 1, 1),      # one step, one partly filled query group
    (5, 7): (1, 1, 1, 1, 1),                # 35 = 2 * 16 + 3: the third wave has 3 valid columns, the fourth is idle
    (8, 8): (1, 1, 1, 1, 1),                # exactly one step
    (5, 13): (2, 2, 2, 1, 2),               # a second step that holds one row
    (32, 32): (16, 16, 16, 1, 16),          # every chunk the scratch has room for, one step each
    (23, 45): (17, 17, 16, 2, 9),           # two steps per chunk, the last chunk one
    (30, 54): (26, 26, 16, 2, 13),          # 480p: fewer chunks launched than asked for
    (33, 63): (33, 33, 16, 3, 11),          # the first frame size beyond 2048 positions
    (45, 80): (57, 57, 9, 7, 9),            # NC from 512 / qblocks; the last chunk one step
    (68, 120): (128, 128, 4, 32, 4),        # 1080p class
}
NAMES = ("steps", "qblocks", "NC", "spc", "NCeff")


def plan(hw):
    from eva_vos_amd import _lib
    pl = (C.c_int32 * 5)()
    _lib.check(_lib.lib().stcn_attention_plan(hw, pl), "stcn_attention_plan")
    return tuple(pl)


def restated(hw):
    steps, qblocks = -(-hw // 64), -(-hw // 64)
    NC = min(-(-512 // qblocks), 16, steps)
    spc = -(-steps // NC)
    return steps, qblocks, NC, spc, -(-steps // spc)


def test_every_plan_is_the_restated_one_and_fits_the_kernels():
    for hw in range(1, 40001):
        p = plan(hw)
        assert p == restated(hw), (hw, p)
        steps, qblocks, NC, spc, NCeff = p
        assert steps == qblocks == -(-hw // 64), (hw, p)
        assert 1 <= NCeff <= NC <= 16, (hw, p)
        assert NCeff * 16 <= 256, (hw, p)
        assert (NCeff - 1) * spc < steps <= NCeff * spc, (hw, p)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_shapes_of_the_gpu_test_are_in_the_regimes_they_were_chosen_for(shape):
    hw = shape[0] * shape[1]
    p = dict(zip(NAMES, plan(hw)))
    assert tuple(p.values()) == SHAPES[shape], (shape, p)
    last = p["steps"] - (p["NCeff"] - 1) * p["spc"]                  # steps of the last chunk
    if hw <= 64:
        assert p["steps"] == 1
    if shape in ((1, 1), (1, 3), (3, 5)):
        assert hw < 16 and (min(shape) == 1 or shape == (3, 5))         # the x16 upsample with a single source row or column
    if shape == (5, 7):
        assert hw // 16 == 2 and hw % 16 == 3 and hw <= 48
    if shape == (8, 8):
        assert hw == 64
    if shape == (5, 13):
        assert hw - 64 == 1 and p["steps"] == 2
    if shape == (32, 32):
        assert p["NC"] == p["NCeff"] == 16 and p["spc"] == 1 and hw % 64 == 0
    if shape == (23, 45):
        assert p["spc"] == 2 and p["NCeff"] == 9 and last == 1 and hw % 16 != 0
    if shape == (30, 54):
        assert p["NC"] == 16 and p["spc"] == 2 and p["NCeff"] == 13 < p["NC"] and last == p["spc"]
    if shape == (33, 63):
        assert hw > 2048 and p["qblocks"] == 33 and p["NC"] == -(-512 // 33) == 16 and p["spc"] == 3 and p["NCeff"] == 11
    if shape == (45, 80):
        assert p["NC"] == -(-512 // p["qblocks"]) == 9 < 16 and p["spc"] == 7 and last == 1
    if shape == (68, 120):
        assert p["NC"] == 4 and p["spc"] == 32 and p["NCeff"] == 4


def test_the_sweep_meets_every_branch_of_the_plan():
    """each of the three caps of NC (512 / qblocks, 16, steps) binds somewhere, and chunks are dropped (NCeff < NC) somewhere"""
    plans = {hw: dict(zip(NAMES, plan(hw))) for hw in range(1, 40001, 7)}
    assert any(p["NC"] == p["steps"] < 16 for p in plans.values())
    assert any(p["NC"] == 16 < p["steps"] and -(-512 // p["qblocks"]) > 16 for p in plans.values())
    assert any(p["NC"] == -(-512 // p["qblocks"]) < 16 for p in plans.values())
    assert any(p["NCeff"] < p["NC"] for p in plans.values())
    assert plan(40000)[2] == 1              # beyond 512 query blocks: one chunk walks the whole memory


def test_attention_plan_rejects_bad_arguments():
    from eva_vos_amd import _lib
    lib = _lib.lib()
    pl = (C.c_int32 * 5)()
    assert lib.stcn_attention_plan(0, pl) != 0 and lib.stcn_attention_plan(-5, pl) != 0 and lib.stcn_attention_plan(64, None) != 0


def test_attention_ex_checks_its_arguments_before_any_device_call():
    """on a machine without a GPU each of these fails with STCN_E_INVALID and a message, never with a HIP error"""
    from eva_vos_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(16)
    bad = [
        dict(mk=None), dict(qk=None), dict(attn=None), dict(kk=0), dict(kk=34), dict(nh=0), dict(nh=24), dict(nw=8), dict(nh=4096, nw=4112),
        dict(pos=None), dict(neg=None), dict(pooled_in=one), dict(pos=None, neg=None),
    ]
    for b in bad:
        a = dict(mk=one, qk=one, pos=one, neg=one, kk=2, nh=16, nw=32, msq=None, pooled_in=None, pooled_out=None, amap_out=None, attn=one)
        a.update(b)
        rc = lib.stcn_test_attention_ex(None, a["mk"], a["qk"], a["pos"], a["neg"], a["kk"], a["nh"], a["nw"], a["msq"], a["pooled_in"],
                                        a["pooled_out"], a["amap_out"], a["attn"])
        assert rc == -1 and b"stcn_test_attention_ex" in lib.stcn_last_error(), b
    assert lib.stcn_test_attention(None, one, one, None, one, 2, 16, 32, one) == -1
    assert lib.stcn_test_attention(None, one, one, one, one, 2, 16, 24, one) == -1
