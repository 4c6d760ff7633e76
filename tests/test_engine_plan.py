"""CPU: the configuration of an engine is pure host code (plan_engine, through stcn_test_engine_plan): which option, environment variable
or default decides each tunable, every clamp, the dual sweep's conditions, what the bank is sized for and what the three workspaces are
built with - against values worked out by hand from the rules include/stcn_hip.h states, on a machine without a GPU."""
import ctypes as C

import pytest

ENV = ("STCN_LOOKAHEAD", "STCN_DECODE_BATCH", "STCN_KEY_BATCH", "STCN_FUSE_SIDE", "STCN_DUAL_SWEEP")
STCN_E_INVALID = -1


def engine_plan(monkeypatch, T, k, mem_freq, has_fuse, opts=None, env=None):
    """the plan as a dict, under exactly the variables of `env` (the other engine variables are cleared)"""
    from eva_vos_amd import _lib
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        assert "STCN_" + name in ENV
        monkeypatch.setenv("STCN_" + name, str(value))
    o = _lib.EngineOpts(-1, -1, -1, -1)
    for name, value in (opts or {}).items():
        setattr(o, name, value)
    n = len(_lib.ENGINE_PLAN_FIELDS)
    out = (C.c_int32 * n)()
    _lib.check(_lib.lib().stcn_test_engine_plan(T, k, mem_freq, int(has_fuse), C.byref(o) if opts is not None else None, out, n), "stcn_test_engine_plan")
    return dict(zip(_lib.ENGINE_PLAN_FIELDS, out))


def check_workspaces(p):
    la = p["lookahead"] > 0
    assert (p["main_key_batch"], p["main_group"]) == (1 if la else p["key_batch"], p["group"])
    assert p["has_side"] == int(la or p["fuse_side"] == 1)
    assert (p["side_key_batch"], p["side_group"]) == (p["key_batch"] if la else 1, 1)
    assert (p["second_key_batch"], p["second_group"]) == (p["main_key_batch"], p["main_group"])      # it exists iff dual_sweep


# (T, k, mem_freq, has_fuse), opts, env -> lookahead, group, key_batch, fuse_side, dual_sweep, bank_lo, bank_initial
CASES = [
    ((9, 1, 3, True), None, None, (2, 3, 4, 1, 1, 4, 15)),
    ((9, 1, 3, True), None, {"DECODE_BATCH": 2}, (2, 2, 4, 1, 1, 4, 15)),
    ((9, 1, 3, True), {"lookahead": 0, "decode_batch": 3, "key_batch": 2}, None, (0, 3, 2, 0, 0, 0, 11)),
    ((104, 5, 1, True), None, None, (2, 1, 4, 1, 1, 105, 217)),
    ((120, 1, 5, True), None, None, (0, 5, 5, 1, 0, 0, 32)),
    ((30, 5, 5, True), None, None, (2, 3, 4, 1, 1, 7, 21)),
    ((30, 3, 8, True), None, None, (2, 5, 5, 1, 1, 5, 17)),
    ((2, 1, 5, True), None, None, (2, 5, 5, 1, 0, 0, 9)),
    ((9, 1, 5, False), None, None, (2, 5, 5, 0, 1, 3, 13)),
    ((9, 1, 5, True), None, {"DUAL_SWEEP": 0}, (2, 5, 5, 1, 0, 0, 10)),
    ((9, 1, 5, True), {"key_batch": 12, "decode_batch": 0}, None, (2, 1, 8, 1, 1, 3, 13)),
]


@pytest.mark.parametrize("shape,opts,env,want", CASES, ids=[f"T{s[0]}k{s[1]}m{s[2]}{'' if s[3] else 'nofuse'}-{i}" for i, (s, *_) in enumerate(CASES)])
def test_engine_plan_resolves_and_clamps(monkeypatch, shape, opts, env, want):
    p = engine_plan(monkeypatch, *shape, opts=opts, env=env)
    got = tuple(p[n] for n in ("lookahead", "group", "key_batch", "fuse_side", "dual_sweep", "bank_lo", "bank_initial"))
    assert got == want, p
    T = shape[0]
    assert p["n_slots"] == min(T, 106)
    assert p["lookahead_req"] == (opts or {}).get("lookahead", 2), "what was asked for, before the long-clip rule"
    check_workspaces(p)


@pytest.mark.parametrize("field,var,plan_name,env_value,opt_value", [
    ("lookahead", "LOOKAHEAD", "lookahead", 0, 3),
    ("decode_batch", "DECODE_BATCH", "group", 2, 4),
    ("key_batch", "KEY_BATCH", "key_batch", 2, 7),
    ("fuse_side", "FUSE_SIDE", "fuse_side", 0, 1),
])
def test_an_explicit_option_beats_the_environment(monkeypatch, field, var, plan_name, env_value, opt_value):
    shape = (9, 1, 5, True)
    from_env = engine_plan(monkeypatch, *shape, env={var: env_value})
    assert from_env[plan_name] == env_value, "the environment decides where no option is given"
    both = engine_plan(monkeypatch, *shape, opts={field: opt_value}, env={var: env_value})
    assert both[plan_name] == opt_value
    assert both == engine_plan(monkeypatch, *shape, env={var: opt_value}), "an option and a variable of the same value make the same plan"
    check_workspaces(from_env)
    check_workspaces(both)


def test_engine_plan_rejects_bad_arguments():
    from eva_vos_amd import _lib
    lib = _lib.lib()
    n = len(_lib.ENGINE_PLAN_FIELDS)
    out = (C.c_int32 * n)()
    assert lib.stcn_test_engine_plan(9, 1, 5, 1, None, None, n) == STCN_E_INVALID
    assert lib.stcn_test_engine_plan(9, 1, 5, 1, None, out, n - 1) == STCN_E_INVALID
    assert lib.stcn_test_engine_plan(9, 1, 5, 1, None, out, 0) == STCN_E_INVALID
    assert lib.stcn_test_engine_plan(0, 1, 5, 1, None, out, n) == STCN_E_INVALID
    assert lib.stcn_test_engine_plan(9, 0, 5, 1, None, out, n) == STCN_E_INVALID
    assert lib.stcn_test_engine_plan(9, 1, 0, 1, None, out, n) == STCN_E_INVALID
    assert lib.stcn_engine_get_plan(None, out, n) == STCN_E_INVALID
    assert lib.stcn_test_engine_plan(9, 1, 5, 1, None, out, n) == 0
