"""CPU: what every documented process-level switch does to the launch plans, one child process per arm (tests/switch_arm_cases.py in `plan`
mode: the switches are read once per process, so each arm needs a process of its own).  Every conv case must plan to the path and the numbers
the arm table states, every Winograd plan must be consistent (test_conv_plan.check_winograd_plan), every memory-read plan must cover its
steps - and every arm that a plan can show must plan at least one of its own cases differently from the default arm: an arm that plans like
the default tests nothing."""
import json
import subprocess

import pytest

import switch_arm_cases as S
from test_conv_plan import WINO2, WINO4, check_winograd_plan

_CHILD = {}


def plan_child(arm):
    """the JSON lines of the arm's child, run once"""
    if arm not in _CHILD:
        p = subprocess.run(S.child_argv(arm, "plan"), env=S.child_env(arm), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (arm, p.stdout[-2000:], p.stderr[-3000:])
        _CHILD[arm] = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{"arm"')]
    return _CHILD[arm]


def convs_of(lines):
    return {tuple(l["case"]): l for l in lines if l["kind"] == "conv"}


def banks_of(lines):
    return {tuple(l["bank"]): l["plan"] for l in lines if l["kind"] == "memread"}


def check_memread_plan(p, N):
    assert p["steps"] == -(-N // 64) and p["ss"] >= 1
    assert p["ns"] == -(-p["steps"] // p["ss"])
    assert (p["nc1"] - 1) * p["spc1"] < p["ns"] <= p["nc1"] * p["spc1"]
    assert (p["nc2"] - 1) * p["spc2"] < p["steps"] <= p["nc2"] * p["spc2"]
    assert 1 <= p["nc1"] <= 8 and 1 <= p["nc2"] <= 32                   # what the kernels hold (test_memread_plan.py)


def test_the_table_names_every_documented_switch():
    """each of the twelve switches has an arm, and each arm sets nothing else"""
    used = {k for a in S.ARMS.values() for k in a["env"]}
    assert used == set(S.SWITCHES)
    assert "default" in S.ARMS and S.ARMS["default"]["env"] == {}


@pytest.mark.parametrize("arm", list(S.ARMS))
def test_arm_plans_what_the_table_states(arm):
    spec = S.ARMS[arm]
    lines = plan_child(arm)
    assert lines[0]["kind"] == "start" and lines[0]["env"] == spec["env"] and lines[-1]["kind"] == "done", lines[:1]
    got, default = convs_of(lines), convs_of(plan_child("default"))
    assert arm == "default" or len(got) == len(spec.get("convs", ()))
    differs = []
    for c in spec.get("convs", ()):
        case, line = c["case"], got[c["case"]]
        path, pl = line["path"], line["plan"]
        print(arm, case, path, {k: pl[k] for k in ("splitk", "mb", "tiles_m", "grid", "full_wg", "pieces", "per", "tile_big", "tail")})
        assert path.startswith(c["prefix"]), (case, path, c["prefix"])
        assert c["says_tail"] is None or ("+tail" in path) == c["says_tail"], (case, path)
        assert {k: pl[k] for k in c["plan"]} == c["plan"], (case, pl, c["plan"])
        if pl["family"] in (WINO4, WINO2):
            check_winograd_plan(case + (0,), pl)
        d = default[case]
        differs.append(path != d["path"] or pl != d["plan"])
    banks = banks_of(lines)
    for b in spec.get("banks", ()):
        N, Q = S.BANK_NQ[b]
        p = banks[(N, Q)]
        print(arm, "memread", N, Q, p)
        check_memread_plan(p, N)
        want = spec.get("memplan", {}).get((N, Q))
        if isinstance(want, list):
            assert [p[k] for k in ("steps", "ss", "ns", "nc1", "spc1", "nc2", "spc2")] == want, (N, Q, p)
        elif want:
            assert {k: p[k] for k in want} == want, (N, Q, p)
        differs.append(p != banks_of(plan_child("default"))[(N, Q)])
    if arm == "default":
        assert set(got) == set(S.DEFAULT_PLAN_CONVS)
    elif "plan_same" in spec:
        assert not any(differs), (arm, "the table says no plan shows this switch:", spec["plan_same"])
    else:
        assert any(differs), f"{arm} plans every one of its cases as the default arm does"


def test_conv_big_0_takes_the_large_extent_case_off_the_big_tile():
    """the stride-2 case of the multi-GiB tests that runs direct_big by default"""
    from large_extents import LARGE_CONVS
    name, case, _, path, _ = next(c for c in LARGE_CONVS if c[0] == "big-s2-x1.98G")
    assert path.startswith("direct_big")
    code = ("import sys; sys.path[:0] = %r; from test_conv_plan import conv_path; print('PATH=' + conv_path(*%r))" % ([S.ROOT, S.HERE], tuple(case)))
    p = subprocess.run([S.sys.executable, "-c", code], env=S.child_env("conv_big=0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    ran = [l for l in p.stdout.splitlines() if l.startswith("PATH=")][0][5:]
    assert ran.startswith("direct") and not ran.startswith("direct_big"), ran
