"""GPU: the other arm of every documented process-level switch runs, and computes what the default computes - one fresh child process per arm
(tests/switch_arm_cases.py in `gpu` mode; the switches are read once per process).  The child checks its conv cases against fp64, its banks
against the CPU oracle, its engine runs against the reference's goldens and the conv trace of the first interact() against the arm's
statement; this module starts the children, one at a time, and compares what needs two arms.

A child that ends by a signal, runs into its time limit or reports an illegal memory access has faulted the device: the first such child is
latched, and every later arm fails at once without starting anything (no skip - a skip would hide the fault; no retry).

CHILD_TIMEOUT: the default-arm child (6 conv cases, 5 banks at two cuts, seqA and the first round of seq480) measured 6.3 s of wall
time on an MI355X (MEASURED_DEFAULT_S; the other children 2.3 to 5.9 s); the limit of every child is ten times that, and at least 120 s."""
import json
import subprocess
import time

import pytest

import switch_arm_cases as S

pytestmark = pytest.mark.gpu

MEASURED_DEFAULT_S = 6.3
CHILD_TIMEOUT = max(120.0, 10 * MEASURED_DEFAULT_S)
FAULT_CODES = (134, 139, 124, 137)

_FAULTED = []          # the first arm whose child faulted
_CHILD = {}


def gpu_child(arm):
    """the JSON lines of the arm's child; started at most once, and never after another child has faulted"""
    if arm in _CHILD:
        return _CHILD[arm]
    assert not _FAULTED, f"not started: {_FAULTED[0]} faulted"
    t0 = time.time()
    try:
        p = subprocess.run(S.child_argv(arm, "gpu"), env=S.child_env(arm), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        rc, out, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as ex:
        text = lambda b: b if isinstance(b, str) else (b or b"").decode(errors="replace")        # noqa: E731
        rc, out, err = "timeout", text(ex.stdout), text(ex.stderr)
    wall = time.time() - t0
    print(out[-6000:])
    if rc == "timeout" or rc < 0 or rc in FAULT_CODES or "illegal memory access" in out + err:
        _FAULTED.append(arm)
        raise AssertionError(f"{arm}: the child faulted (return code {rc})\n{err[-3000:]}")
    assert rc == 0, (arm, rc, err[-3000:])
    lines = [json.loads(l) for l in out.splitlines() if l.startswith('{"arm"')]
    assert lines[0]["kind"] == "start" and lines[0]["env"] == S.ARMS[arm]["env"] and lines[-1]["kind"] == "done", lines[:1]
    lines[-1]["wall_s"] = wall
    _CHILD[arm] = lines
    return lines


def traces_of(lines):
    return {l["tag"]: l["trace"] for l in lines if l["kind"] == "engine"}


@pytest.mark.parametrize("arm", list(S.ARMS))
def test_arm_runs_and_computes_what_the_default_computes(arm):
    spec = S.ARMS[arm]
    lines = gpu_child(arm)
    convs = [l for l in lines if l["kind"] == "conv"]
    reads = [l for l in lines if l["kind"] == "memread"]
    assert [tuple(l["case"]) for l in convs] == [c["case"] for c in spec.get("convs", ())]
    assert len(reads) == len(spec.get("banks", ())) * len(S.TOP_KS)
    traces = traces_of(lines)
    assert sorted(traces) == sorted(t for t, _ in spec.get("engine", ()))
    print(f"{arm}: child {lines[-1]['wall_s']:.1f} s of wall time ({lines[-1]['seconds']} s after its imports); worst conv error "
          f"{max([l['err'] for l in convs], default=None)}; near-tie queries {sum(l.get('near', 0) for l in reads)}, "
          f"selected differently {sum(l.get('differ', 0) for l in reads)}")
    if spec.get("trace"):
        shapes = next(l["shapes"] for l in lines if l["kind"] == "shapes")
        spec["trace"](traces, shapes, traces_of(gpu_child("default")))
