"""The other arm of every documented launch switch, one process per arm.

The switches below ("Engine knobs") are read ONCE per process into function-local statics, so monkeypatch.setenv cannot reach
them: a test has to start a fresh process with the variable set.  This file is that process -

    python tests/switch_arm_cases.py <arm> <plan|gpu>

- and the table of arms (ARMS) that tests/test_switch_arms_plan.py (CPU) and tests/test_gpu_switch_arms.py (GPU) walk.  It is neither a test
module nor a conftest.  The parent sets the arm's variables in the child's environment only; the child refuses to run when its environment
does not carry exactly the arm's values (an arm that silently ran as the default would test nothing).

plan: one JSON line per case - stcn_test_conv_path / stcn_test_conv_plan of every conv case, stcn_memread_plan of every bank.  Needs no GPU.
gpu:  every conv case against F.conv2d in fp64 (the operands and the bound of test_gpu_kernels.test_conv_matches_fp64_reference, the output
      NaN before the call and finite after, the kernel family asserted), every bank at top_k 50 and 20 (the statements of
      test_gpu_topk.test_memory_read_k_matches_oracle, the rising-scores bank with its 5e-5), the engine on the goldens the arm names
      (test_oracle_golden.check_sequence_against_golden at the bounds of test_gpu_sequence.test_sequences_match_reference_goldens) with the
      conv trace of the first interact(), which the parent holds against the arm's statement (ARMS[arm]['trace']).  Plain asserts: the first failure ends the process, nothing else
      is launched after a HIP error.  One JSON line per case with its figures, one last line with the wall time.

Expected paths and plan numbers are what the planners give for 256 CUs (the MI355X; also what they assume without a device)."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SWITCHES = ("STCN_WINOGRAD", "STCN_WINO4", "STCN_WINO4_KEY", "STCN_WINO4_KEYPROJ", "STCN_WINO4_SMALL", "STCN_WINO4_TAIL", "STCN_WINO4_MB",
            "STCN_CONV_TAIL", "STCN_CONV_BIG", "STCN_MEMREAD_SAMPLE", "STCN_MEMREAD_RESCORE", "STCN_POOL_GB")
# per-workspace knobs the other GPU tests toggle: a child must not inherit one from the parent's environment
KNOBS = ("STCN_WINO_PPW", "STCN_WINO_MIN_CIN", "STCN_WINO4_CHUNK_MB", "STCN_PW_CHAIN", "STCN_FUSION_WINO", "STCN_FUSION_CONV12")


def conv(case, prefix, says_tail=None, **plan):
    """case (B,H,W,Cin,Cout,K,stride,flags) - flags as in test_gpu_kernels.CONVS: bit 0 ReLU in, bit 1 ReLU out, bit 2 F(4x4) layer; a case
    with B = 2 carries a residual.  prefix: what the path string starts with; says_tail: whether it says "+tail" (None: not stated); plan: numbers
    of stcn_test_conv_plan that must be exactly these."""
    return dict(case=tuple(case), prefix=prefix, says_tail=says_tail, plan=plan)


T23, TINY, C64, D16 = (2, 17, 23, 128, 128, 3, 1, 7), (1, 6, 5, 128, 32, 3, 1, 5), (1, 37, 51, 64, 96, 3, 1, 5), (1, 30, 54, 256, 512, 3, 1, 7)
RAG, QUARTER, TRUNK = (2, 52, 78, 256, 512, 3, 1, 7), (2, 120, 216, 128, 256, 3, 1, 7), (3, 61, 45, 64, 64, 3, 1, 6)
F2_A, F2_B, F2_C, FUSION = (2, 17, 23, 128, 128, 3, 1, 3), (2, 10, 12, 1024, 512, 3, 1, 3), (1, 30, 54, 256, 256, 3, 1, 2), (1, 21, 37, 32, 32, 3, 1, 2)
DT_A, DT_B, DT_C, DT_D = (2, 67, 65, 64, 256, 3, 1, 3), (1, 184, 192, 64, 32, 3, 1, 2), (4, 60, 108, 256, 256, 3, 2, 2), (3, 60, 108, 512, 512, 3, 2, 3)
BIG_A, BIG_B = (2, 39, 41, 256, 256, 3, 2, 3), (2, 30, 54, 512, 128, 3, 2, 2)
# the smallest of (B,60,108,512,512,3,2,.) and (B,60,108,256,512,3,2,.), B = 1..8, whose DEFAULT plan is direct_big: B = 6 either way; the
# 256-channel one has an fp64 reference of 23 GFLOP (the 512-channel one 46)
BIG_OFF = (6, 60, 108, 256, 512, 3, 2, 2)

RISING = "rising"                                 # the bank of test_gpu_topk.test_rising_scores_cut_full_lists_back_to_top_k (N = 4000, Q = 48)
BANKS = [(50, 16, 1), (1620, 333, 2), (6500, 97, 1), (32400, 97, 1), RISING]          # (N, Q, k)
BANK_NQ = {b: (4000, 48) if b == RISING else b[:2] for b in BANKS}
TOP_KS = (50, 20)


# ---------------------------------------------------------------------------------------------- statements about the conv trace
def _all_paths(paths):
    return [(n, q) for n, p in paths.items() for q in p]


def _none_starts(paths, prefix, names=lambda n: True):
    bad = [(n, q) for n, q in _all_paths(paths) if names(n) and q.startswith(prefix)]
    assert not bad, bad


def _all_start(paths, prefix, names):
    hit = [(n, q) for n, q in _all_paths(paths) if names(n)]
    assert hit, "no such layer in the trace"
    bad = [(n, q) for n, q in hit if not q.startswith(prefix)]
    assert not bad, bad


def _decoder_3x3(shapes):
    """names of the decoder's 3x3 layers but decoder.pred, and key_comp, as the trace spells them (the two halves of a conv over a channel
    concat are traced as <name>#a / <name>#b)"""
    def is_one(n):
        base = n.split("#")[0]
        return (base == "key_comp" or (base.startswith("decoder.") and base != "decoder.pred")) and tuple(shapes[base][2:]) == (3, 3)
    return is_one


def _key_conv2(n):
    return n.startswith("key_encoder.") and n.endswith(".conv2")


def wino4_flagged(name):
    """engine.cpp wino4_layer() under the default STCN_WINO4_KEY / STCN_WINO4_KEYPROJ, as INTEGRATION.md states it"""
    base = name.split("#")[0]
    if base in ("value_encoder.layer2.0.conv1", "value_encoder.layer3.0.conv1", "key_encoder.layer2.0.conv2", "key_encoder.layer3.0.conv2"):
        return False                              # the stride-2 3x3 convs of the two trunks
    return (_key_conv2(base) or base == "key_proj.key_proj" or base.startswith("decoder.") or base == "key_comp" or
            base.startswith("value_encoder.fuser.") or base.startswith("value_encoder.layer"))


def wino4_shape_ok(name, shapes):
    """what wino4_plan asks of a layer's weights [Cout, Cin, kh, kw] (a half of a split conv has fewer input channels, still a multiple of 32)"""
    cout, cin, kh, kw = shapes[name.split("#")[0]]
    return (kh, kw) == (3, 3) and cin % 32 == 0 and cin >= 64 and cout % 32 == 0


# A statement takes the arm's traces {tag: {layer: [path of every launch]}}, the weight shapes {layer: [Cout, Cin, kh, kw]} and the default
# arm's traces of the same goldens (the engine enqueues the same launches in the same order under every arm).
def trace_wino4_off(tr, shapes, dflt):
    for paths in tr.values():
        _none_starts(paths, "wino4")


def trace_winograd_off(tr, shapes, dflt):
    """STCN_WINOGRAD=0 switches F(2x2) only: no launch runs wino2, every launch the default arm runs as wino4 stays wino4 - among them every
    launch of a 3x3 layer of the decoder (decoder.pred apart) and of key_comp, except those the default arm ITSELF keeps off F(4x4) for too
    few workgroups (on seqA: one single-frame launch of decoder.up_16_8.out_conv.conv2), which now run the direct kernel."""
    for tag, paths in tr.items():
        _none_starts(paths, "wino2")
        assert set(paths) == set(dflt[tag]), sorted(set(paths) ^ set(dflt[tag]))
        dec, kept = _decoder_3x3(shapes), 0
        for n, p in paths.items():
            d = dflt[tag][n]
            assert len(p) == len(d), (n, p, d)
            for got, was in zip(p, d):
                if was.startswith("wino4"):
                    assert got.startswith("wino4"), (tag, n, got, was)
                    kept += dec(n)
                else:
                    assert not got.startswith("wino"), (tag, n, got, was)
            assert not dec(n) or any(q.startswith("wino4") for q in p), (tag, n, p)
        off = [(n, q) for n, q in _all_paths(dflt[tag]) if dec(n) and not q.startswith("wino4")]
        assert kept and len(off) <= 1, off                 # the default arm has (nearly) every such launch on F(4x4): the statement is not vacuous


def trace_both_off(tr, shapes, dflt):
    for paths in tr.values():
        _none_starts(paths, "wino")


def trace_wino4_always(tr, shapes, dflt):
    """on seqA's small frames every flagged layer whose shape F(4x4) takes runs it - and that is not what the default arm does"""
    want = lambda n: wino4_flagged(n) and wino4_shape_ok(n, shapes)             # noqa: E731
    _all_start(tr["seqA"], "wino4", want)
    moved = [n for n, p in dflt["seqA"].items() if want(n) and not all(q.startswith("wino4") for q in p)]
    assert moved, "the default arm already runs every such layer on F(4x4): STCN_WINO4=2 shows nothing on this golden"


def trace_key_off(tr, shapes, dflt):
    _none_starts(tr["seq480"], "wino4", _key_conv2)
    _all_start(tr["seq480"], "wino4", _decoder_3x3(shapes))
    _all_start(dflt["seq480"], "wino4", lambda n: _key_conv2(n) and wino4_flagged(n))


def trace_keyproj_off(tr, shapes, dflt):
    _all_start(tr["seq480"], "wino2", lambda n: n == "key_proj.key_proj")
    _all_start(tr["seq480"], "wino4", lambda n: _key_conv2(n) and wino4_flagged(n))
    assert any(q.startswith("wino4") for q in dflt["seq480"]["key_proj.key_proj"]), dflt["seq480"]["key_proj.key_proj"]


def trace_default(tr, shapes, dflt):
    """what the arms above are the other side of, at 480p: the key trunk and the decoder side on F(4x4), key_proj in its batched launches"""
    _all_start(tr["seq480"], "wino4", lambda n: _key_conv2(n) and wino4_flagged(n))
    _all_start(tr["seq480"], "wino4", _decoder_3x3(shapes))
    assert any(q.startswith("wino4") for q in tr["seq480"]["key_proj.key_proj"])
    assert any(q.startswith("wino2") for p in tr["seqA"].values() for q in p)


# ---------------------------------------------------------------------------------------------- the arms
# engine: goldens run through the engine, (tag, rounds) with rounds = None for the whole script.  seqA: 12 frames of 128x160, k = 1.
SEQA, SEQ480 = ("seqA", None), ("seq480", 1)
SAMPLE3 = {(6500, 97): [102, 3, 34, 7, 5, 26, 4]}
SAMPLE1000 = {BANK_NQ[b]: dict(ss=1000, ns=1, nc1=1, spc1=1) for b in BANKS}

ARMS = {
    # the yardstick: every conv case of every arm (plan mode) and a share of each kind of work (gpu mode) under no switch at all
    "default": dict(env={}, convs=[conv(T23, "wino4", True, grid=16, pieces=2), conv(TINY, "wino4", True, grid=4, pieces=2), conv(C64, "wino4", False, grid=18),
                                   conv(D16, "wino4", True, grid=256, pieces=4, per=8), conv(F2_A, "wino2 ppw=1 splitk=2"), conv(FUSION, "fusion_wino")],
                    banks=BANKS, engine=[SEQA, SEQ480], trace=trace_default),
    "wino4=0": dict(env={"STCN_WINO4": "0"},
                    convs=[conv(T23, "wino2 ppw=1 splitk=2"), conv(TINY, "direct_narrow splitk=9"), conv(C64, "direct splitk=4"), conv(D16, "wino2 ppw=1 splitk=4")],
                    engine=[SEQA], trace=trace_wino4_off),
    # the FusionNet shape: STCN_WINOGRAD=0 takes the in-workgroup Winograd kernel of the FusionNet layers off as well (wants_wino_fusion12 /
    # wants_wino): it runs the direct FusionNet kernel
    "winograd=0": dict(env={"STCN_WINOGRAD": "0"},
                       convs=[conv(F2_A, "direct splitk=9"), conv(F2_B, "direct splitk=16"), conv(F2_C, "direct splitk=4"),
                              conv(T23, "wino4", True, grid=16, pieces=2), conv(FUSION, "fusion_direct")],
                       engine=[SEQA], trace=trace_winograd_off),
    "wino4=0,winograd=0": dict(env={"STCN_WINO4": "0", "STCN_WINOGRAD": "0"},
                               convs=[conv(T23, "direct splitk=9"), conv(TINY, "direct_narrow splitk=9")], engine=[SEQA], trace=trace_both_off),
    # engine only: stcn_test_conv already plans with wino4_min_wg = 0.  plan_same: no plan export shows the switch
    "wino4=2": dict(env={"STCN_WINO4": "2"}, engine=[SEQA], trace=trace_wino4_always, plan_same="acts on Model::wino4_min_wg, which the conv hook sets to 0 itself"),
    "wino4_key=0": dict(env={"STCN_WINO4_KEY": "0"}, engine=[SEQA, SEQ480], trace=trace_key_off, plan_same="read at model creation: which layers get F(4x4) weights"),
    "wino4_keyproj=0": dict(env={"STCN_WINO4_KEYPROJ": "0"}, engine=[SEQA, SEQ480], trace=trace_keyproj_off, plan_same="read at model creation: which layers get F(4x4) weights"),
    "wino4_small=0": dict(env={"STCN_WINO4_SMALL": "0"},
                          convs=[conv(T23, "wino4", False, grid=8, pieces=1), conv(TINY, "wino4", False, grid=2, pieces=1), conv(D16, "wino4", False, grid=64, per=32, pieces=1)]),
    "wino4_tail=0": dict(env={"STCN_WINO4_TAIL": "0"},
                         convs=[conv(RAG, "wino4", False, mb=1, grid=288, full_wg=288, pieces=1), conv(T23, "wino4", False, pieces=1)]),
    "wino4_mb=1": dict(env={"STCN_WINO4_MB": "1"},
                       convs=[conv(QUARTER, "wino4", True, mb=1, tiles_m=102, grid=864, full_wg=768, pieces=2, per=8)]),
    "wino4_mb=2": dict(env={"STCN_WINO4_MB": "2"},
                       convs=[conv(TINY, "wino4", False, mb=2, grid=1, pieces=1), conv(T23, "wino4", False, mb=2, grid=4, pieces=1),
                              conv(TRUNK, "wino4", False, mb=2, grid=18, pieces=1), conv(D16, "wino4", False, mb=2, grid=32, pieces=1)]),
    "conv_tail=0": dict(env={"STCN_CONV_TAIL": "0"},
                        convs=[conv(DT_A, "direct splitk=1", False, tail=0), conv(DT_B, "direct_narrow splitk=1", False, tail=0),
                               conv(DT_C, "direct splitk=3", False, tail=0), conv(DT_D, "direct_big splitk=5", False, tile_big=1, tail=0)]),
    # BIG_A: M = 2 * 20 * 21 = 840, the last 128-row tile is ragged; BIG_B: one n-tile
    "conv_big=2": dict(env={"STCN_CONV_BIG": "2"},
                       convs=[conv(BIG_A, "direct_big splitk=18", False, tile_big=1), conv(BIG_B, "direct_big splitk=29", False, tile_big=1),
                              conv(DT_C, "direct_big splitk=5", False, tile_big=1)]),
    "conv_big=0": dict(env={"STCN_CONV_BIG": "0"}, convs=[conv(BIG_OFF, "direct splitk=1", False, tile_big=0)]),
    "memread_sample=3": dict(env={"STCN_MEMREAD_SAMPLE": "3"}, banks=BANKS, memplan=SAMPLE3),
    "memread_sample=1000": dict(env={"STCN_MEMREAD_SAMPLE": "1000"}, banks=BANKS, memplan=SAMPLE1000),
    "memread_rescore=0": dict(env={"STCN_MEMREAD_RESCORE": "0"}, banks=BANKS, plan_same="acts in the launch sequence of the read, not in its plan"),
    "pool_gb=0": dict(env={"STCN_POOL_GB": "0"}, engine=[SEQA], second_core=True, plan_same="acts on the engine's allocator"),
}
# plan mode of the default arm: every conv case and bank of every arm
DEFAULT_PLAN_CONVS = sorted({c["case"] for a in ARMS.values() for c in a.get("convs", ())})


def child_env(arm):
    """the environment of the arm's child: the parent's without any switch or knob, plus the arm's own values"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES + KNOBS}
    env.update(ARMS[arm]["env"])
    return env


def child_argv(arm, mode):
    return [sys.executable, os.path.join(HERE, "switch_arm_cases.py"), arm, mode]


# ---------------------------------------------------------------------------------------------- the child
def emit(arm, **kv):
    print(json.dumps(dict(arm=arm, **kv)), flush=True)


def run_plan(arm):
    from test_conv_plan import conv_path, conv_plan
    from test_memread_plan import plan as memread_plan
    cases = DEFAULT_PLAN_CONVS if arm == "default" else [c["case"] for c in ARMS[arm].get("convs", ())]
    for case in cases:
        emit(arm, kind="conv", case=case, path=conv_path(*case, 0), plan=conv_plan(*case, 0))
    for b in ARMS[arm].get("banks", ()):
        N, Q = BANK_NQ[b]
        emit(arm, kind="memread", bank=[N, Q], plan=memread_plan(N, Q))


def run_conv_case(arm, c):
    import torch
    from gpu_util import call, dev, nhwc, stream
    from test_gpu_kernels import conv_fp64_case, last_path
    B, H, W, Cin, Cout, K, s, flags = c["case"]
    x, w, b, res, ref, OH, OW = conv_fp64_case(B, H, W, Cin, Cout, K, s, flags)
    assert (res is not None) == (B == 2 or (Cin, Cout) == (32, 32))
    y = torch.full((B, OH, OW, Cout), float("nan"), device="cuda")
    call("stcn_test_conv", stream(), nhwc(x), dev(w.permute(0, 2, 3, 1)), dev(b), None if res is None else nhwc(res), y,
         B, H, W, Cin, Cout, K, K, s, K // 2, flags, 0)
    got = y.permute(0, 3, 1, 2).cpu().double()
    ran = last_path()
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    emit(arm, kind="conv", case=c["case"], path=ran, err=err, finite=finite)
    assert finite, "the kernel left part of the output unwritten (NaN before the call)"
    assert err < 2e-5, err                    # fp32 accumulation vs fp64
    assert ran.startswith(c["prefix"]), (ran, c["prefix"])
    assert c["says_tail"] is None or ("+tail" in ran) == c["says_tail"], ran


def run_bank(arm, bank, top_k):
    from oracle import stcn_oracle as O
    from test_gpu_topk import check_read_k_against_oracle, check_rising_scores_read, random_bank
    O.TOP_K = top_k
    if bank == RISING:
        dw, err = check_rising_scores_read(top_k)
        emit(arm, kind="memread", bank=RISING, top_k=top_k, dweight=dw, err=err)
    else:
        near, differ = check_read_k_against_oracle(*random_bank(*bank), top_k)
        emit(arm, kind="memread", bank=list(bank), top_k=top_k, near=near, differ=differ)


class FirstInteractTraced:
    """a core whose first interact() runs under the conv trace"""

    def __init__(self, core):
        self.core, self.paths = core, None

    @property
    def prob(self):
        return self.core.prob

    def interact(self, *a, **kw):
        from test_gpu_sequence import _conv_trace
        if self.paths is not None:
            return self.core.interact(*a, **kw)
        out, self.paths = _conv_trace(lambda: self.core.interact(*a, **kw))
        return out


def make_nets():
    """conftest's `weights` / `nets` fixtures"""
    from eva_vos_amd import synth
    from eva_vos_amd.params import FusionNet, PropagationNetwork
    p, f = PropagationNetwork(), FusionNet()
    weights = synth.recipe_state_dict(p), synth.recipe_state_dict(f)
    p.load_state_dict(weights[0], strict=True)
    f.load_state_dict(weights[1], strict=True)
    return (p.eval(), f.eval()), weights


def run_engine(arm, nets, weights, tag, rounds):
    from conftest import load_golden
    from test_gpu_sequence import make_core, nets_of
    from test_oracle_golden import check_sequence_against_golden, run_sequence
    g = load_golden(tag)
    if rounds is not None:
        g[f"{tag}.script"] = g[f"{tag}.script"][:rounds]
    nets, _ = nets_of(g, tag, nets, weights)
    cores = []

    def factory(img, k, mf):
        cores.append(FirstInteractTraced(make_core(nets)(img, k, mf)))
        return cores[0]

    outs = run_sequence(factory, tag, g)
    emit(arm, kind="engine", tag=tag, rounds=len(outs), trace=cores[0].paths)
    check_sequence_against_golden(outs, tag, g, prob_atol=3e-3, who=arm)
    return cores[0].paths


def run_gpu(arm):
    import gc
    import torch
    spec = ARMS[arm]
    assert torch.cuda.is_available(), "gpu mode needs the GPU"
    for c in spec.get("convs", ()):
        run_conv_case(arm, c)
    for bank in spec.get("banks", ()):
        for top_k in TOP_KS:
            run_bank(arm, bank, top_k)
    if spec.get("engine"):
        nets, weights = make_nets()
        shapes = {n[:-len(".weight")]: tuple(v.shape) for n, v in weights[0].items() if n.endswith(".weight") and v.dim() == 4}
        for tag, rounds in spec["engine"]:
            run_engine(arm, nets, weights, tag, rounds)
        if spec.get("second_core"):              # a second engine built on, and returned to, the plain allocator
            from eva_vos_amd import synth
            from test_gpu_sequence import make_core
            core = make_core(nets)(synth.synthetic_clip(3, 128, 160), 1, 5)
            assert core.interact(synth.synthetic_mask(3, 128, 160, 1)[:, 0], 0).shape == (3, 128, 160)
            del core
            gc.collect()
            torch.cuda.synchronize()
        emit(arm, kind="shapes", shapes=shapes)


def main(argv):
    arm, mode = argv[1], argv[2]
    assert arm in ARMS and mode in ("plan", "gpu"), argv
    seen = {k: os.environ[k] for k in SWITCHES + KNOBS if k in os.environ}
    assert seen == ARMS[arm]["env"], (seen, ARMS[arm]["env"])
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import conftest  # noqa: F401  (no gradients, the host's thread count: what the suite's own references run under)
    t0 = time.time()
    emit(arm, kind="start", mode=mode, env=seen)
    (run_plan if mode == "plan" else run_gpu)(arm)
    emit(arm, kind="done", seconds=round(time.time() - t0, 2))


if __name__ == "__main__":
    main(sys.argv)
