"""CPU: sessions suspended between their rounds (sessions.annotation_rounds, the ``steps=True`` of the ``run_*``) and the live ranking over
them (budget.run_ranked) on the fakes of session_fakes.py.  The ranked runs replay the sessions of tests/golden/ranking.npz through scripted
sessions: what is checked is the loop - its commit order and curve against ``ranking.rank_curve``, where it stops, how many rounds it ran."""
import random

import numpy as np
import pytest
import torch

from eva_vos_amd import budget, eval_driver, fq_driver, metrics, ranking, sessions
from session_fakes import Annotator, DriverScorer, Proc, Scorer, clip, fake_core_class
from ranking_cases import golden_sessions


# ------------------------------------------------------------------------------------------------ steppable sessions
class MaskScorer(Scorer):
    """``RoundScorer``'s ``score`` (no ``types``: every annotation is a mask) over the typed fake."""

    def score(self, processor, annotated_frames, keep_gen=True, incremental=True):
        return super().score(processor, annotated_frames, keep_gen, incremental, types=[1] * len(annotated_frames))


def _mask_policy(gt, log):
    return sessions.SessionPolicy(lambda f: gt[f][None], lambda worst, types, gen, frames: worst)


def _typed_policy(gt, log):
    """Clicks on odd frames, masks on even ones; the next frame is the first that has no mask yet, so clicked frames repeat."""
    annotator = Annotator(log)

    def action(frame, gen, frame_annots):
        kind = "click" if frame % 2 and "click" not in frame_annots["annotations"] else "mask"
        mask, cost, _, logits, clicks, labels, bbox = annotator.annotate(kind, gt[frame, 0], None, gen[frame][None].to(torch.bool), frame_annots)
        return mask, cost, kind, logits, clicks, labels, bbox

    def choose(worst, types, gen, frames):
        left = np.where(types != 1)[0]
        return int(left[0]) if len(left) else None
    return sessions.SessionPolicy(lambda f: gt[f][None], choose, action=action, stop_at_T=False)


def _plain(ses):
    return {k: ([g.tolist() for g in v] if k == "gens" else v) for k, v in ses.items()}


@pytest.mark.parametrize("make,T,rounds,empty", [(_mask_policy, 5, 7, [3]), (_mask_policy, 4, 3, []), (_typed_policy, 4, 9, [2]), (_typed_policy, 5, 4, [])])
def test_rounds_stepped_to_the_end_are_the_session_call_for_call(make, T, rounds, empty):
    gt, _ = clip(T, empty)
    logs, results, stats = [[], []], [], [{}, {"propagated_frames": 5}]
    scorer = MaskScorer if make is _mask_policy else Scorer
    results.append(sessions.annotation_session(Proc(logs[0]), scorer(gt[:, 0], logs[0], trace=True), T, rounds, make(gt, logs[0]), stats[0]))
    stepped = sessions.annotation_rounds(Proc(logs[1]), scorer(gt[:, 0], logs[1], trace=True), T, rounds, make(gt, logs[1]), stats[1])
    steps = 0
    while stepped.step():
        steps += 1
        assert len(stepped.ses["costs"]) == steps and stepped.ses["costs"][-1] == stepped.costs[-1]
    assert not stepped.step() and not stepped.more()                                 # the end stays the end
    results.append(stepped.ses)
    print(logs[0], results[0]["frames"], results[0]["costs"])
    assert logs[0] == logs[1] and _plain(results[0]) == _plain(results[1]) and steps == len(results[0]["costs"]) > 1
    assert stats[1]["interactions"] == stats[0]["interactions"] == steps and stats[1]["propagated_frames"] == stats[0]["propagated_frames"] + 5


def test_more_says_whether_a_step_would_run_without_running_it():
    for make, T, rounds, empty in ((_mask_policy, 5, 7, [3]), (_mask_policy, 4, 3, []), (_typed_policy, 4, 9, [2])):
        gt, _ = clip(T, empty)
        log = []
        stepped = sessions.annotation_rounds(Proc(log), (MaskScorer if make is _mask_policy else Scorer)(gt[:, 0], log), T, rounds, make(gt, log))
        assert stepped.more()
        while True:
            before, expect = list(log), stepped.more()
            assert log == before                                                    # asking runs nothing
            assert stepped.step() == expect
            if not expect:
                break


def _typed_run(policy, seed, log, steps):
    gt, rgb = clip(5, [2])
    return eval_driver.run_typed_policy(policy, Proc(log), {"num_frames": 5, "gt": gt[None], "rgb": rgb}, 7, Annotator(log), ["click", "mask"], "j_and_f",
                                        rng=random.Random(seed), stats={}, scorer=Scorer(gt[:, 0], log, trace=True), steps=steps)


def test_sessions_stepped_in_turn_give_what_each_gives_straight_through():
    straight = []
    for seed in (2, 3):
        log = []
        straight.append((_typed_run("rand_rand", seed, log, False), log))
    logs = [[], []]
    stepped = [_typed_run("rand_rand", seed, logs[j], True) for j, seed in enumerate((2, 3))]
    assert logs == [[], []]                                                          # steps=True runs nothing
    live = [True, True]
    while any(live):
        for j, s in enumerate(stepped):
            live[j] = live[j] and s.step()
    for j, s in enumerate(stepped):
        s.close()
        res, want = s.result(), straight[j][0]
        assert logs[j] == straight[j][1]
        assert res.keys() == want.keys() and all(np.array_equal(np.asarray(res[k], dtype=object), np.asarray(want[k], dtype=object)) for k in res if k != "round_metrics")
        assert np.array_equal(np.stack(res["round_metrics"]), np.stack(want["round_metrics"]))


def test_the_mask_policies_and_eva_vos_hand_back_suspended_sessions_too(monkeypatch):
    from session_fakes import Agent, Selector
    monkeypatch.setattr(metrics, "RoundScorer", DriverScorer)
    gt, rgb = clip(4, [])
    sample = {"num_frames": 4, "gt": gt[None], "rgb": rgb}
    want = eval_driver.run_policy("oracle_mask", Proc([]), sample, 6, "j")
    s = eval_driver.run_policy("oracle_mask", Proc([]), sample, 6, "j", steps=True)
    assert s.step() and s.result()["annotation_times"] == [80] and s.result()["frames"] == want["frames"][:2]
    assert s.run()["frames"] == want["frames"] and s.result()["mu_metrics"] == want["mu_metrics"]
    runs = []
    for steps in (False, True):
        log = []
        r = eval_driver.run_eva_vos(Proc(log), sample, 5, Annotator(log), "qnet", Agent([(1, 0.75), (0, 0.5)], log), "j_and_f", stats={},
                                    scorer=Scorer(gt[:, 0], log), selector=Selector([1, 2, 3], log), steps=steps)
        runs.append((r.run() if steps else r, [e[:3] for e in log]))
    assert runs[0][1] == runs[1][1] and runs[0][0]["rl_values"] == runs[1][0]["rl_values"] == [-2, 0.75, 0.5]
    assert runs[0][0]["annotated_frames"] == runs[1][0]["annotated_frames"]


# ------------------------------------------------------------------------------------------------ the ranked run on scripted sessions
class Replay:
    """A suspended session that replays one recorded session: ``step`` reveals its next round."""

    def __init__(self, rec):
        self.rec, self.n, self.step_calls, self.closed = rec, 0, 0, False

    def step(self):
        self.step_calls += 1
        ran = self.n < len(self.rec["mu_metrics"])
        self.n += ran
        return ran

    def more(self):
        return self.n < len(self.rec["mu_metrics"])

    def close(self):
        self.closed = True

    def result(self):
        r, n = self.rec, self.n
        names = ["3clicks", "mask", "no_object"]
        return dict(mu_metrics=r["mu_metrics"][:n], annotation_times=r["annotation_times"][:n], round_metrics=[np.array(q) for q in r["round_metrics"][:n]],
                    frames=r["annotated_frames"][:n], rl_values=r["rl_values"][:n], annotations_actions=[names[a] for a in r["annotation_actions"][:n]],
                    propagated_frames=0)


@pytest.fixture(scope="module")
def replay_tree(tmp_path_factory):
    """A dataset tree with the fixture's videos as one-object clips of the fixture's lengths: sample i is fixture video i, named ``<name>__1``."""
    _, recs = golden_sessions()
    root = str(tmp_path_factory.mktemp("replay"))
    imset = fq_driver.make_synthetic_tree(root, {rec["video"]: (len(rec["round_metrics"][0]), 16, 16, 1) for rec in recs})
    return root, imset, recs


def _ranked(monkeypatch, replay_tree, policy, **kw):
    """run_ranked over the replayed fixture under ``policy``'s rule: (what it returned, the replays, its stats)."""
    import mivos.inference_core
    root, imset, recs = replay_tree
    replays = {}

    def runner(job, proc, sample, i, session):
        assert job.steps
        replays[i] = Replay(recs[i])
        return replays[i]
    spec = eval_driver.PolicySpec(runner, tail=(eval_driver.VALUES, eval_driver.ACTIONS), seconds=float,
                                  action_names=lambda annotation_types: ["3clicks", "mask", "no_object"])
    monkeypatch.setitem(budget.POLICY_TABLE, policy, spec)
    monkeypatch.setattr(mivos.inference_core, "InferenceCore", fake_core_class([]))
    stats = {}
    out = budget.run_ranked(root, imset, kw.pop("out_csv", ""), None, None, policy, device="cpu", lanes=2, stats=stats, **kw)
    return out, [replays[i] for i in range(len(recs))], stats


def _full_curve(recs, policy):
    """rank_curve on the fixture as a run's float32 rows hold it."""
    spec = eval_driver.PolicySpec(None, tail=(eval_driver.VALUES, eval_driver.ACTIONS))
    rows = []
    for i, rec in enumerate(recs):
        res = Replay(rec)
        res.n = len(rec["mu_metrics"])
        rows += eval_driver.result_rows(res.result(), i, None, False, spec, ["3clicks", "mask", "no_object"], 6 + 10 + 2)
    return ranking.rank_curve(ranking.read_rows(np.stack(rows), spec), use_values=budget.uses_values(policy)), np.stack(rows)


@pytest.mark.parametrize("policy", ["oracle_oracle", "eva_vos"])
def test_the_live_ranking_commits_what_rank_curve_commits(monkeypatch, replay_tree, tmp_path, policy):
    g, recs = golden_sessions()
    (hours, points, order), full_rows = _full_curve(recs, policy)
    (rows, h, p, o), replays, stats = _ranked(monkeypatch, replay_tree, policy, ranking_csv=str(tmp_path / "ranking.csv"),
                                              reference_csv=str(tmp_path / "ref.csv"), out_csv=str(tmp_path / "rows.csv"))
    assert o == order and np.array_equal(h, hours) and np.array_equal(p, points)
    if policy == "oracle_oracle":                                                    # the gain rule reads nothing float32 rounds: the reference's own curve
        assert np.array_equal(h, g["gain.hours"]) and np.array_equal(p, g["gain.points"])
    # every video ran all its rounds once (its last as a look-ahead that is never committed), and the rows are the committed rounds' rows
    assert [r.step_calls for r in replays] == [len(rec["mu_metrics"]) for rec in recs] and all(r.closed for r in replays)
    keep = np.concatenate([np.arange(len(rec["mu_metrics"]) - 1) + sum(len(x["mu_metrics"]) for x in recs[:i]) for i, rec in enumerate(recs)])
    assert np.array_equal(rows, full_rows[keep], equal_nan=True)
    assert stats["committed_rounds"] == len(rows) and stats["lookahead_rounds"] == len(recs)
    rh, rp, ro = ranking.read_ranking_csv(str(tmp_path / "ranking.csv"))
    assert np.array_equal(rh, h) and np.array_equal(rp, p) and ro == [(recs[i]["video"] + "__1", r) for i, r in o]
    assert ranking.read_rows(rows, budget.POLICY_TABLE[policy], [r["video"] + "__1" for r in recs]) == ranking.read_reference_csv(str(tmp_path / "ref.csv"), ["3clicks", "mask", "no_object"])
    assert len(open(str(tmp_path / "rows.csv")).readlines()) == 1 + len(rows)


@pytest.mark.parametrize("policy", ["oracle_oracle", "eva_vos"])
def test_a_budget_stops_before_the_first_commit_beyond_it(monkeypatch, replay_tree, policy):
    _, recs = golden_sessions()
    (hours, points, order), _ = _full_curve(recs, policy)
    k = len(order) // 2
    for budget_hours, commits in ((hours[k], k), ((hours[k] + hours[k + 1]) / 2, k), (hours[0], 0), (hours[-1] + 1, len(order))):
        (rows, h, p, o), replays, stats = _ranked(monkeypatch, replay_tree, policy, budget_hours=budget_hours)
        assert o == order[:commits] and np.array_equal(h, hours[:commits + 1]) and np.array_equal(p, points[:commits + 1])
        assert h[-1] <= budget_hours and (commits == len(order) or hours[commits + 1] > budget_hours)
        for i, r in enumerate(replays):                                              # one look-ahead round per video at the most
            committed = 1 + sum(1 for v, _ in o if v == i)
            assert r.step_calls <= committed + 1, (i, r.step_calls, committed)
        assert stats["committed_rounds"] == len(rows) == len(recs) + commits and stats["lookahead_rounds"] <= len(recs)
        assert sum(r.n for r in replays) == stats["committed_rounds"] + stats["lookahead_rounds"]
    assert sum(r.n for r in replays) > 0


@pytest.mark.parametrize("policy", ["oracle_oracle", "eva_vos"])
def test_a_target_metric_stops_at_the_first_point_that_reaches_it(monkeypatch, replay_tree, policy):
    _, recs = golden_sessions()
    (hours, points, order), _ = _full_curve(recs, policy)
    k = len(order) // 2
    for target in (points[k], (points[k] + points[k - 1]) / 2, points[0], 2.0):
        first = next((j for j, v in enumerate(points) if v >= target), len(points) - 1)
        (rows, h, p, o), replays, _ = _ranked(monkeypatch, replay_tree, policy, target_metric=target)
        assert np.array_equal(p, points[:first + 1]) and np.array_equal(h, hours[:first + 1]) and o == order[:first]
        assert (p[:-1] < target).all()
        for i, r in enumerate(replays):
            assert r.step_calls <= 2 + sum(1 for v, _ in o if v == i)


# ------------------------------------------------------------------------------------------------ residency and refusals
def test_the_residency_rule_refuses_before_the_engine_that_does_not_fit(monkeypatch, tmp_path):
    import mivos.inference_core
    root = str(tmp_path / "db")
    imset = fq_driver.make_synthetic_tree(root, {"a": (3, 16, 16, 1), "b": (3, 16, 16, 1), "c": (3, 16, 16, 1)})
    log = []
    monkeypatch.setattr(mivos.inference_core, "InferenceCore", fake_core_class(log))
    monkeypatch.setattr(metrics, "RoundScorer", DriverScorer)
    engines = lambda: sum(1 for e in log if e[0] == "new")                          # noqa: E731
    # 150 units free; an engine and its first two rounds take 40: the second is admitted at 110 (>= 40 + 40), the third is not at 70
    monkeypatch.setattr(budget, "free_device_bytes", lambda device: 150 - 40 * engines())
    with pytest.raises(ValueError, match=r"2 of the 3 videos fit .*--working-size.*smaller imset"):
        budget.run_ranked(root, imset, "", None, None, "oracle_mask", rounds=3, device="cpu", lanes=1)
    assert engines() == 2                                                            # nobody asked for a third
    del log[:]
    monkeypatch.setattr(budget, "free_device_bytes", lambda device: 160 - 40 * engines())
    stats = {}
    rows, hours, points, order = budget.run_ranked(root, imset, "", None, None, "oracle_mask", rounds=3, device="cpu", lanes=1, stats=stats)
    assert engines() == 3 and stats["engine_footprint_bytes"] == 40 and stats["engines_created"] == 3
    assert stats["interactions"] == stats["committed_rounds"] + stats["lookahead_rounds"] == sum(1 for e in log if e[0] == "interact")


def test_what_a_ranked_run_refuses(monkeypatch):
    import torch.distributed as dist
    with pytest.raises(ValueError, match="--multi-object is refused"):
        budget.run_ranked("nowhere", "nothing", "", None, None, "oracle_mask", multi_object=True)
    with pytest.raises(ValueError, match="upper_bound_mask is refused.*look-ahead"):
        budget.run_ranked("nowhere", "nothing", "", None, None, "upper_bound_mask")
    with pytest.raises(ValueError, match="eva_vos needs qnet"):
        budget.run_ranked("nowhere", "nothing", "", None, None, "eva_vos")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(ValueError, match="world_size 2 > 1 is refused"):
        budget.run_ranked("nowhere", "nothing", "", None, None, "oracle_mask")
