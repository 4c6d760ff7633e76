"""CPU: the video ranking (eva_vos_amd/ranking.py) against the reference's own ``rank_policy``.  tests/golden/ranking.npz holds made-up
session records and what the reference's ``read_exp`` returned for them under both rules (tools/gen_golden_ranking.py).  The comparison is
EXACT in float64: the fixture's qualities are multiples of 1/1024 over 4 or 8 frames and its seconds multiples of 1/4, so every mean and
every sum the reference takes is exact in whichever order its ``set`` of names iterates, and the decimal text pandas reads them from
carries them exactly."""
import numpy as np
import pytest

from eva_vos_amd import eval_driver, ranking
from ranking_cases import golden_sessions


@pytest.mark.parametrize("rule,use_values", [("gain", False), ("values", True)])
def test_rank_curve_equals_the_reference_curve_exactly(rule, use_values):
    g, sessions = golden_sessions()
    hours, points, order = ranking.rank_curve(sessions, use_values=use_values)
    print(rule, "hours", hours.tolist(), "points", points.tolist(), "order", order)
    assert hours.dtype == points.dtype == np.float64
    assert np.array_equal(hours, g[f"{rule}.hours"]) and np.array_equal(points, g[f"{rule}.points"])
    # the reference never reaches a video's last round: 1 + sum(rounds - 2) points, every (video, round) once, rounds in order
    assert len(points) == 1 + sum(len(s["mu_metrics"]) - 2 for s in sessions) == 1 + len(order)
    for i, s in enumerate(sessions):
        assert [r for v, r in order if v == i] == list(range(1, len(s["mu_metrics"]) - 1))


def test_the_fixture_covers_what_it_is_meant_to():
    g, sessions = golden_sessions()
    assert sorted(len(s["mu_metrics"]) for s in sessions) == [3, 4, 5, 6, 7, 9]
    costs = {c for s in sessions for c in s["annotation_times"]}
    assert {80.0, 3.0} <= costs and any(c != int(c) for c in costs)
    assert any(20.0 in row for s in sessions for row in s["round_metrics"])
    read = [v for s in sessions for v in s["rl_values"][1:-1]]
    assert -2.04 in read and -2.0 in read
    # the two rules rank differently on it: each golden curve pins its own branch
    assert not np.array_equal(g["gain.points"], g["values.points"]) and not np.array_equal(g["gain.hours"], g["values.hours"])


def test_the_shifted_value_is_what_is_compared_with_minus_two():
    rec = dict(annotation_times=[80.0, 4.0], rl_values=[-2.0, -2.04])
    assert ranking.video_score(rec, 0, 0.6, True) == 0.0                                # -2.04 + 0.04 == -2: replaced by 0
    rec["rl_values"][1] = -2.0
    assert ranking.video_score(rec, 0, 0.6, True) == (-2.0 + 0.04) / 4.0                # -2 itself is not caught
    rec = dict(annotation_times=[80.0, 80.0, 5.0], rl_values=[-2.0, 0.5, 1.0])
    assert ranking.video_score(rec, 1, 0.5, True) == (1.0 + 0.04) * 0.5 / 5.0           # gamma ** pointer
    assert ranking.video_score(rec, 1, 0.5, True, more=False) == -1e10


def _rec(mus, times, frames, metrics):
    return dict(mu_metrics=mus, annotation_times=times, annotated_frames=frames, round_metrics=metrics)


def test_ties_go_to_the_video_that_appears_first_and_a_short_session_stays_constant():
    a = _rec([0.5, 0.75, 1.0, 1.0], [80, 80, 80, 80], [0, 1, 0, 1], [[1, 0.5], [1, 1.0], [1, 1], [1, 1]])
    b = _rec([0.5, 0.75, 1.0, 1.0], [80, 80, 80, 80], [0, 1, 0, 1], [[1, 0.5], [1, 1.0], [1, 1], [1, 1]])
    short = _rec([0.25], [80], [0], [[0.25, 0.25]])
    hours, points, order = ranking.rank_curve([a, short, b])
    assert order == [(0, 1), (2, 1), (0, 2), (2, 2)]                                   # equal scores: a before b, every time
    assert hours.tolist() == [240 / 3600, 320 / 3600, 400 / 3600, 480 / 3600, 560 / 3600]
    assert points.tolist() == [np.mean([0.5, 0.25, 0.5]), np.mean([0.75, 0.25, 0.5]), np.mean([0.75, 0.25, 0.75]), np.mean([1.0, 0.25, 0.75]),
                               np.mean([1.0, 0.25, 1.0])]
    two = _rec([0.5, 1.0], [80, 80], [0, 1], [[1, 0], [1, 1]])                           # two rounds: its last round is never reached
    hours, points, order = ranking.rank_curve([two])
    assert order == [] and points.tolist() == [0.5] and hours.tolist() == [80 / 3600]
    with pytest.raises(ValueError, match="first round"):
        ranking.rank_curve([_rec([], [], [], [])])


@pytest.mark.parametrize("with_tail", [True, False])
def test_the_reference_csv_gives_its_records_back_exactly(tmp_path, with_tail):
    g, sessions = golden_sessions()
    names = [str(n) for n in g["action_names"]]
    if not with_tail:
        sessions = [{k: v for k, v in s.items() if k not in ("rl_values", "annotation_actions")} for s in sessions]
    path = str(tmp_path / "sub" / "eva_vos_reference.csv")
    ranking.write_reference_csv(path, sessions, names)
    head = open(path).readline().strip().split(",")
    assert head == ["video", "mu_metric", "annotation_time", "round", "round_metrics", "annotated_frames"] + (["rl_values", "annotation_actions"] if with_tail else [])
    assert ranking.read_reference_csv(path, names) == sessions
    if with_tail:
        assert ranking.read_reference_csv(path)[0]["annotation_actions"][0] == "mask"     # the file holds the names


def test_awkward_floats_survive_the_reference_csv(tmp_path):
    rec = dict(video="v__1", mu_metrics=[1 / 3, float(np.float32(0.1))], annotation_times=[80, 4.5], annotated_frames=[0, 3],
               round_metrics=[[0.1, 20.0, 1e-7, 2 / 3], [float(np.float32(1 / 3)), 20.0, 1.0, 5e-324]], rl_values=[-2, 0.1 + 0.2])
    path = str(tmp_path / "x.csv")
    ranking.write_reference_csv(path, [rec], seconds=float)
    assert ranking.read_reference_csv(path) == [rec]


def test_read_rows_builds_the_records_from_a_run_s_rows():
    spec = eval_driver.POLICY_TABLE["eva_vos"]
    width = 6 + 4 + 2

    def row(sid, r, mu, sec, f, q, action, value):
        x = np.full(width, np.nan, np.float32)
        x[:6] = (sid, r, mu, sec, f, len(q))
        x[6:6 + len(q)] = q
        x[-1], x[-2] = value, action
        return x
    rows = np.stack([row(1, 1, 0.75, 4.5, 2, [1, 0.5, 1], 0, 0.3), row(0, 0, 0.5, 80, 0, [1, 0.25, 20, 0.5], 1, -2), row(1, 0, 0.5, 80, 0, [1, 0.5, 0.5], 1, -2),
                     row(0, 1, 0.625, 3, 2, [1, 0.5, 20, 0.5], 2, 0)])
    recs = ranking.read_rows(rows, spec, names=["a__1", "a__2"])
    assert [r["video"] for r in recs] == ["a__1", "a__2"]                             # by sample id, whatever the order of the rows
    assert recs[0] == dict(video="a__1", mu_metrics=[0.5, 0.625], annotation_times=[80.0, 3.0], annotated_frames=[0, 2],
                           round_metrics=[[1, 0.25, 20, 0.5], [1, 0.5, 20, 0.5]], rl_values=[-2.0, 0.0], annotation_actions=[1, 2])
    assert recs[1]["rl_values"] == [-2.0, float(np.float32(0.3))] and recs[1]["round_metrics"][1] == [1, 0.5, 1]
    plain = ranking.read_rows(rows[:, :10], None)
    assert "rl_values" not in plain[0] and plain[0]["video"] == 0 and plain[0]["mu_metrics"] == [0.5, 0.625]
    with pytest.raises(ValueError, match="rounds"):
        ranking.read_rows(rows[:1], spec)


def test_the_ranking_csv_reads_back(tmp_path):
    _, sessions = golden_sessions()
    hours, points, order = ranking.rank_curve(sessions)
    path = str(tmp_path / "ranking.csv")
    ranking.write_ranking_csv(path, sessions, hours, points, order)
    assert open(path).readline().strip() == "step,video,round,hours,metric"
    h, p, o = ranking.read_ranking_csv(path)
    assert np.array_equal(h, hours) and np.array_equal(p, points) and o == [(sessions[i]["video"], r) for i, r in order]
