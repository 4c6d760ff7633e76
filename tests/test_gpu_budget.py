"""The ranked run on the GPU (budget.run_ranked) against the full run (eval_driver.run) on one tree: 3 synthetic videos of 8 frames at
128 x 160 - 80 keys, the smallest frame that still takes the default ``top_k = 50`` - 5 rounds, recipe weights, the ``component`` annotator;
``oracle_mask`` ranks by gain, ``eva_vos`` by the agent's values.  Every comparison is exact: the committed rounds are the full run's rounds,
byte for byte, and the live curve is ``rank_curve`` on the full run's rows."""
import numpy as np
import pytest
import torch

from eva_vos_amd import _lib, budget, eval_driver, fq_driver, ranking, synth

pytestmark = pytest.mark.gpu
ROUNDS, SEED = 5, 4
TREE = {"v0": (8, 128, 160, 1), "v1": (8, 128, 160, 1), "v2": (8, 128, 160, 1)}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("db"))
    return root, fq_driver.make_synthetic_tree(root, TREE)


@pytest.fixture(scope="module")
def policy_args():
    from eva_vos_amd import agent as A
    from eva_vos_amd import qnet as Q
    net = Q.QualityNet()
    net.load_state_dict(synth.recipe_state_dict(net, seed=3))
    agent = A.PPOAgent(state_dict=synth.recipe_state_dict(A.ActorCritic(), seed=5))
    return {"oracle_mask": {}, "eva_vos": dict(annotator="component", qnet=net.cuda().eval(), agent=agent)}


@pytest.fixture(scope="module", params=["oracle_mask", "eva_vos"])
def runs(request, tree, nets, policy_args, tmp_path_factory):
    """Per policy, computed once: the full run's rows (sorted by sample and round) and stats, the ranked run to exhaustion, and the ranked run
    under a budget that admits about half the exhaustive curve's steps."""
    policy, kw = request.param, dict(policy_args[request.param], rounds=ROUNDS, seed=SEED)
    out = tmp_path_factory.mktemp(policy)
    full_stats, live_stats, half_stats = {}, {}, {}
    full = eval_driver.run(*tree, "", nets[0], nets[1], policy, stats=full_stats, **kw)
    full = full[np.lexsort((full[:, 1], full[:, 0]))]
    live = budget.run_ranked(*tree, str(out / "rows.csv"), nets[0], nets[1], policy, stats=live_stats, reference_csv=str(out / "reference.csv"),
                             ranking_csv=str(out / "ranking.csv"), **kw)
    hours = live[1]
    half = budget.run_ranked(*tree, "", nets[0], nets[1], policy, stats=half_stats, budget_hours=float(hours[len(hours) // 2]), lanes=1, **kw)
    print(policy, "full", full_stats.get("interactions"), "live", {k: live_stats[k] for k in ("committed_rounds", "lookahead_rounds", "interactions")},
          "half", {k: half_stats[k] for k in ("committed_rounds", "lookahead_rounds", "interactions")}, "hours", hours.tolist(), "points", live[2].tolist())
    return dict(policy=policy, out=out, full=full, full_stats=full_stats, live=live, live_stats=live_stats, half=half, half_stats=half_stats)


def _same_rounds(full, rows):
    """The rows of ``full`` with the (sample, round) of ``rows``, in their order."""
    index = {(int(r[0]), int(r[1])): j for j, r in enumerate(full)}
    return full[[index[(int(r[0]), int(r[1]))] for r in rows]]


def test_the_committed_rounds_are_the_full_run_s_rounds_byte_for_byte(runs):
    full, (rows, hours, points, order) = runs["full"], runs["live"]
    assert rows.dtype == full.dtype == np.float32 and rows.shape[1] == full.shape[1]
    assert len(full) == 3 * ROUNDS and len(rows) == 3 * (ROUNDS - 1) == runs["live_stats"]["committed_rounds"]     # a video's last round is never reached
    assert np.array_equal(rows.view(np.uint32), _same_rounds(full, rows).view(np.uint32))
    assert sorted(order) == [(i, r) for i in range(3) for r in range(1, ROUNDS - 1)]
    assert runs["live_stats"]["lookahead_rounds"] == 3 and runs["live_stats"]["interactions"] == len(full) == runs["full_stats"]["interactions"]


def test_the_live_ranking_is_rank_curve_on_the_full_run_s_rows(runs):
    spec = eval_driver.POLICY_TABLE[runs["policy"]]
    names = [f"{v}__1" for v in TREE]
    recs = ranking.read_rows(runs["full"], spec, names)
    hours, points, order = ranking.rank_curve(recs, use_values=budget.uses_values(runs["policy"]))
    _, h, p, o = runs["live"]
    assert np.array_equal(h, hours) and np.array_equal(p, points) and o == order and len(p) == 1 + 3 * (ROUNDS - 2)
    fh, fp, fo = ranking.read_ranking_csv(str(runs["out"] / "ranking.csv"))
    assert np.array_equal(fh, hours) and np.array_equal(fp, points) and fo == [(names[i], r) for i, r in order]
    # the reference-schema file holds the committed rounds, value for value
    action_names = spec.action_names(None) if spec.action_names else None
    assert ranking.read_reference_csv(str(runs["out"] / "reference.csv"), action_names) == ranking.read_rows(runs["live"][0], spec, names)
    assert len(open(str(runs["out"] / "rows.csv")).readlines()) == 1 + len(runs["live"][0])


def test_a_budget_runs_a_prefix_of_the_curve_and_fewer_rounds(runs):
    (_, hours, points, order), (rows, h, p, o), stats = runs["live"], runs["half"], runs["half_stats"]
    n = len(hours) // 2
    assert np.array_equal(h, hours[:n + 1]) and np.array_equal(p, points[:n + 1]) and o == order[:n]
    assert np.array_equal(rows.view(np.uint32), _same_rounds(runs["full"], rows).view(np.uint32))
    assert stats["committed_rounds"] == len(rows) == 3 + n
    assert stats["interactions"] == stats["committed_rounds"] + stats["lookahead_rounds"] and stats["lookahead_rounds"] <= 3
    assert stats["interactions"] < runs["full_stats"]["interactions"]
    assert stats["engine_footprint_bytes"] >= 0 and stats["engines_created"] == 3


def test_the_library_is_the_one_built_from_the_tree_s_sources():
    assert _lib.src_hash() == _lib.tree_hash()
