"""CPU: the rows and the CSV files of the two drivers (eval_driver.run for a mask policy in both modes, a random one, two mixed-annotation
policies and ``eva_vos``; fq_driver.run) on the fakes of session_fakes.py and a synthetic dataset tree.  tests/golden/driver_rows.npz holds
what the drivers returned and wrote before their session loops, policy branches and rank plumbing were merged: the row arrays have to
come back bit for bit (NaN padding included) and the files byte for byte - column order, ``annotation_time`` as an int for the mask policies and
as a float for the typed ones, the ``rl_values`` and ``annotation_actions`` tails."""
import os

import numpy as np
import pytest

from eva_vos_amd import eval_driver, fq_driver, metrics
from session_fakes import Annotator, CyclingAgent, DriverObjectScorer, DriverScorer, DriverSelector, DriverTypedScorer, fake_core_class

GOLD = os.path.join(os.path.dirname(__file__), "golden", "driver_rows.npz")
TREE = {"a": (3, 48, 64, 3), "b": (4, 48, 64, 2)}
ROUNDS, SEED = 5, 4
# policy, keywords of eval_driver.run
CASES = {
    "oracle_mask": ("oracle_mask", {}),
    "rand_mask": ("rand_mask", {}),
    "oracle_mask_multi_object": ("oracle_mask", dict(multi_object=True)),
    "rand_type": ("rand_type", dict(annotation_types=["3clicks"])),
    "oracle_oracle": ("oracle_oracle", dict(annotation_types=["click", "bbox", "mask"])),
    "eva_vos": ("eva_vos", dict(qnet="qnet")),
    "fq": (None, {}),
}


def install_fakes(monkeypatch):
    import mivos.inference_core
    from eva_vos_amd import qnet
    monkeypatch.setattr(mivos.inference_core, "InferenceCore", fake_core_class([]))
    monkeypatch.setattr(metrics, "TypedRoundScorer", DriverTypedScorer)
    monkeypatch.setattr(qnet, "QNetSelector", DriverSelector)


def drive(case, monkeypatch, root, imset, out_dir):
    """(rows, CSV bytes) of one run."""
    policy, kw = CASES[case]
    monkeypatch.setattr(metrics, "RoundScorer", DriverObjectScorer if kw.get("multi_object") else DriverScorer)
    if policy is None:
        rows = fq_driver.run(root, imset, out_dir, None, None, rounds=ROUNDS, save_masks=False, device="cpu", lanes=1)
        path = os.path.join(out_dir, "res_synthetic.csv")
    else:
        kw = dict(kw)
        if policy in eval_driver.TYPED_POLICIES + eval_driver.AGENT_POLICIES:
            kw["annotator"] = lambda: Annotator([])
        if policy in eval_driver.AGENT_POLICIES:
            kw["agent"] = CyclingAgent()
        path = os.path.join(out_dir, "rows.csv")
        rows = eval_driver.run(root, imset, path, None, None, policy, rounds=ROUNDS, seed=SEED, device="cpu", lanes=1, **kw)
    return np.asarray(rows), open(path, "rb").read()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("db"))
    return root, fq_driver.make_synthetic_tree(root, TREE)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_drivers_return_the_recorded_rows_and_write_the_recorded_csv(case, tree, tmp_path, monkeypatch):
    install_fakes(monkeypatch)
    rows, text = drive(case, monkeypatch, *tree, str(tmp_path))
    gold = np.load(GOLD)
    print(case, rows.shape, text[:200])
    assert rows.dtype == gold[case + "_rows"].dtype and np.array_equal(rows, gold[case + "_rows"], equal_nan=True)
    assert text == gold[case + "_csv"].tobytes()


def test_the_recorded_runs_cover_what_they_are_meant_to():
    gold = np.load(GOLD)
    width = {c: gold[c + "_rows"].shape[1] for c in CASES}
    t_max = max(v[0] for v in TREE.values())
    assert width["fq"] == 4 + t_max and width["oracle_mask"] == width["rand_mask"] == width["oracle_mask_multi_object"] == 6 + t_max
    assert width["rand_type"] == width["oracle_oracle"] == 7 + t_max and width["eva_vos"] == 8 + t_max
    head = {c: gold[c + "_csv"].tobytes().split(b"\r\n")[0] for c in CASES}
    assert head["oracle_mask"] == head["oracle_mask_multi_object"] == b"video,mu_metric,annotation_time,round"
    assert head["rand_type"] == b"video,mu_metric,annotation_time,round,annotation_actions"
    assert head["eva_vos"] == b"video,mu_metric,annotation_time,round,rl_values,annotation_actions" and head["fq"] == b"state_name,ious,selected_frame"
    second = {c: gold[c + "_csv"].tobytes().split(b"\r\n")[1].split(b",") for c in CASES}
    assert second["oracle_mask"][2] == b"80" and second["rand_type"][2] == b"80.0" and second["eva_vos"][2] == b"80.0"      # int against float seconds
    assert second["eva_vos"][4:] == [b"-2.0", b"mask"]
    multi = gold["oracle_mask_multi_object_rows"]
    assert (multi[:, 3] == eval_driver.SKIP_SECONDS).any() and len(np.unique(multi[:, 0])) == 5                     # an object absent from the annotated frame
    for c in ("rand_type", "oracle_oracle", "eva_vos"):                                                               # more than one action, frames that repeat
        rows = gold[c + "_rows"]
        col = -2 if c == "eva_vos" else -1
        assert len(np.unique(rows[:, col])) > 1 or c == "rand_type", c
        assert any(len(set(r[4] for r in rows if r[0] == s)) < (rows[:, 0] == s).sum() for s in np.unique(rows[:, 0])), c
