"""The sessions of tests/golden/ranking.npz as the records ``ranking.rank_curve`` takes, for the tests of the ranking and of the ranked run.
A plain module, not a conftest: the tests import what they use."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ranking.npz")


def golden_sessions():
    g = np.load(GOLD)
    sessions = []
    for i, name in enumerate(g["names"]):
        sessions.append(dict(video=str(name), mu_metrics=g[f"v{i}.mu"].tolist(), annotation_times=g[f"v{i}.times"].tolist(),
                             annotated_frames=g[f"v{i}.frames"].tolist(), round_metrics=g[f"v{i}.metrics"].tolist(),
                             rl_values=g[f"v{i}.values"].tolist(), annotation_actions=g[f"v{i}.actions"].tolist()))
    return g, sessions
