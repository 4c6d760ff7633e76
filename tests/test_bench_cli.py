"""CPU: bench.py's options - a plain run is the headline alone (--full adds the other legs), --dump-outputs writes float32 arrays
within the size budget, a large output as a fixed seeded sample."""
import os

import numpy as np


def test_plain_run_is_the_default_and_full_is_an_option():
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out", "--steps", "5", "--warmup", "2"])
    assert a.full is True and a.dump_outputs == "out" and a.steps == 5 and a.warmup == 2


def test_dump_outputs_float32_within_budget_and_seeded(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    big = [(f"masks_clip{c}", rng.integers(0, 3, (40, 480, 854), dtype=np.uint8)) for c in range(8)]
    small = [("small", np.arange(12, dtype=np.uint8).reshape(3, 4))]
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big + small)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted([n + ".npy" for n, _ in big + small])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6
    share = bench.DUMP_ELEMS // len(big + small)
    for name, x in big:
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == (share,)
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{name}.npy")), "same arguments, same sample"
        assert set(np.unique(got).tolist()) <= {0.0, 1.0, 2.0}
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, np.arange(12).reshape(3, 4)), "an array within its share is written whole"
