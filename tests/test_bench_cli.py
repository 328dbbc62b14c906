"""CPU-side checks of bench.py's output dump (no GPU needed): the files a
--dump-outputs run leaves are float32/float64 .npy arrays holding exactly
what the timed step returned."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "dingo-store_amd")]

import bench  # noqa: E402


def test_dump_outputs_roundtrip(tmp_path):
    rng = np.random.default_rng(5)
    dist = rng.random((7, 10), dtype=np.float32)
    ids = rng.integers(-1, 10_000_000, (7, 10), dtype=np.int64)
    out = tmp_path / "nested" / "dump"  # created on demand
    bench.dump_outputs(str(out), torch.from_numpy(dist),
                       torch.from_numpy(ids))
    assert sorted(os.listdir(out)) == ["distances.npy", "ids.npy"]
    d = np.load(out / "distances.npy")
    i = np.load(out / "ids.npy")
    assert d.dtype == np.float32 and i.dtype == np.float64
    np.testing.assert_array_equal(d, dist)
    np.testing.assert_array_equal(i.astype(np.int64), ids)


def test_dump_outputs_samples_large_output(tmp_path):
    """Above the size cap the dump is a fixed seeded row sample: within the
    cap, identical from call to call, and rows.npy says which rows."""
    rng = np.random.default_rng(6)
    nq, k, cap = 500, 10, 16 << 10
    dist = torch.from_numpy(rng.random((nq, k), dtype=np.float32))
    ids = torch.from_numpy(rng.integers(0, 1 << 40, (nq, k), dtype=np.int64))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), dist, ids, max_bytes=cap)
    bench.dump_outputs(str(b), dist, ids, max_bytes=cap)
    total = sum(os.path.getsize(a / f) for f in os.listdir(a))
    assert total <= cap
    rows = np.load(a / "rows.npy").astype(np.int64)
    assert 1 <= len(rows) < nq and len(set(rows.tolist())) == len(rows)
    np.testing.assert_array_equal(np.load(a / "distances.npy"),
                                  dist.numpy()[rows])
    np.testing.assert_array_equal(
        np.load(a / "ids.npy").astype(np.int64), ids.numpy()[rows])
    for f in ("rows.npy", "distances.npy", "ids.npy"):
        np.testing.assert_array_equal(np.load(a / f), np.load(b / f))
