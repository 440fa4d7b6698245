"""CPU: bench.py's instance cache returns what the generator returned (same arrays, bit for bit, same scene
draws), whole files only, and a stored slice is what a later call loads instead of generating."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_cached_slice_equals_the_generated_slice(tmp_path, monkeypatch):
    cache = str(tmp_path / "cache")
    fresh = bench.generate_own_slice(6, "D", 0, 1, procs=1)
    first = bench.cached_own_slice(6, "D", 0, 1, 1, cache)            # generates and stores
    files = os.listdir(cache)
    assert len(files) == 1 and files[0].startswith("D_orchard_6_0of1_") and files[0].endswith(".npz")
    assert ".tmp." not in files[0]
    monkeypatch.setattr(bench, "generate_own_slice", lambda *a, **k: (_ for _ in ()).throw(AssertionError("generated")))
    again = bench.cached_own_slice(6, "D", 0, 1, 1, cache)            # loads
    for got in (first, again):
        assert got.batch == fresh.batch and got.n_var == fresh.n_var and got.turns == fresh.turns
        assert json.loads(json.dumps(got.metas)) == json.loads(json.dumps(fresh.metas))   # stored as JSON
        for k in fresh.INPUTS:
            a, b = getattr(fresh, k), getattr(got, k)
            assert (a is None and b is None) or (a.dtype == b.dtype and a.tobytes() == b.tobytes()), k
        assert np.array_equal(got.obs_edges, fresh.obs_edges) and np.array_equal(got.body_edges, fresh.body_edges)
