"""The step's fused vector passes (obca_core.h HTP_STEP_FUSE) return the doubles of the passes they replace: the
device solves of tests/_step_cases.py equal, bit for bit, what the device emulation of the commit before the fusion
returned (tests/golden/step_fuse.npz, tests/golden/make_step_fuse.py) -- solution vector, objective, status,
iteration, factorization and restoration counts."""
import numpy as np
import pytest

import _step_cases as S
from headland_trajectory_planning_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _native.Context(0)


@pytest.fixture(scope="module")
def stored():
    return np.load(S.FIXTURE)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", list(S.CASES))
def test_device_equals_the_emulation_before_the_fusion(ctx, stored, name):
    dev = ctx.solve(_native.PackedBatch([S.instance(name)]))
    z = {k: stored[f"{name}_{k}"] for k in ("x", "objective", "status", "iters", "n_factor", "n_resto")}
    assert int(dev.status[0]) == int(z["status"][0]), (dev.status[0], z["status"][0])
    assert int(dev.iterations[0]) == int(z["iters"][0]), (dev.iterations[0], z["iters"][0])
    assert int(dev.n_factor[0]) == int(z["n_factor"][0]), (dev.n_factor[0], z["n_factor"][0])
    assert int(dev.n_resto[0]) == int(z["n_resto"][0]), (dev.n_resto[0], z["n_resto"][0])
    assert np.array_equal(_bits(dev.x[0]), _bits(z["x"])), float(np.max(np.abs(dev.x[0] - z["x"])))
    assert _bits(dev.objective[:1])[0] == _bits(z["objective"])[0]
