"""fhip_solve with the matrix as fixed parameters - tapes of 21 to 121 inputs, one set of tapes for every draw - bit for bit with the
host build of the same arithmetic (tests/host_build/solve_host.cpp, 16 threads), and with the reference's acceptance checks: the
reference's medium_linear, big_linear and large_quadratic as one batched call each (SOLVER.md)."""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import solver_util as U
from test_solver_gpu import same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,count", [(10, 1000), (50, 50)], ids=["medium_linear", "big_linear"])
def test_linear_system_batched(n, count):
    fs, keys, free = U.linear_system(F, n)
    os_ = U.linear_system(O, n)[0]
    assert fs[0].var_count() == 2 * n + 1
    rows, mats, sols = U.linear_draws(np.random.default_rng(300 + n), n, count)
    dev = F.solve_batch(fs, keys, free, rows)
    same(dev, U.host_solve(os_, keys, free, rows, threads=16))
    ok = sum(U.linear_ok(mats[i], sols[i], dev[0][i]) for i in range(count))
    assert ok >= 0.9 * count, f"{ok} of {count} solved"


@pytest.mark.parametrize("n,count", [(5, 100), (10, 50)])
def test_quadratic_system_batched(n, count):
    fs, keys, free = U.quadratic_system(F, n)
    os_ = U.quadratic_system(O, n)[0]
    assert fs[0].var_count() == n + n * n + n + 1
    rows, mats, sols = U.quadratic_draws(np.random.default_rng(400 + n), n, count)
    dev = F.solve_batch(fs, keys, free, rows)
    same(dev, U.host_solve(os_, keys, free, rows, threads=16))
    ok = sum(U.quadratic_ok(mats[i], sols[i], dev[0][i]) for i in range(count))
    assert ok >= 0.9 * count, f"{ok} of {count} solved"
