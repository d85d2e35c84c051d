"""CPU: the numpy restatement of GCRO-DR with a carried recycle space (tests/gcrodr_recycle_reference.py) -- without a
space it is oracle/gcrodr.py; with one, every later solve of a slowly changing sequence needs fewer Arnoldi steps, reaches
the same solution, and the guards (too short a first cycle, a rank-deficient space) fall back to the fresh solve."""
import numpy as np
import pytest

from isph_amd import workload
import oracle as orc
import gcrodr as gcro
import gcrodr_recycle_reference as rec
from problems import Problem, tgv_spec

TOL = 1e-8


@pytest.fixture(scope="module")
def jitter16():
    pr = Problem(tgv_spec(dim=3, n=16, mode=workload.JITTER))
    return pr.poisson()


def _true_residual(rp, ci, val, b, x):
    n = len(b)
    nv = np.ones(n) / np.sqrt(n)
    bp = b - (b @ nv) * nv
    r = bp - orc.spmv(rp, ci, val, x)
    r -= (r @ nv) * nv
    return np.linalg.norm(r) / np.linalg.norm(bp)


@pytest.mark.parametrize("m,k,prec", rec.PAIRS_D)
def test_without_a_space_it_is_the_oracle(jitter16, m, k, prec):
    rp, ci, val, b = jitter16
    minv = rec.PRECS[prec](rp, ci, val)
    xo, io = gcro.solve(rp, ci, val, b, singular=True, prec=minv, num_blocks=m, num_recycled=k)
    x, info, U = rec.solve(rp, ci, val, b, singular=True, prec=minv, num_blocks=m, num_recycled=k, U0=None, keep=False)
    assert U is None
    assert info["iters"] == io["iters"] and info["restarts"] == io["restarts"] and info["converged"] == io["converged"]
    assert np.linalg.norm(x - xo) <= 1e-12 * np.linalg.norm(xo)


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_carried_space_saves_steps_on_a_sequence(name):
    _, _, prec, m, k = rec.SEQUENCES[name]
    systems = rec.sequence_systems(name)
    fresh = rec.run_sequence(systems, prec, m, k, carry=False)
    carried = rec.run_sequence(systems, prec, m, k, carry=True)
    print(name, "fresh", [i["iters"] for _, i in fresh], "carried",
          ["%d+%d" % (i["iters"], i["applications"]) for _, i in carried])
    assert carried[0][1]["iters"] == fresh[0][1]["iters"] and carried[0][1]["applications"] == 0
    for s in range(1, len(systems)):
        (xf, inf), (xc, inc) = fresh[s], carried[s]
        assert inc["started"] and inc["discarded"] == 0 and inc["applications"] == inc["kk_in"] > 0
        assert inc["converged"] and inf["converged"]
        assert inc["iters"] <= inf["iters"] - 3
        res = _true_residual(*systems[s], xc)
        print("  solve", s, "true residual %.3e" % res)
        assert res <= TOL
        assert np.linalg.norm(xc - xf) <= 1e-6 * np.linalg.norm(xf)


@pytest.mark.parametrize("m,k,prec", rec.PAIRS_D)
def test_same_system_twice(jitter16, m, k, prec):
    rp, ci, val, b = jitter16
    res = rec.run_sequence([jitter16, jitter16], prec, m, k, carry=True)
    (x1, i1), (x2, i2) = res
    print((m, k, prec), "first", i1["iters"], "second %d+%d" % (i2["iters"], i2["applications"]))
    assert i1["converged"] and i2["converged"] and i2["started"]
    assert i2["iters"] <= i1["iters"] - 3
    assert _true_residual(rp, ci, val, b, x2) <= TOL
    assert np.linalg.norm(x2 - x1) <= 1e-6 * np.linalg.norm(x1)


def test_short_first_cycle_keeps_nothing():
    """3-D n = 16 ADVECT, m = 30, k = 10: the first cycle converges in 9 steps <= k"""
    pr = Problem(tgv_spec(dim=3, n=16, mode=workload.ADVECT))
    rp, ci, val, b = pr.poisson()
    x, info, U = rec.solve(rp, ci, val, b, singular=True, num_blocks=30, num_recycled=10, keep=True)
    assert info["converged"] and info["iters"] <= 10 and info["restarts"] == 0
    assert U is None


def test_duplicated_column_trips_the_guard(jitter16):
    rp, ci, val, b = jitter16
    m, k = 20, 5
    x1, i1, U = rec.solve(rp, ci, val, b, singular=True, num_blocks=m, num_recycled=k, keep=True)
    assert U is not None and U.shape[1] >= 2
    bad = U.copy()
    bad[:, 1] = bad[:, 0]
    x2, i2, _ = rec.solve(rp, ci, val, b, singular=True, num_blocks=m, num_recycled=k, U0=bad, keep=True)
    assert i2["discarded"] == 2 and not i2["started"] and i2["applications"] == bad.shape[1]
    assert i2["iters"] == i1["iters"] and i2["restarts"] == i1["restarts"]
    assert np.linalg.norm(x2 - x1) <= 1e-12 * np.linalg.norm(x1)


def test_same_operator_columns_need_no_applications(jitter16):
    """the space and C = Op U of one right-hand side's exit serve the next right-hand side of the same operator as they are"""
    rp, ci, val, b = jitter16
    rng = np.random.default_rng(3)
    m, k = 20, 5
    x1, i1, U = rec.solve(rp, ci, val, b, singular=True, num_blocks=m, num_recycled=k, keep=True)
    b2 = rng.standard_normal(len(b))
    x2, i2, U2 = rec.solve(rp, ci, val, b2, singular=True, num_blocks=m, num_recycled=k, U0=U, C0=i1["C"], keep=True)
    x3, i3, _ = rec.solve(rp, ci, val, b2, singular=True, num_blocks=m, num_recycled=k, U0=U, keep=True)
    assert i2["applications"] == 0 and i3["applications"] == U.shape[1] and i2["started"] and i3["started"]
    assert i2["converged"] and abs(i2["iters"] - i3["iters"]) <= 1
    assert np.linalg.norm(x2 - x3) <= 1e-6 * np.linalg.norm(x3)
