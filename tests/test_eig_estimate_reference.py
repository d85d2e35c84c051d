"""-m "not gpu": the numpy restatement of the eigenvalue estimate (tests/eig_estimate_reference.py) on the four fixtures
of chebyshev_reference.system at k = 10, with the Philox start vector the device uses.

Checked: lambda_est <= rho (the estimate is a Ritz value of D^-1 A, rho a bound of its spectrum -- for the nonsymmetric
fixtures the field of values may exceed the spectrum, so this is a property of these operators, not a theorem), and
1.1 lambda_used >= the true largest real part of the spectrum (numpy.linalg.eigvals of the dense D^-1 A): the condition
for the Chebyshev interval [lambda / ratio, 1.1 lambda] to cover the spectrum.

Measured: the rounding spread s of lambda_est -- the largest relative difference between the restatement as written, with
every dot and norm summed in reversed order, and with numpy.longdouble accumulation.  It is printed here and recomputed
(same function) by tests/test_gpu_eig_estimate.py, whose bound for the device's lambda is max(100 s, 1e-13).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import chebyshev_reference as cr
import eig_estimate_reference as er

FIXTURES = ["tgv16", "wall42", "stencil", "spd"]
K = 10


@functools.lru_cache(maxsize=None)
def matrix(name):
    rp, ci, val, _, _ = cr.system(name)
    n = len(rp) - 1
    return sps.csr_matrix((val, ci, rp), shape=(n, n))


def test_philox_start_vector_is_the_generator_of_the_random_stress():
    """the first word against body_force_reference.philox4x32_10 (the restatement the random stress is pinned with), and
    u in (-1, 1)"""
    import body_force_reference as br
    g = np.array([0, 1, 2, 4095, 2 ** 31 + 5], dtype=np.int64)
    for level in (0, 3):
        w = er.philox_first_word(g, level)
        for gi, wi in zip(g, w):
            ref = br.philox4x32_10((int(gi) & 0xFFFFFFFF, level, 0, 0), er.KEY)
            assert int(np.asarray(ref[0]).ravel()[0]) == int(wi)
    u = er.start_vector(4096)
    assert np.all(np.abs(u) < 1.0) and abs(u.mean()) < 0.05 and len(np.unique(u)) == 4096
    assert not np.array_equal(er.start_vector(64, level=1), er.start_vector(64, level=0))
    assert np.array_equal(er.start_vector(64, offset=64), er.start_vector(128)[64:])


@pytest.mark.parametrize("name", FIXTURES)
def test_estimate_is_below_rho_and_its_boost_covers_the_spectrum(name):
    A = matrix(name)
    e = er.estimate(A, K)
    true = er.true_lambda_max(A)
    s = er.rounding_spread(A, K)
    print("eig-ref %-8s rho %.4f true %.4f lambda_est %.4f steps %d spread %.2e" % (name, e["rho"], true, e["lambda_est"], e["steps"], s))
    assert e["steps"] == K
    assert e["lambda_est"] <= e["rho"]
    assert e["lambda_used"] == e["lambda_est"]
    assert 1.1 * e["lambda_used"] >= true
    assert s < 1e-12


def test_early_stop_and_more_steps_than_rows():
    """a diagonal matrix has D^-1 A = I, an invariant subspace after one step; k is cut to the row count; the clipping"""
    n = 12
    e = er.estimate(sps.diags(np.array([1.0, 2.0, 4.0] * 4)).tocsr(), 10)
    assert e["steps"] == 1 and abs(e["lambda_est"] - 1.0) < 1e-14     # D^-1 A = I: invariant at once
    T = sps.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    e = er.estimate(T, 50)
    assert e["steps"] == n
    assert abs(e["lambda_est"] - er.true_lambda_max(T)) < 1e-12
    assert er.clip(float("nan"), 2.0) == 2.0 and er.clip(-1.0, 2.0) == 2.0 and er.clip(3.0, 2.0) == 2.0 and er.clip(1.5, 2.0) == 1.5


def test_vcycle_with_rho_per_level_is_the_chebyshev_references_cycle():
    """the per-level-lambda V cycle with lambda_l = rho_l is chebyshev_reference.amg_vcycle, bit for bit"""
    rng = np.random.default_rng(2)
    A = matrix("stencil")
    n = A.shape[0]
    agg = np.arange(n) // 6
    P = er.smoothed_prolongator(A, er.tentative_prolongator(agg, np.ones(n)), 4.0 / 3.0, cr.rho_anorm(A))
    Ac = (P.T @ A @ P).tocsr()
    levels = [(A, P), (Ac, None)]
    b = rng.standard_normal(n)
    z = er.amg_vcycle(levels, [cr.rho_anorm(A), cr.rho_anorm(Ac)], b, sweeps=2)
    assert np.array_equal(z, cr.amg_vcycle(levels, b, sweeps=2))
