"""CPU: the plain Krylov iterate reference (tests/krylov_reference.py) against the oracle's GMRES / PCG at tol = 0.

The oracle's x_k must reproduce the reference's for every orthogonalisation, flexible or not, singular or not, with
and without restarts; its recurrence residual must equal the true residual of x_k.  The negative controls show that
the comparison rejects the neighbouring iterates and an iterate from a Hessenberg matrix perturbed by 1e-8.

Measured (oracle vs reference, maximum over k): GMRES iterates <= 5.3e-14 relative, PCG <= 4.5e-14; recurrence
residuals within 1.4e-14 of the true ones (relative to ||r0||).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import krylov_reference as kr

KS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 61, 62]   # every multi-dot batch / k_multi_axpy_dot instance edge
ITER_TOL = 2e-13      # oracle vs reference, x_k relative (measured <= 5.3e-14)
RES_TOL = 5e-14       # |rel_res_implicit - true_rel_res| (measured <= 1.4e-14)
ROUND_OFF = 1e-10     # below this true residual x_k is round-off: no case may sit there


@functools.lru_cache(maxsize=None)
def system(singular):
    rp, ci, val = kr.tgv_rows(None if singular else kr.SHIFT)
    n = len(rp) - 1
    return rp, ci, val, sps.csr_matrix((val, ci, rp), shape=(n, n)), np.random.default_rng(7).standard_normal(n)


@functools.lru_cache(maxsize=None)
def reference(singular, prec, m=62, ks=tuple(KS)):
    rp, ci, val, A, b = system(singular)
    n = A.shape[0]
    return kr.gmres_iterates(A, b, np.zeros(n), ks, m, kr.minv_for(prec, rp, ci, val), kr.unit_null(None, n) if singular else None)


def kept(singular, prec):
    ref = reference(singular, prec)
    return [k for k in KS if ref[k].rel_res >= ROUND_OFF]


@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("prec", ["none", "jacobi", "bjacobi-ilu0"])
@pytest.mark.parametrize("flexible", [1, 0])
@pytest.mark.parametrize("ortho", [0, 1, 2])
def test_oracle_iterates_equal_the_reference(ortho, flexible, singular, prec):
    rp, ci, val, A, b = system(singular)
    ref = reference(singular, prec)
    ks = kept(singular, prec)
    assert len(ks) >= (6 if prec == "bjacobi-ilu0" else 13)    # ILU(0) converges faster: only the k above round-off
    gx = gr = 0.0
    for k in ks:
        x, info = kr.oracle_solve(rp, ci, val, b, None, k, 62, ortho, flexible, singular, prec)
        assert info.iters == k and info.restarts == 0 and info.converged == 0
        gx = max(gx, kr.iterate_gap(x, ref[k].x))
        gr = max(gr, kr.residual_gap(info.rel_res_implicit, ref[k]))
    assert gx <= ITER_TOL and gr <= RES_TOL, (gx, gr)


@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("flexible", [1, 0])
@pytest.mark.parametrize("ortho", [0, 1, 2])
@pytest.mark.parametrize("m", [1, 5])
def test_oracle_restarted_iterates_equal_the_reference(m, ortho, flexible, singular):
    rp, ci, val, A, b = system(singular)
    n = A.shape[0]
    x0 = np.random.default_rng(8).standard_normal(n)
    ref = kr.gmres_iterates(A, b, x0, [13], m, kr.minv_for("jacobi", rp, ci, val), kr.unit_null(None, n) if singular else None)[13]
    assert ref.rel_res >= ROUND_OFF
    x, info = kr.oracle_solve(rp, ci, val, b, x0, 13, m, ortho, flexible, singular, "jacobi")
    assert info.iters == 13 and info.restarts == 12 // m
    assert kr.iterate_gap(x, ref.x) <= ITER_TOL and kr.residual_gap(info.rel_res_implicit, ref) <= RES_TOL


@pytest.mark.parametrize("k", [2, 17, 33, 49, 61])
def test_the_comparison_rejects_neighbours_and_a_perturbed_hessenberg(k):
    """the tolerance bites: x_{k-1}, x_{k+1} and x_k from a Hessenberg matrix with H[0,0] scaled by (1 + 1e-8) all fail
    the comparison that the oracle's x_k passes"""
    rp, ci, val, A, b = system(True)
    n = A.shape[0]
    nul = kr.unit_null(None, n)
    ref = kr.gmres_iterates(A, b, np.zeros(n), [k - 1, k, k + 1], 62, None, nul)
    bad = kr.gmres_iterates(A, b, np.zeros(n), [k], 62, None, nul, perturb=(0, 0, 1e-8))[k]
    x, _ = kr.oracle_solve(rp, ci, val, b, None, k, 62, singular=True)
    assert kr.iterate_gap(x, ref[k].x) <= ITER_TOL
    for wrong in (ref[k - 1].x, ref[k + 1].x, bad.x):
        assert kr.iterate_gap(wrong, ref[k].x) > 100 * ITER_TOL
        assert kr.iterate_gap(x, wrong) > 100 * ITER_TOL


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_tiny_sizes_and_the_exact_solution_at_k_equal_n(n):
    A = kr.tiny(n)
    b = np.random.default_rng(n).standard_normal(n)
    rp, ci, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data
    ks = sorted({k for k in (1, 2, 17, 62, n) if k <= n})
    ref = kr.gmres_iterates(A, b, np.zeros(n), ks, 62, None)
    for k in ks:
        x, info = kr.oracle_solve(rp, ci, val, b, None, k, 62)
        assert info.iters == k
        assert kr.iterate_gap(x, ref[k].x) <= ITER_TOL and kr.residual_gap(info.rel_res_implicit, ref[k]) <= RES_TOL
    if n <= 62:   # a full Krylov space without restart: the exact solution
        assert kr.iterate_gap(ref[n].x, np.linalg.solve(A.toarray(), b)) <= 1e-14


@pytest.mark.parametrize("singular", [False, True])
@pytest.mark.parametrize("prec", ["none", "jacobi"])
def test_oracle_pcg_iterates_equal_the_reference(singular, prec):
    A = kr.laplace2d(121, 119, seed=3, shift=None if singular else 0.3)
    n = A.shape[0]
    rp, ci, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data
    b = np.random.default_rng(4).standard_normal(n)
    ks = [1, 2, 17, 49]
    ref = kr.pcg_iterates(A, b, np.zeros(n), ks, kr.minv_for(prec, rp, ci, val), kr.unit_null(None, n) if singular else None)
    for k in ks:
        assert ref[k].rel_res >= ROUND_OFF
        x, info = kr.oracle_solve(rp, ci, val, b, None, k, 62, singular=singular, prec=prec, solver_type=1)
        assert info.iters == k
        assert kr.iterate_gap(x, ref[k].x) <= ITER_TOL and kr.residual_gap(info.rel_res_implicit, ref[k]) <= RES_TOL
