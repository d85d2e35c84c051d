"""Host checks of tests/chebyshev_reference.py, the expected values of tests/test_gpu_chebyshev.py (no GPU).

The recurrence against the closed form of the scaled-and-shifted Chebyshev polynomial, its error bound, the premise
rho >= lambda_max(D^-1 A) on every fixture, and the preconditioned reference solves the GPU tests gate their iteration
counts on.  Iterations of the reference to a true relative residual of 1e-8 (GMRES(50) unless noted), as the tests below
find them:
  stand-alone, degree 3, ratio 30:  tgv16 (singular) 15,  wall42 38,  stencil 34,  spd 19
  SA-AMG with the polynomial, 2 sweeps, ratio 20:  tgv16 (null vector: polynomial on the coarsest level) 14,
  wall42 (dense coarse solve) 14,  spd with PCG 11
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import chebyshev_reference as cr
import krylov_reference as kr

FIXTURES = ["tgv16", "wall42", "stencil", "spd"]
AMG_KW = dict(theta=0.0, block=256, coarse_max=64)


@functools.lru_cache(maxsize=None)
def fixture(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    return sps.csr_matrix((val, ci, rp), shape=(n, n)), b, singular


@functools.lru_cache(maxsize=None)
def oracle_levels(name):
    """the hierarchy on the host: the oracle's restatement, pinned level by level against the device's elsewhere"""
    import oracle as orc
    rp, ci, val, _, singular = cr.system(name)
    n = len(rp) - 1
    nv = np.ones(n) / np.sqrt(n) if singular else None
    G = orc.AMG(rp, ci, val, nullvec=nv, **AMG_KW)
    assert G.levels >= 2
    return cr.levels_from(G, n)


def small_spd():
    return kr.laplace2d(6, 5, seed=3, shift=0.4)


def symmetric_eig(A):
    """eigenpairs of D^-1 A through S = D^-1/2 A D^-1/2: (t, V) with D^-1 A V = V diag(t), V = D^-1/2 Q"""
    d = A.diagonal()
    s = 1.0 / np.sqrt(d)
    S = (A.toarray() * s[:, None]) * s[None, :]
    t, Q = np.linalg.eigh(0.5 * (S + S.T))
    return t, Q * s[:, None], Q / s[:, None]   # V, and the rows of V^-1 as columns: V^-1 = (D^1/2 Q)^T


@pytest.mark.parametrize("ratio", [30.0, 5.0])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 6])
def test_zero_guess_is_the_chebyshev_polynomial_in_the_scaled_operator(degree, ratio):
    """y = p(D^-1 A) D^-1 b with p(t) = (1 - T_d((theta - t) / delta) / T_d(sigma)) / t, through the eigen-decomposition"""
    A = small_spd()
    n = A.shape[0]
    b = np.random.default_rng(degree).standard_normal(n)
    t, V, Vinv_t = symmetric_eig(A)
    alpha, beta, _, _, _ = cr.interval(cr.rho_anorm(A), ratio)
    p = (1.0 - cr.error_polynomial(degree, t, alpha, beta)) / t
    want = V @ (p * (Vinv_t.T @ (b / A.diagonal())))
    got = cr.cheb_apply(A, b, None, degree, ratio)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("ratio", [30.0, 5.0])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 7])
def test_error_propagation_is_bounded_by_one_over_T_d_of_sigma(degree, ratio):
    """from a guess, b = 0: an eigenvector v of D^-1 A with eigenvalue t comes back as e_d(t) v, and
    |e_d(t)| <= 1 / T_d(sigma) on [alpha, beta]"""
    A = small_spd()
    t, V, _ = symmetric_eig(A)
    alpha, beta, _, _, sigma = cr.interval(cr.rho_anorm(A), ratio)
    bound = 1.0 / cr.chebyshev_t(degree, np.array([sigma]))[0]
    e = cr.error_polynomial(degree, t, alpha, beta)
    inside = (t >= alpha) & (t <= beta)
    assert inside.sum() >= 3 and t.max() <= beta
    for k in range(len(t)):
        y = cr.cheb_apply(A, np.zeros(A.shape[0]), V[:, k], degree, ratio)
        assert np.max(np.abs(y - e[k] * V[:, k])) <= 1e-12 * np.max(np.abs(V[:, k]))
    assert np.all(np.abs(e[inside]) <= bound * (1.0 + 1e-12))
    grid = np.linspace(alpha, beta, 2001)
    assert np.max(np.abs(cr.error_polynomial(degree, grid, alpha, beta))) <= bound * (1.0 + 1e-12)


def largest_eigenvalue_modulus(A):
    d = A.diagonal()
    keep = np.flatnonzero(d != 0.0)
    A = A[keep][:, keep]
    B = sps.diags(1.0 / A.diagonal()) @ A
    if B.shape[0] <= 600:
        return float(np.max(np.abs(np.linalg.eigvals(B.toarray()))))
    return float(np.max(np.abs(spla.eigs(B, k=1, which="LM", return_eigenvectors=False, tol=1e-10))))


@pytest.mark.parametrize("name", FIXTURES)
def test_rho_bounds_the_spectrum_on_every_fixture(name):
    """the recurrence assumes lambda_max(D^-1 A) <= rho: verified on the fixtures and on every level the smoother sees"""
    A, _, _ = fixture(name)
    mats = [A] if name == "stencil" else [a for a, _ in oracle_levels(name)]
    for l, a in enumerate(mats):
        d = a.diagonal()
        keep = np.flatnonzero(d != 0.0)
        rho = cr.rho_anorm(a[keep][:, keep])
        lam = largest_eigenvalue_modulus(a)
        print("cheb-rho %-8s level %d rows %5d rho %.4f lambda_max %.4f" % (name, l, a.shape[0], rho, lam))
        assert rho >= lam * (1.0 - 1e-9)


KS = list(range(1, 81))


def reference_iterations(name, kind, solver="gmres"):
    A, b, singular = fixture(name)
    n = A.shape[0]
    null = kr.unit_null(None, n) if singular else None
    if kind == "cheb":
        minv = cr.cheb_minv(A, 3, 30.0)
    else:
        minv = cr.amg_minv(oracle_levels(name), sweeps=2, ratio=20.0, coarse_polynomial=singular)
    if solver == "gmres":
        its = kr.gmres_iterates(A, b, np.zeros(n), KS, 50, minv, null)
    else:
        its = kr.pcg_iterates(A, b, np.zeros(n), KS, minv, null)
    return cr.first_below(its, 1e-8)


@pytest.mark.parametrize("name,kind,solver", [("tgv16", "cheb", "gmres"), ("wall42", "cheb", "gmres"), ("stencil", "cheb", "gmres"),
                                              ("spd", "cheb", "gmres"), ("tgv16", "amg", "gmres"), ("wall42", "amg", "gmres"),
                                              ("spd", "amg", "pcg")])
def test_preconditioned_reference_solves_converge(name, kind, solver):
    """what lets the GPU tests gate on the reference's iteration count"""
    k = reference_iterations(name, kind, solver)
    print("cheb-ref-iters %-8s %-4s %-5s %s" % (name, kind, solver, k))
    assert k is not None and k <= 500


def test_a_symmetric_matrix_gives_a_symmetric_cycle():
    """the polynomial and the V cycle built on it are symmetric operators for a symmetric A: what "Block CG" needs"""
    A, _, _ = fixture("spd")
    n = A.shape[0]
    rng = np.random.default_rng(2)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    for minv in (cr.cheb_minv(A, 3, 30.0), cr.amg_minv(oracle_levels("spd"), 2, 20.0)):
        a, b = np.dot(u, minv(v)), np.dot(v, minv(u))
        assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
