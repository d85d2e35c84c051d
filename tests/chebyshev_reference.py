"""Plain numpy / scipy restatement of the Chebyshev polynomial in D^-1 A and of the SA-AMG V cycle that smooths with it
(host only, not a test module).  Nothing here shares code with the device.

The recurrence is Ifpack_Chebyshev::ApplyInverse / ML_Cheby as include/isph_hip.h states it (isph_cheb_params):
    lambda = rho = max_i sum_j |a_ij| / |a_ii|,  beta = 1.1 lambda,  alpha = lambda / ratio,
    theta = (beta + alpha) / 2,  delta = (beta - alpha) / 2,  sigma = theta / delta,  rho_0 = 1 / sigma
    step 1:        w = (1 / theta) D^-1 (b - A y),                                          y += w
    step k = 2..d: rho_k = 1 / (2 sigma - rho_{k-1}),
                   w = rho_k rho_{k-1} w + (2 rho_k / delta) D^-1 (b - A y),                y += w
"""
import numpy as np
import scipy.sparse as sps


def as_csr(A):
    A = sps.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    return A


def rho_anorm(A):
    """||D^-1 A||_inf: an upper bound of the spectral radius of D^-1 A ("eigen-analysis: type" Anorm)"""
    A = as_csr(A)
    d = A.diagonal()
    assert np.all(d != 0.0)
    return float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / np.abs(d)))


def interval(lam, ratio):
    """(alpha, beta, theta, delta, sigma)"""
    beta, alpha = 1.1 * lam, lam / ratio
    theta, delta = 0.5 * (beta + alpha), 0.5 * (beta - alpha)
    return alpha, beta, theta, delta, theta / delta


def cheb_apply(A_csr, b, y0, degree, ratio, lam=None):
    """y after `degree` steps from y0 (None: the zero guess, whose first step needs no product)"""
    A = as_csr(A_csr)
    dinv = 1.0 / A.diagonal()
    lam = rho_anorm(A) if lam is None else float(lam)
    _, _, theta, delta, sigma = interval(lam, ratio)
    b = np.asarray(b, dtype=np.float64)
    if y0 is None:
        y = np.zeros(A.shape[0])
        w = dinv * b / theta
    else:
        y = np.array(y0, dtype=np.float64)
        w = dinv * (b - A @ y) / theta
    y = y + w
    rho_old = 1.0 / sigma
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho_old)
        w = rho_new * rho_old * w + (2.0 * rho_new / delta) * (dinv * (b - A @ y))
        y = y + w
        rho_old = rho_new
    return y


def cheb_minv(A_csr, degree, ratio, lam=None):
    """the stand-alone preconditioner: zero start"""
    A = as_csr(A_csr)
    lam = rho_anorm(A) if lam is None else lam
    return lambda r: cheb_apply(A, r, None, degree, ratio, lam)


def levels_from(M, n0):
    """[(A_l, P_l or None)] of a hip.PrecondAMG (or anything with levels / level_info / export)"""
    out, n = [], n0
    for l in range(M.levels):
        rp, ci, v = M.export(l, "A")
        A = sps.csr_matrix((v, ci, rp), shape=(n, n))
        P = None
        if l < M.levels - 1:
            nc = M.level_info(l + 1)["rows"]
            rp, ci, v = M.export(l, "P")
            P = sps.csr_matrix((v, ci, rp), shape=(n, nc))
            n = nc
        out.append((A, P))
    return out


def _level_smooth(A, b, y0, degree, ratio):
    """the polynomial of one level; a row without entries (coarse operators can have them) is left alone"""
    d = A.diagonal()
    if np.all(d != 0.0):
        return cheb_apply(A, b, y0, degree, ratio)
    keep = np.flatnonzero(d != 0.0)
    assert abs(A[d == 0.0]).sum() == 0.0
    y = np.zeros(A.shape[0]) if y0 is None else np.array(y0, dtype=np.float64)
    y[keep] = cheb_apply(A[keep][:, keep], np.asarray(b)[keep], None if y0 is None else y[keep], degree, ratio)
    return y


def amg_vcycle(levels, b, sweeps=1, ratio=20.0, coarse_polynomial=False, l=0):
    """one V cycle over levels = [(A_l, P_l)], R = P^T: Chebyshev of degree `sweeps` from a zero guess before the coarse
    correction and from x after it; the coarsest level is numpy.linalg.solve, or the polynomial when a null vector was
    given to the hierarchy (coarse_polynomial)"""
    A, P = levels[l]
    if l == len(levels) - 1:
        if coarse_polynomial:
            return _level_smooth(A, b, None, sweeps, ratio)
        return np.linalg.solve(A.toarray(), b)
    x = _level_smooth(A, b, None, sweeps, ratio)
    e = amg_vcycle(levels, P.T @ (b - A @ x), sweeps, ratio, coarse_polynomial, l + 1)
    x = x + P @ e
    return _level_smooth(A, b, x, sweeps, ratio)


def amg_minv(levels, sweeps=1, ratio=20.0, coarse_polynomial=False):
    return lambda r: amg_vcycle(levels, r, sweeps, ratio, coarse_polynomial)


def chebyshev_t(d, x):
    """T_d(x) for real x, |x| <= 1 or not"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    inside = np.abs(x) <= 1.0
    out[inside] = np.cos(d * np.arccos(x[inside]))
    xo = x[~inside]
    out[~inside] = np.sign(xo) ** d * np.cosh(d * np.arccosh(np.abs(xo)))
    return out


def error_polynomial(d, lam_values, alpha, beta):
    """e_d(t) = T_d((theta - t) / delta) / T_d(sigma): what the d-step recurrence leaves of the error component with
    eigenvalue t of D^-1 A; 1 - t p(t) with p the polynomial cheb_apply applies"""
    theta, delta = 0.5 * (beta + alpha), 0.5 * (beta - alpha)
    return chebyshev_t(d, (theta - np.asarray(lam_values)) / delta) / chebyshev_t(d, np.array([theta / delta]))[0]


# ---------------------------------------------------------------- systems the Chebyshev tests share
def first_below(iterates, tol=1e-8):
    """smallest k whose true relative residual is <= tol (None when no recorded iterate gets there)"""
    for k in sorted(iterates):
        if iterates[k].rel_res <= tol:
            return k
    return None


def system(name):
    """(rowptr, colidx, val, b, singular) of the fixtures by name:
    tgv16   3-D TGV pressure rows, 16^3 = 4096 rows (four column windows of 1024), singular
    wall42  2-D wall case, NotSingular, 42^2 = 1764 rows: not a multiple of 64, the last slice is a tail
    stencil krylov_reference.stencil3d(7, 6, 5) + 0.5 I: 210 rows, nonsymmetric
    spd     krylov_reference.laplace2d(40, 37) + shift: 1480 rows, symmetric positive definite"""
    import krylov_reference as kr
    if name in ("tgv16", "wall42"):
        import oracle as orc
        from isph_amd import workload
        from problems import Problem, tgv_spec, wall_types
        if name == "tgv16":
            pr = Problem(tgv_spec(dim=3, n=16, mode=workload.JITTER, brick=8))
        else:
            pr = Problem(tgv_spec(dim=2, n=42, mode=workload.JITTER, brick=7), singular=orc.NOT_SINGULAR,
                         kinds=[orc.FLUID, orc.SOLID], types=wall_types)
        rp, ci, val, b = pr.poisson()
        return rp, ci, val, b, name == "tgv16"
    A = kr.stencil3d(7, 6, 5, shift=0.5) if name == "stencil" else kr.laplace2d(40, 37, seed=21, shift=0.3)
    n = A.shape[0]
    b = np.random.default_rng(31).standard_normal(n)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), b, False


def coordinates(name):
    """row coordinates of the lattice fixtures (for the library's own numbering)"""
    if name == "stencil":
        nx, ny, nz = 7, 6, 5
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64), 3
    assert name == "spd"
    j, i = np.meshgrid(np.arange(37), np.arange(40), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), np.zeros(40 * 37)], axis=1).astype(np.float64), 2
