"""Plain numpy restatement of the eigenvalue estimate behind isph_cheb_params::eig_type = 1 and
isph_amg_params::eig_type = 1 (host only, not a test module).  Nothing here shares code with the device.

    B = D^-1 A,  v_0 = u / |u|,  u_g = (w_g + 0.5) / 2^31 - 1 with w_g the first word of Philox4x32-10, key (0x15B4, 0),
    counter (g, level, 0, 0),  g = the global row number in the caller's numbering
    step j: w = B v_j; classical Gram-Schmidt against v_0..v_j applied twice (c1 = V^T w, w -= V c1, c2 = V^T w, w -= V c2),
            h_ij = c1_i + c2_i, h_{j+1,j} = |w|, v_{j+1} = w / |w|; stop when h_{j+1,j} <= 1e-14 |h_00|
    lambda_est = max Re eig(H[:m, :m]),  lambda_used = min(lambda_est, rho), rho when lambda_est is not finite or <= 0

Every dot and norm goes through one function, so that the rounding spread of lambda_est can be measured by changing the
order (reversed) and the width (numpy.longdouble) of the accumulation.
"""
import numpy as np
import scipy.sparse as sps

import chebyshev_reference as cr

KEY = (0x15B4, 0)
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox_first_word(g, level):
    """first output word of Philox4x32-10 for the counters (g_i, level, 0, 0) and KEY; g: integer array"""
    c0 = (np.asarray(g, dtype=np.uint64) & np.uint64(_MASK)).copy()
    c1 = np.full_like(c0, level & _MASK)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = KEY
    sh, mk = np.uint64(32), np.uint64(_MASK)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0   # 32 x 32 -> 64 bits: fits
        p1 = np.uint64(_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> sh, p0 & mk, p1 >> sh, p1 & mk
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0


def start_vector(n, level=0, offset=0, rows=None):
    """u of the rows `rows` (default 0..n-1) shifted by the rank offset"""
    g = (np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)) + offset
    w = philox_first_word(g, level)
    return (w.astype(np.float64) + 0.5) / 2.0 ** 31 - 1.0


def _dot(a, b, mode):
    if mode == "reversed":
        return float(np.dot(a[::-1], b[::-1]))
    if mode == "longdouble":
        return float(np.dot(a.astype(np.longdouble), b.astype(np.longdouble)))
    return float(np.dot(a, b))


def arnoldi(A, k, level=0, mode="plain", offset=0, rows=None):
    """(H, m): the k x k upper Hessenberg matrix and the number of steps taken (m <= k; the leading m x m block counts)"""
    A = cr.as_csr(A)
    n = A.shape[0]
    d = A.diagonal()
    dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)
    k = min(int(k), n)
    u = start_vector(n, level, offset, rows)
    V = np.zeros((k + 1, n))
    V[0] = u / np.sqrt(_dot(u, u, mode))
    H = np.zeros((k, k))
    m = 0
    for j in range(k):
        w = dinv * (A @ V[j])
        c = np.zeros(j + 1)
        for _ in range(2):
            ci = np.array([_dot(V[i], w, mode) for i in range(j + 1)])
            w = w - ci @ V[:j + 1]
            c += ci
        H[:j + 1, j] = c
        hn = np.sqrt(_dot(w, w, mode))
        m = j + 1
        if not np.isfinite(hn) or hn <= 1e-14 * abs(H[0, 0]):
            break
        if j + 1 < k:
            H[j + 1, j] = hn
            V[j + 1] = w / hn
    return H, m


def ritz_max(H, m):
    return float(np.max(np.linalg.eigvals(H[:m, :m]).real))


def clip(lambda_est, rho):
    if not np.isfinite(lambda_est) or lambda_est <= 0.0:
        return rho
    return min(lambda_est, rho)


def rho_anorm(A):
    """||D^-1 A||_inf over the rows that have a diagonal (coarse operators can hold empty rows)"""
    A = cr.as_csr(A)
    d = A.diagonal()
    s = np.asarray(abs(A).sum(axis=1)).ravel()
    keep = d != 0.0
    return float(np.max(s[keep] / np.abs(d[keep]))) if keep.any() else 0.0


def estimate(A, k=10, level=0, mode="plain", offset=0, rows=None):
    """dict(lambda_est, lambda_used, rho, steps)"""
    H, m = arnoldi(A, k, level, mode, offset, rows)
    est = ritz_max(H, m)
    rho = rho_anorm(A)
    return dict(lambda_est=est, lambda_used=clip(est, rho), rho=rho, steps=m)


def rounding_spread(A, k=10, level=0):
    """largest relative difference of lambda_est between the restatement as written, with every dot and norm summed in
    reversed order, and with numpy.longdouble accumulation"""
    vals = [estimate(A, k, level, mode)["lambda_est"] for mode in ("plain", "reversed", "longdouble")]
    return float((max(vals) - min(vals)) / abs(vals[0]))


def true_lambda_max(A):
    """largest real part of the spectrum of D^-1 A (dense)"""
    A = cr.as_csr(A)
    return float(np.max(np.linalg.eigvals((sps.diags(1.0 / A.diagonal()) @ A).toarray()).real))


def fl32(A):
    A = cr.as_csr(A).copy()
    A.data = A.data.astype(np.float32).astype(np.float64)
    return A


# ---------------------------------------------------------------- the V cycle with one lambda per level
def _level_smooth(A, b, y0, degree, ratio, lam):
    d = A.diagonal()
    if np.all(d != 0.0):
        return cr.cheb_apply(A, b, y0, degree, ratio, lam=lam)
    keep = np.flatnonzero(d != 0.0)
    assert abs(A[d == 0.0]).sum() == 0.0
    y = np.zeros(A.shape[0]) if y0 is None else np.array(y0, dtype=np.float64)
    y[keep] = cr.cheb_apply(A[keep][:, keep], np.asarray(b)[keep], None if y0 is None else y[keep], degree, ratio, lam=lam)
    return y


def amg_vcycle(levels, lams, b, sweeps=1, ratio=20.0, coarse_polynomial=False, l=0):
    """chebyshev_reference.amg_vcycle with the interval of level l taken from lams[l] in place of rho"""
    A, P = levels[l]
    if l == len(levels) - 1:
        if coarse_polynomial:
            return _level_smooth(A, b, None, sweeps, ratio, lams[l])
        return np.linalg.solve(A.toarray(), b)
    x = _level_smooth(A, b, None, sweeps, ratio, lams[l])
    e = amg_vcycle(levels, lams, P.T @ (b - A @ x), sweeps, ratio, coarse_polynomial, l + 1)
    x = x + P @ e
    return _level_smooth(A, b, x, sweeps, ratio, lams[l])


def amg_minv(levels, lams, sweeps=1, ratio=20.0, coarse_polynomial=False):
    return lambda r: amg_vcycle(levels, lams, r, sweeps, ratio, coarse_polynomial)


def _sgs_apply(A, r, block):
    """z = M_B^-1 r, M_B = blockdiag[(D + L_B) D^-1 (D + U_B)] over blocks of `block` consecutive rows (rows without a
    diagonal are left at 0)"""
    import scipy.linalg as sla
    n = A.shape[0]
    z = np.zeros(n)
    for s in range(0, n, block):
        e = min(s + block, n)
        B = A[s:e, s:e].toarray()
        keep = np.flatnonzero(np.diag(B) != 0.0)
        if len(keep) == 0:
            continue
        B = B[np.ix_(keep, keep)]
        d = np.diag(B)
        y = sla.solve_triangular(np.tril(B), r[s:e][keep], lower=True)
        z[s + keep] = sla.solve_triangular(np.triu(B), d * y, lower=False)
    return z


def amg_vcycle_sgs(levels, b, sweeps=1, block=256, coarse_block=64, coarse_smooth=False, l=0):
    """one V cycle with `sweeps` block-local symmetric Gauss-Seidel sweeps x += M_B^-1 (b - A x) before (from zero) and
    after the coarse correction; blocks of `block` rows on level 0 and of `coarse_block` rows below; the coarsest level
    is numpy.linalg.solve, or the same sweeps when a null vector was given to the hierarchy (coarse_smooth)"""
    A, P = levels[l]
    bl = block if l == 0 else coarse_block
    if l == len(levels) - 1 and not coarse_smooth:
        return np.linalg.solve(A.toarray(), b)
    x = _sgs_apply(A, b, bl)
    for _ in range(1, sweeps):
        x = x + _sgs_apply(A, b - A @ x, bl)
    if l == len(levels) - 1:
        return x
    e = amg_vcycle_sgs(levels, P.T @ (b - A @ x), sweeps, block, coarse_block, coarse_smooth, l + 1)
    x = x + P @ e
    for _ in range(sweeps):
        x = x + _sgs_apply(A, b - A @ x, bl)
    return x


def tentative_prolongator(agg, nullvec, nagg=None):
    """P_tent from exported aggregates: column = aggregate, entries = the null vector normalised per aggregate (rows
    outside every aggregate, agg < 0, stay empty)"""
    agg = np.asarray(agg)
    nv = np.asarray(nullvec, dtype=np.float64)
    inside = agg >= 0
    nagg = int(agg.max()) + 1 if nagg is None else int(nagg)
    norm = np.sqrt(np.bincount(agg[inside], weights=nv[inside] ** 2, minlength=nagg))
    rows = np.flatnonzero(inside)
    return sps.csr_matrix((nv[rows] / norm[agg[rows]], (rows, agg[rows])), shape=(len(agg), nagg))


def smoothed_prolongator(A, P_tent, omega, lam):
    A = cr.as_csr(A)
    d = A.diagonal()
    dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)
    return (P_tent - (omega / lam) * (sps.diags(dinv) @ A @ P_tent)).tocsr()
