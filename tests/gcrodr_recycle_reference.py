"""GCRO-DR(m, k) with the recycle space carried from one solve to the next -- TEST INFRASTRUCTURE, numpy.

oracle/gcrodr.py restates the cycle of csrc/gcrodr.hpp; this module is that cycle plus the three additions of the carried
space (notation of oracle/gcrodr.py: Op = P_n A M^-1, the space lives in the preconditioned variable t):

  entry with U0 (n x kk)   Cn = Op U0 (kk applications); Cholesky-QR twice: G = Cn^T Cn = R^T R, C <- Cn R^-1,
                           U <- U0 R^-1, and once more.  The space is dropped (the solve is then the fresh one) when a
                           Cholesky pivot is not a positive finite number or when the second Gram matrix has
                           kk max|G2 - I| > 1/2.  Then c = C^T r0, t = U c, r = r0 - C c; the convergence scale stays
                           |r0|; |r| / |r0| <= tol is convergence with 0 iterations; otherwise the kk > 0 cycles follow.
  exit (keep)              the recycle step also runs after the last cycle, converged or not; a first cycle that ended
                           with j <= k steps keeps nothing; a solve that converged at the projection keeps U R^-1.
  same operator (C0)       U0 and C0 = Op U0 of the previous right-hand side's exit carry over: no applications, no QR.

solve(..., U0=None, keep=False) is oracle/gcrodr.py::solve.
"""
import numpy as np
import scipy.linalg as sla

import oracle as orc
from gcrodr import _real_basis

GUARD = 0.5


def cholqr2(U, C):
    """Cholesky-QR twice on C, the same triangular factors applied to U.  Returns (U, C) or None (guard)."""
    kk = C.shape[1]
    for it in range(2):
        G = C.T @ C
        if it == 1 and kk * np.abs(G - np.eye(kk)).max() > GUARD:
            return None
        if not np.all(np.isfinite(G)):
            return None
        R = np.zeros((kk, kk))                              # G = R^T R, R upper triangular
        for i in range(kk):
            d = G[i, i] - R[:i, i] @ R[:i, i]
            if not (np.isfinite(d) and d > 0.0):
                return None
            R[i, i] = np.sqrt(d)
            R[i, i + 1:] = (G[i, i + 1:] - R[:i, i] @ R[:i, i + 1:]) / R[i, i]
        Rinv = sla.solve_triangular(R, np.eye(kk))
        C = C @ Rinv
        U = U @ Rinv
    return U, C


def solve(rowptr, colidx, val, b, x0=None, singular=False, null_mask=None, prec=None, num_blocks=50, num_recycled=20,
          tol=1e-8, max_iters=500, max_restarts=15, U0=None, keep=True, C0=None):
    """prec: callable r -> M^-1 r (or None).  Returns (x, info, U): info as oracle/gcrodr.py plus applications (operator
    applications that rebuilt C), started (the carried space was used), discarded (reason, 0 none / 2 guard / 3 too many
    vectors for this k) and C (Op U of the kept space, for the next right-hand side of the same operator); U is the space
    to carry on (None: nothing kept)."""
    n = len(rowptr) - 1
    m, k = int(num_blocks), int(num_recycled)
    assert 0 < k < m
    b = np.array(b, dtype=np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    nvec = None
    if singular:
        nvec = np.ones(n) if null_mask is None else np.asarray(null_mask, dtype=np.float64).copy()
        nvec /= np.linalg.norm(nvec)
        b -= (b @ nvec) * nvec
    Minv = (lambda r: r) if prec is None else prec

    def A(v):
        y = orc.spmv(rowptr, colidx, val, v)
        return y - (y @ nvec) * nvec if singular else y

    def op(v):
        return A(Minv(v))

    r = b - A(x)
    beta0 = np.linalg.norm(r)
    scale = beta0 if beta0 > 0 else 1.0
    info = dict(converged=beta0 / scale <= tol, iters=0, restarts=0, rel_res=beta0 / scale, applications=0, started=False,
                discarded=0, C=None)
    t = np.zeros(n)
    U = C = None

    # ---- entry with a carried space
    if U0 is not None and U0.shape[1] > 0:
        kk = U0.shape[1]
        if kk > k + 1:
            info["discarded"] = 3
        elif C0 is not None:
            U, C = np.array(U0), np.array(C0)
            info["started"] = True
        else:
            Cn = np.stack([op(U0[:, i]) for i in range(kk)], axis=1)
            info["applications"] = kk
            uc = cholqr2(np.array(U0), Cn)
            if uc is None:
                info["discarded"] = 2
            else:
                U, C = uc
                info["started"] = True
        if U is not None and not info["converged"]:
            c = C.T @ r
            t = t + U @ c
            r = r - C @ c
            info["rel_res"] = np.linalg.norm(r) / scale
            if info["rel_res"] <= tol:
                info["converged"] = True

    def arnoldi(r, steps, C):
        """returns V (n x (j+1)), Hbar ((j+1) x j), B (k x j), j, converged"""
        beta = np.linalg.norm(r)
        V = np.zeros((n, steps + 1))
        H = np.zeros((steps + 1, steps))
        B = np.zeros((0 if C is None else C.shape[1], steps))
        V[:, 0] = r / beta
        j = 0
        conv = False
        while j < steps:
            w = op(V[:, j])
            if C is not None:
                B[:, j] = C.T @ w
                w = w - C @ B[:, j]
            for _ in range(2):                                 # two classical Gram-Schmidt passes
                c = V[:, :j + 1].T @ w
                w = w - V[:, :j + 1] @ c
                H[:j + 1, j] += c
            H[j + 1, j] = np.linalg.norm(w)
            V[:, j + 1] = w / H[j + 1, j]
            j += 1
            info["iters"] += 1
            e1 = np.zeros(j + 1)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(H[:j + 1, :j], e1, rcond=None)
            info["rel_res"] = np.linalg.norm(e1 - H[:j + 1, :j] @ y) / scale
            if info["rel_res"] <= tol:
                conv = True
                break
            if info["iters"] >= max_iters:
                break
        return V[:, :j + 1], H[:j + 1, :j], B[:, :j], j, conv, beta

    while not info["converged"] and info["iters"] < max_iters:
        if U is None:
            V, H, _, j, conv, beta = arnoldi(r, m, None)
            e1 = np.zeros(j + 1)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(H, e1, rcond=None)
            t += V[:, :j] @ y
            r = V @ (e1 - H @ y)
            more = not conv and info["iters"] < max_iters and info["restarts"] < max_restarts
            if conv:
                info["converged"] = True
            if not more and (not keep or j <= k):
                break
            Hm = H[:j, :j]
            em = np.zeros(j)
            em[-1] = 1.0
            f = np.linalg.solve(Hm.T, em)
            theta, Z = np.linalg.eig(Hm + H[j, j - 1] ** 2 * np.outer(f, em))
            P = _real_basis(theta, Z, k)
            Q, R = np.linalg.qr(H @ P)
            C = V @ Q
            U = np.linalg.solve(R.T, (V[:, :j] @ P).T).T
        else:
            kk = U.shape[1]
            V, H, B, j, conv, beta = arnoldi(r, m - kk, C)
            d = 1.0 / np.linalg.norm(U, axis=0)
            Ut = U * d
            G = np.zeros((kk + j + 1, kk + j))
            G[:kk, :kk] = np.diag(d)
            G[:kk, kk:] = B
            G[kk:, kk:] = H
            W = np.concatenate([C, V], axis=1)
            Vh = np.concatenate([Ut, V[:, :j]], axis=1)
            rhs = np.concatenate([C.T @ r, np.eye(j + 1)[:, 0] * beta])
            y, *_ = np.linalg.lstsq(G, rhs, rcond=None)
            t += Vh @ y
            r = r - W @ (G @ y)
            more = not conv and info["iters"] < max_iters and info["restarts"] < max_restarts
            if conv:
                info["converged"] = True
            if not more and not keep:
                break
            WtV = np.zeros((kk + j + 1, kk + j))
            WtV[:kk, :kk] = C.T @ Ut
            WtV[kk:, :kk] = V.T @ Ut
            WtV[kk:kk + j, kk:] = np.eye(j)
            theta, Z = sla.eig(G.T @ G, G.T @ WtV)
            P = _real_basis(theta, Z, k)
            Q, R = np.linalg.qr(G @ P)
            C = W @ Q
            U = np.linalg.solve(R.T, (Vh @ P).T).T
        if not more:
            break
        info["restarts"] += 1
    x = x + Minv(t)
    if singular:
        x -= (x @ nvec) * nvec
    if not keep:
        info.pop("C")
        return x, info, None
    info["C"] = C
    return x, info, U


# ---- the sequences of slowly changing systems the tests (CPU and GPU) run ------------------------------------------------
def jacobi(rp, ci, val):
    n = len(rp) - 1
    d = np.array([val[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i][0] for i in range(n)])
    return lambda r: r / d


def ilu0_blocks(rp, ci, val, bs=256):
    n = len(rp) - 1
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    return orc.ILU(rp, ci, val, 0, bp).apply


PRECS = {"none": lambda rp, ci, val: None, "jacobi": jacobi, "bjacobi-ilu0": ilu0_blocks}

# name -> (dim, n, prec, m, k): Poisson systems of tgv_spec in ADVECT mode with advect_dt = spec.dt (1 + 0.1 s), s = 0..3
SEQUENCES = {"A": (2, 64, "jacobi", 30, 10), "B": (2, 48, "jacobi", 20, 6), "C": (3, 20, "bjacobi-ilu0", 50, 6),
             "E": (3, 16, "none", 50, 4)}
# the same 3-D n = 16 JITTER system solved twice
PAIRS_D = [(10, 4, "none"), (20, 5, "bjacobi-ilu0"), (12, 6, "jacobi"), (50, 20, "none")]


def sequence_systems(name, steps=4, coords=False):
    """[(rowptr, colidx, val, b)] of sequence `name`; coords: [(rowptr, colidx, val, b, x [n, 3])]"""
    from isph_amd import workload
    from problems import Problem, tgv_spec
    dim, n = SEQUENCES[name][:2]
    base = tgv_spec(dim=dim, n=n, mode=workload.ADVECT)
    out = []
    for s in range(steps):
        pr = Problem(tgv_spec(dim=dim, n=n, mode=workload.ADVECT, advect_dt=base.dt * (1.0 + 0.1 * s)))
        sysm = pr.poisson()
        out.append(tuple(sysm) + (np.ascontiguousarray(pr.parts["x"][:pr.n]),) if coords else sysm)
    return out


def helmholtz_like(rp, ci, val):
    """values of I + A (non-singular: the Poisson matrices here have a positive diagonal and rows that sum to zero)"""
    v = np.array(val, dtype=np.float64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    v[rows == ci] += 1.0
    return v


def run_sequence(systems, prec, m, k, carry, tol=1e-8):
    """solves the systems in turn (singular, null-space projection); carry: hand U from one solve to the next.
    Returns [(x, info)]."""
    U = None
    res = []
    for rp, ci, val, b in systems:
        x, info, Un = solve(rp, ci, val, b, singular=True, prec=PRECS[prec](rp, ci, val), num_blocks=m, num_recycled=k,
                            tol=tol, U0=U if carry else None, keep=True)
        info["kk_in"] = 0 if (U is None or not carry) else U.shape[1]
        U = Un
        res.append((x, info))
    return res
