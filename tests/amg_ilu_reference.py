"""Plain numpy / scipy restatement of the SA-AMG V cycle that smooths with block ILU(k) Richardson sweeps -- ML's
"smoother: type" = "IFPACK" with "smoother: ifpack type" = "ILU", isph_amg_params::smoother = 4 (host only, not a test
module).  Nothing here shares code with the device.

One smoothing step on level l is x += (L_B U_B)^-1 (b - A_l x); from a zero guess it is x = (L_B U_B)^-1 b.  L_B U_B is
the block-Jacobi ILU(fill) of A_l from ilu_shapes._ref_iluk (Ifpack's level rule, a symbolic pass, then the numeric IKJ
pass on the final pattern, in-block entries only, long double), on runs of `block` rows on level 0 and of COARSE_BLOCK
rows below.  `sweeps` steps run before and `sweeps` after the coarse correction.  The coarsest level is numpy.linalg.solve
-- or, when a null vector was given to the hierarchy (coarse_smoother), `sweeps` block-local symmetric Gauss-Seidel sweeps,
the rule of the Gauss-Seidel smoothers: the ILU of a small singular coarsest block is its complete LU.  A level with a row
that stores no diagonal entry is smoothed by the same Gauss-Seidel sweeps instead of the ILU.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

import ilu_shapes
import krylov_reference as kr

COARSE_BLOCK = 64   # kAmgCoarseBlock: rows the smoothers are local to on levels >= 1


def as_csr(A):
    A = sps.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    return A


def level_block(l, block):
    return block if l == 0 else COARSE_BLOCK


def every_row_keeps_its_diagonal(A):
    """every row of the CSR matrix stores its diagonal entry (whatever its value)"""
    A = as_csr(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return int(np.count_nonzero(A.indices == rows)) == A.shape[0]


class BlockILU:
    """(L_B U_B)^-1 r of one level: the factors of ilu_shapes._ref_iluk rounded to double once, two triangular solves per
    block"""

    def __init__(self, A, bs, fill):
        A = as_csr(A)
        self.bp = kr.block_ptr(A.shape[0], bs)
        dense = ilu_shapes._ref_iluk(A.indptr, A.indices, A.data, self.bp, int(fill))[3]
        self.factors = [np.asarray(W, dtype=np.float64) for W, _ in dense]

    def apply(self, r):
        z = np.zeros(len(r))
        for b, W in enumerate(self.factors):
            lo, hi = int(self.bp[b]), int(self.bp[b + 1])
            y = sla.solve_triangular(W, np.asarray(r[lo:hi], dtype=np.float64), lower=True, unit_diagonal=True)
            z[lo:hi] = sla.solve_triangular(W, y, lower=False)
        return z


class OracleILU:
    """the same operator through the oracle's restatement of block ILU(k)"""

    def __init__(self, A, bs, fill):
        import oracle as orc
        A = as_csr(A)
        self.F = orc.ILU(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, int(fill), kr.block_ptr(A.shape[0], bs))

    def apply(self, r):
        return self.F.apply(r)


class BlockSGS:
    """M_B^-1 r, M_B = blockdiag[(D + L_B) D^-1 (D + U_B)]: the symmetric Gauss-Seidel sweep local to the blocks; a zero
    pivot keeps its unknown at zero"""

    def __init__(self, A, bs):
        A = as_csr(A)
        bp = kr.block_ptr(A.shape[0], bs)
        self.bp, self.blocks = bp, [A[int(bp[b]):int(bp[b + 1]), int(bp[b]):int(bp[b + 1])].toarray() for b in range(len(bp) - 1)]

    def apply(self, r):
        z = np.zeros(len(r))
        for b, B in enumerate(self.blocks):
            lo, m = int(self.bp[b]), B.shape[0]
            d = B.diagonal()
            if np.all(d != 0.0):
                y = sla.solve_triangular(B, np.asarray(r[lo:lo + m], dtype=np.float64), lower=True) * d
                z[lo:lo + m] = sla.solve_triangular(B, y, lower=False)
                continue
            y = np.zeros(m)
            for i in range(m):
                s = r[lo + i] - np.dot(B[i, :i], y[:i])
                y[i] = s / d[i] if d[i] != 0.0 else 0.0
            y = y * d
            for i in range(m - 1, -1, -1):
                s = y[i] - np.dot(B[i, i + 1:], y[i + 1:])
                y[i] = s / d[i] if d[i] != 0.0 else 0.0
            z[lo:lo + m] = y
        return z


def build_smoothers(levels, fill, block=256, coarse_smoother=False, ilu_on_coarsest=False, factor=BlockILU):
    """one smoother per level (None on a coarsest level that is solved directly).  ilu_on_coarsest keeps the ILU on a
    coarsest level the smoother solves: what ML would do, and the negative control of the Gauss-Seidel rule."""
    out = []
    for l, (A, _) in enumerate(levels):
        last = l == len(levels) - 1
        bs = level_block(l, block)
        if last and not coarse_smoother:
            out.append(None)
        elif (last and not ilu_on_coarsest) or not every_row_keeps_its_diagonal(A):
            out.append(BlockSGS(A, bs))
        else:
            out.append(factor(A, bs, fill))
    return out


def _smooth(A, S, b, x, sweeps):
    """`sweeps` steps from x (None: the zero guess, whose first step needs no product)"""
    first = 0
    if x is None:
        x = S.apply(b)
        first = 1
    for _ in range(first, sweeps):
        x = x + S.apply(b - A @ x)
    return x


def amg_vcycle(levels, smoothers, b, sweeps=1, l=0):
    """one V cycle over levels = [(A_l, P_l)], R = P^T, with smoothers = build_smoothers(levels, ...)"""
    A, P = levels[l]
    S = smoothers[l]
    if l == len(levels) - 1:
        if S is None:
            return np.linalg.solve(A.toarray(), b)
        return _smooth(A, S, b, None, sweeps)
    x = _smooth(A, S, b, None, sweeps)
    e = amg_vcycle(levels, smoothers, P.T @ (b - A @ x), sweeps, l + 1)
    x = x + P @ e
    return _smooth(A, S, b, x, sweeps)


def amg_minv(levels, fill, sweeps=1, block=256, coarse_smoother=False, ilu_on_coarsest=False, factor=BlockILU):
    smoothers = build_smoothers(levels, fill, block, coarse_smoother, ilu_on_coarsest, factor)
    return lambda r: amg_vcycle(levels, smoothers, np.asarray(r, dtype=np.float64), sweeps)


def sgs_minv(levels, sweeps=1, block=256, coarse_smoother=False):
    """the cycle of smoother 0 over the same levels: the yardstick of the iteration counts"""
    smoothers = [None if (l == len(levels) - 1 and not coarse_smoother) else BlockSGS(A, level_block(l, block))
                 for l, (A, _) in enumerate(levels)]
    return lambda r: amg_vcycle(levels, smoothers, np.asarray(r, dtype=np.float64), sweeps)


# ---------------------------------------------------------------- systems the ILU smoother tests share
FIXTURES = ["stencil", "wall42", "spd", "tgv16", "lap96s"]


def system(name):
    """(rowptr, colidx, val, b, singular): the fixtures of chebyshev_reference.system plus
    lap96s  krylov_reference.laplace2d(96, 90, seed=21, shift=0.3) with rows scaled by default_rng(77).uniform(0.5, 2, n):
            8640 rows, nonsymmetric; its middle level has 19 blocks of 64 rows with a 62-row tail"""
    import chebyshev_reference as cr
    if name != "lap96s":
        return cr.system(name)
    A = kr.laplace2d(96, 90, seed=21, shift=0.3)
    n = A.shape[0]
    A = as_csr(sps.diags(np.random.default_rng(77).uniform(0.5, 2.0, n)) @ A)
    b = np.random.default_rng(31).standard_normal(n)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), b, False
