"""Expected values of the value_bits = 32 mode of the Chebyshev polynomial (host only, not a test module).

The mode is defined in one sentence (include/isph_hip.h, isph_cheb_params): the fp64 recurrence of
tests/chebyshev_reference.py applied to A~ = fl32(A) in place of A.  So everything here is chebyshev_reference on a
matrix whose values went through float32 once; nothing shares code with the device.
"""
import numpy as np
import scipy.sparse as sps

import chebyshev_reference as cr


def fl32(A):
    """A~: every stored value rounded to the nearest float (ties to even, subnormals kept), pattern unchanged -- an
    entry that rounds to 0 stays in the pattern, as it stays in the device's value plane"""
    A = cr.as_csr(A)
    return sps.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def gap_max(z, ref):
    return float(np.max(np.abs(np.asarray(z) - ref)) / np.max(np.abs(ref)))


def _level_smooth(A_s, b, y0, degree, ratio):
    """chebyshev_reference._level_smooth for a level operator A_s (already rounded or not): rows without entries are
    left alone"""
    return cr._level_smooth(A_s, b, y0, degree, ratio)


def amg_vcycle(levels, b, sweeps=1, ratio=20.0, coarse_polynomial=False, single=True, l=0):
    """chebyshev_reference.amg_vcycle with the smoother of every level acting on fl32(A_l) (single = True) while the
    residual, the restriction, the prolongation and the dense coarse solve use A_l itself.  single = False is the fp64
    cycle, restated here so that both come from the same lines."""
    A, P = levels[l]
    A_s = fl32(A) if single else cr.as_csr(A)
    if l == len(levels) - 1:
        if coarse_polynomial:
            return _level_smooth(A_s, b, None, sweeps, ratio)
        return np.linalg.solve(A.toarray(), b)
    x = _level_smooth(A_s, b, None, sweeps, ratio)
    e = amg_vcycle(levels, P.T @ (b - A @ x), sweeps, ratio, coarse_polynomial, single, l + 1)
    x = x + P @ e
    return _level_smooth(A_s, b, x, sweeps, ratio)
