"""Host restatement of the cycle_bits = 32 V cycle of the Chebyshev-smoothed SA-AMG (host only, not a test module).
Nothing here shares code with the device; it is built on chebyshev_reference / chebyshev_f32_reference.

The arithmetic is the one include/isph_hip.h states for isph_amg_params::cycle_bits = 32:
  * the hierarchy [(A_l, P_l)] is the fp64 one;
  * every operator the cycle applies is a float plane: A~_l = fl32(A_l), P~_l = fl32(P_l), R~_l = P~_l^T and, with the
    shortcut, fl32(A_l P_l) of the fp64 product;
  * D^-1 is fl32(1 / a~_ii) (quotient in fp64); rho, the interval and the Chebyshev scalars come from A~_l (or from the
    lambda the caller passes for the level: the estimate on fl32(A_l));
  * every stored vector is float: each kernel widens, computes in fp64 and rounds ONCE per stored element.  A product of two
    floats is exact in fp64, so a row sum is an fp64 sum of exact products.  In a Chebyshev step wn is fp64, w = fl32(wn) and
    yout = fl32(y + wn) with the unrounded wn;
  * b_0 = fl32(r) on entry, the float result widened on exit; the dense coarsest solve is fp64 on the float b, rounded once;
  * the order: pre-smoother from a zero guess (product-free first step), r = fl32(b - A~ x), b_c = fl32(R~ r), recursion,
    x = fl32(x + P~ e), then with the shortcut r = fl32(r - fl32(A P) e) feeds the post-smoother's first step, otherwise that
    step forms b - A~ x itself.

Floats are carried as float64 arrays that hold float32 values (f32() rounds), so every sum below is an fp64 sum.
`order` permutes the summation order of every matrix-vector product (None: the CSR order; an integer seeds a shuffle of the
entries within each row): the restatement's own noise is the spread of its results under different orders.
"""
import numpy as np
import scipy.sparse as sps

import chebyshev_reference as cr
import chebyshev_f32_reference as c32


def f32(v):
    """round to the nearest float (ties to even, subnormals kept), carried as float64"""
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


class Plane:
    """a CSR operator whose product sums each row in a chosen order"""

    def __init__(self, A, order=None):
        A = cr.as_csr(A)
        self.shape = A.shape
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        cols, vals = A.indices.copy(), A.data.copy()
        if order is not None:
            key = rows + np.random.default_rng(order).random(len(rows)) * 0.999
            p = np.argsort(key, kind="stable")
            rows, cols, vals = rows[p], cols[p], vals[p]
        self.rows, self.cols, self.vals = rows, cols, vals

    def dot(self, x):
        # np.bincount adds the weights one after the other in the order given: a sequential fp64 sum per row
        return np.bincount(self.rows, weights=self.vals * np.asarray(x)[self.cols], minlength=self.shape[0])


def scalars(lam, ratio, degree):
    """(c1[k], c2[k]) of w = c1 w + c2 D^-1 (b - A y): the recurrence of chebyshev_reference.cheb_apply as two scalars a step"""
    _, _, theta, delta, sigma = cr.interval(lam, ratio)
    c1, c2 = [0.0], [1.0 / theta]
    rho_old = 1.0 / sigma
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho_old)
        c1.append(rho_new * rho_old)
        c2.append(2.0 * rho_new / delta)
        rho_old = rho_new
    return c1, c2


class Level:
    """the float planes and scalars of one level"""

    def __init__(self, A, P, degree, ratio, lam, order, shortcut, smoother):
        A32 = c32.fl32(A)
        self.n = A.shape[0]
        self.A = Plane(A32, order)
        self.A64 = cr.as_csr(A)
        if smoother:
            d = A32.diagonal()
            assert abs(A32[d == 0.0]).sum() == 0.0          # a zero diagonal only on a row without entries: left alone
            with np.errstate(divide="ignore"):
                self.dinv = f32(np.where(d != 0.0, 1.0 / d, 0.0))
            if lam is None:
                s = np.asarray(abs(A32).sum(axis=1)).ravel()
                q = s[d != 0.0] / np.abs(d[d != 0.0])
                lam = float(q.max()) if len(q) else 1.0
            self.c1, self.c2 = scalars(float(lam), ratio, degree)
        self.P = self.R = self.AP = None
        if P is not None:
            P32 = c32.fl32(P)
            self.P = Plane(P32, order)
            self.R = Plane(P32.T.tocsr(), order)
            if shortcut:
                self.AP = Plane(c32.fl32(cr.as_csr(A) @ cr.as_csr(P)), order)

    def smooth(self, b, y, r0=None):
        """the polynomial on float vectors; y None: the zero guess; r0: b - A~ y is already there"""
        k0 = 0
        if y is None or r0 is not None:
            wn = self.c2[0] * (self.dinv * (b if y is None else r0))
            w = f32(wn)
            y = f32(wn) if y is None else f32(y + wn)
            k0 = 1
        else:
            w = np.zeros(self.n)
        for k in range(k0, len(self.c1)):
            r = b - self.A.dot(y)
            wn = self.c1[k] * w + self.c2[k] * (self.dinv * r)
            w = f32(wn)
            y = f32(y + wn)
        return y


def _rounded(L, l, b, coarse_polynomial):
    lev = L[l]
    if l == len(L) - 1:
        if coarse_polynomial:
            return lev.smooth(b, None)
        return f32(np.linalg.solve(lev.A64.toarray(), b))
    x = lev.smooth(b, None)
    r = f32(b - lev.A.dot(x))
    e = _rounded(L, l + 1, f32(lev.R.dot(r)), coarse_polynomial)
    x = f32(x + lev.P.dot(e))
    if lev.AP is not None:
        r = f32(r - lev.AP.dot(e))
        return lev.smooth(b, x, r0=r)
    return lev.smooth(b, x)


def cycle(levels, b, sweeps=1, ratio=20.0, lams=None, coarse_polynomial=False, shortcut=True, rounded=True, order=None):
    """one V cycle over levels = [(A_l, P_l or None)] applied to the fp64 vector b.
    lams: one lambda per level in place of rho of the level (None: rho); for rounded=True the estimate on fl32(A_l).
    rounded=False calls through to the fp64 cycle (chebyshev_reference.amg_vcycle, or its lambda form)."""
    if not rounded:
        if lams is None:
            return cr.amg_vcycle(levels, b, sweeps, ratio, coarse_polynomial)
        import eig_estimate_reference as er
        return er.amg_vcycle(levels, lams, b, sweeps, ratio, coarse_polynomial)
    last = len(levels) - 1
    L = [Level(A, P, sweeps, ratio, None if lams is None else lams[l], order, shortcut, l < last or coarse_polynomial)
         for l, (A, P) in enumerate(levels)]
    return _rounded(L, 0, f32(b), coarse_polynomial)


def minv(levels, **kw):
    return lambda r: cycle(levels, r, **kw)


# ---------------------------------------------------------------- a numpy hierarchy for the host tests
def lattice_hierarchy(A, nx, ny, nz=1, omega=2.0 / 3.0, coarse_max=64):
    """[(A_l, P_l)] for a matrix on an nx x ny (x nz) lattice (row = (k * ny + j) * nx + i): aggregates of 3 x 3 cells of
    every lattice plane, tentative prolongator of normalised ones, smoothed by one damped-Jacobi step
    P = (I - omega D^-1 A) P_t, A_c = P^T A P"""
    levels = []
    A = cr.as_csr(A)
    assert nx * ny * nz == A.shape[0]
    while A.shape[0] > coarse_max and min(nx, ny) >= 3:
        n = nx * ny * nz
        cx, cy = (nx + 2) // 3, (ny + 2) // 3
        k, rem = np.divmod(np.arange(n), nx * ny)
        j, i = np.divmod(rem, nx)
        agg = (k * cy + j // 3) * cx + (i // 3)
        cnt = np.bincount(agg, minlength=cx * cy * nz)
        Pt = sps.csr_matrix((1.0 / np.sqrt(cnt[agg]), (np.arange(n), agg)), shape=(n, cx * cy * nz))
        Dinv = sps.diags(1.0 / A.diagonal())
        P = cr.as_csr(Pt - omega * (Dinv @ A @ Pt))
        levels.append((A, P))
        A = cr.as_csr(P.T @ A @ P)
        nx, ny = cx, cy
    levels.append((A, None))
    return levels
