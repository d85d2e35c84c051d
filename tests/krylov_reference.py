"""Plain float64 reference for the iterates of restarted GMRES(m) and of PCG (host only, not a test module).

isph_solve with tol = 0 and max_iters = k returns the k-th iterate of the method from the given x0.  That vector is
defined independently of how a solver computes it, so every correct orthogonalisation (DGKS, ICGS, IMGS), flexible or
not, must return it to round-off, and its recurrence residual must equal the true residual of that vector.

Nothing here shares code with the device or with the oracle's Krylov code: the Krylov basis is built with two full
classical Gram-Schmidt passes in float64 and the small least-squares (GMRES) or Galerkin (CG) problem is solved densely
-- no Givens recurrence, no short recurrences.  The singular form is the one isph_solve documents (include/isph_hip.h):
b <- b - (b.n) n, operator P A with P = I - n n^T, and x <- x - (x.n) n at the end.
"""
import numpy as np
import scipy.sparse as sps

DGKS_TOL = 1.0 / np.sqrt(2.0)   # Belos DGKS dep_tol: a second pass when |w_new| < dep_tol |w_old|


def as_csr(A):
    A = sps.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    return A


def unit_null(mask_or_vec, n):
    """n = mask / ||mask|| (SolverLin::createNullVector); None -> the vector of ones"""
    v = np.ones(n) if mask_or_vec is None else np.asarray(mask_or_vec, dtype=np.float64)
    return v / np.linalg.norm(v)


def jacobi_minv(A):
    """point Jacobi: 1/diag, and 1 where the diagonal is 0"""
    d = as_csr(A).diagonal()
    inv = np.ones_like(d)
    nz = d != 0.0
    inv[nz] = 1.0 / d[nz]
    return lambda r: inv * r


def ilu0_minv(rowptr, colidx, val, block_ptr):
    """block-Jacobi ILU(0) through the oracle's restatement (pinned elsewhere against the device factor)"""
    import oracle as orc
    F = orc.ILU(rowptr, colidx, val, 0, block_ptr)
    return lambda r, F=F: F.apply(r)


def _proj(v, null):
    return v if null is None else v - np.dot(v, null) * null


def _matvec_ld(A, x):
    """A x with np.longdouble products and row sums"""
    prod = A.data.astype(np.longdouble) * np.asarray(x, dtype=np.longdouble)[A.indices]
    prod = np.append(prod, np.longdouble(0.0))
    starts = A.indptr[:-1]
    y = np.add.reduceat(prod, starts)
    y[A.indptr[1:] == starts] = 0.0
    return y


def true_residual_norm(A, b, x, null=None):
    """||P (b - A x)|| with longdouble accumulation (b already projected by the caller when null is given)"""
    r = np.asarray(b, dtype=np.longdouble) - _matvec_ld(A, x)
    if null is not None:
        nl = np.asarray(null, dtype=np.longdouble)
        r = r - np.sum(r * nl) * nl
    return float(np.sqrt(np.sum(r * r)))


def _cgs2(V, w):
    """two classical Gram-Schmidt passes of w against the rows of V; returns (w, h, first-pass norm ratio)"""
    old = np.linalg.norm(w)
    h = V @ w
    w = w - V.T @ h
    ratio = np.linalg.norm(w) / old if old > 0 else 0.0
    h2 = V @ w
    w = w - V.T @ h2
    return w, h + h2, ratio


class Iterate:
    """x: the iterate (projected when singular); rel_res: ||P(b - A x_k)|| / ||P(b - A x0)|| (before the final
    projection, which is what the recurrence residual measures); ratios: per step, |w| after / before the first
    Gram-Schmidt pass (GMRES only), from which the DGKS decision follows"""

    def __init__(self, x, rel_res, ratios=()):
        self.x, self.rel_res, self.ratios = x, rel_res, np.asarray(ratios)

    def dgks_second_passes(self):
        return int(np.sum(self.ratios < DGKS_TOL))

    def dgks_margin(self):
        """smallest relative distance of a first-pass ratio to the DGKS threshold"""
        return float(np.min(np.abs(self.ratios / DGKS_TOL - 1.0))) if len(self.ratios) else np.inf


def gmres_iterates(A, b, x0, ks, m, Minv=None, null=None, perturb=None):
    """{k: Iterate} of restarted GMRES(m) with right preconditioning by a fixed linear Minv, for every k in ks
    (iterations in total, restarts included).  null: unit null vector (the singular form).
    perturb = (i, j, rel): multiply entry (i, j) of every cycle's Hessenberg matrix by (1 + rel) before the
    least-squares solve (negative control only)."""
    A = as_csr(A)
    N = A.shape[0]
    Minv = Minv or (lambda r: r.copy())
    b = _proj(np.asarray(b, dtype=np.float64), null)
    x = np.array(x0, dtype=np.float64)

    def op(v):
        return _proj(A @ v, null)

    scale = true_residual_norm(A, b, x, null)
    scale = scale if scale > 0 else 1.0
    ks = sorted(set(int(k) for k in ks))
    out, ratios, it = {}, [], 0

    def record(k, xk):
        out[k] = Iterate(_proj(xk, null), true_residual_norm(A, b, xk, null) / scale, list(ratios))

    while it < ks[-1]:
        r = b - op(x)
        beta = np.linalg.norm(r)
        if beta == 0.0:
            break
        L = min(m, ks[-1] - it)
        V = np.zeros((L + 1, N))
        Z = np.zeros((L, N))
        H = np.zeros((L + 1, L))
        V[0] = r / beta

        def lsq(j):  # y of min || beta e1 - H[:j+1, :j] y ||
            Hj = H[:j + 1, :j].copy()
            if perturb is not None and perturb[0] < j + 1 and perturb[1] < j:
                Hj[perturb[0], perturb[1]] *= 1.0 + perturb[2]
            e = np.zeros(j + 1)
            e[0] = beta
            return np.linalg.lstsq(Hj, e, rcond=None)[0]

        for j in range(L):
            Z[j] = Minv(V[j])
            w, h, ratio = _cgs2(V[:j + 1], op(Z[j]))
            ratios.append(ratio)
            H[:j + 1, j] = h
            H[j + 1, j] = np.linalg.norm(w)
            if H[j + 1, j] > 0.0:
                V[j + 1] = w / H[j + 1, j]
            it += 1
            if it in ks and j + 1 < L:
                record(it, x + Z[:j + 1].T @ lsq(j + 1))
        x = x + Z.T @ lsq(L)
        if it in ks:
            record(it, x)
    for k in ks:  # a zero residual ends the method: the later iterates are the last one
        if k not in out:
            record(k, x)
    return out


def gmres_iterate(A, b, x0, k, m, Minv=None, null=None):
    """(x_k, true_rel_res) of restarted GMRES(m) after k iterations in total"""
    it = gmres_iterates(A, b, x0, [k], m, Minv, null)[k]
    return it.x, it.rel_res


def pcg_iterates(A, b, x0, ks, Minv=None, null=None):
    """{k: Iterate} of preconditioned CG: the minimiser of the A-norm of the error over x0 + K_k(M^-1 A, M^-1 r0),
    i.e. the x in that space whose residual is orthogonal to it (Galerkin), solved densely on an orthonormal basis"""
    A = as_csr(A)
    N = A.shape[0]
    Minv = Minv or (lambda r: r.copy())
    b = _proj(np.asarray(b, dtype=np.float64), null)
    x0 = np.array(x0, dtype=np.float64)

    def op(v):
        return _proj(A @ v, null)

    scale = true_residual_norm(A, b, x0, null)
    scale = scale if scale > 0 else 1.0
    ks = sorted(set(int(k) for k in ks))
    r0 = b - op(x0)
    z = Minv(r0)
    Q = np.zeros((ks[-1], N))
    AQ = np.zeros((ks[-1], N))
    Q[0] = z / np.linalg.norm(z)
    out = {}
    for j in range(ks[-1]):
        AQ[j] = op(Q[j])
        if j + 1 in ks:
            G = Q[:j + 1] @ AQ[:j + 1].T
            y = np.linalg.solve(G, Q[:j + 1] @ r0)
            xk = x0 + Q[:j + 1].T @ y
            out[j + 1] = Iterate(_proj(xk, null), true_residual_norm(A, b, xk, null) / scale)
        if j + 1 < ks[-1]:
            w, _, _ = _cgs2(Q[:j + 1], Minv(AQ[j]))
            Q[j + 1] = w / np.linalg.norm(w)
    return out


def pcg_iterate(A, b, x0, k, Minv=None, null=None):
    it = pcg_iterates(A, b, x0, [k], Minv, null)[k]
    return it.x, it.rel_res


def iterate_gap(x, x_ref):
    """||x - x_ref|| / ||x_ref||"""
    x = np.asarray(x, dtype=np.float64)
    return float(np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref))


def residual_gap(rel_res_implicit, ref):
    """|rel_res_implicit - true_rel_res| (both relative to ||r0||)"""
    return abs(float(rel_res_implicit) - ref.rel_res)


# ---------------------------------------------------------------- systems the Krylov iterate tests share
SHIFT = 0.03   # the non-singular variant: with + I the residual falls below 1e-10 by k = 31 and x_k becomes round-off


def tgv_rows(shift=None):
    """(rowptr, colidx, val) of the 2-D TGV pressure rows, JITTER, 33 x 33 = 1089 rows (odd); shift: + shift * I"""
    from isph_amd import workload
    from problems import Problem, tgv_spec
    pr = Problem(tgv_spec(dim=2, n=33, mode=workload.JITTER))
    rp, ci, val, _ = pr.poisson()
    if shift is None:
        return rp, ci, val
    val = val.copy()
    for i in range(pr.n):
        val[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i] += shift
    return rp, ci, val


def block_ptr(n, bs):
    return np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)


def minv_for(prec, rp, ci, val, bs=256):
    """the reference's M^-1 for the preconditioner names of isph_prec_create"""
    n = len(rp) - 1
    if prec == "none":
        return None
    if prec == "jacobi":
        return jacobi_minv(sps.csr_matrix((val, ci, rp), shape=(n, n)))
    assert prec == "bjacobi-ilu0"
    return ilu0_minv(rp, ci, val, block_ptr(n, bs))


def oracle_solve(rp, ci, val, b, x0, k, m, ortho=0, flexible=1, singular=False, prec="none", null_mask=None,
                 solver_type=0, bs=256):
    """the oracle's x_k (tol = 0, max_iters = k) and its SolveInfo"""
    import oracle as orc
    n = len(rp) - 1
    prm = orc.SolverParams(solver_type=solver_type, num_blocks=m, max_iters=k, max_restarts=10 ** 6, tol=0.0, ortho=ortho,
                           flexible=flexible)
    name = {"none": "none", "jacobi": "jacobi", "bjacobi-ilu0": "ilu"}[prec]
    ilu = orc.ILU(rp, ci, val, 0, block_ptr(n, bs)) if prec == "bjacobi-ilu0" else None
    x, info, _ = orc.solve(rp, ci, val, b, x0=x0, singular=singular, null_mask=null_mask, prec=name, ilu=ilu, params=prm)
    return x, info


def stencil3d(nx, ny, nz, conv=(0.4, -0.25, 0.15), shift=0.0):
    """periodic 3-D convection-diffusion, 7-point, central differences: nonsymmetric; every row sums to `shift`"""
    N = nx * ny * nz
    idx = np.arange(N).reshape(nz, ny, nx)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(N, 6.0 + shift)]
    for axis, c in zip((2, 1, 0), conv):
        for s, sign in ((1, 1.0), (-1, -1.0)):
            rows.append(idx.ravel())
            cols.append(np.roll(idx, -s, axis=axis).ravel())
            vals.append(np.full(N, -1.0 + sign * c))
    A = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    A.sort_indices()
    return A


def laplace2d(nx, ny, seed, shift=None):
    """variable-coefficient 5-point Laplacian with Neumann walls (symmetric, every row sums to 0, null vector = ones);
    shift: + diag(shift * U(0.5, 1.5)), symmetric positive definite"""
    rng = np.random.default_rng(seed)
    N = nx * ny
    idx = np.arange(N).reshape(ny, nx)
    ea, eb = idx[:, :-1].ravel(), idx[:, 1:].ravel()
    na, nb = idx[:-1, :].ravel(), idx[1:, :].ravel()
    a, c = np.concatenate([ea, na]), np.concatenate([eb, nb])
    w = rng.uniform(0.5, 2.0, len(a))
    d = np.bincount(a, w, N) + np.bincount(c, w, N)
    if shift is not None:
        d = d + shift * rng.uniform(0.5, 1.5, N)
    A = sps.csr_matrix((np.concatenate([-w, -w, d]), (np.concatenate([a, c, np.arange(N)]),
                                                      np.concatenate([c, a, np.arange(N)]))), shape=(N, N))
    A.sort_indices()
    return A


def tiny(n):
    """non-singular, nonsymmetric n x n: 1-D convection-diffusion plus a few seeded far entries"""
    A = sps.diags([np.full(n - 1, -1.3), np.full(n, 2.05), np.full(n - 1, -0.7)], [-1, 0, 1], shape=(n, n), format="lil")
    rng = np.random.default_rng(100 + n)
    for _ in range(n // 8):
        i, j = rng.integers(0, n, 2)
        if i != j:
            A[i, j] += 0.1 * rng.standard_normal()
    return as_csr(A)
