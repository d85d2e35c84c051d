"""Plain numpy restatement of the GMRES-polynomial preconditioner "gmres-poly<d>" (csrc/gmres_poly.hpp; host only, not a
test module).  Nothing here shares code with the device.

    B = D^-1 A,  v_0 = u / |u| with u the Philox start vector of eig_estimate_reference (level 0, the caller's global
    row); with a unit null vector n, u and every product are projected: w <- w - (w.n) n
    d Arnoldi steps, classical Gram-Schmidt twice  ->  H, (d + 1) x d;  a breakdown h_{j+1,j} <= 1e-14 |h_00| gives degree j
    H^ = H_d + h_{d+1,d}^2 f e_d^T,  H_d^T f = e_d;  the roots theta are the eigenvalues of H^ (harmonic Ritz values);
    |Im theta| <= 1e-8 |theta| counts as real
    modified Leja order: largest modulus first, then always the root with the largest product of distances to the chosen
    ones, a conjugate directly behind its partner
    z = p(B) D^-1 r in product form:  r <- D^-1 r, z = 0;
        real theta:   z += r / theta,                       r <- r - (B r) / theta
        pair a +- ib: t = 2a r - B r, z += t / (a^2 + b^2), r <- r - (B t) / (a^2 + b^2)
    and no product behind the last root.

apply() runs in the dtype it is given (numpy.float64, numpy.longdouble), so that the rounding of the restatement itself
can be measured on the inputs of a test.
"""
import numpy as np

import chebyshev_reference as cr
import eig_estimate_reference as er

MAX_DEGREE = 25
REAL_TOL = 1e-8
ZERO_TOL = 1e-10
BREAKDOWN = 1e-14


class NearZeroRoot(ValueError):
    pass


def dinv_of(A):
    d = cr.as_csr(A).diagonal()
    assert np.all(d != 0.0)
    return 1.0 / d


def _proj(w, null):
    return w if null is None else w - np.dot(w, null) * null


def arnoldi(A, d, null=None, offset=0, rows=None, start=None, mode="plain"):
    """(H, m, breakdown, v0): H is (m + 1) x m.  start: another start vector than the Philox one (tests of the restatement).
    mode: how every dot and norm is accumulated (eig_estimate_reference._dot: "plain", "reversed", "longdouble")"""
    dot = lambda a, b: er._dot(a, b, mode)
    A = cr.as_csr(A)
    n = A.shape[0]
    dinv = dinv_of(A)
    if null is not None:
        null = np.asarray(null, dtype=np.float64)
        null = null / np.sqrt(dot(null, null))
    proj = (lambda w: w) if null is None else (lambda w: w - dot(w, null) * null)
    d = min(int(d), n)
    u = er.start_vector(n, 0, offset, rows) if start is None else np.array(start, dtype=np.float64)
    u = proj(u)
    V = np.zeros((d + 1, n))
    V[0] = u / np.sqrt(dot(u, u))
    H = np.zeros((d + 1, d))
    m, breakdown = 0, False
    for j in range(d):
        w = proj(dinv * (A @ V[j]))
        c = np.zeros(j + 1)
        for _ in range(2):
            ci = np.array([dot(V[i], w) for i in range(j + 1)])
            w = w - ci @ V[:j + 1]
            c += ci
        H[:j + 1, j] = c
        hn = np.sqrt(dot(w, w))
        H[j + 1, j] = hn
        m = j + 1
        if hn <= BREAKDOWN * abs(H[0, 0]):
            breakdown = True
            break
        if j + 1 < d:
            V[j + 1] = w / hn
    return H[:m + 1, :m].copy(), m, breakdown, V[0].copy()


def harmonic_matrix(H, breakdown=False):
    """H^ of the (m + 1) x m Hessenberg matrix H"""
    m = H.shape[1]
    Hd = np.array(H[:m, :m], dtype=np.float64)
    h = 0.0 if breakdown else H[m, m - 1]
    if h != 0.0:
        e = np.zeros(m)
        e[m - 1] = 1.0
        f = np.linalg.solve(Hd.T, e)
        Hd[:, m - 1] += h * h * f
    return Hd


def pair_roots(lam):
    """[(a, b)]: b == 0 a real root, b > 0 the pair a +- ib"""
    lam = np.asarray(lam, dtype=np.complex128)
    out, used = [], np.zeros(len(lam), dtype=bool)
    for i, l in enumerate(lam):
        if abs(l.imag) <= REAL_TOL * abs(l):
            out.append((l.real, 0.0))
            used[i] = True
    for i, l in enumerate(lam):
        if used[i] or l.imag < 0.0:
            continue
        used[i] = True
        cand = [j for j in range(len(lam)) if not used[j] and lam[j].imag < 0.0]
        if not cand:
            out.append((l.real, 0.0))
            continue
        j = min(cand, key=lambda q: abs(lam[q] - np.conj(l)))
        used[j] = True
        out.append((0.5 * (l.real + lam[j].real), 0.5 * (l.imag - lam[j].imag)))
    for i, l in enumerate(lam):
        if not used[i]:
            out.append((l.real, 0.0))
    return out


def leja_order(units):
    """modified Leja order of [(a, b)]; ties go to the earlier entry"""
    units = list(units)
    m = len(units)
    used, score, out = [False] * m, [0.0] * m, []
    for k in range(m):
        best, sb = None, -np.inf
        for i in range(m):
            if used[i]:
                continue
            s = np.hypot(*units[i]) if k == 0 else score[i]
            if best is None or s > sb:
                best, sb = i, s
        used[best] = True
        out.append(units[best])
        c = complex(*units[best])
        for i in range(m):
            if used[i]:
                continue
            t = complex(*units[i])
            with np.errstate(divide="ignore"):
                score[i] += np.log(abs(t - c))
                if units[best][1] > 0.0:
                    score[i] += np.log(abs(t - np.conj(c)))
    return out


def expand(units):
    """[(a, b)] -> the complex roots in application order, a + ib directly followed by a - ib"""
    out = []
    for a, b in units:
        out.append(complex(a, b))
        if b > 0.0:
            out.append(complex(a, -b))
    return np.array(out, dtype=np.complex128)


def units_of(roots):
    """the inverse of expand() for roots in application order"""
    roots = np.asarray(roots, dtype=np.complex128)
    out, k = [], 0
    while k < len(roots):
        if roots[k].imag == 0.0:
            out.append((roots[k].real, 0.0))
            k += 1
        else:
            assert k + 1 < len(roots) and roots[k + 1] == np.conj(roots[k]) and roots[k].imag > 0.0
            out.append((roots[k].real, roots[k].imag))
            k += 2
    return out


def roots_from_hessenberg(H, breakdown=False):
    try:
        Hhat = harmonic_matrix(H, breakdown)
    except np.linalg.LinAlgError:
        raise NearZeroRoot("the Hessenberg matrix is singular (near-zero root: a singular matrix needs the null vector)")
    units = leja_order(pair_roots(np.linalg.eigvals(Hhat)))
    big = max(np.hypot(a, b) for a, b in units)
    if any(not np.hypot(a, b) > ZERO_TOL * big for a, b in units):
        raise NearZeroRoot("near-zero root: a singular matrix needs the null vector")
    return expand(units)


def roots(A, d, null=None, offset=0, rows=None, mode="plain"):
    """the roots of the degree-d polynomial in application order (complex array; shorter after a breakdown)"""
    H, _, breakdown, _ = arnoldi(A, d, null, offset, rows, mode=mode)
    return roots_from_hessenberg(H, breakdown)


def rounding_spread(A, d, null=None, rows=None):
    """(spread of H, spread of the roots): the largest difference between the restatement as written, with every dot and
    norm summed in reversed order, and with numpy.longdouble accumulation -- relative to max |H| and max |theta|"""
    Hs = [arnoldi(A, d, null, rows=rows, mode=m) for m in ("plain", "reversed", "longdouble")]
    rs = [roots_from_hessenberg(h[0], h[2]) for h in Hs]
    sh = max(float(np.max(np.abs(h[0] - Hs[0][0]))) for h in Hs[1:]) / float(np.max(np.abs(Hs[0][0])))
    sr = max(float(np.max(np.abs(r - rs[0]))) for r in rs[1:]) / float(np.max(np.abs(rs[0])))
    return sh, sr


def _matvec(A, x, dtype):
    if dtype == np.float64:
        return A @ x
    prod = A.data.astype(dtype) * x[A.indices]
    y = np.zeros(A.shape[0], dtype=dtype)
    np.add.at(y, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), prod)
    return y


def poly_of_b(A, roots, v, dtype=np.float64):
    """p(B) v in product form, every operation in `dtype`"""
    A = cr.as_csr(A)
    dinv = dinv_of(A).astype(dtype)

    def B(x):
        return dinv * _matvec(A, x, dtype)

    units = units_of(roots)
    r = np.array(v, dtype=dtype)
    z = np.zeros(len(r), dtype=dtype)
    for k, (a, b) in enumerate(units):
        last = k + 1 == len(units)
        a, b = dtype(a), dtype(b)
        if b == 0:
            z = z + r / a
            if not last:
                r = r - B(r) / a
        else:
            mod = a * a + b * b
            t = 2 * a * r - B(r)
            z = z + t / mod
            if not last:
                r = r - B(t) / mod
    return z


def apply(A, roots, r, dtype=np.float64):
    """z = p(B) D^-1 r"""
    return poly_of_b(A, roots, dinv_of(A).astype(dtype) * np.asarray(r, dtype=dtype), dtype)


def minv(A, roots):
    A = cr.as_csr(A)
    return lambda r: apply(A, roots, r)


def rounding_gap(A, roots, r):
    """max |z_fp64 - z_longdouble| of the restatement on these inputs, and max |z|"""
    z = apply(A, roots, r)
    zl = apply(A, roots, r, np.longdouble)
    return float(np.max(np.abs(z - zl))), float(np.max(np.abs(z)))


def sigma_min_bound(Hhat, roots):
    """max over the roots of sigma_min(H^ - theta I) / ||H^||_2"""
    nrm = np.linalg.norm(Hhat, 2)
    m = Hhat.shape[0]
    return max(float(np.linalg.svd(Hhat - th * np.eye(m), compute_uv=False)[-1]) for th in roots) / nrm


def cyclic(n=130):
    """I + 0.5 S_+ + 0.05 S_-, S_+- the cyclic shifts: nonsymmetric, a circle of eigenvalues around 1"""
    import scipy.sparse as sps
    i = np.arange(n)
    A = sps.csr_matrix((np.ones(n), (i, i)), shape=(n, n)) + sps.csr_matrix((np.full(n, 0.5), (i, (i + 1) % n)), shape=(n, n)) \
        + sps.csr_matrix((np.full(n, 0.05), (i, (i - 1) % n)), shape=(n, n))
    A = A.tocsr()
    A.sort_indices()
    return A
