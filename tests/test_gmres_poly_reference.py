"""-m "not gpu": the restatement tests/gmres_poly_reference.py itself -- the polynomial it builds is the GMRES polynomial
(its iterate and its residual are those of numpy's least squares on H), the real-arithmetic pair step is the complex
product, the Leja order keeps conjugates together, the roots are eigenvalues of H^ to the backward error of a stable
QR, and as a preconditioner it beats Jacobi on the project's pressure systems."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import chebyshev_reference as cr
import gmres_poly_reference as gp
import krylov_reference as kr

KS = list(range(1, 121))


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "cyclic":
        return gp.cyclic(130), None
    if name == "jitter8":
        from isph_amd import workload
        from problems import Problem, tgv_spec
        rp, ci, val, b = Problem(tgv_spec(dim=3, n=8, mode=workload.JITTER, brick=8)).poisson()
        return sps.csr_matrix((val, ci, rp), shape=(len(rp) - 1,) * 2), b
    rp, ci, val, b, _ = cr.system(name)
    return sps.csr_matrix((val, ci, rp), shape=(len(rp) - 1,) * 2), b


def basis(A, d, null=None, start=None):
    """V of the restatement's Arnoldi, rebuilt here from H: v_{j+1} = (B v_j - V h_j) / h_{j+1,j}"""
    H, m, bd, v0 = gp.arnoldi(A, d, null, start=start)
    dinv = gp.dinv_of(A)
    V = [v0]
    for j in range(m - 1):
        w = dinv * (A @ V[j])
        if null is not None:
            w = w - np.dot(w, null) * null
        V.append((w - np.array(V).T @ H[:j + 1, j]) / H[j + 1, j])
    return H, np.array(V), v0


@pytest.mark.parametrize("name,d", [("cyclic", 2), ("cyclic", 4), ("cyclic", 5), ("cyclic", 8), ("stencil", 6), ("spd", 12), ("wall42", 25)])
def test_polynomial_is_the_gmres_iterate_and_leaves_the_least_squares_residual(name, d):
    A = matrix(name)[0]
    H, V, v0 = basis(A, d)
    roots = gp.roots_from_hessenberg(H)
    e1 = np.zeros(d + 1)
    e1[0] = 1.0
    y, *_ = np.linalg.lstsq(H, e1, rcond=None)
    x_gmres = V.T @ y
    z = gp.poly_of_b(A, roots, v0)
    res = np.linalg.norm(v0 - gp.dinv_of(A) * (A @ z))
    lsq = np.linalg.norm(e1 - H @ y)
    gap = np.linalg.norm(z - x_gmres) / np.linalg.norm(x_gmres)
    print("poly-ref %-8s d %2d iterate gap %.2e residual %.6e least squares %.6e" % (name, d, gap, res, lsq))
    # the roots are computed to ~1e-15 ||H^||; the polynomial's values move by that times the conditioning of the root
    # set, which the monomial-free product form keeps near cond(V_d^T B V_d) -- 1e-9 covers d = 25 on these systems
    assert gap <= 1e-9
    assert abs(res - lsq) <= 1e-9 * max(lsq, 1e-3)
    assert lsq < 1.0


def test_random_start_vectors_give_the_root_patterns_of_the_cyclic_matrix():
    """one conjugate pair alone, reals and pairs mixed, a real root in front of / behind pairs: every branch of the product
    form is met by some start vector and degree"""
    A = matrix("cyclic")[0]
    seen = set()
    for seed in range(8):
        u = np.random.default_rng(seed).standard_normal(130)
        for d in (2, 3, 4, 5, 8):
            H, _, bd, _ = gp.arnoldi(A, d, start=u)
            units = gp.units_of(gp.roots_from_hessenberg(H, bd))
            kinds = "".join("p" if b > 0 else "r" for _, b in units)
            seen.add(kinds)
    print("poly-ref patterns", sorted(seen))
    assert any(k == "p" for k in seen) and any("r" in k and "p" in k for k in seen)
    assert any(k.endswith("p") and len(k) > 1 for k in seen) and any(k.endswith("r") and "p" in k for k in seen)


@pytest.mark.parametrize("d", [3, 4, 5, 7, 10])
def test_the_real_pair_step_equals_complex_arithmetic(d):
    A = matrix("cyclic")[0]
    roots = gp.roots(A, d)
    assert np.any(np.abs(roots.imag) > 1e-3)
    Bm = (sps.diags(gp.dinv_of(A)) @ A).toarray().astype(np.complex128)
    v = np.random.default_rng(d).standard_normal(130)
    # z = sum_k (1 / theta_k) prod_{j < k} (I - B / theta_j) v, one complex root at a time
    r, z = v.astype(np.complex128), np.zeros(130, dtype=np.complex128)
    for th in roots:
        z = z + r / th
        r = r - (Bm @ r) / th
    got = gp.poly_of_b(A, roots, v)
    print("poly-ref pair step d %d max imaginary part %.2e gap %.2e" % (d, np.max(np.abs(z.imag)), np.max(np.abs(got - z.real))))
    assert np.max(np.abs(z.imag)) <= 1e-13 * np.max(np.abs(z.real))
    assert np.max(np.abs(got - z.real)) <= 1e-13 * np.max(np.abs(z.real))


@pytest.mark.parametrize("name,d", [("cyclic", d) for d in range(1, 13)] + [("stencil", 9), ("wall42", 16), ("spd", 25)])
def test_leja_order_starts_at_the_largest_root_and_keeps_conjugates_together(name, d):
    roots = gp.roots(matrix(name)[0], d)
    assert len(roots) == d
    assert abs(roots[0]) >= np.max(np.abs(roots)) * (1.0 - 4e-16)   # (|conj(t)| and |t| may differ in the last bit)
    k = 0
    while k < d:
        if roots[k].imag != 0.0:
            assert roots[k].imag > 0.0 and roots[k + 1] == np.conj(roots[k])
            k += 2
        else:
            k += 1
    # every later root is the farthest of those left from the ones in front of it
    units = gp.units_of(roots)
    for k in range(1, len(units)):
        front = gp.expand(units[:k])
        dist = [np.sum(np.log(np.abs(complex(*u) - front))) for u in units[k:]]
        assert dist[0] >= max(dist) - 1e-12


@pytest.mark.parametrize("name,d", [("cyclic", 8), ("cyclic", 25), ("stencil", 25), ("wall42", 25), ("spd", 25), ("tgv16", 25)])
def test_roots_are_eigenvalues_of_the_harmonic_matrix_to_the_backward_error_of_qr(name, d):
    A = matrix(name)[0]
    null = np.ones(A.shape[0]) / np.sqrt(A.shape[0]) if name == "tgv16" else None
    H, _, bd, _ = gp.arnoldi(A, d, null)
    roots = gp.roots_from_hessenberg(H, bd)
    s = gp.sigma_min_bound(gp.harmonic_matrix(H, bd), roots)
    print("poly-ref sigma_min %-8s d %2d %.2e" % (name, d, s))
    assert s <= 1e-12


def test_breakdown_gives_the_lower_degree_and_a_singular_matrix_is_refused():
    n = 130
    D = sps.diags(1.0 + np.arange(n) % 7).tocsr()            # B = I: an invariant subspace after one step
    H, m, bd, _ = gp.arnoldi(D, 5)
    assert (m, bd) == (1, True)
    assert np.allclose(gp.roots_from_hessenberg(H, bd), [1.0], atol=1e-15)
    # the Neumann Laplacian on 6 points without its null vector: six steps span the whole space, zero eigenvalue included
    n = 6
    L = sps.diags([np.full(n - 1, -1.0), np.r_[1.0, np.full(n - 2, 2.0), 1.0], np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    with pytest.raises(gp.NearZeroRoot):
        gp.roots(L, 6)
    r = gp.roots(L, 5, null=np.ones(n))                      # with it: the five other eigenvalues of D^-1 A
    ev = np.sort(np.linalg.eigvals((sps.diags(gp.dinv_of(L)) @ L).toarray()).real)[1:]
    assert len(r) == 5 and np.allclose(np.sort(r.real), ev, atol=1e-12) and np.all(r.imag == 0.0)


@pytest.mark.parametrize("name", ["tgv16", "jitter8"])
def test_degree_4_needs_fewer_iterations_than_jacobi(name):
    A, b = matrix(name)
    n = A.shape[0]
    null = kr.unit_null(None, n)                             # both are all-Neumann pressure systems: singular
    counts = {}
    for kind in ("jacobi", "poly4"):
        Minv = kr.jacobi_minv(A) if kind == "jacobi" else gp.minv(A, gp.roots(A, 4, null))
        counts[kind] = cr.first_below(kr.gmres_iterates(A, b, np.zeros(n), KS, 50, Minv, null), 1e-8)
    print("poly-ref %-8s iterations jacobi %s gmres-poly4 %s" % (name, counts["jacobi"], counts["poly4"]))
    assert counts["poly4"] is not None and counts["jacobi"] is not None
    assert counts["poly4"] < counts["jacobi"]
