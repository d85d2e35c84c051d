"""Host checks behind tests/test_gpu_chebyshev_f32.py (no GPU): what the value_bits = 32 mode of the Chebyshev
polynomial is expected to compute, from the numpy restatements alone.

The mode is the fp64 recurrence on A~ = fl32(A) (chebyshev_f32_reference.fl32).  Two facts keep the GPU tests from being
vacuous, and both are established here on the CPU:
  * the polynomial of A~ is NOT the polynomial of A: one application differs by at least 1e-9 max|z| for degrees >= 2,
    four orders above the 1e-12 the device has to reach against the A~ restatement -- so a device that silently read
    doubles would be caught.  (Degree 1 from a zero guess is (1 / theta) D^-1 r: it sees A~ only through the diagonal
    and rho, and is not asserted.)
  * as a preconditioner A~ is as good as A: GMRES(50), and PCG on the symmetric fixture, reach 1e-8 on the same
    iteration.
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import chebyshev_reference as cr
import chebyshev_f32_reference as c32
import krylov_reference as kr

FIXTURES = ["tgv16", "wall42", "stencil", "spd"]
DIFFERS = 1e-9
KS = list(range(1, 201))     # (wall42 with degree 1 needs more than the 80 of the degree-3 tests)


@functools.lru_cache(maxsize=None)
def fixture(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    A = sps.csr_matrix((val, ci, rp), shape=(n, n))
    return A, c32.fl32(A), b, singular


def test_fl32_rounds_values_and_keeps_the_pattern():
    A = sps.csr_matrix(np.array([[1.0 + 2.0 ** -30, 1e-50, 0.0], [0.1, 3.0, -1.0 / 3.0], [0.0, 2.0 ** -140, 7.0]]))
    B = c32.fl32(A)
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    assert B.nnz == A.nnz == 7                                  # 1e-50 -> 0 stays a stored entry
    assert B[0, 0] == 1.0 and B[0, 1] == 0.0
    assert B[2, 1] == 2.0 ** -140                               # a float subnormal is kept
    assert B[1, 0] == float(np.float32(0.1)) != 0.1
    assert np.array_equal(B.data, B.data.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("ratio", [30.0, 5.0])
@pytest.mark.parametrize("name", FIXTURES)
def test_the_single_precision_polynomial_is_another_operator(name, ratio):
    A, A32, _, _ = fixture(name)
    r = np.random.default_rng(5).standard_normal(A.shape[0])
    for d in (2, 3, 7):
        g = c32.gap_max(cr.cheb_apply(A32, r, None, d, ratio), cr.cheb_apply(A, r, None, d, ratio))
        print("cheb-f32-reference %-8s degree %d ratio %4.1f  fl32(A) against A: %.2e" % (name, d, ratio, g))
        assert g >= DIFFERS, (name, d, ratio, g)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("name,method", [("tgv16", "gmres"), ("wall42", "gmres"), ("stencil", "gmres"), ("spd", "gmres"),
                                         ("spd", "pcg")])
def test_solves_converge_on_the_same_iteration(name, method, degree):
    A, A32, b, singular = fixture(name)
    n = A.shape[0]
    null = kr.unit_null(None, n) if singular else None
    counts = []
    for Ap in (A, A32):                                         # the Krylov method always works on the true A
        minv = cr.cheb_minv(Ap, degree, 30.0)
        if method == "gmres":
            it = kr.gmres_iterates(A, b, np.zeros(n), KS, 50, minv, null)
        else:
            it = kr.pcg_iterates(A, b, np.zeros(n), KS, minv, null)
        counts.append(cr.first_below(it, 1e-8))
    print("cheb-f32-reference %-8s %-5s degree %d ratio 30: %s iterations with A, %s with fl32(A)" %
          (name, method, degree, counts[0], counts[1]))
    assert counts[0] is not None and counts[0] == counts[1], counts


@pytest.mark.parametrize("name", ["spd"])
def test_the_cycle_that_smooths_with_fl32_is_another_cycle(name):
    """the numpy V cycle of the GPU test on a hierarchy the host can build itself (the oracle's): smoothing with fl32(A_l)
    against smoothing with A_l"""
    import oracle as orc
    rp, ci, val, _, singular = cr.system(name)
    n = len(rp) - 1
    G = orc.AMG(rp, ci, val, nullvec=None, theta=0.0, block=256, coarse_max=64)
    levels = cr.levels_from(G, n)
    r = np.random.default_rng(10).standard_normal(n)
    for sweeps in (1, 2, 4):
        z64 = c32.amg_vcycle(levels, r, sweeps=sweeps, single=False)
        z32 = c32.amg_vcycle(levels, r, sweeps=sweeps, single=True)
        zcr = cr.amg_vcycle(levels, r, sweeps=sweeps)
        g = float(np.linalg.norm(z32 - z64) / np.linalg.norm(z64))
        print("cheb-f32-reference %-8s cycle sweeps %d  fl32 against fp64 smoothing: %.2e" % (name, sweeps, g))
        assert np.array_equal(z64, zcr)                         # single = False is chebyshev_reference's cycle
        assert g >= 1e-10
