"""Host checks behind tests/test_gpu_ilu_f32.py (no GPU): what the value_bits = 32 mode of the block ILU is expected to
compute, from the numpy restatement alone (tests/ilu_f32_reference.py).

Two facts keep the GPU tests from being vacuous, and both are established here on the CPU:
  * the solves with rounded strict-L / strict-U values are NOT the solves with the doubles: on every fixture of
    tests/ilu_shapes.py one application moves by 3.3e-9 .. 5.5e-9 ||z|| (ILU(0) fixtures) and 8.3e-9 .. 9.5e-9 ||z|| (the
    fill fixtures, K = 1, 2, 3) -- two orders above the 1e-11 the device has to reach against the restatement, and inside
    the [1e-10, 1e-6] asserted below: float rounding is 6e-8 relative per entry, diagonal dominance averages it down;
  * as a preconditioner the rounded factor is as good as the unrounded one: GMRES(50), and PCG on the symmetric fixture,
    reach 1e-8 on the same iteration (measured 21/21, 22/22, PCG 22/22).
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import chebyshev_reference as cr
import ilu_f32_reference as i32
import ilu_shapes as sh
import krylov_reference as kr

LD = np.longdouble
CASES = [(name, 0) for name in sh.ILU0_FIXTURES] + [(name, K) for name in sh.ILUK_FIXTURES for K in (1, 2, 3)]
KS = list(range(1, 81))


def rhs(n):
    """the right-hand side of test_gpu_ilu_shapes.rhs"""
    return np.random.default_rng(5).standard_normal(n)


def test_round_factor_rounds_the_off_diagonals_and_keeps_the_pivots():
    frp = np.array([0, 2, 5, 7], dtype=np.int32)
    fci = np.array([0, 1, 0, 1, 2, 1, 2], dtype=np.int32)
    fv = np.array([1.0 + 2.0 ** -30, 1e-50, 0.1, 3.0 + 2.0 ** -40, -1.0 / 3.0, 2.0 ** -140, 7.1])
    g = i32.round_factor(frp, fci, fv)
    assert g.dtype == LD
    assert g[0] == LD(fv[0]) and g[3] == LD(fv[3]) and g[6] == LD(fv[6])       # the pivots keep their doubles
    assert g[1] == 0.0                                                          # 1e-50 -> 0 stays a stored entry
    assert g[2] == LD(np.float32(0.1)) != LD(0.1)
    assert g[5] == LD(2.0) ** -140                                              # a float subnormal is kept
    assert np.array_equal(i32.round_factor(frp, fci, fv, single=False), fv.astype(LD))


@pytest.mark.parametrize("name,K", CASES)
def test_the_rounded_factor_is_another_operator(name, K):
    rp, ci, val, bp = sh.fixture(name)
    frp, fci, fv = sh.ref_iluk_of(name, K)
    r = rhs(len(rp) - 1)
    z64 = sh.ref_apply_of(name, K, r)
    z32 = i32.apply(frp, fci, fv, bp, r)
    same = i32.rel(i32.apply(frp, fci, fv, bp, r, single=False), z64)
    g = i32.rel(z32, z64)
    print("ilu-f32-reference %-8s K=%d  rounded against unrounded factor: %.2e (unrounded restatement against ilu_shapes: %.1e)" %
          (name, K, g, same))
    assert same == 0.0                                          # single = False is ilu_shapes' application
    assert 1e-10 <= g <= 1e-6, (name, K, g)


@functools.lru_cache(maxsize=None)
def _system(name, bs):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    assert not singular
    bp = kr.block_ptr(n, bs)
    frp, fci, fv = sh.ref_iluk(rp, ci, val, bp, 0)
    return sps.csr_matrix((val, ci, rp), shape=(n, n)), b, bp, frp, fci, fv


@pytest.mark.parametrize("name,bs,method", [("stencil", 64, "gmres"), ("spd", 256, "gmres"), ("spd", 256, "pcg")])
def test_solves_converge_on_the_same_iteration(name, bs, method):
    A, b, bp, frp, fci, fv = _system(name, bs)
    n = A.shape[0]
    counts = []
    for single in (False, True):                                # the Krylov method always works on the true A
        op = i32.operator(frp, fci, fv, bp, single)
        minv = lambda r, op=op: np.asarray(op(r), dtype=np.float64)
        if method == "gmres":
            it = kr.gmres_iterates(A, b, np.zeros(n), KS, 50, minv, None)
        else:
            it = kr.pcg_iterates(A, b, np.zeros(n), KS, minv, None)
        counts.append(cr.first_below(it, 1e-8))
    print("ilu-f32-reference %-8s %-5s blocks of %d: %s iterations with the doubles, %s with the rounded factor" %
          (name, method, bs, counts[0], counts[1]))
    assert counts[0] is not None and counts[0] == counts[1], counts
