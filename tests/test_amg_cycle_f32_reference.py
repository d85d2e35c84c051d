"""Host checks of tests/amg_cycle_f32_reference.py, the restatement the cycle_bits = 32 GPU tests compare against:

  1. rounded=False is chebyshev_reference.amg_vcycle (<= 1e-14);
  2. its own noise against what it resolves.  With a numpy hierarchy (aggregates of 3 x 3 cells, damped-Jacobi smoothed P)
     on `spd` and `stencil`: the spread of the rounded cycle under three summation orders is below 0.1 of the separation
     ||rounded - fp64|| / ||fp64||, and the separation lies in [1e-8, 1e-6] -- a handful of float roundings (2^-24 = 6e-8
     each, averaging down over a vector) per stored vector of a cycle, far from fp64 round-off and far from a wrong operator.
     Measured (degrees 1-3, three right-hand sides, with and without the A P shortcut): spread exactly 0 everywhere;
     separation 5.6e-8 .. 9.1e-8 on spd (1480, 182 and 25 rows), 4.0e-8 .. 7.0e-8 on stencil (210 and 30 rows);
  3. a plain FGMRES(50) to 1e-8 with the rounded cycle takes within one iteration of the fp64 cycle and reaches an explicit
     residual <= 1e-8 * 1.01 (measured on spd: 12/12, 11/11, 8/8 iterations for degrees 1-3, 15/15, 12/12, 11/11 with
     shift 0.01, residuals equal to four digits).
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import amg_cycle_f32_reference as a32
import chebyshev_reference as cr
import krylov_reference as kr

DEGREES = [1, 2, 3]
ORDERS = [None, 1, 2]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def hierarchy(name, shift=None):
    if name == "spd":
        A = kr.laplace2d(40, 37, seed=21, shift=0.3 if shift is None else shift)
        return a32.lattice_hierarchy(A, 40, 37)
    rp, ci, val = cr.system("stencil")[:3]
    n = len(rp) - 1
    return a32.lattice_hierarchy(sps.csr_matrix((val, ci, rp), shape=(n, n)), 7, 6, 5)


def rhs(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


@pytest.mark.parametrize("name", ["spd", "stencil"])
def test_unrounded_is_the_fp64_cycle(name):
    levels = hierarchy(name)
    n = levels[0][0].shape[0]
    for d in DEGREES:
        for cp in (False, True):
            b = rhs(n, 40 + d)
            z, z0 = a32.cycle(levels, b, d, 20.0, coarse_polynomial=cp, rounded=False), cr.amg_vcycle(levels, b, d, 20.0, cp)
            g = rel(z, z0)
            print("amg-f32-ref unrounded %-8s degree %d coarse polynomial %d gap %.2e" % (name, d, cp, g))
            assert g <= 1e-14


def test_the_lattice_hierarchy_of_spd_has_the_sizes_the_figures_were_taken_on():
    assert [A.shape[0] for A, _ in hierarchy("spd")] == [1480, 182, 25]
    assert [A.shape[0] for A, _ in hierarchy("stencil")][0] == 210 and len(hierarchy("stencil")) >= 2


@pytest.mark.parametrize("shortcut", [True, False])
@pytest.mark.parametrize("name", ["spd", "stencil"])
def test_own_noise_is_far_below_the_separation_from_fp64(name, shortcut):
    levels = hierarchy(name)
    n = levels[0][0].shape[0]
    for d in DEGREES:
        for seed in (50, 51, 52):
            b = rhs(n, seed)
            z64 = a32.cycle(levels, b, d, 20.0, rounded=False)
            zs = [a32.cycle(levels, b, d, 20.0, shortcut=shortcut, order=o) for o in ORDERS]
            spread = max(rel(z, zs[0]) for z in zs[1:])
            sep = rel(zs[0], z64)
            print("amg-f32-ref %-8s shortcut %d degree %d rhs %d spread %.2e separation %.2e" % (name, shortcut, d, seed, spread, sep))
            assert spread < 0.1 * sep
            assert 1e-8 <= sep <= 1e-6


def fgmres(A, b, minv, m=50, tol=1e-8):
    """plain flexible GMRES(m) from x = 0, modified Gram-Schmidt; (x, iterations)"""
    n = len(b)
    x, nb, its = np.zeros(n), np.linalg.norm(b), 0
    for _ in range(20):
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= tol * nb:
            break
        V, Z, H = np.zeros((m + 1, n)), np.zeros((m, n)), np.zeros((m + 1, m))
        V[0] = r / beta
        j_end = 0
        for j in range(m):
            Z[j] = minv(V[j])
            w = A @ Z[j]
            for i in range(j + 1):
                H[i, j] = V[i] @ w
                w = w - H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(w)
            V[j + 1] = w / H[j + 1, j]
            its, j_end = its + 1, j + 1
            e1 = np.zeros(j + 2); e1[0] = beta
            y = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)[0]
            if np.linalg.norm(e1 - H[:j + 2, :j + 1] @ y) <= tol * nb:
                break
        x = x + Z[:j_end].T @ y
    return x, its


@pytest.mark.parametrize("shift", [None, 0.01])
def test_fgmres_with_the_rounded_cycle_keeps_the_iteration_count(shift):
    levels = hierarchy("spd", shift)
    A = levels[0][0]
    b = rhs(A.shape[0], 31)
    for d in DEGREES:
        out = {}
        for rounded in (False, True):
            x, its = fgmres(A, b, a32.minv(levels, sweeps=d, ratio=20.0, rounded=rounded))
            out[rounded] = (its, float(np.linalg.norm(b - A @ x) / np.linalg.norm(b)))
        print("amg-f32-ref fgmres spd shift %s degree %d iterations %d (fp64 cycle: %d) explicit residual %.3e (%.3e)" %
              (shift, d, out[True][0], out[False][0], out[True][1], out[False][1]))
        assert abs(out[True][0] - out[False][0]) <= 1
        assert out[True][1] <= 1e-8 * 1.01 and out[False][1] <= 1e-8 * 1.01
