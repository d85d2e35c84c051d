"""Host checks of tests/amg_ilu_reference.py, the expected values of tests/test_gpu_amg_ilu.py (no GPU).

The restated cycle against the same cycle built on the oracle's block ILU(k), and the preconditioned reference solves the
GPU tests gate their iteration counts on.  Iterations of GMRES(50) to a true relative residual of 1e-8 on the oracle's
hierarchy (block 256, coarse_max 64, theta 0), sweeps 1 / 2 / 3, as the tests below find them:

  fixture   level rows        smoother 0   fill 0         fill 1         fill 4
  stencil   210, 17            6           6 / 4 / 3      4 / 3 / 2      3 / 2 / 1
  wall42    1764, 35          14           13 / 10 / 9    18 / 13 / 10   21 / 15 / 12
  spd       1480, 222, 16      8           8 / 5 / 4      9 / 6 / 5      9 / 6 / 5
  tgv16     4096, 15 (null)   13           12 / 9 / 7     13 / 9 / 7     13 / 9 / 8
  lap96s    8640, 1214, 76     9           9 / - / 5      -              11 / - / 6

(krylov_reference.gmres_iterates' count of the first iterate whose TRUE residual is below 1e-8; a GMRES that stops on its
recurrence residual can report one more.)  The restated cycle agrees with the cycle on the oracle's ILU to 1.3e-16 ..
1.5e-15 (gate 1e-13).

tgv16 with the ILU kept on its 15-row singular coarsest level does not converge: the reason for the Gauss-Seidel rule.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import amg_ilu_reference as ar
import chebyshev_reference as cr
import krylov_reference as kr

AMG_KW = dict(theta=0.0, block=256, coarse_max=64)
KS = list(range(1, 51))
SETTINGS = [(name, fill, sweeps) for name in ar.FIXTURES[:4] for fill in (0, 1, 4) for sweeps in (1, 2, 3)]
SETTINGS += [("lap96s", fill, sweeps) for fill in (0, 4) for sweeps in (1, 3)]


@functools.lru_cache(maxsize=None)
def fixture(name):
    rp, ci, val, b, singular = ar.system(name)
    n = len(rp) - 1
    return sps.csr_matrix((val, ci, rp), shape=(n, n)), b, singular


@functools.lru_cache(maxsize=None)
def oracle_levels(name):
    import oracle as orc
    rp, ci, val, _, singular = ar.system(name)
    n = len(rp) - 1
    nv = np.ones(n) / np.sqrt(n) if singular else None
    G = orc.AMG(rp, ci, val, nullvec=nv, **AMG_KW)
    assert G.levels >= 2
    return cr.levels_from(G, n)


@functools.lru_cache(maxsize=None)
def smoothers(name, fill, factor=ar.BlockILU, ilu_on_coarsest=False):
    return ar.build_smoothers(oracle_levels(name), fill, AMG_KW["block"], coarse_smoother=fixture(name)[2],
                              ilu_on_coarsest=ilu_on_coarsest, factor=factor)


def minv(name, fill, sweeps, **kw):
    S, levels = smoothers(name, fill, **kw), oracle_levels(name)
    return lambda r: ar.amg_vcycle(levels, S, np.asarray(r, dtype=np.float64), sweeps)


def iterations(name, M):
    A, b, singular = fixture(name)
    n = A.shape[0]
    null = kr.unit_null(None, n) if singular else None
    return cr.first_below(kr.gmres_iterates(A, b, np.zeros(n), KS, 50, M, null), 1e-8)


@pytest.mark.parametrize("name", ar.FIXTURES)
def test_level_rows_of_the_fixtures(name):
    rows = [A.shape[0] for A, _ in oracle_levels(name)]
    print("amg-ilu-levels %-8s %s" % (name, rows))
    assert rows == {"stencil": [210, 17], "wall42": [1764, 35], "spd": [1480, 222, 16], "tgv16": [4096, 15],
                    "lap96s": [8640, 1214, 76]}[name]


@pytest.mark.parametrize("name", ar.FIXTURES)
@pytest.mark.parametrize("fill", [0, 1, 4])
def test_restated_cycle_agrees_with_the_cycle_on_the_oracle_ilu(name, fill):
    """<= 1e-13 relative for sweeps 1 and 3: the restated block ILU(k) is the oracle's"""
    A, b, _ = fixture(name)
    for sweeps in (1, 3):
        z = minv(name, fill, sweeps)(b)
        zo = minv(name, fill, sweeps, factor=ar.OracleILU)(b)
        gap = np.linalg.norm(z - zo) / np.linalg.norm(zo)
        print("amg-ilu-oracle-gap %-8s fill %d sweeps %d %.2e" % (name, fill, sweeps, gap))
        assert gap <= 1e-13


@pytest.mark.parametrize("name,fill,sweeps", SETTINGS)
def test_gmres_with_the_restated_cycle_converges_without_a_restart(name, fill, sweeps):
    k = iterations(name, minv(name, fill, sweeps))
    print("amg-ilu-ref-iters %-8s fill %d sweeps %d %s" % (name, fill, sweeps, k))
    assert k is not None and k <= 50


@pytest.mark.parametrize("name", ar.FIXTURES)
def test_gmres_with_the_gauss_seidel_cycle_converges(name):
    """smoother 0 over the same levels: the yardstick of the table above"""
    k = iterations(name, ar.sgs_minv(oracle_levels(name), 1, AMG_KW["block"], coarse_smoother=fixture(name)[2]))
    print("amg-ilu-ref-iters %-8s smoother 0 %s" % (name, k))
    assert k is not None and k <= 50


def test_ilu_on_the_singular_coarsest_level_does_not_converge():
    """ILU(0) of tgv16's 15-row coarsest operator -- one full block -- is the complete LU of a singular matrix: the cycle
    blows up and GMRES(50) does not reach 1e-8 in 400 iterations.  Hence the Gauss-Seidel rule on that level."""
    A, b, _ = fixture("tgv16")
    n = A.shape[0]
    M = minv("tgv16", 0, 1, ilu_on_coarsest=True)
    with np.errstate(all="ignore"):
        z = M(b)
        print("amg-ilu-coarsest-ilu |z| %.3e against %.3e with the rule" % (np.linalg.norm(z), np.linalg.norm(minv("tgv16", 0, 1)(b))))
        its = kr.gmres_iterates(A, b, np.zeros(n), [400], 50, M, kr.unit_null(None, n))
    assert not (its[400].rel_res <= 1e-8)


def test_a_level_with_a_row_without_a_diagonal_falls_back_to_gauss_seidel():
    A = sps.lil_matrix(kr.laplace2d(12, 11, seed=5, shift=0.2))
    A[7, :] = 0.0
    A[:, 7] = 0.0
    A = sps.csr_matrix(A)
    A.eliminate_zeros()
    assert not ar.every_row_keeps_its_diagonal(A)
    P = sps.csr_matrix(np.kron(np.eye(A.shape[0] // 4), np.ones((4, 1))))
    levels = [(A, P), (sps.csr_matrix(P.T @ A @ P), None)]
    S = ar.build_smoothers(levels, 1, 64)
    assert isinstance(S[0], ar.BlockSGS) and S[1] is None
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    assert S[0].apply(b)[7] == 0.0   # the empty row's unknown stays at zero
    z = ar.amg_vcycle(levels, S, b, 2)
    assert np.all(np.isfinite(z))
    with pytest.raises(ValueError, match="diagonal"):
        ar.BlockILU(A, 64, 1)
