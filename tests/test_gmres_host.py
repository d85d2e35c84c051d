"""CPU: the host side of a GMRES cycle (csrc/gmres_host.hpp: Givens-rotated Hessenberg matrix, back-substitution, the
restart rule that gmres_t, gmres_lockstep_t and gcrodr share) against numpy's least squares, on degenerate columns, and
through every row of the restart rule."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 2.5
SEEDS = range(20)                                          # x 5 sizes = 100 matrices


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gmres_host") / "test_gmres_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_gmres_host.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "implicit-sph_amd", "csrc"), "-o", out, src],
                   check=True)
    return out


def _hessenberg_cmd(H, beta):
    m = H.shape[1]
    return "H %d %.17g\n" % (m, beta) + "\n".join(" ".join("%.17g" % v for v in row) for row in H) + "\n"


def _push_all(exe, Hs, beta=BETA):
    """per matrix: [(residual, cs, sn, g[j], g[j+1], y[0..j+1)) after the push of column j, j = 0..m-1]"""
    r = subprocess.run([exe], input="".join(_hessenberg_cmd(H, beta) for H in Hs), capture_output=True, text=True, check=True)
    lines = iter(r.stdout.split("\n"))
    out = []
    for H in Hs:
        steps = []
        for _ in range(H.shape[1]):
            head = [float(v) for v in next(lines).split()]
            steps.append(tuple(head) + (np.array([float(v) for v in next(lines).split()]),))
        out.append(steps)
    return out


@pytest.mark.parametrize("m", [1, 2, 3, 17, 62])
def test_cycle_solves_the_least_squares_problem(exe, m):
    """y and the recurrence residual after j columns against numpy.linalg.lstsq(H[:j+1, :j], beta e_0).  Bounds: a numpy
    restatement of the arithmetic differs from lstsq by at most 4.5e-12 (y, relative) and 2.9e-14 beta (residual) on
    matrices of this kind (condition numbers up to a few thousand); 1e-10 and 1e-12 are roughly 20x and 30x that."""
    Hs = []
    for seed in SEEDS:
        rng = np.random.default_rng([m, seed])
        Hs.append(np.triu(rng.standard_normal((m + 1, m)), -1) + 3 * np.eye(m + 1, m))
    worst_y = worst_r = 0.0
    for H, steps in zip(Hs, _push_all(exe, Hs)):
        for j in sorted({1, m // 2, m} - {0}):
            res, y = steps[j - 1][0], steps[j - 1][5]
            rhs = np.zeros(j + 1)
            rhs[0] = BETA
            yo, *_ = np.linalg.lstsq(H[:j + 1, :j], rhs, rcond=None)
            worst_y = max(worst_y, np.linalg.norm(y - yo) / np.linalg.norm(yo))
            worst_r = max(worst_r, abs(res - np.linalg.norm(rhs - H[:j + 1, :j] @ yo)) / BETA)
    print("m = %d: worst gap to lstsq: y %.3e (relative), residual %.3e beta" % (m, worst_y, worst_r))
    assert worst_y <= 1e-10 and worst_r <= 1e-12


def test_degenerate_columns_are_exact(exe):
    z0 = np.array([[0.0, 1.0], [0.0, 2.0], [0.0, 3.0]])            # first column zero
    z1 = np.array([[3.0, 0.0], [4.0, 0.0], [0.0, 0.0]])            # second column zero: still zero after the first rotation
    hb = np.array([[3.0, 1.0], [4.0, -7.0], [0.0, 0.0]])           # happy breakdown in the second column
    s0, s1, sb = _push_all(exe, [z0, z1, hb])
    res, cs, sn, gj, gj1, _ = s0[0]
    assert (res, cs, sn, gj, gj1) == (0.0, 1.0, 0.0, BETA, 0.0)     # g[0] = beta unchanged
    g1_before = s1[0][4]                                            # g[1] as the first push left it
    assert s1[0][1:3] == (0.6, 0.8) and g1_before == -0.8 * BETA
    res, cs, sn, gj, gj1, _ = s1[1]
    assert (res, cs, sn, gj, gj1) == (0.0, 1.0, 0.0, g1_before, 0.0)
    res, cs, sn, gj, gj1, y = sb[1]
    assert res == 0.0 and sn == 0.0 and gj1 == 0.0 and abs(cs) == 1.0
    yo = np.linalg.solve(hb[:2], [BETA, 0.0])                       # the breakdown makes the square system exact
    assert np.linalg.norm(y - yo) <= 1e-14 * np.linalg.norm(yo)


MAX_ITERS, MAX_RESTARTS = 10, 3
SCALE, TOL = 2.0, 1e-8
# (f32, converged, iters, restarts, residual_restarts) -> (residual needed, converged, iters, restarts, residual_restarts)
AFTER_UPDATE = [
    ((0, 0, 5, 1, 0), (1, 0, 5, 2, 0)),      # plain restart: counted in restarts only
    ((0, 0, 5, 2, 0), (1, 0, 5, 3, 0)),      # ... the last one allowed
    ((0, 1, 5, 1, 0), (0, 1, 5, 1, 0)),      # converged: stop
    ((0, 0, 10, 1, 0), (0, 0, 10, 1, 0)),    # iteration limit
    ((0, 0, 11, 1, 0), (0, 0, 11, 1, 0)),
    ((0, 0, 5, 3, 0), (0, 0, 5, 3, 0)),      # restart limit
    ((0, 1, 10, 3, 0), (0, 1, 10, 3, 0)),
    ((1, 0, 5, 1, 1), (1, 0, 5, 2, 1)),      # float basis, not converged: as above
    ((1, 0, 10, 1, 0), (0, 0, 10, 1, 0)),
    ((1, 0, 5, 3, 2), (0, 0, 5, 3, 2)),
    ((1, 1, 5, 1, 0), (1, 1, 5, 1, 0)),      # float basis, recurrence converged: residual needed, nothing counted
    ((1, 1, 10, 1, 0), (1, 1, 10, 1, 0)),    # ... whatever the limits say
    ((1, 1, 5, 3, 0), (1, 1, 5, 3, 0)),
]
# (state as above, beta) -> (new cycle, converged, iters, restarts, residual_restarts); beta / SCALE against TOL
AFTER_RESIDUAL = [
    (((0, 0, 5, 2, 0), 1.0), (1, 0, 5, 2, 0)),       # nothing to confirm: a new cycle
    (((0, 0, 5, 2, 0), 1e-9), (1, 0, 5, 2, 0)),      # ... also below tol: the recurrence decides at 64 bits
    (((0, 0, 5, 2, 0), 0.0), (0, 1, 5, 2, 0)),       # ... zero residual: converged
    (((1, 0, 5, 2, 1), 1.0), (1, 0, 5, 2, 1)),
    (((1, 0, 5, 2, 1), 0.0), (0, 1, 5, 2, 1)),
    (((1, 1, 5, 2, 0), 1e-8), (0, 1, 5, 2, 0)),      # confirmed
    (((1, 1, 5, 2, 0), 2e-8), (0, 1, 5, 2, 0)),      # ... at beta / scale == tol
    (((1, 1, 5, 2, 0), 0.0), (0, 1, 5, 2, 0)),
    (((1, 1, 5, 2, 0), 1.0), (1, 0, 5, 3, 1)),       # not confirmed: restarts and residual_restarts both count it
    (((1, 1, 5, 0, 0), 3e-8), (1, 0, 5, 1, 1)),
    (((1, 1, 10, 2, 0), 1.0), (0, 0, 10, 2, 0)),     # not confirmed at the iteration limit: stop, not converged
    (((1, 1, 5, 3, 1), 1.0), (0, 0, 5, 3, 1)),       # ... at the restart limit
]


def test_restart_rule_row_by_row(exe):
    txt = "".join("U %d %d %d %d %d %d %d\n" % (s + (MAX_ITERS, MAX_RESTARTS)) for s, _ in AFTER_UPDATE)
    txt += "".join("R %d %d %d %d %d %d %d %.17g %.17g %.17g\n" % (s + (MAX_ITERS, MAX_RESTARTS, beta, SCALE, TOL))
                   for (s, beta), _ in AFTER_RESIDUAL)
    r = subprocess.run([exe], input=txt, capture_output=True, text=True, check=True)
    got = [tuple(int(v) for v in l.split()) for l in r.stdout.split("\n") if l]
    want = [w for _, w in AFTER_UPDATE] + [w for _, w in AFTER_RESIDUAL]
    assert len(got) == len(want)
    for case, g, w in zip([s for s, _ in AFTER_UPDATE] + [s for s, _ in AFTER_RESIDUAL], got, want):
        assert g == w, (case, g, w)
