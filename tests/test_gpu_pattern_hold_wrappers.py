"""-m gpu: SolverLin_HIP::holdPattern through the C++ mirror (tests/cpp/test_pattern_hold_wrappers.cpp): three
solveProblem calls on one refilled Epetra matrix with and without hold give the same bits; the second and third ingress
of a held matrix move 8 B per entry; a changed row pointer falls back to the full ingress; holdPattern(false) gives
everything back; PrecondWrapper_ML rebuilds on the updated matrix."""
import subprocess

import numpy as np
import pytest

from isph_amd import build
import test_gpu_pattern_hold as tph

pytestmark = pytest.mark.gpu


def system():
    """the 30 x 30 lattice of test_gpu_pattern_hold in shuffled atom order, symmetric positive definite values in three sets"""
    rp, ci, _, n, xy = tph.lattice()
    diag = ci == np.repeat(np.arange(n), np.diff(rp))
    base = np.where(diag, 8.5, -1.0)
    vals = np.stack([base, np.where(diag, 10.0, -1.0), np.where(diag, 17.5, -2.0)])
    bs = np.random.default_rng(11).standard_normal((3, n))
    return rp, ci, vals, bs, n, xy


def movable_row(rp, ci):
    """a row whose last entry is off the diagonal, whose column the next row does not hold, and which lies with that
    column and the next row in one 256-row subdomain (an entry outside the subdomain is dropped by block Jacobi: moving it
    would leave the in-block pattern, and so the kept factor, valid)"""
    for r in range(len(rp) - 2):
        c = ci[rp[r + 1] - 1]
        if c != r and c not in ci[rp[r + 1]:rp[r + 2]] and rp[r + 1] - rp[r] > 2 and r // 256 == c // 256 == (r + 1) // 256:
            return r
    raise AssertionError("no movable row")


def parse(stdout):
    calls, pool = [], None
    for line in stdout.splitlines():
        if line.startswith("call "):
            kv = dict(t.split("=") for t in line.split()[1:])
            calls.append((kv["seq"], int(kv["k"]), int(kv["converged"]), int(kv["iters"]), int(kv["link_bytes"])))
        if line.startswith("pool "):
            pool = tuple(int(t.split("=")[1]) for t in line.split()[1:])
    return calls, pool


@pytest.mark.parametrize("coords", [0, 1])
@pytest.mark.parametrize("fill", [0, 1])
def test_held_solves_are_the_plain_solves(tmp_path, fill, coords):
    rp, ci, vals, bs, n, xy = system()
    nnz = len(ci)
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, nnz], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); vals.tofile(f); bs.tofile(f)
        np.ascontiguousarray(xy[:, 0]).tofile(f); np.ascontiguousarray(xy[:, 1]).tofile(f)
    r = subprocess.run([build.build_cpp_pattern_hold_test(), fin, fout, str(fill), str(coords), str(movable_row(rp, ci))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    calls, pool = parse(r.stdout)
    assert [c[:2] for c in calls] == ([("plain", k) for k in range(3)] + [("held", k) for k in range(3)] + [("moved", 0)] +
                                      [("mlplain", k) for k in range(2)] + [("mlheld", k) for k in range(2)])
    x = np.fromfile(fout).reshape(len(calls), n)
    assert all(c[2] == 1 for c in calls), calls
    for k in range(3):                                                       # same bits, same iteration counts
        assert np.array_equal(x[k].view(np.uint64), x[3 + k].view(np.uint64)), k
        assert calls[k][3] == calls[3 + k][3]
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])
    assert calls[3][4] > 8 * nnz                                             # the first held call is a full ingress
    assert calls[4][4] == 8 * nnz and calls[5][4] == 8 * nnz                 # then the values alone
    assert calls[6][4] != 8 * nnz and calls[6][4] > 8 * nnz                  # changed row pointer: the full ingress again
    assert not np.array_equal(x[6], x[0])
    if fill > 0 and not coords:      # the kept ILU meets another in-block pattern: one notice, then destroy + create
        assert r.stdout.count("could not be refactored") == 1                # (fill 0 without coordinates adopts the fused
                                                                             # ILU; with coordinates the moved entry may
                                                                             # couple two bricks, which block Jacobi drops)
    assert pool is not None and pool[0] == pool[1], pool
    for k in range(2):                                                       # ML: matrix updated, hierarchy rebuilt
        assert np.array_equal(x[7 + k].view(np.uint64), x[9 + k].view(np.uint64)), k
        assert calls[7 + k][3] == calls[9 + k][3]
    assert calls[10][4] == 8 * nnz
