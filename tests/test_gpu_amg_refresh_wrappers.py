"""-m gpu: the callers of the SA-AMG / Chebyshev refresh.
  * the C++ mirror (tests/cpp/test_amg_refresh_wrappers.cpp): under SolverLin_HIP::holdPattern a PrecondWrapper_ML with
    "isph: amg refresh" keeps its hierarchy and refreshes it on the refilled matrix (the counter says so), with the
    iterations of a mirror without hold to +-1; the Chebyshev polynomial of PrecondWrapper_Ifpack is kept and refreshed to
    the bits of a rebuild; a changed parameter means a fresh build;
  * the Newton driver of the Poisson-Boltzmann solve with prec_refresh = 1 against prec_refresh = 0."""
import subprocess

import numpy as np
import pytest

from isph_amd import build, hip
import test_gpu_pattern_hold as tph
import test_gpu_poisson_boltzmann as tpb

pytestmark = pytest.mark.gpu


def parse(stdout):
    calls = []
    for line in stdout.splitlines():
        if line.startswith("call "):
            kv = dict(t.split("=") for t in line.split()[1:])
            calls.append((kv["seq"], int(kv["k"]), int(kv["converged"]), int(kv["iters"]), int(kv["refreshes"])))
    return calls


def test_mirror_refreshes_its_hierarchy_and_its_polynomial_under_hold(tmp_path):
    rp, ci, _, n, xy = tph.lattice()
    nnz = len(ci)
    diag = ci == np.repeat(np.arange(n), np.diff(rp))
    vals = np.stack([np.where(diag, 8.5, -1.0), np.where(diag, 17.5, -2.5)])
    bs = np.random.default_rng(11).standard_normal((2, n))
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, nnz], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); vals.tofile(f); bs.tofile(f)
    r = subprocess.run([build.build_cpp_amg_refresh_test(), fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    calls = parse(r.stdout)
    names = [c[:2] for c in calls]
    assert names == [(s, k) for s in ("mlplain", "mlheld", "chebplain", "chebheld", "mlchanged") for k in range(2)], names
    assert all(c[2] == 1 for c in calls), calls
    x = np.fromfile(fout).reshape(len(calls), n)
    by = {c[:2]: (c, x[i]) for i, c in enumerate(calls)}
    # ML: the second held solve is a refresh of the hierarchy of the first; without hold nothing outlives the solve (-1)
    assert by[("mlplain", 1)][0][4] == -1 and by[("mlheld", 0)][0][4] == 0 and by[("mlheld", 1)][0][4] == 1
    for k in range(2):
        (cp, xp), (ch, xh) = by[("mlplain", k)], by[("mlheld", k)]
        assert abs(cp[3] - ch[3]) <= 1, (cp, ch)
        assert np.linalg.norm(xp - xh) <= 1e-6 * np.linalg.norm(xp)
    # Chebyshev: kept and set up again -- the bits and the iterations of the rebuild
    for k in range(2):
        (cp, xp), (ch, xh) = by[("chebplain", k)], by[("chebheld", k)]
        assert cp[3] == ch[3] and np.array_equal(xp.view(np.uint64), xh.view(np.uint64)), k
    # a parameter changed between two held solves: one notice, a fresh hierarchy (its counter starts again)
    assert by[("mlchanged", 1)][0][4] == 0 and r.stdout.count("its parameters changed") == 1


@pytest.mark.parametrize("kind", [0, 1])
def test_newton_driver_refreshes_its_preconditioner(gpu_ctx, kind):
    """the harmonic case at N = 32, prec_max_age = 1: every Newton step after the first refreshes (prec_refresh = 1) where
    prec_refresh = 0 destroys and builds; same Newton steps, psi to the table's tolerance (1e-8 of err_psi)"""
    h = tpb._harmonic(gpu_ctx, 32)
    out = {}
    for refresh in (0, 1):
        J = tpb._assemble_harmonic(gpu_ctx, h)
        psi = np.zeros(h["n"])
        prm = hip.PBParams(f_tol=1e-6, update_tol=4e-16 * h["n"], max_iters=30, linear=dict(tol=1e-13, max_iters=400),
                           prec_max_age=1, prec_kind=kind, prec_refresh=refresh)
        info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, h["f"], params=prm)
        J.close()
        assert info.status == 1, (info.status, info.newton_iters, info.norm_f, info.norm_update)
        out[refresh] = (info, psi, tpb._harmonic_errors(gpu_ctx, h, psi))
    (i0, p0, r0), (i1, p1, r1) = out[0], out[1]
    assert i0.newton_iters == i1.newton_iters and i0.prec_builds == i1.prec_builds == i0.newton_iters
    assert i0.prec_refreshes == 0 and i1.prec_refreshes == i1.prec_builds - 1 >= 1
    assert abs(r0["err_psi"] - r1["err_psi"]) <= 1e-8 * r0["err_psi"]
    assert abs(r0["err_grad"] - r1["err_grad"]) <= 1e-8 * r0["err_grad"]
    assert np.max(np.abs(p0 - p1)) <= 1e-10 * np.max(np.abs(p0))
    assert hip.PBParams().prec_refresh == 0
