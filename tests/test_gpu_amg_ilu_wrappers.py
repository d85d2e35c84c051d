"""-m gpu: ML's IFPACK smoother through the C++ mirror -- PrecondWrapper_ML with the keys of the reference's
sph-script/ml-ifpack.xml set by hand ("smoother: type" = "IFPACK", "smoother: ifpack type" = "ILU", "smoother: ifpack
overlap" = 0, "fact: level-of-fill" in the sublist "smoother: ifpack list", "smoother: sweeps", "smoother: pre or post" =
"both"), driven through tests/cpp/test_amg_ilu_wrappers.cpp and SolverLin_Belos::solveProblem on the fixture wall42."""
import subprocess

import numpy as np
import pytest

from isph_amd import build, hip
import amg_ilu_reference as ar

pytestmark = pytest.mark.gpu


def run_cpp(tmp_path, fill, sweeps, *more):
    rp, ci, val, b, singular = ar.system("wall42")
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_amg_ilu_test(), fin, fout, "1" if singular else "0", str(fill), str(sweeps)] + list(more),
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


def c_abi_solve(ctx, fill, sweeps):
    rp, ci, val, b, singular = ar.system("wall42")
    n = len(rp) - 1
    A = hip.Matrix.from_csr(ctx, rp, ci, val)
    M = hip.PrecondAMG(ctx, A, params=hip.AmgParams(coarse_max=64, block=256, smoother=4, ilu_fill=fill, sweeps=sweeps))
    x = np.zeros(n)
    info = hip.solve(ctx, A, b.copy(), x, prec=M, singular=singular, params=hip.SolverParams())
    M.close(); A.close()
    return x, info


@pytest.mark.parametrize("fill,sweeps", [(4, 3), (0, 1)])     # ml-ifpack.xml's own setting, and the defaults
def test_wrapper_solves_like_the_c_abi(gpu_ctx, tmp_path, fill, sweeps):
    r, xc = run_cpp(tmp_path, fill, sweeps)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    conv, iters = (int(t.split("=")[1]) for t in line.split()[:2])
    x, info = c_abi_solve(gpu_ctx, fill, sweeps)
    g = np.linalg.norm(xc - x) / np.linalg.norm(x)
    print("amg-ilu wrapper fill %d sweeps %d iterations %d (C ABI %d) x gap %.2e" % (fill, sweeps, iters, info.iters, g))
    assert conv == 1 and info.converged == 1
    assert iters == info.iters
    assert g <= 1e-6


def test_wrapper_refuses_other_ifpack_types_and_overlaps(tmp_path):
    r, _ = run_cpp(tmp_path, 0, 1, "ILUT")
    assert r.returncode == 1
    assert "smoother: ifpack type" in r.stderr and "'ILUT' is not available; available: \"ILU\"" in r.stderr, r.stderr
    r, _ = run_cpp(tmp_path, 0, 1, "ILU", "1")
    assert r.returncode == 1
    assert "\"smoother: ifpack overlap\" = 1 is not available; available: 0" in r.stderr, r.stderr
    r, _ = run_cpp(tmp_path, 9, 1)
    assert r.returncode == 1 and "ilu_fill" in r.stderr, r.stderr
