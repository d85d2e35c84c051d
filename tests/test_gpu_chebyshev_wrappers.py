"""-m gpu: the Chebyshev requests of the C++ mirrors -- PrecondWrapper_Ifpack "Precond Type" = "Chebyshev" and
PrecondWrapper_ML "smoother: type" = "Chebyshev" / "MLS" -- through tests/cpp/test_chebyshev_wrappers.cpp, against the
Python path on the same system: x to 1e-6, iteration counts equal."""
import subprocess

import numpy as np
import pytest

from isph_amd import build, hip
import chebyshev_reference as cr

pytestmark = pytest.mark.gpu


def run_cpp(tmp_path, name, mode):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_chebyshev_test(), fin, fout, "1" if singular else "0", mode],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


def python_solve(ctx, name, mode):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    A = hip.Matrix.from_csr(ctx, rp, ci, val)
    if mode == "ifpack":
        M = hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0)
    elif mode == "ifpack-eig":
        M = hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0, lambda_max=1.7, lambda_min=1.7 / 8.0)
    else:   # the wrapper's list: PrecondWrapper_ML's defaults, "coarse: max size" 64, Chebyshev with 2 sweeps, alpha 20
        nv = np.ones(n) / np.sqrt(n) if singular else None
        M = hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(coarse_max=64, block=256, smoother=2, sweeps=2, cheb_ratio=20.0))
    x = np.zeros(n)
    info = hip.solve(ctx, A, b.copy(), x, prec=M, singular=singular,
                     params=hip.SolverParams(solver_type=1 if mode == "ml-cg" else 0))
    M.close(); A.close()
    return x, info


@pytest.mark.parametrize("name,mode", [("tgv16", "ifpack"), ("wall42", "ifpack"), ("wall42", "ifpack-eig"), ("tgv16", "ml"),
                                       ("wall42", "mls"), ("spd", "ml-cg")])
def test_wrappers_match_the_python_path(gpu_ctx, tmp_path, name, mode):
    r, xc = run_cpp(tmp_path, name, mode)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    x, info = python_solve(gpu_ctx, name, mode)
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    conv, iters = (int(t.split("=")[1]) for t in line.split()[:2])
    print("cheb-wrapper %-8s %-10s iterations %d (python %d) x gap %.2e" %
          (name, mode, iters, info.iters, np.linalg.norm(xc - x) / np.linalg.norm(x)))
    assert conv == 1 and info.converged == 1 and iters == info.iters
    assert np.linalg.norm(xc - x) <= 1e-6 * np.linalg.norm(x)
    if mode == "ifpack":      # two solves: the notice about the ignored keys is printed once
        assert r.stdout.count("mean nothing for this type") == 1
        assert r.stdout.count("Belos::Status - Passed!") == 2


@pytest.mark.parametrize("mode,names", [("bad-ifpack", ['"ILU"', '"Chebyshev"']),
                                        ("bad-ml", ['"symmetric Gauss-Seidel"', '"Chebyshev"', '"MLS"'])])
def test_other_types_are_refused_and_the_message_names_what_is_available(tmp_path, mode, names):
    r, _ = run_cpp(tmp_path, "stencil", mode)
    assert r.returncode == 1
    assert "not available" in r.stderr
    for nm in names:
        assert nm in r.stderr, r.stderr
