"""-m gpu: the GMRES polynomial behind the layers above the C ABI --
  1. PrecondWrapper_Ifpack's "Precond Type" = "GMRES Polynomial" with "isph: polynomial degree" (host/precond_ifpack.h; the
     C++ driver tests/cpp/test_gmres_poly_wrappers.cpp): the iteration count and x of the C ABI with the same degree and the
     null vector the wrapper passes on; a degree out of range fails the solve with the library's message;
  2. the time-step driver: hip.InsStep with prec_poisson = "gmres-poly4" against the written-out chain of
     tests/test_gpu_ins_driver.py with hip.PrecondGmresPoly(ctx, A, 4, nullvec) in place of its block ILU -- three TGV steps
     at N = 16, bit for bit when the chain itself is reproducible run to run (its own tolerances otherwise)."""
import subprocess

import numpy as np
import pytest

from isph_amd import build, hip
import chebyshev_reference as cr
import test_gpu_ins_driver as tid

pytestmark = pytest.mark.gpu


def run_cpp(tmp_path, name, mode):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_gmres_poly_test(), fin, fout, "1" if singular else "0", mode],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


@pytest.mark.parametrize("name,mode,degree", [("wall42", "default", 4), ("tgv16", "default", 4), ("tgv16", "degree6", 6), ("wall42", "degree1", 1)])
def test_wrapper_gives_the_c_abi_count(gpu_ctx, tmp_path, name, mode, degree):
    r, xc = run_cpp(tmp_path, name, mode)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondGmresPoly(gpu_ctx, A, degree, nullvec=np.ones(n) / np.sqrt(n) if singular else None)
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular)
    M.close(); A.close()
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    conv, iters = (int(t.split("=")[1]) for t in line.split()[:2])
    print("poly-wrapper %-8s %-8s iterations %d (C ABI %d) x gap %.2e" % (name, mode, iters, info.iters, np.linalg.norm(xc - x) / np.linalg.norm(x)))
    assert "GMRES polynomial of degree %d" % degree in r.stdout
    assert ("with the null vector" in r.stdout) == singular
    assert conv == 1 and info.converged == 1 and iters == info.iters
    assert np.linalg.norm(xc - x) <= 1e-6 * np.linalg.norm(x)


def test_wrapper_reports_a_degree_out_of_range(tmp_path):
    r, _ = run_cpp(tmp_path, "stencil", "degree26")
    assert r.returncode == 1
    assert "degree must be in [1,25]" in r.stderr, r.stderr


def test_driver_with_the_polynomial_equals_the_chain(gpu_ctx, monkeypatch):
    case = tid.tgv2d_case(16, True, 0.0)                   # theta = 0: the Poisson solve is the step's one preconditioned solve
    n = case.n
    nullvec = np.full(n, 1.0 / np.sqrt(float(n)))          # every particle is fluid: what the driver forms from its mask
    made = []

    def poly_for_the_chain(ctx, A, kind, block_size=512, block_ptr=None):
        made.append(kind)
        return hip.PrecondGmresPoly(ctx, A, 4, nullvec=nullvec)

    with monkeypatch.context() as mp:
        mp.setattr(hip, "Precond", poly_for_the_chain)    # the chain names its preconditioner in one place
        ref = tid.chain(gpu_ctx, case, 3)
        again = tid.chain(gpu_ctx, case, 3)
    assert made == ["bjacobi-ilu0"] * 6                    # three Poisson solves per chain, no Helmholtz solve
    reproducible = all(ref[k].tobytes() == again[k].tobytes() for k in ("x", "v", "p"))
    S = case.driver(gpu_ctx, prec_poisson="gmres-poly4")
    S.run(3, diag=False)
    got = dict(x=S.get("x"), v=S.get("v"), p=S.get("p"))
    S.close()
    print("poly-driver chain run-to-run reproducible: %s" % reproducible)
    assert np.max(np.abs(ref["x"] - case.x)) > 0 and np.isfinite(ref["p"]).all()
    if reproducible:
        tid._same_bits(got, ref, "gmres-poly4")
    else:
        tid._same_to_tolerance(got, ref, 2 * np.pi, 0.1)
