"""-m gpu: parity of the HIP path (through the C ABI) against the CPU oracle on
seeded TGV problems.  Tolerances are stated per test; integer/index work
(sparsity pattern) must match exactly."""
import time

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip, workload
import oracle as orc
from problems import Problem, tgv_spec

pytestmark = pytest.mark.gpu
ROOT_DIR = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))

CASES = [
    dict(dim=2, n=16, mode=workload.JITTER),
    dict(dim=2, n=33, mode=workload.ADVECT),            # ragged: 1089 rows, not a multiple of 64
    dict(dim=3, n=12, mode=workload.JITTER),
    dict(dim=3, n=16, mode=workload.ADVECT),
    dict(dim=3, n=10, mode=workload.JITTER, kernel="quintic", cut_over_h=3.0),
    dict(dim=2, n=12, mode=workload.LATTICE, kernel="cubic", cut_over_h=2.0),
]


def _csr(rp, ci, v, n):
    return sps.csr_matrix((v, ci, rp), shape=(n, n))


@pytest.mark.parametrize("case", CASES)
def test_csr_ingress_roundtrip_and_spmv(gpu_ctx, case):
    pr = Problem(tgv_spec(**case))
    rp, ci, val, b = pr.poisson()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    info = A.info()
    assert info["nrow"] == pr.n and info["nnz"] == len(val)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci) and np.array_equal(v2, val)   # bit-exact layout round trip
    x = np.random.default_rng(1).standard_normal(pr.n)
    y = A.spmv(x)
    yo = orc.spmv(rp, ci, val, x)
    scale = np.abs(_csr(rp, ci, np.abs(val), pr.n) @ np.abs(x))
    assert np.max(np.abs(y - yo) / scale) < 1e-14          # fp64, different summation order only
    # linearity (size-independent property)
    x2 = np.random.default_rng(2).standard_normal(pr.n)
    assert np.allclose(A.spmv(2.0 * x + x2), 2.0 * y + A.spmv(x2), rtol=1e-12, atol=1e-12 * scale.max())


def test_empty_and_tiny_matrices(gpu_ctx):
    A = hip.Matrix.from_csr(gpu_ctx, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert A.info()["nrow"] == 0
    rp = np.array([0, 1, 1, 3], np.int32)            # row 1 is empty
    ci = np.array([0, 0, 2], np.int32)
    v = np.array([2.0, -1.0, 4.0])
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    assert np.array_equal(A.spmv(np.array([1.0, 5.0, 0.5])), np.array([2.0, 0.0, 1.0]))
    with pytest.raises(hip.IsphError):
        hip.Matrix.from_csr(gpu_ctx, rp, np.array([0, 0, 7], np.int32), v)     # column out of range


def test_entry_points_read_no_more_than_the_abi_documents():
    """tests/guarded_operands.py in a child process: every host operand ends at an unreadable page, so an entry point
    that reads past the element counts of include/isph_hip.h dies with SIGSEGV there (return code -11) instead of
    passing by luck."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "guarded_operands.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "rc %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "every entry point stayed inside its buffers" in r.stdout
    # the guard itself: an operand that is one element short must kill the child (SIGSEGV)
    r = subprocess.run([sys.executable, os.path.join(here, "guarded_operands.py"), "--negative-control"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == -11 and "unnoticed" not in r.stdout, (r.returncode, r.stdout[-500:])


def test_device_buffer_canary_mode_bites():
    """ISPH_POOL_CANARY=1 (csrc/common.hpp): every pooled device buffer carries a pattern behind its last element that
    is checked when the buffer is given back -- the stand-in for the GPU address sanitizer this pool does not offer;
    the whole -m gpu suite runs clean under it.  Here: the mode's own self-test, a deliberate one-byte
    overrun, must abort the child process, and the same child without the overrun must not."""
    import os
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); import isph_amd; from isph_amd import hip; c = hip.Context(0); c.close(); print('alive')" % ROOT_DIR
    env = dict(os.environ, ISPH_POOL_CANARY="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "alive" in r.stdout, r.stderr[-2000:]
    env["ISPH_POOL_CANARY_SELFTEST"] = "1"
    r = subprocess.run([sys.executable, "-c", "import resource; resource.setrlimit(resource.RLIMIT_CORE, (0, 0)); " + code],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == -6 and "ISPH_POOL_CANARY: a kernel wrote" in r.stderr and "alive" not in r.stdout, (r.returncode, r.stderr[-500:])


def test_rank_without_particles(gpu_ctx):
    """LAMMPS subdomains may be empty: nlocal = nall = 0 goes through computePre, the assembly, every preconditioner
    set-up and the solve (which still takes part in the collectives) and comes back converged after 0 iterations."""
    spec = tgv_spec(dim=3, n=8, mode=workload.JITTER)
    e = dict(workload.make_tgv(spec))
    e.update(nlocal=0, nall=0, x=np.zeros((0, 3)), type=np.zeros(0, np.int32), neigh_ptr=np.zeros(1, np.int32),
             neigh_idx=np.zeros(0, np.int32))
    colmap = np.zeros(0, np.int32)
    assert hip.compute_volumes(gpu_ctx, e, colmap).shape == (0,)
    A, b = hip.assemble_poisson(gpu_ctx, e, colmap, spec.dt, np.zeros(0), np.zeros((0, 3)), vfrac=np.zeros(0))
    assert A.info()["nrow"] == 0 and A.info()["nnz"] == 0 and b.shape == (0,)
    for make in (lambda: hip.Precond(gpu_ctx, A, "jacobi", 512), lambda: hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 512),
                 lambda: hip.Precond(gpu_ctx, A, "bjacobi-ilu1", 512), lambda: hip.PrecondAMG(gpu_ctx, A, nullvec=np.zeros(0))):
        M = make()
        info = hip.solve(gpu_ctx, A, b, np.zeros(0), prec=M, singular=True)
        assert info.converged == 1 and info.iters == 0
        M.close()
    Ah, bh = hip.assemble_helmholtz(gpu_ctx, e, colmap, spec.dt, 0.5, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3)),
                                    np.zeros(3), np.zeros((0, 3)), vfrac=np.zeros(0))
    assert Ah.info()["nrow"] == 0 and bh.shape == (0,)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("antisym", [True, False])
def test_gpu_assembly_matches_oracle(gpu_ctx, case, antisym):
    pr = Problem(tgv_spec(**case), antisym=antisym)
    rp, ci, val, b = pr.poisson()
    p = pr.parts
    vfrac = pr.P.vfrac.copy()
    # volumes first (FunctorOuterVolume): parity 1e-14 relative
    vg = hip.compute_volumes(gpu_ctx, p, pr.colmap, kernel=pr.spec.kernel)
    assert np.max(np.abs(vg - vfrac[:pr.n]) / vfrac[:pr.n]) < 1e-13
    keep = []
    pv, dev, keep = hip.particles_view(p, pr.colmap, kernel=pr.spec.kernel, vfrac=vfrac,
                                       Gc=None if antisym else pr.P.Gc, Lc=None if antisym else pr.P.Lc, keep=keep)
    import ctypes as C
    A = hip.Matrix(gpu_ctx)
    bg = np.zeros(pr.n)
    hip._check(hip.lib().isph_assemble_poisson(gpu_ctx.h, C.byref(pv), int(antisym), float(pr.spec.dt),
                                               hip._ptr(p["rho"]), hip._ptr(np.ascontiguousarray(p["v"])),
                                               hip.NULLSPACE, 1, pr.n, C.byref(A.h), hip._ptr(bg), 0))
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)          # sparsity pattern: exact
    scale = np.abs(val).max()
    assert np.max(np.abs(v2 - val)) < 1e-12 * scale                     # values: fp64 round-off only
    # RHS scale: |div v| terms are O(umax/h) before cancellation (b ~ 1e-16 on the exact lattice)
    assert np.max(np.abs(bg - b)) < 1e-12 * max(np.abs(b).max(), pr.spec.umax / pr.spec.h)


@pytest.mark.parametrize("mode", [hip.PINZERO, hip.DOUBLEDIAG, hip.NOT_SINGULAR])
def test_gpu_assembly_singular_modes(gpu_ctx, mode):
    pr = Problem(tgv_spec(dim=2, n=12, mode=workload.JITTER), singular=mode)
    rp, ci, val, b = pr.poisson()
    A, bg = hip.assemble_poisson(gpu_ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                 np.ascontiguousarray(pr.parts["v"]), singular=mode, vfrac=pr.P.vfrac)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(ci2, ci)
    assert np.max(np.abs(v2 - val)) < 1e-12 * np.abs(val).max()
    assert np.max(np.abs(bg - b)) < 1e-12 * np.abs(b).max()


def test_gpu_assembly_merges_duplicate_images(gpu_ctx):
    pr = Problem(tgv_spec(dim=2, n=4, mode=workload.JITTER, brick=0))
    rp, ci, val, b = pr.poisson()
    A, bg = hip.assemble_poisson(gpu_ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                 np.ascontiguousarray(pr.parts["v"]), vfrac=pr.P.vfrac)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    assert np.max(np.abs(v2 - val)) < 1e-12 * np.abs(val).max()


SOLVES = [("none", 0), ("jacobi", 0)]


@pytest.mark.parametrize("case", CASES[:4])
@pytest.mark.parametrize("prec,bs", SOLVES)
def test_gmres_solve_matches_oracle(gpu_ctx, case, prec, bs):
    """Pressure vector parity: ||x_gpu - x_cpu|| / ||x_cpu|| <= 1e-6 with both at
    relative residual <= 1e-8; iteration counts within +-1;
    x.n = 0 to 1e-12."""
    pr = Problem(tgv_spec(**case))
    rp, ci, val, b = pr.poisson()
    xo, io, bo = orc.solve(rp, ci, val, b, singular=True, prec=prec)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, prec, 0)
    bg, xg = b.copy(), np.zeros(pr.n)
    info = hip.solve(gpu_ctx, A, bg, xg, prec=M, singular=True)
    assert info.converged == 1 and info.rel_res_implicit <= 1e-8
    assert abs(info.iters - io.iters) <= 1
    assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6
    assert abs(xg.sum()) / np.sqrt(pr.n) <= 1e-12 * np.linalg.norm(xg)
    assert np.allclose(bg, bo, rtol=0, atol=1e-14 * np.abs(bo).max())   # b projected in place like the reference
    assert abs(info.rel_res_explicit - io.rel_res_explicit) <= 1e-6 * max(io.rel_res_explicit, 1e-12) + 1e-12


def test_cg_solve_matches_oracle(gpu_ctx):
    pr = Problem(tgv_spec(dim=2, n=32, mode=workload.LATTICE))
    rp, ci, val, _ = pr.poisson()
    x = pr.parts["x"][:pr.n]
    b = np.cos(2 * x[:, 0]) + np.cos(2 * x[:, 1])
    prm_o = orc.SolverParams(solver_type=1, tol=1e-8)
    xo, io, _ = orc.solve(rp, ci, val, b, singular=True, prec="jacobi", params=prm_o)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "jacobi", 0)
    bg, xg = b.copy(), np.zeros(pr.n)
    info = hip.solve(gpu_ctx, A, bg, xg, prec=M, singular=True, params=hip.SolverParams(solver_type=1, tol=1e-8))
    assert info.converged == 1 and abs(info.iters - io.iters) <= 1
    assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6


def test_nonconvergence_is_reported_not_raised(gpu_ctx):
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    xg = np.zeros(pr.n)
    info = hip.solve(gpu_ctx, A, b.copy(), xg, singular=True, params=hip.SolverParams(max_iters=3))
    assert info.converged == 0 and info.iters == 3            # LAMMPS_SUCCESS, solver_lin_belos.h:194-221


def test_multi_rhs_and_restart(gpu_ctx):
    """nvec=3 column-major [lda x nvec] like the Helmholtz call (pair_isph.cpp:936-942),
    with a short restart length to exercise restarts."""
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER), singular=orc.NOT_SINGULAR)
    rp, ci, val, b = pr.poisson()
    val = val.copy()
    for i in range(pr.n):                      # make it Helmholtz-like: I + A
        val[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i] += 1.0
    rng = np.random.default_rng(3)
    B = np.asfortranarray(rng.standard_normal((pr.n, 3)))
    X = np.zeros_like(B, order="F")
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    prm = hip.SolverParams(num_blocks=5, max_iters=500, max_restarts=100)
    bflat, xflat = B.ravel(order="F").copy(), X.ravel(order="F").copy()
    info = hip.solve(gpu_ctx, A, bflat, xflat, params=prm, nvec=3, lda=pr.n)
    assert info.converged == 1 and info.restarts > 0
    for c in range(3):
        xo, io, _ = orc.solve(rp, ci, val, B[:, c], params=orc.SolverParams(num_blocks=5, max_iters=500, max_restarts=100))
        xc = xflat[c * pr.n:(c + 1) * pr.n]
        assert np.linalg.norm(xc - xo) / np.linalg.norm(xo) < 1e-6


def test_full_size_properties(gpu_ctx):
    """Size-independent properties at a size the oracle would not finish quickly:
    48^3 assembled and solved entirely on the GPU: row sums vanish, the solve
    reaches the tolerance, the solution is mean-free, residual re-checked on host."""
    import torch
    sp = tgv_spec(dim=3, n=48, mode=workload.ADVECT)
    p = workload.make_tgv(sp)
    colmap = workload.single_rank_colmap(p)
    vf = hip.compute_volumes(gpu_ctx, p, colmap)
    vfrac = np.zeros(p["nall"])
    vfrac[:p["nlocal"]] = vf
    vfrac[p["nlocal"]:] = vf[p["owner_index"][p["nlocal"]:]]
    A, b = hip.assemble_poisson(gpu_ctx, p, colmap, sp.dt, p["rho"], np.ascontiguousarray(p["v"]), vfrac=vfrac)
    n = p["nlocal"]
    ones = A.spmv(np.ones(n))
    rp, ci, v = A.export_csr()
    assert np.max(np.abs(ones)) < 1e-11 * np.abs(v).max()
    x = np.zeros(n)
    bb = b.copy()
    info = hip.solve(gpu_ctx, A, bb, x, singular=True)
    assert info.converged == 1
    r = bb - _csr(rp, ci, v, n) @ x
    r -= r.mean()
    assert np.linalg.norm(r) / np.linalg.norm(bb) < 2e-8
    assert abs(x.mean()) < 1e-12 * np.abs(x).max()


def test_config1_full_size_100cubed(gpu_ctx_bricks):
    """BASELINE configs[1] at its full size and in bench.py's own configuration: 3-D TGV, 100^3 = 1 M particles handed over
    in lexicographic atom order (create_atoms on the lattice), the library numbering the rows itself (its 10 x 10 x 5
    bricks = the block-Jacobi subdomains), FGMRES(50) + block ILU(0) rebuilt per solve.  Every entry of the exported
    matrix, b and the volumes against the oracle's own assembly of the whole system (pattern exact, values 1e-12).  Then,
    against the ORACLE on the same system (solver_lin_belos.h:130-222): the oracle is handed the library's permutation and subdomain table, factors and
    solves P A P^T (1-2 s on the host cores): iterations +-1, ||x_gpu - x_cpu|| / ||x_cpu|| <= 1e-6, the ILU factor of
    200 sampled subdomains <= 1e-10 with the pattern exact.  Kept from the earlier rounds, the size-independent properties:
    zero row sums, b orthogonal to the null vector after projection, x . n = 0, the residual re-computed on the host with
    an independent CSR product <= 2e-8, and the same solution from the Jacobi-preconditioned solve (two different Krylov
    paths agree to 1e-6)."""
    import order as oorder
    ctx = gpu_ctx_bricks
    sp = workload.TGVSpec(dim=3, ncell=(100, 100, 100), brick=(100, 100, 100), mode=workload.ADVECT)
    p = workload.make_tgv(sp)
    colmap = workload.single_rank_colmap(p)
    n = p["nlocal"]
    assert n == 10 ** 6
    vf = hip.compute_volumes(ctx, p, colmap)
    vfrac = np.ascontiguousarray(vf[p["owner_index"]])
    A, b = hip.assemble_poisson(ctx, p, colmap, sp.dt, p["rho"], np.ascontiguousarray(p["v"]), vfrac=vfrac)
    info_m = A.info()
    assert info_m["nrow"] == n and 100 < info_m["nnz"] / n < 108
    rp, ci, v = A.export_csr()                                          # the caller's numbering
    assert np.max(np.abs(A.spmv(np.ones(n)))) < 1e-11 * np.abs(v).max()
    # ---- every entry against the oracle's own assembly of the whole system (volumes included)
    t0 = time.perf_counter()
    P = orc.Particles(p, colmap)
    P.precompute(corrections=False)
    rpo, cio, vo, bo = P.poisson(sp.dt, p["rho"], np.ascontiguousarray(p["v"]))
    t_orc = time.perf_counter() - t0
    assert np.max(np.abs(vf - P.vfrac[:n]) / P.vfrac[:n]) < 1e-13
    assert np.array_equal(rp, rpo) and np.array_equal(ci, cio)          # pattern: exact
    dval = np.max(np.abs(v - vo)) / np.abs(vo).max()
    db = np.max(np.abs(b - bo)) / max(np.abs(bo).max(), sp.umax / sp.h)
    print("config1 AntiSymmetric, all %d rows: oracle %.1f s, max|dval|/max|val| %.3g, max|db|/scale %.3g" % (n, t_orc, dval, db))
    assert dval <= 1e-12 and db <= 1e-12
    del P, rpo, cio, vo, bo
    o = A.ordering()
    sizes = np.diff(o["block_ptr"])
    assert len(sizes) == 2000 and sizes.min() == sizes.max() == 500     # 10 x 10 x 5 bricks tile the lattice
    assert np.array_equal(o["perm"], oorder.order(p["x"][:n], o["geom"], o["faces"]))
    M = hip.Precond(ctx, A, "bjacobi-ilu0", 0)
    x, bb = np.zeros(n), b.copy()
    info = hip.solve(ctx, A, bb, x, prec=M, singular=True)
    assert info.converged == 1
    # ---- the oracle on the same system with the same subdomains
    rpi, cii, vi, bi = oorder.permute_system(rp, ci, v, b, o["perm"])
    ref = orc.ILU(rpi, cii, vi, 0, o["block_ptr"])
    xoi, io, _ = orc.solve(rpi, cii, vi, bi, singular=True, prec="ilu", ilu=ref)
    assert io.converged == 1 and abs(info.iters - io.iters) <= 1, (info.iters, io.iters)
    assert abs(info.iters - 71) <= 2, info.iters                        # the figure bench.py reports
    xo = np.empty(n)
    xo[o["perm"]] = xoi
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-6
    frp, fci, fv = ref.export()
    grp, gci, gv = M.export_ilu()                                       # the matrix' own numbering, like the oracle's copy
    assert np.array_equal(grp, frp)
    pick = np.sort(np.random.default_rng(4).choice(len(sizes), size=200, replace=False))
    for bk in pick:
        lo, hi = frp[o["block_ptr"][bk]], frp[o["block_ptr"][bk + 1]]
        assert np.array_equal(gci[lo:hi], fci[lo:hi]), bk
        fb = fv[lo:hi]
        assert np.max(np.abs(gv[lo:hi] - fb) / np.maximum(np.abs(fb), 1e-10 * np.abs(fb).max())) < 1e-10, bk
    M.close()
    # ---- size-independent properties
    assert abs(bb.sum()) < 1e-10 * np.abs(bb).sum()                     # b was projected in place
    assert abs(x.mean()) < 1e-12 * np.abs(x).max()
    Ah = _csr(rp, ci, v, n)
    r = bb - Ah @ x
    r -= r.mean()
    assert np.linalg.norm(r) / np.linalg.norm(bb) < 2e-8
    xj, bj = np.zeros(n), b.copy()
    ij = hip.solve(ctx, A, bj, xj, prec=hip.Precond(ctx, A, "jacobi", 0), singular=True)
    assert ij.converged == 1
    assert np.linalg.norm(x - xj) / np.linalg.norm(xj) < 1e-6
    A.close()


def test_config1_symmetric_rows_match_the_oracle_window(gpu_ctx_bricks):
    """configs[1] at 100^3 with the Symmetric (corrected) operator family, the whole chain on the device: volumes, G_i and
    L_i, then the Poisson rows and right-hand side, in the library's own row numbering.  At least 2^16 rows -- 1040 runs
    of 64 consecutive rows spread over the lattice plus the first and last 512 -- against the oracle's row window
    (tests/row_window.py), which assembles exactly those rows bit for bit as the whole system would.  Tolerances of the
    small Symmetric chain (test_gpu_corrections_match_oracle_and_feed_assembly): V 1e-13, G 1e-11, L 1e-9 (6x6 LU pivot
    order), values 1e-9 (they carry L); b 1e-12 of max(|b|, umax/h) (it carries G only)."""
    import row_window as rw
    ctx = gpu_ctx_bricks
    sp = workload.TGVSpec(dim=3, ncell=(100, 100, 100), brick=(100, 100, 100), mode=workload.ADVECT)
    p = workload.make_tgv(sp)
    colmap = workload.single_rank_colmap(p)
    n = p["nlocal"]
    own = p["owner_index"]
    vf = hip.compute_volumes(ctx, p, colmap)
    vfrac = np.ascontiguousarray(vf[own])
    G, L = hip.compute_corrections(ctx, p, colmap, vfrac)
    A, b = hip.assemble_poisson(ctx, p, colmap, sp.dt, p["rho"], np.ascontiguousarray(p["v"]), antisym=False, vfrac=vfrac,
                                Gc=np.ascontiguousarray(G[own]), Lc=np.ascontiguousarray(L[own]))
    rp, ci, v = A.export_csr()
    A.close()
    rows = np.unique(np.r_[rw.runs(n, 1040, 64, seed=1), np.arange(512), np.arange(n - 512, n)])
    assert len(rows) >= 2 ** 16
    t0 = time.perf_counter()
    win, P, (wrp, wci, wv, wb) = rw.poisson(p, colmap, rows, sp.dt, p["rho"], p["v"], antisym=False)
    t_orc = time.perf_counter() - t0
    k = win.nrows
    assert np.max(np.abs(vf[rows] - P.vfrac[:k]) / P.vfrac[:k]) < 1e-13
    assert np.max(np.abs(G[rows] - P.Gc[:k])) < 1e-11 * np.abs(P.Gc[:k]).max()
    assert np.max(np.abs(L[rows] - P.Lc[:k])) < 1e-9 * np.abs(P.Lc[:k]).max()
    skip = rows != 0                                                    # row 0: the first fluid row (rank0 edit)
    dev = rw.rows_of(rp, ci, v, rows[skip])
    dval = rw.assert_rows_match(dev, rw.rows_of(wrp, wci, wv, np.flatnonzero(skip)), 1e-9)
    db = np.max(np.abs(b[rows] - wb)[skip]) / max(np.abs(wb).max(), sp.umax / sp.h)
    print("config1 Symmetric, %d window rows (%d window particles): oracle %.1f s, max|dval|/max|val| %.3g, "
          "max|db|/scale %.3g" % (k, win.parts["nlocal"], t_orc, dval, db))
    assert db <= 1e-12


def test_neigh_ptr64_gives_the_same_system(gpu_ctx):
    """isph_particles::neigh_ptr64 (64-bit offsets of the flattened neighbour list, for lists beyond 2^31 entries)
    against the 32-bit neigh_ptr: volumes, correction tensors, Poisson matrix and right-hand side bit for bit."""
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER), antisym=False)
    p32 = pr.parts
    p64 = dict(p32)
    p64["neigh_ptr"] = p32["neigh_ptr"].astype(np.int64)
    out = []
    for p in (p32, p64):
        vf = hip.compute_volumes(gpu_ctx, p, pr.colmap)
        vfrac = np.ascontiguousarray(vf[p["owner_index"]])
        G, L = hip.compute_corrections(gpu_ctx, p, pr.colmap, vfrac)
        Gc = np.ascontiguousarray(G[p["owner_index"]]); Lc = np.ascontiguousarray(L[p["owner_index"]])
        A, b = hip.assemble_poisson(gpu_ctx, p, pr.colmap, pr.spec.dt, p["rho"], np.ascontiguousarray(p["v"]),
                                    antisym=False, vfrac=vfrac, Gc=Gc, Lc=Lc)
        g = hip.gradient(gpu_ctx, p, pr.colmap, np.cos(p["x"][:, 0]), vfrac, antisym=False, Gc=Gc)
        out.append((vf, G, L, A.export_csr(), b, g))
    for a32, a64 in zip(out[0], out[1]):
        if isinstance(a32, tuple):
            assert all(np.array_equal(u, w) for u, w in zip(a32, a64))
        else:
            assert np.array_equal(a32, a64)


def test_exact_lattice_ties_count_and_fill_agree(gpu_ctx):
    """Regression (round 2): on an exact lattice 30 neighbours of every particle sit EXACTLY on the cut radius
    (|(3,0,0)| = |(2,2,1)| = 3 dx = cut).  ROCm's __dmul_rn/__dadd_rn are plain operators, so the compiler fused
    x*x + s into an fma in the fill kernel but not in the counting kernel: rows got padding inside their counted
    length (the row's own column, several times), and above the 32 768-row duplicate-merge threshold the ILU level
    walk ran through uninitialised levels -> GPU memory fault.  r^2 now comes from one function with contraction off.
    64^3 lattice (n > 32768): every row has its own column exactly once, strictly ascending columns, the pattern is
    the one IEEE arithmetic without fma gives (numpy), ILU(0) builds and the solve converges."""
    sp = tgv_spec(dim=3, n=64, mode=workload.LATTICE)
    p = workload.make_tgv(sp)
    n = p["nlocal"]
    colmap = workload.single_rank_colmap(p)
    vf = hip.compute_volumes(gpu_ctx, p, colmap)
    vfrac = np.ascontiguousarray(vf[p["owner_index"]])
    v = np.zeros((p["nall"], 3))
    v[:, 0] = np.sin(p["x"][:, 1])
    A, b = hip.assemble_poisson(gpu_ctx, p, colmap, sp.dt, p["rho"], v, vfrac=vfrac)
    rp, ci, val = A.export_csr()
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.all(np.diff(ci)[np.diff(rows) == 0] > 0)                 # strictly ascending inside every row
    assert np.array_equal(np.bincount(rows[ci == rows], minlength=n), np.ones(n, dtype=np.int64))
    x, ptr, idx = p["x"], p["neigh_ptr"], p["neigh_idx"]
    io = np.repeat(np.arange(n), np.diff(ptr))
    d = x[io] - x[idx]
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]   # same order, no fma
    expect = np.bincount(io[r2 < float(p["cut"]) ** 2], minlength=n) + 1
    assert np.array_equal(np.diff(rp), expect) and expect.max() > 93   # ties are really there
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 512)
    xs = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), xs, prec=M, singular=True)
    assert info.converged == 1


# ---------------------------------------------------------------- block-Jacobi ILU(0)
ILU_CASES = [
    (dict(dim=2, n=16, mode=workload.JITTER, brick=8), 64),
    (dict(dim=2, n=33, mode=workload.ADVECT, brick=8), 256),      # ragged last block
    (dict(dim=3, n=12, mode=workload.JITTER, brick=4), 64),
    (dict(dim=3, n=16, mode=workload.ADVECT, brick=8), 512),
    (dict(dim=3, n=10, mode=workload.JITTER, kernel="quintic", cut_over_h=3.0, brick=5), 1024),  # one block, wide rows
    (dict(dim=2, n=16, mode=workload.LATTICE, brick=16), 256),    # row-major block: few rows per level (stream fallback)
]


@pytest.mark.parametrize("case,bs", ILU_CASES)
def test_ilu0_factor_and_apply_match_oracle(gpu_ctx, case, bs):
    pr = Problem(tgv_spec(**case))
    rp, ci, val, b = pr.poisson()
    n = pr.n
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    ref = orc.ILU(rp, ci, val, 0, bp)
    frp, fci, fv = ref.export()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs)
    grp, gci, gv = M.export_ilu()
    assert np.array_equal(grp, frp) and np.array_equal(gci, fci)            # factor pattern: exact
    assert np.max(np.abs(gv - fv) / np.maximum(np.abs(fv), 1e-300 + 1e-10 * np.abs(fv).max())) < 1e-10
    r = np.random.default_rng(5).standard_normal(n)
    z = M.apply(r)
    zo = ref.apply(r)
    assert np.linalg.norm(z - zo) / np.linalg.norm(zo) < 1e-11


@pytest.mark.parametrize("case,bs", ILU_CASES[:4])
def test_gmres_bjacobi_ilu0_matches_oracle(gpu_ctx, case, bs):
    pr = Problem(tgv_spec(**case))
    rp, ci, val, b = pr.poisson()
    n = pr.n
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    xo, io, bo = orc.solve(rp, ci, val, b, singular=True, prec="ilu", ilu=orc.ILU(rp, ci, val, 0, bp))
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs)
    bg, xg = b.copy(), np.zeros(n)
    info = hip.solve(gpu_ctx, A, bg, xg, prec=M, singular=True)
    assert info.converged == 1 and abs(info.iters - io.iters) <= 1
    assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6


ILUK_CASES = [(c, bs, k) for (c, bs) in ILU_CASES[:4] for k in (1, 2)] + [(ILU_CASES[2][0], 64, 3), (ILU_CASES[4][0], 1024, 1),
                                                                         (ILU_CASES[5][0], 256, 4)]


@pytest.mark.parametrize("case,bs,k", ILUK_CASES)
def test_iluk_pattern_factor_and_apply_match_oracle(gpu_ctx, case, bs, k):
    """"fact: level-of-fill" = k > 0 (precond_ifpack.h:35, the reference default is 1): the device symbolic phase (level
    sweeps) must give exactly the level-of-fill pattern of the sequential definition, the numeric factor its values."""
    pr = Problem(tgv_spec(**case))
    rp, ci, val, b = pr.poisson()
    n = pr.n
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    ref = orc.ILU(rp, ci, val, k, bp)
    frp, fci, fv = ref.export()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu%d" % k, bs)
    grp, gci, gv = M.export_ilu()
    assert np.array_equal(grp, frp) and np.array_equal(gci, fci)            # pattern with fill: exact
    assert grp[-1] > hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs).export_ilu()[0][-1] or bs == 64 and k == 0
    assert np.max(np.abs(gv - fv)) <= 1e-10 * np.abs(fv).max()
    r = np.random.default_rng(5).standard_normal(n)
    z = M.apply(r)
    zo = ref.apply(r)
    assert np.linalg.norm(z - zo) / np.linalg.norm(zo) < 1e-10


@pytest.mark.parametrize("k", [1, 2])
def test_gmres_bjacobi_iluk_matches_oracle(gpu_ctx, k):
    pr = Problem(tgv_spec(dim=3, n=16, mode=workload.ADVECT, brick=8))
    rp, ci, val, b = pr.poisson()
    n, bs = pr.n, 512
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    xo, io, bo = orc.solve(rp, ci, val, b, singular=True, prec="ilu", ilu=orc.ILU(rp, ci, val, k, bp))
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu%d" % k, bs)
    bg, xg = b.copy(), np.zeros(n)
    info = hip.solve(gpu_ctx, A, bg, xg, prec=M, singular=True)
    assert info.converged == 1 and abs(info.iters - io.iters) <= 1
    assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6


def test_iluk_rejects_levels_out_of_range(gpu_ctx):
    pr = Problem(tgv_spec(dim=2, n=16, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    with pytest.raises(hip.IsphError):
        hip.Precond(gpu_ctx, A, "bjacobi-ilu9", 64)


def test_ilu0_one_row_per_level_uses_the_safe_stream_capacity(gpu_ctx):
    """Tridiagonal chain: every level holds one row, so the triangular-solve stream needs one chunk per row and
    direction -- far above the first-attempt capacity; the build must fall back to its proven bound, not fail."""
    n, bs = 1200, 512
    rp = np.zeros(n + 1, np.int32)
    ci, val = [], []
    rng = np.random.default_rng(11)
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                ci.append(j)
                val.append(4.0 + rng.random() if j == i else -1.0 - rng.random())
        rp[i + 1] = len(ci)
    ci, val = np.asarray(ci, np.int32), np.asarray(val)
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    ref = orc.ILU(rp, ci, val, 0, bp)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs)
    frp, fci, fv = ref.export()
    grp, gci, gv = M.export_ilu()
    assert np.array_equal(grp, frp) and np.array_equal(gci, fci)
    assert np.max(np.abs(gv - fv)) < 1e-12
    r = rng.standard_normal(n)
    assert np.linalg.norm(M.apply(r) - ref.apply(r)) / np.linalg.norm(r) < 1e-12


def test_ilu_rejects_bad_block_size(gpu_ctx):
    pr = Problem(tgv_spec(dim=2, n=16, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    with pytest.raises(hip.IsphError):
        hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 100)


# ---------------------------------------------------------------- RCCL halo path on one GPU
def test_rccl_self_halo_spmv_and_solve(gpu_ctx):
    """The multi-GPU machinery (pack kernel -> ncclSend/ncclRecv -> ghost columns,
    ncclAllReduce of the dot products) exercised on a single GPU: the periodic
    images are routed through the halo plan as ghosts received from rank 0 itself.
    Must reproduce the folded single-rank operator."""
    from isph_amd import dist
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    ctx = hip.Context(0, rank=0, nranks=1, uid=hip.Context.unique_id())
    try:
        plan = dist.make_self_halo_plan(pr.parts)
        assert plan.ncol > pr.n
        A, bg = hip.assemble_poisson(ctx, pr.parts, plan.colmap, pr.spec.dt, pr.parts["rho"],
                                     np.ascontiguousarray(pr.parts["v"]), vfrac=pr.P.vfrac, ncol=plan.ncol)
        A.set_halo(plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        assert np.max(np.abs(bg - b)) < 1e-12 * np.abs(b).max()
        x = np.random.default_rng(7).standard_normal(pr.n)
        y = A.spmv(x)
        yo = orc.spmv(rp, ci, val, x)
        assert np.max(np.abs(y - yo)) < 1e-12 * np.abs(yo).max()
        M = hip.Precond(ctx, A, "bjacobi-ilu0", 256)
        xg = np.zeros(pr.n)
        info = hip.solve(ctx, A, bg.copy(), xg, prec=M, singular=True)
        bp = np.arange(0, pr.n + 256, 256).clip(0, pr.n).astype(np.int32)
        xo, io, _ = orc.solve(rp, ci, val, b, singular=True, prec="ilu", ilu=orc.ILU(rp, ci, val, 0, bp))
        assert info.converged == 1 and abs(info.iters - io.iters) <= 1
        assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6
    finally:
        ctx.close()


def test_rccl_forward_comm_of_per_atom_fields(gpu_ctx):
    """isph_halo_create / isph_halo_forward = comm->forward_comm_pair for the pair's per-atom arrays
    (pair_isph.cpp:1924-2110): scalars (Vfrac) and 3-vectors (Vstar) from host and from device memory, through the
    self-peer plan on one GPU.  Index work: ghost values must equal their owners' bit for bit."""
    import torch
    from isph_amd import dist
    pr = Problem(tgv_spec(dim=3, n=10, mode=workload.JITTER))
    ctx = hip.Context(0, rank=0, nranks=1, uid=hip.Context.unique_id())
    try:
        plan = dist.make_self_halo_plan(pr.parts)
        nl, nall = pr.parts["nlocal"], pr.parts["nall"]
        fwd = hip.HaloForward(ctx, nl, plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        assert fwd.nrecv == plan.ncol - nl
        own = pr.parts["owner_index"].astype(np.int64)
        rng = np.random.default_rng(3)
        s = rng.standard_normal(nl)
        v = rng.standard_normal((nl, 3))
        g = fwd.forward(s)
        assert np.array_equal(np.concatenate([s, g])[plan.colmap], s[own])          # every ghost holds its owner's value
        gv = fwd.forward(v, ncomp=3)
        assert np.array_equal(np.concatenate([v, gv])[plan.colmap], v[own])
        dev = torch.device("cuda", 0)
        gd = fwd.forward(torch.from_numpy(v).to(dev), ncomp=3)
        assert gd.is_cuda and np.array_equal(gd.cpu().numpy(), gv)
        full = dist.forward_scalar_rccl(fwd, plan, torch.from_numpy(s).to(dev))
        assert full.shape[0] == nall and np.array_equal(full.cpu().numpy(), s[own])
        with pytest.raises(hip.IsphError):
            hip.HaloForward(ctx, nl, plan.peers, plan.send_ptr, plan.send_idx + nl, plan.recv_ptr)   # send index out of range
        fwd.close()
        # a plan without peers is a no-op on any context
        f0 = hip.HaloForward(gpu_ctx, nl, [], [0], [], [0])
        assert f0.forward(s).shape == (0,)
    finally:
        ctx.close()


# ---------------------------------------------------------------- C++ mirror of the reference interface
@pytest.mark.parametrize("singular,cg", [(1, False), (0, True), (1, "ml"), (1, "ml-xml"), (1, "ifpack-defaults"), (1, "ifpack-reference"),
                                         (1, "recycling")])
def test_cpp_solver_lin_mirror(tmp_path, singular, cg):
    """SolverLin_Belos / PrecondWrapper_Ifpack (implicit-sph_amd/host/*.h) driven
    exactly like USER-REAXC-T/fix_qeq_reax.cpp:671-693 drives the reference."""
    import subprocess
    from isph_amd import build
    exe = build.build_cpp_test()
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER if singular else workload.LATTICE),
                 singular=orc.NULLSPACE if singular else orc.NOT_SINGULAR)
    rp, ci, val, b = pr.poisson()
    if not singular:                       # SPD system for the CG path: lattice matrix + I
        val = val.copy()
        for i in range(pr.n):
            val[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i] += 1.0
        b = np.cos(pr.parts["x"][:pr.n, 0]) + 0.3
    fin, fout = tmp_path / "sys.bin", tmp_path / "x.bin"
    with open(fin, "wb") as f:
        np.array([pr.n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f)
        val.tofile(f); b.tofile(f)
    ml = cg in ("ml", "ml-xml")
    ml_xml = cg == "ml-xml"
    mode = cg if isinstance(cg, str) else None
    fill = 1 if mode in ("ifpack-defaults", "ifpack-reference") else 0   # PrecondWrapper_Ifpack's own defaults: fill 1
    cg = bool(cg) and mode is None
    r = subprocess.run([exe, str(fin), str(fout), str(singular)] + (["cg"] if cg else [mode] if mode else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ">> Belos::Status - Passed!" in r.stdout
    out = np.fromfile(fout)
    x, bproj = out[:pr.n], out[pr.n:]
    bp = np.arange(0, pr.n + 256, 256).clip(0, pr.n).astype(np.int32)
    prm = orc.SolverParams(solver_type=1, tol=1e-8) if cg else orc.SolverParams()
    if ml:   # PrecondWrapper_ML mirror: setNullVector reaches the AMG through solveProblem (solver_lin_belos.h:149-151)
        # ("ml-xml": the keys of the benchmark protocol's ml.xml -- Gauss-Seidel, efficient symmetric, 4 sweeps, 10 levels asked)
        kw = dict(theta=0.0, sweeps=4, smoother=1, max_levels=8) if ml_xml else dict(theta=0.02)
        G = orc.AMG(rp, ci, val, nullvec=np.full(pr.n, 1.0 / np.sqrt(pr.n)), coarse_max=64, block=256, **kw)
        xo, io, bo = orc.solve(rp, ci, val, b, singular=True, prec="amg", amg=G, params=prm)
    elif mode == "ifpack-reference":   # "isph: block rows" = 0: ILU(1) of the whole matrix, the reference on one rank
        xo, io, bo = orc.solve(rp, ci, val, b, singular=True, prec="ilu", ilu=orc.ILU(rp, ci, val, 1), params=prm)
        assert "iters=%d" % io.iters in r.stdout or "iters=%d" % (io.iters + 1) in r.stdout or "iters=%d" % (io.iters - 1) in r.stdout
    elif mode == "recycling":          # "Solver Type" = "Recycling GMRES" -> GCRO-DR(20, 5) with block-Jacobi ILU(0)
        import gcrodr as gcro
        xo, ig = gcro.solve(rp, ci, val, b, singular=True, prec=orc.ILU(rp, ci, val, 0, bp).apply, num_blocks=20, num_recycled=5)
        bo = b - b.mean()
        assert ig["converged"]
    else:
        xo, io, bo = orc.solve(rp, ci, val, b, singular=bool(singular), prec="ilu",
                               ilu=orc.ILU(rp, ci, val, fill, bp), params=prm)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-6
    assert np.allclose(bproj, bo, rtol=0, atol=1e-13 * np.abs(bo).max())   # b view updated in place


def test_cpp_solver_lin_mirror_with_halo(tmp_path):
    """The N > 1 code path of the C++ surface on one GPU: the matrix handed to SolverLin_Belos carries ghost columns
    and an Epetra_Import (periodic images routed as ghosts received from this very rank), so solveProblem goes through
    isph_comm_unique_id -> isph_ctx_create_dist -> isph_mat_set_halo and the overlapped RCCL exchange.  Must give the
    folded single-rank solution."""
    import subprocess
    from isph_amd import build, dist
    exe = build.build_cpp_test()
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    plan = dist.make_self_halo_plan(pr.parts)
    # the same system with the images as ghost columns: oracle graph over the plan's column map
    Ph = orc.Particles(pr.parts, plan.colmap)
    Ph.precompute(corrections=False)
    rph, cih, valh, bh = Ph.poisson(pr.spec.dt, pr.parts["rho"], pr.parts["v"], singular=orc.NULLSPACE)
    assert cih.max() >= pr.n and np.allclose(bh, b, rtol=0, atol=1e-13 * np.abs(b).max())
    fin, fout = tmp_path / "sys.bin", tmp_path / "x.bin"
    with open(fin, "wb") as f:
        np.array([pr.n, plan.ncol, len(valh)], np.int32).tofile(f)
        rph.astype(np.int32).tofile(f); cih.astype(np.int32).tofile(f); valh.tofile(f); bh.tofile(f)
        np.array([len(plan.send_idx)], np.int32).tofile(f)
        plan.send_idx.astype(np.int32).tofile(f)
    r = subprocess.run([exe, str(fin), str(fout), "1", "selfhalo"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    x = np.fromfile(fout)
    bp = np.arange(0, pr.n + 256, 256).clip(0, pr.n).astype(np.int32)
    xo, io, _ = orc.solve(rp, ci, val, b, singular=True, prec="ilu", ilu=orc.ILU(rp, ci, val, 0, bp))
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-6


def test_cpp_ifpack_overlap_level_one_through_the_importer(tmp_path):
    """PrecondWrapper_Ifpack with "isph: block rows" = 0 and the reference's default "Overlap Level" 1 on a matrix that
    carries an Epetra_Import (precond_ifpack.h:43,60-74): the adapter imports the rows of the ghost columns
    (host/halo_lists.h) and factors the extended subdomain (isph_prec_create_overlap).  Same iteration count and solution
    as the Python plumbing of the same preconditioner (dist.extend_rows + hip.PrecondOverlap, pinned against the oracle in
    tests/test_gpu_schwarz.py)."""
    import subprocess
    from isph_amd import build, dist
    exe = build.build_cpp_test()
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    plan = dist.make_self_halo_plan(pr.parts)
    Ph = orc.Particles(pr.parts, plan.colmap)
    Ph.precompute(corrections=False)
    rph, cih, valh, bh = Ph.poisson(pr.spec.dt, pr.parts["rho"], pr.parts["v"], singular=orc.NULLSPACE)
    fin, fout = tmp_path / "sys.bin", tmp_path / "x.bin"
    with open(fin, "wb") as f:
        np.array([pr.n, plan.ncol, len(valh)], np.int32).tofile(f)
        rph.astype(np.int32).tofile(f); cih.astype(np.int32).tofile(f); valh.tofile(f); bh.tofile(f)
        np.array([len(plan.send_idx)], np.int32).tofile(f)
        plan.send_idx.astype(np.int32).tofile(f)
    r = subprocess.run([exe, str(fin), str(fout), "1", "selfhalo-overlap"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    x = np.fromfile(fout)
    it_cpp = int(r.stdout.split("iters=")[1].split()[0])
    ctx = hip.Context(0, rank=0, nranks=1, uid=hip.Context.unique_id())
    try:
        A = hip.Matrix.from_csr(ctx, rph.astype(np.int32), cih.astype(np.int32), valh, ncol=plan.ncol)
        A.set_halo(plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        rpe, cie, ve = dist.extend_rows(plan, rph, cih, valh, None)
        Aext = hip.Matrix.from_csr(ctx, rpe, cie, ve)
        M = hip.PrecondOverlap(ctx, Aext, plan, level_of_fill=0, combine="add")
        xp = np.zeros(pr.n)
        info = hip.solve(ctx, A, bh.copy(), xp, prec=M, singular=True)
    finally:
        ctx.close()
    assert info.converged == 1 and abs(info.iters - it_cpp) <= 1, (info.iters, it_cpp)
    xo, io, _ = orc.solve(rp, ci, val, b, singular=True, prec="none")
    assert it_cpp < io.iters
    assert np.linalg.norm(x - xp) <= 1e-6 * np.linalg.norm(xp)
    assert np.linalg.norm(x - xo) <= 1e-6 * np.linalg.norm(xo)


# ---------------------------------------------------------------- Helmholtz builder
@pytest.mark.parametrize("case", [dict(dim=2, n=20, mode=workload.JITTER), dict(dim=3, n=12, mode=workload.ADVECT),
                                  dict(dim=2, n=4, mode=workload.JITTER, brick=0)])
@pytest.mark.parametrize("antisym", [True, False])
@pytest.mark.parametrize("theta", [0.0, 0.5, 1.0])
def test_gpu_helmholtz_matches_oracle(gpu_ctx_both, case, antisym, theta):
    gpu_ctx = gpu_ctx_both
    pr = Problem(tgv_spec(**case), antisym=antisym)
    p = pr.parts
    x, nall = p["x"], p["nall"]
    rng = np.random.default_rng(11)
    pres = np.cos(x[:, 0]) * np.sin(x[:, 1])
    force = np.ascontiguousarray(0.01 * np.stack([np.sin(x[:, 1]), np.cos(x[:, 0]), np.zeros(nall)], axis=1))
    nu = p["nu"] * (1.0 + 0.1 * np.sin(x[:, 0]))            # variable viscosity exercises grad(m)
    g = np.array([0.05, -0.02, 0.01 if pr.spec.dim == 3 else 0.0])
    vel = np.ascontiguousarray(p["v"])
    rp, ci, val, b = pr.P.helmholtz(pr.spec.dt, theta, nu, p["rho"], pres, force, g, vel, antisym=antisym)
    A, bg = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, theta, nu, p["rho"], pres, force, g, vel,
                                   antisym=antisym, vfrac=pr.P.vfrac, Gc=None if antisym else pr.P.Gc,
                                   Lc=None if antisym else pr.P.Lc, kernel=pr.spec.kernel)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    assert np.max(np.abs(v2 - val)) < 1e-12 * max(np.abs(val).max(), 1.0)
    bo = b.ravel()                                            # oracle b is [dim][nlocal] == column-major flattened
    assert np.max(np.abs(bg - bo)) < 1e-12 * np.abs(bo).max()
    # right-hand side only (theta = 0 callers): same b, no matrix
    A0, b0 = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, theta, nu, p["rho"], pres, force, g, vel,
                                    antisym=antisym, vfrac=pr.P.vfrac, Gc=None if antisym else pr.P.Gc,
                                    Lc=None if antisym else pr.P.Lc, kernel=pr.spec.kernel, rhs_only=True)
    assert A0 is None and np.max(np.abs(b0 - bg)) <= 1e-13 * np.abs(bg).max()   # unsorted neighbour sums: round-off only


def test_helmholtz_solve_three_rhs(gpu_ctx_both):
    gpu_ctx = gpu_ctx_both
    """computeHelmholtz + solveProblem("Helmholtz") with x0 = v^n (pair_isph.cpp:932-971), theta = 0.5."""
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    p = pr.parts
    nall, n = p["nall"], pr.n
    zeros = np.zeros(nall)
    vel = np.ascontiguousarray(p["v"])
    A, bg = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, 0.5, p["nu"], p["rho"], zeros,
                                   np.zeros((nall, 3)), np.zeros(3), vel, vfrac=pr.P.vfrac)
    rp, ci, val, b = pr.P.helmholtz(pr.spec.dt, 0.5, p["nu"], p["rho"], zeros, np.zeros((nall, 3)), np.zeros(3), vel)
    xg = np.ascontiguousarray(vel[:n].T).ravel().copy()       # initial guess = v^n, column-major
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 256)
    info = hip.solve(gpu_ctx, A, bg.copy(), xg, prec=M, nvec=3, lda=n)
    assert info.converged == 1
    bp = np.arange(0, n + 256, 256).clip(0, n).astype(np.int32)
    for k in range(3):
        xo, io, _ = orc.solve(rp, ci, val, b[k], x0=vel[:n, k], prec="ilu", ilu=orc.ILU(rp, ci, val, 0, bp))
        nrm = max(np.linalg.norm(xo), 1e-30)
        assert np.linalg.norm(xg[k * n:(k + 1) * n] - xo) / nrm <= 1e-6 or np.linalg.norm(xo) < 1e-12


@pytest.mark.parametrize("prec", ["bjacobi-ilu0", "jacobi", "sa-amg"])
@pytest.mark.parametrize("restart", [50, 4])
def test_lockstep_right_hand_sides_equal_one_solve_after_the_other(gpu_ctx, prec, restart):
    """nvec > 1 on a non-singular system advances the Krylov spaces together (one matrix sweep for all operator
    applications of an iteration).  Belos solves the right-hand sides one after the other;
    every vector must come out with the bits of its own separate solve, iterations and restarts included."""
    pr = Problem(tgv_spec(dim=3, n=14, mode=workload.JITTER))
    p = pr.parts
    nall, n = p["nall"], pr.n
    zeros = np.zeros(nall)
    vel = np.ascontiguousarray(p["v"])
    A, bg = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, 0.5, p["nu"], p["rho"], zeros,
                                   np.zeros((nall, 3)), np.zeros(3), vel, vfrac=pr.P.vfrac)
    bg[2 * n:3 * n] = np.sin(np.arange(n))                                 # w = 0 in the 2-D vortex: give it a right-hand side
    M = hip.PrecondAMG(gpu_ctx, A) if prec == "sa-amg" else hip.Precond(gpu_ctx, A, prec, 256)
    prm = hip.SolverParams(num_blocks=restart, max_restarts=40)
    x3 = np.ascontiguousarray(vel[:n].T).ravel().copy()
    i3 = hip.solve(gpu_ctx, A, bg.copy(), x3, prec=M, nvec=3, lda=n, params=prm)
    its, rst = 0, 0
    for k in range(3):
        xk = vel[:n, k].copy()
        ik = hip.solve(gpu_ctx, A, bg[k * n:(k + 1) * n].copy(), xk, prec=M, params=prm)
        assert ik.converged == 1
        assert np.array_equal(xk, x3[k * n:(k + 1) * n])
        its += ik.iters
        rst += ik.restarts
    assert i3.converged == 1 and i3.iters == its and i3.restarts == rst
    if restart == 4 and prec != "sa-amg":
        assert rst > 0                                                     # the restart path of a single system was taken


# ---------------------------------------------------------------- solid particles + MorrisHolmes mirror
from problems import wall_types, fake_pnd  # noqa: E402


@pytest.mark.parametrize("dim,n", [(2, 20), (3, 12)])
@pytest.mark.parametrize("antisym", [True, False])
@pytest.mark.parametrize("singular", [orc.NOT_SINGULAR, orc.NULLSPACE])
@pytest.mark.parametrize("morris", [False, True])
def test_gpu_poisson_with_solid_wall(gpu_ctx, dim, n, antisym, singular, morris):
    pr = Problem(tgv_spec(dim=dim, n=n, mode=workload.JITTER), antisym=antisym, singular=singular,
                 kinds=[orc.FLUID, orc.SOLID], types=wall_types, pnd=fake_pnd if morris else None)
    assert (pr.parts["type"][:pr.n] == 2).sum() > 0
    rp, ci, val, b = pr.poisson()
    A, bg = hip.assemble_poisson(gpu_ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                 np.ascontiguousarray(pr.parts["v"]), antisym=antisym, singular=singular,
                                 vfrac=pr.P.vfrac, kinds=[orc.FLUID, orc.SOLID], pnd=pr.pnd,
                                 Gc=None if antisym else pr.P.Gc, Lc=None if antisym else pr.P.Lc)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    assert np.max(np.abs(v2 - val)) < 1e-12 * np.abs(val).max()
    assert np.max(np.abs(bg - b)) < 1e-12 * np.abs(b).max()
    solid = pr.parts["type"][:pr.n] == 2
    d = sps.csr_matrix((v2, ci2, rp2)).diagonal()
    assert np.all(d[solid] == 1.0) and np.all(bg[solid] == 0.0)          # functor_incomp_navier_stokes_poisson.h:137-147
    if singular == orc.NULLSPACE:
        # null-space mask = non-solid particles (pair_isph.cpp:996-1005); GMRES + block-ILU(0) vs oracle
        mask = (~solid).astype(np.int32)
        bs = 256
        bp = np.arange(0, pr.n + bs, bs).clip(0, pr.n).astype(np.int32)
        xo, io, _ = orc.solve(rp, ci, val, b, singular=True, null_mask=mask, prec="ilu", ilu=orc.ILU(rp, ci, val, 0, bp))
        M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs)
        xg = np.zeros(pr.n)
        info = hip.solve(gpu_ctx, A, bg.copy(), xg, prec=M, singular=True, null_mask=mask)
        assert info.converged == 1 and abs(info.iters - io.iters) <= 1
        assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6


@pytest.mark.parametrize("morris", [False, True])
@pytest.mark.parametrize("antisym", [True, False])
def test_gpu_helmholtz_with_solid_wall(gpu_ctx, morris, antisym):
    pr = Problem(tgv_spec(dim=2, n=20, mode=workload.JITTER), antisym=antisym, kinds=[orc.FLUID, orc.SOLID],
                 types=wall_types, pnd=fake_pnd if morris else None)
    p = pr.parts
    nall = p["nall"]
    pres = np.cos(p["x"][:, 0])
    force = np.zeros((nall, 3))
    g = np.array([0.0, -0.1, 0.0])
    vel = np.ascontiguousarray(p["v"])
    rp, ci, val, b = pr.P.helmholtz(pr.spec.dt, 0.5, p["nu"], p["rho"], pres, force, g, vel, antisym=antisym,
                                    morris=int(morris))
    A, bg = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, 0.5, p["nu"], p["rho"], pres, force, g, vel,
                                   antisym=antisym, vfrac=pr.P.vfrac, kinds=[orc.FLUID, orc.SOLID], pnd=pr.pnd,
                                   Gc=None if antisym else pr.P.Gc, Lc=None if antisym else pr.P.Lc)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(ci2, ci)
    assert np.max(np.abs(v2 - val)) < 1e-12 * np.abs(val).max()
    assert np.max(np.abs(bg - b.ravel())) < 1e-12 * np.abs(b).max()


# ---------------------------------------------------------------- computePre tensors on the GPU
@pytest.mark.parametrize("case", [dict(dim=2, n=20, mode=workload.JITTER), dict(dim=3, n=12, mode=workload.JITTER),
                                  dict(dim=3, n=10, mode=workload.ADVECT, kernel="quintic", cut_over_h=3.0)])
def test_gpu_corrections_match_oracle_and_feed_assembly(gpu_ctx, case):
    pr = Problem(tgv_spec(**case), antisym=False)
    n = pr.n
    G, Lc = hip.compute_corrections(gpu_ctx, pr.parts, pr.colmap, pr.P.vfrac, kernel=pr.spec.kernel)
    Go, Lo = pr.P.Gc[:n], pr.P.Lc[:n]
    assert np.max(np.abs(G - Go)) < 1e-11 * np.abs(Go).max()
    assert np.max(np.abs(Lc - Lo)) < 1e-9 * np.abs(Lo).max()            # 6x6 LU: pivot order may differ in ties
    # whole Symmetric-family pipeline on the device: volumes -> G,L -> Poisson rows
    Gf = np.zeros_like(pr.P.Gc); Gf[:n] = G
    Lf = np.zeros_like(pr.P.Lc); Lf[:n] = Lc
    rp, ci, val, b = pr.poisson()
    A, bg = hip.assemble_poisson(gpu_ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                 np.ascontiguousarray(pr.parts["v"]), antisym=False, vfrac=pr.P.vfrac, Gc=Gf, Lc=Lf,
                                 kernel=pr.spec.kernel)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(ci2, ci) and np.max(np.abs(v2 - val)) < 1e-9 * np.abs(val).max()


# ---------------------------------------------------------------- device-pointer ingress (on_device = 1)
def test_device_pointer_paths(gpu_ctx):
    """The same calls with HBM-resident operands (torch CUDA tensors passed as raw pointers):
    CSR ingress, SpMV, preconditioner apply, solve -- identical results to the host-pointer path."""
    import torch
    dev = torch.device("cuda", 0)
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ah = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    Ad = hip.Matrix.from_csr(gpu_ctx, t(rp), t(ci), t(val))
    gpu_ctx.sync()
    for x, y in zip(Ah.export_csr(), Ad.export_csr()):
        assert np.array_equal(x, y)
    xr = np.random.default_rng(3).standard_normal(pr.n)
    yd = Ad.spmv(t(xr))
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), Ah.spmv(xr))              # same kernel, same order: bitwise
    M = hip.Precond(gpu_ctx, Ad, "bjacobi-ilu0", 128)
    zd = M.apply(t(xr))
    torch.cuda.synchronize()
    assert np.array_equal(zd.cpu().numpy(), M.apply(xr))
    bd, xd = t(b), torch.zeros(pr.n, dtype=torch.float64, device=dev)
    info_d = hip.solve(gpu_ctx, Ad, bd, xd, prec=M, singular=True)
    bh, xh = b.copy(), np.zeros(pr.n)
    info_h = hip.solve(gpu_ctx, Ah, bh, xh, prec=M, singular=True)
    assert info_d.iters == info_h.iters and info_d.converged == 1
    assert np.array_equal(xd.cpu().numpy(), xh) and np.array_equal(bd.cpu().numpy(), bh)   # deterministic reductions
    with pytest.raises(ValueError):
        hip.solve(gpu_ctx, Ad, bd, xh, prec=M, singular=True)          # mixing host and device operands is refused


# ---------------------------------------------------------------- wall Neumann rows
from problems import wall_normals  # noqa: E402


@pytest.mark.parametrize("dim,n", [(2, 20), (3, 12)])
@pytest.mark.parametrize("antisym", [True, False])
@pytest.mark.parametrize("snd", [1.0, 0.0])
def test_gpu_poisson_wall_neumann_rows(gpu_ctx, dim, n, antisym, snd):
    """Solid rows with a wall normal carry -dt n.grad (functor_gradient_dot_operator_matrix.h); their diagonal is
    the state A.diagonal was left in (solid_normal_diag), solids without a normal get a unit row."""
    pr = Problem(tgv_spec(dim=dim, n=n, mode=workload.JITTER), antisym=antisym, singular=orc.NULLSPACE,
                 kinds=[orc.FLUID, orc.SOLID], types=wall_types, normal=wall_normals, solid_normal_diag=snd)
    solid = pr.parts["type"][:pr.n] == 2
    withn = np.abs(pr.normal[:pr.n]).sum(axis=1) > 0.5
    assert (solid & withn).sum() > 0 and (solid & ~withn).sum() > 0
    rp, ci, val, b = pr.poisson()
    A, bg = hip.assemble_poisson(gpu_ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                 np.ascontiguousarray(pr.parts["v"]), antisym=antisym, singular=orc.NULLSPACE,
                                 vfrac=pr.P.vfrac, kinds=[orc.FLUID, orc.SOLID], Gc=pr.P.Gc,
                                 Lc=None if antisym else pr.P.Lc, normal=pr.normal, solid_normal_diag=snd)
    rp2, ci2, v2 = A.export_csr()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    assert np.max(np.abs(v2 - val)) < 1e-12 * np.abs(val).max()
    assert np.max(np.abs(bg - b)) < 1e-12 * np.abs(b).max()
    M = sps.csr_matrix((v2, ci2, rp2))
    d = M.diagonal()
    assert np.all(d[solid & withn] == snd) and np.all(d[solid & ~withn] == 1.0)
    offdiag = np.abs(M - sps.diags(d)).sum(axis=1).A1
    assert np.all(offdiag[solid & withn] > 0) and np.all(offdiag[solid & ~withn] == 0)


# ---------------------------------------------------------------- BASELINE configs[0]: 2-D TGV 128^2, CG + ILU(0)
def test_baseline_config0_2d_tgv_cg_ilu0(gpu_ctx):
    """BASELINE.json configs[0]: 2-D Taylor-Green vortex (fix_isph_tgv lattice, origin 0.5), ~16k particles,
    Wendland, CG + ILU(0) (the USER-REAXC-T defaults: Block CG, tol 1e-6,
    USER-REAXC-T/solver_lin_belos.h:236-245, precond_ifpack.h:35).  Exact lattice => the
    momentum-preserving operator is symmetric, so CG applies; one ILU(0) subdomain of 1024 rows per block."""
    pr = Problem(tgv_spec(dim=2, n=128, mode=workload.LATTICE, brick=8))
    assert pr.n == 16384
    rp, ci, val, _ = pr.poisson()
    A0 = _csr(rp, ci, val, pr.n)
    assert abs(A0 - A0.T).max() < 1e-12 * abs(A0).max()
    x = pr.parts["x"][:pr.n]
    b = -0.5 * (np.cos(2 * x[:, 0]) + np.cos(2 * x[:, 1]))          # TGV pressure source shape (the lattice RHS itself is ~1e-16)
    bs = 1024
    bp = np.arange(0, pr.n + bs, bs).clip(0, pr.n).astype(np.int32)
    prm_o = orc.SolverParams(solver_type=1, tol=1e-6)
    xo, io, bo = orc.solve(rp, ci, val, b, singular=True, prec="ilu", ilu=orc.ILU(rp, ci, val, 0, bp), params=prm_o)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs)
    bg, xg = b.copy(), np.zeros(pr.n)
    info = hip.solve(gpu_ctx, A, bg, xg, prec=M, singular=True, params=hip.SolverParams(solver_type=1, tol=1e-6))
    assert io.converged and info.converged == 1 and abs(info.iters - io.iters) <= 1
    # both stop at 1e-6 relative residual: the solutions agree to that level times the conditioning of the
    # restricted operator; in practice far better because the iterations track each other
    assert np.linalg.norm(xg - xo) / np.linalg.norm(xo) <= 1e-6
    r = bg - A0 @ xg
    r -= r.mean()
    assert np.linalg.norm(r) / np.linalg.norm(bg) <= 2e-6


# ---------------------------------------------------------------- streaming operators
@pytest.mark.parametrize("dim,kernel", [(2, "wendland"), (3, "wendland"), (3, "quintic")])
@pytest.mark.parametrize("antisym", [True, False])
@pytest.mark.parametrize("filt", [None, (orc.FLUID, orc.FLUID), (orc.FLUID, orc.ALL)])
def test_gradient_and_divergence_match_oracle(gpu_ctx, dim, kernel, antisym, filt):
    """functor_gradient.h / functor_divergence.h incl. the type filters, on a domain with a solid slab."""
    n = 20 if dim == 2 else 10
    pr = Problem(tgv_spec(dim=dim, n=n, mode=workload.JITTER, kernel=kernel), antisym=antisym,
                 kinds=[orc.FLUID, orc.SOLID], types=wall_types)
    parts, P = pr.parts, pr.P
    nall = parts["nall"]
    rng = np.random.default_rng(3)
    own = parts["owner_index"]
    f = rng.standard_normal(parts["nlocal"])[own]
    u = rng.standard_normal((parts["nlocal"], 3))[own]
    if dim == 2:
        u[:, 2] = 0.0
    Gc = None if antisym else P.Gc
    kw = dict(antisym=antisym, alpha=0.7, filt=filt, Gc=Gc, kernel=kernel, kinds=[orc.FLUID, orc.SOLID])
    g = hip.gradient(gpu_ctx, parts, pr.colmap, f, P.vfrac, **kw)
    go = P.gradient(f, antisym, alpha=0.7, filt=filt)
    assert np.max(np.abs(g - go)) <= 1e-12 * np.abs(go).max()
    d = hip.divergence(gpu_ctx, parts, pr.colmap, u, P.vfrac, **kw)
    do = P.divergence(u, antisym, alpha=0.7, filt=filt)
    assert np.max(np.abs(d - do)) <= 1e-12 * np.abs(do).max()
    assert nall == len(f)


@pytest.mark.parametrize("antisym", [True, False])
@pytest.mark.parametrize("incremental", [True, False])
def test_correct_velocity_pressure_and_advance_match_oracle_formulas(gpu_ctx, antisym, incremental):
    """functor_correct_velocity.h, functor_correct_pressure.h, functor_advance_time_{begin,end}.h."""
    pr = Problem(tgv_spec(dim=3, n=10, mode=workload.JITTER), antisym=antisym)
    parts, P = pr.parts, pr.P
    n, own = parts["nlocal"], parts["owner_index"]
    rng = np.random.default_rng(9)
    dt = 0.013
    rho = (1.0 + 0.2 * rng.random(n))[own]
    dp = rng.standard_normal(n)[own]
    vstar = rng.standard_normal((n, 3))[own]
    p = rng.standard_normal(n)[own]
    v = rng.standard_normal((n, 3))[own]
    Gc = None if antisym else P.Gc
    filt = (orc.FLUID, orc.FLUID)
    gdp = P.gradient(dp, antisym, filt=filt)
    vs_ref = vstar[:n] - dt / rho[:n, None] * gdp
    p_ref = p + dp if incremental else dp.copy()       # over nlocal + nghost (pair_isph_corrected.cpp:1046)
    vs_g, p_g = np.ascontiguousarray(vstar.copy()), p.copy()
    hip.correct_velocity_pressure(gpu_ctx, parts, pr.colmap, dt, rho, dp, vs_g, p_g, P.vfrac, antisym=antisym,
                                  incremental=incremental, Gc=Gc)
    assert np.max(np.abs(vs_g[:n] - vs_ref)) <= 1e-12 * np.abs(vs_ref).max()
    assert np.array_equal(p_g, p_ref)
    assert np.array_equal(vs_g[n:], vstar[n:])          # ghost velocities wait for the next forward comm
    # advance
    dxp = 0.5 * dt * (vstar[:n] + v[:n])
    dpa_ref = np.sum(P.gradient(p, antisym, filt=filt) * dxp, axis=1)
    dpa = hip.advance_begin(gpu_ctx, parts, pr.colmap, dt, p, v, vstar, P.vfrac, antisym=antisym, Gc=Gc)
    assert np.max(np.abs(dpa - dpa_ref)) <= 1e-12 * np.abs(dpa_ref).max()
    x_g = np.ascontiguousarray(parts["x"][:n].copy())
    v_g, pp = np.ascontiguousarray(v[:n].copy()), p[:n].copy()
    hip.advance_end(gpu_ctx, n, 3, dt, dpa, np.ascontiguousarray(vstar[:n]), pp, x_g, v_g)
    assert np.max(np.abs(x_g - (parts["x"][:n] + dxp))) < 1e-14
    assert np.array_equal(v_g, vstar[:n]) and np.max(np.abs(pp - (p[:n] + dpa))) < 1e-14


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("antisym", [True, False])
def test_particle_shifting_matches_oracle(gpu_ctx, dim, antisym):
    """functor_compute_shift.h / functor_apply_shift.h / PairISPH_Corrected::shiftParticles with a solid slab
    (non-fluid weight) and a shift cut-off shorter than the kernel support."""
    n = 20 if dim == 2 else 10
    kinds = [orc.FLUID, orc.SOLID]
    pr = Problem(tgv_spec(dim=dim, n=n, mode=workload.JITTER), antisym=antisym, kinds=kinds, types=wall_types)
    parts, P = pr.parts, pr.P
    nl, own = parts["nlocal"], parts["owner_index"]
    rng = np.random.default_rng(21)
    v = np.ascontiguousarray(parts["v"][:nl][own])
    p = rng.standard_normal(nl)[own]
    shift, weight, dt = 0.05, 0.7, pr.spec.dt
    shiftcut = 0.8 * parts["cut"]
    fluid = parts["type"][:nl] == 1
    vmax_ref = np.sqrt((v[:nl][fluid] ** 2).sum(axis=1)).max()
    alpha = shift * dt * vmax_ref
    dr_o = P.compute_shift(alpha, shiftcut, weight)
    dr_g = hip.compute_shift(gpu_ctx, parts, pr.colmap, alpha, shiftcut, weight, kinds=kinds)
    assert np.abs(dr_o).max() > 0 and not dr_o[~fluid].any()
    assert np.max(np.abs(dr_g - dr_o)) <= 1e-12 * np.abs(dr_o).max()
    Gc = None if antisym else P.Gc
    fixed = np.array([0, 0, 1], np.int32)
    xo, vo, po = P.apply_shift(antisym, dr_o, v, p, fixed=fixed, sequential=False)
    xg, vg, pg = np.ascontiguousarray(parts["x"].copy()), v.copy(), p.copy()
    hip.apply_shift(gpu_ctx, parts, pr.colmap, dr_o, xg, vg, pg, P.vfrac, antisym=antisym, fixed=fixed, Gc=Gc, kinds=kinds)
    assert np.max(np.abs(xg - xo)) < 1e-14
    assert np.max(np.abs(vg - vo)) <= 1e-12 * np.abs(vo).max()
    assert np.max(np.abs(pg - po)) <= 1e-12 * np.abs(po).max()
    assert np.array_equal(xg[nl:], parts["x"][nl:]) and np.array_equal(pg[nl:], p[nl:])   # ghosts wait for the comm
    # whole shiftParticles(): vmax on the device, then compute + apply
    x2, v2, p2 = np.ascontiguousarray(parts["x"].copy()), v.copy(), p.copy()
    vmax = hip.shift_particles(gpu_ctx, parts, pr.colmap, shift, shiftcut, weight, dt, x2, v2, p2, P.vfrac, antisym=antisym,
                               fixed=fixed, Gc=Gc, kinds=kinds)
    assert vmax == vmax_ref
    assert np.max(np.abs(x2 - xo)) < 1e-13 and np.max(np.abs(p2 - po)) <= 1e-11 * np.abs(po).max()
    assert np.max(np.abs(v2 - vo)) <= 1e-11 * np.abs(vo).max()


# ---------------------------------------------------------------- small / degenerate inputs
@pytest.mark.parametrize("prec", ["none", "jacobi", "bjacobi-ilu0", "bjacobi-ilu2", "sa-amg"])
def test_tiny_systems_with_every_preconditioner(gpu_ctx, prec):
    """3x3 and 1x1 SPD systems: single block, single level, rows shorter than a wave."""
    for dense in (np.array([[4.0, -1.0, 0.0], [-1.0, 4.0, -1.0], [0.0, -1.0, 3.0]]), np.array([[2.5]])):
        S = sps.csr_matrix(dense)
        S.sort_indices()
        n = S.shape[0]
        A = hip.Matrix.from_csr(gpu_ctx, S.indptr, S.indices, S.data)
        M = hip.PrecondAMG(gpu_ctx, A) if prec == "sa-amg" else hip.Precond(gpu_ctx, A, prec, 64)
        b = np.arange(1.0, n + 1.0)
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M)
        assert info.converged == 1
        assert np.allclose(x, np.linalg.solve(dense, b), rtol=1e-8, atol=1e-12)


def test_iluk_with_complete_fill_is_a_direct_solve(gpu_ctx):
    """5-point Laplacian on an 8 x 8 grid in natural order: every fill entry of the complete LU factorisation has level
    <= 8, so ILU(8) is that factorisation and one application of the preconditioner solves the system (no oracle
    involved); ILU(k) for smaller k approaches it monotonically."""
    m = 8
    T = sps.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    S = (sps.kron(sps.identity(m), T) + sps.kron(sps.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sps.identity(m))).tocsr()
    S.sort_indices()
    n = m * m
    A = hip.Matrix.from_csr(gpu_ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)
    b = np.cos(np.arange(n, dtype=float))
    exact = np.linalg.solve(S.toarray(), b)
    nnz_prev, err_prev = 0, np.inf
    for k in (0, 1, 3, 8):
        M = hip.Precond(gpu_ctx, A, "bjacobi-ilu%d" % k, 64)
        nnz = M.info()["factor_nnz"]
        err = np.linalg.norm(M.apply(b) - exact) / np.linalg.norm(exact)
        assert nnz > nnz_prev and err < err_prev
        nnz_prev, err_prev = nnz, err
    assert err_prev < 1e-12
    D = S.toarray() != 0                                  # pattern of the complete factorisation, textbook elimination
    for p in range(n):
        rows = np.nonzero(D[p + 1:, p])[0] + p + 1
        D[np.ix_(rows, np.nonzero(D[p, p + 1:])[0] + p + 1)] = True
    assert nnz_prev == int(D.sum())


def test_solve_with_zero_right_hand_side(gpu_ctx):
    """Belos scales by |r0|; a zero residual means scale 1 and immediate convergence (x stays at the guess)."""
    pr = Problem(tgv_spec(dim=2, n=16, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    x = np.zeros(pr.n)
    info = hip.solve(gpu_ctx, A, np.zeros(pr.n), x, prec=hip.Precond(gpu_ctx, A, "jacobi"), singular=True)
    assert info.converged == 1 and info.iters == 0 and not x.any()


def test_assembly_with_an_isolated_particle(gpu_ctx):
    """a particle without neighbours: its row is the diagonal alone (and zero for the Laplacian), on both sides"""
    pr = Problem(tgv_spec(dim=2, n=12, mode=workload.JITTER))
    p = dict(pr.parts)
    nl = p["nlocal"]
    # cut every link of particle 5: drop its list and remove it from the others' lists
    ptr, idx = p["neigh_ptr"], p["neigh_idx"]
    own = p["owner_index"]
    new_ptr, new_idx = [0], []
    for i in range(nl):
        nb = idx[ptr[i]:ptr[i + 1]]
        nb = nb[own[nb] != 5] if i != 5 else nb[:0]
        new_idx.append(nb)
        new_ptr.append(new_ptr[-1] + len(nb))
    p["neigh_ptr"] = np.asarray(new_ptr, np.int32)
    p["neigh_idx"] = np.concatenate(new_idx).astype(np.int32)
    P = orc.Particles(p, pr.colmap, kernel=pr.spec.kernel)
    P.precompute(corrections=False)
    rp, ci, val, b = P.poisson(pr.spec.dt, p["rho"], p["v"], antisym=True, singular=orc.NOT_SINGULAR)
    A, bg = hip.assemble_poisson(gpu_ctx, p, pr.colmap, pr.spec.dt, p["rho"], p["v"], antisym=True, vfrac=P.vfrac,
                                 singular=hip.NOT_SINGULAR)
    rg, cg, vg = A.export_csr()
    assert rp[6] - rp[5] == 1 and np.array_equal(rg, rp) and np.array_equal(cg, ci)
    assert np.max(np.abs(vg - val)) <= 1e-12 * np.abs(val).max()
    assert np.max(np.abs(bg - b)) <= 1e-12 * max(np.abs(b).max(), 1e-300)


def test_spmv_window_compressed_columns_and_fallback(gpu_ctx, monkeypatch):
    """The SpMV re-encodes columns as (window, offset) in 16 bits per slice when a slice touches <= 64 windows of
    1024 columns; a matrix that scatters its columns keeps the 32-bit kernel.  Both must agree with SciPy, through
    the host-pointer and the device-pointer entry."""
    rng = np.random.default_rng(8)
    n = 150_000
    # (a) banded: columns within +-20000 of the row in 40 clusters -> compressible
    rows = np.repeat(np.arange(n), 40)
    cols_a = (rows + rng.integers(-20000, 20000, size=rows.size)) % n
    # (b) scattered over the whole range -> more than 64 windows per slice
    cols_b = rng.integers(0, n, size=rows.size)
    x = rng.standard_normal(n)
    for cols in (cols_a, cols_b):
        S = sps.csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(n, n))
        S.sum_duplicates(); S.sort_indices()
        ys = S @ x
        A = hip.Matrix.from_csr(gpu_ctx, S.indptr, S.indices, S.data)
        y = A.spmv(x)
        assert np.max(np.abs(y - ys)) <= 1e-12 * np.abs(ys).max()
    import torch
    S = sps.csr_matrix((rng.standard_normal(rows.size), (rows, cols_a)), shape=(n, n))
    S.sum_duplicates(); S.sort_indices()
    A = hip.Matrix.from_csr(gpu_ctx, S.indptr, S.indices, S.data)
    xd = torch.from_numpy(x).cuda()
    yd = torch.zeros_like(xd)
    hip._check(hip.lib().isph_spmv(gpu_ctx.h, A.h, hip._ptr(xd), hip._ptr(yd), 1))
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), A.spmv(x))


def test_gpu_matches_committed_golden_fixture(gpu_ctx):
    """tests/golden/tgv2d_walls_12.npz: assembly (both families), Helmholtz, ILU(0) factor, solve and AMG aggregates on
    the device against the committed expected outputs -- no live oracle in the comparison."""
    import importlib.util
    import os
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(gdir, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    G = np.load(os.path.join(gdir, "tgv2d_walls_12.npz"))
    kinds = [orc.FLUID, orc.SOLID]
    for fam, pr in mg.golden_problem().items():
        p = pr.parts
        antisym = fam == "antisym"
        kw = dict(antisym=antisym, vfrac=pr.P.vfrac, kinds=kinds, Gc=None if antisym else pr.P.Gc,
                  Lc=None if antisym else pr.P.Lc)
        A, bg = hip.assemble_poisson(gpu_ctx, p, pr.colmap, pr.spec.dt, p["rho"], p["v"], singular=hip.NOT_SINGULAR, **kw)
        rg, cg, vg = A.export_csr()
        assert np.array_equal(rg, G[fam + "_rowptr"]) and np.array_equal(cg, G[fam + "_colidx"])
        assert np.max(np.abs(vg - G[fam + "_val"])) <= 1e-12 * np.abs(G[fam + "_val"]).max()
        assert np.max(np.abs(bg - G[fam + "_b"])) <= 1e-12 * np.abs(G[fam + "_b"]).max()
        x = p["x"]
        nall = p["nall"]
        pres = np.cos(x[:, 0]) * np.sin(x[:, 1])
        force = np.ascontiguousarray(0.01 * np.stack([np.sin(x[:, 1]), np.cos(x[:, 0]), np.zeros(nall)], axis=1))
        H, bh = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, 0.5, p["nu"], p["rho"], pres, force,
                                       np.array([0.05, -0.02, 0.0]), np.ascontiguousarray(p["v"]), **kw)
        assert np.max(np.abs(H.export_csr()[2] - G[fam + "_helm_val"])) <= 1e-12 * np.abs(G[fam + "_helm_val"]).max()
        assert np.max(np.abs(bh - G[fam + "_helm_b"].ravel())) <= 1e-12 * np.abs(G[fam + "_helm_b"]).max()
        if antisym:
            M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 64)
            assert np.max(np.abs(M.export_ilu()[2] - G["ilu_val"])) <= 1e-10 * np.abs(G["ilu_val"]).max()
            g1rp, g1ci, g1v = hip.Precond(gpu_ctx, A, "bjacobi-ilu1", 64).export_ilu()   # level-of-fill pattern: exact
            assert np.array_equal(g1rp, G["ilu1_rowptr"]) and np.array_equal(g1ci, G["ilu1_colidx"])
            assert np.max(np.abs(g1v - G["ilu1_val"])) <= 1e-10 * np.abs(G["ilu1_val"]).max()
            xs = np.zeros(pr.n)
            info = hip.solve(gpu_ctx, A, bg.copy(), xs, prec=M)
            assert info.converged == 1 and abs(info.iters - int(G["iters"][0])) <= 1
            assert np.linalg.norm(xs - G["x"]) <= 1e-6 * np.linalg.norm(G["x"])
            Mg = hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(theta=0.05, block=64, coarse_max=16))
            assert np.array_equal(Mg.aggregates(0), G["amg_aggregates"])


@pytest.mark.parametrize("antisym", [True, False])
def test_assembly_without_row_sort_above_the_merge_threshold(gpu_ctx, antisym):
    """n > 32768 rows: the neighbour lists are ordered by column up front, the row kernels emit sorted rows with the
    diagonal in its slot and the SELL row sort is skipped -- pattern and values must still be the oracle's."""
    pr = Problem(tgv_spec(dim=3, n=34, mode=workload.JITTER, brick=8), antisym=antisym)
    assert pr.n > 32768
    rp, ci, val, b = pr.poisson()
    p = pr.parts
    kw = dict(antisym=antisym, vfrac=pr.P.vfrac, Gc=None if antisym else pr.P.Gc, Lc=None if antisym else pr.P.Lc)
    A, bg = hip.assemble_poisson(gpu_ctx, p, pr.colmap, pr.spec.dt, p["rho"], p["v"], **kw)
    rg, cg, vg = A.export_csr()
    assert np.array_equal(rg, rp) and np.array_equal(cg, ci)
    assert np.max(np.abs(vg - val)) <= 1e-12 * np.abs(val).max()
    assert np.max(np.abs(bg - b)) <= 1e-12 * np.abs(b).max()
    # rows really are column-sorted on the device (the ILU and the export rely on it): ILU(0) pattern == A's in-block one
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 512)
    frp, fci, fv = M.export_ilu()
    assert all(np.all(np.diff(fci[frp[i]:frp[i + 1]]) > 0) for i in range(0, pr.n, 97))
    nall = p["nall"]
    zeros = np.zeros(nall)
    H, bh = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, 0.5, p["nu"], p["rho"], zeros, np.zeros((nall, 3)),
                                   np.zeros(3), np.ascontiguousarray(p["v"]), **kw)
    rph, cih, vh, bho = pr.P.helmholtz(pr.spec.dt, 0.5, p["nu"], p["rho"], zeros, np.zeros((nall, 3)), np.zeros(3),
                                       np.ascontiguousarray(p["v"]), antisym=antisym)
    rg, cg, vg = H.export_csr()
    assert np.array_equal(cg, cih) and np.max(np.abs(vg - vh)) <= 1e-12 * np.abs(vh).max()


@pytest.mark.parametrize("antisym", [True, False])
def test_manufactured_solution_consistency_of_the_assembled_operator(gpu_ctx, antisym):
    """The reference's own unit-test template (mls-src/test_mls_laplacian_matrix_compact_poisson.cpp:34-142: u = sin x sin y
    on a periodic lattice, residual of the assembled operator against the analytic Laplacian), applied to the device
    assembly without any oracle in the loop: A = -dt/rho * Laplacian, so A u must approach 2 dt/rho u, and the error must
    fall when the lattice is refined."""
    errs = []
    for n in (24, 48):
        pr = Problem(tgv_spec(dim=2, n=n, mode=workload.LATTICE, brick=8), antisym=antisym)
        p = pr.parts
        kw = dict(antisym=antisym, vfrac=pr.P.vfrac, Gc=None if antisym else pr.P.Gc, Lc=None if antisym else pr.P.Lc)
        A, _ = hip.assemble_poisson(gpu_ctx, p, pr.colmap, pr.spec.dt, p["rho"], p["v"], **kw)
        x = p["x"][:pr.n]
        u = np.sin(x[:, 0]) * np.sin(x[:, 1])
        scale = 2.0 * pr.spec.dt / p["rho"][0]
        r = A.spmv(u) - scale * u
        errs.append(np.sqrt(np.mean(r * r)) / (scale * np.sqrt(np.mean(u * u))))
    assert errs[0] < 0.08 and errs[1] < 0.5 * errs[0]


def test_operators_with_device_tensors_and_refusal_of_mislabelled_pointers(gpu_ctx):
    """The streaming operators take device pointers (on_device = 1) as well; a device pointer handed over as a host
    pointer is refused instead of being dereferenced on the host."""
    import ctypes as C
    import torch
    pr = Problem(tgv_spec(dim=3, n=10, mode=workload.JITTER))
    parts, P = pr.parts, pr.P
    dev = torch.device("cuda", 0)
    dparts = dict(parts)
    for k in ("x", "type", "neigh_ptr", "neigh_idx"):
        dparts[k] = torch.from_numpy(np.ascontiguousarray(parts[k])).to(dev)
    cm = torch.from_numpy(pr.colmap).to(dev)
    vf = torch.from_numpy(P.vfrac).to(dev)
    own = parts["owner_index"]
    f = np.random.default_rng(2).standard_normal(pr.n)[own]
    g_host = hip.gradient(gpu_ctx, parts, pr.colmap, f, P.vfrac, filt=(orc.FLUID, orc.FLUID))
    g_dev = hip.gradient(gpu_ctx, dparts, cm, torch.from_numpy(f).to(dev), vf, filt=(orc.FLUID, orc.FLUID))
    torch.cuda.synchronize()
    assert isinstance(g_dev, torch.Tensor) and np.array_equal(g_dev.cpu().numpy(), g_host)
    u = np.random.default_rng(3).standard_normal((pr.n, 3))[own]
    d_host = hip.divergence(gpu_ctx, parts, pr.colmap, u, P.vfrac)
    d_dev = hip.divergence(gpu_ctx, dparts, cm, torch.from_numpy(np.ascontiguousarray(u)).to(dev), vf)
    torch.cuda.synchronize()
    assert np.array_equal(d_dev.cpu().numpy(), d_host)
    # mislabelled: device particle arrays, on_device = 0
    keep = []
    pv, isdev, keep = hip.particles_view(dparts, cm, vfrac=vf, keep=keep)
    out = np.zeros((pr.n, 3))
    rc = hip.lib().isph_gradient(gpu_ctx.h, C.byref(pv), 1, hip._ptr(f), 1.0, 0, 127, 127, hip._ptr(out), 0)
    assert rc != 0 and b"on_device = 0" in hip.lib().isph_last_error()
    with pytest.raises(ValueError):
        hip.gradient(gpu_ctx, dparts, cm, f, vf)      # host field with device particles


def test_repeated_setups_do_not_grow_device_memory(gpu_ctx):
    """The reference rebuilds matrix and preconditioner every time step; here the released buffers go back to the
    library's pool and the next set-up takes them from there: device memory in use must be flat from round to round
    (scripts/soak.py is the 200-round version at 100^3)."""
    import torch
    pr = Problem(tgv_spec(dim=3, n=32, mode=workload.JITTER))
    used = []
    for r in range(8):
        A, b = hip.assemble_poisson(gpu_ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                    np.ascontiguousarray(pr.parts["v"]), vfrac=pr.P.vfrac)
        M = hip.PrecondAMG(gpu_ctx, A, nullvec=np.full(pr.n, 1.0 / np.sqrt(pr.n))) if r % 2 else hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 512)
        x = np.zeros(pr.n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=True)
        assert info.converged == 1
        M.close()
        A.close()
        gpu_ctx.sync()
        fr, tot = torch.cuda.mem_get_info()
        used.append(tot - fr)
    assert max(used[3:]) - min(used[3:]) <= 8 << 20, used          # after both kinds ran once: flat to within 8 MB
    assert hip.pool_cached_bytes() > 0


@pytest.mark.parametrize("kind", ["bjacobi-ilu0", "bjacobi-ilu1", "sa-amg"])
def test_exactly_sized_stream_gives_the_same_preconditioner(gpu_ctx, kind):
    """The triangular-solve stream sized by a counting pass of the schedule (what streams beyond 4 GiB get: the
    Gauss-Seidel smoother of BASELINE configs[4]) against the one-pass capacity rule: the same factor, the same stream
    length, the same application bit for bit -- only the reservation differs."""
    pr = Problem(tgv_spec(dim=3, n=20, mode=workload.JITTER))
    rp, ci, val, b = pr.poisson()
    n = pr.n
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    nv = np.ones(n) / np.sqrt(n)
    r = np.random.default_rng(9).standard_normal(n)

    def make():
        if kind == "sa-amg":
            return hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=hip.AmgParams(block=256, coarse_max=64))
        return hip.Precond(gpu_ctx, A, kind, 256)
    M0 = make()
    z0 = M0.apply(r)
    i0 = M0.info() if kind != "sa-amg" else None
    try:
        hip.set_exact_stream_threshold(0)
        M1 = make()
        z1 = M1.apply(r)
        if kind != "sa-amg":
            i1 = M1.info()
            assert i1["stream_chunks"] == i0["stream_chunks"] and i1["factor_nnz"] == i0["factor_nnz"]
            assert i1["stream_capacity"] < i0["stream_capacity"]              # exact: used chunks + the per-block pads
            assert i1["stream_capacity"] <= i1["stream_chunks"] + 33 * (i1["nblocks"] + 1) + 32
            for a, c in zip(M0.export_ilu(), M1.export_ilu()):
                assert np.array_equal(a, c)
        if kind == "sa-amg":   # two AMG set-ups differ in the last bits (the Galerkin products accumulate with LDS atomics)
            assert np.linalg.norm(z0 - z1) <= 1e-11 * np.linalg.norm(z0)
        else:
            assert np.array_equal(z0, z1)
        M1.close()
    finally:
        hip.set_exact_stream_threshold(-1)
    M0.close(); A.close()
