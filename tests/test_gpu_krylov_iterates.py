"""-m gpu: the device's GMRES / PCG iterates against the plain reference (tests/krylov_reference.py) and the oracle.

With tol = 0 and max_iters = k, isph_solve returns x_k of restarted GMRES(m) (or of PCG) from the given x0: a vector
that every correct orthogonalisation, flexible or not, must reproduce to round-off, whose recurrence residual must
equal its true residual.  Each case checks x_k, |rel_res_implicit - true_rel_res|, iters == k, restarts and reorth.

Bound per case: max(C * oracle gap, floor), the oracle's gap to the same reference measured in the same case.  No case
sits where x_k is round-off: the reference's true residual is at least 1e-10 wherever the iterate is compared.

Measured on an MI355X, max over k of ||x - x_ref|| / ||x_ref||, device / oracle:
  TGV 1089 rows, DGKS / ICGS / IMGS, flexible or not:  singular 1.6e-14 / 1.6e-14, shifted 5.7e-14 / 5.3e-14
  restarts m = 1, 5 (k = 13): 1.3e-15 / 1.5e-15;  n = 1..129: 9.2e-15 / 9.6e-15 (k = n <= 62: the exact solution)
  599 675-row stencil, k = 17, 49: 4.2e-15 / 4.3e-15;  PCG on 600 625 rows: 1.0e-13 / 1.0e-13
  wall mask, x0 along n: 4.3e-13 / 3.7e-13 (that system's round-off level, the same on both sides)
Device / oracle ratio at most 2.6 in any case and k; recurrence residuals within 1.2e-14 of the true ones.  reorth:
ICGS k, IMGS 0, DGKS every step on the TGV and Helmholtz systems and the reference's count elsewhere (11 of 13 steps
restarted every 5, 3 of 13 restarted every step, from a random x0).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip, workload
import oracle as orc
import krylov_reference as kr
from problems import Problem, tgv_spec, wall_types

pytestmark = pytest.mark.gpu

KS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 61, 62]   # every multi-dot batch / k_multi_axpy_dot instance edge
C_ORACLE = 10.0      # measured device / oracle gap ratio: at most 2.6 over every case and k
ITER_FLOOR = 1e-14   # x_k relative, where the oracle happens to land closer than that
RES_FLOOR = 1e-15    # |rel_res_implicit - true_rel_res|, both relative to ||r0||
ROUND_OFF = 1e-10
DGKS, ICGS, IMGS = 0, 1, 2


def params(k, m=62, ortho=DGKS, flexible=1, solver_type=0, tol=0.0):
    return hip.SolverParams(solver_type=solver_type, num_blocks=m, max_iters=k, max_restarts=10 ** 6, tol=tol, ortho=ortho,
                            flexible=flexible)


def check(label, info, x, ref, k, restarts, orc_x, orc_info, reorth=None):
    """x_k, recurrence residual, counters of one device solve; the oracle's x_k sets the scale of the bound"""
    go, gro = kr.iterate_gap(orc_x, ref.x), kr.residual_gap(orc_info.rel_res_implicit, ref)
    gx, gr = kr.iterate_gap(x, ref.x), kr.residual_gap(info.rel_res_implicit, ref)
    print("krylov-gap %-40s k=%-3d dev %.2e orc %.2e | res dev %.2e orc %.2e | true %.2e reorth %d" %
          (label, k, gx, go, gr, gro, ref.rel_res, info.reorth))
    assert ref.rel_res >= ROUND_OFF, (label, k, ref.rel_res)
    assert info.iters == k and info.restarts == restarts and info.converged == 0, (label, k, info.iters, info.restarts)
    assert orc_info.iters == k
    assert gx <= max(C_ORACLE * go, ITER_FLOOR), (label, k, gx, go)
    assert gr <= max(C_ORACLE * gro, RES_FLOOR), (label, k, gr, gro)
    if reorth is not None:
        assert info.reorth == reorth, (label, k, info.reorth, reorth)


def expected_reorth(ortho, ref, k):
    """ICGS: every step; IMGS: 0 (include/isph_hip.h); DGKS: the steps whose first pass left |w| < |w_old| / sqrt(2)
    in the reference (None where a step lies within 1e-6 of that threshold)"""
    if ortho == ICGS:
        return k
    if ortho == IMGS:
        return 0
    return ref.dgks_second_passes() if ref.dgks_margin() > 1e-6 else None


def dev_prec(ctx, A, prec, bs=256):
    return None if prec == "none" else hip.Precond(ctx, A, prec, bs if prec == "bjacobi-ilu0" else 0)


# ---------------------------------------------------------------- variant product on the 1089-row TGV system
@functools.lru_cache(maxsize=None)
def tgv_system(singular):
    rp, ci, val = kr.tgv_rows(None if singular else kr.SHIFT)
    n = len(rp) - 1
    return rp, ci, val, sps.csr_matrix((val, ci, rp), shape=(n, n)), np.random.default_rng(7).standard_normal(n)


@functools.lru_cache(maxsize=None)
def tgv_reference(singular, prec):
    rp, ci, val, A, b = tgv_system(singular)
    n = A.shape[0]
    return kr.gmres_iterates(A, b, np.zeros(n), KS, 62, kr.minv_for(prec, rp, ci, val), kr.unit_null(None, n) if singular else None)


@pytest.fixture(scope="module")
def tgv_dev(gpu_ctx):
    cache = {}

    def get(singular, prec):
        if (singular, prec) not in cache:
            rp, ci, val, _, _ = tgv_system(singular)
            A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
            cache[(singular, prec)] = (A, dev_prec(gpu_ctx, A, prec))
        return cache[(singular, prec)]
    return get


@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("prec", ["none", "jacobi", "bjacobi-ilu0"])
@pytest.mark.parametrize("flexible", [1, 0])
@pytest.mark.parametrize("ortho", [DGKS, ICGS, IMGS])
def test_iterates_of_every_variant(gpu_ctx, tgv_dev, ortho, flexible, singular, prec):
    rp, ci, val, A_h, b = tgv_system(singular)
    n = A_h.shape[0]
    ref = tgv_reference(singular, prec)
    ks = [k for k in KS if ref[k].rel_res >= ROUND_OFF]
    assert len(ks) >= (6 if prec == "bjacobi-ilu0" else 13)
    A, M = tgv_dev(singular, prec)
    for k in ks:
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=params(k, 62, ortho, flexible))
        xo, io = kr.oracle_solve(rp, ci, val, b, None, k, 62, ortho, flexible, singular, prec)
        check("tgv o%d f%d s%d %s" % (ortho, flexible, singular, prec), info, x, ref[k], k, 0, xo, io,
              expected_reorth(ortho, ref[k], k))


@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("flexible", [1, 0])
@pytest.mark.parametrize("ortho", [DGKS, ICGS, IMGS])
@pytest.mark.parametrize("m", [1, 5])
def test_restarted_iterates(gpu_ctx, tgv_dev, m, ortho, flexible, singular):
    rp, ci, val, A_h, b = tgv_system(singular)
    n = A_h.shape[0]
    x0 = np.random.default_rng(8).standard_normal(n)
    ref = kr.gmres_iterates(A_h, b, x0, [13], m, kr.minv_for("jacobi", rp, ci, val), kr.unit_null(None, n) if singular else None)[13]
    A, M = tgv_dev(singular, "jacobi")
    x = x0.copy()
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=params(13, m, ortho, flexible))
    xo, io = kr.oracle_solve(rp, ci, val, b, x0, 13, m, ortho, flexible, singular, "jacobi")
    check("restart m%d o%d f%d s%d" % (m, ortho, flexible, singular), info, x, ref, 13, 12 // m, xo, io,
          expected_reorth(ortho, ref, 13))


# ---------------------------------------------------------------- vector lengths
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_tiny_sizes(gpu_ctx, n):
    """odd and even lengths below one wave, the odd last row of the paired multi-dot; k = n <= 62 is a full Krylov space
    (the exact solution, breakdown included); k = n > 62 crosses a restart"""
    A_h = kr.tiny(n)
    rp, ci, val = A_h.indptr.astype(np.int32), A_h.indices.astype(np.int32), A_h.data
    b = np.random.default_rng(n).standard_normal(n)
    ks = sorted({k for k in (1, 2, 17, 62, n) if k <= n})
    ref = kr.gmres_iterates(A_h, b, np.zeros(n), ks, 62, None)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    exact = np.linalg.solve(A_h.toarray(), b)
    for ortho in (DGKS, ICGS, IMGS):
        for k in ks:
            x = np.zeros(n)
            info = hip.solve(gpu_ctx, A, b.copy(), x, params=params(k, 62, ortho))
            xo, io = kr.oracle_solve(rp, ci, val, b, None, k, 62, ortho)
            go, gx = kr.iterate_gap(xo, ref[k].x), kr.iterate_gap(x, ref[k].x)
            gro, gr = kr.residual_gap(io.rel_res_implicit, ref[k]), kr.residual_gap(info.rel_res_implicit, ref[k])
            print("krylov-gap %-40s k=%-3d dev %.2e orc %.2e | res dev %.2e orc %.2e | true %.2e reorth %d" %
                  ("tiny n%d o%d" % (n, ortho), k, gx, go, gr, gro, ref[k].rel_res, info.reorth))
            assert info.iters == k and info.restarts == (k - 1) // 62 and io.iters == k
            assert gx <= max(C_ORACLE * go, ITER_FLOOR) and gr <= max(C_ORACLE * gro, RES_FLOOR)
            e = expected_reorth(ortho, ref[k], k)
            assert e is None or info.reorth == e, (ortho, k, info.reorth, e)
            if k == n <= 62:
                assert kr.iterate_gap(x, exact) <= ITER_FLOOR and info.rel_res_implicit <= RES_FLOOR


@functools.lru_cache(maxsize=None)
def big_stencil(singular):
    A_h = kr.stencil3d(85, 85, 83, shift=0.0 if singular else 0.5)   # 599 675 rows: odd, past both grid caps
    n = A_h.shape[0]
    b = np.random.default_rng(11).standard_normal(n)
    ref = kr.gmres_iterates(A_h, b, np.zeros(n), [17, 49], 62, None, kr.unit_null(None, n) if singular else None)
    return A_h, b, ref


@pytest.mark.parametrize("singular", [True, False])
def test_long_vectors_take_several_grid_trips(gpu_ctx, singular):
    A_h, b, ref = big_stencil(singular)
    n = A_h.shape[0]
    assert n % 2 == 1 and n > 2 * 512 * 256 and n > 2048 * 256
    rp, ci, val = A_h.indptr.astype(np.int32), A_h.indices.astype(np.int32), A_h.data
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    for ortho in (DGKS, ICGS):
        for k in (17, 49):
            x = np.zeros(n)
            info = hip.solve(gpu_ctx, A, b.copy(), x, singular=singular, params=params(k, 62, ortho))
            xo, io = kr.oracle_solve(rp, ci, val, b, None, k, 62, ortho, 1, singular)
            check("stencil3d o%d s%d" % (ortho, singular), info, x, ref[k], k, 0, xo, io, expected_reorth(ortho, ref[k], k))


# ---------------------------------------------------------------- the second Gram-Schmidt pass
def test_dgks_reorthogonalises_every_step_of_a_helmholtz_system(gpu_ctx):
    """I - theta dt nu L: every Arnoldi step loses more than 1 - 1/sqrt(2) of its norm in the first pass, so DGKS runs the
    second pass at every step and the Pythagoras norm |w_new|^2 - |c2|^2 carries every Hessenberg column"""
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER))
    p = pr.parts
    nall, n = p["nall"], pr.n
    zeros = np.zeros(nall)
    A, _ = hip.assemble_helmholtz(gpu_ctx, p, pr.colmap, pr.spec.dt, 0.5, p["nu"], p["rho"], zeros, np.zeros((nall, 3)),
                                  np.zeros(3), np.ascontiguousarray(p["v"]), vfrac=pr.P.vfrac)
    rp, ci, val = A.export_csr()
    A_h = sps.csr_matrix((val, ci, rp), shape=(n, n))
    b = np.random.default_rng(5).standard_normal(n)
    ks = [1, 5, 9]
    ref = kr.gmres_iterates(A_h, b, np.zeros(n), ks, 62)
    for k in ks:
        assert ref[k].dgks_second_passes() == k and ref[k].dgks_margin() > 0.5
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, params=params(k))
        xo, io = kr.oracle_solve(rp, ci, val, b, None, k, 62)
        check("helmholtz dgks", info, x, ref[k], k, 0, xo, io, reorth=k)


# ---------------------------------------------------------------- singular forms
@pytest.mark.parametrize("prec", ["none", "jacobi"])
def test_null_vector_from_a_mask_and_x0_along_it(gpu_ctx, prec):
    """the wall case: n = mask / ||mask|| over the non-solid rows; x0 has a component along n, which the iterate loses"""
    pr = Problem(tgv_spec(dim=2, n=20, mode=workload.JITTER), kinds=[orc.FLUID, orc.SOLID], types=wall_types)
    rp, ci, val, b = pr.poisson()
    n = pr.n
    mask = (pr.parts["type"][:n] != 2).astype(np.int32)
    assert 0 < mask.sum() < n
    A_h = sps.csr_matrix((val, ci, rp), shape=(n, n))
    nul = kr.unit_null(mask, n)
    x0 = np.random.default_rng(9).standard_normal(n) + 5.0 * nul
    ref = kr.gmres_iterates(A_h, b, x0, [17, 49], 62, kr.minv_for(prec, rp, ci, val), nul)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = dev_prec(gpu_ctx, A, prec)
    for ortho in (DGKS, ICGS, IMGS):
        for k in (17, 49):
            x = x0.copy()
            info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=True, null_mask=mask, params=params(k, 62, ortho))
            xo, io = kr.oracle_solve(rp, ci, val, b, x0, k, 62, ortho, 1, True, prec, null_mask=mask)
            check("wall mask o%d %s" % (ortho, prec), info, x, ref[k], k, 0, xo, io, expected_reorth(ortho, ref[k], k))
            assert abs(np.dot(x, nul)) <= 1e-12 * np.linalg.norm(x)


# ---------------------------------------------------------------- several right-hand sides
def lockstep_columns(A_h, nvec, seed):
    """column 0: b = A x0 with x0 a multiple of one unit vector (the residual is exactly 0 in any summation order);
    the others: seeded random b and x0"""
    n = A_h.shape[0]
    rng = np.random.default_rng(seed)
    B, X0 = rng.standard_normal((nvec, n)), 0.1 * rng.standard_normal((nvec, n))
    X0[0] = 0.0
    X0[0, n // 2] = 1.5
    B[0] = A_h @ X0[0]
    return B, X0


@pytest.mark.parametrize("nvec", [2, 3, 4, 5])
@pytest.mark.parametrize("ortho", [DGKS, ICGS])
@pytest.mark.parametrize("k,m", [(33, 62), (13, 5)])
def test_lockstep_columns_are_their_own_iterates(gpu_ctx, tgv_dev, nvec, ortho, k, m):
    """nvec 2..4 advance together (k_sell_spmm16<2|3|4>), 5 one after the other; every column carries the bits of its own
    single solve and is the k-th iterate of its own Krylov space; the zero-residual column stays at x0"""
    rp, ci, val, A_h, _ = tgv_system(False)
    n = A_h.shape[0]
    A, M = tgv_dev(False, "jacobi")
    B, X0 = lockstep_columns(A_h, nvec, seed=20 + nvec)
    bflat, xflat = B.ravel().copy(), X0.ravel().copy()
    info = hip.solve(gpu_ctx, A, bflat, xflat, prec=M, nvec=nvec, lda=n, params=params(k, m, ortho))
    minv = kr.minv_for("jacobi", rp, ci, val)
    reorth = 0
    for c in range(nvec):
        xc = xflat[c * n:(c + 1) * n]
        xs = X0[c].copy()
        single = hip.solve(gpu_ctx, A, B[c].copy(), xs, prec=M, params=params(k, m, ortho))
        assert np.array_equal(xs, xc), c
        if c == 0:
            assert single.iters == 0 and single.converged == 1 and np.array_equal(xc, X0[0])
            continue
        ref = kr.gmres_iterates(A_h, B[c], X0[c], [k], m, minv)[k]
        xo, io = kr.oracle_solve(rp, ci, val, B[c], X0[c], k, m, ortho, 1, False, "jacobi")
        check("lockstep nvec%d o%d m%d col%d" % (nvec, ortho, m, c), single, xc, ref, k, (k - 1) // m, xo, io,
              expected_reorth(ortho, ref, k))
        reorth += single.reorth
    assert info.iters == (nvec - 1) * k and info.restarts == (nvec - 1) * ((k - 1) // m) and info.reorth == reorth


@pytest.mark.parametrize("nvec", [2, 3, 4, 5])
@pytest.mark.parametrize("ortho", [DGKS, ICGS])
def test_lockstep_columns_converging_at_different_iterations(gpu_ctx, tgv_dev, nvec, ortho):
    rp, ci, val, A_h, _ = tgv_system(False)
    n = A_h.shape[0]
    A, M = tgv_dev(False, "jacobi")
    B, X0 = lockstep_columns(A_h, nvec, seed=40 + nvec)
    xs = np.linspace(0.0, 1.0, n)
    B[1] = A_h @ np.sin(np.pi * xs)                      # smooth: converges in fewer iterations than the random columns
    if nvec > 2:
        B[2] *= 1e3
        X0[2] = 0.0
    prm = params(500, 5, ortho, tol=1e-8)
    bflat, xflat = B.ravel().copy(), X0.ravel().copy()
    info = hip.solve(gpu_ctx, A, bflat, xflat, prec=M, nvec=nvec, lda=n, params=prm)
    its = []
    for c in range(nvec):
        x = X0[c].copy()
        single = hip.solve(gpu_ctx, A, B[c].copy(), x, prec=M, params=prm)
        assert single.converged == 1 and np.array_equal(x, xflat[c * n:(c + 1) * n]), c
        its.append(single.iters)
    assert len(set(its)) >= min(nvec, 3), its
    assert info.converged == 1 and info.iters == sum(its)


# ---------------------------------------------------------------- PCG
@functools.lru_cache(maxsize=None)
def big_laplacian(singular, prec):
    A_h = kr.laplace2d(775, 775, seed=12, shift=None if singular else 0.3)   # 600 625 rows
    n = A_h.shape[0]
    rp, ci, val = A_h.indptr.astype(np.int32), A_h.indices.astype(np.int32), A_h.data
    b = np.random.default_rng(13).standard_normal(n)
    ref = kr.pcg_iterates(A_h, b, np.zeros(n), [1, 2, 17, 49], kr.minv_for(prec, rp, ci, val),
                          kr.unit_null(None, n) if singular else None)
    return rp, ci, val, b, ref


@pytest.mark.parametrize("singular", [False, True])
@pytest.mark.parametrize("prec", ["none", "jacobi"])
def test_pcg_iterates(gpu_ctx, singular, prec):
    rp, ci, val, b, ref = big_laplacian(singular, prec)
    n = len(rp) - 1
    assert n % 2 == 1 and n > 2048 * 256
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = dev_prec(gpu_ctx, A, prec)
    for k in (1, 2, 17, 49):
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=params(k, solver_type=1))
        xo, io = kr.oracle_solve(rp, ci, val, b, None, k, 62, singular=singular, prec=prec, solver_type=1)
        check("pcg s%d %s" % (singular, prec), info, x, ref[k], k, 0, xo, io, reorth=0)


# ---------------------------------------------------------------- operand paths
def test_device_tensors_give_the_host_bits(gpu_ctx, tgv_dev):
    import torch
    rp, ci, val, A_h, b = tgv_system(True)
    n = A_h.shape[0]
    A, M = tgv_dev(True, "jacobi")
    ref = tgv_reference(True, "jacobi")
    xo, io = kr.oracle_solve(rp, ci, val, b, None, 33, 62, DGKS, 1, True, "jacobi")
    xh = np.zeros(n)
    hip.solve(gpu_ctx, A, b.copy(), xh, prec=M, singular=True, params=params(33))
    bd = torch.tensor(b, dtype=torch.float64, device="cuda")
    xd = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = hip.solve(gpu_ctx, A, bd, xd, prec=M, singular=True, params=params(33))
    x = xd.cpu().numpy()
    assert np.array_equal(x, xh)
    check("device tensors", info, x, ref[33], 33, 0, xo, io, expected_reorth(DGKS, ref[33], 33))


@pytest.mark.parametrize("prec", ["none", "jacobi"])
def test_library_row_numbering(gpu_ctx_bricks, prec):
    """an assembled Poisson matrix in the library's own numbering: isph_solve gathers b, x and scatters x; with a
    permutation-invariant preconditioner the iterate is that of the caller's matrix (export_csr)"""
    pr = Problem(tgv_spec(dim=2, n=33, mode=workload.JITTER))
    A, _ = hip.assemble_poisson(gpu_ctx_bricks, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                np.ascontiguousarray(pr.parts["v"]), vfrac=pr.P.vfrac)
    assert A.ordering() is not None
    rp, ci, val = A.export_csr()
    n = pr.n
    A_h = sps.csr_matrix((val, ci, rp), shape=(n, n))
    b = np.random.default_rng(14).standard_normal(n)
    ref = kr.gmres_iterates(A_h, b, np.zeros(n), [17, 49], 62, kr.minv_for(prec, rp, ci, val), kr.unit_null(None, n))
    M = dev_prec(gpu_ctx_bricks, A, prec)
    for k in (17, 49):
        x = np.zeros(n)
        info = hip.solve(gpu_ctx_bricks, A, b.copy(), x, prec=M, singular=True, params=params(k))
        xo, io = kr.oracle_solve(rp, ci, val, b, None, k, 62, singular=True, prec=prec)
        check("bricks %s" % prec, info, x, ref[k], k, 0, xo, io, expected_reorth(DGKS, ref[k], k))


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("m", [0, 63])
@pytest.mark.parametrize("nvec", [1, 3])
def test_num_blocks_outside_1_to_62_is_refused(gpu_ctx, tgv_dev, m, nvec):
    rp, ci, val, A_h, b = tgv_system(False)
    n = A_h.shape[0]
    A, _ = tgv_dev(False, "none")
    with pytest.raises(hip.IsphError, match="Num Blocks"):
        hip.solve(gpu_ctx, A, np.tile(b, nvec), np.zeros(n * nvec), nvec=nvec, lda=n, params=params(10, m))
