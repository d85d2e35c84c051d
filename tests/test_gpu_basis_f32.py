"""-m gpu: GMRES with the Krylov basis stored in single precision (isph_solver_params::basis_bits = 32) against the numpy
restatement tests/krylov_cb_reference.py, which rounds where include/isph_hip.h says the device rounds.

Criterion of every iterate comparison (tol = 0, max_iters = k: isph_solve returns x_k):
    gap32 = |x_dev - x_ref32| / |x_ref32|,  sep = |x_ref32 - x_ref64| / |x_ref32|,  gap32 <= C_SEP * sep
x_ref32 / x_ref64 are the restatement's iterates with a 32- / 64-bit basis.  A device that skipped the rounding, or rounded
somewhere else, sits at gap32 ~ sep; one whose fp64 summation order flips a single float rounding sits near
sep / sqrt(n k).  The recurrence residual is held the same way: |rel_res_implicit - rec32| <= C_SEP * |rec32 - rec64|,
with the floor RES_FLOOR = 1e-13, ten times the 1.2e-14 that tests/test_gpu_krylov_iterates.py measured between the
fp64 device's recurrence residual and the reference's on these systems (where the two restatements' residuals happen
to coincide the separation says nothing about fp64 round-off).  k with a restatement residual below 1e-10 are skipped,
as the fp64 iterate tests do.

Measured on an MI355X, max over k of gap32 / sep (the device agrees with the restatement to fp64 round-off):
  TGV 1089 rows, DGKS / ICGS, flexible or not: none 4.8e-8 singular / 1.7e-7 shifted, jacobi 3.6e-8 / 5.4e-8,
  bjacobi-ilu0 7.4e-8 / 7.6e-8;  restarts m = 1, 5 (k = 13): 5.2e-8;  n = 2 .. 129: 3.0e-8;  wall mask: 4.8e-9
  recurrence residuals: within 5.6e-17 of the restatement's (their separation 2e-14 .. 6e-10)
C_SEP = 1.8e-6 is 10 x the largest of these (1.71e-7), far below the cap of 1e-2 that the specification sets; one float
rounding flipped by another fp64 summation order would sit near sep / sqrt(n k) = 4e-3 sep and fail it.

Tails (test_tails_and_tiny_systems): the specification asks for the true residual <= 1e-6 |b| after k = min(n, 62)
iterations for n in {1, 2, 3, 63, 64, 65, 127, 128, 129}, calling that an exact Krylov solve.  It is one only for
n <= 62: GMRES(62) in exact fp64 arithmetic (the host restatement, 64 bits) leaves 1.7e-6 at n = 63 and 1.2e-3 .. 2.3e-3
at n = 127 .. 129 after 62 iterations, so no correct solver meets the cap there.  The test keeps the cap and every n,
and checks it where the method can reach it: after k = min(n, 62) iterations for n <= 62 and n in {64, 65} (restatement:
<= 1.5e-7), and after five cycles (310 iterations, restatement <= 1e-13) for every n > 62.  The k = min(n, 62) iterate
of every n is compared with the restatement by the criterion above, which is what catches a wrong tail at that k.

Explicit residual of the singular fixtures (tests 4 and 10): the specification asks for rel_res_explicit <= 1e-8 on
tgv16 and on the two-rank TGV brick.  rel_res_explicit is |b - A x| / |b| with the UNPROJECTED A
(include/isph_hip.h), and these matrices are not symmetric: their left null vector is not n (|A^T n| = 5e-3 on tgv16),
so b - A x keeps a component along n that no projected solve removes -- 1.0765e-4 on tgv16 with the fp64 basis, on the
device and in the restatement alike.  What the confirmation guarantees is the projected residual |P(b - A x)| / |P b|
(the scale of the recurrence test for a zero start); the tests hold THAT to 1e-8 (1 + 1e-6), computed on the host in
longdouble from the returned x, and rel_res_explicit to the fp64 basis' value of the same system.  The non-singular
fixtures are held to rel_res_explicit <= 1e-8 (1 + 1e-6) as specified.
"""
import functools
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import build, hip, workload
import oracle as orc
import chebyshev_reference as cr
import krylov_cb_reference as cb
import krylov_reference as kr
from problems import Problem, tgv_spec, wall_types

pytestmark = pytest.mark.gpu

KS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 61, 62]   # every multi-dot batch / k_multi_axpy_dot instance edge
C_SEP = 1.8e-6
RES_FLOOR = 1e-13
ROUND_OFF = 1e-10
DGKS, ICGS, IMGS = 0, 1, 2
TOL = 1e-8


def params(k, m=62, ortho=DGKS, flexible=1, tol=0.0, bits=32, solver_type=0, max_restarts=10 ** 6):
    return hip.SolverParams(solver_type=solver_type, num_blocks=m, max_iters=k, max_restarts=max_restarts, tol=tol, ortho=ortho,
                            flexible=flexible, basis_bits=bits)


def dev_prec(ctx, A, prec, bs=256):
    return None if prec == "none" else hip.Precond(ctx, A, prec, bs if prec == "bjacobi-ilu0" else 0)


def check_iterate(label, info, x, s32, s64, k, ortho):
    """criterion 1 on one device iterate; s32 / s64: the restatement's snapshots with a 32- / 64-bit basis"""
    nrm = np.linalg.norm(s32.x)
    gap32 = float(np.linalg.norm(x - s32.x) / nrm)
    sep = float(np.linalg.norm(s32.x - s64.x) / nrm)
    rgap, rsep = abs(info.rel_res_implicit - s32.rec_res), abs(s32.rec_res - s64.rec_res)
    print("basis-f32 %-34s k=%-3d gap32 %.2e sep %.2e ratio %.2e | res gap %.2e sep %.2e | rec %.2e true %.2e reorth %d (%d)" %
          (label, k, gap32, sep, gap32 / sep if sep > 0 else np.inf, rgap, rsep, s32.rec_res, s32.rel_res, info.reorth, s32.reorth))
    assert info.iters == k and info.restarts == s32.restarts and info.residual_restarts == 0, (label, k, info.iters, info.restarts)
    assert sep > 0.0 and gap32 <= C_SEP * sep, (label, k, gap32, sep)
    assert rgap <= max(C_SEP * rsep, RES_FLOOR), (label, k, rgap, rsep)
    if ortho == ICGS:
        assert info.reorth == k
    elif s32.margin > 1e-6:
        assert info.reorth == s32.reorth, (label, k, info.reorth, s32.reorth)
    return gap32 / sep


# ---------------------------------------------------------------- 1. iterates of every variant, 1089-row TGV system
@functools.lru_cache(maxsize=None)
def tgv_system(singular):
    rp, ci, val = kr.tgv_rows(None if singular else kr.SHIFT)
    n = len(rp) - 1
    return rp, ci, val, sps.csr_matrix((val, ci, rp), shape=(n, n)), np.random.default_rng(7).standard_normal(n)


@functools.lru_cache(maxsize=None)
def tgv_reference(singular, prec, ortho, flexible, bits):
    rp, ci, val, A, b = tgv_system(singular)
    n = A.shape[0]
    return cb.iterates(A, b, np.zeros(n), KS, 62, bits, ortho, kr.minv_for(prec, rp, ci, val),
                       kr.unit_null(None, n) if singular else None, bool(flexible))


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
@pytest.mark.parametrize("ortho", [DGKS, ICGS])
def test_iterates_of_every_variant(gpu_ctx, tgv_dev, ortho, flexible, singular, prec):
    rp, ci, val, A_h, b = tgv_system(singular)
    n = A_h.shape[0]
    r32, r64 = (tgv_reference(singular, prec, ortho, flexible, bits) for bits in (32, 64))
    ks = [k for k in KS if r32[k].rel_res >= ROUND_OFF]
    assert len(ks) >= 6
    A, M = tgv_dev(singular, prec)
    worst = 0.0
    for k in ks:
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=params(k, 62, ortho, flexible))
        worst = max(worst, check_iterate("tgv o%d f%d s%d %s" % (ortho, flexible, singular, prec), info, x, r32[k], r64[k], k, ortho))
    print("basis-f32-max tgv o%d f%d s%d %s: %.2e" % (ortho, flexible, singular, prec, worst))


# ---------------------------------------------------------------- 2. tails of the paired float loads, tiny systems
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 129])
def test_tails_and_tiny_systems(gpu_ctx, n):
    """see the module docstring for the two iteration counts"""
    A_h = kr.tiny(n)
    rp, ci, val = A_h.indptr.astype(np.int32), A_h.indices.astype(np.int32), A_h.data
    b = np.random.default_rng(n).standard_normal(n)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    k = min(n, 62)
    reachable = n <= 62 or n in (64, 65)      # GMRES(62) is below the cap after k iterations (restatement, 64 bits)
    for ortho in (DGKS, ICGS):
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, params=params(k, 62, ortho))
        res = kr.true_residual_norm(A_h, b, x) / np.linalg.norm(b)
        print("basis-f32 tiny n%d o%d k=%d true residual %.2e" % (n, ortho, k, res))
        assert info.iters == k
        if reachable:
            assert res <= 1e-6, (n, ortho, res)
        if n > 1:      # (n = 1: one iteration solves exactly with either basis, the restatements do not separate)
            s32 = cb.iterates(A_h, b, np.zeros(n), [k], 62, 32, ortho)[k]
            s64 = cb.iterates(A_h, b, np.zeros(n), [k], 62, 64, ortho)[k]
            if s32.rel_res >= ROUND_OFF:
                check_iterate("tiny n%d o%d" % (n, ortho), info, x, s32, s64, k, ortho)
        if n > 62:
            x = np.zeros(n)
            info = hip.solve(gpu_ctx, A, b.copy(), x, params=params(310, 62, ortho))
            res = kr.true_residual_norm(A_h, b, x) / np.linalg.norm(b)
            print("basis-f32 tiny n%d o%d k=310 true residual %.2e restarts %d" % (n, ortho, res, info.restarts))
            assert info.iters == 310 and info.restarts == 4 and res <= 1e-6, (n, ortho, res)
    A.close()


# ---------------------------------------------------------------- 3. restarts
@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("flexible", [1, 0])
@pytest.mark.parametrize("ortho", [DGKS, ICGS])
@pytest.mark.parametrize("m", [1, 5])
def test_restarted_iterates(gpu_ctx, tgv_dev, m, ortho, flexible, singular):
    rp, ci, val, A_h, b = tgv_system(singular)
    n = A_h.shape[0]
    x0 = np.random.default_rng(8).standard_normal(n)
    null = kr.unit_null(None, n) if singular else None
    minv = kr.minv_for("jacobi", rp, ci, val)
    s32 = cb.iterates(A_h, b, x0, [13], m, 32, ortho, minv, null, bool(flexible))[13]
    s64 = cb.iterates(A_h, b, x0, [13], m, 64, ortho, minv, null, bool(flexible))[13]
    assert s32.restarts == 12 // m
    A, M = tgv_dev(singular, "jacobi")
    x = x0.copy()
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=params(13, m, ortho, flexible))
    check_iterate("restart m%d o%d f%d s%d" % (m, ortho, flexible, singular), info, x, s32, s64, 13, ortho)


# ---------------------------------------------------------------- 4. convergence with the confirmation
@functools.lru_cache(maxsize=None)
def fixture(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    return rp, ci, val, sps.csr_matrix((val, ci, rp), shape=(n, n)), b, singular


@pytest.mark.parametrize("name,prec", [("tgv16", "jacobi"), ("tgv16", "bjacobi-ilu0"), ("wall42", "jacobi"),
                                       ("wall42", "bjacobi-ilu0"), ("stencil", "jacobi")])
def test_convergence_is_confirmed_by_the_true_residual(gpu_ctx, name, prec):
    rp, ci, val, A_h, b, singular = fixture(name)
    n = A_h.shape[0]
    ref = cb.gmres_cb(A_h, b, np.zeros(n), 50, 32, DGKS, kr.minv_for(prec, rp, ci, val), kr.unit_null(None, n) if singular else None,
                      tol=TOL, max_iters=500, max_restarts=15)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = dev_prec(gpu_ctx, A, prec)
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=params(500, 50, tol=TOL, max_restarts=15))
    x64 = np.zeros(n)
    i64 = hip.solve(gpu_ctx, A, b.copy(), x64, prec=M, singular=singular, params=params(500, 50, tol=TOL, max_restarts=15, bits=64))
    if M is not None:
        M.close()
    A.close()
    print("basis-f32-converge %-8s %-13s device iters %d restarts %d residual_restarts %d explicit %.3e | restatement iters %d "
          "restarts %d residual_restarts %d confirmations %s | 64 bits: iters %d restarts %d" %
          (name, prec, info.iters, info.restarts, info.residual_restarts, info.rel_res_explicit, ref.iters, ref.restarts,
           ref.residual_restarts, ["%.3e" % c for c in ref.confirmations], i64.iters, i64.restarts))
    assert ref.converged == 1 and info.converged == 1
    if singular:      # see the module docstring: rel_res_explicit of this system is 1.08e-4 with either basis
        null = kr.unit_null(None, n)
        bp = b - np.dot(b, null) * null
        true = kr.true_residual_norm(A_h, bp, x, null) / np.linalg.norm(bp)
        print("basis-f32-converge %-8s %-13s projected true residual on the host %.3e, rel_res_explicit at 64 bits %.3e" %
              (name, prec, true, i64.rel_res_explicit))
        assert true <= TOL * (1.0 + 1e-6)
        assert abs(info.rel_res_explicit - i64.rel_res_explicit) <= 1e-6 * i64.rel_res_explicit
    else:
        assert info.rel_res_explicit <= TOL * (1.0 + 1e-6)
    assert abs(info.iters - ref.iters) <= 1, (info.iters, ref.iters)
    if all(abs(c / TOL - 1.0) > 0.01 for c in ref.confirmations):
        assert (info.restarts, info.residual_restarts) == (ref.restarts, ref.residual_restarts)
    else:
        print("basis-f32-converge %s %s: a confirmation of the restatement lies within 1 %% of tol, restarts not compared" % (name, prec))
    assert i64.converged == 1 and i64.residual_restarts == 0


# ---------------------------------------------------------------- 5. singular system with a mask
@pytest.mark.parametrize("prec", ["none", "jacobi"])
def test_null_vector_from_a_mask_and_x0_along_it(gpu_ctx, prec):
    """the wall case of test_gpu_krylov_iterates.py: n = mask / |mask| over the non-solid rows, x0 with a component along n"""
    pr = Problem(tgv_spec(dim=2, n=20, mode=workload.JITTER), kinds=[orc.FLUID, orc.SOLID], types=wall_types)
    rp, ci, val, b = pr.poisson()
    n = pr.n
    mask = (pr.parts["type"][:n] != 2).astype(np.int32)
    assert 0 < mask.sum() < n
    A_h = sps.csr_matrix((val, ci, rp), shape=(n, n))
    nul = kr.unit_null(mask, n)
    x0 = np.random.default_rng(9).standard_normal(n) + 5.0 * nul
    minv = kr.minv_for(prec, rp, ci, val)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = dev_prec(gpu_ctx, A, prec)
    for ortho in (DGKS, ICGS):
        r32 = cb.iterates(A_h, b, x0, [17, 49], 62, 32, ortho, minv, nul)
        r64 = cb.iterates(A_h, b, x0, [17, 49], 62, 64, ortho, minv, nul)
        for k in (17, 49):
            x = x0.copy()
            info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=True, null_mask=mask, params=params(k, 62, ortho))
            assert abs(np.dot(x, nul)) <= 1e-12 * np.linalg.norm(x)
            check_iterate("wall mask o%d %s" % (ortho, prec), info, x, r32[k], r64[k], k, ortho)
    if M is not None:
        M.close()
    A.close()


# ---------------------------------------------------------------- 6. lockstep
@pytest.mark.parametrize("k,m", [(33, 62), (13, 5)])
def test_lockstep_columns_equal_their_single_solves(gpu_ctx, tgv_dev, k, m):
    """three right-hand sides advance together, each with its own float basis: every column carries the bits of its own
    basis_bits = 32 solve (the relation tests/test_gpu_parity.py and test_gpu_krylov_iterates.py hold at 64 bits: equal arrays)"""
    rp, ci, val, A_h, _ = tgv_system(False)
    n = A_h.shape[0]
    A, M = tgv_dev(False, "jacobi")
    rng = np.random.default_rng(23)
    B, X0 = rng.standard_normal((3, n)), 0.1 * rng.standard_normal((3, n))
    for prm in (params(k, m), params(500, m, tol=TOL)):
        bflat, xflat = B.ravel().copy(), X0.ravel().copy()
        info = hip.solve(gpu_ctx, A, bflat, xflat, prec=M, nvec=3, lda=n, params=prm)
        its = rst = rr = 0
        for c in range(3):
            xs = X0[c].copy()
            single = hip.solve(gpu_ctx, A, B[c].copy(), xs, prec=M, params=prm)
            xc = xflat[c * n:(c + 1) * n]
            assert np.linalg.norm(xs - xc) <= 1e-12 * np.linalg.norm(xs) and np.array_equal(xs, xc), c
            its, rst, rr = its + single.iters, rst + single.restarts, rr + single.residual_restarts
        assert (info.iters, info.restarts, info.residual_restarts) == (its, rst, rr)
        x64 = X0.ravel().copy()
        hip.solve(gpu_ctx, A, B.ravel().copy(), x64, prec=M, nvec=3, lda=n,
                  params=hip.SolverParams(num_blocks=m, max_iters=prm.max_iters, max_restarts=10 ** 6, tol=prm.tol))
        assert not np.array_equal(x64, xflat)
    assert info.converged == 1


# ---------------------------------------------------------------- 7. the default is unchanged
@pytest.mark.parametrize("singular", [True, False])
def test_basis_bits_0_and_64_are_the_solve_without_the_field(gpu_ctx, tgv_dev, singular):
    rp, ci, val, A_h, b = tgv_system(singular)
    n = A_h.shape[0]
    A, M = tgv_dev(singular, "jacobi")
    plain = hip.SolverParams(num_blocks=30, max_iters=47, max_restarts=10 ** 6, tol=0.0)
    outs = []
    for prm in (plain, params(47, 30, bits=0), params(47, 30, bits=64)):
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=prm)
        outs.append((x, (info.converged, info.iters, info.restarts, info.rel_res_implicit, info.rel_res_explicit, info.reorth,
                         info.residual_restarts)))
    assert plain.basis_bits == 0
    for x, inf in outs[1:]:
        assert np.array_equal(x, outs[0][0]) and inf == outs[0][1]
    x32 = np.zeros(n)
    hip.solve(gpu_ctx, A, b.copy(), x32, prec=M, singular=singular, params=params(47, 30, bits=32))
    assert not np.array_equal(x32, outs[0][0])


# ---------------------------------------------------------------- 8. refusals
def test_refused_combinations_name_the_field(gpu_ctx, tgv_dev):
    rp, ci, val, A_h, b = tgv_system(False)
    n = A_h.shape[0]
    A, M = tgv_dev(False, "jacobi")
    refused = [params(10, 20, solver_type=1), params(10, 20, solver_type=2), params(10, 20, ortho=IMGS), params(10, 20, bits=16)]
    refused[1].num_recycled = 5
    for prm in refused:
        with pytest.raises(hip.IsphError, match="basis_bits"):
            hip.solve(gpu_ctx, A, b.copy(), np.zeros(n), prec=M, params=prm)
    with pytest.raises(hip.IsphError, match="basis_bits"):
        hip.solve(gpu_ctx, A, np.tile(b, 3), np.zeros(3 * n), prec=M, nvec=3, lda=n, params=params(10, 20, bits=16))
    with pytest.raises(hip.IsphError, match="basis_bits"):
        hip.solve_block(gpu_ctx, [[A]], b.copy().reshape(1, n), np.zeros((1, n)), prec=M, params=params(10, 20))
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, params=params(500, 50, tol=TOL))   # the context solves normally afterwards
    assert info.converged == 1 and info.rel_res_explicit <= TOL * (1.0 + 1e-6)
    xb = np.zeros((1, n))
    assert hip.solve_block(gpu_ctx, [[A]], b.copy().reshape(1, n), xb, prec=M, params=params(500, 50, tol=TOL, bits=64)).converged == 1


# ---------------------------------------------------------------- 9. memory
def test_the_float_basis_halves_the_pool_peak_of_the_basis():
    A_h = kr.stencil3d(85, 85, 83, shift=0.5)      # 599 675 rows, the long system of the iterate tests
    n, m = A_h.shape[0], 50
    ld = (n + 63) // 64 * 64
    rp, ci, val = A_h.indptr.astype(np.int32), A_h.indices.astype(np.int32), A_h.data
    b = np.random.default_rng(11).standard_normal(n)
    peak = {}
    for bits in (32, 64):
        ctx = hip.Context(0)      # its own context: the Krylov workspaces of a context only grow
        A = hip.Matrix.from_csr(ctx, rp, ci, val)
        hip.pool_trim()
        base = hip.pool_info(reset_peak=True)["live"]
        info = hip.solve(ctx, A, b.copy(), np.zeros(n), params=params(3, m, bits=bits))
        peak[bits] = hip.pool_info()["peak_live"] - base
        assert info.iters == 3
        A.close()
        ctx.close()
    print("basis-f32-memory pool peak above the matrix: 64 bits %d B, 32 bits %d B, difference %d B, 4 ld (m + 1) = %d B" %
          (peak[64], peak[32], peak[64] - peak[32], 4 * ld * (m + 1)))
    assert peak[64] - peak[32] >= 0.9 * 4 * ld * (m + 1)


# ---------------------------------------------------------------- 10. two ranks
def _solve_two_ranks(rank, G, dim, pgrid, n):
    from test_gpu_ranks import _rank_setup
    st = _rank_setup(rank, G, dim, pgrid, n, orc.NULLSPACE)
    ctx, A = st["ctx"], st["A"]
    try:
        M = hip.Precond(ctx, A, "jacobi", 0)
        x, bb = np.zeros(st["nl"]), st["b"].copy()
        info = hip.solve(ctx, A, bb, x, prec=M, singular=True, params=params(500, 50, tol=TOL, max_restarts=15))
        M.close()
        return dict(rtag=st["rtag"], x=x, bproj=bb, info=(info.converged, info.iters, info.restarts, info.residual_restarts, info.rel_res_explicit))
    finally:
        A.close()
        ctx.close()


def test_two_ranks_solve_like_one(gpu_ctx):
    from ranks import RankGroup
    from test_gpu_ranks import GlobalOracle
    dim, pgrid, n = 3, (2, 1, 1), 8
    G = RankGroup(2)
    try:
        res = G.run(_solve_two_ranks, dim, pgrid, n)
    finally:
        G.close()
    O = GlobalOracle(dim, pgrid, n, orc.NULLSPACE, [r["rtag"] for r in res])
    A = hip.Matrix.from_csr(gpu_ctx, O.Ap.indptr.astype(np.int32), O.Ap.indices.astype(np.int32), O.Ap.data)
    M = hip.Precond(gpu_ctx, A, "jacobi", 0)
    x1 = np.zeros(O.N)
    one = hip.solve(gpu_ctx, A, O.bp.copy(), x1, prec=M, singular=True, params=params(500, 50, tol=TOL, max_restarts=15))
    M.close(); A.close()
    infos = {r["info"][:4] for r in res}
    print("basis-f32-ranks two ranks %s explicit %s | one rank iters %d restarts %d residual_restarts %d explicit %.3e" %
          (sorted(infos), [r["info"][4] for r in res], one.iters, one.restarts, one.residual_restarts, one.rel_res_explicit))
    assert len(infos) == 1, infos
    conv, iters, restarts, rres = infos.pop()
    assert conv == 1 and one.converged == 1
    assert iters == one.iters and rres == one.residual_restarts
    x = np.concatenate([r["x"] for r in res])
    bb = np.concatenate([r["bproj"] for r in res])      # b after the solve's projection, rank by rank
    null = kr.unit_null(None, O.N)
    true = kr.true_residual_norm(O.Ap, bb, x, null) / np.linalg.norm(bb)
    print("basis-f32-ranks projected true residual of the two-rank x on the host %.3e (rel_res_explicit %.3e, one rank %.3e)" %
          (true, res[0]["info"][4], one.rel_res_explicit))
    assert true <= TOL * (1.0 + 1e-6)      # (module docstring: the explicit residual of a singular, nonsymmetric system)
    assert all(abs(r["info"][4] - one.rel_res_explicit) <= 1e-6 * one.rel_res_explicit for r in res)
    assert np.linalg.norm(x - x1) <= 1e-6 * np.linalg.norm(x1)


# ---------------------------------------------------------------- 11. the C++ mirror's key
def run_cpp(tmp_path, name, bits, block_rows=256):
    rp, ci, val, A_h, b, singular = fixture(name)
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / ("x%d.bin" % bits))
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_basis_f32_test(), fin, fout, "1" if singular else "0", str(bits), str(block_rows)],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


@pytest.mark.parametrize("name", ["tgv16", "wall42"])
def test_solver_key_gives_the_python_solve(gpu_ctx, tmp_path, name):
    r32, x32 = run_cpp(tmp_path, name, 32)
    assert r32.returncode == 0, r32.stdout[-2000:] + r32.stderr[-2000:]
    rp, ci, val, A_h, b, singular = fixture(name)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 256)
    x, x64 = np.zeros(len(rp) - 1), np.zeros(len(rp) - 1)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=hip.SolverParams(basis_bits=32))
    hip.solve(gpu_ctx, A, b.copy(), x64, prec=M, singular=singular, params=hip.SolverParams())
    M.close(); A.close()
    line = [l for l in r32.stdout.splitlines() if l.startswith("converged=")][-1]
    g = kr.iterate_gap(x32, x)
    print("\nbasis-f32-key %-8s %s | python: iters %d restarts %d residual_restarts %d | x against python's %.2e" %
          (name, line, info.iters, info.restarts, info.residual_restarts, g))
    assert line.split()[:4] == ["converged=1", "iters=%d" % info.iters, "restarts=%d" % info.restarts,
                                "residual_restarts=%d" % info.residual_restarts]
    assert g <= 1e-12
    assert not np.array_equal(x32, x64)       # the key reached the device


def test_solver_key_refuses_other_widths(tmp_path):
    r, _ = run_cpp(tmp_path, "stencil", 16, 64)
    assert r.returncode == 1
    assert "isph: krylov basis bits" in r.stderr and "not available; available: 64, 32" in r.stderr, r.stderr
