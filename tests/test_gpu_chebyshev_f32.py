"""-m gpu: value_bits = 32 of the Chebyshev polynomial in D^-1 A -- the stand-alone preconditioner
(isph_cheb_params::value_bits, "chebyshev<d>-f32"), the smoother of the SA-AMG (isph_amg_params::cheb_value_bits), one
rank and two, and the key "isph: chebyshev value bits" of the C++ wrappers.

What is expected (include/isph_hip.h): exactly the fp64 recurrence of tests/chebyshev_reference.py on A~ = fl32(A), the
matrix whose stored values went through float once (tests/chebyshev_f32_reference.py).  Only the values the sweeps read
are single precision; vectors, accumulators and the update are double, so the device has to reach the SAME bounds
against the A~ restatement as the fp64 mode reaches against the A restatement:
  one application                     <= 1e-12 max|z|   (APPLY_TOL of tests/test_gpu_chebyshev.py, the gate for sweeps)
  fused against ISPH_CHEB_UNFUSED=1   <= 1e-14 max
  library numbering against caller's  <= 1e-13
  one AMG cycle                       <= 1e-12 ||z||    (the suite's 1e-9 for AMG cycles cannot tell this operator from
                                                         the fp64 one, they differ by ~1e-8; the fp64 cycle measured
                                                         2e-16 .. 1.5e-15 against numpy and this one does the same
                                                         arithmetic on other values)
and it has to be on the fl32 side: for degree >= 2 one application differs from the A restatement by >= 1e-10 (the two
restatements differ by 5e-9 .. 8e-8 on these fixtures, tests/test_chebyshev_f32_reference.py), so a silent fall-back to
the doubles fails.  Solves: converged with an explicit residual <= 1e-7, iteration counts within one of the 64-bit solve
of the same test (the project's parity gate), x within 1e-6 of its x.  Every gap is printed before it is asserted.
"""
import functools
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import build, hip
import chebyshev_reference as cr
import chebyshev_f32_reference as c32
import krylov_reference as kr

pytestmark = pytest.mark.gpu

APPLY_TOL = 1e-12          # against the restatement on fl32(A)
NOT_FP64 = 1e-10           # against the restatement on A, degree >= 2
CYCLE_TOL = 1e-12
DEGREES = [1, 2, 3, 4, 7]
AMG_KW = dict(theta=0.0, block=256, coarse_max=64)
FIXTURES = ["tgv16", "wall42", "stencil", "spd"]
gap_max = c32.gap_max


@functools.lru_cache(maxsize=None)
def system(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    A = sps.csr_matrix((val, ci, rp), shape=(n, n))
    return rp, ci, val, b, singular, A, c32.fl32(A)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            rp, ci, val = system(name)[:3]
            cache[name] = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        return cache[name]
    yield get
    for A in cache.values():
        A.close()


def rhs(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def nullvec(name):
    n = system(name)[5].shape[0]
    return np.ones(n) / np.sqrt(n) if system(name)[4] else None


def amg(ctx, A, name, bits, sweeps=2, **kw):
    prm = hip.AmgParams(smoother=2, sweeps=sweeps, cheb_value_bits=bits, **dict(AMG_KW, **kw))
    return hip.PrecondAMG(ctx, A, nullvec=nullvec(name), params=prm)


# ---------------------------------------------------------------- 1. one application
@pytest.mark.parametrize("ratio", [30.0, 5.0])
@pytest.mark.parametrize("name", FIXTURES)
def test_apply_is_the_recurrence_on_the_rounded_matrix(gpu_ctx, dev, name, ratio):
    A_h, A32 = system(name)[5:]
    r = rhs(A_h.shape[0])
    for d in DEGREES:
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, ratio=ratio, value_bits=32)
        assert M.value_bits == 32
        z = M.apply(r)
        g32, g64 = gap_max(z, cr.cheb_apply(A32, r, None, d, ratio)), gap_max(z, cr.cheb_apply(A_h, r, None, d, ratio))
        print("cheb-f32-apply %-8s degree %d ratio %4.1f gap to fl32(A) %.2e to A %.2e" % (name, d, ratio, g32, g64))
        assert g32 <= APPLY_TOL, (name, d, ratio, g32)
        if d >= 2:
            assert g64 >= NOT_FP64, (name, d, ratio, g64)
        M.close()


@pytest.mark.parametrize("name", ["tgv16", "stencil"])
def test_given_eigenvalues_the_string_form_and_the_handles_value_bits(gpu_ctx, dev, name):
    A_h, A32 = system(name)[5:]
    r = rhs(A_h.shape[0], 6)
    lam = 1.7
    for d in DEGREES:
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, ratio=30.0, lambda_max=lam, value_bits=32)
        z = M.apply(r)
        assert gap_max(z, cr.cheb_apply(A32, r, None, d, 30.0, lam=lam)) <= APPLY_TOL
        if d >= 2:
            assert gap_max(z, cr.cheb_apply(A_h, r, None, d, 30.0, lam=lam)) >= NOT_FP64
        M.close()
    M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=4, ratio=30.0, lambda_max=lam, lambda_min=lam / 8.0, value_bits=32)
    assert gap_max(M.apply(r), cr.cheb_apply(A32, r, None, 4, 8.0, lam=lam)) <= APPLY_TOL
    M.close()
    for d in (1, 3, 16):
        M = hip.Precond(gpu_ctx, dev(name), "chebyshev%d-f32" % d, 0)
        z = M.apply(r)
        g32, g64 = gap_max(z, cr.cheb_apply(A32, r, None, d, 30.0)), gap_max(z, cr.cheb_apply(A_h, r, None, d, 30.0))
        print("cheb-f32-string %-8s chebyshev%d-f32 gap to fl32(A) %.2e to A %.2e" % (name, d, g32, g64))
        assert M.value_bits == 32 and g32 <= APPLY_TOL
        assert d < 2 or g64 >= NOT_FP64
        M.close()
    # the plain forms stay double, 0 means 64, and every other preconditioner answers 0
    M = hip.Precond(gpu_ctx, dev(name), "chebyshev3", 0)
    z64 = M.apply(r)
    assert M.value_bits == 64 and gap_max(z64, cr.cheb_apply(A_h, r, None, 3, 30.0)) <= APPLY_TOL
    M.close()
    for bits in (0, 64):
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3, value_bits=bits)
        assert M.value_bits == 64 and np.array_equal(M.apply(r), z64)
        M.close()
    M = hip.Precond(gpu_ctx, dev(name), "jacobi", 0)
    assert M.value_bits == 0
    M.close()
    assert hip.ChebParams().value_bits == 64 and hip.AmgParams().cheb_value_bits == 64


# ---------------------------------------------------------------- 2. the fused step against the composition
@pytest.mark.parametrize("name", FIXTURES)
def test_fused_step_against_the_unfused_composition(gpu_ctx, dev, monkeypatch, name):
    A_h, A32 = system(name)[5:]
    r = rhs(A_h.shape[0], 9)
    for d in (2, 3, 7):
        Mf = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, value_bits=32)
        monkeypatch.setenv("ISPH_CHEB_UNFUSED", "1")
        Mu = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, value_bits=32)
        monkeypatch.delenv("ISPH_CHEB_UNFUSED")
        zf, zu = Mf.apply(r), Mu.apply(r)
        g = gap_max(zf, zu)
        print("cheb-f32-fused %-8s degree %d gap %.2e" % (name, d, g))
        assert g <= 1e-14
        assert gap_max(zu, cr.cheb_apply(A32, r, None, d, 30.0)) <= APPLY_TOL      # the float-valued SpMV, on its own
        assert gap_max(zu, cr.cheb_apply(A_h, r, None, d, 30.0)) >= NOT_FP64
        Mf.close(); Mu.close()
    if name == "stencil":
        return
    # the AMG cycle: 32-bit columns on the coarse levels, the step from a guess
    for sweeps in (1, 2, 3):
        Mf = amg(gpu_ctx, dev(name), name, 32, sweeps)
        monkeypatch.setenv("ISPH_CHEB_UNFUSED", "1")
        Mu = amg(gpu_ctx, dev(name), name, 32, sweeps)
        monkeypatch.delenv("ISPH_CHEB_UNFUSED")
        zf, zu = Mf.apply(r), Mu.apply(r)
        g = float(np.linalg.norm(zf - zu) / np.linalg.norm(zu))
        print("cheb-f32-fused %-8s amg sweeps %d gap %.2e" % (name, sweeps, g))
        assert g <= 1e-13
        Mf.close(); Mu.close()


# ---------------------------------------------------------------- 3. operands and numberings
@pytest.mark.parametrize("name", ["tgv16", "wall42"])
def test_device_operands_give_the_host_bits(gpu_ctx, dev, name):
    import torch
    n = system(name)[5].shape[0]
    r = rhs(n, 7)
    for d in (1, 2, 7):
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, value_bits=32)
        zh = M.apply(r)
        zd = M.apply(torch.tensor(r, dtype=torch.float64, device="cuda"))
        assert np.array_equal(zd.cpu().numpy(), zh)
        buf = torch.zeros(2 * n + 2, dtype=torch.float64, device="cuda")      # 8-byte aligned operands only
        buf[1:n + 1] = torch.tensor(r, dtype=torch.float64, device="cuda")
        zo = M.apply(buf[1:n + 1], buf[n + 2:2 * n + 2])
        assert np.array_equal(zo.cpu().numpy(), zh) and float(buf[n + 1]) == 0.0
        M.close()


@pytest.mark.parametrize("name", ["stencil", "spd"])
def test_the_librarys_row_numbering_gives_the_callers_result(gpu_ctx, gpu_ctx_bricks, dev, name):
    rp, ci, val, _, _, A_h, A32 = system(name)
    xyz, dim = cr.coordinates(name)
    Ab = hip.Matrix.from_host_csr_with_coords(gpu_ctx_bricks, rp, ci, val, xyz, dim=dim)
    assert Ab.ordering() is not None
    r = rhs(A_h.shape[0], 8)
    for d in DEGREES:
        Mb = hip.PrecondChebyshev(gpu_ctx_bricks, Ab, degree=d, value_bits=32)
        Mc = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, value_bits=32)
        zb, zc = Mb.apply(r), Mc.apply(r)
        g = gap_max(zb, zc)
        print("cheb-f32-numbering %-8s degree %d gap %.2e" % (name, d, g))
        assert g <= 1e-13, (name, d)
        assert gap_max(zb, cr.cheb_apply(A32, r, None, d, 30.0)) <= APPLY_TOL
        Mb.close(); Mc.close()
    Ab.close()


# ---------------------------------------------------------------- 4. the AMG smoother
def assert_same_hierarchy(M, M0):
    """patterns, values (bit for bit), sizes and aggregates"""
    assert M.levels == M0.levels >= 2
    for l in range(M.levels):
        assert M.level_info(l) == M0.level_info(l)
        for what in ("A", "P") if l < M.levels - 1 else ("A",):
            (rp, ci, v), (rp0, ci0, v0) = M.export(l, what), M0.export(l, what)
            assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0), (l, what)
            assert np.array_equal(v, v0), (l, what, float(np.max(np.abs(v - v0))))
        if l < M.levels - 1:
            assert np.array_equal(M.aggregates(l), M0.aggregates(l))


@pytest.mark.parametrize("sweeps", [1, 2, 4])
@pytest.mark.parametrize("name", ["tgv16", "wall42", "spd"])
def test_amg_smooths_with_the_rounded_level_operators(gpu_ctx, dev, name, sweeps):
    """tgv16: a null vector, the coarsest level is the polynomial (of fl32 of that level too); wall42 / spd: the dense
    inverse of the fp64 coarsest operator.  The hierarchy is the fp64 one; only the smoother reads floats."""
    singular, A_h = system(name)[4:6]
    n = A_h.shape[0]
    M, M64 = amg(gpu_ctx, dev(name), name, 32, sweeps), amg(gpu_ctx, dev(name), name, 64, sweeps)
    assert M.value_bits == 32 and M64.value_bits == 64
    assert_same_hierarchy(M, M64)
    levels = cr.levels_from(M, n)
    r = rhs(n, 10)
    z = M.apply(r)
    z32 = c32.amg_vcycle(levels, r, sweeps=sweeps, ratio=20.0, coarse_polynomial=singular, single=True)
    z64 = c32.amg_vcycle(levels, r, sweeps=sweeps, ratio=20.0, coarse_polynomial=singular, single=False)
    nz = np.linalg.norm(z32)
    g32, g64, apart = np.linalg.norm(z - z32) / nz, np.linalg.norm(z - z64) / nz, np.linalg.norm(z32 - z64) / nz
    print("cheb-f32-amg-cycle %-8s sweeps %d levels %d gap to the fl32 cycle %.2e to the fp64 cycle %.2e (the two cycles: %.2e)" %
          (name, sweeps, M.levels, g32, g64, apart))
    assert g32 <= CYCLE_TOL
    assert apart >= NOT_FP64 and g64 >= NOT_FP64 and g32 < g64
    # the 64-bit build of the same test is the fp64 cycle
    assert np.linalg.norm(M64.apply(r) - z64) <= CYCLE_TOL * np.linalg.norm(z64)
    M.close(); M64.close()


def test_amg_only_reads_cheb_value_bits_for_the_chebyshev_smoother(gpu_ctx, dev):
    r = rhs(1764)
    z = []
    for bits in (64, 32, 16):
        M = hip.PrecondAMG(gpu_ctx, dev("wall42"), params=hip.AmgParams(smoother=0, cheb_value_bits=bits, **AMG_KW))
        assert M.value_bits == 0
        z.append(M.apply(r))
        M.close()
    assert np.array_equal(z[0], z[1]) and np.array_equal(z[0], z[2])


# ---------------------------------------------------------------- 5. solves
def solver_params(solver_type=0):
    return hip.SolverParams(solver_type=solver_type, num_blocks=50, max_iters=500, max_restarts=10 ** 6, tol=1e-8)


def make_prec(ctx, A, name, kind, bits):
    if kind == "cheb":
        return hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0, value_bits=bits)
    return amg(ctx, A, name, bits, 2)


@pytest.mark.parametrize("name,kind,solver_type", [("tgv16", "cheb", 0), ("wall42", "cheb", 0), ("stencil", "cheb", 0), ("spd", "cheb", 0),
                                                   ("spd", "cheb", 1), ("spd", "amg", 1), ("tgv16", "amg", 0), ("wall42", "amg", 0)])
def test_solves_keep_the_iteration_count_of_the_double_preconditioner(gpu_ctx, dev, name, kind, solver_type):
    b, singular, A_h = system(name)[3:6]
    n = A_h.shape[0]
    A = dev(name)
    out = {}
    for bits in (64, 32):
        M = make_prec(gpu_ctx, A, name, kind, bits)
        assert M.value_bits == bits
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=solver_params(solver_type))
        out[bits] = (x, info)
        M.close()
    (x64, i64), (x32, i32) = out[64], out[32]
    gx = kr.iterate_gap(x32, x64)
    # the explicit residual: of a singular system the solver reports ||b - A x|| / ||b|| with the UNPROJECTED operator, as
    # the reference does (isph_solve_info; 1e-4 on tgv16 whatever the preconditioner, printed below for both widths), so
    # for tgv16 the residual of the system that is solved, P (b - A x) with P = I - n n^T, is formed here
    if singular:
        proj = lambda v: v - v.mean()
        eres = {bits: float(np.linalg.norm(proj(b - A_h @ out[bits][0])) / np.linalg.norm(proj(b))) for bits in (64, 32)}
    else:
        eres = {64: i64.rel_res_explicit, 32: i32.rel_res_explicit}
    print("cheb-f32-solve %-8s %-4s type %d iterations %d (64 bits: %d) explicit residual %.2e (64 bits: %.2e; reported %.2e, %.2e) "
          "x against the 64-bit x %.2e" % (name, kind, solver_type, i32.iters, i64.iters, eres[32], eres[64],
                                            i32.rel_res_explicit, i64.rel_res_explicit, gx))
    assert i64.converged == 1 and i32.converged == 1
    assert eres[32] <= 1e-7
    assert abs(i32.iters - i64.iters) <= 1, (i32.iters, i64.iters)
    assert gx <= 1e-6


def test_three_columns_against_single_solves(gpu_ctx, dev):
    n = system("wall42")[5].shape[0]
    A = dev("wall42")
    M = hip.PrecondChebyshev(gpu_ctx, A, degree=3, value_bits=32)
    B = np.random.default_rng(11).standard_normal((3, n))
    singles = []
    for c in range(3):
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, B[c].copy(), x, prec=M, params=solver_params())
        assert info.converged == 1
        singles.append((x, info.iters))
    xflat = np.zeros(3 * n)
    info = hip.solve(gpu_ctx, A, B.ravel().copy(), xflat, prec=M, nvec=3, lda=n, params=solver_params())
    assert info.converged == 1 and info.iters == sum(k for _, k in singles)
    for c in range(3):
        g = kr.iterate_gap(xflat[c * n:(c + 1) * n], singles[c][0])
        print("cheb-f32-nvec column %d gap %.2e" % (c, g))
        assert g <= 1e-12, c
    M.close()


# ---------------------------------------------------------------- 6. refusals
def _entry(rp, ci, i, j):
    return rp[i] + int(np.flatnonzero(ci[rp[i]:rp[i + 1]] == j)[0])


def test_refusals(gpu_ctx, dev):
    A = dev("wall42")
    for bits in (16, 33, -1):
        with pytest.raises(hip.IsphError, match="value_bits"):
            hip.PrecondChebyshev(gpu_ctx, A, degree=2, value_bits=bits)
        with pytest.raises(hip.IsphError, match="cheb_value_bits"):
            hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=2, cheb_value_bits=bits, **AMG_KW))
    for kind in ("chebyshev3-f3", "chebyshev3-f64x", "chebyshev3-f32x", "chebyshev17-f32", "chebyshev-f32"):
        with pytest.raises(hip.IsphError, match="unknown preconditioner type"):
            hip.Precond(gpu_ctx, A, kind, 0)
    with pytest.raises(hip.IsphError, match="chebyshev<d>-f32"):
        hip.Precond(gpu_ctx, A, "chebyshev3-f3", 0)
    rp, ci, val = system("wall42")[:3]
    n = len(rp) - 1
    i = 77
    j = int(ci[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] != i][0])
    r = rhs(n, 12)
    # beyond FLT_MAX (finite in fp64): refused by the 32-bit form only
    v = val.copy(); v[_entry(rp, ci, i, j)] = 1e39
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    with pytest.raises(hip.IsphError, match="single precision"):
        hip.PrecondChebyshev(gpu_ctx, Az, degree=2, value_bits=32)
    with pytest.raises(hip.IsphError, match="single precision"):
        hip.Precond(gpu_ctx, Az, "chebyshev2-f32", 0)
    hip.PrecondChebyshev(gpu_ctx, Az, degree=2, value_bits=64).close()
    Az.close()
    # a diagonal entry that rounds to 0
    v = val.copy(); v[_entry(rp, ci, i, i)] = 1e-50
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    with pytest.raises(hip.IsphError, match="zero diagonal"):
        hip.PrecondChebyshev(gpu_ctx, Az, degree=2, value_bits=32)
    with pytest.raises(hip.IsphError, match="zero diagonal"):
        hip.PrecondAMG(gpu_ctx, Az, params=hip.AmgParams(smoother=2, cheb_value_bits=32, **AMG_KW))
    Az.close()
    # an off-diagonal entry that rounds to 0 is accepted: it is 0 in fl32(A)
    v = val.copy(); v[_entry(rp, ci, i, j)] = 1e-50
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    A_h = sps.csr_matrix((v, ci, rp), shape=(n, n))
    A32 = c32.fl32(A_h)
    assert A32[i, j] == 0.0 and A32.nnz == A_h.nnz
    M = hip.PrecondChebyshev(gpu_ctx, Az, degree=3, value_bits=32)
    g = gap_max(M.apply(r), cr.cheb_apply(A32, r, None, 3, 30.0))
    print("cheb-f32-underflow gap %.2e" % g)
    assert g <= APPLY_TOL
    M.close(); Az.close()


# ---------------------------------------------------------------- 7. two thread ranks on one GPU
def _rank_solve(rank, G, dim, pgrid, n, kind):
    import oracle as orc
    import test_gpu_ranks as tr
    st = tr._rank_setup(rank, G, dim, pgrid, n, orc.NULLSPACE)
    ctx, A = st["ctx"], st["A"]
    try:
        nl = st["nl"]
        ntot = float(np.prod(pgrid[:dim])) * n ** dim
        r = np.cos(0.37 * st["rtag"].astype(np.float64))
        out = dict(nl=nl, rtag=st["rtag"], col_tag=st["col_tag"], csr=st["csr"], b=st["b"], r=r)
        for bits in (64, 32):                                     # (collective: every rank walks the same sequence)
            if kind == "cheb":
                M = hip.PrecondChebyshev(ctx, A, degree=3, value_bits=bits)
            else:
                M = hip.PrecondAMG(ctx, A, nullvec=np.full(nl, 1.0 / np.sqrt(ntot)),
                                   params=hip.AmgParams(smoother=2, sweeps=2, theta=0.02, block=256, coarse_max=64,
                                                        cheb_value_bits=bits))
            vb = M.value_bits
            z = M.apply(r)
            x, bb = np.zeros(nl), st["b"].copy()
            info = hip.solve(ctx, A, bb, x, prec=M, singular=True)
            M.close()
            out[bits] = dict(z=z, x=x, value_bits=vb, info=(info.converged, info.iters, info.rel_res_explicit))
        return out
    finally:
        A.close()
        ctx.close()


@pytest.mark.parametrize("kind", ["cheb", "amg"])
def test_two_ranks_on_one_gpu(gpu_ctx, kind):
    from ranks import RankGroup
    import test_gpu_chebyshev as tc
    dim, pgrid, n = 3, (2, 1, 1), 8
    G = RankGroup(2)
    try:
        res = G.run(_rank_solve, dim, pgrid, n, kind)
    finally:
        G.close()
    Ag, bg = tc._global_system(res)
    N = Ag.shape[0]
    info = {}
    for bits in (64, 32):
        assert all(r[bits]["value_bits"] == bits for r in res)
        got = {r[bits]["info"][:2] for r in res}
        assert len(got) == 1, got
        info[bits] = got.pop()
        assert info[bits][0] == 1
    x = np.concatenate([r[32]["x"] for r in res])
    proj = lambda v: v - v.mean()
    eres = float(np.linalg.norm(proj(bg - Ag @ x)) / np.linalg.norm(proj(bg)))
    rr, z = np.concatenate([r["r"] for r in res]), np.concatenate([r[32]["z"] for r in res])
    print("cheb-f32-ranks %-4s iterations %d (two ranks, 64 bits: %d) explicit residual %.2e" % (kind, info[32][1], info[64][1], eres))
    assert eres <= 1e-7
    if kind == "amg":
        assert abs(info[32][1] - info[64][1]) <= 1
        return
    A1 = hip.Matrix.from_csr(gpu_ctx, Ag.indptr.astype(np.int32), Ag.indices.astype(np.int32), Ag.data)
    M1 = hip.PrecondChebyshev(gpu_ctx, A1, degree=3, value_bits=32)
    g1, g32 = gap_max(z, M1.apply(rr)), gap_max(z, cr.cheb_apply(c32.fl32(Ag), rr, None, 3, 30.0))
    g64 = gap_max(z, cr.cheb_apply(Ag, rr, None, 3, 30.0))
    x1 = np.zeros(N)
    i1 = hip.solve(gpu_ctx, A1, bg.copy(), x1, prec=M1, singular=True)
    print("cheb-f32-ranks cheb apply against one rank %.2e, against fl32(A) %.2e, against A %.2e; one rank %d iterations" %
          (g1, g32, g64, i1.iters))
    assert g1 <= 1e-13 and g32 <= APPLY_TOL and g64 >= NOT_FP64
    assert i1.converged == 1 and info[32][1] == i1.iters
    M1.close(); A1.close()


# ---------------------------------------------------------------- 8. the C++ wrappers
def run_cpp(tmp_path, name, mode, bits):
    rp, ci, val, b, singular = system(name)[:5]
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_chebyshev_f32_test(), fin, fout, "1" if singular else "0", mode, str(bits)],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


@pytest.mark.parametrize("name,mode", [("tgv16", "ifpack"), ("wall42", "ifpack"), ("tgv16", "ml"), ("wall42", "ml")])
def test_wrappers_match_the_python_path(gpu_ctx, tmp_path, name, mode):
    r, xc = run_cpp(tmp_path, name, mode, 32)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rp, ci, val, b, singular = system(name)[:5]
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    if mode == "ifpack":
        M = hip.PrecondChebyshev(gpu_ctx, A, degree=3, ratio=30.0, value_bits=32)
    else:
        M = hip.PrecondAMG(gpu_ctx, A, nullvec=nullvec(name),
                           params=hip.AmgParams(coarse_max=64, block=256, smoother=2, sweeps=2, cheb_ratio=20.0, cheb_value_bits=32))
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=hip.SolverParams())
    M.close(); A.close()
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    conv, iters = (int(t.split("=")[1]) for t in line.split()[:2])
    g = np.linalg.norm(xc - x) / np.linalg.norm(x)
    print("cheb-f32-wrapper %-8s %-7s iterations %d (python %d) x gap %.2e" % (name, mode, iters, info.iters, g))
    assert conv == 1 and info.converged == 1 and iters == info.iters
    assert g <= 1e-6
    if mode == "ifpack":
        assert "32-bit matrix values" in r.stdout


@pytest.mark.parametrize("mode", ["ifpack", "ml"])
def test_wrappers_refuse_other_widths_and_name_the_key(tmp_path, mode):
    r, _ = run_cpp(tmp_path, "stencil", mode, 16)
    assert r.returncode == 1
    assert "isph: chebyshev value bits" in r.stderr and "not available" in r.stderr, r.stderr
