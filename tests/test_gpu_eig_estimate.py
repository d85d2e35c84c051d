"""-m gpu: the eigenvalue estimate behind isph_cheb_params::eig_type = 1 and isph_amg_params::eig_type = 1 -- k Arnoldi
steps on D^-1 A from a Philox start vector, clipped by rho = ||D^-1 A||_inf -- against the numpy restatement
tests/eig_estimate_reference.py.

Fixtures (chebyshev_reference.system): tgv16 (4096 rows, four 1024-column windows, singular), wall42 (1764 rows, a tail
slice), stencil (210 rows, nonsymmetric, one window), spd (1480 rows, three AMG levels).  The stand-alone preconditioner
walks the 16-bit windowed columns, the level operators of the AMG the 32-bit ones.

Bounds.  lambda of the device against the restatement: max(100 s, 1e-13) relative, s the rounding spread of the
restatement itself (plain, reversed and longdouble accumulation; tests/test_eig_estimate_reference.py) for the same
matrix and k.  Fused against ISPH_EIG_UNFUSED=1: 1e-14 (the project's fused / unfused gate).  One application: 1e-12 max
(APPLY_TOL of tests/test_gpu_chebyshev.py).  P_0 and A_1 rebuilt in numpy: 1e-12 max.  One AMG cycle: 1e-9 ||z|| (the
bound of tests/test_gpu_amg.py).  Converged solves: the restatement's iteration count.  Every gap is printed before it
is asserted.

Measured on an MI355X: lambda against the restatement 0 .. 1.9e-15 (k = 1: 0; stencil k = 50: 4.8e-16) under bounds of
1.0e-13 .. 1.5e-13 (s = 0 .. 1.5e-15); fused against unfused 0 in every case; a shuffled caller order renumbered by the
library 1.2e-16 .. 8.1e-16; applications 1.0e-16 .. 4.0e-15 (0.014 .. 0.80 away from the polynomial of the rho
interval); value_bits 32 against the restatement on fl32(A) 0 .. 1.4e-15, 6.5e-11 .. 1.2e-9 away from the one on A;
P_0 2.3e-16 .. 1.7e-15, A_1 3.6e-16 .. 2.6e-15, level estimates 0 .. 1.9e-15; cycles 1.9e-16 .. 8.6e-16; two ranks
against one 0, against the restatement 2.0e-16, 18 iterations either way.  Iterations, eig_type 0 -> 1, each the
restatement's count: "chebyshev3" tgv16 15 -> 18, wall42 38 -> 32; Chebyshev-2 AMG tgv16 14 -> 12, wall42 14 -> 12.
"""
import functools
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import build, hip
import chebyshev_reference as cr
import eig_estimate_reference as er
import krylov_reference as kr

pytestmark = pytest.mark.gpu

APPLY_TOL = 1e-12
FIXTURES = ["tgv16", "wall42", "stencil", "spd"]
AMG_FIXTURES = ["tgv16", "wall42", "spd"]
AMG_KW = dict(theta=0.0, block=256, coarse_max=64)
KS = list(range(1, 81))


@functools.lru_cache(maxsize=None)
def system(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    return rp, ci, val, b, singular, sps.csr_matrix((val, ci, rp), shape=(n, n))


@functools.lru_cache(maxsize=None)
def ref(name, k, f32=False):
    A = system(name)[5]
    return er.estimate(er.fl32(A) if f32 else A, k)


@functools.lru_cache(maxsize=None)
def bound(name, k, f32=False):
    A = system(name)[5]
    return max(100.0 * er.rounding_spread(er.fl32(A) if f32 else A, k), 1e-13)


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            rp, ci, val, _, _, _ = system(name)
            cache[name] = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        return cache[name]
    return get


def rhs(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def gap_max(z, zref):
    return float(np.max(np.abs(np.asarray(z) - zref)) / np.max(np.abs(zref)))


def nullvec(name):
    n = system(name)[5].shape[0]
    return np.ones(n) / np.sqrt(n) if system(name)[4] else None


def amg(ctx, A, name, **kw):
    return hip.PrecondAMG(ctx, A, nullvec=nullvec(name), params=hip.AmgParams(**dict(AMG_KW, **kw)))


# ---------------------------------------------------------------- 1. the device's lambda against the restatement
@pytest.mark.parametrize("name,k", [(nm, k) for nm in FIXTURES for k in (1, 5, 10)] + [("stencil", 50)])
def test_lambda_matches_the_restatement_fused_and_unfused(gpu_ctx, dev, monkeypatch, name, k):
    r = ref(name, k)
    M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=2, eig_type=1, eig_iters=k)
    e = M.eig_estimate()
    monkeypatch.setenv("ISPH_EIG_UNFUSED", "1")
    Mu = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=2, eig_type=1, eig_iters=k)
    monkeypatch.delenv("ISPH_EIG_UNFUSED")
    eu = Mu.eig_estimate()
    M.close(); Mu.close()
    g, gu = rel(e["lambda_used"], r["lambda_used"]), rel(e["lambda_used"], eu["lambda_used"])
    print("eig-lambda %-8s k %2d lambda %.15f restatement %.15f gap %.2e bound %.2e fused-unfused %.2e steps %d rho %.6f" %
          (name, k, e["lambda_used"], r["lambda_used"], g, bound(name, k), gu, e["steps"], e["rho"]))
    assert e["steps"] == r["steps"] == eu["steps"] == k
    assert rel(e["rho"], r["rho"]) <= 1e-14
    assert g <= bound(name, k)
    assert gu <= 1e-14
    assert e["lambda_used"] <= e["rho"]


def test_early_stop_and_more_steps_than_rows(gpu_ctx):
    """D^-1 A = I for a diagonal matrix: an invariant subspace after one step; k is cut to the row count"""
    n = 130
    d = 1.0 + np.arange(n) % 7
    A = hip.Matrix.from_csr(gpu_ctx, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d)
    M = hip.PrecondChebyshev(gpu_ctx, A, degree=2, eig_type=1, eig_iters=10)
    e = M.eig_estimate()
    assert e["steps"] == 1 and abs(e["lambda_used"] - 1.0) <= 1e-14 and e["rho"] == 1.0
    M.close(); A.close()
    n = 5
    T = sps.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    A = hip.Matrix.from_csr(gpu_ctx, T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data)
    M = hip.PrecondChebyshev(gpu_ctx, A, degree=2, eig_type=1, eig_iters=50)
    e, r = M.eig_estimate(), er.estimate(T, 50)
    assert e["steps"] == r["steps"] == n
    assert rel(e["lambda_used"], r["lambda_used"]) <= 1e-13 and rel(e["lambda_used"], er.true_lambda_max(T)) <= 1e-12
    M.close(); A.close()


# ---------------------------------------------------------------- 2. numbering independence
@pytest.mark.parametrize("name", ["stencil", "spd"])
def test_the_librarys_row_numbering_gives_the_callers_lambda(gpu_ctx_bricks, name):
    """the caller hands the rows over in a shuffled order (the fixtures' own order is already the lattice order the
    library would choose); the library renumbers them by position, and the start vector still follows the caller's rows"""
    A_h = system(name)[5]
    n = A_h.shape[0]
    xyz, dim = cr.coordinates(name)
    q = np.random.default_rng(17).permutation(n)
    As = A_h[q][:, q].tocsr()
    As.sort_indices()
    Ab = hip.Matrix.from_host_csr_with_coords(gpu_ctx_bricks, As.indptr.astype(np.int32), As.indices.astype(np.int32), As.data,
                                              np.ascontiguousarray(xyz[q]), dim=dim)
    assert Ab.ordering() is not None and not np.array_equal(Ab.ordering()["perm"], np.arange(n))
    for k in (5, 10):
        Mb = hip.PrecondChebyshev(gpu_ctx_bricks, Ab, degree=2, eig_type=1, eig_iters=k)
        e, r = Mb.eig_estimate(), er.estimate(As, k)
        b = max(100.0 * er.rounding_spread(As, k), 1e-13)
        g = rel(e["lambda_used"], r["lambda_used"])
        print("eig-bricks %-8s k %2d gap %.2e bound %.2e" % (name, k, g, b))
        assert g <= b and e["steps"] == k
        Mb.close()
    Ab.close()


# ---------------------------------------------------------------- 3. applications
@pytest.mark.parametrize("name", FIXTURES)
def test_apply_is_the_polynomial_of_the_estimated_interval(gpu_ctx, dev, name):
    A_h = system(name)[5]
    r = rhs(A_h.shape[0])
    for d in (1, 2, 3, 7):
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, ratio=30.0, eig_type=1)
        lam = M.eig_estimate()["lambda_used"]
        g = gap_max(M.apply(r), cr.cheb_apply(A_h, r, None, d, 30.0, lam=lam))
        g_rho = gap_max(M.apply(r), cr.cheb_apply(A_h, r, None, d, 30.0))
        print("eig-apply %-8s degree %d gap %.2e (against the rho interval %.2e)" % (name, d, g, g_rho))
        assert g <= APPLY_TOL
        assert g_rho > 1e-3       # not the polynomial of [rho / 30, 1.1 rho]
        M.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_value_bits_32_estimates_the_rounded_matrix(gpu_ctx, dev, name):
    k = 10
    M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3, value_bits=32, eig_type=1, eig_iters=k)
    e = M.eig_estimate()
    g32, g64 = rel(e["lambda_used"], ref(name, k, True)["lambda_used"]), rel(e["lambda_used"], ref(name, k)["lambda_used"])
    print("eig-f32 %-8s gap to fl32(A) %.2e bound %.2e gap to A %.2e" % (name, g32, bound(name, k, True), g64))
    assert M.value_bits == 32
    assert g32 <= bound(name, k, True)
    assert g64 > max(bound(name, k, True), bound(name, k))
    A32 = er.fl32(system(name)[5])
    r = rhs(A32.shape[0], 6)
    assert gap_max(M.apply(r), cr.cheb_apply(A32, r, None, 3, 30.0, lam=e["lambda_used"])) <= APPLY_TOL
    M.close()


# ---------------------------------------------------------------- 4. the hierarchy
@pytest.mark.parametrize("name", AMG_FIXTURES)
def test_amg_hierarchy_is_damped_by_the_estimate(gpu_ctx, dev, name):
    A_h = system(name)[5]
    n = A_h.shape[0]
    M1 = amg(gpu_ctx, dev(name), name, smoother=2, sweeps=2, eig_type=1)
    M0 = amg(gpu_ctx, dev(name), name, smoother=2, sweeps=2)
    assert M1.levels >= 2 and M0.levels >= 2
    assert np.array_equal(M1.aggregates(0), M0.aggregates(0))
    levels = cr.levels_from(M1, n)
    lam0 = M1.eig_estimate(0)
    nv = nullvec(name)
    Pt = er.tentative_prolongator(M1.aggregates(0), np.ones(n) if nv is None else nv, levels[0][1].shape[1])
    P_ref = er.smoothed_prolongator(A_h, Pt, 4.0 / 3.0, lam0["lambda_used"])
    gp = float(abs(levels[0][1] - P_ref).max() / abs(P_ref).max())
    A1_ref = (levels[0][1].T @ A_h @ levels[0][1]).tocsr()
    ga = float(abs(levels[1][0] - A1_ref).max() / abs(A1_ref).max())
    P_rho = er.smoothed_prolongator(A_h, Pt, 4.0 / 3.0, lam0["rho"])
    print("eig-amg %-8s levels %d P_0 gap %.2e A_1 gap %.2e (P_0 against the rho damping %.2e)" %
          (name, M1.levels, gp, ga, float(abs(levels[0][1] - P_rho).max() / abs(P_rho).max())))
    assert gp <= 1e-12 and ga <= 1e-12
    assert abs(levels[0][1] - P_rho).max() > 1e-3 * abs(P_rho).max()
    P0_0 = cr.levels_from(M0, n)[0][1]
    assert abs(P0_0 - P_rho).max() <= 1e-12 * abs(P_rho).max()       # eig_type 0 still damps with rho
    for l, (A_l, _) in enumerate(levels):
        e, r = M1.eig_estimate(l), er.estimate(A_l, 10, level=l)
        b = max(100.0 * er.rounding_spread(A_l, 10, level=l), 1e-13)
        g = rel(e["lambda_used"], r["lambda_used"])
        print("eig-amg %-8s level %d rows %d lambda %.6f rho %.6f steps %d gap %.2e bound %.2e" %
              (name, l, A_l.shape[0], e["lambda_used"], e["rho"], e["steps"], g, b))
        assert g <= b and e["steps"] == r["steps"] and rel(e["rho"], r["rho"]) <= 1e-13
        e0 = M0.eig_estimate(l)
        assert e0["steps"] == 0 and e0["lambda_used"] == e0["rho"]
    M1.close(); M0.close()


# ---------------------------------------------------------------- 5. one cycle
@pytest.mark.parametrize("name", AMG_FIXTURES)
def test_one_cycle_matches_the_restated_cycle_with_the_levels_lambda(gpu_ctx, dev, name):
    A_h, singular = system(name)[5], system(name)[4]
    n = A_h.shape[0]
    r = rhs(n, 10)
    M = amg(gpu_ctx, dev(name), name, smoother=2, sweeps=2, eig_type=1)
    levels = cr.levels_from(M, n)
    lams = [M.eig_estimate(l)["lambda_used"] for l in range(M.levels)]
    z, zr = M.apply(r), er.amg_vcycle(levels, lams, r, sweeps=2, ratio=20.0, coarse_polynomial=singular)
    g2 = float(np.linalg.norm(z - zr) / np.linalg.norm(zr))
    z_rho = cr.amg_vcycle(levels, r, sweeps=2, ratio=20.0, coarse_polynomial=singular)
    M.close()
    M = amg(gpu_ctx, dev(name), name, smoother=0, sweeps=1, eig_type=1)
    levels = cr.levels_from(M, n)
    z0, z0r = M.apply(r), er.amg_vcycle_sgs(levels, r, sweeps=1, block=256, coarse_smooth=singular)
    g0 = float(np.linalg.norm(z0 - z0r) / np.linalg.norm(z0r))
    M.close()
    print("eig-cycle %-8s smoother 2 gap %.2e smoother 0 gap %.2e" % (name, g2, g0))
    assert g2 <= 1e-9 and g0 <= 1e-9
    assert np.linalg.norm(z - z_rho) > 1e-3 * np.linalg.norm(z)      # not the cycle of the rho intervals


# ---------------------------------------------------------------- 6. solves
def solver_params(k=500, tol=1e-8):
    return hip.SolverParams(solver_type=0, num_blocks=50, max_iters=k, max_restarts=10 ** 6, tol=tol)


def make_prec(ctx, A, name, kind, eig_type):
    if kind == "cheb":
        return hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0, eig_type=eig_type)
    return amg(ctx, A, name, smoother=2, sweeps=2, eig_type=eig_type)


@pytest.mark.parametrize("name,kind", [("tgv16", "cheb"), ("wall42", "cheb"), ("tgv16", "amg"), ("wall42", "amg")])
def test_solves_converge_on_the_restatements_count(gpu_ctx, dev, name, kind):
    _, _, _, b, singular, A_h = system(name)
    n = A_h.shape[0]
    A = dev(name)
    counts = {}
    for eig_type in (0, 1):
        M = make_prec(gpu_ctx, A, name, kind, eig_type)
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=solver_params())
        assert info.converged == 1
        counts[eig_type] = info.iters
        if eig_type == 1:
            if kind == "cheb":
                minv = cr.cheb_minv(A_h, 3, 30.0, lam=M.eig_estimate()["lambda_used"])
            else:
                lams = [M.eig_estimate(l)["lambda_used"] for l in range(M.levels)]
                minv = er.amg_minv(cr.levels_from(M, n), lams, sweeps=2, ratio=20.0, coarse_polynomial=singular)
            refit = kr.gmres_iterates(A_h, b, np.zeros(n), KS, 50, minv, kr.unit_null(None, n) if singular else None)
            kref = cr.first_below(refit, 1e-8)
            gx = kr.iterate_gap(x, refit[info.iters].x) if info.iters in refit else np.inf
        M.close()
    print("eig-solve %-8s %-4s iterations eig_type 0: %d, eig_type 1: %d (restatement %s) x gap %.2e" %
          (name, kind, counts[0], counts[1], kref, gx))
    assert kref is not None and counts[1] == kref
    assert gx <= 1e-6


# ---------------------------------------------------------------- 7. defaults change nothing
def test_defaults_and_an_explicit_lambda_max_keep_todays_bits(gpu_ctx, dev):
    assert hip.ChebParams().eig_type == 0 and hip.ChebParams().eig_iters == 10
    assert hip.AmgParams().eig_type == 0 and hip.AmgParams().eig_iters == 10
    name = "wall42"
    A_h = system(name)[5]
    n = A_h.shape[0]
    r = rhs(n, 12)
    base = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3)
    zb = base.apply(r)
    e = base.eig_estimate()
    assert e["steps"] == 0 and e["lambda_used"] == e["rho"] and rel(e["rho"], cr.rho_anorm(A_h)) <= 1e-14
    assert gap_max(zb, cr.cheb_apply(A_h, r, None, 3, 30.0)) <= APPLY_TOL
    for kw in (dict(eig_type=0, eig_iters=7), dict(eig_type=0, eig_iters=50)):
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3, **kw)
        assert np.array_equal(M.apply(r), zb)
        M.close()
    base.close()
    Ms = hip.Precond(gpu_ctx, dev(name), "chebyshev3", 0)               # the string form keeps eig_type 0
    assert np.array_equal(Ms.apply(r), zb) and Ms.eig_estimate()["steps"] == 0
    Ms.close()
    # an explicit lambda_max wins over eig_type 1
    Ma = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3, lambda_max=1.7, eig_type=0)
    Mb = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3, lambda_max=1.7, eig_type=1)
    assert np.array_equal(Ma.apply(r), Mb.apply(r)) and Mb.eig_estimate()["steps"] == 0
    Ma.close(); Mb.close()
    # the hierarchy and the cycle of untouched fields against eig_type 0 spelled out, and through "sa-amg"
    G0 = amg(gpu_ctx, dev(name), name, smoother=2, sweeps=2)
    G1 = amg(gpu_ctx, dev(name), name, smoother=2, sweeps=2, eig_type=0, eig_iters=33)
    assert G0.levels == G1.levels
    for l in range(G0.levels):
        for what in ("A", "P") if l < G0.levels - 1 else ("A",):
            for a, b in zip(G0.export(l, what), G1.export(l, what)):
                assert np.array_equal(a, b)
        e = G0.eig_estimate(l)
        assert e["steps"] == 0 and e["lambda_used"] == e["rho"]
    assert rel(G0.eig_estimate(0)["rho"], cr.rho_anorm(A_h)) <= 1e-14
    assert np.array_equal(G0.apply(r), G1.apply(r))
    G0.close(); G1.close()
    Gs = hip.Precond(gpu_ctx, dev(name), "sa-amg", 256)
    assert Gs.eig_estimate(0)["steps"] == 0
    Gs.close()


# ---------------------------------------------------------------- 8. refusals
def test_parameter_errors(gpu_ctx, dev):
    A = dev("stencil")
    with pytest.raises(hip.IsphError, match="eig_type"):
        hip.PrecondChebyshev(gpu_ctx, A, degree=2, eig_type=2)
    with pytest.raises(hip.IsphError, match="eig_type"):
        hip.PrecondChebyshev(gpu_ctx, A, degree=2, eig_type=-1)
    for it in (0, 51):
        with pytest.raises(hip.IsphError, match="eig_iters"):
            hip.PrecondChebyshev(gpu_ctx, A, degree=2, eig_type=1, eig_iters=it)
        with pytest.raises(hip.IsphError, match="eig_iters"):
            hip.PrecondAMG(gpu_ctx, dev("wall42"), params=hip.AmgParams(eig_type=1, eig_iters=it, **AMG_KW))
    with pytest.raises(hip.IsphError, match="eig_type"):
        hip.PrecondAMG(gpu_ctx, dev("wall42"), params=hip.AmgParams(eig_type=2, **AMG_KW))
    M = hip.PrecondChebyshev(gpu_ctx, A, degree=2, eig_type=1)
    for level in (-1, 1):
        with pytest.raises(hip.IsphError, match="level out of range"):
            M.eig_estimate(level)
    M.close()
    G = hip.PrecondAMG(gpu_ctx, dev("wall42"), params=hip.AmgParams(eig_type=1, **AMG_KW))
    for level in (-1, G.levels):
        with pytest.raises(hip.IsphError, match="level out of range"):
            G.eig_estimate(level)
    G.close()
    ilu = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 64)
    with pytest.raises(hip.IsphError, match="not a Chebyshev or an AMG"):
        ilu.eig_estimate()
    ilu.close()


# ---------------------------------------------------------------- 9. two thread ranks on one GPU
def _rank_estimate(rank, G, dim, pgrid, n):
    import oracle as orc
    import test_gpu_ranks as tr
    st = tr._rank_setup(rank, G, dim, pgrid, n, orc.NULLSPACE)
    ctx, A = st["ctx"], st["A"]
    try:
        nl = st["nl"]
        M = hip.PrecondChebyshev(ctx, A, degree=3, eig_type=1)                # collective: dots and norms are all-reduced
        e = M.eig_estimate()
        x, bb = np.zeros(nl), st["b"].copy()
        info = hip.solve(ctx, A, bb, x, prec=M, singular=True)
        M.close()
        return dict(nl=nl, rtag=st["rtag"], col_tag=st["col_tag"], csr=st["csr"], b=st["b"], x=x, eig=e,
                    info=(info.converged, info.iters))
    finally:
        A.close()
        ctx.close()


def test_two_ranks_estimate_the_global_operator(gpu_ctx):
    from ranks import RankGroup
    from test_gpu_chebyshev import _global_system
    dim, pgrid, n = 3, (2, 1, 1), 8
    G = RankGroup(2)
    try:
        res = G.run(_rank_estimate, dim, pgrid, n)
    finally:
        G.close()
    Ag, bg = _global_system(res)
    N = Ag.shape[0]
    assert res[0]["eig"] == res[1]["eig"]
    e2 = res[0]["eig"]
    r = er.estimate(Ag, 10)
    b = max(100.0 * er.rounding_spread(Ag, 10), 1e-13)
    A1 = hip.Matrix.from_csr(gpu_ctx, Ag.indptr.astype(np.int32), Ag.indices.astype(np.int32), Ag.data)
    M1 = hip.PrecondChebyshev(gpu_ctx, A1, degree=3, eig_type=1)
    e1 = M1.eig_estimate()
    x1 = np.zeros(N)
    i1 = hip.solve(gpu_ctx, A1, bg.copy(), x1, prec=M1, singular=True)
    g1, gr = rel(e2["lambda_used"], e1["lambda_used"]), rel(e2["lambda_used"], r["lambda_used"])
    infos = {q["info"] for q in res}
    print("eig-ranks lambda 2 ranks %.15f one rank %.15f gap %.2e restatement gap %.2e bound %.2e iterations %s (one rank %d)" %
          (e2["lambda_used"], e1["lambda_used"], g1, gr, b, sorted(infos), i1.iters))
    assert g1 <= b and gr <= b and e2["steps"] == e1["steps"] == 10
    assert infos == {(1, i1.iters)} and i1.converged == 1
    M1.close(); A1.close()


# ---------------------------------------------------------------- 10. the wrappers' keys
def run_cpp(tmp_path, name, mode):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_eig_estimate_test(), fin, fout, "1" if singular else "0", mode],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


@pytest.mark.parametrize("name,mode", [("wall42", "ml-cg"), ("tgv16", "ml-cg5"), ("wall42", "ml-anorm"), ("wall42", "ifpack-arnoldi")])
def test_wrapper_keys_give_the_c_abi_counts(gpu_ctx, tmp_path, name, mode):
    r, xc = run_cpp(tmp_path, name, mode)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rp, ci, val, b, singular, _ = system(name)
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    if mode.startswith("ml"):
        M = amg(gpu_ctx, A, name, smoother=2, sweeps=2, cheb_ratio=20.0, eig_type=0 if mode == "ml-anorm" else 1,
                eig_iters=5 if mode == "ml-cg5" else 10)
    else:
        M = hip.PrecondChebyshev(gpu_ctx, A, degree=3, ratio=30.0, eig_type=1)
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular)
    M.close(); A.close()
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    conv, iters = (int(t.split("=")[1]) for t in line.split()[:2])
    print("eig-wrapper %-8s %-14s iterations %d (C ABI %d) x gap %.2e" % (name, mode, iters, info.iters, np.linalg.norm(xc - x) / np.linalg.norm(x)))
    assert conv == 1 and info.converged == 1 and iters == info.iters
    assert np.linalg.norm(xc - x) <= 1e-6 * np.linalg.norm(x)


@pytest.mark.parametrize("mode,names", [("ml-bad", ['"Anorm"', '"cg"', "power-method"]), ("ifpack-bad", ['"Anorm"', '"arnoldi"'])])
def test_unknown_eigen_analysis_types_are_reported_as_not_available(tmp_path, mode, names):
    r, _ = run_cpp(tmp_path, "stencil", mode)
    assert r.returncode == 1
    assert "not available" in r.stderr
    for nm in names:
        assert nm in r.stderr, r.stderr
