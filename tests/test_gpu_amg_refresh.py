"""-m gpu: isph_prec_refactor of "sa-amg" and "chebyshev<d>" -- the hierarchy (the polynomial) of new matrix values, with the
aggregates, the patterns and the layouts of the create call kept (csrc/amg.hpp amg_refactor; ML's ReComputePreconditioner).

What is compared with what:
  1. where a fresh create on the new values aggregates as the kept hierarchy does, the refresh IS that create to round-off
     (bounds of test_amg_fallback_kernels_build_the_same_hierarchy and test_amg_hierarchy_cycle_and_solve_match_oracle);
  2. for general new values the refresh is the hierarchy of those values on the kept aggregates: against
     tests/amg_refresh_reference.py fed the exported aggregates;
  3. the same on the constructed graphs of tests/amg_shapes.py that put the rows of P, A P and P^T A P on every width the
     refresh kernels treat differently, and against the two-pass kernels (ISPH_AMG_REFRESH_TWO_PASS=1);
  4. two refreshes from the same values give the same bits;
  5. what is refused, by name, and that the hierarchy and the pool survive it;
  6. with the mode off a create reserves what it reserved before;
  7. the Chebyshev polynomial, bit for bit."""
import contextlib
import functools

import numpy as np
import pytest

from isph_amd import hip, workload
import oracle as orc
import amg_refresh_reference as arr
import amg_shapes as S
from problems import Problem, tgv_spec, wall_types

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def held(ctx):
    ctx.hold_pattern(True)
    try:
        yield
    finally:
        ctx.hold_pattern(False)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


SPECS = {"3d": dict(dim=3, n=16, mode=workload.ADVECT, brick=8), "2d": dict(dim=2, n=48, mode=workload.JITTER, brick=8)}
SYSTEMS = [("3d", True), ("3d", False), ("2d", True), ("2d", False)]


@functools.lru_cache(maxsize=None)
def system(name, singular):
    """(rp, ci, val, b, nullvec): the pressure Poisson system of the oracle; singular with its null vector, or NotSingular with
    a solid wall (a direct coarse solve)"""
    if singular:
        pr = Problem(tgv_spec(**SPECS[name]))
    else:
        pr = Problem(tgv_spec(**SPECS[name]), singular=orc.NOT_SINGULAR, kinds=[orc.FLUID, orc.SOLID], types=wall_types)
    rp, ci, val, b = pr.poisson()
    nv = np.ones(pr.n) / np.sqrt(pr.n) if singular else None
    for a in (rp, ci, val, b):
        a.setflags(write=False)
    return rp, ci, val, b, nv


def scaled_values(rp, ci, val):
    """off-diagonal entries x 2.5, the diagonal x 1.7 + a shift: the order of a row's off-diagonal couplings stands and the
    diagonal does not enter the aggregation (pass 2 picks the strongest coupling), so a fresh create aggregates level 0 alike.
    The shift is the largest diagonal entry: 1.7 d + shift > 2.5 d keeps the rows diagonally dominant (and the matrix regular,
    so the solves below run without the null-space projection)"""
    diag = ci == rows_of(rp)
    v = np.where(diag, 1.7 * val + np.abs(val[diag]).max(), 2.5 * val)
    return np.ascontiguousarray(v)


def general_values(rp, ci, val, seed=11, shift=0.05):
    """every off-diagonal entry x (1 + 0.3 u), u uniform in [-1, 1]; the diagonal = -(sum of the row's off-diagonals) + a shift
    (a fraction of the mean diagonal: the matrix is not singular)"""
    rows = rows_of(rp)
    diag = ci == rows
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, len(val))
    v = np.where(diag, 0.0, val * (1.0 + 0.3 * u))
    s = np.zeros(len(rp) - 1)
    np.add.at(s, rows, v)
    ref = np.abs(val[diag]).mean() if diag.any() else 1.0
    d = -s + shift * (ref if ref > 0 else 1.0)
    return np.ascontiguousarray(np.where(diag, d[rows], v))


def exports(M):
    out = []
    for l in range(M.levels):
        out.append(dict(A=M.export(l, "A"), P=M.export(l, "P") if l < M.levels - 1 else None,
                        agg=M.aggregates(l) if l < M.levels - 1 else None, info=M.level_info(l)))
    return out


def close(*objs):
    for o in objs:
        o.close()


# ---------------------------------------------------------------------------------------------------- 1
VARIANTS = {
    "sgs": dict(smoother=0),
    "gs_eff": dict(smoother=1),
    "cheb": dict(smoother=2, sweeps=2),
    "ilu0": dict(smoother=4, ilu_fill=0),
    "ilu1": dict(smoother=4, ilu_fill=1),
    "cheb_f32": dict(smoother=2, sweeps=2, cheb_value_bits=32),
    "cycle_f32": dict(smoother=2, sweeps=2, cycle_bits=32),
    "cheb_eig": dict(smoother=2, sweeps=2, eig_type=1),
    "sgs_eig": dict(smoother=0, eig_type=1),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,singular", SYSTEMS)
def test_refresh_equals_a_fresh_create_where_the_aggregates_agree(gpu_ctx, name, singular, variant):
    rp, ci, val, b, nv = system(name, singular)
    n = len(rp) - 1
    val2 = scaled_values(rp, ci, val)
    kw = dict(block=256, coarse_max=64, **VARIANTS[variant])
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=hip.AmgParams(**kw))
    kept = [M.aggregates(l) for l in range(M.levels - 1)]
    paths = [M.path(l) for l in range(M.levels)]
    assert M.refreshes == 0
    A.update_values(val2)
    M.refactor(A)
    assert M.refreshes == 1 and M.levels >= 2
    assert [M.path(l) for l in range(M.levels)] == paths
    A2 = hip.Matrix.from_csr(gpu_ctx, rp, ci, val2)
    F = hip.PrecondAMG(gpu_ctx, A2, nullvec=nv, params=hip.AmgParams(**kw))
    assert F.levels == M.levels
    assert np.array_equal(F.aggregates(0), kept[0])                       # first: level 0 aggregates alike
    agree = 1
    while agree < M.levels - 1 and np.array_equal(F.aggregates(agree), kept[agree]):
        agree += 1
    compared = max(2, agree + 1)                                          # levels 0 and 1 always
    for l in range(min(compared, M.levels)):
        assert M.level_info(l) == F.level_info(l)
        whats = ("A", "P") if (l < M.levels - 1 and l < agree) else ("A",)
        for what in whats:
            r0, c0, v0 = F.export(l, what)
            r1, c1, v1 = M.export(l, what)
            assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (l, what)
            err = np.max(np.abs(v0 - v1)) / np.abs(v0).max()
            print("%s %s level %d %s: %.3g" % (name, variant, l, what, err))
            assert err <= 1e-12, (l, what, err)
    assert agree == M.levels - 1, "deeper aggregates differ (%d of %d levels agree): the cycles are not comparable" % (agree, M.levels - 1)
    r = np.random.default_rng(4).standard_normal(n)
    z0, z1 = np.array(F.apply(r)), np.array(M.apply(r))
    zerr = np.linalg.norm(z0 - z1) / np.linalg.norm(z0)
    print("%s %s cycle: %.3g" % (name, variant, zerr))
    assert zerr <= 1e-10
    x0, x1 = np.zeros(n), np.zeros(n)
    i0 = hip.solve(gpu_ctx, A2, b.copy(), x0, prec=F)
    i1 = hip.solve(gpu_ctx, A, b.copy(), x1, prec=M)
    assert i0.converged == 1 and i1.converged == 1 and abs(i0.iters - i1.iters) <= 1, (i0.iters, i1.iters)
    assert np.linalg.norm(x0 - x1) <= 1e-6 * np.linalg.norm(x0)
    close(M, F, A, A2)


# ---------------------------------------------------------------------------------------------------- 2, 3
def refresh_against_helper(ctx, rp, ci, val, val2, nv, kw, label):
    """create on val while the pattern is held, refresh on val2: aggregates and patterns stand, the values are the helper's"""
    with held(ctx):
        A = hip.Matrix.from_csr(ctx, rp, ci, val)
        M = hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(**kw))
    before = exports(M)
    A.update_values(val2)
    M.refactor(A)
    after = exports(M)
    assert len(after) == len(before) >= 2
    for l, (x, y) in enumerate(zip(before, after)):
        assert x["info"] == y["info"]
        assert np.array_equal(x["A"][0], y["A"][0]) and np.array_equal(x["A"][1], y["A"][1])
        if x["P"] is not None:
            assert np.array_equal(x["agg"], y["agg"])
            assert np.array_equal(x["P"][0], y["P"][0]) and np.array_equal(x["P"][1], y["P"][1])
    ref = arr.hierarchy(rp, ci, val2, [x["agg"] for x in after[:-1]], nullvec=nv, omega=kw.get("omega", 4.0 / 3.0))
    for l, (g, h) in enumerate(zip(after, ref)):
        assert np.array_equal(g["A"][0], h["A"][0]) and np.array_equal(g["A"][1], h["A"][1]), (label, l)
        ea = np.max(np.abs(g["A"][2] - h["A"][2])) / np.abs(h["A"][2]).max()
        print("%s level %d A: %.3g" % (label, l, ea))
        assert ea <= 1e-11, (label, l, ea)
        if g["P"] is not None:
            assert np.array_equal(g["P"][0], h["P"][0]) and np.array_equal(g["P"][1], h["P"][1]), (label, l)
            ep = np.max(np.abs(g["P"][2] - h["P"][2])) / np.abs(h["P"][2]).max()
            print("%s level %d P: %.3g" % (label, l, ep))
            assert ep <= 1e-12, (label, l, ep)
    return A, M, after


@pytest.mark.parametrize("name,singular", [("3d", True), ("2d", False)])
def test_general_new_values_on_the_kept_aggregates(gpu_ctx, name, singular):
    rp, ci, val, b, nv = system(name, singular)
    n = len(rp) - 1
    val2 = general_values(rp, ci, val)
    kw = dict(block=256, coarse_max=64)
    A, M, _ = refresh_against_helper(gpu_ctx, rp, ci, val, val2, nv, kw, name)
    # the shifted matrix is not singular; both solves run to 1e-11 so that their x agree beyond the bound asked for
    prm_o, prm_g = orc.SolverParams(tol=1e-11), hip.SolverParams(tol=1e-11)
    xo, io_, _ = orc.solve(rp, ci, val2, b, prec="amg", amg=orc.AMG(rp, ci, val2, block=256, coarse_max=64), params=prm_o)
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, params=prm_g)
    assert info.converged == 1 and io_.converged == 1
    assert np.linalg.norm(x - xo) <= 1e-6 * np.linalg.norm(xo)
    close(M, A)


LADDER = ["hub_16", "hub_17", "hub_64", "hub_65", "hub_257", "shared_hubs_40x64", "star_1100", "unsymmetric_150",
          "masked_grid_21x13", "long_chain_15200", "islands_16"]
# three levels: the refresh of level 1 starts from a coarse operator it has just written (the systems above stop at two)
DEEP = ["chain_257", "ring_192"]


@pytest.mark.parametrize("name", LADDER + DEEP)
def test_width_ladders_of_the_refresh_kernels(gpu_ctx, monkeypatch, name):
    (rp, ci, val), nv, prm = S.fixture(name)
    rp, ci = np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32)
    val = np.asarray(val, dtype=np.float64)
    n = len(rp) - 1
    val2 = general_values(rp, ci, val, seed=5, shift=0.25)
    A, M, new = refresh_against_helper(gpu_ctx, rp, ci, val, val2, nv, dict(prm), name)
    assert M.levels >= (3 if name in DEEP else 2)
    r = np.random.default_rng(6).standard_normal(n)
    z_new = np.array(M.apply(r))
    monkeypatch.setenv("ISPH_AMG_REFRESH_TWO_PASS", "1")
    M.refactor(A)
    monkeypatch.delenv("ISPH_AMG_REFRESH_TWO_PASS")
    assert M.refreshes == 2
    two = exports(M)
    for l, (x, y) in enumerate(zip(new, two)):
        for what in ("A", "P"):
            if x[what] is None:
                continue
            assert np.array_equal(x[what][0], y[what][0]) and np.array_equal(x[what][1], y[what][1])
            e = np.max(np.abs(x[what][2] - y[what][2])) / np.abs(x[what][2]).max()
            print("%s level %d %s against the two passes: %.3g" % (name, l, what, e))
            assert e <= 1e-12, (name, l, what, e)
    z_two = np.array(M.apply(r))
    assert np.linalg.norm(z_new - z_two) <= 1e-10 * np.linalg.norm(z_new)
    close(M, A)


# ---------------------------------------------------------------------------------------------------- 4
def state_bits(M, r):
    out = [bits(M.apply(r))]
    for x in exports(M):
        out.append(bits(x["A"][2]))
        if x["P"] is not None:
            out.append(bits(x["P"][2]))
    return out


def same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", ["sgs", "cheb_eig", "ilu1", "cycle_f32"])
def test_two_refreshes_from_the_same_values_give_the_same_bits(gpu_ctx, variant):
    rp, ci, val, b, nv = system("3d", True)
    n = len(rp) - 1
    val2 = general_values(rp, ci, val, seed=3)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=hip.AmgParams(block=256, coarse_max=64, **VARIANTS[variant]))
    r = np.random.default_rng(8).standard_normal(n)
    M.refactor(A)
    first = state_bits(M, r)
    A.update_values(val2)
    M.refactor(A)
    t1 = state_bits(M, r)
    A.update_values(val2)
    M.refactor(A)
    t2 = state_bits(M, r)
    assert same_state(t1, t2) and not same_state(t1, first)
    A.update_values(val)
    M.refactor(A)
    assert same_state(state_bits(M, r), first)
    assert M.refreshes == 4
    close(M, A)


# ---------------------------------------------------------------------------------------------------- 5
def untouched_coupling(rp, ci, agg):
    """(row, column): a column in an aggregate that no entry of the row (nor the row itself) belongs to"""
    n = len(rp) - 1
    for i in range(n):
        mine = set(agg[ci[rp[i]:rp[i + 1]]].tolist()) | {int(agg[i])}
        for j in range(n):
            if agg[j] >= 0 and int(agg[j]) not in mine:
                return i, j
    raise AssertionError("every row touches every aggregate")


def test_refusals_by_name_leave_the_hierarchy_and_the_pool_as_they_were(gpu_ctx):
    rp, ci, val, b, nv = system("2d", True)
    n = len(rp) - 1
    prm = hip.AmgParams(block=256, coarse_max=64)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    r = np.random.default_rng(2).standard_normal(n)
    # created with the mode off
    M0 = hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=prm)
    z0 = np.array(M0.apply(r))
    live = hip.pool_info()["live"]
    with pytest.raises(hip.IsphError, match="created while the pattern was not held"):
        M0.refactor(A)
    assert hip.pool_info()["live"] <= live and np.array_equal(bits(M0.apply(r)), bits(z0)) and M0.refreshes == 0
    with held(gpu_ctx):
        Ah = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondAMG(gpu_ctx, Ah, nullvec=nv, params=prm)
        Mn = hip.PrecondAMG(gpu_ctx, Ah, params=hip.AmgParams(block=256, coarse_max=64, max_levels=2))
    M.refactor(Ah)
    z = np.array(M.apply(r))
    # another row count
    (rp3, ci3, v3), _, _ = S.fixture("grid_21x13")
    A3 = hip.Matrix.from_csr(gpu_ctx, np.asarray(rp3, dtype=np.int32), np.asarray(ci3, dtype=np.int32), np.asarray(v3, dtype=np.float64))
    live = hip.pool_info()["live"]
    with pytest.raises(hip.IsphError, match="%d rows" % (len(rp3) - 1)):
        M.refactor(A3)
    assert hip.pool_info()["live"] <= live
    # one more coupling, into an aggregate the row did not touch
    i, j = untouched_coupling(rp, ci, M.aggregates(0))
    at = int(np.searchsorted(ci[rp[i]:rp[i + 1]], j)) + int(rp[i])
    rp4 = np.asarray(rp).copy()
    rp4[i + 1:] += 1
    A4 = hip.Matrix.from_csr(gpu_ctx, rp4.astype(np.int32), np.insert(ci, at, j).astype(np.int32), np.insert(val, at, -0.125))
    live = hip.pool_info()["live"]
    with pytest.raises(hip.IsphError, match="level 0, row %d " % i):
        M.refactor(A4)
    assert hip.pool_info()["live"] <= live
    M.refactor(Ah)                                                         # valid for another refactor: the bits of before
    assert np.array_equal(bits(M.apply(r)), bits(z))
    # no null vector at create, none later
    live = hip.pool_info()["live"]
    with pytest.raises(hip.IsphError, match="created without a null vector"):
        Mn.set_nullvec(np.ones(n))
    assert hip.pool_info()["live"] <= live
    M.set_nullvec(np.ones(n) / np.sqrt(n))                                 # the same vector again: the same hierarchy
    M.refactor(Ah)
    assert np.array_equal(bits(M.apply(r)), bits(z))
    x = np.zeros(n)
    assert hip.solve(gpu_ctx, Ah, b.copy(), x, prec=M, singular=True).converged == 1   # the context is usable
    close(M0, M, Mn, A, Ah, A3, A4)


def test_set_nullvec_is_read_by_the_next_refactor(gpu_ctx):
    rp, ci, val, b, nv = system("2d", True)
    n = len(rp) - 1
    nv2 = 1.0 + 0.5 * np.cos(np.arange(n) * 0.37)
    kw = dict(block=256, coarse_max=64)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=hip.AmgParams(**kw))
    M.set_nullvec(nv2)
    M.refactor(A)
    ref = arr.hierarchy(rp, ci, val, [M.aggregates(l) for l in range(M.levels - 1)], nullvec=nv2)
    for l in range(M.levels - 1):
        g = M.export(l, "P")
        assert np.array_equal(g[1], ref[l]["P"][1])
        assert np.max(np.abs(g[2] - ref[l]["P"][2])) <= 1e-12 * np.abs(ref[l]["P"][2]).max()
    close(M, A)


# ---------------------------------------------------------------------------------------------------- 6
PARENT_LIVE_BYTES = {"sgs": 17410708, "cheb": 2123184}


@pytest.mark.parametrize("variant", ["sgs", "cheb"])
def test_hold_off_reserves_what_the_create_call_reserved_before(gpu_ctx, variant):
    """With the mode off the create call keeps nothing for a refresh.  The bytes an SA-AMG of the 3-D system holds after
    create (pool `live` after minus before, from an emptied pool so that every block has its exact size) are compared with
    the figure of the commit before this feature, measured once there with this very sequence of calls:
        smoother 0: 17 410 708 bytes        smoother 2, degree 2: 2 123 184 bytes        (MI355X, one run, 2026-10-20)
    With the mode on the same call holds more (the member lists, the pattern of A P, the transposition map)."""
    rp, ci, val, b, nv = system("3d", True)
    prm = hip.AmgParams(block=256, coarse_max=64, **VARIANTS[variant])
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    gpu_ctx.sync()
    hip.pool_trim()
    base = hip.pool_info()["live"]
    M = hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=prm)
    off = hip.pool_info()["live"] - base
    M.close()
    gpu_ctx.sync()
    hip.pool_trim()
    with held(gpu_ctx):
        Mh = hip.PrecondAMG(gpu_ctx, A, nullvec=nv, params=prm)
    on = hip.pool_info()["live"] - base
    print("%s: live bytes after create, mode off %d, mode on %d" % (variant, off, on))
    assert off <= PARENT_LIVE_BYTES[variant]
    assert on > off
    close(Mh, A)


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("eig_type", [0, 1])
@pytest.mark.parametrize("value_bits", [64, 32])
def test_chebyshev_refactor_is_a_fresh_create(gpu_ctx, value_bits, eig_type):
    rp, ci, val, b, nv = system("2d", False)
    n = len(rp) - 1
    val2 = scaled_values(rp, ci, val)
    kw = dict(degree=3, value_bits=value_bits, eig_type=eig_type)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondChebyshev(gpu_ctx, A, **kw)
    r = np.random.default_rng(9).standard_normal(n)
    z_old = np.array(M.apply(r))
    A.update_values(val2)
    M.refactor(A)
    A2 = hip.Matrix.from_csr(gpu_ctx, rp, ci, val2)
    F = hip.PrecondChebyshev(gpu_ctx, A2, **kw)
    z, zf = np.array(M.apply(r)), np.array(F.apply(r))
    assert np.array_equal(bits(z), bits(zf)) and not np.array_equal(bits(z), bits(z_old))
    assert M.eig_estimate() == F.eig_estimate() and M.value_bits == F.value_bits == value_bits
    M.refactor(A)                                                          # a refreshed polynomial can be refreshed again
    assert np.array_equal(bits(M.apply(r)), bits(zf))
    with held(gpu_ctx):
        P = hip.Precond(gpu_ctx, A, "chebyshev2", 0)                       # the route by name refreshes too
    A.update_values(val)
    P.refactor(A)
    Pf = hip.Precond(gpu_ctx, A, "chebyshev2", 0)                          # created with the mode off: refused, and untouched
    zp = np.array(Pf.apply(r))
    assert np.array_equal(bits(P.apply(r)), bits(zp))
    with pytest.raises(hip.IsphError, match="chebyshev<d>.*created while the pattern was not held"):
        Pf.refactor(A)
    assert np.array_equal(bits(Pf.apply(r)), bits(zp))
    with pytest.raises(hip.IsphError, match="rows"):
        (rp3, ci3, v3), _, _ = S.fixture("grid_21x13")
        A3 = hip.Matrix.from_csr(gpu_ctx, np.asarray(rp3, dtype=np.int32), np.asarray(ci3, dtype=np.int32), np.asarray(v3, dtype=np.float64))
        M.refactor(A3)
    close(M, F, P, Pf, A, A2, A3)
