"""-m gpu: the Navier-Stokes time-step driver on a brick of ranks (isph_ins_create_dist, hip.InsStep(ctx, params, decomp)),
its distributed glue (isph_zero_mean_pressure_dist, isph_status_dist, isph_tgv_error_dist) and the forward comm of several
arrays in one exchange (isph_nlist_forward_multi).  The ranks are the threads of tests/ranks.py on one GPU over the
host-staged transport.

  1. one rank, no communicator: bit for bit the one-rank driver and the one-rank primitives;
  2. 2 x 2 ranks with migration and 3. 2 x 2 x 2 ranks with shift against the one-rank driver on the whole cloud, at the
     tolerances of the same chain under another summation order (test_gpu_ins_driver._same_to_tolerance);
  4. walls on two ranks; 5. the reference's convergence table through the ranks; 6. the primitives on their own;
  7. forward_multi against the single forwards; 8. the message budget of DESIGN.md; 9. refusals; 10. the pool."""
import os

import numpy as np
import pytest
import torch

from isph_amd import hip
import ins_reference as R
import test_gpu_ins_driver as D
import tgv_driver as T
from ranks import RankGroup

pytestmark = pytest.mark.gpu

DEV = "cuda"
L = 2 * np.pi
JACOBI = dict(prec_helmholtz="jacobi", prec_poisson="jacobi")
KBLOCK = 256            # kBlock of the reductions (csrc/common.hpp)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_decomp(dim, pgrid, faces=None):
    return hip.Decomp(dim, (0.0,) * dim, (L,) * dim, (1,) * dim, pgrid, faces=faces)


def owner_of(dc, x):
    """the rank whose sub-box holds every wrapped position: cell c owns faces[c] <= x < faces[c + 1]"""
    r, mul = np.zeros(len(x), dtype=np.int64), 1
    for a in range(dc.dim):
        f = dc.faces[a] if dc.faces[a] is not None else dc.lo[a] + np.arange(dc.pgrid[a] + 1) * ((dc.hi[a] - dc.lo[a]) / dc.pgrid[a])
        xa = dc.lo[a] + np.mod(x[:, a] - dc.lo[a], dc.hi[a] - dc.lo[a])
        c = np.clip(np.searchsorted(f, xa, side="right") - 1, 0, dc.pgrid[a] - 1)
        r += mul * c
        mul *= dc.pgrid[a]
    return r


def dist_driver(ctx, case, dc, mine, **kw):
    S = hip.InsStep(ctx, case.params(**kw), dc)
    S.set_state(*[_dev(a[mine]) for a in (case.x, case.v, case.p, case.typ, case.rho, case.nu)], tag=_dev(mine.astype(np.int32)))
    return S


def _rank_steps(rank, G, case, dc, owner, nsteps, kw, extra_rebuild):
    """run(1) nsteps times; per step the diag row and sizes(); the owned fields by tag at the end"""
    ctx = G.context(rank)
    try:
        S = dist_driver(ctx, case, dc, np.nonzero(owner == rank)[0], **kw)
        rows, sizes = [], []
        for _ in range(nsteps):
            rows.append(S.run(1)[0])
            sizes.append(S.sizes())
        if extra_rebuild:
            S.rebuild()
            sizes.append(S.sizes())
        out = dict(rows=np.array(rows), sizes=sizes, tag=S.get("tag"), x=S.get("x"), v=S.get("v"), p=S.get("p"))
        if case.shift > 0.0:      # one more step by phases: the vmax the shift used
            S.rebuild(); S.pre(); S.solve(); S.advance()
            out["vmax"] = S.shift()
        S.close()
        return out
    finally:
        ctx.close()


def gather(res, n):
    """the fields of all ranks by tag; every particle exactly once"""
    tag = np.concatenate([o["tag"] for o in res])
    assert np.array_equal(np.sort(tag), np.arange(n)), "a particle was lost or doubled"
    out = {}
    for k in ("x", "v", "p"):
        a = np.concatenate([o[k] for o in res])
        full = np.zeros_like(a)
        full[tag] = a
        out[k] = full
    return out


def wrapped_gap(a, b, dim):
    d = a - b
    d[:, :dim] = np.mod(d[:, :dim] + L / 2, L) - L / 2
    return np.max(np.abs(d))


def check_against_one_rank(got, ref, rows, ref_rows, dim, umax=0.1):
    """the tolerances of test_gpu_ins_driver._same_to_tolerance (x wrapped: an owner may stand on the other side of the
    box); the error columns 1e-6 relative; iterations +-1, both solves converged"""
    gx = wrapped_gap(got["x"], ref["x"], dim)
    gv = np.max(np.abs(got["v"] - ref["v"]))
    gp = np.max(np.abs(got["p"] - ref["p"]))
    ge = max(np.max(np.abs(rows[:, c] / ref_rows[:, c] - 1)) for c in (0, 2))
    print("gaps: x %.3e L, v %.3e umax, p %.3e max|p|, error columns %.3e relative"
          % (gx / L, gv / umax, gp / np.abs(ref["p"]).max(), ge))
    assert gx < 1e-8 * L
    assert gv < 1e-7 * umax
    assert gp < 1e-6 * np.abs(ref["p"]).max()
    assert ge <= 1e-6
    assert np.all(np.abs(rows[:, 12:14] - ref_rows[:, 12:14]) <= 1), (rows[:, 12:14], ref_rows[:, 12:14])
    assert np.all(rows[:, 14:] == 1) and np.all(ref_rows[:, 14:] == 1)


_one_rank_cache = {}


def one_rank_steps(ctx, key, case, nsteps, **kw):
    """the one-rank driver on the whole cloud, step by step: the final fields, the diag rows and the positions after every
    step -- computed once per configuration, never modified"""
    if key not in _one_rank_cache:
        S = case.driver(ctx, **kw)
        rows, xs = [], []
        for _ in range(nsteps):
            rows.append(S.run(1)[0])
            xs.append(S.get("x"))
        st = dict(x=S.get("x"), v=S.get("v"), p=S.get("p"))
        S.close()
        _one_rank_cache[key] = (st, np.array(rows), xs)
    return _one_rank_cache[key]


# ---- 1. one rank, no communicator -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [2, 3])
def test_one_rank_without_a_communicator_is_the_one_rank_driver_bit_for_bit(gpu_ctx, dim):
    case = D.tgv2d_case(16, False, 0.5) if dim == 2 else D.tgv3d_case(8, shift=0.05)
    ref, ref_rows = D.driver_run(gpu_ctx, case, 3)
    S = dist_driver(gpu_ctx, case, make_decomp(dim, (1,) * dim), np.arange(case.n))
    rows = S.run(3)
    sz = S.sizes()
    got = dict(x=S.get("x"), v=S.get("v"), p=S.get("p"))
    assert np.array_equal(S.get("tag"), np.arange(case.n)) and not S.get("owner_rank", ghosts=True).any()
    assert np.array_equal(S.get("colmap", ghosts=True), S.get("owner", ghosts=True))
    S.close()
    D._same_bits(got, ref, "1 x 1 grid")
    assert rows.tobytes() == ref_rows.tobytes()
    assert sz["nglobal"] == case.n and sz["ncol"] == case.n and sz["npeers"] == 0 and sz["sent"] == 0 and sz["received"] == 0


def test_the_dist_primitives_without_a_communicator_equal_the_one_rank_primitives(gpu_ctx):
    rng = np.random.default_rng(5)
    n, nall = 3 * KBLOCK + 7, 4 * KBLOCK
    kinds = [R.FLUID, R.SOLID]
    typ = _dev(rng.integers(1, 3, nall).astype(np.int32))
    f = rng.uniform(0.5, 1.5, nall)
    x, v = _dev(rng.uniform(0, L, (nall, 3))), _dev(rng.standard_normal((nall, 3)))
    vf, rho, nu, p = (_dev(rng.uniform(0.5, 1.5, nall)) for _ in range(4))
    fa, fb = _dev(f), _dev(f)
    ma = hip.zero_mean_pressure(gpu_ctx, n, typ, kinds, fa)
    mb = hip.zero_mean_pressure_dist(gpu_ctx, n, typ, kinds, fb)
    assert np.float64(ma).tobytes() == np.float64(mb).tobytes() and fa.cpu().numpy().tobytes() == fb.cpu().numpy().tobytes()
    sa = hip.status(gpu_ctx, n, x, typ, vf, v, rho, centre=(3.0, 3.0, 3.0), radius=2.5)
    sb = hip.status_dist(gpu_ctx, n, x, typ, vf, v, rho, centre=(3.0, 3.0, 3.0), radius=2.5)
    assert sa.tobytes() == sb.tobytes() and sa[7] > 0
    ea = hip.tgv_error(gpu_ctx, n, x, v, p, rho, nu, 0.3, 0.1)
    eb = hip.tgv_error_dist(gpu_ctx, n, x, v, p, rho, nu, 0.3, 0.1)
    assert np.array(ea).tobytes() == np.array(eb).tobytes()


# ---- 2. 2 x 2 ranks with migration ----------------------------------------------------------------------------------------------

def case_2x2():
    case = D.tgv2d_case(16, False, 0.5)
    dx = L / 16
    dc = make_decomp(2, (2, 2), faces=[np.array([0.0, 4.55 * dx, L]), np.array([0.0, 9.45 * dx, L])])
    return case, dc


def test_2x2_ranks_with_migration_equal_the_one_rank_driver(gpu_ctx):
    """tgv2d_case(16, False, 0.5), "jacobi" for both solves on both sides, faces [0, 4.55 dx, L] x [0, 9.45 dx, L], 3 steps:
    ownership 45 / 99 / 35 / 77 at t = 0; 10 particles change owner after step 1, 4 after step 2, none after step 3"""
    case, dc = case_2x2()
    ref, ref_rows, xs = one_rank_steps(gpu_ctx, "2d-jacobi", case, 3, **JACOBI)
    own = [owner_of(dc, case.x)] + [owner_of(dc, x) for x in xs]
    assert [int(np.sum(own[0] == r)) for r in range(4)] == [45, 99, 35, 77]
    G = RankGroup(4, timeout_s=90.0)
    try:
        res = G.run(_rank_steps, case, dc, own[0], 3, JACOBI, True)
    finally:
        G.close()
    # rebuild k migrates what moved during step k - 1: nothing, then 10, then 4, then (the extra rebuild) none
    moved = [0, 10, 4, 0]
    for k in range(4):
        a, b = (own[0], own[0]) if k == 0 else (own[k - 1], own[k])
        assert int(np.sum(a != b)) == moved[k]
        tot_s = tot_r = 0
        for r in range(4):
            sz = res[r]["sizes"][k]
            assert sz["sent"] == int(np.sum((a == r) & (b != r))) and sz["received"] == int(np.sum((a != r) & (b == r))), (k, r, sz)
            assert sz["nlocal"] == int(np.sum(b == r)) and sz["nglobal"] == case.n and sz["npeers"] >= 2
            tot_s += sz["sent"]; tot_r += sz["received"]
        assert tot_s == moved[k] and tot_r == moved[k]
    for r in range(1, 4):
        assert res[r]["rows"].tobytes() == res[0]["rows"].tobytes(), "the diag rows differ between rank 0 and rank %d" % r
    check_against_one_rank(gather(res, case.n), ref, res[0]["rows"], ref_rows, 2)


# ---- 3. 3-D, 2 x 2 x 2 ranks, corrected family with shift -----------------------------------------------------------------------

def test_3d_2x2x2_ranks_with_shift_equal_the_one_rank_driver(gpu_ctx):
    case = D.tgv3d_case(8, shift=0.05)
    dc = make_decomp(3, (2, 2, 2))
    ref, ref_rows, _ = one_rank_steps(gpu_ctx, "3d-jacobi", case, 3, **JACOBI)
    owner = owner_of(dc, case.x)
    G = RankGroup(8, timeout_s=120.0)
    try:
        res = G.run(_rank_steps, case, dc, owner, 3, JACOBI, False)
    finally:
        G.close()
    vmax = [o["vmax"] for o in res]
    assert len(set(np.float64(v).tobytes() for v in vmax)) == 1 and vmax[0] > 0.0, vmax
    for r in range(1, 8):
        assert res[r]["rows"].tobytes() == res[0]["rows"].tobytes()
    # the 2-D TGV error columns say little about a 3-D field; the fields and the status columns are compared
    got = gather(res, case.n)
    gx, gv = wrapped_gap(got["x"], ref["x"], 3), np.max(np.abs(got["v"] - ref["v"]))
    gp = np.max(np.abs(got["p"] - ref["p"]))
    print("gaps: x %.3e L, v %.3e umax, p %.3e max|p|" % (gx / L, gv / 0.1, gp / np.abs(ref["p"]).max()))
    assert gx < 1e-8 * L and gv < 1e-7 * 0.1 and gp < 1e-6 * np.abs(ref["p"]).max()
    rows = res[0]["rows"]
    assert np.all(np.abs(rows[:, 12:14] - ref_rows[:, 12:14]) <= 1) and np.all(rows[:, 14:] == 1) and np.all(ref_rows[:, 14:] == 1)
    for c in (0, 2, 4, 8, 9, 10):     # both error columns, count, volume, mass, kinetic energy
        assert np.max(np.abs(rows[:, c] / ref_rows[:, c] - 1)) <= 1e-6, (c, rows[:, c], ref_rows[:, c])


# ---- 4. walls ---------------------------------------------------------------------------------------------------------------------

def _rank_walls(rank, G, case, dc, owner):
    ctx = G.context(rank)
    try:
        mine = np.nonzero(owner == rank)[0]
        S = dist_driver(ctx, case, dc, mine, **JACOBI)
        S.rebuild(); S.pre()
        info = S.solve()
        n = S.sizes()["nlocal"]
        typ, dp = S.get("type", ghosts=True, device=True), S.get("dp", ghosts=True, device=True)
        mean = hip.zero_mean_pressure_dist(ctx, n, typ, case.kinds, dp + 1.0, update=False)
        out = dict(tag=S.get("tag", ghosts=True), owner_rank=S.get("owner_rank", ghosts=True), n=n, mean=mean,
                   normal=S.get("normal", ghosts=True), pnd=S.get("pnd", ghosts=True), dp=S.get("dp"), type=S.get("type"),
                   x=S.get("x"), v=S.get("vstar"), p=S.get("p"), conv=(info.helmholtz.converged, info.poisson.converged),
                   iters=(info.helmholtz.iters, info.poisson.iters))
        S.close()
        return out
    finally:
        ctx.close()


def test_walled_droplet_on_two_ranks(gpu_ctx):
    case = D.droplet_case()
    dc = make_decomp(2, (2, 1))
    owner = owner_of(dc, case.x)
    solid = R.kind_of(case.typ, case.kinds) == R.SOLID
    for r in range(2):
        assert (solid & (owner == r)).any() and (~solid & (owner == r)).any()
    S1 = case.driver(gpu_ctx, **JACOBI)
    S1.rebuild(); S1.pre()
    i1 = S1.solve()
    ref = dict(x=S1.get("x"), v=S1.get("vstar"), p=S1.get("p"), dp=S1.get("dp"))
    typ1, dp1 = S1.get("type", ghosts=True, device=True), S1.get("dp", ghosts=True, device=True)
    mean1 = hip.zero_mean_pressure(gpu_ctx, case.n, typ1, case.kinds, dp1 + 1.0, update=False)
    S1.close()
    G = RankGroup(2, timeout_s=90.0)
    try:
        res = G.run(_rank_walls, case, dc, owner)
    finally:
        G.close()
    for r, o in enumerate(res):
        n = o["n"]
        assert o["conv"] == (1, 1) and (i1.helmholtz.converged, i1.poisson.converged) == (1, 1)
        assert abs(o["iters"][0] - i1.helmholtz.iters) <= 1 and abs(o["iters"][1] - i1.poisson.iters) <= 1, (o["iters"], i1.poisson.iters)
        # normal and pnd of every ghost are its owner's, bit for bit
        assert len(o["tag"]) > n
        for g in range(n, len(o["tag"])):
            src = res[int(o["owner_rank"][g])]
            i = int(np.nonzero(src["tag"][:src["n"]] == o["tag"][g])[0][0])
            assert o["normal"][g].tobytes() == src["normal"][i].tobytes() and o["pnd"][g].tobytes() == src["pnd"][i].tobytes(), (r, g)
        assert np.all(o["dp"][R.kind_of(o["type"], case.kinds) == R.SOLID] == 0.0)
        assert abs(o["mean"] - mean1) <= 1e-12 * abs(mean1), (o["mean"], mean1)
    assert res[0]["mean"] == res[1]["mean"]
    for o in res:
        o["tag"] = o["tag"][:o["n"]]
    got = gather(res, case.n)
    gx, gv, gp = wrapped_gap(got["x"], ref["x"], 2), np.max(np.abs(got["v"] - ref["v"])), np.max(np.abs(got["p"] - ref["p"]))
    print("gaps: x %.3e L, vstar %.3e umax, p %.3e max|p|" % (gx / L, gv / 0.1, gp / np.abs(ref["p"]).max()))
    assert gx < 1e-8 * L and gv < 1e-7 * 0.1 and gp < 1e-6 * np.abs(ref["p"]).max()


# ---- 5. the reference's table through the ranks -------------------------------------------------------------------------------------

def _rank_table(rank, G, case, dc, owner, nsteps):
    ctx = G.context(rank)
    try:
        S = dist_driver(ctx, case, dc, np.nonzero(owner == rank)[0])
        rows = S.run(nsteps)
        S.close()
        return rows
    finally:
        ctx.close()


@pytest.mark.parametrize("N", [16, 32])
def test_2x2_ranks_reproduce_the_reference_tgv_table(N):
    """conv-taylor-green-vortex-2d-rev390.txt with the pinned settings of oracle/tgv_driver.py and the default
    "bjacobi-ilu0": both error columns to 2.5e-3 relative, the bound of test_run_reproduces_the_reference_tgv_table"""
    ref = T.known_answers()["conv_taylor_green_vortex_2d_rev390"]["rows"][str(N)]
    case = D.tgv2d_case(N, T.PINNED["antisym"], T.PINNED["theta"], block=512)
    dc = make_decomp(2, (2, 2))
    G = RankGroup(4, timeout_s=120.0)
    try:
        res = G.run(_rank_table, case, dc, owner_of(dc, case.x), ref["step"])
    finally:
        G.close()
    last = res[0][-1]
    print("N = %d: p_err %.6e (table %.6e), u_err %.6e (table %.6e)" % (N, last[0], ref["p_err"], last[2], ref["u_err"]))
    assert abs(ref["step"] * case.dt - ref["time"]) < 1e-6
    assert abs(last[0] / ref["p_err"] - 1) < 2.5e-3, (last[0], ref["p_err"])
    assert abs(last[2] / ref["u_err"] - 1) < 2.5e-3, (last[2], ref["u_err"])
    assert np.all(res[0][:, 14:] == 1)
    for r in range(1, 4):
        assert res[r].tobytes() == res[0].tobytes()


# ---- 6. the primitives on their own ---------------------------------------------------------------------------------------------------

COUNTS = {2: [(0, 3001), (1, KBLOCK - 1), (KBLOCK + 1, 0), (KBLOCK - 1, KBLOCK + 1)],
          4: [(0, 1, KBLOCK - 1, KBLOCK + 1), (3001, 0, KBLOCK + 1, 1)]}
KINDS = [R.FLUID, R.SOLID]


def primitive_data(counts, all_solid, seed):
    """per rank: owned rows and 5 ghost rows of random fields"""
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        nall = n + 5
        typ = np.full(nall, 2, dtype=np.int32) if all_solid else rng.integers(1, 3, nall).astype(np.int32)
        out.append(dict(n=n, type=typ, f=rng.uniform(0.5, 1.5, nall), x=rng.uniform(0, L, (nall, 3)), v=rng.standard_normal((nall, 3)),
                        vf=rng.uniform(0.5, 1.5, nall), rho=rng.uniform(0.5, 1.5, nall), nu=rng.uniform(0.05, 0.15, nall),
                        p=rng.uniform(-1.0, 1.0, nall)))
    return out


def _rank_primitives(rank, G, sets):
    ctx = G.context(rank)
    out = []
    try:
        for data in sets:
            d = data[rank]
            n = d["n"]
            for _ in range(2):                      # twice: the bits do not change from run to run
                f = _dev(d["f"])
                mean = hip.zero_mean_pressure_dist(ctx, n, _dev(d["type"]), KINDS, f)
                st = hip.status_dist(ctx, n, _dev(d["x"]), _dev(d["type"]), _dev(d["vf"]), _dev(d["v"]), _dev(d["rho"]),
                                     type_mask=1, centre=(3.0, 3.0, 3.0), radius=2.5)
                e = hip.tgv_error_dist(ctx, n, _dev(d["x"]), _dev(d["v"]), _dev(d["p"]), _dev(d["rho"]), _dev(d["nu"]), 0.3, 0.1)
                host_f = d["f"].copy()              # host operands take the same path after staging
                mean_h = hip.zero_mean_pressure_dist(ctx, n, d["type"], KINDS, host_f)
                out.append(dict(mean=mean, f=f.cpu().numpy(), status=st, tgv=np.array(e), mean_h=mean_h, f_h=host_f))
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("nranks", [2, 4])
def test_the_primitives_over_the_ranks_equal_the_global_sums(nranks):
    sets = [primitive_data(c, False, 11 + k) for k, c in enumerate(COUNTS[nranks])]
    sets.append(primitive_data(COUNTS[nranks][0], True, 3))          # every row Solid: count 0, mean 0, nothing subtracted
    G = RankGroup(nranks, timeout_s=60.0)
    try:
        res = G.run(_rank_primitives, sets)
    finally:
        G.close()
    for k, data in enumerate(sets):
        all_solid = k == len(sets) - 1
        cat = lambda key: np.concatenate([d[key][:d["n"]] for d in data])
        typ, f = cat("type"), cat("f")
        fluid = R.kind_of(typ, KINDS) != R.SOLID
        want_mean = float(np.sum(f[fluid]) / fluid.sum()) if fluid.any() else 0.0
        N = len(typ)
        want_st, _ = R.status(cat("x"), typ, cat("vf"), cat("v"), cat("rho"), N, type_mask=1, centre=(3.0, 3.0, 3.0), radius=2.5)
        want_e = R.tgv_error(cat("x"), cat("v"), cat("p"), cat("rho"), cat("nu"), 0.3, 0.1, N)
        for r in range(nranks):
            a, b = res[r][2 * k], res[r][2 * k + 1]
            d = data[r]
            assert np.float64(a["mean"]).tobytes() == np.float64(b["mean"]).tobytes() == np.float64(res[0][2 * k]["mean"]).tobytes()
            assert np.float64(a["mean_h"]).tobytes() == np.float64(a["mean"]).tobytes() and a["f_h"].tobytes() == a["f"].tobytes()
            assert a["f"].tobytes() == b["f"].tobytes() and a["status"].tobytes() == b["status"].tobytes() == res[0][2 * k]["status"].tobytes()
            assert a["tgv"].tobytes() == b["tgv"].tobytes() == res[0][2 * k]["tgv"].tobytes()
            assert abs(a["mean"] - want_mean) <= 1e-12 * abs(want_mean)
            # owned Solid rows are zeroed, ghost Solid rows stay, every other row loses the mean (one rounding)
            kind = R.kind_of(d["type"], KINDS)
            want_f = np.where(kind == R.SOLID, d["f"], d["f"] - a["mean"])
            want_f[:d["n"]][kind[:d["n"]] == R.SOLID] = 0.0
            assert np.array_equal(a["f"], want_f)
            if all_solid:
                assert a["mean"] == 0.0 and a["status"][0] == 0.0
            else:
                assert np.all(np.abs(a["status"] - want_st) <= 1e-12 * np.abs(want_st)), (a["status"], want_st)
            assert np.all(np.abs(a["tgv"] - np.array(want_e)) <= 1e-12 * np.abs(np.array(want_e))), (a["tgv"], want_e)


# ---- 7. forward_multi --------------------------------------------------------------------------------------------------------------------

def _rank_forward_multi(rank, G, case, dc, owner):
    ctx = G.context(rank)
    out = {}
    try:
        mine = np.nonzero(owner == rank)[0]
        for prune in (0, 1):
            nl = hip.NeighbourListDist(ctx, _dev(case.x[mine]), dc, case.cut, prune=bool(prune))
            i = nl.info
            n, nall = i["nlocal"], i["nlocal"] + i["nghost"]
            def fresh():
                arrs = [np.full((nall, 3), -1.0), np.full(nall, -1.0), np.full(nall, -1.0), np.full(nall, -1.0),
                        np.full(nall, -1, dtype=np.int32), np.full((nall, 2), -1, dtype=np.int32)]
                r2 = np.random.default_rng(100 + rank)
                for a in arrs:
                    a[:n] = r2.standard_normal(a[:n].shape) if a.dtype == np.float64 else r2.integers(0, 1 << 30, a[:n].shape)
                arrs[4][:n] = mine
                return arrs
            single = [_dev(a) for a in fresh()]
            for a in single:
                nl.forward(a)
            multi = [_dev(a) for a in fresh()]
            G._barrier.wait()
            c1 = G.counts()
            G._barrier.wait()
            nl.forward_multi(multi)
            G._barrier.wait()
            c2 = G.counts()
            G._barrier.wait()
            host = fresh()
            nl.forward_multi(host)
            same = all(s.cpu().numpy().tobytes() == m.cpu().numpy().tobytes() == h.tobytes() for s, m, h in zip(single, multi, host))
            out[prune] = dict(same=same, exchanges=c2["exchanges"] - c1["exchanges"], gid=multi[4].cpu().numpy(), n=n,
                              npeers=i["npeers"], nghost=i["nghost"])
            nl.close()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("grid", [(2, 2), (2, 1)], ids=["2x2", "2x1-a-particle-arrives-twice"])
def test_forward_multi_equals_the_single_forwards_in_one_exchange(grid):
    """arrays of 3, 1, 1, 1 doubles and two int arrays in one call, prune 0 and 1, device and host operands; on 2 x 1 ranks
    of the periodic N = 8 box (cut 3 dx, sub-box 4 dx) a particle reaches its neighbour through both faces"""
    case = D.tgv2d_case(16 if grid == (2, 2) else 8, False, 0.5)
    dc = make_decomp(2, grid)
    owner = owner_of(dc, case.x)
    nr = grid[0] * grid[1]
    G = RankGroup(nr, timeout_s=60.0)
    try:
        res = G.run(_rank_forward_multi, case, dc, owner)
    finally:
        G.close()
    for prune in (0, 1):
        for r in range(nr):
            o = res[r][prune]
            assert o["same"] and o["npeers"] > 0 and o["nghost"] > 0
            assert o["exchanges"] == nr, "ONE exchange per rank expected, %d over %d ranks seen" % (o["exchanges"], nr)
            assert o["gid"].min() >= 0
            if grid == (2, 1):      # two ghosts of one particle of the other rank
                g = o["gid"][o["n"]:]
                other = g[owner[g] != r]
                assert len(other) > len(np.unique(other))


# ---- 8. the message budget ------------------------------------------------------------------------------------------------------------------

# DESIGN.md, "The distributed driver": exchanges and all-reduces PER RANK.  The glue rows are counted from the code.  The
# Krylov rows are the share of the two isph_solve calls in this one deterministic configuration (tgv2d_case(16, False,
# 0.5) on the 2 x 2 faces of check 2, "jacobi", fixed-order reductions: the iteration counts do not change from run to
# run), recorded in the table beside the iteration counts, so that solve and run(1) are asserted exactly
BUDGET = dict(rebuild=(6, 9), pre=(1, 0), advance=(1, 0), diagnostics=(0, 4), solve_glue=(3, 3), shift=(1, 1),
              krylov_step1=(29, 54), krylov_step2=(26, 48))


def _counted(G, out, name, fn):
    """fn() on every rank between barriers; out[name] = (exchanges, all-reduces) of all ranks together"""
    G._barrier.wait()
    a = G.counts()
    G._barrier.wait()
    r = fn()
    G._barrier.wait()
    b = G.counts()
    G._barrier.wait()
    out[name] = (b["exchanges"] - a["exchanges"], b["allreduces"] - a["allreduces"])
    return r


def _rank_budget(rank, G, case, dc, owner):
    ctx = G.context(rank)
    out = {}
    try:
        S = dist_driver(ctx, case, dc, np.nonzero(owner == rank)[0], **JACOBI)
        _counted(G, out, "rebuild", S.rebuild)
        _counted(G, out, "pre", S.pre)
        info = _counted(G, out, "solve", S.solve)
        out["iters1"] = (info.helmholtz.iters, info.poisson.iters)
        _counted(G, out, "diagnostics", lambda: S.diagnostics(case.dt))
        _counted(G, out, "advance", S.advance)
        if case.shift > 0.0:
            _counted(G, out, "shift", S.shift)
        rows = _counted(G, out, "run1", lambda: S.run(1))
        out["iters2"] = (int(rows[0, 12]), int(rows[0, 13]))
        # the six state arrays of a rebuild travel in one exchange: the list alone costs one exchange less
        mg = _counted(G, out, "migrate", lambda: hip.migrate(ctx, dc, S.get("x", device=True)))
        nl = _counted(G, out, "list", lambda: hip.NeighbourListDist(ctx, mg[0], dc, case.cut, prune=True))
        nl.close()
        S.close()
    finally:
        ctx.close()
    return out


def _per_rank(o, nr):
    out = {}
    for k, v in o.items():
        if not k.startswith("iters"):
            assert v[0] % nr == 0 and v[1] % nr == 0, (k, v)          # every rank makes every call
            out[k] = (v[0] // nr, v[1] // nr)
    return out


def _sum(*rows):
    return tuple(sum(r[c] for r in rows) for c in (0, 1))


def test_the_message_budget_of_a_step_is_the_one_of_the_design_table():
    case, dc = case_2x2()
    nr = 4
    G = RankGroup(nr, timeout_s=90.0)
    try:
        res = G.run(_rank_budget, case, dc, owner_of(dc, case.x))
    finally:
        G.close()
    o = _per_rank(res[0], nr)
    print(o, "iterations", res[0]["iters1"], res[0]["iters2"])
    for name in ("rebuild", "pre", "advance", "diagnostics"):
        assert o[name] == BUDGET[name], (name, o[name])
    # a rebuild = migration + list + ONE exchange for v, p, rho, nu, type, tag (+ the driver's three consensus)
    assert o["rebuild"] == _sum(o["migrate"], o["list"], (1, 3))
    # the solve phase = the glue of the table + the share of the two Krylov solves, nothing else
    assert o["solve"] == _sum(BUDGET["solve_glue"], BUDGET["krylov_step1"]), (o["solve"], res[0]["iters1"])
    # isph_ins_run(1) = rebuild + pre + solve + diagnostics + advance, nothing else
    want = _sum(BUDGET["rebuild"], BUDGET["pre"], BUDGET["solve_glue"], BUDGET["krylov_step2"], BUDGET["diagnostics"], BUDGET["advance"])
    assert o["run1"] == want, (o["run1"], want, res[0]["iters2"])


def test_the_message_budget_of_a_shift_step_on_2x2x2_ranks():
    """one step by phases of the 3-D case with shift 0.05: the shift row of the table, and the rows that do not depend on
    iteration counts once more, with 7 peers per rank"""
    case = D.tgv3d_case(8, shift=0.05)
    dc = make_decomp(3, (2, 2, 2))
    nr = 8
    G = RankGroup(nr, timeout_s=120.0)
    try:
        res = G.run(_rank_budget, case, dc, owner_of(dc, case.x))
    finally:
        G.close()
    o = _per_rank(res[0], nr)
    print(o, "iterations", res[0]["iters1"], res[0]["iters2"])
    for name in ("rebuild", "pre", "advance", "diagnostics", "shift"):
        assert o[name] == BUDGET[name], (name, o[name])
    assert o["rebuild"] == _sum(o["migrate"], o["list"], (1, 3))
    # the Krylov share of this case is not tabulated; what the phases add to it is: run(1) = the fixed rows + a solve phase
    fixed = _sum(BUDGET["rebuild"], BUDGET["pre"], BUDGET["diagnostics"], BUDGET["advance"], BUDGET["shift"])
    assert o["run1"][0] - fixed[0] >= BUDGET["solve_glue"][0] + 2 and o["run1"][1] - fixed[1] >= BUDGET["solve_glue"][1] + 2


# ---- 9. refusals and failing together --------------------------------------------------------------------------------------------------------

def _rank_refusals(rank, G, case, dc, owner):
    ctx = G.context(rank)
    msgs = {}

    def attempt(name, fn):
        try:
            fn()
            msgs[name] = None
        except hip.IsphError as e:
            msgs[name] = str(e)
    try:
        attempt("grid", lambda: hip.InsStep(ctx, case.params(), make_decomp(2, (2, 2))))
        other = hip.Decomp(2, (0.0, 0.0), (L, 2 * L), (1, 1), (2, 1))
        attempt("box", lambda: hip.InsStep(ctx, case.params(), other))
        nocut = hip.InsParams(2, case.dt, case.h, case.cut, antisym=0, theta=0.5)
        attempt("cut", lambda: hip.InsStep(ctx, nocut, dc))
        mine = np.nonzero(owner == rank)[0]
        S = hip.InsStep(ctx, case.params(**JACOBI), dc)
        typ = case.typ[mine].copy()
        if rank == 0:
            typ[0] = 7
        args = [_dev(a[mine]) for a in (case.x, case.v, case.p)] + [_dev(typ)] + [_dev(a[mine]) for a in (case.rho, case.nu)]
        attempt("type", lambda: S.set_state(*args, tag=_dev(mine.astype(np.int32))))
        attempt("plain", lambda: hip.lib() and hip._check(hip.lib().isph_ins_set_state(S.h, 0, *[hip._ptr(np.zeros(3))] * 6, 0)))
        # the group is usable afterwards
        S.set_state(*[_dev(a[mine]) for a in (case.x, case.v, case.p, case.typ, case.rho, case.nu)], tag=_dev(mine.astype(np.int32)))
        S.rebuild()
        sz = S.sizes()
        attempt("set_list", lambda: S.set_list(S.get("x", ghosts=True), S.get("owner", ghosts=True),
                                               np.zeros(sz["nlocal"] + 1, dtype=np.int32), np.zeros(1, dtype=np.int32)))
        rows = S.run(1)
        msgs["rows"] = rows
        S.close()
        # the stand-alone forward of several arrays: refused arguments on rank 0 alone fail rank 1 at its consensus
        nl = hip.NeighbourListDist(ctx, _dev(case.x[mine]), dc, case.cut)
        a = _dev(np.zeros(nl.info["nlocal"] + nl.info["nghost"]))
        rec = (hip._FwdArray * 1)()
        rec[0].a, rec[0].ncomp, rec[0].is_int = hip._ptr(a), (0 if rank == 0 else 1), 0
        attempt("forward_multi", lambda: hip._check(hip.lib().isph_nlist_forward_multi(ctx.h, nl.h, 1, rec, 1)))
        nl.forward_multi([a])
        nl.close()
    finally:
        ctx.close()
    return msgs


def test_refusals_by_name_and_failing_together():
    case = D.tgv2d_case(16, False, 0.5)
    dc = make_decomp(2, (2, 1))
    G = RankGroup(2, timeout_s=60.0)
    try:
        res = G.run(_rank_refusals, case, dc, owner_of(dc, case.x))
    finally:
        G.close()
    for r in range(2):
        assert "differs from the number of ranks" in res[r]["grid"], res[r]
        assert "contradict the decomposition" in res[r]["box"], res[r]
        assert "isph_ins_create_dist: cut" in res[r]["cut"], res[r]
        assert "isph_ins_set_list: a distributed state" in res[r]["set_list"], res[r]
        assert "isph_ins_set_state_dist" in res[r]["plain"], res[r]
        assert res[r]["rows"].shape == (1, 16) and np.all(res[r]["rows"][:, 14:] == 1)
    assert "ncomp must be" in res[0]["forward_multi"] and "another rank" in res[1]["forward_multi"], (res[0], res[1])
    assert "a type outside [1, ntypes]" in res[0]["type"], res[0]
    assert "another rank" in res[1]["type"], res[1]
    assert res[0]["rows"].tobytes() == res[1]["rows"].tobytes()


# ---- 10. the pool ------------------------------------------------------------------------------------------------------------------------------

def _rank_pool(rank, G, case, dc, owner, live):
    ctx = G.context(rank)
    try:
        mine = np.nonzero(owner == rank)[0]
        # a first pass of the same two steps grows the contexts' own workspaces (the second step's migration changes the
        # row counts); a buffer the driver kept per pass would still show in the second
        S = dist_driver(ctx, case, dc, mine, **JACOBI)
        S.run(2)
        S.close()
        ctx.hold_neighbours(False)
        ctx.sync()
        G._barrier.wait()
        if rank == 0:
            live["before"] = hip.pool_info()["live"]
        G._barrier.wait()
        S = dist_driver(ctx, case, dc, mine, **JACOBI)
        S.run(2)
        ctx.sync()
        G._barrier.wait()
        if rank == 0:
            live["during"] = hip.pool_info()["live"]
        G._barrier.wait()
        S.close()
        ctx.sync()
        G._barrier.wait()
        if rank == 0:
            live["after"] = hip.pool_info()["live"]
        G._barrier.wait()
    finally:
        ctx.close()


def test_two_ranks_run_clean_under_the_pool_canary():
    """ISPH_POOL_CANARY is read once, when the library first touches its pool, which in this process happened long before
    this test: it cannot be set for contexts made here.  So the two-rank run (create, 2 steps, destroy) goes through a
    child process that starts with it (tests/ins_dist_two_ranks.py); an overrun of a pooled buffer aborts the child."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ISPH_POOL_CANARY="1")
    r = subprocess.run([sys.executable, os.path.join(here, "ins_dist_two_ranks.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "two ranks, two steps: clean" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "ISPH_POOL_CANARY" not in r.stderr


def test_destroy_gives_every_buffer_back_on_two_ranks():
    """create, 2 steps, destroy on two ranks (the pool is the process's: the rank threads share it, so the live bytes are
    read between barriers) leave no more live bytes than before create"""
    case = D.tgv2d_case(16, False, 0.5)
    dc = make_decomp(2, (2, 1))
    live = {}
    G = RankGroup(2, timeout_s=60.0)
    try:
        G.run(_rank_pool, case, dc, owner_of(dc, case.x), live)
    finally:
        G.close()
    assert live["during"] > live["before"] and live["after"] <= live["before"], live
