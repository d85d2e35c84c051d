"""-m gpu: migration, ghost atoms, neighbour list, column map, halo plan and forward comm on a brick of ranks, built on the
device (isph_migrate, isph_nlist_build_dist, isph_nlist_forward; hip.migrate, hip.NeighbourListDist,
workload.make_cloud_dist_device).  The ranks are the threads of tests/ranks.py on one GPU over the host-staged transport.

Every array of every rank is compared bit for bit with the numpy restatement tests/nlist_dist_reference.py, which
tests/test_nlist_dist_host.py pins to workload.make_cloud and dist.make_plan; one rank is compared with isph_nlist_build;
the end-to-end test assembles and solves the NullSpace Poisson system from the device-built arrays and compares with the
one-rank device solve of the whole cloud (entries 1e-12 max, DESIGN row a3; solution 1e-6, iterations +-1, row a12)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import isph_amd  # noqa: F401
from isph_amd import hip, workload
import nlist_dist_reference as ref
from ranks import RankGroup

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
CASES, CLOUDS = ref.CASES, ref.CLOUDS
PLAN_KEYS = ("peers", "send_ptr", "send_idx", "recv_ptr")


def hip_decomp(dc):
    d = dc.dim
    return hip.Decomp(d, dc.lo[:d], dc.hi[:d], dc.periodic[:d], dc.pgrid[:d], faces=dc.user_faces)


@functools.lru_cache(maxsize=None)
def problem(ci, kind):
    """the global cloud of case ci, who owns what, the restatement with prune 0 and 1 -- computed once, never changed"""
    dc, dx, L, h, cut = ref.geometry(CASES[ci])
    x = ref.cloud(CASES[ci], kind)
    gids = ref.split(dc, x)
    return x, gids, {p: ref.build(dc, [x[g] for g in gids], cut, p) for p in (0, 1)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def assert_equals_restatement(got, info, plan, want, where):
    n, nall = want["nlocal"], want["nall"]
    assert (info["nlocal"], info["nghost"], info["entries"], info["ncol"]) == (n, nall - n, len(want["neigh_idx"]), want["ncol"]), where
    assert info["npeers"] == len(want["peers"]) and info["nsend"] == len(want["send_idx"]), where
    assert info["noffrank"] == int(np.sum(want["owner_rank"][n:] != plan.rank)), where
    assert same_bits(got["x"], want["x"]), where
    for k in ("owner_rank", "owner_index", "neigh_ptr", "neigh_idx", "colmap"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert np.array_equal(plan.colmap, want["colmap"]) and plan.ncol == want["ncol"], where
    for k in PLAN_KEYS:
        assert getattr(plan, k).dtype == np.int32 and np.array_equal(getattr(plan, k), want[k]), (where, k)


def _rank_builds(rank, G, ci, kinds):
    dc, dx, L, h, cut = ref.geometry(CASES[ci])
    hd = hip_decomp(dc)
    ctx = G.context(rank)
    out = {}
    try:
        for kind in kinds:
            x, gids, _ = problem(ci, kind)
            for prune in (0, 1):
                nl = hip.NeighbourListDist(ctx, np.ascontiguousarray(x[gids[rank]]), hd, cut, prune=prune)
                out[kind, prune] = (nl.get(ptr64=True), nl.info, nl.plan())
                nl.close()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[ref.case_id(c) for c in CASES])
def test_every_array_of_every_rank_equals_the_restatement(ci):
    """x_all, owner_rank, owner_index, offsets, entries, colmap, peers, send_ptr, send_idx, recv_ptr -- bit for bit, prune 0
    and 1, on the jittered lattices, the exact lattice (particles on the faces, pairs on the cut radius), a particle at
    x = hi before the wrap and a void that leaves the last rank empty"""
    dc = ref.geometry(CASES[ci])[0]
    for kind in CLOUDS:
        problem(ci, kind)
    G = RankGroup(dc.nranks, timeout_s=60.0)
    try:
        res = G.run(_rank_builds, ci, CLOUDS)
    finally:
        G.close()
    pruned = 0
    for kind in CLOUDS:
        want = problem(ci, kind)[2]
        for prune in (0, 1):
            for r in range(dc.nranks):
                got, info, plan = res[r][kind, prune]
                assert_equals_restatement(got, info, plan, want[prune][r], (ref.case_id(CASES[ci]), kind, prune, r))
            pruned += sum(want[0][r]["nall"] - want[1][r]["nall"] for r in range(dc.nranks))
    if dc.dim == 3 or min(dc.pgrid[:2]) > 1:
        assert pruned > 0                      # the corners of the grown sub-box lie outside every neighbourhood


@pytest.mark.parametrize("dim", [2, 3])
def test_one_rank_equals_isph_nlist_build(gpu_ctx, dim):
    """(1,1) / (1,1,1) without a communicator: the whole result equals isph_nlist_build bit for bit, host and device side"""
    case = (dim, 16 if dim == 2 else 12, (1,) * dim, (1,) * dim, False)
    dc, dx, L, h, cut = ref.geometry(case)
    for kind in ("jitter0.3-s1", "lattice", "at-hi"):
        x = ref.cloud(case, kind)
        for xs in (x, T(x)):
            one = hip.NeighbourList(gpu_ctx, xs, (0.0,) * dim, (L,) * dim, (1,) * dim, cut, dim, wrap=True)
            nl = hip.NeighbourListDist(gpu_ctx, xs, hip_decomp(dc), cut, prune=False)
            a, b, ia, ib = one.get(), nl.get(), one.info, nl.info
            one.close(); nl.close()
            assert all(ia[k] == ib[k] for k in ia) and ib["ncol"] == ia["nlocal"] and ib["npeers"] == 0 and ib["noffrank"] == 0
            cpu = lambda v: v.cpu().numpy() if hip._is_torch(v) else v
            assert same_bits(cpu(a["x"]), cpu(b["x"]))
            for k in ("owner_index", "neigh_ptr", "neigh_idx"):
                assert str(a[k].dtype) == str(b[k].dtype) and np.array_equal(cpu(a[k]), cpu(b[k])), k
            assert np.array_equal(cpu(b["colmap"]), cpu(a["owner_index"])) and not cpu(b["owner_rank"]).any()


def _rank_forward(rank, G, ci, kind):
    dc, dx, L, h, cut = ref.geometry(CASES[ci])
    x, gids, _ = problem(ci, kind)
    ctx = G.context(rank)
    out = {}
    try:
        for prune in (0, 1):
            nl = hip.NeighbourListDist(ctx, np.ascontiguousarray(x[gids[rank]]), hip_decomp(dc), cut, prune=prune)
            g, i = nl.get(), nl.info
            n, nall = i["nlocal"], i["nlocal"] + i["nghost"]
            a = np.full((nall, 4), -1.0)
            a[:n, 0], a[:n, 1:] = gids[rank], g["x"][:n]
            ai = np.full(nall, -1, dtype=np.int32)
            ai[:n] = gids[rank]
            ad, aid = T(a), T(ai)
            nl.forward(a, 4); nl.forward(ai); nl.forward(ad); nl.forward(aid)
            assert same_bits(ad.cpu().numpy(), a) and np.array_equal(aid.cpu().numpy(), ai)
            out[prune] = (g, a, ai)
            nl.close()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("ci", range(1, len(CASES)), ids=[ref.case_id(c) for c in CASES[1:]])
def test_forward_fills_every_ghost_row_from_its_owner(ci):
    """a field holding the global id and the position arrives in every ghost row, as doubles and as ints, host and device
    side; the ghost's own position is the forwarded one plus the known shift"""
    kind = "jitter0.3-s1"
    dc = ref.geometry(CASES[ci])[0]
    x, gids, want = problem(ci, kind)
    xw = dc.wrap(x)
    G = RankGroup(dc.nranks, timeout_s=60.0)
    try:
        res = G.run(_rank_forward, ci, kind)
    finally:
        G.close()
    for prune in (0, 1):
        for r in range(dc.nranks):
            g, a, ai = res[r][prune]
            w = want[prune][r]
            gid = np.array([gids[int(rr)][int(ii)] for rr, ii in zip(w["owner_rank"], w["owner_index"])], dtype=np.int64)
            assert np.array_equal(ai, gid) and np.array_equal(a[:, 0], gid.astype(np.float64))
            assert same_bits(a[:, 1:], xw[gid])
            pos = a[:, 1:] + w["shift"].astype(np.float64) * dc.period
            if dc.dim == 2:
                pos[:, 2] = g["x"][:, 2]
            assert same_bits(pos, g["x"])


def _moved(ci, frac, seed=17):
    """per rank: the owned particles of the jittered cloud displaced by up to frac of the narrowest sub-box per axis, with
    two doubles and two ints each"""
    dc, dx, L, h, cut = ref.geometry(CASES[ci])
    x, gids, _ = problem(ci, "jitter0.05-s1")
    w = min(float(np.min(np.diff(dc.faces[a]))) for a in range(dc.dim))
    rng = np.random.default_rng(seed)
    disp = np.zeros_like(x)
    disp[:, :dc.dim] = frac * w * rng.uniform(-1.0, 1.0, size=(len(x), dc.dim))
    xs = [np.ascontiguousarray(x[g] + disp[g]) for g in gids]
    fd = [np.ascontiguousarray(np.stack([np.sqrt(2.0) * g, -1.0 / (1.0 + g)], axis=1)) for g in gids]
    fi = [np.ascontiguousarray(np.stack([g, 7 - g], axis=1).astype(np.int32)) for g in gids]
    return x + disp, xs, fd, fi


def _rank_migrate(rank, G, ci, refuse):
    dc, dx, L, h, cut = ref.geometry(CASES[ci])
    hd = hip_decomp(dc)
    _, xs, fd, fi = _moved(ci, 0.8)
    ctx = G.context(rank)
    out = {}
    try:
        if refuse:
            far = np.ascontiguousarray(xs[rank] + np.array([1.5 * L / dc.pgrid[0], 0.0, 0.0]))
            if rank == dc.nranks - 1:
                far = far[:0]                                    # a rank without particles fails with the others
            try:
                hip.migrate(ctx, hd, far, fd[rank][:len(far)], fi[rank][:len(far)])
                out["refused"] = None
            except hip.IsphError as e:
                out["refused"] = str(e)
        out["host"] = hip.migrate(ctx, hd, xs[rank], fd[rank], fi[rank])           # the group is still usable
        xd, fdd, fid, info = hip.migrate(ctx, hd, T(xs[rank]), T(fd[rank]), T(fi[rank]))
        out["dev"] = (xd.cpu().numpy(), fdd.cpu().numpy(), fid.cpu().numpy(), info)
        out["bare"] = hip.migrate(ctx, hd, xs[rank])
        # the next step: ghosts, list and plan of the new owners, global ids forwarded
        nl = hip.NeighbourListDist(ctx, xd, hd, cut, prune=True)
        g, i = nl.get(), nl.info
        gid = torch.full((i["nlocal"] + i["nghost"],), -1, dtype=torch.int32, device=DEV)
        gid[:i["nlocal"]] = fid[:, 0]
        nl.forward(gid)
        out["list"] = (g["x"].cpu().numpy(), g["neigh_ptr"].cpu().numpy(), g["neigh_idx"].cpu().numpy(), gid.cpu().numpy())
        nl.close()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("ci", [3, 4, 7], ids=[ref.case_id(CASES[i]) for i in (3, 4, 7)])
def test_migrate_then_build(ci):
    """displaced by up to 0.8 of the narrowest sub-box: order, wrapped positions and payload equal the restatement bit for
    bit; 1.5 sub-boxes fail on ALL ranks by name (where the grid has a second neighbour) and the group stays usable;
    migrate -> build_dist gives, by global id, the rows of the global build of the moved cloud"""
    case = CASES[ci]
    dc, dx, L, h, cut = ref.geometry(case)
    refuse = dc.pgrid[0] >= 4
    moved, xs, fd, fi = _moved(ci, 0.8)
    want = ref.migrate(dc, xs, fd, fi)
    G = RankGroup(dc.nranks, timeout_s=60.0)
    try:
        res = G.run(_rank_migrate, ci, refuse)
    finally:
        G.close()
    _, grows = ref.global_rows(case, moved)
    xw = dc.wrap(moved)
    assert sum(w[3] for w in want) > 0
    for r in range(dc.nranks):
        if refuse:
            assert res[r]["refused"] is not None and ref.FAR in res[r]["refused"], (r, res[r]["refused"])
        wx, wfd, wfi, sent, recv = want[r]
        for side in ("host", "dev"):
            gx, gfd, gfi, info = res[r][side]
            assert info == dict(nlocal=len(wx), sent=sent, received=recv), (r, side)
            assert same_bits(gx, wx) and same_bits(gfd, wfd) and np.array_equal(gfi, wfi), (r, side)
        bx, bfd, bfi, _ = res[r]["bare"]
        assert same_bits(bx, wx) and bfd.shape == (len(wx), 0) and bfi.shape == (len(wx), 0)
        x_all, ptr, idx, gid = res[r]["list"]
        gid = gid.astype(np.int64)
        assert np.array_equal(gid[:len(wx)], wfi[:, 0]) and gid.min() >= 0
        sh = np.rint((x_all - xw[gid]) / L).astype(np.int64)
        sh[:, dc.dim:] = 0
        for i in range(len(wx)):
            j = idx[ptr[i]:ptr[i + 1]]
            assert sorted(zip(gid[j].tolist(), *(sh[j, a].tolist() for a in range(3)))) == grows[int(gid[i])], (r, i)


def _rank_refusals(rank, G):
    case = CASES[1]
    dc, dx, L, h, cut = ref.geometry(case)
    x, gids, _ = problem(1, "jitter0.05-s1")
    mine = np.ascontiguousarray(x[gids[rank]])
    ctx = G.context(rank)
    msgs = {}

    def attempt(name, xs, decomp, c):
        try:
            hip.NeighbourListDist(ctx, xs, decomp, c, prune=True).close()
            msgs[name] = None
        except hip.IsphError as e:
            msgs[name] = str(e)

    try:
        stray = np.ascontiguousarray(np.concatenate([mine, x[gids[1]][:2]])) if rank == 0 else mine
        attempt("outside", stray, hip_decomp(dc), cut)
        narrow = hip.Decomp(2, (0.0, 0.0), (L, L), (1, 1), (2, 1), faces=[np.array([0.0, 2.0 * dx, L]), None])
        attempt("narrow", mine, narrow, cut)
        attempt("ranks", mine, hip.Decomp(2, (0.0, 0.0), (L, L), (1, 1), (2, 2)), cut)
        attempt("good", mine, hip_decomp(dc), cut)
    finally:
        ctx.close()
    return msgs


def test_refusals_by_name_fail_on_all_ranks_together():
    problem(1, "jitter0.05-s1")
    G = RankGroup(2, timeout_s=60.0)
    try:
        res = G.run(_rank_refusals)
    finally:
        G.close()
    assert "2 owned particles lie outside the rank's sub-box" in res[0]["outside"]
    assert res[1]["outside"] is not None and "another rank" in res[1]["outside"]
    for r in range(2):
        assert "a sub-box is narrower than the cut" in res[r]["narrow"], res[r]
        assert "differs from the number of ranks" in res[r]["ranks"], res[r]
        assert res[r]["good"] is None, res[r]


def _vstar(xw, dim):
    v = np.zeros_like(xw)
    v[:, 0] = np.sin(xw[:, 0]) * np.cos(xw[:, 1])
    v[:, 1] = -np.cos(xw[:, 0]) * np.sin(xw[:, 1])
    if dim == 3:
        v[:, 0] *= np.cos(xw[:, 2])
        v[:, 1] *= np.cos(xw[:, 2])
    return 0.1 * v


def _solve(ctx, A, b):
    M = hip.Precond(ctx, A, "jacobi")
    p = torch.zeros_like(b)
    info = hip.solve(ctx, A, b, p, prec=M, singular=True, params=hip.SolverParams(num_blocks=50))
    M.close()
    return p.cpu().numpy(), (int(info.converged), int(info.iters))


def _rank_poisson(rank, G, ci, dt):
    dc, dx, L, h, cut = ref.geometry(CASES[ci])
    x, gids, _ = problem(ci, "jitter0.05-s1")
    mine = gids[rank]
    n = len(mine)
    ctx = G.context(rank)
    like = dict(rho=np.ones(n), nu=np.full(n, 0.1), type=np.ones(n, dtype=np.int32), dt=dt)
    d = workload.make_cloud_dist_device(ctx, T(x[mine]), hip_decomp(dc), h, cut, like=like, tags=(mine + 1).astype(np.int32))
    nl, plan = d["nlist"], d["plan"]
    try:
        nall = d["nall"]
        vfrac = torch.zeros(nall, dtype=torch.float64, device=DEV)
        vfrac[:n] = hip.compute_volumes(ctx, d, d["colmap"])
        nl.forward(vfrac)
        vstar = torch.zeros((nall, 3), dtype=torch.float64, device=DEV)
        vstar[:n] = T(_vstar(dc.wrap(x[mine]), dc.dim))
        nl.forward(vstar, 3)
        A, b = hip.assemble_poisson(ctx, d, d["colmap"], dt, d["rho"], vstar, vfrac=vfrac, ncol=plan.ncol, rank0=(rank == 0))
        if plan.npeers:
            A.set_halo(plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        rp, ci_, v = A.export_csr()
        col_gid = np.zeros(plan.ncol, dtype=np.int64)
        col_gid[plan.colmap] = d["tag"].cpu().numpy().astype(np.int64) - 1
        p, info = _solve(ctx, A, b)
        A.close()
        return dict(rows=(rp, col_gid[ci_], v), p=p, info=info, gid=mine, npeers=plan.npeers)
    finally:
        nl.close()
        ctx.close()


@pytest.mark.parametrize("ci", [3, 7], ids=[ref.case_id(CASES[i]) for i in (3, 7)])
def test_poisson_system_and_solution_equal_the_one_rank_solve(gpu_ctx, ci):
    """16^2 on (2,2) and 12^3 on (2,2,2): the NullSpace Poisson system assembled from make_cloud_dist_device + forward of
    vfrac / rho / vstar, the halo from .plan(), FGMRES(50) + "jacobi" -- against the one-rank device solve of the whole cloud"""
    case = CASES[ci]
    dc, dx, L, h, cut = ref.geometry(case)
    dim = dc.dim
    x = problem(ci, "jitter0.05-s1")[0]
    N, dt = len(x), 0.05 * dx / 0.1
    G = RankGroup(dc.nranks, timeout_s=90.0)
    try:
        res = G.run(_rank_poisson, ci, dt)
    finally:
        G.close()
    like = dict(spec=None, rho=np.ones(N), nu=np.full(N, 0.1), type=np.ones(N, dtype=np.int32), dt=dt)
    d1 = workload.make_cloud_device(gpu_ctx, T(x), [L] * dim, h, cut, dim=dim, like=like)
    own = d1["owner_index"].to(torch.int64)
    vfrac = hip.compute_volumes(gpu_ctx, d1, d1["owner_index"])[own].contiguous()
    vstar = T(_vstar(dc.wrap(x), dim))[own].contiguous()
    A1, b1 = hip.assemble_poisson(gpu_ctx, d1, d1["owner_index"], dt, d1["rho"], vstar, vfrac=vfrac)
    rp, ci1, v1 = A1.export_csr()
    p1, info1 = _solve(gpu_ctx, A1, b1)
    A1.close()
    want = sps.csr_matrix((v1, ci1, rp), shape=(N, N))
    want.sort_indices()
    scale = np.abs(v1).max()
    got_p = np.full(N, np.nan)
    for r, o in enumerate(res):
        assert o["npeers"] > 0
        rp_r, cg, v = o["rows"]
        sub = sps.csr_matrix((v, cg, rp_r), shape=(len(o["gid"]), N))
        sub.sort_indices()
        w = want[o["gid"]]
        assert np.array_equal(sub.indptr, w.indptr) and np.array_equal(sub.indices, w.indices), "rank %d: pattern differs" % r
        assert np.max(np.abs(sub.data - w.data)) <= 1e-12 * scale, "rank %d: values differ" % r
        got_p[o["gid"]] = o["p"]
        assert o["info"][0] == 1 and abs(o["info"][1] - info1[1]) <= 1, (o["info"], info1)
    assert info1[0] == 1 and info1[1] > 3
    assert np.max(np.abs(got_p - p1)) <= 1e-6 * np.max(np.abs(p1))
