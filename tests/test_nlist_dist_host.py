"""not gpu: the numpy restatement of the multi-rank ghost / list / plan build (tests/nlist_dist_reference.py) against ground
truth that exists without it -- workload.make_cloud on the whole box (the rows, as sets of (global id, image shift)) and
dist.make_plan on the restatement's (owner rank, owner index) (column map, peers, send / receive lists)."""
import types

import numpy as np
import pytest

from isph_amd import dist, workload
import nlist_dist_reference as ref

CASES, CLOUDS, case_id, geometry, cloud, global_rows = ref.CASES, ref.CLOUDS, ref.case_id, ref.geometry, ref.cloud, ref.global_rows


class _LoopTD:
    """the collective of dist.make_plan as a plain loop: a first sweep over the ranks records what every rank contributes
    (each sees empty contributions of the others, its plan is thrown away), a second hands everybody the whole list"""

    def __init__(self, nranks, rank, gathered):
        self.n, self.rank, self.gathered = nranks, rank, gathered
        self.said = None

    def get_world_size(self):
        return self.n

    def all_gather_object(self, out, obj):
        self.said = obj
        for r in range(self.n):
            out[r] = self.gathered[r] if self.gathered is not None else {}


def make_plans(res):
    R = len(res)
    parts = [dict(spec=types.SimpleNamespace(rank=r), nlocal=o["nlocal"], nall=o["nall"], owner_rank=o["owner_rank"],
                  owner_index=o["owner_index"]) for r, o in enumerate(res)]
    if R == 1:
        return [dist.make_plan(parts[0], None)]
    said = []
    for r in range(R):
        td = _LoopTD(R, r, None)
        dist.make_plan(parts[r], td)
        said.append(td.said)
    return [dist.make_plan(parts[r], _LoopTD(R, r, said)) for r in range(R)]


@pytest.fixture(scope="module", params=CASES, ids=case_id)
def case(request):
    return request.param


@pytest.mark.parametrize("kind", CLOUDS)
def test_rows_equal_the_global_build_and_the_plan_equals_make_plan(case, kind):
    dim, nlat, pgrid, periodic, _ = case
    dc, dx, L, h, cut = geometry(case)
    x = cloud(case, kind)
    gp, grows = global_rows(case, x)
    gids = ref.split(dc, x)
    if kind == "void" and dc.nranks > 1:
        assert len(gids[-1]) == 0
    if kind == "lattice":
        assert any(np.any(dc.wrap(x)[:, 0] == f) for f in dc.faces[0][:-1])          # particles ON a face
    xw = dc.wrap(x)
    for prune in (0, 1):
        res = ref.build(dc, [x[g] for g in gids], cut, prune)
        for r, o in enumerate(res):
            n = o["nlocal"]
            assert n == len(gids[r])
            gid = np.array([gids[int(rr)][int(ii)] for rr, ii in zip(o["owner_rank"], o["owner_index"])], dtype=np.int64)
            sh = np.rint((o["x"] - xw[gid]) / L).astype(np.int64) if len(gid) else np.zeros((0, 3), np.int64)
            sh[:, dim:] = 0
            assert np.array_equal(sh, o["shift"])
            for i in range(n):
                j = o["neigh_idx"][o["neigh_ptr"][i]:o["neigh_ptr"][i + 1]]
                assert np.all(np.diff(j) > 0)
                row = sorted(zip(gid[j].tolist(), *(sh[j, a].tolist() for a in range(3))))
                assert row == grows[int(gids[r][i])], (r, i)
            if prune:
                keep = np.zeros(o["nall"], dtype=bool)
                keep[:n] = True
                keep[o["neigh_idx"]] = True
                assert keep.all()
        plans = make_plans(res)
        for r, (o, plan) in enumerate(zip(res, plans)):
            assert np.array_equal(plan.colmap, o["colmap"]) and plan.ncol == o["ncol"], r
            # what rank r sends to p is what p's make_plan receives from r, in that order
            for k, q in enumerate(o["peers"]):
                s = o["send_idx"][o["send_ptr"][k]:o["send_ptr"][k + 1]]
                pq = plans[int(q)]
                kk = np.flatnonzero(pq.peers == r)
                got = pq.recv_idx[pq.recv_ptr[kk[0]]:pq.recv_ptr[kk[0] + 1]] if len(kk) else np.zeros(0, np.int32)
                assert np.array_equal(s, got), (r, int(q))
            if plan.ncol == plan.nlocal and len(o["peers"]):
                continue      # make_plan returns early for a rank without off-rank ghosts and leaves out what it sends
            assert np.array_equal(plan.peers, o["peers"]), r
            assert np.array_equal(plan.send_ptr, o["send_ptr"]) and np.array_equal(plan.send_idx, o["send_idx"]), r
            assert np.array_equal(plan.recv_ptr, o["recv_ptr"]), r


def test_one_rank_equals_make_cloud_bit_for_bit():
    case = CASES[0]
    dc, dx, L, h, cut = geometry(case)
    for kind in CLOUDS:
        x = cloud(case, kind)
        p = workload.make_cloud(x, [L, L], h, cut, dim=2)
        for prune in (0,):
            o = ref.build(dc, [x], cut, prune)[0]
            assert o["nall"] == p["nall"]
            assert np.array_equal(o["x"].view(np.int64), p["x"].view(np.int64))
            assert np.array_equal(o["owner_index"], p["owner_index"])
            assert np.array_equal(o["neigh_ptr"], p["neigh_ptr"]) and np.array_equal(o["neigh_idx"], p["neigh_idx"])
            assert np.array_equal(o["colmap"], p["owner_index"]) and len(o["peers"]) == 0


def test_migration_order_and_refusal():
    case = CASES[3]
    dc, dx, L, h, cut = geometry(case)
    x = cloud(case, "jitter0.05-s1")
    gids = ref.split(dc, x)
    rng = np.random.default_rng(11)
    xo = [x[g] + np.pad(0.8 * (L / 2) * rng.uniform(-1, 1, size=(len(g), 2)), ((0, 0), (0, 1))) for g in gids]
    fd = [np.stack([g.astype(np.float64), -g.astype(np.float64)], axis=1) for g in gids]
    fi = [g.astype(np.int32)[:, None] for g in gids]
    res = ref.migrate(dc, xo, fd, fi)
    moved = np.zeros((len(x), 3))
    for r in range(dc.nranks):
        moved[gids[r]] = xo[r]
    own = dc.owner(dc.wrap(moved))
    seen = 0
    for r, (xn, fdn, fin, sent, recv) in enumerate(res):
        g = fin[:, 0].astype(np.int64)
        assert np.all(own[g] == r) and np.array_equal(xn, dc.wrap(moved)[g]) and np.array_equal(fdn[:, 0], g.astype(np.float64))
        nstay = len(g) - recv
        assert np.all(np.diff(g[:nstay]) > 0)                               # the stayers in their old order
        src = np.array([next(q for q in range(dc.nranks) if gg in set(gids[q].tolist())) for gg in g[nstay:]], dtype=np.int64)
        key = src * (1 << 32) + np.array([int(np.searchsorted(gids[s], gg)) for s, gg in zip(src, g[nstay:])], dtype=np.int64)
        assert np.all(np.diff(key) > 0)                                      # the arrivals by (source rank, source index)
        seen += len(g)
    assert seen == len(x) and sum(r[3] for r in res) == sum(r[4] for r in res) > 0
    dc4 = geometry(CASES[4])[0]
    g4 = ref.split(dc4, x)
    with pytest.raises(ValueError, match=ref.FAR):
        ref.migrate(dc4, [x[g] + np.array([1.5 * L / 4, 0.0, 0.0]) for g in g4], [np.zeros((len(g), 0)) for g in g4],
                    [np.zeros((len(g), 0), np.int32) for g in g4])
