"""-m gpu: the SA-AMG hierarchy at BASELINE configs[1]'s full size against the oracle (oracle/isph_amg_oracle.c), level
by level.  The 1 M-row system is assembled once, in the library's own row numbering (the product default), and handed
to the oracle permuted (P A P^T, oracle/order.py): the hierarchy's internals are exported in the matrix' numbering,
vectors cross the C ABI in the caller's.

At this size the set-up runs the paths that small systems rarely reach: MIS-2 work lists over a million rows, scratch
rows of (size_t) i * CAP slots packed by k_rows_compact, and, with a threshold, prolongator rows of more than 16
aggregates (the 64-lane and two-pass fallbacks of amg_prolongator).  Tolerances are those of tests/test_gpu_amg.py:
patterns and aggregates exact, P within 1e-12 and A_l within 1e-11 of their max, one V cycle within 1e-9, FGMRES + AMG
iterations within +-1 and x within 1e-6.  The one-pass kernels add in arrival order, so two device builds may differ in
their last bits: they must give the same patterns and aggregates and values within the same tolerances."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip, workload
import oracle as orc
from amg_levels import compare_levels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def config1(gpu_ctx_bricks):
    """test_config1_full_size_100cubed's system: 100^3 TGV particles in lexicographic atom order, the library's bricks"""
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
    rp, ci, v = A.export_csr()
    perm = A.ordering()["perm"]
    rpi, cii, vi, bi = oorder.permute_system(rp, ci, v, b, perm)
    del rp, ci, v
    yield SimpleNamespace(ctx=ctx, A=A, b=b, n=n, perm=perm, rp=rpi, ci=cii, v=vi, bi=bi, nv=np.full(n, 1.0 / np.sqrt(n)))
    A.close()


@pytest.mark.parametrize("name,kw", [
    ("bench.py solve line", dict(block=512, theta=0.0)),
    ("ml.xml step line", dict(block=512, theta=0.0, max_levels=8, sweeps=4, smoother=1)),
])
def test_config1_amg_hierarchy_matches_oracle(config1, name, kw):
    s = config1
    t0 = time.perf_counter()
    G = orc.AMG(s.rp, s.ci, s.v, nullvec=s.nv, **kw)
    t_orc = time.perf_counter() - t0
    M = hip.PrecondAMG(s.ctx, s.A, nullvec=s.nv, params=hip.AmgParams(**kw))
    assert M.levels == G.levels >= 3, (M.levels, G.levels)
    gp, ga = compare_levels(M, G)
    # one V cycle on a seeded r: the caller's numbering on the device, the matrix' in the oracle
    r = np.random.default_rng(7).standard_normal(s.n)
    zo = np.empty(s.n)
    zo[s.perm] = G.apply(r[s.perm])
    zg = M.apply(r)
    gz = np.linalg.norm(zg - zo) / np.linalg.norm(zo)
    assert gz <= 1e-9
    # FGMRES + AMG
    t1 = time.perf_counter()
    xoi, io, _ = orc.solve(s.rp, s.ci, s.v, s.bi, singular=True, prec="amg", amg=G)
    t_solve = time.perf_counter() - t1
    xo = np.empty(s.n)
    xo[s.perm] = xoi
    xg = np.zeros(s.n)
    info = hip.solve(s.ctx, s.A, s.b.copy(), xg, prec=M, singular=True)
    assert info.converged == 1 and io.converged == 1 and abs(info.iters - io.iters) <= 1, (info.iters, io.iters)
    gx = np.linalg.norm(xg - xo) / np.linalg.norm(xo)
    assert gx <= 1e-6
    # a second device build
    M1 = hip.PrecondAMG(s.ctx, s.A, nullvec=s.nv, params=hip.AmgParams(**kw))
    rp_, ra = compare_levels(M1, M)
    print("config1 AMG, %s: %d levels %s; oracle set-up %.1f s, solve %.1f s; device vs oracle: P %.2g, A_l %.2g, "
          "V cycle %.2g, iters %d vs %d, x %.2g; two device builds: P %.2g, A_l %.2g"
          % (name, M.levels, [M.level_info(l)["rows"] for l in range(M.levels)], t_orc, t_solve, gp, ga, gz,
             info.iters, io.iters, gx, rp_, ra))
    M.close(); M1.close()


def test_config1_thresholded_amg_takes_the_wide_prolongator_rows(config1):
    """theta = 0.02: the strength test leaves aggregates small enough that some rows of P_0 meet more than 16 of them,
    beyond the 16-lane scratch rows of the fast path.  The aggregates of level 1 on depend on the last bits of A_1, which
    the unordered additions of the device do not reproduce (test_amg_rows_with_many_aggregates_take_the_wider_scratch_rows):
    the comparison with the oracle stops at A_1.  The V cycle runs through the deeper levels and is not compared; the
    FGMRES solve it preconditions must converge, with the residual re-computed on the host <= 2e-8."""
    s = config1
    kw = dict(block=512, theta=0.02)
    t0 = time.perf_counter()
    G = orc.AMG(s.rp, s.ci, s.v, nullvec=s.nv, **kw)
    t_orc = time.perf_counter() - t0
    M = hip.PrecondAMG(s.ctx, s.A, nullvec=s.nv, params=hip.AmgParams(**kw))
    assert M.levels >= 3 and G.levels >= 3
    rP = M.export(0, "P")[0]
    assert np.diff(rP).max() > 16, np.diff(rP).max()                 # the premise
    gp, ga = compare_levels(M, G, deep=2)
    M1 = hip.PrecondAMG(s.ctx, s.A, nullvec=s.nv, params=hip.AmgParams(**kw))
    rp_, ra = compare_levels(M1, M, deep=2)
    M1.close()
    xg, bb = np.zeros(s.n), s.b.copy()
    info = hip.solve(s.ctx, s.A, bb, xg, prec=M, singular=True)
    assert info.converged == 1
    Ah = sps.csr_matrix((s.v, s.ci, s.rp), shape=(s.n, s.n))         # the matrix' numbering: internal row r = caller perm[r]
    r = bb[s.perm] - Ah @ xg[s.perm]
    r -= r.mean()
    res = np.linalg.norm(r) / np.linalg.norm(bb)
    assert res < 2e-8
    print("config1 AMG, theta 0.02: %d levels, widest P_0 row %d; oracle set-up %.1f s; device vs oracle to A_1: P %.2g, "
          "A_l %.2g; two device builds: P %.2g, A_l %.2g; FGMRES %d iterations, host residual %.2g"
          % (M.levels, np.diff(rP).max(), t_orc, gp, ga, rp_, ra, info.iters, res))
    M.close()
