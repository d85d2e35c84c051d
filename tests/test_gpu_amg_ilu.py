"""-m gpu: block ILU(k) as the smoother of the SA-AMG (isph_amg_params::smoother = 4, ML's "IFPACK" smoother with "ILU",
"sa-amg-ilu<k>") against the numpy restatement tests/amg_ilu_reference.py.

Fixtures (amg_ilu_reference.system): stencil (210 rows: a single level-0 block with a tail slice), wall42 (1764 rows),
spd (1480 / 222 / 16 rows), tgv16 (4096 / 15 rows, singular: null vector, Gauss-Seidel on the coarsest level), lap96s
(8640 / 1214 / 76 rows, nonsymmetric; the middle level has 19 blocks of 64 rows and a 62-row tail).
tests/test_amg_ilu_reference.py pins the restatement to the oracle's block ILU(k) and records the reference's counts.

Bounds.  One cycle against the restatement over the device's exported levels: 1e-9 ||z_ref||, the cycle gate of
tests/test_gpu_amg.py.  Dense block inverses against the chunk stream on the same levels: 1e-10 ||z||, the gate two
device builds get there.  Solves: explicit residual <= 1e-7, iterations within one of the reference's FGMRES with the
restated cycle, x within 1e-6 -- the project's parity gate.  Every value is printed before it is asserted.
Measured on an MI355X: cycles 1.3e-16 .. 1.1e-15, dense against stream 6.3e-17 .. 1.1e-16, every solve on the
reference's iteration count with x to 4e-16 .. 1.4e-15 and explicit residuals 1.6e-12 .. 9.2e-9, two thread ranks 8
iterations like one rank with x to 7.9e-9.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip
import amg_ilu_reference as ar
import chebyshev_reference as cr
import krylov_reference as kr

pytestmark = pytest.mark.gpu

AMG_KW = dict(theta=0.0, block=256, coarse_max=64)
KS = list(range(1, 51))
FILLS = [0, 1, 4]


@functools.lru_cache(maxsize=None)
def system(name):
    rp, ci, val, b, singular = ar.system(name)
    n = len(rp) - 1
    return rp, ci, val, b, singular, sps.csr_matrix((val, ci, rp), shape=(n, n))


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            rp, ci, val, _, _, _ = system(name)
            cache[name] = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        return cache[name]
    return get


def rhs(n, seed=10):
    return np.random.default_rng(seed).standard_normal(n)


def nullvec(name):
    n = system(name)[5].shape[0]
    return np.ones(n) / np.sqrt(n) if system(name)[4] else None


def make(ctx, A, name, fill, sweeps=1, **kw):
    prm = dict(AMG_KW)
    prm.update(kw)
    return hip.PrecondAMG(ctx, A, nullvec=nullvec(name), params=hip.AmgParams(smoother=4, ilu_fill=fill, sweeps=sweeps, **prm))


_LEVELS, _SMOOTHERS = {}, {}


def levels_of(M, name):
    """the device's exported levels, once per fixture (the hierarchy does not depend on the smoother or on the build)"""
    if name not in _LEVELS:
        _LEVELS[name] = cr.levels_from(M, system(name)[5].shape[0])
    return _LEVELS[name]


def reference_minv(M, name, fill, sweeps):
    levels = levels_of(M, name)
    if (name, fill) not in _SMOOTHERS:
        _SMOOTHERS[(name, fill)] = ar.build_smoothers(levels, fill, AMG_KW["block"], coarse_smoother=system(name)[4])
    S = _SMOOTHERS[(name, fill)]
    return lambda r: ar.amg_vcycle(levels, S, np.asarray(r, dtype=np.float64), sweeps)


def rel(z, ref):
    return float(np.linalg.norm(np.asarray(z) - ref) / np.linalg.norm(ref))


# ---------------------------------------------------------------- 1. one application
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", ar.FIXTURES)
def test_one_cycle_is_the_restated_cycle(gpu_ctx, dev, name, fill):
    """sweeps 1: the A P shortcut alone; sweeps >= 2: the residual plus accumulate form"""
    n = system(name)[5].shape[0]
    r = rhs(n)
    for sweeps in (1, 2, 3):
        M = make(gpu_ctx, dev(name), name, fill, sweeps)
        z, zr = M.apply(r), reference_minv(M, name, fill, sweeps)(r)
        g = rel(z, zr)
        print("amg-ilu-cycle %-8s fill %d sweeps %d levels %d gap %.2e" % (name, fill, sweeps, M.levels, g))
        M.close()
        assert g <= 1e-9, (name, fill, sweeps, g)


# ---------------------------------------------------------------- 2. the fill is honoured on coarse blocks
@pytest.mark.parametrize("name", ["spd", "lap96s"])
def test_the_fill_reaches_the_coarse_blocks(gpu_ctx, dev, name):
    n = system(name)[5].shape[0]
    r = rhs(n)
    M0, M4 = make(gpu_ctx, dev(name), name, 0), make(gpu_ctx, dev(name), name, 4)
    d = float(np.linalg.norm(M0.apply(r) - M4.apply(r)))
    dr = float(np.linalg.norm(reference_minv(M0, name, 0, 1)(r) - reference_minv(M0, name, 4, 1)(r)))
    print("amg-ilu-fill %-8s |z(0) - z(4)| device %.3e reference %.3e" % (name, d, dr))
    M0.close(); M4.close()
    assert dr > 0.0 and d >= 0.5 * dr


# ---------------------------------------------------------------- 3. paths
@pytest.mark.parametrize("name", ar.FIXTURES)
def test_paths(gpu_ctx, dev, monkeypatch, name):
    singular = system(name)[4]
    M = make(gpu_ctx, dev(name), name, 1)
    paths = [M.path(l) for l in range(M.levels)]
    monkeypatch.setenv("ISPH_AMG_COARSE_STREAM", "1")
    Ms = make(gpu_ctx, dev(name), name, 1)
    monkeypatch.delenv("ISPH_AMG_COARSE_STREAM")
    spaths = [Ms.path(l) for l in range(Ms.levels)]
    print("amg-ilu-paths %-8s %s stream %s" % (name, [(p["smoother"], p["coarse"]) for p in paths],
                                               [(p["smoother"], p["coarse"]) for p in spaths]))
    M.close(); Ms.close()
    assert paths[0]["smoother"] == 5 and spaths[0]["smoother"] == 5
    for p, ps in zip(paths[1:-1], spaths[1:-1]):
        assert p["smoother"] == 4 and ps["smoother"] == 5
    if name in ("spd", "lap96s"):
        assert len(paths) == 3
    if singular:      # Gauss-Seidel solves the coarsest level
        assert paths[-1]["coarse"] == 2 and paths[-1]["smoother"] == 1 and spaths[-1]["smoother"] == 2
    else:
        assert paths[-1]["coarse"] == 1 and paths[-1]["smoother"] == 0


# ---------------------------------------------------------------- 4. dense block inverses against the chunk stream
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", ["spd", "lap96s"])
def test_dense_block_inverses_against_the_stream(gpu_ctx, dev, monkeypatch, name, fill):
    """the stream ILU(k) is pinned to the oracle elsewhere: this pins k_ilu_dense_build"""
    n = system(name)[5].shape[0]
    r = rhs(n, 12)
    for sweeps in (1, 2):
        M = make(gpu_ctx, dev(name), name, fill, sweeps)
        monkeypatch.setenv("ISPH_AMG_COARSE_STREAM", "1")
        Ms = make(gpu_ctx, dev(name), name, fill, sweeps)
        monkeypatch.delenv("ISPH_AMG_COARSE_STREAM")
        assert M.path(1)["smoother"] == 4 and Ms.path(1)["smoother"] == 5
        z, zs = M.apply(r), Ms.apply(r)
        g = rel(z, zs)
        print("amg-ilu-dense-vs-stream %-8s fill %d sweeps %d gap %.2e" % (name, fill, sweeps, g))
        M.close(); Ms.close()
        assert g <= 1e-10, (name, fill, sweeps, g)


# ---------------------------------------------------------------- 5. solves
def solver_params(k=500, tol=1e-8):
    return hip.SolverParams(solver_type=0, num_blocks=50, max_iters=k, max_restarts=10 ** 6, tol=tol)


@pytest.mark.parametrize("name,fill,sweeps", [("stencil", 0, 1), ("stencil", 4, 2), ("wall42", 0, 1), ("wall42", 4, 3), ("spd", 1, 1),
                                              ("spd", 4, 2), ("tgv16", 0, 1), ("tgv16", 1, 3), ("lap96s", 0, 1), ("lap96s", 4, 3)])
def test_solves_against_the_reference(gpu_ctx, dev, name, fill, sweeps):
    _, _, _, b, singular, A_h = system(name)
    n = A_h.shape[0]
    A = dev(name)
    M = make(gpu_ctx, A, name, fill, sweeps)
    null = kr.unit_null(None, n) if singular else None
    ref = kr.gmres_iterates(A_h, b, np.zeros(n), KS, 50, reference_minv(M, name, fill, sweeps), null)
    kref = cr.first_below(ref, 1e-8)
    assert kref is not None
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=solver_params())
    M.close()
    gx = kr.iterate_gap(x, ref[info.iters].x) if info.iters in ref else np.inf
    bp = kr._proj(b, null)
    eres = kr.true_residual_norm(A_h, bp, x, null) / np.linalg.norm(bp)
    print("amg-ilu-solve %-8s fill %d sweeps %d iters %d reference %d x gap %.2e explicit residual %.2e" %
          (name, fill, sweeps, info.iters, kref, gx, eres))
    assert info.converged == 1 and eres <= 1e-7
    assert abs(info.iters - kref) <= 1, (info.iters, kref)
    assert gx <= 1e-6


def test_the_string_form_is_the_default_parameter_set(gpu_ctx, dev):
    n = system("wall42")[5].shape[0]
    r = rhs(n, 13)
    M = hip.Precond(gpu_ctx, dev("wall42"), "sa-amg-ilu0", 512)
    Mp = hip.PrecondAMG(gpu_ctx, dev("wall42"), params=hip.AmgParams(smoother=4))
    assert hip.AmgParams().ilu_fill == 0 and hip.AmgParams().smoother == 0
    assert np.array_equal(M.apply(r), Mp.apply(r))
    M4 = hip.Precond(gpu_ctx, dev("wall42"), "sa-amg-ilu4", 512)
    Mp4 = hip.PrecondAMG(gpu_ctx, dev("wall42"), params=hip.AmgParams(smoother=4, ilu_fill=4))
    assert np.array_equal(M4.apply(r), Mp4.apply(r)) and not np.array_equal(M4.apply(r), M.apply(r))
    for P in (M, Mp, M4, Mp4):
        P.close()
    for bad in ("sa-amg-ilu9", "sa-amg-ilu", "sa-amg-ilu1x"):
        with pytest.raises(hip.IsphError, match="unknown preconditioner type"):
            hip.Precond(gpu_ctx, dev("wall42"), bad, 512)


def test_multi_path_is_one_vector_after_the_other(gpu_ctx, dev):
    M = make(gpu_ctx, dev("wall42"), "wall42", 1, 2)
    assert M.multi_path(2) == 0 and M.multi_path(3) == 0
    M.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(gpu_ctx, dev):
    A = dev("wall42")
    for fill in (-1, 9):
        with pytest.raises(hip.IsphError, match="ilu_fill"):
            hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=4, ilu_fill=fill, **AMG_KW))
    with pytest.raises(hip.IsphError, match="cycle_bits = 32 needs the Chebyshev smoother"):
        hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=4, cycle_bits=32, **AMG_KW))
    with pytest.raises(hip.IsphError, match="cheb_value_bits = 32 needs the Chebyshev smoother"):
        hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=4, cheb_value_bits=32, **AMG_KW))
    for other in (3, 5, -1):      # 3 names no smoother: refused as before
        with pytest.raises(hip.IsphError, match="smoother must be"):
            hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=other, **AMG_KW))
    # ilu_fill is read with smoother 4 only
    M = hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=0, ilu_fill=9, **AMG_KW))
    M0 = hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=0, **AMG_KW))
    r = rhs(1764)
    assert np.array_equal(M.apply(r), M0.apply(r))
    M.close(); M0.close()


# ---------------------------------------------------------------- 7. memory
@pytest.mark.parametrize("name", ["spd", "tgv16"])
def test_create_and_destroy_leave_the_pool_where_it_was(gpu_ctx, dev, name):
    A = dev(name)
    r = rhs(system(name)[5].shape[0])
    make(gpu_ctx, A, name, 1, 2).close()      # (the first build may fill the cache)
    before, seen = hip.pool_info(), []
    for _ in range(3):
        M = make(gpu_ctx, A, name, 1, 2)
        M.apply(r)
        M.close()
        seen.append(hip.pool_info())
    print("amg-ilu-pool %-8s before %s after %s" % (name, before, seen))
    assert all(s["live"] == before["live"] for s in seen)


# ---------------------------------------------------------------- 8. two ranks
def _rank_solve(rank, G, dim, pgrid, n):
    import oracle as orc
    import test_gpu_ranks as tr
    st = tr._rank_setup(rank, G, dim, pgrid, n, orc.NULLSPACE)
    ctx, A = st["ctx"], st["A"]
    try:
        nl = st["nl"]
        ntot = float(np.prod(pgrid[:dim])) * n ** dim
        M = hip.PrecondAMG(ctx, A, nullvec=np.full(nl, 1.0 / np.sqrt(ntot)),
                           params=hip.AmgParams(smoother=4, ilu_fill=1, sweeps=2, theta=0.02, block=256, coarse_max=64))
        x, bb = np.zeros(nl), st["b"].copy()
        info = hip.solve(ctx, A, bb, x, prec=M, singular=True)
        M.close()
        return dict(nl=nl, rtag=st["rtag"], col_tag=st["col_tag"], csr=st["csr"], b=st["b"], x=x,
                    info=(info.converged, info.iters, info.rel_res_explicit))
    finally:
        A.close()
        ctx.close()


def _global_system(res):
    """the ranks' rows as one matrix in rank-concatenated order, entry for entry what the ranks hold"""
    tags = np.concatenate([r["rtag"] for r in res])
    pos = np.zeros(int(tags.max()) + 1, dtype=np.int64)
    pos[tags] = np.arange(len(tags))
    rows, cols, vals = [], [], []
    off = 0
    for r in res:
        rp, ci, v = r["csr"]
        if r["nl"] > 0:
            rows.append(off + np.repeat(np.arange(r["nl"]), np.diff(rp)))
            cols.append(pos[r["col_tag"][ci]])
            vals.append(v)
        off += r["nl"]
    N = len(tags)
    A = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    A.sort_indices()
    return A, np.concatenate([r["b"] for r in res])


def test_two_ranks_on_one_gpu(gpu_ctx):
    from ranks import RankGroup
    dim, pgrid, n = 3, (2, 1, 1), 8
    G = RankGroup(2)
    try:
        res = G.run(_rank_solve, dim, pgrid, n)
    finally:
        G.close()
    Ag, bg = _global_system(res)
    N = Ag.shape[0]
    infos = {r["info"][:2] for r in res}
    assert len(infos) == 1, infos
    conv, iters = infos.pop()
    assert conv == 1
    x = np.concatenate([r["x"] for r in res])
    proj = lambda v: v - v.mean()
    eres = float(np.linalg.norm(proj(bg - Ag @ x)) / np.linalg.norm(proj(bg)))
    A1 = hip.Matrix.from_csr(gpu_ctx, Ag.indptr.astype(np.int32), Ag.indices.astype(np.int32), Ag.data)
    M1 = hip.PrecondAMG(gpu_ctx, A1, nullvec=np.full(N, 1.0 / np.sqrt(N)),
                        params=hip.AmgParams(smoother=4, ilu_fill=1, sweeps=2, theta=0.02, block=256, coarse_max=64))
    x1 = np.zeros(N)
    i1 = hip.solve(gpu_ctx, A1, bg.copy(), x1, prec=M1, singular=True)
    g = kr.iterate_gap(x, x1)
    print("amg-ilu-ranks iterations %d (one rank %d) x gap %.2e explicit residual %.2e" % (iters, i1.iters, g, eres))
    M1.close(); A1.close()
    assert i1.converged == 1 and eres <= 1e-7
    assert g <= 1e-6
