"""-m gpu: the preconditioner layer by kind -- what isph_prec_create accepts and refuses, what every accessor answers for
an object of another kind, which kinds isph_prec_refactor refuses by name, and the operand routes of isph_prec_apply,
isph_prec_apply_multi and isph_spmv (host or device operands, the caller's row numbering or the library's own).

One system: the pressure Poisson matrix of a 12^3 Taylor-Green cloud with its first fluid row pinned (regular, so "sa-amg"
has a direct coarse solve), assembled once per numbering.  The routes are compared bit for bit (np.array_equal): they
differ in copies and in gathers / scatters, never in arithmetic.  tests/test_gpu_prec_multi.py holds the K-vector forms
themselves and, for the Chebyshev polynomial and the AMG in the caller's numbering, device operands with lda > n.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip, workload
from problems import Problem, tgv_spec

pytestmark = pytest.mark.gpu

KINDS = ["none", "jacobi", "bjacobi-ilu0", "ilu0", "chebyshev2", "sa-amg"]
ACCEPTED = KINDS + ["bjacobi-ilu3", "bjacobi-ilu8", "bjacobi-ilu0-f32", "bjacobi-ilu8-f32", "ilu1", "ilu8", "sa-amg-ilu0",
                    "sa-amg-ilu8", "chebyshev1", "chebyshev9", "chebyshev10", "chebyshev16", "chebyshev1-f32", "chebyshev16-f32"]
REFUSED = ["bjacobi-ilu9", "bjacobi-ilu0-f64", "ilu0-f32", "ilu9", "sa-amg-ilu", "sa-amg-ilu3x", "chebyshev", "chebyshev0",
           "chebyshev17", "chebyshev1x", "chebyshev2-f16", "Jacobi", ""]
NGHOST = 37


@pytest.fixture(scope="module")
def problem():
    return Problem(tgv_spec(dim=3, n=12, mode=workload.ADVECT))


@pytest.fixture(scope="module")
def poisson(problem):
    """the matrix of a context, assembled on first use: in the numbering the context asks for"""
    cache = {}
    pr = problem

    def get(ctx):
        if id(ctx) not in cache:
            cache[id(ctx)], _ = hip.assemble_poisson(ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"],
                                                     np.ascontiguousarray(pr.parts["v"]), vfrac=pr.P.vfrac, singular=hip.PINZERO)
        return cache[id(ctx)]
    yield get
    for A in cache.values():
        A.close()


def precond(ctx, A, kind):
    """the block stream on the library's bricks where the matrix has them; 256 rows per block otherwise (and for the
    Gauss-Seidel block of the AMG, which is no subdomain of the numbering)"""
    return hip.Precond(ctx, A, kind, 0 if kind.startswith("bjacobi") and A.ordering() is not None else 256)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a).ravel(), dtype=torch.float64, device="cuda")


# ---------------------------------------------------------------- 1. the type string
def test_every_accepted_spelling_builds(gpu_ctx_both, poisson):
    A = poisson(gpu_ctx_both)
    r = np.random.default_rng(2).standard_normal(A.info()["nrow"])
    for kind in ACCEPTED:
        M = precond(gpu_ctx_both, A, kind)
        assert np.all(np.isfinite(M.apply(r))), kind
        M.close()


@pytest.mark.parametrize("kind", REFUSED)
def test_every_other_spelling_is_refused(gpu_ctx, poisson, kind):
    with pytest.raises(hip.IsphError, match="unknown preconditioner type"):
        hip.Precond(gpu_ctx, poisson(gpu_ctx), kind, 256)


# ---------------------------------------------------------------- 2. accessors on an object of another kind
def _fails(rc, text):
    assert rc != 0
    msg = hip.lib().isph_last_error().decode()
    assert text in msg, msg


@pytest.mark.parametrize("kind", ["jacobi", "ilu0"])
def test_accessors_of_other_kinds(gpu_ctx, poisson, kind):
    L, ctx = hip.lib(), gpu_ctx
    A = poisson(ctx)
    n, nnz = A.info()["nrow"], A.info()["nnz"]
    M = precond(ctx, A, kind)
    i8, d8 = (C.c_longlong * 16)(), (C.c_double * 8)()
    rows, lp, rp = (np.zeros(n + 1, dtype=np.int32) for _ in range(3))
    rp64 = np.zeros(n + 1, dtype=np.int64)
    ci, v, nv = np.zeros(16 * nnz, dtype=np.int32), np.zeros(16 * nnz), np.ones(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _fails(L.isph_prec_amg_info(ctx.h, M.h, 0, i8), "not an AMG preconditioner")
    _fails(L.isph_prec_amg_export(ctx.h, M.h, 0, 0, p(rp), p(ci), p(v)), "not an AMG preconditioner")
    _fails(L.isph_prec_amg_aggregates(ctx.h, M.h, 0, p(rows)), "not an AMG preconditioner")
    _fails(L.isph_prec_amg_path(ctx.h, M.h, 0, i8), "not an AMG preconditioner")
    _fails(L.isph_prec_amg_set_nullvec(ctx.h, M.h, p(nv), 0), "not an AMG preconditioner, or the null vector is NULL")
    _fails(L.isph_prec_export_ilu(ctx.h, M.h, p(rp), p(ci), p(v)), "not an ILU preconditioner")
    _fails(L.isph_prec_eig_estimate(ctx.h, M.h, 0, d8), "isph_prec_eig_estimate: not a Chebyshev or an AMG preconditioner")
    if kind == "jacobi":
        _fails(L.isph_prec_schwarz_info(M.h, i8), "not a Schwarz preconditioner")
        _fails(L.isph_prec_schwarz_paths(M.h, i8), "not a Schwarz preconditioner")
        _fails(L.isph_prec_schwarz_timing(M.h, d8), "not a Schwarz preconditioner")
        _fails(L.isph_prec_schwarz_export(ctx.h, M.h, p(rows), p(lp), p(rp64), p(ci), p(v)), "bad argument")
    else:                                                   # the object's own kind: they answer
        assert L.isph_prec_schwarz_info(M.h, i8) == 0 and i8[0] == n and i8[1] <= 16 * nnz and i8[2] == 1
        assert L.isph_prec_schwarz_paths(M.h, i8) == 0
        assert L.isph_prec_schwarz_timing(M.h, d8) == 0
        assert L.isph_prec_schwarz_export(ctx.h, M.h, p(rows), p(lp), p(rp64), p(ci), p(v)) == 0
    assert L.isph_prec_nnz(M.h) == 0 and L.isph_prec_amg_levels(M.h) == 0 and L.isph_prec_amg_refreshes(M.h) == 0
    assert M.value_bits == 0 and M.cycle_bits == 64
    assert M.info() == dict(factor_nnz=0, stream_chunks=0, stream_capacity=0, nblocks=0)
    M.close()


@pytest.mark.parametrize("kind,name", [("none", "none"), ("jacobi", "jacobi"), ("ilu0", "ilu<k> / additive Schwarz")])
def test_refactor_refuses_the_kind_by_name(gpu_ctx_both, poisson, kind, name):
    A = poisson(gpu_ctx_both)
    M = precond(gpu_ctx_both, A, kind)
    with pytest.raises(hip.IsphError) as e:
        M.refactor(A)
    assert 'of type "%s"' % name in str(e.value), str(e.value)
    M.close()


# ---------------------------------------------------------------- 3. operand routes of the applications
@pytest.mark.parametrize("kind", KINDS)
def test_apply_routes_agree_bit_for_bit(gpu_ctx_both, poisson, kind):
    ctx = gpu_ctx_both
    A = poisson(ctx)
    ordered = A.ordering() is not None
    n, K = A.info()["nrow"], 3
    lda = n + 5
    M = precond(ctx, A, kind)
    R = np.zeros((K, lda))
    R[:, :n] = np.random.default_rng(13).standard_normal((K, n))
    ref = np.stack([M.apply(R[k, :n].copy()) for k in range(K)])               # host operands, one vector
    assert np.all(np.isfinite(ref)) and np.all(np.any(ref != 0.0, axis=1))
    for k in range(K):                                                          # device operands, one vector
        assert np.array_equal(M.apply(dev(R[k, :n])).cpu().numpy(), ref[k]), k
    Z = np.full((K, lda), -7.0)                                                 # host operands, nvec 3, lda > n
    M.apply_multi(R, Z)
    assert np.array_equal(Z[:, :n], ref)
    assert np.all(Z[:, n:] == -7.0)                                             # rows beyond n keep what they held
    if ordered or kind not in ("chebyshev2", "sa-amg"):                         # (those two: test_gpu_prec_multi.py)
        Zd = dev(np.full((K, lda), -7.0))
        M.apply_multi(dev(R), Zd, nvec=K, lda=lda)
        Zh = Zd.cpu().numpy().reshape(K, lda)
        assert np.array_equal(Zh[:, :n], ref)
        assert np.all(Zh[:, n:] == -7.0)
    M.close()


# ---------------------------------------------------------------- 4. operand routes of the product
def _spmv_check(A, A_h, x, device_route=True):
    y = A.spmv(x.copy())
    if device_route:
        assert np.array_equal(y, A.spmv(dev(x)).cpu().numpy())
    # 1e-13 ||A||_inf ||x||_inf: a thousand roundings of the row's magnitude, where a row of up to 114 entries takes a few
    # hundred at the very worst
    bound = 1e-13 * abs(A_h).sum(axis=1).max() * np.abs(x).max()
    err = np.max(np.abs(y - A_h @ x))
    print("spmv: error %.3e, bound %.3e, widest row %d" % (err, bound, np.diff(A_h.indptr).max()))
    assert err <= bound


def test_spmv_routes(gpu_ctx_both, poisson):
    A = poisson(gpu_ctx_both)
    rp, ci, val = A.export_csr()
    n = len(rp) - 1
    A_h = sps.csr_matrix((val, ci, rp), shape=(n, n))
    _spmv_check(A, A_h, np.random.default_rng(3).standard_normal(n))


def test_spmv_with_the_callers_ghost_values(gpu_ctx_both, poisson, problem):
    """ncol > nrow and no halo plan: x holds the ghost values behind the owned ones"""
    ctx = gpu_ctx_both
    A = poisson(ctx)
    ordered = A.ordering() is not None
    rp, ci, val = A.export_csr()
    n = len(rp) - 1
    G = sps.random(n, NGHOST, density=0.02, random_state=np.random.default_rng(4), data_rvs=np.random.default_rng(5).standard_normal)
    A_h = sps.hstack([sps.csr_matrix((val, ci, rp), shape=(n, n)), G]).tocsr()
    A_h.sort_indices()
    assert A_h[:, n:].nnz > 0
    args = (A_h.indptr.astype(np.int32), A_h.indices.astype(np.int32), A_h.data)
    if ordered:
        Ag = hip.Matrix.from_host_csr_with_coords(ctx, *args, problem.parts["x"], dim=3, ncol=n + NGHOST)
    else:
        Ag = hip.Matrix.from_csr(ctx, *args, ncol=n + NGHOST)
    assert (Ag.ordering() is not None) == ordered
    x = np.random.default_rng(6).standard_normal(n + NGHOST)
    _spmv_check(Ag, A_h, x, device_route=ordered)
    if not ordered:
        # Pinned as found: device operands in the caller's numbering go to the product that wants a halo plan for the ghost
        # columns, and are refused; host operands, and both routes of an ordered matrix, read the caller's ghost values.
        with pytest.raises(hip.IsphError, match="a matrix with a halo needs a context"):
            Ag.spmv(dev(x))
    Ag.close()
