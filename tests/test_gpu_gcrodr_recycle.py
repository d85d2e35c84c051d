"""-m gpu: "Recycling GMRES" with the recycle space carried from one solve to the next (isph_solve_recycle, isph_recycle;
csrc/gcrodr.hpp, csrc/tall_skinny.hpp) against the numpy restatement tests/gcrodr_recycle_reference.py, and the two dense
kernels of the handle path alone: k_tall_gemm bit for bit against the fma chain, k_block_gram against the float64 Gram
matrix."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                  # the child process of the ISPH_GCRODR_UNFUSED test
    for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

from isph_amd import build, hip, workload  # noqa: E402
import gcrodr_recycle_reference as rec  # noqa: E402
from problems import Problem, tgv_spec  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- an exact fma in numpy: Dekker's two-product, then the sum of three by rounding to odd (Boldo, Melquiond 2008) -------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    c = 134217729.0                                         # 2^27 + 1 (Veltkamp split)
    ta, tb = c * a, c * b
    ah, bh = ta - (ta - a), tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_np(a, b, c):
    """round(a b + c) with one rounding, elementwise (no overflow, no subnormal products: the data here is O(1))"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    ph, pl = _two_prod(a, b)                                # a b = ph + pl exactly
    sh, sl = _two_sum(ph, c)                                # ph + c = sh + sl exactly
    v, e = _two_sum(sl, pl)                                 # v = RN(sl + pl), e its error
    bits = v.view(np.int64).copy()
    fix = (e != 0.0) & ((bits & 1) == 0)                    # round to odd: an inexact even result moves towards the error
    away = (e > 0.0) == (v > 0.0)
    bits = np.where(fix, np.where(v == 0.0, bits, bits + np.where(away, 1, -1)), bits)
    vo = np.where(fix & (v == 0.0), e, bits.view(np.float64))
    return sh + vo


def test_fma_emulation_is_exact():
    rng = np.random.default_rng(0)
    a, b, c = rng.standard_normal((3, 4000))
    c[:1000] = -(a[:1000] * b[:1000]) * (1.0 + rng.integers(-3, 4, 1000) * 2.0 ** -52)     # heavy cancellation
    c[1000:1200] = 0.0
    a[1200:1300] = 0.0
    got = fma_np(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)


def _chain(blocks, coef, start):
    """per output one fma chain over the basis vectors in ascending order: blocks [p, n], coef [p, q], start [q, n]"""
    acc = np.array(start, dtype=np.float64)
    for i in range(blocks.shape[0]):
        acc = fma_np(coef[i][:, None], blocks[i][None, :], acc)
    return acc


def _block(rng, nv, n, ld):
    """nv vectors of n rows, ld apart, as the flat array the C ABI takes (what lies between the vectors is poison)"""
    flat = np.full(ld * max(nv - 1, 0) + n, np.nan)
    for v in range(nv):
        flat[v * ld:v * ld + n] = rng.standard_normal(n)
    return flat


def _vectors(flat, nv, n, ld):
    return np.stack([flat[v * ld:v * ld + n] for v in range(nv)]) if nv else np.zeros((0, n))


def _splits(p):
    return sorted({(p, 0), (0, p), (p // 3, p - p // 3), (p - p // 3, p // 3)})


NS = [1, 63, 64, 65, 257, 4099]
PS = [1, 16, 17, 63]
QS = [1, 4, 17, 24, 25, 62]


def _chain_snapshots(basis, coef, start, at):
    """the chain of _chain, with its state after `at` basis vectors: {p: [q, n]}"""
    acc = np.array(start, dtype=np.float64)
    snap = {}
    for i in range(basis.shape[0]):
        acc = fma_np(coef[i][:, None], basis[i][None, :], acc)
        if i + 1 in at:
            snap[i + 1] = acc.copy()
    return snap


def _as_block(vecs, n, ld):
    flat = np.full(ld * max(len(vecs) - 1, 0) + n, np.nan)
    for v, x in enumerate(vecs):
        flat[v * ld:v * ld + n] = x
    return flat


@pytest.mark.parametrize("n", NS)
def test_tall_gemm_has_the_bits_of_the_fma_chain(gpu_ctx, n):
    """every (p, split, q, set / accumulate) and the in-place triangular form.  Output c depends on column c of the
    coefficients only and the chain over p vectors is a prefix of the chain over more, so one chain over 63 vectors and
    62 outputs per form holds the expected bits of every case: the cases take the leading vectors, rows and columns."""
    rng = np.random.default_rng(n)
    ld = (n + 63) // 64 * 64
    pmax, qmax = max(PS), max(QS)
    basis = rng.standard_normal((pmax, n))
    coef = rng.standard_normal((pmax, qmax))
    out0 = rng.standard_normal((qmax, n))
    want = {0: _chain_snapshots(basis, coef, np.zeros((qmax, n)), PS), 1: _chain_snapshots(basis, coef, out0, PS)}
    for p in PS:
        for pa, pb in _splits(p):
            A = _as_block(basis[:pa], n, ld) if pa else None
            B = _as_block(basis[pa:p], n, ld) if pb else None
            for q in QS:
                for mode in (0, 1):                         # set, accumulate
                    out = _as_block(out0[:q], n, ld)
                    hip.dense_tall_gemm(gpu_ctx, n, A, ld, B, ld, coef[:p, :q], out, ld, mode=mode)
                    assert np.array_equal(_vectors(out, q, n, ld), want[mode][p][:q]), (n, pa, pb, q, mode)
                    gap = np.ones(out.size, dtype=bool)
                    for v in range(q):
                        gap[v * ld:v * ld + n] = False
                    assert np.all(np.isnan(out[gap]))       # nothing written between the vectors
    # X <- X T in place, T upper triangular: column c of the p x p case is column c of the 63 x 63 one
    T = np.triu(rng.standard_normal((pmax, pmax)))
    tri = _chain(basis, T, np.zeros((pmax, n)))
    for p in PS:
        X = _as_block(basis[:p], n, ld)
        hip.dense_tall_gemm(gpu_ctx, n, X, ld, None, ld, T[:p, :p], None, ld, mode=2)
        assert np.array_equal(_vectors(X, p, n, ld), tri[:p]), (n, p)
        assert np.array_equal(np.isnan(X), np.isnan(_as_block(basis[:p], n, ld)))


@pytest.mark.parametrize("n", NS)
def test_block_gram_against_float64_and_run_to_run(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    ld = (n + 63) // 64 * 64
    for p in PS:
        for pa, pb in _splits(p):
            XA = _block(rng, pa, n, ld) if pa else None
            XB = _block(rng, pb, n, ld) if pb else None
            X = np.concatenate([_vectors(XA, pa, n, ld), _vectors(XB, pb, n, ld)])
            for q in QS:
                Yf = _block(rng, q, n, ld)
                Y = _vectors(Yf, q, n, ld)
                G1 = hip.dense_block_gram(gpu_ctx, n, XA, ld, XB, ld, Yf, ld)
                G2 = hip.dense_block_gram(gpu_ctx, n, XA, ld, XB, ld, Yf, ld)
                assert np.array_equal(G1, G2), (n, pa, pb, q)
                bound = 1e-12 * np.outer(np.linalg.norm(X, axis=1), np.linalg.norm(Y, axis=1))
                assert np.all(np.abs(G1 - X @ Y.T) <= bound), (n, pa, pb, q)


def test_kernels_take_device_operands(gpu_ctx):
    import torch
    rng = np.random.default_rng(7)
    n, ld, p, q = 257, 320, 17, 25
    A = _block(rng, p, n, ld)
    coef = rng.standard_normal((p, q))
    out = torch.zeros(ld * (q - 1) + n, dtype=torch.float64, device="cuda")
    hip.dense_tall_gemm(gpu_ctx, n, torch.from_numpy(A).cuda(), ld, None, ld, coef, out, ld, mode=0)
    want = _chain(_vectors(A, p, n, ld), coef, np.zeros((q, n)))
    assert np.array_equal(_vectors(out.cpu().numpy(), q, n, ld), want)
    G = hip.dense_block_gram(gpu_ctx, n, torch.from_numpy(A).cuda(), ld, None, ld, out, ld)
    assert np.all(np.abs(G - _vectors(A, p, n, ld) @ want.T) <= 1e-12 * np.outer(np.linalg.norm(_vectors(A, p, n, ld), axis=1),
                                                                               np.linalg.norm(want, axis=1)))


# ---- solves --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jitter16():
    return Problem(tgv_spec(dim=3, n=16, mode=workload.JITTER)).poisson()


_REF = {}


def _reference(name):
    """(systems, carried restatement results) of sequence `name`, computed once"""
    if name not in _REF:
        _, _, prec, m, k = rec.SEQUENCES[name]
        systems = rec.sequence_systems(name, coords=True)
        _REF[name] = (systems, rec.run_sequence([s[:4] for s in systems], prec, m, k, carry=True))
    return _REF[name]


def _prm(m, k):
    return hip.SolverParams(solver_type=2, num_blocks=m, num_recycled=k)


def _gpu_solve(ctx, system, prec, m, k, space, singular=True, make=None):
    rp, ci, val, b = system[:4]
    A = make(rp, ci, val) if make else hip.Matrix.from_csr(ctx, rp, ci, val)
    M = hip.Precond(ctx, A, prec, 256)
    x = np.zeros(len(b))
    info = hip.solve(ctx, A, b.copy(), x, prec=M, singular=singular, params=_prm(m, k), recycle=space)
    M.close()
    A.close()
    return x, info


def _check_against(x, info, ri, xr, ir):
    assert info.converged == 1 and ir["converged"]
    assert abs(info.iters - ir["iters"]) <= 1, (info.iters, ir["iters"])
    assert info.restarts == ir["restarts"]
    assert ri["applications"] == ir["applications"] and ri["steps"] == info.iters
    assert np.linalg.norm(x - xr) <= 1e-6 * np.linalg.norm(xr)


@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_sequence_with_a_carried_space_matches_the_restatement(gpu_ctx, name):
    _, _, prec, m, k = rec.SEQUENCES[name]
    systems, ref = _reference(name)
    space = hip.RecycleSpace(gpu_ctx)
    try:
        for s, system in enumerate(systems):
            x, info = _gpu_solve(gpu_ctx, system, prec, m, k, space)
            ri = space.info()
            print(name, s, "iters %d (restatement %d) applications %d vectors %d" % (info.iters, ref[s][1]["iters"],
                                                                                   ri["applications"], ri["vectors"]))
            _check_against(x, info, ri, *ref[s])
            assert abs(x.mean()) < 1e-12 * np.abs(x).max()
            assert ri["n"] == len(x) and ri["started"] == s and ri["discarded"] == 0 and ri["bytes"] >= 8 * len(x) * ri["vectors"]
    finally:
        space.close()


@pytest.mark.parametrize("m,k,prec", rec.PAIRS_D)
def test_same_system_twice(gpu_ctx, jitter16, m, k, prec):
    ref = rec.run_sequence([jitter16, jitter16], prec, m, k, carry=True)
    space = hip.RecycleSpace(gpu_ctx)
    try:
        for s in range(2):
            x, info = _gpu_solve(gpu_ctx, jitter16, prec, m, k, space)
            _check_against(x, info, space.info(), *ref[s])
            assert abs(x.mean()) < 1e-12 * np.abs(x).max()
        assert space.info()["started"] == 1
    finally:
        space.close()


def test_columns_of_one_call_share_the_space(gpu_ctx):
    """nvec = 3, random right-hand sides, I + A: column 0 rebuilds C for a new matrix (kk applications), columns 1 and 2
    start from U and C as the column before left them.  isph_solve_info holds the SUM of the columns' iterations, so
    iterations +-1 per column can only be asserted as +-3 on that sum; the solutions are compared column by column, and
    the same right-hand sides go through three nvec = 1 calls on a second handle as well, where every call is +-1 against
    its own restatement (there every call after the first rebuilds C: kk applications each)."""
    _, _, prec, m, k = rec.SEQUENCES["E"]
    systems = rec.sequence_systems("E", steps=2)
    rng = np.random.default_rng(5)
    space, single = hip.RecycleSpace(gpu_ctx), hip.RecycleSpace(gpu_ctx)
    U = U1 = None
    try:
        for s, (rp, ci, val, _) in enumerate(systems):
            n = len(rp) - 1
            v2 = rec.helmholtz_like(rp, ci, val)
            B = rng.standard_normal((3, n))
            xr, apps, iters, restarts, C = [], 0, 0, 0, None
            for c in range(3):                              # the restatement, column by column
                xc, ic, U = rec.solve(rp, ci, v2, B[c], num_blocks=m, num_recycled=k, U0=U, C0=C, keep=True)
                assert ic["applications"] == (U.shape[1] if (c == 0 and s > 0) else 0)
                C = ic["C"]
                xr.append(xc)
                apps, iters, restarts = apps + ic["applications"], iters + ic["iters"], restarts + ic["restarts"]
            A = hip.Matrix.from_csr(gpu_ctx, rp, ci, v2)
            x = np.zeros(3 * n)
            info = hip.solve(gpu_ctx, A, B.reshape(-1).copy(), x, params=_prm(m, k), nvec=3, lda=n, recycle=space)
            A.close()
            ri = space.info()
            print("system", s, "iters", info.iters, "restatement", iters, "applications", ri["applications"])
            assert info.converged == 1 and abs(info.iters - iters) <= 3 and info.restarts == restarts   # +-1 per column
            assert ri["applications"] == apps == (0 if s == 0 else ri["vectors"])
            for c in range(3):
                assert np.linalg.norm(x[c * n:(c + 1) * n] - xr[c]) <= 1e-6 * np.linalg.norm(xr[c])
            A = hip.Matrix.from_csr(gpu_ctx, rp, ci, v2)
            for c in range(3):                              # one call per column
                kk_in = 0 if U1 is None else U1.shape[1]
                xc, ic, U1 = rec.solve(rp, ci, v2, B[c], num_blocks=m, num_recycled=k, U0=U1, keep=True)
                x1 = np.zeros(n)
                i1 = hip.solve(gpu_ctx, A, B[c].copy(), x1, params=_prm(m, k), recycle=single)
                assert i1.converged == 1 and abs(i1.iters - ic["iters"]) <= 1 and i1.restarts == ic["restarts"]
                assert single.info()["applications"] == ic["applications"] == kk_in
                assert np.linalg.norm(x1 - xc) <= 1e-6 * np.linalg.norm(xc)
            A.close()
    finally:
        space.close()
        single.close()


def _trip_the_guard(ctx, system, prec, m, k, space):
    """hands `space` (holding a space of this system) back with its second vector replaced by the first, solves again;
    returns (iterations and restarts of that solve, of the plain solve, solutions, info of the space)"""
    U = space.export()
    assert U.shape[1] >= 2
    U[:, 1] = U[:, 0]
    before = space.info()
    space.import_(U)
    x, info = _gpu_solve(ctx, system, prec, m, k, space)
    xf, inf = _gpu_solve(ctx, system, prec, m, k, None)
    # the bound of a solve with an empty handle against the plain solve (the restart's W^T U is summed in another order
    # by k_block_gram): iterations +-1, restarts equal, x to 1e-6
    same = (info.converged == 1 and abs(info.iters - inf.iters) <= 1 and info.restarts == inf.restarts and
            np.linalg.norm(x - xf) <= 1e-6 * np.linalg.norm(xf))
    return same, info.iters, before, space.info()


def test_rank_deficient_space_trips_the_guard_on_the_device(gpu_ctx, jitter16):
    """a space with a repeated vector (isph_recycle_import): kk applications, the second Gram matrix is off the
    identity or a pivot is not positive, the space goes with reason 2 and the solve is the one without a handle; the
    space that solve leaves is usable again"""
    m, k, prec = 12, 6, "jacobi"                            # the pair of PAIRS_D whose second solve saves 5 steps
    space = hip.RecycleSpace(gpu_ctx)
    try:
        _gpu_solve(gpu_ctx, jitter16, prec, m, k, space)
        same, iters, before, ri = _trip_the_guard(gpu_ctx, jitter16, prec, m, k, space)
        assert ri["discarded"] == before["discarded"] + 1 and ri["last_reason"] == 2 and ri["started"] == before["started"]
        assert ri["applications"] == before["vectors"] and ri["vectors"] >= k
        assert same
        x2, i2 = _gpu_solve(gpu_ctx, jitter16, prec, m, k, space)
        ri2 = space.info()
        assert i2.converged == 1 and ri2["started"] == before["started"] + 1 and ri2["discarded"] == ri["discarded"]
        assert i2.iters <= iters - 3
    finally:
        space.close()


def _signed_match(U, Uref, tol):
    assert U.shape == Uref.shape and U.shape[1] > 0
    for c in range(U.shape[1]):
        sgn = 1.0 if U[:, c] @ Uref[:, c] >= 0 else -1.0
        assert np.linalg.norm(U[:, c] - sgn * Uref[:, c]) <= tol * np.linalg.norm(Uref[:, c]), c


def test_space_is_kept_in_the_callers_numbering(gpu_ctx_bricks):
    """sequence B in the library's own row numbering, from shuffled caller rows: the exported space, in the caller's
    numbering, is the one of the unshuffled run -- the gather at entry and the scatter at exit"""
    ctx = gpu_ctx_bricks
    _, _, prec, m, k = rec.SEQUENCES["B"]
    systems, ref = _reference("B")
    n = len(systems[0][3])
    shuffle = np.random.default_rng(11).permutation(n)      # caller row i of the shuffled run = row shuffle[i]

    def run(perm):
        space = hip.RecycleSpace(ctx)
        out = []
        try:
            for s, (rp, ci, val, b, xyz) in enumerate(systems):
                Ap = sps.csr_matrix((val, ci, rp), shape=(n, n))[perm][:, perm].tocsr()
                Ap.sort_indices()
                make = lambda *_: hip.Matrix.from_host_csr_with_coords(ctx, Ap.indptr.astype(np.int32), Ap.indices.astype(np.int32),
                                                                        Ap.data, np.ascontiguousarray(xyz[perm, :2]), dim=2)
                x, info = _gpu_solve(ctx, (rp, ci, val, b[perm]), prec, m, k, space, make=make)
                U = space.export()
                back = np.argsort(perm)
                out.append((x[back], info, space.info(), U[back]))
        finally:
            space.close()
        return out

    plain, shuffled = run(np.arange(n)), run(shuffle)
    for s in range(len(systems)):
        (xp, ip, rip, Up), (xs, is_, ris, Us) = plain[s], shuffled[s]
        _check_against(xp, ip, rip, *ref[s])
        _check_against(xs, is_, ris, *ref[s])
        assert is_.iters == ip.iters and ris["vectors"] == rip["vectors"] > 0
        _signed_match(Us, Up, 1e-8)
    assert plain[-1][2]["started"] == len(systems) - 1


def test_empty_handle_is_the_plain_solve(gpu_ctx, jitter16):
    m, k, prec = 20, 5, "bjacobi-ilu0"
    rp, ci, val, b = jitter16
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, prec, 256)
    x0 = np.zeros(len(b))
    i0 = hip.solve(gpu_ctx, A, b.copy(), x0, prec=M, singular=True, params=_prm(m, k))
    space = hip.RecycleSpace(gpu_ctx)
    x1 = np.zeros(len(b))
    i1 = hip.solve(gpu_ctx, A, b.copy(), x1, prec=M, singular=True, params=_prm(m, k), recycle=space)
    assert i0.converged == 1 and i1.converged == 1 and abs(i1.iters - i0.iters) <= 1
    assert np.linalg.norm(x1 - x0) <= 1e-6 * np.linalg.norm(x0)
    assert space.info()["vectors"] >= k and space.info()["started"] == 0
    space.close()
    M.close()
    A.close()


def _child(out):
    """sequence B with a handle, in this process's environment; iterations and solutions to `out`"""
    hip.DEFAULT_ORDERING = "caller"
    _, _, prec, m, k = rec.SEQUENCES["B"]
    systems = rec.sequence_systems("B")
    ctx = hip.Context(0)
    space = hip.RecycleSpace(ctx)
    its, xs = [], []
    for system in systems:
        x, info = _gpu_solve(ctx, system, prec, m, k, space)
        its.append((info.converged, info.iters, info.restarts, space.info()["applications"]))
        xs.append(x)
    same, _, before, ri = _trip_the_guard(ctx, systems[-1], prec, m, k, space)   # the guard with the per-column launches
    guard = (same and ri["last_reason"] == 2 and ri["discarded"] == before["discarded"] + 1 and
             ri["applications"] == before["vectors"])
    space.close()
    ctx.close()
    np.savez(out, its=np.array(its), xs=np.array(xs), guard=np.array(int(guard)))


def test_unfused_launches_give_the_same_solves(gpu_ctx, tmp_path):
    """ISPH_GCRODR_UNFUSED=1 is read when a handle is created: a fresh child process runs sequence B with the per-column
    launches"""
    _, _, prec, m, k = rec.SEQUENCES["B"]
    systems, ref = _reference("B")
    out = str(tmp_path / "unfused.npz")
    env = dict(os.environ, ISPH_GCRODR_UNFUSED="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    d = np.load(out)
    assert int(d["guard"]) == 1, "the guard with the per-column launches did not fall back to the plain solve"
    space = hip.RecycleSpace(gpu_ctx)
    try:
        for s, system in enumerate(systems):
            x, info = _gpu_solve(gpu_ctx, system, prec, m, k, space)
            conv, iters, restarts, apps = (int(v) for v in d["its"][s])
            assert conv == 1 and abs(iters - info.iters) <= 1 and apps == space.info()["applications"]
            assert np.linalg.norm(d["xs"][s] - x) <= 1e-6 * np.linalg.norm(x)
            assert abs(iters - ref[s][1]["iters"]) <= 1
    finally:
        space.close()


def test_refusals_and_discards(gpu_ctx, jitter16):
    rp, ci, val, b = jitter16
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    space = hip.RecycleSpace(gpu_ctx)
    x = np.zeros(len(b))
    for st in (0, 1):
        with pytest.raises(hip.IsphError, match="recycle handle"):
            hip.solve(gpu_ctx, A, b.copy(), x, singular=True, params=hip.SolverParams(solver_type=st), recycle=space)
    with pytest.raises(hip.IsphError, match="basis_bits"):
        hip.solve(gpu_ctx, A, b.copy(), x, singular=True, recycle=space,
                  params=hip.SolverParams(solver_type=2, num_blocks=20, num_recycled=5, basis_bits=32))
    assert space.info()["vectors"] == 0
    i1 = hip.solve(gpu_ctx, A, b.copy(), x, singular=True, params=_prm(20, 5), recycle=space)
    assert i1.converged == 1 and space.info()["vectors"] >= 5 and space.info()["n"] == len(b)
    # another number of rows: the space goes (reason 1), the solve is the fresh one
    pr2 = Problem(tgv_spec(dim=2, n=16, mode=workload.JITTER))
    rp2, ci2, val2, b2 = pr2.poisson()
    A2 = hip.Matrix.from_csr(gpu_ctx, rp2, ci2, val2)
    x2, x2f = np.zeros(len(b2)), np.zeros(len(b2))
    i2 = hip.solve(gpu_ctx, A2, b2.copy(), x2, singular=True, params=_prm(20, 5), recycle=space)
    i2f = hip.solve(gpu_ctx, A2, b2.copy(), x2f, singular=True, params=_prm(20, 5))
    ri = space.info()
    assert ri["discarded"] == 1 and ri["last_reason"] == 1 and ri["started"] == 0 and ri["applications"] == 0
    assert i2.converged == 1 and i2.iters == i2f.iters and np.array_equal(x2, x2f)
    assert ri["n"] == len(b2)
    # fewer recycled vectors than the space holds: reason 3
    x2[:] = 0.0
    hip.solve(gpu_ctx, A2, b2.copy(), x2, singular=True, params=_prm(20, 5), recycle=space)
    kk = space.info()["vectors"]
    assert kk >= 5
    x2[:] = 0.0
    i3 = hip.solve(gpu_ctx, A2, b2.copy(), x2, singular=True, params=_prm(20, 2), recycle=space)
    ri = space.info()
    assert i3.converged == 1 and ri["discarded"] == 2 and ri["last_reason"] == 3
    space.reset()
    ri = space.info()
    assert ri["vectors"] == 0 and ri["bytes"] == 0 and space.export().shape[1] == 0
    # R = NULL through isph_solve_recycle: the bits of isph_solve
    import ctypes as C
    xa, xb = np.zeros(len(b)), np.zeros(len(b))
    ia = hip.solve(gpu_ctx, A, b.copy(), xa, singular=True, params=_prm(20, 5))
    ib = hip.SolveInfo()
    prm = _prm(20, 5)
    bb = b.copy()
    hip._check(hip.lib().isph_solve_recycle(gpu_ctx.h, A.h, None, hip._ptr(bb), hip._ptr(xb), 1, len(b), 1, None, C.byref(prm),
                                            C.byref(ib), 0, None))
    assert ia.iters == ib.iters and ia.restarts == ib.restarts and np.array_equal(xa, xb)
    space.close()
    A.close()
    A2.close()


# ---- two ranks ---------------------------------------------------------------------------------------------------------------
def _rank_sequence(rank, G, dts, m, k):
    """the Poisson systems of sequence B split 2 x 1, solved in turn with one handle per rank"""
    from isph_amd import dist
    ctx = G.context(rank)
    space = hip.RecycleSpace(ctx)
    out = []
    try:
        for adt in dts:
            spec = workload.TGVSpec(dim=2, ncell=(48, 48), brick=(8, 8), origin=(0.5, 0.5), mode=workload.ADVECT, advect_dt=adt,
                                    pgrid=(2, 1), rank=rank)
            parts = dist.prune_ghosts(workload.make_tgv(spec))
            plan = dist.make_plan(parts, G.td(rank))
            nl = int(parts["nlocal"])
            fwd = hip.HaloForward(ctx, nl, plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
            vfrac = np.ascontiguousarray(dist.forward_scalar_rccl(fwd, plan, hip.compute_volumes(ctx, parts, plan.colmap)))
            fwd.close()
            A, b = hip.assemble_poisson(ctx, parts, plan.colmap, spec.dt, parts["rho"], np.ascontiguousarray(parts["v"]),
                                        vfrac=vfrac, ncol=plan.ncol, singular=hip.NULLSPACE, rank0=(rank == 0))
            if plan.ncol > nl:
                A.set_halo(plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
            M = hip.Precond(ctx, A, "jacobi", 256)
            x = np.zeros(nl)
            info = hip.solve(ctx, A, b.copy(), x, prec=M, singular=True, params=_prm(m, k), recycle=space)
            ri = space.info()
            out.append((info.converged, info.iters, info.restarts, ri["applications"], ri["vectors"], ri["started"]))
            M.close()
            A.close()
    finally:
        space.close()
        ctx.close()
    return out


def test_two_ranks_keep_and_use_their_spaces_together():
    from ranks import RankGroup
    _, _, prec, m, k = rec.SEQUENCES["B"]
    _, ref = _reference("B")
    base = tgv_spec(dim=2, n=48, mode=workload.ADVECT)
    dts = [base.dt * (1.0 + 0.1 * s) for s in range(4)]
    G = RankGroup(2)
    try:
        res = G.run(_rank_sequence, dts, m, k)
    finally:
        G.close()
    assert res[0] == res[1], "the ranks disagree"
    for s, (conv, iters, restarts, apps, vectors, started) in enumerate(res[0]):
        print("solve", s, "iters", iters, "single-rank restatement", ref[s][1]["iters"])
        assert conv == 1 and abs(iters - ref[s][1]["iters"]) <= 1
        assert apps == ref[s][1]["applications"] and started == s


def _rank_same_system_twice(rank, G, m, k):
    """2 x 1 x 1 bricks + one rank without particles: the same Poisson system twice with one handle per rank"""
    from test_gpu_ranks import _rank_setup
    import oracle as orc
    st = _rank_setup(rank, G, 3, (2, 1, 1), 8, orc.NULLSPACE)
    ctx, A = st["ctx"], st["A"]
    space = hip.RecycleSpace(ctx)
    out = []
    try:
        M = hip.Precond(ctx, A, "bjacobi-ilu0", 256)        # what the project's empty-rank solve uses
        for _ in range(3):
            x = np.zeros(st["nl"])
            info = hip.solve(ctx, A, st["b"].copy(), x, prec=M, singular=True, params=_prm(m, k), recycle=space)
            ri = space.info()
            out.append((info.converged, info.iters, info.restarts, ri["applications"], ri["vectors"], ri["started"], ri["discarded"]))
        M.close()
    finally:
        space.close()
        A.close()
        ctx.close()
    return st["nl"], out


def test_a_rank_without_rows_keeps_the_count_of_the_others():
    """a rank that owns no rows holds no values but the same number of vectors, so that the next solve enters the same
    all-reduces on every rank (the Gram matrices of the Cholesky-QR, C^T r0, the norms) and runs cycles of the same length"""
    from ranks import RankGroup
    m, k = 20, 5
    G = RankGroup(3)
    try:
        res = G.run(_rank_same_system_twice, m, k)
    finally:
        G.close()
    assert res[2][0] == 0 and res[0][0] > 0 and res[1][0] > 0
    assert res[0][1] == res[1][1] == res[2][1], "the ranks disagree"
    first, second, third = res[2][1]
    print("iterations", first[1], second[1], third[1], "vectors", first[4])
    assert first[0] == second[0] == third[0] == 1
    assert first[4] >= k and second[3] == first[4] and second[5] == 1 and third[5] == 2 and third[6] == 0
    assert second[1] < first[1]


# ---- the C++ mirror --------------------------------------------------------------------------------------------------
def _driver_input(path, steps=3):
    """per time step a "Helmholtz" system (I + A, random right-hand side) and the "Poisson" system of sequence E"""
    systems = rec.sequence_systems("E", steps=steps)
    rng = np.random.default_rng(9)
    lst = []
    for rp, ci, val, b in systems:
        lst.append(("Helmholtz", 0, rp, ci, rec.helmholtz_like(rp, ci, val), rng.standard_normal(len(b))))
        lst.append(("Poisson", 1, rp, ci, val, b))
    with open(path, "wb") as f:
        f.write(np.int32(len(lst)).tobytes())
        for name, singular, rp, ci, val, b in lst:
            f.write(np.int32(len(name)).tobytes())
            f.write(name.encode())
            f.write(np.array([singular, len(b), len(val)], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(rp, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(ci, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(val, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(b, dtype=np.float64).tobytes())
    return lst


def _parse(stdout):
    solves = [dict(kv.split("=") for kv in l.split()) for l in stdout.splitlines() if l.startswith("name=")]
    spaces = {l.split()[1].split("=")[1]: l for l in stdout.splitlines() if l.startswith("recycle ")}
    return solves, spaces


def test_cpp_mirror_keeps_one_space_per_name(gpu_ctx, tmp_path):
    exe = build.build_cpp_recycle_test()
    _, _, _, m, k = rec.SEQUENCES["E"]
    inp = str(tmp_path / "in.bin")
    lst = _driver_input(inp)
    n = len(lst[0][5])
    runs = {}
    for key in (1, 0, -1):
        out = str(tmp_path / ("out%d.bin" % key))
        r = subprocess.run([exe, inp, out, str(key), str(m), str(k)], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[key] = (r.stdout, np.fromfile(out).reshape(len(lst), n)) + _parse(r.stdout)
    # key = 1: every later solve of a name starts from that name's space
    _, X1, solves, spaces = runs[1]
    assert [s["name"] for s in solves] == ["Helmholtz", "Poisson"] * 3 and all(s["converged"] == "1" for s in solves)
    pois = [int(s["iters"]) for s in solves if s["name"] == "Poisson"]
    print("Poisson iterations", pois, "Helmholtz", [int(s["iters"]) for s in solves if s["name"] == "Helmholtz"])
    assert pois[1] < pois[0] and pois[2] < pois[0]
    for name in ("Helmholtz", "Poisson"):
        assert "started=2 discarded=0" in spaces[name] and "n=%d " % n in spaces[name], spaces[name]
    # setParameters once more, with the same list, before the third Poisson system: the spaces go, that solve is fresh
    out = str(tmp_path / "again.bin")
    r = subprocess.run([exe, inp, out, "1", str(m), str(k), "5"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    again, aspaces = _parse(r.stdout)
    pa = [int(s["iters"]) for s in again if s["name"] == "Poisson"]
    assert pa[:2] == pois[:2] and pa[2] == int(runs[0][2][5]["iters"]) > pois[2]
    assert "started=0" in aspaces["Poisson"] and "none" in aspaces["Helmholtz"]
    # key = 0 and no key: no space is kept, and every solve is the plain solver_type = 2 solve
    assert "none" in runs[0][3]["Poisson"] and "none" in runs[0][3]["Helmholtz"]
    assert [l for l in runs[0][0].splitlines() if l.startswith("name=")] == [l for l in runs[-1][0].splitlines() if l.startswith("name=")]
    assert np.array_equal(runs[0][1], runs[-1][1])
    for s, (name, singular, rp, ci, val, b) in enumerate(lst):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, singular=bool(singular), params=_prm(m, k))
        A.close()
        assert int(runs[0][2][s]["iters"]) == info.iters and int(runs[0][2][s]["restarts"]) == info.restarts
        assert np.linalg.norm(runs[0][1][s] - x) <= 1e-12 * np.linalg.norm(x)
        assert np.linalg.norm(X1[s] - x) <= 1e-6 * np.linalg.norm(x)


if __name__ == "__main__":
    _child(sys.argv[1])
