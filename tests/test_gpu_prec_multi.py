"""-m gpu: one preconditioner applied to several vectors per sweep -- isph_prec_apply_multi / isph_prec_multi_path, and
through them the lockstep solve (isph_solve with nvec > 1) and isph_solve_block.

The contract is bit identity with one application per vector (the K-vector kernels run every vector through the single
kernels' operations in their order), so every comparison here is np.array_equal: no tolerance is needed or allowed.

Fixtures (chebyshev_reference.system): stencil (210 rows: three slices and a tail of 18, n no multiple of 4, 32-bit-column
coarse operators), wall42 (a tail slice), tgv16 (four 16-bit windows; singular, with its null vector), spd (three AMG
levels: restriction, prolongation, the A P shortcut and the dense coarsest solve all run); and `ladder`, built here: one
slice per width around the K-vector walk's trip of TRIP pairs -- shorter than a trip (its tail loop alone), exactly one or
two trips (the unrolled loop with an empty tail), longer (both) -- every row with a dominant diagonal, 659 rows (odd).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip
import chebyshev_reference as cr

pytestmark = pytest.mark.gpu

DEGREES = [1, 2, 3, 4, 7]  # both parities of the ping-pong, the product-free degree 1
AMG_KW = dict(theta=0.0, block=256, coarse_max=64)
FIXTURES = ["stencil", "wall42", "tgv16", "spd", "ladder"]
KS = [2, 3, 4]
TRIP = 4                   # kSellMultiUnroll (csrc/sell.hpp): pairs of entries per unrolled trip of the K-vector walk
LADDER_NPAIR = [1, 3, 4, 8, 5, 7, 9, 12, 2, 16]   # one slice of 64 rows each; then 19 rows of 6 pairs: the tail slice


def ladder():
    """Symmetric, diagonally dominant: inside slice s every row is coupled to its p neighbours on either side (cyclically
    within the slice), and row i to rows i - 64 and i + 64, so the slice's width in pairs is LADDER_NPAIR[s] -- below TRIP,
    on TRIP, 2 TRIP and 4 TRIP, above TRIP -- and 6 in the tail slice; off-diagonal entries in (-1, 0), the diagonal 1 + their
    absolute sum"""
    rng = np.random.default_rng(77)
    sizes = [64] * len(LADDER_NPAIR) + [19]
    n = sum(sizes)
    ii, jj = [], []
    base = 0
    for s, size in enumerate(sizes):
        want = LADDER_NPAIR[s] if s < len(LADDER_NPAIR) else 6
        both = 0 < s < len(sizes) - 1                       # a neighbour slice on either side
        p = want - 2 if both else want - 1 if s == 0 else 5
        for j in range(size):
            for k in range(1, p + 1):
                ii.append(base + j); jj.append(base + (j + k) % size)
            if base + j + 64 < n:
                ii.append(base + j); jj.append(base + j + 64)
        base += size
    U = sps.coo_matrix((-rng.uniform(0.05, 1.0, size=len(ii)), (ii, jj)), shape=(n, n)).tocsr()
    U.sum_duplicates()                                      # (2 p + 1 = the slice: a pair met from both sides)
    A = (U + U.T).tocsr()
    A = (A + sps.diags(1.0 + np.asarray(abs(A).sum(axis=1)).ravel())).tocsr()
    A.sort_indices()
    npair = [(int(np.diff(A.indptr)[r:r + 64].max()) + 1) // 2 for r in range(0, n, 64)]
    assert n % 2 == 1 and npair == LADDER_NPAIR + [6], npair
    assert any(q < TRIP for q in npair) and any(q % TRIP == 0 for q in npair) and any(q > TRIP and q % TRIP for q in npair)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), rng.standard_normal(n), False


@functools.lru_cache(maxsize=None)
def system(name):
    rp, ci, val, b, singular = ladder() if name == "ladder" else cr.system(name)
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


def vectors(n, K, seed=5):
    return np.random.default_rng(seed).standard_normal((K, n))


def amg(ctx, A, name, **kw):
    _, _, _, _, singular, A_h = system(name)
    n = A_h.shape[0]
    nv = np.ones(n) / np.sqrt(n) if singular else None
    prm = dict(AMG_KW, smoother=2, sweeps=2)
    prm.update(kw)
    return hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(**prm))


def singles(M, R):
    return np.stack([M.apply(R[k].copy()) for k in range(R.shape[0])])


def check_multi(M, n, Ks=KS, path=1, seed=5):
    for K in Ks:
        R = vectors(n, K, seed + K)
        ref = singles(M, R)
        assert M.multi_path(K) == path, (K, M.multi_path(K))
        Z = M.apply_multi(R)
        assert Z.shape == (K, n)
        assert np.array_equal(Z, ref), (K, float(np.max(np.abs(Z - ref))))


# ---------------------------------------------------------------- 1. apply_multi equals K apply calls
@pytest.mark.parametrize("value_bits", [64, 32])
@pytest.mark.parametrize("name", FIXTURES)
def test_chebyshev_apply_multi_is_k_applies(gpu_ctx, dev, name, value_bits):
    n = system(name)[5].shape[0]
    for d in DEGREES:
        M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, value_bits=value_bits)
        check_multi(M, n)
        M.close()


@pytest.mark.parametrize("value_bits", [64, 32])
@pytest.mark.parametrize("name", FIXTURES)
def test_amg_apply_multi_is_k_applies(gpu_ctx, dev, name, value_bits):
    n = system(name)[5].shape[0]
    for sweeps in (1, 2, 3):
        M = amg(gpu_ctx, dev(name), name, sweeps=sweeps, cheb_value_bits=value_bits)
        if name == "spd":
            assert M.levels >= 3
        check_multi(M, n)
        M.close()


# ---------------------------------------------------------------- 2. pointer alignment
def device_columns(M, n, lda, K, seed):
    """device operands [lda x K]: every column against its own apply; the padding rows of Z keep what they held"""
    import torch
    R = np.zeros((K, lda))
    R[:, :n] = vectors(n, K, seed)
    Rd = torch.tensor(R.ravel(), dtype=torch.float64, device="cuda")
    Zd = torch.full((K * lda,), -7.0, dtype=torch.float64, device="cuda")
    ref = np.stack([M.apply(Rd[k * lda:k * lda + n]).cpu().numpy() for k in range(K)])
    assert np.array_equal(ref, singles(M, R[:, :n]))
    M.apply_multi(Rd, Zd, nvec=K, lda=lda)
    Z = Zd.cpu().numpy().reshape(K, lda)
    assert np.array_equal(Z[:, :n], ref), K
    assert np.all(Z[:, n:] == -7.0)


@pytest.mark.parametrize("kind", ["cheb", "cheb32", "amg"])
@pytest.mark.parametrize("name,pad", [("stencil", 7), ("spd", 7), ("ladder", 0), ("ladder", 7)])
def test_columns_that_are_only_8_byte_aligned(gpu_ctx, dev, name, pad, kind):
    """lda = n + 7 (odd for the even n of stencil / spd) and lda = n of the odd ladder: the columns behind the first
    start 8 bytes off a 16-byte boundary, where the streaming kernel must take its scalar form; lda = n + 7 of the ladder
    is even, every column aligned"""
    n = system(name)[5].shape[0]
    lda = n + pad
    assert (lda % 2 == 1) == (not (name == "ladder" and pad == 7))
    for d in (1, 2, 3):
        if kind == "amg":
            M = amg(gpu_ctx, dev(name), name, sweeps=d)
        else:
            M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=d, value_bits=32 if kind == "cheb32" else 64)
        for K in KS:
            assert M.multi_path(K) == 1
            device_columns(M, n, lda, K, seed=11 + K)
        M.close()


# ---------------------------------------------------------------- 3. fallbacks
@pytest.mark.parametrize("name", ["wall42", "spd"])
def test_fallbacks_apply_one_vector_after_the_other(gpu_ctx, dev, name, monkeypatch):
    n = system(name)[5].shape[0]
    for kw in (dict(smoother=0), dict(smoother=1), dict(cycle_bits=32)):
        M = amg(gpu_ctx, dev(name), name, **kw)
        check_multi(M, n, path=0)
        M.close()
    monkeypatch.setenv("ISPH_PREC_MULTI_SINGLE", "1")
    forced = [amg(gpu_ctx, dev(name), name), hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3),
              hip.Precond(gpu_ctx, dev(name), "bjacobi-ilu0", 256)]
    monkeypatch.delenv("ISPH_PREC_MULTI_SINGLE")
    for M in forced:                                       # read at creation: the objects keep the loop
        check_multi(M, n, path=0)
        M.close()
    monkeypatch.setenv("ISPH_CHEB_UNFUSED", "1")
    unfused = [amg(gpu_ctx, dev(name), name), hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3)]
    monkeypatch.delenv("ISPH_CHEB_UNFUSED")
    for M in unfused:
        check_multi(M, n, path=0)
        M.close()


@pytest.mark.parametrize("name", ["stencil", "spd"])
def test_one_vector_groups_and_the_block_ilu(gpu_ctx, dev, name):
    n = system(name)[5].shape[0]
    for M in (hip.PrecondChebyshev(gpu_ctx, dev(name), degree=4), amg(gpu_ctx, dev(name), name)):
        assert M.multi_path(1) == 0 and M.multi_path(0) == 0
        r = vectors(n, 1, 3)
        assert np.array_equal(M.apply_multi(r)[0], M.apply(r[0].copy()))
        for K in (5, 7):                                   # groups of four and a rest of one / three
            R = vectors(n, K, 20 + K)
            assert np.array_equal(M.apply_multi(R), singles(M, R)), K
        M.close()
    M = hip.Precond(gpu_ctx, dev(name), "bjacobi-ilu0", 256)
    check_multi(M, n, path=1)
    assert M.multi_path(1) == 0
    M.close()
    for kind in ("jacobi", "none"):
        M = hip.Precond(gpu_ctx, dev(name), kind, 0)
        check_multi(M, n, path=0)
        M.close()


# ---------------------------------------------------------------- 4. a single apply after an apply_multi
@pytest.mark.parametrize("name", ["stencil", "tgv16", "spd"])
def test_single_apply_after_a_multi_one(gpu_ctx, dev, name):
    n = system(name)[5].shape[0]
    r = vectors(n, 1, 9)[0]
    for M in (hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3), hip.PrecondChebyshev(gpu_ctx, dev(name), degree=4, value_bits=32),
              amg(gpu_ctx, dev(name), name)):
        before = M.apply(r.copy())
        for K in (2, 4, 3):                                # the K-fold vectors are taken, grown, and reused
            M.apply_multi(vectors(n, K, 30 + K))
            assert np.array_equal(M.apply(r.copy()), before), K
        M.close()


# ---------------------------------------------------------------- 5. lockstep
def lockstep_system(A_h, M):
    """three columns that converge at different iterations (the active set shrinks 3 -> 2 -> 1).  b = A u with u a seeded
    random vector after 60, 8 and 0 steps of u <- (I - M^-1 A) u: the more steps, the fewer eigenvectors of M^-1 A are left
    in u, and GMRES on A M^-1 is done with b = A u after as many iterations as u has components (an eigenvector: one).
    The last column also starts from a random guess."""
    n = A_h.shape[0]
    rng = np.random.default_rng(41)
    v = rng.standard_normal(n)
    B, X0 = np.zeros((3, n)), np.zeros((3, n))
    for c, steps in enumerate((60, 8, 0)):
        u = v.copy()
        for _ in range(steps):
            u = u - M.apply(A_h @ u)
            u /= np.linalg.norm(u)
        B[c] = A_h @ u
    X0[2] = 0.1 * rng.standard_normal(n)
    return B, X0


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("kind", ["cheb", "amg"])
@pytest.mark.parametrize("name", ["wall42", "spd"])
def test_lockstep_columns_are_their_single_solves(gpu_ctx, dev, name, kind, forced, monkeypatch):
    A_h = system(name)[5]
    n = A_h.shape[0]
    if forced:
        monkeypatch.setenv("ISPH_PREC_MULTI_SINGLE", "1")
    M = hip.PrecondChebyshev(gpu_ctx, dev(name), degree=3) if kind == "cheb" else amg(gpu_ctx, dev(name), name)
    if forced:
        monkeypatch.delenv("ISPH_PREC_MULTI_SINGLE")
    assert M.multi_path(3) == (0 if forced else 1)
    prm = hip.SolverParams(num_blocks=30, max_iters=500, max_restarts=10 ** 6, tol=1e-9)
    B, X0 = lockstep_system(A_h, M)
    bflat, xflat = B.ravel().copy(), X0.ravel().copy()
    info = hip.solve(gpu_ctx, dev(name), bflat, xflat, prec=M, nvec=3, lda=n, params=prm)
    its = []
    for c in range(3):
        x = X0[c].copy()
        single = hip.solve(gpu_ctx, dev(name), B[c].copy(), x, prec=M, params=prm)
        assert single.converged == 1
        assert np.array_equal(x, xflat[c * n:(c + 1) * n]), c
        its.append(single.iters)
    print("lockstep %s %s forced %d iterations %s" % (name, kind, forced, its))
    assert len(set(its)) == 3, its
    assert info.converged == 1 and info.iters == sum(its)
    M.close()


# ---------------------------------------------------------------- 6. the block solve
@pytest.mark.parametrize("name", ["wall42", "spd"])
def test_block_solve_with_padded_components(gpu_ctx, dev, name, monkeypatch):
    A_h = system(name)[5]
    n = A_h.shape[0]
    lda, A = n + 7, dev(name)
    M = amg(gpu_ctx, A, name)
    monkeypatch.setenv("ISPH_PREC_MULTI_SINGLE", "1")
    Ms = amg(gpu_ctx, A, name)
    monkeypatch.delenv("ISPH_PREC_MULTI_SINGLE")
    assert M.multi_path(2) == 1 and Ms.multi_path(2) == 0
    rhs = vectors(n, 2, 51)
    out = []
    for P in (M, Ms):
        b = np.zeros((2, lda)); b[:, :n] = rhs
        x = np.full((2, lda), 3.25); x[:, :n] = 0.0
        info = hip.solve_block(gpu_ctx, [[A, None], [None, A]], b, x, prec=P, lda=lda)
        assert info.converged == 1
        assert np.all(x[:, n:] == 3.25)                     # padding rows of the multivector untouched
        out.append((x[:, :n].copy(), info.iters))
    assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0])
    M.close(); Ms.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(gpu_ctx, dev):
    import ctypes as C
    n = system("stencil")[5].shape[0]
    M = hip.PrecondChebyshev(gpu_ctx, dev("stencil"), degree=2)
    R, Z = vectors(n, 2, 1), np.zeros((2, n))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = hip.lib()
    assert L.isph_prec_apply_multi(gpu_ctx.h, M.h, 2, p(R), p(Z), n, 0) == 0
    assert L.isph_prec_apply_multi(gpu_ctx.h, M.h, 0, p(R), p(Z), n, 0) != 0          # nvec = 0
    assert L.isph_prec_apply_multi(gpu_ctx.h, M.h, -1, p(R), p(Z), n, 0) != 0
    assert L.isph_prec_apply_multi(gpu_ctx.h, M.h, 2, p(R), p(Z), n - 1, 0) != 0      # lda < n
    assert L.isph_prec_apply_multi(gpu_ctx.h, M.h, 2, None, p(Z), n, 0) != 0
    with pytest.raises(hip.IsphError):
        M.apply_multi(R.ravel(), nvec=0)
    with pytest.raises(hip.IsphError):
        M.apply_multi(R.ravel(), nvec=2, lda=n - 1)
    M.close()
