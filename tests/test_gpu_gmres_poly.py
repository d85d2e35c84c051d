"""-m gpu: the GMRES-polynomial preconditioner "gmres-poly<d>" (csrc/gmres_poly.hpp) against the numpy restatement
tests/gmres_poly_reference.py.

Systems: cyclic = I + 0.5 S_+ + 0.05 S_- with 130 rows (three slices, the last one partial, nonsymmetric: real roots and
conjugate pairs -- which degree gives which pattern is read from the restatement, never assumed); tgv2d12 (2-D TGV, 144
rows) and jitter8 (jittered 3-D, 512 rows), both singular and given their null vector, each in the caller's and in the
library's row numbering; w32 = the 65-window slice of sell_shapes.self_halo("fallback") folded square with a dominant
diagonal (66 620 rows: the 32-bit column kernel).

Bounds.
  Hessenberg matrix against the restatement: max(100 s, 1e-13) max |H|, s the rounding spread of the restatement itself
  (plain, reversed and longdouble accumulation of every dot) -- the rule of tests/test_gpu_eig_estimate.py for the same
  Arnoldi.  The roots of two numberings / rank counts: the same rule with the spread of the restatement's roots.
  Device roots: sigma_min(H^ - theta I) <= 1e-12 ||H^|| on the device's own H^.
  One application against the restatement fed the device's exported roots: 8 g + 1e-13 max |z|, g the gap between the
  restatement in fp64 and in numpy.longdouble on the same inputs (the device contracts fmas and sums rows in another
  order).  Fused against ISPH_POLY_UNFUSED=1: the same bits (the epilogue rounds like the two kernels).
  Solves: the restatement's iteration count +-1 and x within 1e-6 (the project's convention).
Every gap is printed before it is asserted.

Measured on an MI355X: H against the restatement 0 .. 3.0e-16 of max |H| under the floor 1e-13 (tgv2d12 at
d = 25: 5.7e-15 under 2.9e-13, the restatement's spread there 2.9e-15); sigma_min 0 .. 7.6e-16; one application 1.1e-16 ..
2.2e-15 under tolerances of 6.6e-14 .. 4.8e-13 (fp64 against longdouble 9.6e-17 .. 2.3e-15; cyclic at degree 25: 8.9e-16,
w32 8.9e-16); fused against unfused 0 in all 13 cases; roots of the library's numbering against the caller's 9.0e-17 ..
5.4e-16 of max |theta| (against the restatement 5.4e-16 .. 1.6e-15) under 1.0e-13 .. 2.5e-13; two ranks against one 2.0e-16,
their application 4.4e-16 under 4.2e-14, 8 iterations either way; iterations = the restatement's in every solve (cyclic 6,
tgv2d12 8, jitter8 6 and 3 at d = 8; Jacobi 28 / 25 / 18), x within 1.8e-15; pool: 18 432 live bytes with the polynomial of
jitter8, none left after close.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import hip, workload
import chebyshev_reference as cr
import gmres_poly_reference as gp
import krylov_reference as kr
import sell_shapes as sh

pytestmark = pytest.mark.gpu

KS = list(range(1, 81))


class System:
    def __init__(self, A, b, singular, xyz=None, dim=3):
        A = sps.csr_matrix(A)
        A.sort_indices()
        self.A, self.b, self.singular, self.xyz, self.dim = A, b, singular, xyz, dim
        self.n = A.shape[0]
        self.null = np.ones(self.n) / np.sqrt(self.n) if singular else None

    def csr(self):
        return self.A.indptr.astype(np.int32), self.A.indices.astype(np.int32), self.A.data


@functools.lru_cache(maxsize=None)
def system(name):
    rng = np.random.default_rng(31)
    if name == "cyclic":
        n = 130
        t = 2 * np.pi * np.arange(n) / n
        return System(gp.cyclic(n), rng.standard_normal(n), False, np.stack([np.cos(t), np.sin(t), np.zeros(n)], axis=1) * 10.0, 2)
    if name in ("tgv2d12", "jitter8"):
        from problems import Problem, tgv_spec
        pr = Problem(tgv_spec(dim=2, n=12, mode=workload.JITTER, brick=6) if name == "tgv2d12" else
                     tgv_spec(dim=3, n=8, mode=workload.JITTER, brick=8))
        rp, ci, val, b = pr.poisson()
        return System(sps.csr_matrix((val, ci, rp), shape=(pr.n, pr.n)), b, True, np.ascontiguousarray(pr.parts["x"][:pr.n]),
                      2 if name == "tgv2d12" else 3)
    assert name == "w32"
    rp, ci, val, ncol, plan = sh.fixture("halo_fallback")
    n = len(rp) - 1
    F = sps.csr_matrix((np.array(val), sh.fold(ci, n, plan["send_idx"]), np.array(rp)), shape=(n, n))   # (the fixture is read-only)
    F.sum_duplicates()
    F = F - sps.diags(F.diagonal())
    A = F + sps.diags(1.0 + 2.0 * np.asarray(abs(F).sum(axis=1)).ravel())   # D^-1 A = I + N, ||N||_inf <= 1/2: no root near 0
    return System(A, rng.standard_normal(n), False)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = hip.Matrix.from_csr(gpu_ctx, *system(name).csr())
        return cache[name]
    yield get
    for A in cache.values():
        A.close()


def pattern(roots):
    return "".join("p" if b > 0 else "r" for _, b in gp.units_of(roots))


@functools.lru_cache(maxsize=None)
def cyclic_degrees():
    """degrees of the cyclic matrix by what the restatement's roots look like (Philox start vector)"""
    A = system("cyclic").A
    pats = {d: pattern(gp.roots(A, d)) for d in range(1, 13)}
    pick = lambda cond: next(d for d in sorted(pats) if cond(pats[d]))
    out = dict(one_pair_in_front=pick(lambda k: k.startswith("p")),
               mixed=pick(lambda k: "r" in k and "p" in k),
               pair_last=pick(lambda k: len(k) > 1 and k.endswith("p")),
               real_last_behind_a_pair=pick(lambda k: k.endswith("r") and "p" in k),
               real_between_pairs=pick(lambda k: "prp" in k),
               all_pairs=pick(lambda k: len(k) > 1 and set(k) == {"p"}),
               all_real=pick(lambda k: len(k) > 1 and set(k) == {"r"}))
    return out, pats


def bound_from(s):
    return max(100.0 * s, 1e-13)


def check_apply(M, S, r, label):
    """one application against the restatement fed the device's roots, under the measured rounding of the restatement"""
    roots = M.roots()
    z = np.array(M.apply(r))
    zr = gp.apply(S.A, roots, r)
    g, zmax = gp.rounding_gap(S.A, roots, r)
    gap, tol = float(np.max(np.abs(z - zr))), 8.0 * g + 1e-13 * zmax
    print("poly-apply %-28s degree %2d %-8s gap %.2e tolerance %.2e (fp64-longdouble %.2e, max |z| %.2e)" %
          (label, len(roots), pattern(roots), gap, tol, g, zmax))
    assert gap <= tol
    return z


# ---------------------------------------------------------------- 1. Hessenberg matrix and roots
@pytest.mark.parametrize("name,d", [("cyclic", 1), ("cyclic", 5), ("cyclic", 12), ("cyclic", 25), ("tgv2d12", 4), ("tgv2d12", 25),
                                    ("jitter8", 6), ("w32", 4)])
def test_hessenberg_and_roots(gpu_ctx, dev, name, d):
    S = system(name)
    M = hip.PrecondGmresPoly(gpu_ctx, dev(name), d, nullvec=S.null)
    H, roots = M.hessenberg(), M.roots()
    M.close()
    Hr, m, bd, _ = gp.arnoldi(S.A, d, S.null)
    sH, _ = gp.rounding_spread(S.A, d, S.null)
    assert H.shape == Hr.shape == (d + 1, d) and not bd and len(roots) == d
    gap = float(np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)))
    s = gp.sigma_min_bound(gp.harmonic_matrix(H), roots)
    print("poly-hess %-8s d %2d H gap %.2e bound %.2e sigma_min %.2e pattern %s" % (name, d, gap, bound_from(sH), s, pattern(roots)))
    assert gap <= bound_from(sH)
    assert s <= 1e-12
    assert np.array_equal(np.tril(H, -2), np.zeros_like(H))
    if d <= 12:                                    # (at degree 25 two close real roots may come out as a pair on one side)
        assert pattern(roots) == pattern(gp.roots_from_hessenberg(Hr))
    # application order: modified Leja -- largest modulus first, conjugates together (units_of asserts the pairing)
    assert abs(roots[0]) >= np.max(np.abs(roots)) * (1.0 - 4e-16)


# ---------------------------------------------------------------- 2. one application
def test_cyclic_degrees_reach_every_branch_of_the_product_form():
    picks, pats = cyclic_degrees()
    print("poly-patterns", pats, picks)
    k = pats[picks["one_pair_in_front"]]
    roots = gp.roots(system("cyclic").A, picks["one_pair_in_front"])
    assert k[0] == "p" and abs(roots[0].imag) > 1e-3


@pytest.mark.parametrize("which", ["degree1", "one_pair_in_front", "mixed", "pair_last", "real_last_behind_a_pair", "real_between_pairs",
                                   "all_pairs", "all_real", "degree25"])
def test_apply_on_the_cyclic_matrix(gpu_ctx, dev, which):
    S = system("cyclic")
    picks, pats = cyclic_degrees()
    d = {"degree1": 1, "degree25": 25}.get(which) or picks[which]
    M = hip.PrecondGmresPoly(gpu_ctx, dev("cyclic"), d)
    if d in pats:
        assert pattern(M.roots()) == pats[d]       # the premise holds on the device too
    if which == "degree1":
        assert pattern(M.roots()) == "r"
    check_apply(M, S, np.random.default_rng(5).standard_normal(S.n), "cyclic " + which)
    M.close()


@pytest.mark.parametrize("name,d", [("tgv2d12", 1), ("tgv2d12", 4), ("tgv2d12", 9), ("jitter8", 3), ("jitter8", 8), ("w32", 4), ("w32", 7)])
def test_apply_in_both_numberings(gpu_ctx, gpu_ctx_bricks, dev, name, d):
    S = system(name)
    r = np.random.default_rng(6).standard_normal(S.n)
    M = hip.PrecondGmresPoly(gpu_ctx, dev(name), d, nullvec=S.null)
    if name == "w32":
        assert dev(name).column_bits() == 32
    zc = check_apply(M, S, r, name + " caller")
    M.close()
    if S.xyz is None:
        return
    Ab = hip.Matrix.from_host_csr_with_coords(gpu_ctx_bricks, *S.csr(), S.xyz, dim=S.dim)
    assert Ab.ordering() is not None
    Mb = hip.PrecondGmresPoly(gpu_ctx_bricks, Ab, d, nullvec=S.null)
    zb = check_apply(Mb, S, r, name + " bricks")
    Mb.close(); Ab.close()
    assert np.max(np.abs(zb - zc)) <= 1e-10 * np.max(np.abs(zc))     # two polynomials that agree to rounding (section 4)


def test_device_operands_and_the_string_form(gpu_ctx, dev):
    import torch
    S = system("tgv2d12")
    r = np.random.default_rng(7).standard_normal(S.n)
    M = hip.PrecondGmresPoly(gpu_ctx, dev("tgv2d12"), 4, nullvec=S.null)
    Md = hip.PrecondGmresPoly(gpu_ctx, dev("tgv2d12"), 4, nullvec=torch.tensor(S.null, dtype=torch.float64, device="cuda"))
    zh = np.array(M.apply(r))
    assert np.array_equal(Md.apply(r), zh) and np.array_equal(Md.roots(), M.roots())
    zd = M.apply(torch.tensor(r, dtype=torch.float64, device="cuda"))
    assert np.array_equal(zd.cpu().numpy(), zh)
    M.close(); Md.close()
    Sc = system("cyclic")
    rc = np.random.default_rng(8).standard_normal(Sc.n)
    Ms, Mp = hip.Precond(gpu_ctx, dev("cyclic"), "gmres-poly5", 0), hip.PrecondGmresPoly(gpu_ctx, dev("cyclic"), 5)
    assert np.array_equal(Ms.apply(rc), Mp.apply(rc)) and np.array_equal(Ms.roots(), Mp.roots())
    assert np.array_equal(Ms.hessenberg(), Mp.hessenberg())
    Ms.close(); Mp.close()


# ---------------------------------------------------------------- 3. fused against unfused
@pytest.mark.parametrize("name", ["cyclic", "tgv2d12", "jitter8", "w32"])
def test_fused_sweep_has_the_bits_of_the_unfused_composition(gpu_ctx, dev, monkeypatch, name):
    S = system(name)
    r = np.random.default_rng(9).standard_normal(S.n)
    picks, _ = cyclic_degrees()
    degrees = sorted(set(picks.values()) | {2}) if name == "cyclic" else (2, 5, 8)
    for d in degrees:
        Mf = hip.PrecondGmresPoly(gpu_ctx, dev(name), d, nullvec=S.null)
        monkeypatch.setenv("ISPH_POLY_UNFUSED", "1")
        Mu = hip.PrecondGmresPoly(gpu_ctx, dev(name), d, nullvec=S.null)
        monkeypatch.delenv("ISPH_POLY_UNFUSED")
        zf, zu = np.array(Mf.apply(r)), np.array(Mu.apply(r))
        print("poly-fused %-8s degree %d %-8s max |fused - unfused| %.2e" % (name, d, pattern(Mf.roots()), np.max(np.abs(zf - zu))))
        assert np.array_equal(Mf.roots(), Mu.roots())
        assert np.array_equal(zf.view(np.uint64), zu.view(np.uint64))
        Mf.close(); Mu.close()


# ---------------------------------------------------------------- 4. independence of the numbering and of the rank count
@pytest.mark.parametrize("name,d", [("cyclic", 5), ("cyclic", 8), ("tgv2d12", 4), ("jitter8", 6)])
def test_the_librarys_row_numbering_gives_the_callers_polynomial(gpu_ctx, gpu_ctx_bricks, name, d):
    """the caller hands the rows over in a shuffled order; the library renumbers them by position, and the start vector
    still follows the caller's rows"""
    S = system(name)
    q = np.random.default_rng(17).permutation(S.n)
    As = S.A[q][:, q].tocsr()
    As.sort_indices()
    csr = (As.indptr.astype(np.int32), As.indices.astype(np.int32), As.data)
    Ab = hip.Matrix.from_host_csr_with_coords(gpu_ctx_bricks, *csr, np.ascontiguousarray(S.xyz[q]), dim=S.dim)
    Ac = hip.Matrix.from_csr(gpu_ctx, *csr)
    assert Ab.ordering() is not None and not np.array_equal(Ab.ordering()["perm"], np.arange(S.n))
    Mb = hip.PrecondGmresPoly(gpu_ctx_bricks, Ab, d, nullvec=S.null)
    Mc = hip.PrecondGmresPoly(gpu_ctx, Ac, d, nullvec=S.null)
    rb, rc, rr = Mb.roots(), Mc.roots(), gp.roots(As, d, S.null)
    sH, sR = gp.rounding_spread(As, d, S.null)
    scale = np.max(np.abs(rr))
    g, gr = float(np.max(np.abs(rb - rc)) / scale), float(np.max(np.abs(rb - rr)) / scale)
    gh = float(np.max(np.abs(Mb.hessenberg() - Mc.hessenberg())) / np.max(np.abs(Mc.hessenberg())))
    print("poly-bricks %-8s d %d roots gap %.2e (restatement %.2e) bound %.2e H gap %.2e bound %.2e" %
          (name, d, g, gr, bound_from(sR), gh, bound_from(sH)))
    assert g <= bound_from(sR) and gr <= bound_from(sR) and gh <= bound_from(sH)
    Mb.close(); Mc.close(); Ab.close(); Ac.close()


def _rank_solve(rank, G, dim, pgrid, n, degree):
    import oracle as orc
    import test_gpu_ranks as tr
    st = tr._rank_setup(rank, G, dim, pgrid, n, orc.NULLSPACE)
    ctx, A = st["ctx"], st["A"]
    try:
        nl = st["nl"]
        ntot = float(np.prod(pgrid[:dim])) * n ** dim
        M = hip.PrecondGmresPoly(ctx, A, degree, nullvec=np.full(nl, 1.0 / np.sqrt(ntot)))   # collective
        roots, H = M.roots(), M.hessenberg()
        r = np.cos(0.37 * st["rtag"].astype(np.float64))
        z = M.apply(r)
        x, bb = np.zeros(nl), st["b"].copy()
        info = hip.solve(ctx, A, bb, x, prec=M, singular=True)
        M.close()
        return dict(nl=nl, rtag=st["rtag"], col_tag=st["col_tag"], csr=st["csr"], b=st["b"], r=r, z=z, x=x, roots=roots, H=H,
                    info=(info.converged, info.iters))
    finally:
        A.close()
        ctx.close()


def test_two_ranks_build_the_polynomial_of_the_global_operator(gpu_ctx):
    from ranks import RankGroup
    from test_gpu_chebyshev import _global_system
    dim, pgrid, n, d = 3, (2, 1, 1), 8, 4
    G = RankGroup(2)
    try:
        res = G.run(_rank_solve, dim, pgrid, n, d)
    finally:
        G.close()
    Ag, bg = _global_system(res)
    N = Ag.shape[0]
    null = np.ones(N) / np.sqrt(N)
    assert np.array_equal(res[0]["roots"], res[1]["roots"]) and np.array_equal(res[0]["H"], res[1]["H"])
    A1 = hip.Matrix.from_csr(gpu_ctx, Ag.indptr.astype(np.int32), Ag.indices.astype(np.int32), Ag.data)
    M1 = hip.PrecondGmresPoly(gpu_ctx, A1, d, nullvec=null)
    sH, sR = gp.rounding_spread(Ag, d, null)
    r1, r2 = M1.roots(), res[0]["roots"]
    g = float(np.max(np.abs(r2 - r1)) / np.max(np.abs(r1)))
    gr = float(np.max(np.abs(r2 - gp.roots(Ag, d, null))) / np.max(np.abs(r1)))
    rr, z = np.concatenate([q["r"] for q in res]), np.concatenate([q["z"] for q in res])
    zr = gp.apply(Ag, r2, rr)
    gz, zmax = gp.rounding_gap(Ag, r2, rr)
    x1 = np.zeros(N)
    i1 = hip.solve(gpu_ctx, A1, bg.copy(), x1, prec=M1, singular=True)
    infos = {q["info"] for q in res}
    print("poly-ranks roots 2 ranks against one %.2e, against the restatement %.2e, bound %.2e; apply gap %.2e tolerance %.2e; "
          "iterations %s (one rank %d)" % (g, gr, bound_from(sR), np.max(np.abs(z - zr)), 8 * gz + 1e-13 * zmax, sorted(infos), i1.iters))
    assert g <= bound_from(sR) and gr <= bound_from(sR)
    assert np.max(np.abs(z - zr)) <= 8.0 * gz + 1e-13 * zmax
    assert infos == {(1, i1.iters)} and i1.converged == 1
    M1.close(); A1.close()


# ---------------------------------------------------------------- 5. solves
def solver_params(solver_type=0, flexible=1, m=50, k=20):
    return hip.SolverParams(solver_type=solver_type, flexible=flexible, num_blocks=m, max_iters=500, max_restarts=10 ** 6, tol=1e-8,
                            num_recycled=k)


@functools.lru_cache(maxsize=None)
def reference_run(name, d):
    S = system(name)
    minv = gp.minv(S.A, gp.roots(S.A, d, S.null))
    ref = kr.gmres_iterates(S.A, S.b, np.zeros(S.n), KS, 50, minv, S.null)
    return ref, cr.first_below(ref, 1e-8)


@pytest.mark.parametrize("flexible", [1, 0])
@pytest.mark.parametrize("name,d", [("cyclic", 5), ("tgv2d12", 4), ("jitter8", 4), ("jitter8", 8)])
def test_gmres_converges_on_the_restatements_count(gpu_ctx, dev, name, d, flexible):
    S = system(name)
    ref, kref = reference_run(name, d)
    assert kref is not None
    M = hip.PrecondGmresPoly(gpu_ctx, dev(name), d, nullvec=S.null)
    x = np.zeros(S.n)
    info = hip.solve(gpu_ctx, dev(name), S.b.copy(), x, prec=M, singular=S.singular, params=solver_params(0, flexible))
    M.close()
    gx = kr.iterate_gap(x, ref[info.iters].x) if info.iters in ref else np.inf
    kj = cr.first_below(kr.gmres_iterates(S.A, S.b, np.zeros(S.n), KS, 50, kr.jacobi_minv(S.A), S.null), 1e-8)
    print("poly-solve %-8s d %d flexible %d iterations %d restatement %d (jacobi %s) x gap %.2e" % (name, d, flexible, info.iters, kref, kj, gx))
    assert info.converged == 1 and abs(info.iters - kref) <= 1
    assert gx <= 1e-6


@pytest.mark.parametrize("name,d", [("tgv2d12", 4), ("jitter8", 4)])
def test_gcrodr_converges_with_it(gpu_ctx, dev, name, d):
    import gcrodr as gcro
    S = system(name)
    rp, ci, val = S.csr()
    M = hip.PrecondGmresPoly(gpu_ctx, dev(name), d, nullvec=S.null)
    minv = gp.minv(S.A, gp.roots(S.A, d, S.null))
    xo, io = gcro.solve(rp, ci, val, S.b, singular=True, prec=minv, num_blocks=20, num_recycled=5)
    x = np.zeros(S.n)
    info = hip.solve(gpu_ctx, dev(name), S.b.copy(), x, prec=M, singular=True, params=solver_params(2, 0, 20, 5))
    M.close()
    print("poly-gcrodr %-8s d %d iterations %d restatement %d x gap %.2e" % (name, d, info.iters, io["iters"], kr.iterate_gap(x, xo)))
    assert info.converged == 1 and io["converged"] and abs(info.iters - io["iters"]) <= 1
    assert kr.iterate_gap(x, xo) <= 1e-6


def test_cg_takes_it_on_a_symmetric_matrix(gpu_ctx):
    """a fixed linear operator: "Block CG" accepts it (a polynomial in D^-1 A times D^-1 is symmetric when A is)"""
    rp, ci, val, b, _ = cr.system("spd")
    n = len(rp) - 1
    A_h = sps.csr_matrix((val, ci, rp), shape=(n, n))
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondGmresPoly(gpu_ctx, A, 4)
    ref = kr.pcg_iterates(A_h, b, np.zeros(n), KS, gp.minv(A_h, gp.roots(A_h, 4)))
    kref = cr.first_below(ref, 1e-8)
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, params=solver_params(1))
    print("poly-cg spd iterations %d restatement %s" % (info.iters, kref))
    assert kref is not None and info.converged == 1 and abs(info.iters - kref) <= 1
    assert kr.iterate_gap(x, ref[info.iters].x) <= 1e-6
    M.close(); A.close()


def test_three_right_hand_sides_in_lockstep_are_three_single_solves(gpu_ctx):
    """a Helmholtz system (I - c L of the 2-D lattice: what the velocity solve of a time step hands over, three columns)"""
    rp, ci, val, _, _ = cr.system("spd")
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondGmresPoly(gpu_ctx, A, 4)
    assert M.multi_path(3) == 0                                  # one vector after the other
    B = np.random.default_rng(11).standard_normal((3, n))
    prm = hip.SolverParams(num_blocks=30, max_iters=500, max_restarts=10 ** 6, tol=1e-9)
    xflat = np.zeros(3 * n)
    info = hip.solve(gpu_ctx, A, B.ravel().copy(), xflat, prec=M, nvec=3, lda=n, params=prm)
    its = []
    for c in range(3):
        x = np.zeros(n)
        single = hip.solve(gpu_ctx, A, B[c].copy(), x, prec=M, params=prm)
        assert single.converged == 1
        assert np.array_equal(x.view(np.uint64), xflat[c * n:(c + 1) * n].view(np.uint64)), c
        its.append(single.iters)
    assert info.converged == 1 and info.iters == sum(its)
    # isph_prec_apply_multi: K applications, one after the other
    Z = M.apply_multi(B)
    for c in range(3):
        assert np.array_equal(np.asarray(Z[c]).view(np.uint64), np.array(M.apply(B[c])).view(np.uint64))
    M.close(); A.close()


# ---------------------------------------------------------------- 6. refusals, refactor
class held:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.hold_pattern(True)

    def __exit__(self, *exc):
        self.ctx.hold_pattern(False)


def test_refusals_by_text(gpu_ctx, dev):
    A = dev("cyclic")
    for d in (0, 26, -1):
        with pytest.raises(hip.IsphError, match=r"GMRES polynomial: degree must be in \[1,25\]"):
            hip.PrecondGmresPoly(gpu_ctx, A, d)
    for kind in ("gmres-poly0", "gmres-poly26", "gmres-poly4-f32", "gmres-poly"):      # no value_bits = 32 form
        with pytest.raises(hip.IsphError, match=r"unknown preconditioner type \(none\|jacobi\|.*gmres-poly<d>, d = 1\.\.25"):
            hip.Precond(gpu_ctx, A, kind, 0)
    # a singular matrix without its null vector: six steps on the 6-point Neumann Laplacian span the zero eigenvalue
    n = 6
    L = sps.diags([np.full(n - 1, -1.0), np.r_[1.0, np.full(n - 2, 2.0), 1.0], np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    AL = hip.Matrix.from_csr(gpu_ctx, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data)
    with pytest.raises(hip.IsphError, match="near-zero root: a singular matrix needs the null vector"):
        hip.PrecondGmresPoly(gpu_ctx, AL, 6)
    with pytest.raises(gp.NearZeroRoot):
        gp.roots(L, 6)
    Mn = hip.PrecondGmresPoly(gpu_ctx, AL, 5, nullvec=np.ones(n))                      # with it: the five other eigenvalues
    ev = np.sort(np.linalg.eigvals((sps.diags(gp.dinv_of(L)) @ L).toarray()).real)[1:]
    assert np.allclose(np.sort(Mn.roots().real), ev, atol=1e-12)
    Mn.close(); AL.close()
    # a diagonal matrix: D^-1 A = I, an invariant subspace after one step -- degree 1 whatever was asked for
    dg = 1.0 + np.arange(130) % 7
    AD = hip.Matrix.from_csr(gpu_ctx, np.arange(131, dtype=np.int32), np.arange(130, dtype=np.int32), dg)
    MD = hip.PrecondGmresPoly(gpu_ctx, AD, 5)
    assert np.allclose(MD.roots(), [1.0], atol=1e-15) and MD.hessenberg().shape == (2, 1)
    r = np.random.default_rng(3).standard_normal(130)
    assert np.allclose(MD.apply(r), r / dg, rtol=1e-15, atol=0)
    MD.close(); AD.close()
    # another kind has no polynomial to report; a zero diagonal entry
    J = hip.Precond(gpu_ctx, A, "jacobi", 0)
    with pytest.raises(hip.IsphError, match="not a GMRES polynomial"):
        J.roots()
    J.close()
    rp, ci, val = system("cyclic").csr()
    v0 = val.copy()
    v0[rp[77] + int(np.flatnonzero(ci[rp[77]:rp[78]] == 77)[0])] = 0.0
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v0)
    with pytest.raises(hip.IsphError, match="zero diagonal"):
        hip.PrecondGmresPoly(gpu_ctx, Az, 3)
    Az.close()


@pytest.mark.parametrize("name,d", [("cyclic", 5), ("jitter8", 4)])
def test_refactor_is_a_fresh_create_and_needs_the_held_pattern(gpu_ctx, name, d):
    S = system(name)
    rp, ci, val = S.csr()
    col = 1.0 + 0.3 * np.cos(np.arange(S.n))
    val2 = val * col[ci] if not S.singular else val * np.repeat(col, np.diff(rp))   # (rows rescaled: A 1 = 0 stays)
    r = np.random.default_rng(9).standard_normal(S.n)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondGmresPoly(gpu_ctx, A, d, nullvec=S.null)
        P = hip.Precond(gpu_ctx, A, "gmres-poly3", 0)
    z_old = np.array(M.apply(r))
    A.update_values(val2)
    M.refactor(A)
    P.refactor(A)
    A2 = hip.Matrix.from_csr(gpu_ctx, rp, ci, val2)
    F = hip.PrecondGmresPoly(gpu_ctx, A2, d, nullvec=S.null)
    Fp = hip.Precond(gpu_ctx, A2, "gmres-poly3", 0)
    z, zf = np.array(M.apply(r)), np.array(F.apply(r))
    assert np.array_equal(z.view(np.uint64), zf.view(np.uint64)) and not np.array_equal(z, z_old)
    assert np.array_equal(M.roots(), F.roots()) and np.array_equal(M.hessenberg(), F.hessenberg())
    assert np.array_equal(np.array(P.apply(r)).view(np.uint64), np.array(Fp.apply(r)).view(np.uint64))
    M.refactor(A)                                                          # a refreshed polynomial can be refreshed again
    assert np.array_equal(np.array(M.apply(r)).view(np.uint64), zf.view(np.uint64))
    with pytest.raises(hip.IsphError, match="gmres-poly<d>.*created while the pattern was not held"):
        F.refactor(A2)                                                     # created with the mode off: refused, and untouched
    assert np.array_equal(np.array(F.apply(r)).view(np.uint64), zf.view(np.uint64))
    with pytest.raises(hip.IsphError, match="rows"):
        M.refactor(hipmat_other(gpu_ctx))
    for o in (M, P, F, Fp, A, A2):
        o.close()


def hipmat_other(ctx):
    n = 70
    return hip.Matrix.from_csr(ctx, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


# ---------------------------------------------------------------- 8. pool hygiene
def test_close_gives_every_buffer_back(gpu_ctx, dev):
    S = system("jitter8")
    A = dev("jitter8")
    r = np.random.default_rng(4).standard_normal(S.n)
    warm = hip.PrecondGmresPoly(gpu_ctx, A, 4, nullvec=S.null)              # (the context's own scalars and staging vectors)
    warm.apply(r)
    warm.close()
    gpu_ctx.sync()
    before = hip.pool_info()["live"]
    M = hip.PrecondGmresPoly(gpu_ctx, A, 8, nullvec=S.null)
    during = hip.pool_info()["live"]
    M.apply(r)
    M.apply_multi(np.stack([r, 2 * r]))
    M.close()
    gpu_ctx.sync()
    after = hip.pool_info()["live"]
    print("poly-pool live bytes before %d with the polynomial %d after close %d" % (before, during, after))
    assert during > before and after <= before
