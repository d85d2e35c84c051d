"""-m gpu: isph_amg_params::cycle_bits = 32 -- the whole V cycle of the Chebyshev-smoothed SA-AMG in single-precision
storage (operators, level vectors and gathers float; all arithmetic fp64, one rounding per stored element).

What is expected is the restatement tests/amg_cycle_f32_reference.py (include/isph_hip.h states the same arithmetic).
Its own noise is nil (tests/test_amg_cycle_f32_reference.py: the spread under three summation orders is exactly 0), so
what the device can add is a float rounding that its summation order flips on isolated elements; and it rounds the A P
plane from the set-up's product, which agrees with scipy's to fp64 round-off.  Each flip is 2^-24 of one of n elements,
and sep = ||z_ref32 - z_ref64|| / ||z_ref64|| is what all roundings of a cycle add up to, so the gate
    g = ||z_dev - z_ref32|| / ||z_ref32|| <= 0.1 sep
leaves room for about 1 % of the elements to flip.  And ||z_dev - z_ref64|| / ||z_ref64|| >= 0.5 sep: a silent fall-back to
doubles fails.  sep is computed in the same test; every g and sep is printed before it is asserted.

eig_type = 1: the fp64 reference takes lambda of every level from isph_prec_eig_estimate (the estimate of A_l).  The
rounded cycle's interval is defined on fl32(A_l) -- the smoother's second estimate, which isph_prec_eig_estimate does not
report -- so the rounded reference takes it from the host restatement of that estimate (eig_estimate_reference.estimate on
fl32(A_l); tests/test_gpu_eig_estimate.py pins the device's estimate to it).

Solves: converged, explicit residual <= 1e-7, iterations within one of the cycle_bits = 64 solve of the same test (the
project's parity gate), x within 1e-6 of its x.
"""
import functools
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import build, hip
import amg_cycle_f32_reference as a32
import chebyshev_reference as cr
import eig_estimate_reference as er
import krylov_reference as kr

pytestmark = pytest.mark.gpu

AMG_KW = dict(theta=0.0, block=256, coarse_max=64)
FIXTURES = ["stencil", "wall42", "tgv16", "spd"]
RATIO = 20.0


@functools.lru_cache(maxsize=None)
def system(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    return rp, ci, val, b, singular, sps.csr_matrix((val, ci, rp), shape=(n, n))


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            rp, ci, val = system(name)[:3]
            cache[name] = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        return cache[name]
    yield get
    for A in cache.values():
        A.close()


def rhs(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


def nullvec(name):
    n = system(name)[5].shape[0]
    return np.ones(n) / np.sqrt(n) if system(name)[4] else None


def amg(ctx, A, name, bits, sweeps=2, **kw):
    prm = hip.AmgParams(smoother=2, sweeps=sweeps, cycle_bits=bits, **dict(AMG_KW, **kw))
    return hip.PrecondAMG(ctx, A, nullvec=nullvec(name), params=prm)


# ---------------------------------------------------------------- 1. one application against the restatement
@pytest.mark.parametrize("eig_type", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_one_application_is_the_restated_rounded_cycle(gpu_ctx, dev, name, eig_type):
    """stencil: 210 rows, three slices plus a tail of 18, n no multiple of 4 (the 16-byte path of the streaming kernels has
    a remainder); wall42: a tail slice, dense coarsest solve; tgv16: four 16-bit column windows, singular -- 4096 rows
    coarsen to 15 in one step, and the coarsest level is the float polynomial on 32-bit columns; spd: three levels (1480,
    222, 16 rows), so a float level lies between two others and its sweeps read 32-bit columns."""
    singular, A_h = system(name)[4:6]
    n = A_h.shape[0]
    r = rhs(n, 10)
    for sweeps in (1, 2, 3):
        M = amg(gpu_ctx, dev(name), name, 32, sweeps, eig_type=eig_type)
        assert M.cycle_bits == 32 and M.value_bits == 32 and M.levels >= (3 if name == "spd" else 2)
        levels = cr.levels_from(M, n)
        lam64 = lam32 = None
        if eig_type == 1:
            lam64 = [M.eig_estimate(l)["lambda_used"] for l in range(M.levels)]
            lam32 = [er.estimate(er.fl32(A_l), 10, level=l)["lambda_used"] for l, (A_l, _) in enumerate(levels)]
        z = M.apply(r)
        M.close()
        z32 = a32.cycle(levels, r, sweeps, RATIO, lams=lam32, coarse_polynomial=singular, rounded=True)
        z64 = a32.cycle(levels, r, sweeps, RATIO, lams=lam64, coarse_polynomial=singular, rounded=False)
        sep, g, g64 = rel(z32, z64), rel(z, z32), rel(z, z64)
        print("amg-cycle-f32 apply %-8s eig_type %d sweeps %d rows %s g %.2e sep %.2e (g / sep %.3f) to the fp64 cycle %.2e" %
              (name, eig_type, sweeps, [A_l.shape[0] for A_l, _ in levels], g, sep, g / sep, g64))
        assert g <= 0.1 * sep, (name, eig_type, sweeps, g, sep)
        assert g64 >= 0.5 * sep, (name, eig_type, sweeps, g64, sep)


# ---------------------------------------------------------------- 2. fused against ISPH_CHEB_UNFUSED=1
@pytest.mark.parametrize("name", FIXTURES)
def test_fused_cycle_against_the_unfused_composition(gpu_ctx, dev, monkeypatch, name):
    singular, A_h = system(name)[4:6]
    n = A_h.shape[0]
    r = rhs(n, 9)
    for sweeps in (1, 2, 3):
        Mf = amg(gpu_ctx, dev(name), name, 32, sweeps)
        monkeypatch.setenv("ISPH_CHEB_UNFUSED", "1")
        Mu = amg(gpu_ctx, dev(name), name, 32, sweeps)
        monkeypatch.delenv("ISPH_CHEB_UNFUSED")
        levels = cr.levels_from(Mf, n)
        zf, zu = Mf.apply(r), Mu.apply(r)
        Mf.close(); Mu.close()
        sep = rel(a32.cycle(levels, r, sweeps, RATIO, coarse_polynomial=singular),
                  a32.cycle(levels, r, sweeps, RATIO, coarse_polynomial=singular, rounded=False))
        g = rel(zf, zu)
        print("amg-cycle-f32 fused %-8s sweeps %d gap %.2e sep %.2e" % (name, sweeps, g, sep))
        assert g <= 0.1 * sep


# ---------------------------------------------------------------- 3. the hierarchy is untouched
def assert_same_hierarchy(M, M0):
    """patterns, values (bit for bit), sizes and aggregates"""
    assert M.levels == M0.levels >= 2
    for l in range(M.levels):
        assert M.level_info(l) == M0.level_info(l)
        for what in ("A", "P") if l < M.levels - 1 else ("A",):
            (rp, ci, v), (rp0, ci0, v0) = M.export(l, what), M0.export(l, what)
            assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0), (l, what)
            assert np.array_equal(v, v0), (l, what, float(np.max(np.abs(v - v0))))
        if l < M.levels - 1:
            assert np.array_equal(M.aggregates(l), M0.aggregates(l))


@pytest.mark.parametrize("eig_type", [0, 1])
@pytest.mark.parametrize("name", ["tgv16", "wall42"])
def test_hierarchy_is_the_fp64_one_and_the_default_is_untouched(gpu_ctx, dev, name, eig_type):
    n = system(name)[5].shape[0]
    r = rhs(n, 12)
    M32, M64, M0 = (amg(gpu_ctx, dev(name), name, bits, 2, eig_type=eig_type) for bits in (32, 64, 0))
    Mdef = hip.PrecondAMG(gpu_ctx, dev(name), nullvec=nullvec(name),
                          params=hip.AmgParams(smoother=2, sweeps=2, eig_type=eig_type, **AMG_KW))
    assert hip.AmgParams().cycle_bits == 64
    assert (M32.cycle_bits, M32.value_bits) == (32, 32)
    assert (M64.cycle_bits, M64.value_bits) == (64, 64) and (M0.cycle_bits, M0.value_bits) == (64, 64)
    assert_same_hierarchy(M32, M64)
    if eig_type == 1:
        for l in range(M32.levels):
            assert M32.eig_estimate(l) == M64.eig_estimate(l)
    z64, z0, zdef, z32 = M64.apply(r), M0.apply(r), Mdef.apply(r), M32.apply(r)
    assert np.array_equal(z64, z0) and np.array_equal(z64, zdef)
    assert not np.array_equal(z32, z64)
    # cheb_value_bits is not read by the float cycle
    Mb = hip.PrecondAMG(gpu_ctx, dev(name), nullvec=nullvec(name),
                        params=hip.AmgParams(smoother=2, sweeps=2, eig_type=eig_type, cycle_bits=32, cheb_value_bits=64, **AMG_KW))
    assert np.array_equal(Mb.apply(r), z32)
    # every other preconditioner answers 64
    Mj = hip.Precond(gpu_ctx, dev(name), "jacobi", 0)
    Mg = hip.PrecondAMG(gpu_ctx, dev(name), nullvec=nullvec(name), params=hip.AmgParams(smoother=0, **AMG_KW))
    assert Mj.cycle_bits == 64 and Mg.cycle_bits == 64
    for M in (M32, M64, M0, Mdef, Mb, Mj, Mg):
        M.close()


# ---------------------------------------------------------------- 4. the library's numbering
@pytest.mark.parametrize("name", ["stencil", "spd"])
def test_the_librarys_row_numbering_converges_like_the_callers(gpu_ctx, gpu_ctx_bricks, dev, name):
    """the aggregates differ between the numberings, so the two are not compared value by value"""
    rp, ci, val, b, _, A_h = system(name)
    xyz, dim = cr.coordinates(name)
    Ab = hip.Matrix.from_host_csr_with_coords(gpu_ctx_bricks, rp, ci, val, xyz, dim=dim)
    assert Ab.ordering() is not None
    out = {}
    for key, ctx, A in (("bricks", gpu_ctx_bricks, Ab), ("caller", gpu_ctx, dev(name))):
        M = amg(ctx, A, name, 32, 2)
        assert M.cycle_bits == 32
        x = np.zeros(A_h.shape[0])
        info = hip.solve(ctx, A, b.copy(), x, prec=M, params=solver_params())
        out[key] = (info.converged, info.iters, rel(A_h @ x, b))
        M.close()
    Ab.close()
    print("amg-cycle-f32 numbering %-8s bricks %s caller %s" % (name, out["bricks"], out["caller"]))
    for key in out:
        assert out[key][0] == 1 and out[key][2] <= 1e-7
    assert abs(out["bricks"][1] - out["caller"][1]) <= 1


# ---------------------------------------------------------------- 5. solves
def solver_params(solver_type=0, flexible=1, basis_bits=0):
    return hip.SolverParams(solver_type=solver_type, flexible=flexible, num_blocks=50, max_iters=500, max_restarts=10 ** 6, tol=1e-8,
                            basis_bits=basis_bits)


def explicit_residual(name, x, b):
    singular, A_h = system(name)[4:6]
    # a singular system: the residual of the system that is solved, P (b - A x) with P = I - n n^T
    proj = (lambda v: v - v.mean()) if singular else (lambda v: v)
    return float(np.linalg.norm(proj(b - A_h @ x)) / np.linalg.norm(proj(b)))


@pytest.mark.parametrize("basis_bits", [0, 32])
@pytest.mark.parametrize("name", FIXTURES)
def test_solves_keep_the_iteration_count_of_the_double_cycle(gpu_ctx, dev, name, basis_bits):
    b, singular, A_h = system(name)[3:6]
    n = A_h.shape[0]
    A = dev(name)
    out = {}
    for bits in (64, 32):
        M = amg(gpu_ctx, A, name, bits, 2)
        x = np.zeros(n)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=solver_params(basis_bits=basis_bits))
        out[bits] = (x, info)
        M.close()
    (x64, i64), (x32, i32) = out[64], out[32]
    gx, e32, e64 = kr.iterate_gap(x32, x64), explicit_residual(name, x32, b), explicit_residual(name, x64, b)
    print("amg-cycle-f32 solve %-8s basis_bits %d iterations %d (64 bits: %d) explicit residual %.2e (64 bits: %.2e) x against the "
          "64-bit x %.2e" % (name, basis_bits, i32.iters, i64.iters, e32, e64, gx))
    assert i64.converged == 1 and i32.converged == 1
    assert e32 <= 1e-7
    assert abs(i32.iters - i64.iters) <= 1, (i32.iters, i64.iters)
    assert gx <= 1e-6


@pytest.mark.parametrize("basis_bits", [0, 32])
def test_three_columns_in_lockstep(gpu_ctx, dev, basis_bits):
    name = "tgv16"
    A_h = system(name)[5]
    n = A_h.shape[0]
    A = dev(name)
    B = np.random.default_rng(11).standard_normal((3, n))
    out = {}
    for bits in (64, 32):
        M = amg(gpu_ctx, A, name, bits, 2)
        xflat = np.zeros(3 * n)
        info = hip.solve(gpu_ctx, A, B.ravel().copy(), xflat, prec=M, singular=True, nvec=3, lda=n, params=solver_params(basis_bits=basis_bits))
        out[bits] = (xflat.reshape(3, n), info)
        M.close()
    (x64, i64), (x32, i32) = out[64], out[32]
    assert i64.converged == 1 and i32.converged == 1
    assert abs(i32.iters - i64.iters) <= 1, (i32.iters, i64.iters)
    for c in range(3):
        e, gx = explicit_residual(name, x32[c], B[c]), kr.iterate_gap(x32[c], x64[c])
        print("amg-cycle-f32 lockstep basis_bits %d column %d iterations %d (64 bits: %d) explicit residual %.2e x gap %.2e" %
              (basis_bits, c, i32.iters, i64.iters, e, gx))
        assert e <= 1e-7 and gx <= 1e-6


# ---------------------------------------------------------------- 6. refusals
def _entry(rp, ci, i, j):
    return rp[i] + int(np.flatnonzero(ci[rp[i]:rp[i + 1]] == j)[0])


def test_refusals(gpu_ctx, dev):
    A = dev("wall42")
    rp, ci, val, b = system("wall42")[:4]
    n = len(rp) - 1
    for bits in (16, 33, -1):
        with pytest.raises(hip.IsphError, match="cycle_bits"):
            hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=2, cycle_bits=bits, **AMG_KW))
        with pytest.raises(hip.IsphError, match="cycle_bits"):
            hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=0, cycle_bits=bits, **AMG_KW))
    for smoother in (0, 1):
        with pytest.raises(hip.IsphError, match="cycle_bits"):
            hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=smoother, cycle_bits=32, **AMG_KW))
    M = hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=2, sweeps=2, cycle_bits=32, **AMG_KW))
    M64 = hip.PrecondAMG(gpu_ctx, A, params=hip.AmgParams(smoother=2, sweeps=2, cycle_bits=64, **AMG_KW))
    for st, fl in ((1, 1), (2, 1), (0, 0)):
        x = np.zeros(n)
        with pytest.raises(hip.IsphError, match="cycle_bits"):
            hip.solve(gpu_ctx, A, b.copy(), x, prec=M, params=solver_params(st, fl))
        with pytest.raises(hip.IsphError, match="cycle_bits"):
            hip.solve_block(gpu_ctx, [[A]], b.copy(), x, prec=M, params=solver_params(st, fl))
        assert not x.any()
    # the fp64 cycle keeps every driver
    x = np.zeros(n)
    assert hip.solve(gpu_ctx, A, b.copy(), x, prec=M64, params=solver_params(0, 0)).converged == 1
    x = np.zeros(n)
    assert hip.solve_block(gpu_ctx, [[A]], b.copy(), x, prec=M, params=solver_params(0, 1)).converged == 1
    M.close(); M64.close()
    i = 77
    j = int(ci[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] != i][0])
    # beyond FLT_MAX (finite in fp64): refused by the 32-bit form only
    v = val.copy(); v[_entry(rp, ci, i, j)] = 1e39
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    with pytest.raises(hip.IsphError, match="single precision"):
        hip.PrecondAMG(gpu_ctx, Az, params=hip.AmgParams(smoother=2, cycle_bits=32, **AMG_KW))
    Az.close()
    # a diagonal entry that rounds to 0
    v = val.copy(); v[_entry(rp, ci, i, i)] = 1e-50
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    with pytest.raises(hip.IsphError, match="zero diagonal"):
        hip.PrecondAMG(gpu_ctx, Az, params=hip.AmgParams(smoother=2, cycle_bits=32, **AMG_KW))
    Az.close()


# ---------------------------------------------------------------- 7. two thread ranks on one GPU
def _rank_solve(rank, G, dim, pgrid, n, mode):
    import oracle as orc
    import test_gpu_ranks as tr
    st = tr._rank_setup(rank, G, dim, pgrid, n, mode)
    ctx, A = st["ctx"], st["A"]
    try:
        nl = st["nl"]
        ntot = float(np.prod(pgrid[:dim])) * n ** dim
        singular = mode == orc.NULLSPACE
        out = dict(nl=nl, rtag=st["rtag"], col_tag=st["col_tag"], csr=st["csr"], b=st["b"])
        for bits in (64, 32):                                     # (collective: every rank walks the same sequence)
            M = hip.PrecondAMG(ctx, A, nullvec=np.full(nl, 1.0 / np.sqrt(ntot)) if singular else None,
                               params=hip.AmgParams(smoother=2, sweeps=2, theta=0.02, block=256, coarse_max=64, cycle_bits=bits))
            cb, lev = M.cycle_bits, M.levels
            x, bb = np.zeros(nl), st["b"].copy()
            info = hip.solve(ctx, A, bb, x, prec=M, singular=singular)
            M.close()
            out[bits] = dict(x=x, cycle_bits=cb, levels=lev, info=(info.converged, info.iters, info.rel_res_explicit))
        return out
    finally:
        A.close()
        ctx.close()


@pytest.mark.parametrize("mode", ["nullspace", "doublediag"])
def test_two_ranks_on_one_gpu(gpu_ctx, mode):
    """the GHOST / LIST sweeps and the widened halo pack; the coarsest level across ranks is the float polynomial (nullspace:
    a null vector) or the dense inverse of all ranks' rows behind the widened, all-reduced right-hand side (doublediag: the
    regular system)"""
    import oracle as orc
    from ranks import RankGroup
    import test_gpu_chebyshev as tc
    dim, pgrid, n = 3, (2, 1, 1), 8
    singular = mode == "nullspace"
    G = RankGroup(2)
    try:
        res = G.run(_rank_solve, dim, pgrid, n, orc.NULLSPACE if singular else orc.DOUBLEDIAG)
    finally:
        G.close()
    Ag, bg = tc._global_system(res)
    info = {}
    for bits in (64, 32):
        assert all(r[bits]["cycle_bits"] == bits for r in res)
        got = {r[bits]["info"][:2] for r in res}
        assert len(got) == 1, got
        info[bits] = got.pop()
        assert info[bits][0] == 1
    x = np.concatenate([r[32]["x"] for r in res])
    proj = (lambda v: v - v.mean()) if singular else (lambda v: v)
    eres = float(np.linalg.norm(proj(bg - Ag @ x)) / np.linalg.norm(proj(bg)))
    print("amg-cycle-f32 ranks %-10s levels %s iterations %d (two ranks, 64 bits: %d) explicit residual %.2e" %
          (mode, [r[32]["levels"] for r in res], info[32][1], info[64][1], eres))
    assert eres <= 1e-7
    assert abs(info[32][1] - info[64][1]) <= 1


# ---------------------------------------------------------------- 8. the C++ wrapper
def run_cpp(tmp_path, name, bits):
    rp, ci, val, b, singular = system(name)[:5]
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / "x.bin")
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_amg_cycle_f32_test(), fin, fout, "1" if singular else "0", str(bits)],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


@pytest.mark.parametrize("name", ["tgv16", "wall42"])
def test_wrapper_matches_the_python_path(gpu_ctx, tmp_path, name):
    r, xc = run_cpp(tmp_path, name, 32)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rp, ci, val, b, singular = system(name)[:5]
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondAMG(gpu_ctx, A, nullvec=nullvec(name),
                       params=hip.AmgParams(coarse_max=64, block=256, smoother=2, sweeps=2, cheb_ratio=20.0, cycle_bits=32))
    assert M.cycle_bits == 32
    x = np.zeros(n)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=hip.SolverParams())
    M.close(); A.close()
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    conv, iters = (int(t.split("=")[1]) for t in line.split()[:2])
    g = np.linalg.norm(xc - x) / np.linalg.norm(x)
    print("amg-cycle-f32 wrapper %-8s iterations %d (python %d) x gap %.2e" % (name, iters, info.iters, g))
    assert conv == 1 and info.converged == 1
    assert g <= 1e-6


def test_wrapper_refuses_other_widths_and_names_the_key(tmp_path):
    r, _ = run_cpp(tmp_path, "stencil", 16)
    assert r.returncode == 1
    assert "isph: amg cycle bits" in r.stderr and "not available" in r.stderr, r.stderr
