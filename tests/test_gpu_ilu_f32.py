"""-m gpu: value_bits = 32 of the block ILU -- "bjacobi-ilu<k>-f32", isph_prec_create_ilu (isph_ilu_params::value_bits) and
the key "isph: ilu value bits" of PrecondWrapper_Ifpack.

What is expected (include/isph_hip.h): the factorisation is untouched -- the exported factor carries the bits of the
64-bit build -- and the application is exactly the fp64 triangular solves with the strict-L and strict-U entries replaced
by their float roundings (tests/ilu_f32_reference.py, fed the device's own exported factor).  Only the values the solves
stream are single precision; the pivots, the vectors, the accumulators, the scan and the update are double, so the device
has to reach the SAME bound against the rounded restatement as the fp64 mode reaches against the unrounded one:
  one application   <= 1e-11 ||z||   (test_gpu_ilu_shapes.check; a pivot rounded to float would miss it by three orders)
and it has to be on the rounded side: one application differs from the long-double application of the unrounded factor by
>= 1e-10 (the two differ by 3.3e-9 .. 9.5e-9 on these fixtures, tests/test_ilu_f32_reference.py), so a silent fall-back
to the doubles fails.  Solves: converged with an explicit residual <= 1e-7, iteration counts within one of the 64-bit
solve of the same test (the project's parity gate), x within 1e-6 of its x.  Every gap is printed before it is asserted.
"""
import functools
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from isph_amd import build, hip, workload
import chebyshev_reference as cr
import ilu_f32_reference as i32
import ilu_shapes as sh
import krylov_reference as kr
from test_gpu_ilu_shapes import rhs, uniform_block

pytestmark = pytest.mark.gpu

APPLY_TOL = 1e-11          # against the restatement on the rounded device factor
NOT_FP64 = 1e-10           # against the long-double application of the unrounded factor
CASES = [(name, 0) for name in sh.ILU0_FIXTURES] + [(name, K) for name in sh.ILUK_FIXTURES for K in (1, 2, 3)]
rel = i32.rel


def forms32(bp, K):
    """(label, constructor) of every way to ask for the 32-bit block ILU(K) on the decomposition bp: the caller's table and,
    where the table is uniform, the block size -- each through the "-f32" string and through isph_prec_create_ilu"""
    kind = "bjacobi-ilu%d-f32" % K
    out = [("table string", lambda ctx, A: hip.Precond(ctx, A, kind, block_ptr=bp)),
           ("table struct", lambda ctx, A: hip.PrecondILU(ctx, A, level_of_fill=K, block_ptr=bp, value_bits=32))]
    B = uniform_block(bp)
    if B is not None:
        out += [("uniform %d string" % B, lambda ctx, A: hip.Precond(ctx, A, kind, B)),
                ("uniform %d struct" % B, lambda ctx, A: hip.PrecondILU(ctx, A, level_of_fill=K, block_size=B, value_bits=32))]
    return out


def same_factor(f, g):
    return all(np.array_equal(a, b) for a, b in zip(f, g))


# ---------------------------------------------------------------- 1. one application against the restatement
@pytest.mark.parametrize("name,K", CASES)
def test_apply_is_the_solve_with_the_rounded_factor(gpu_ctx, name, K):
    """blocks of 1, 63, 64, 65 and 1024 rows, a block whose stream is empty, rows across the 64/65 and 128/129 boundaries,
    the CONT carries (the fixtures of tests/ilu_shapes.py)"""
    rp, ci, val, bp = sh.fixture(name)
    n = len(rp) - 1
    r = rhs(n)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M64 = hip.Precond(gpu_ctx, A, "bjacobi-ilu%d" % K, block_ptr=bp)
    f64 = M64.export_ilu()
    z64 = M64.apply(r)
    M64.close()
    z_rounded = i32.apply(f64[0], f64[1], f64[2], bp, r)        # the device's own factor, rounded on the host: once
    z_doubles = sh.ref_apply_of(name, K, r)                     # long-double application of the unrounded reference factor
    forms = forms32(bp, K)
    assert len(forms) == (2 if name == "ragged" else 4)
    for label, make in forms:
        M = make(gpu_ctx, A)
        bits, f32, z = M.value_bits, M.export_ilu(), M.apply(r)
        g32, g64 = rel(z, z_rounded), rel(z, z_doubles)
        print("\nilu-f32-apply %-8s K=%d %-18s gap to the rounded factor %.2e, to the doubles %.2e (64-bit build to the doubles %.2e)" %
              (name, K, label, g32, g64, rel(z64, z_doubles)))
        assert bits == 32, label
        assert M.info()["nblocks"] == len(bp) - 1
        assert same_factor(f32, f64), label                     # the factorisation is untouched: bit for bit
        assert g32 <= APPLY_TOL, (name, K, label, g32)
        assert g64 >= NOT_FP64, (name, K, label, g64)
        M.close()
    A.close()


# ---------------------------------------------------------------- 2. the 64-bit forms are untouched
@pytest.mark.parametrize("name,K", [("narrow", 0), ("ragged", 0), ("fill256", 2)])
def test_the_struct_with_64_bits_is_the_string_form(gpu_ctx, name, K):
    rp, ci, val, bp = sh.fixture(name)
    r = rhs(len(rp) - 1)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    B = uniform_block(bp)
    pairs = [(dict(block_ptr=bp), dict(block_ptr=bp))] + ([(dict(block_size=B), dict(block_size=B))] if B is not None else [])
    for kw_string, kw_struct in pairs:
        M0 = hip.Precond(gpu_ctx, A, "bjacobi-ilu%d" % K, **kw_string)
        f0, z0 = M0.export_ilu(), M0.apply(r)
        assert M0.value_bits == 0                               # a plain block ILU still answers 0
        for bits in (0, 64):
            M = hip.PrecondILU(gpu_ctx, A, level_of_fill=K, value_bits=bits, **kw_struct)
            assert M.value_bits == 0 and M.info() == M0.info()
            assert same_factor(M.export_ilu(), f0) and np.array_equal(M.apply(r), z0), (name, bits)
            M.close()
        M0.close()
    A.close()


# ---------------------------------------------------------------- 3. stream sized by the counting pass
def test_exact_stream_gives_the_same_bits(gpu_ctx):
    """isph_set_exact_stream_threshold(0): capacity factor 1, no slack, offsets from the counting pass -- the rounding pass
    and the float solve address the stream through the same offsets"""
    rp, ci, val, bp = sh.fixture("narrow")
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    r = rhs(len(rp) - 1)
    for label, make in forms32(bp, 0):
        M0 = make(gpu_ctx, A)
        f0, z0, i0 = M0.export_ilu(), M0.apply(r), M0.info()
        try:
            hip.set_exact_stream_threshold(0)
            M1 = make(gpu_ctx, A)
        finally:
            hip.set_exact_stream_threshold(-1)
        f1, z1, i1 = M1.export_ilu(), M1.apply(r), M1.info()
        assert M0.value_bits == 32 and M1.value_bits == 32
        assert i1["stream_chunks"] == i0["stream_chunks"] and i1["stream_capacity"] < i0["stream_capacity"], label
        assert same_factor(f0, f1), label
        assert np.array_equal(z0, z1), label
        g = rel(z1, i32.apply(f1[0], f1[1], f1[2], bp, r))
        print("\nilu-f32-exact-stream %-18s gap to the rounded factor %.2e" % (label, g))
        assert g <= APPLY_TOL
        M0.close(); M1.close()
    A.close()


# ---------------------------------------------------------------- 4. several right-hand sides in one sweep
@pytest.mark.parametrize("flexible", [0, 1])
@pytest.mark.parametrize("nvec", [2, 3, 4])
@pytest.mark.parametrize("name", ["narrow", "fan"])
def test_multi_vector_sweep_carries_the_bits_of_single_applications(gpu_ctx, name, nvec, flexible):
    """test_gpu_ilu_shapes' test of k_ilu_solve_stream_multi with the float instantiations: nvec columns advancing together
    through 7 iterations of GMRES(5) equal, bit for bit, their own single-vector solves"""
    rp, ci, val, bp = sh.fixture(name)
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0-f32", block_ptr=bp)
    assert M.value_bits == 32
    rng = np.random.default_rng(100 + nvec)
    B, X0 = rng.standard_normal((nvec, n)), 0.1 * rng.standard_normal((nvec, n))
    prm = hip.SolverParams(num_blocks=5, max_iters=7, max_restarts=10 ** 6, tol=0.0, flexible=flexible)
    bflat, xflat = B.ravel().copy(), X0.ravel().copy()
    info = hip.solve(gpu_ctx, A, bflat, xflat, prec=M, nvec=nvec, lda=n, params=prm)
    assert info.iters == 7 * nvec
    for c in range(nvec):
        x = X0[c].copy()
        single = hip.solve(gpu_ctx, A, B[c].copy(), x, prec=M, params=prm)
        assert single.iters == 7 and np.all(np.isfinite(x)) and not np.array_equal(x, X0[c])
        assert np.array_equal(x, xflat[c * n:(c + 1) * n]), c
    M.close(); A.close()


# ---------------------------------------------------------------- 5. solves
@functools.lru_cache(maxsize=None)
def system(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    return rp, ci, val, b, singular, sps.csr_matrix((val, ci, rp), shape=(n, n))


BLOCK = {"tgv16": 256, "wall42": 256, "stencil": 64, "spd": 256}


@pytest.mark.parametrize("name,solver_type,flexible", [("tgv16", 0, 1), ("tgv16", 0, 0), ("wall42", 0, 1), ("wall42", 0, 0),
                                                       ("stencil", 0, 1), ("stencil", 0, 0), ("spd", 0, 1), ("spd", 0, 0),
                                                       ("spd", 1, 0)])
def test_solves_keep_the_iteration_count_of_the_double_preconditioner(gpu_ctx, name, solver_type, flexible):
    rp, ci, val, b, singular, A_h = system(name)
    n = A_h.shape[0]
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    out = {}
    for bits in (64, 32):
        M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0" + ("-f32" if bits == 32 else ""), BLOCK[name])
        assert M.value_bits == (32 if bits == 32 else 0)
        x = np.zeros(n)
        prm = hip.SolverParams(solver_type=solver_type, num_blocks=50, max_iters=500, max_restarts=10 ** 6, tol=1e-8, flexible=flexible)
        info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=prm)
        out[bits] = (x, info)
        M.close()
    A.close()
    (x64, i64), (x32, i32_) = out[64], out[32]
    gx = kr.iterate_gap(x32, x64)
    # the explicit residual: of a singular system the solver reports ||b - A x|| / ||b|| with the UNPROJECTED operator, as
    # the reference does, so for tgv16 the residual of the system that is solved, P (b - A x) with P = I - n n^T, is
    # formed here (as tests/test_gpu_chebyshev_f32.py forms it)
    if singular:
        proj = lambda v: v - v.mean()
        eres = {bits: float(np.linalg.norm(proj(b - A_h @ out[bits][0])) / np.linalg.norm(proj(b))) for bits in (64, 32)}
    else:
        eres = {64: i64.rel_res_explicit, 32: i32_.rel_res_explicit}
    print("\nilu-f32-solve %-8s type %d flexible %d iterations %d (64 bits: %d) explicit residual %.2e (64 bits: %.2e; reported %.2e, "
          "%.2e) x against the 64-bit x %.2e" % (name, solver_type, flexible, i32_.iters, i64.iters, eres[32], eres[64],
                                                i32_.rel_res_explicit, i64.rel_res_explicit, gx))
    assert i64.converged == 1 and i32_.converged == 1
    assert eres[32] <= 1e-7
    assert abs(i32_.iters - i64.iters) <= 1, (i32_.iters, i64.iters)
    assert gx <= 1e-6


# ---------------------------------------------------------------- 6. the library's own row numbering and bricks
def test_the_librarys_bricks(gpu_ctx_bricks):
    """block_size 0 on a matrix the assembly numbered itself: the third route (the library's table of bricks)"""
    from problems import Problem, tgv_spec
    ctx = gpu_ctx_bricks
    pr = Problem(tgv_spec(dim=3, n=16, mode=workload.ADVECT))
    A, bg = hip.assemble_poisson(ctx, pr.parts, pr.colmap, pr.spec.dt, pr.parts["rho"], np.ascontiguousarray(pr.parts["v"]),
                                 vfrac=pr.P.vfrac)
    assert A.ordering() is not None
    r = rhs(pr.n)
    M64 = hip.Precond(ctx, A, "bjacobi-ilu0", 0)
    out = {}
    for label, make in (("64", lambda: M64), ("string", lambda: hip.Precond(ctx, A, "bjacobi-ilu0-f32", 0)),
                        ("struct", lambda: hip.PrecondILU(ctx, A, level_of_fill=0, block_size=0, value_bits=32))):
        M = make()
        x = np.zeros(pr.n)
        info = hip.solve(ctx, A, bg.copy(), x, prec=M, singular=True)
        out[label] = (M.value_bits, M.export_ilu(), M.apply(r), info, x, M.info())
        M.close()
    A.close()
    b64, f64, z64, s64, x64, n64 = out["64"]
    assert b64 == 0 and s64.converged == 1
    for label in ("string", "struct"):
        bits, f, z, s, x, ninfo = out[label]
        g = rel(z, z64)
        print("\nilu-f32-bricks %-6s application against the 64-bit one %.2e, iterations %d (64 bits: %d), x gap %.2e, %d bricks" %
              (label, g, s.iters, s64.iters, kr.iterate_gap(x, x64), ninfo["nblocks"]))
        assert bits == 32 and ninfo == n64 and same_factor(f, f64)
        assert 1e-10 <= g <= 1e-6, g
        assert s.converged == 1 and abs(s.iters - s64.iters) <= 1
    assert np.array_equal(out["string"][2], out["struct"][2])


# ---------------------------------------------------------------- 7. refusals and edges
def _entry(rp, ci, i, j):
    return rp[i] + int(np.flatnonzero(ci[rp[i]:rp[i + 1]] == j)[0])


def test_refusals(gpu_ctx):
    rp, ci, val, bp = sh.fixture("narrow")
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    for bits in (16, 33, -1):
        with pytest.raises(hip.IsphError, match="value_bits"):
            hip.PrecondILU(gpu_ctx, A, block_ptr=bp, value_bits=bits)
        with pytest.raises(hip.IsphError, match="value_bits"):
            hip.PrecondILU(gpu_ctx, A, block_size=256, value_bits=bits)
    for kind in ("bjacobi-ilu0-f3", "bjacobi-ilu0-f32x", "bjacobi-ilu9-f32"):
        with pytest.raises(hip.IsphError, match="unknown preconditioner type"):
            hip.Precond(gpu_ctx, A, kind, 256)
    with pytest.raises(hip.IsphError, match="bjacobi-ilu<k>-f32"):
        hip.Precond(gpu_ctx, A, "bjacobi-ilu0-f3", 256)
    A.close()


def test_range_check_and_underflow(gpu_ctx):
    rp, ci, val, bp = sh.fixture("narrow")
    n = len(rp) - 1
    r = rhs(n)
    i = int(bp[1])                                              # first row of the second block: u_ij = a_ij, no update
    cols = ci[rp[i]:rp[i + 1]]
    inside = cols[(cols > i) & (cols < bp[2])]
    outside = cols[(cols < bp[1]) | (cols >= bp[2])]
    assert len(inside) and len(outside)
    forms = [lambda A: hip.Precond(gpu_ctx, A, "bjacobi-ilu0-f32", block_ptr=bp), lambda A: hip.Precond(gpu_ctx, A, "bjacobi-ilu0-f32", 256),
             lambda A: hip.PrecondILU(gpu_ctx, A, block_ptr=bp, value_bits=32)]
    # beyond FLT_MAX (finite in fp64) on an in-block upper entry: refused by the 32-bit forms only
    v = val.copy(); v[_entry(rp, ci, i, int(inside[0]))] = 1e39
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    for make in forms:
        with pytest.raises(hip.IsphError, match="exceeds the range of single precision"):
            make(Az)
    M = hip.Precond(gpu_ctx, Az, "bjacobi-ilu0", block_ptr=bp)
    assert M.value_bits == 0
    M.close()
    hip.PrecondILU(gpu_ctx, Az, block_ptr=bp, value_bits=64).close()
    Az.close()
    # the same value on an entry that couples two blocks: dropped by block Jacobi, never in the stream
    v = val.copy(); v[_entry(rp, ci, i, int(outside[0]))] = 1e39
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    for make in forms:
        M = make(Az)
        f = M.export_ilu()
        g = rel(M.apply(r), i32.apply(f[0], f[1], f[2], bp, r))
        print("\nilu-f32-range 1e39 between two blocks: accepted, gap to the rounded factor %.2e" % g)
        assert M.value_bits == 32 and g <= APPLY_TOL
        M.close()
    Az.close()
    # an in-block entry that rounds to 0 is accepted: it is 0 in the solves
    v = val.copy(); v[_entry(rp, ci, i, int(inside[0]))] = 1e-50
    Az = hip.Matrix.from_csr(gpu_ctx, rp, ci, v)
    for make in forms:
        M = make(Az)
        f = M.export_ilu()
        k = _entry(f[0], f[1], i, int(inside[0]))
        assert f[2][k] == 1e-50 and i32.round_factor(f[0], f[1], f[2])[k] == 0.0
        g = rel(M.apply(r), i32.apply(f[0], f[1], f[2], bp, r))
        print("\nilu-f32-underflow gap to the rounded factor %.2e" % g)
        assert g <= APPLY_TOL
        M.close()
    Az.close()


def test_empty_matrix(gpu_ctx):
    """n = 0: nothing to round, the create call succeeds (rowptr = [0]; one unused slot keeps the arrays' pointers non-NULL)"""
    A = hip.Matrix.from_csr(gpu_ctx, np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1))
    assert A.info()["nrow"] == 0
    for make in (lambda: hip.Precond(gpu_ctx, A, "bjacobi-ilu0-f32", 64), lambda: hip.PrecondILU(gpu_ctx, A, block_size=64, value_bits=32)):
        M = make()
        assert M.value_bits == 32
        M.close()
    A.close()


# ---------------------------------------------------------------- 8. the C++ wrapper's key
def run_cpp(tmp_path, name, bits, block_rows, fill=0):
    rp, ci, val, b, singular = system(name)[:5]
    n = len(rp) - 1
    fin, fout = str(tmp_path / "sys.bin"), str(tmp_path / ("x%d.bin" % bits))
    with open(fin, "wb") as f:
        np.array([n, len(val)], np.int32).tofile(f)
        rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); val.tofile(f); b.tofile(f)
    r = subprocess.run([build.build_cpp_ilu_f32_test(), fin, fout, "1" if singular else "0", str(bits), str(block_rows), str(fill)],
                       capture_output=True, text=True, timeout=120)
    return r, (np.fromfile(fout) if r.returncode == 0 else None)


def _iters(r):
    line = [l for l in r.stdout.splitlines() if l.startswith("converged=")][-1]
    return tuple(int(t.split("=")[1]) for t in line.split()[:2])


@pytest.mark.parametrize("name", ["tgv16", "wall42"])
def test_wrapper_key_solves_like_the_64_bit_run(gpu_ctx, tmp_path, name):
    r64, x64 = run_cpp(tmp_path, name, 64, 256)
    r32, x32 = run_cpp(tmp_path, name, 32, 256)
    assert r64.returncode == 0, r64.stdout[-2000:] + r64.stderr[-2000:]
    assert r32.returncode == 0, r32.stdout[-2000:] + r32.stderr[-2000:]
    (c64, k64), (c32, k32) = _iters(r64), _iters(r32)
    g = kr.iterate_gap(x32, x64)
    # the same solve through Python: the wrapper with 32 built what "bjacobi-ilu0-f32" builds
    rp, ci, val, b, singular = system(name)[:5]
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0-f32", 256)
    x = np.zeros(len(rp) - 1)
    info = hip.solve(gpu_ctx, A, b.copy(), x, prec=M, singular=singular, params=hip.SolverParams())
    M.close(); A.close()
    gp = kr.iterate_gap(x32, x)
    print("\nilu-f32-wrapper %-8s iterations %d (64 bits: %d, python 32 bits: %d) x against the 64-bit x %.2e, against python's %.2e" %
          (name, k32, k64, info.iters, g, gp))
    assert c64 == 1 and c32 == 1
    assert abs(k32 - k64) <= 1, (k32, k64)
    assert g <= 1e-6
    assert info.converged == 1 and k32 == info.iters and gp <= 1e-6
    assert not np.array_equal(x32, x64)                         # the key reached the device: another operator


def test_wrapper_refuses_other_widths_and_names_the_key(tmp_path):
    r, _ = run_cpp(tmp_path, "stencil", 16, 64)
    assert r.returncode == 1
    assert "isph: ilu value bits" in r.stderr and "not available" in r.stderr, r.stderr


@pytest.mark.parametrize("block_rows", [0, 2048])
def test_wrapper_refuses_32_bits_on_the_schwarz_routes_and_names_both_keys(tmp_path, block_rows):
    r, _ = run_cpp(tmp_path, "stencil", 32, block_rows)
    assert r.returncode == 1
    assert "isph: ilu value bits" in r.stderr and "isph: block rows" in r.stderr, r.stderr
    if block_rows == 0:
        r, _ = run_cpp(tmp_path, "stencil", 64, block_rows)    # the same request in double is served
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
