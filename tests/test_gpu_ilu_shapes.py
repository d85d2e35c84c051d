"""-m gpu: every row-shape branch of block ILU(k) (csrc/ilu.hpp) and the same matrices through additive Schwarz
(csrc/schwarz.hpp), on the constructed fixtures of tests/ilu_shapes.py against its long-double reference.

tests/test_ilu_shapes_host.py shows, without a GPU, WHICH branch each fixture reaches (the regime table in its docstring)
and that the oracle agrees with the reference; here the device does: factor pattern exact, factor values under the
project's entrywise rule (relative 1e-10, floor 1e-10 max|f|: test_ilu0_factor_and_apply_match_oracle), application within
1e-11.  On these diagonally dominant matrices an omitted or doubled update term is off by 1e-4 or more.

Every test prints the device's deviation from the reference beside the oracle's."""
import numpy as np
import pytest

from isph_amd import hip
import oracle as orc
import ilu_shapes as sh

pytestmark = pytest.mark.gpu

LD = np.longdouble


def entrywise(gv, fv):
    """the project's rule for factor values: relative, with a floor of 1e-10 max|f| under the denominator"""
    fmax = np.abs(fv).max()
    return float(np.max(np.abs(gv - fv) / np.maximum(np.abs(fv), 1e-300 + 1e-10 * fmax)))


def rel(z, zo):
    return float(np.linalg.norm(np.asarray(z, dtype=LD) - zo) / np.linalg.norm(zo))


def uniform_block(bp):
    """the block size whose uniform decomposition IS the table bp (the last block may be shorter), or None"""
    B, n = int(bp[1] - bp[0]), int(bp[-1])
    same = B % 64 == 0 and np.array_equal(bp, np.arange(0, n + B, B).clip(0, n)[:len(bp)]) and len(bp) == (n + B - 1) // B + 1
    return B if same else None


def rhs(n):
    return np.random.default_rng(5).standard_normal(n)


def check(label, name, K, exported, apply):
    """exported: (rowptr, colidx, val) of the device factor in global columns; apply: r -> z on the device"""
    rp, ci, val, bp = sh.fixture(name)
    n = len(rp) - 1
    frp, fci, fv = sh.ref_iluk_of(name, K)
    grp, gci, gv = exported
    O = orc.ILU(rp, ci, val, K, bp)
    ov = O.export()[2]
    r = rhs(n)
    zo = sh.ref_apply_of(name, K, r)
    same_pattern = np.array_equal(np.asarray(grp, dtype=np.int64), frp) and np.array_equal(gci, fci)
    z = apply(r)
    print("\n%s %s K=%d: factor entrywise device %.2e (oracle %.2e), apply device %.2e (oracle %.2e)" %
          (label, name, K, entrywise(gv, fv) if same_pattern else np.nan, entrywise(ov, fv), rel(z, zo), rel(O.apply(r), zo)))
    assert same_pattern                                                     # factor pattern: exact
    assert entrywise(gv, fv) < 1e-10
    assert rel(z, zo) < 1e-11


def bjacobi_forms(bp, K):
    """(label, constructor) of the block-Jacobi forms that give the decomposition bp: the caller's table, and the uniform
    block size where the table is uniform"""
    kind = "bjacobi-ilu%d" % K
    forms = [("table", lambda ctx, A: hip.Precond(ctx, A, kind, block_ptr=bp))]
    B = uniform_block(bp)
    if B is not None:
        forms.append(("uniform %d" % B, lambda ctx, A: hip.Precond(ctx, A, kind, B)))
    return forms


# ---------------------------------------------------------------- block ILU(0)
@pytest.mark.parametrize("name", sh.ILU0_FIXTURES)
def test_block_ilu0_on_every_row_shape(gpu_ctx, name):
    """narrow ladder (fast loop, dg > 64, pivot rows beyond 64 entries in the narrow template), longest row 128 / 129 / 130
    (129: WIDE factor kernel with the NARROW schedule), wide ladder (dg > 64 and pivot rows beyond 128 in the WIDE template,
    rows exactly on 64/65 and 128/129), fan (levels of 232 and 256 rows, three runs of 64 ranks, rows of 65..127
    dependencies in them), ragged table (blocks of 1, 63, 64, 65 and 1024 rows)"""
    rp, ci, val, bp = sh.fixture(name)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    forms = bjacobi_forms(bp, 0)
    assert len(forms) == (1 if name == "ragged" else 2)
    for label, make in forms:
        M = make(gpu_ctx, A)
        assert M.info()["nblocks"] == len(bp) - 1
        check("bjacobi-ilu0 " + label, name, 0, M.export_ilu(), M.apply)
        M.close()
    A.close()


# ---------------------------------------------------------------- block ILU(k)
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("name", sh.ILUK_FIXTURES)
def test_block_iluk_on_nonsymmetric_patterns(gpu_ctx, name, K):
    """k_iluk_merge on structurally nonsymmetric input, rows that grow from at most 15 entries past 64 and past 128 (up to
    714) during the sweeps, blocks of 64 / 256 / 512 / 1024 rows with a ragged tail; the numeric kernels on the result"""
    rp, ci, val, bp = sh.fixture(name)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    forms = bjacobi_forms(bp, K)
    assert len(forms) == 2
    for label, make in forms:
        M = make(gpu_ctx, A)
        check("bjacobi-ilu%d %s" % (K, label), name, K, M.export_ilu(), M.apply)
        M.close()
    A.close()


# ---------------------------------------------------------------- stream sized by the counting pass
def test_exact_stream_gives_the_same_bits(gpu_ctx):
    """isph_set_exact_stream_threshold(0): the schedule's counting pass sizes the stream (capacity factor 1, no slack); the
    factor and the application carry the bits of the default path"""
    rp, ci, val, bp = sh.fixture("narrow")
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    r = rhs(len(rp) - 1)
    for label, make in bjacobi_forms(bp, 0):
        M0 = make(gpu_ctx, A)
        f0, z0, i0 = M0.export_ilu(), M0.apply(r), M0.info()
        try:
            hip.set_exact_stream_threshold(0)
            M1 = make(gpu_ctx, A)
        finally:
            hip.set_exact_stream_threshold(-1)
        f1, z1, i1 = M1.export_ilu(), M1.apply(r), M1.info()
        assert i1["stream_chunks"] == i0["stream_chunks"] and i1["stream_capacity"] < i0["stream_capacity"], label
        for a, b in zip(f0, f1):
            assert np.array_equal(a, b), label
        assert np.array_equal(z0, z1), label
        check("exact stream " + label, "narrow", 0, f1, M1.apply)
        M0.close(); M1.close()
    A.close()


# ---------------------------------------------------------------- several right-hand sides in one sweep
@pytest.mark.parametrize("flexible", [0, 1])
@pytest.mark.parametrize("nvec", [2, 3, 4])
@pytest.mark.parametrize("name", ["narrow", "fan"])
def test_multi_vector_sweep_carries_the_bits_of_single_applications(gpu_ctx, name, nvec, flexible):
    """k_ilu_solve_stream_multi "every vector goes through exactly the operations of k_ilu_solve_stream, in the same order":
    nvec columns advancing together through 7 iterations of GMRES(5) with a block ILU(0) preconditioner equal, bit for
    bit, their own single-vector solves.  (flexible 0 solves the columns one after the other: the control.  The library
    sweeps once for all vectors only while 32 (nvec + 1) B bytes fit the LDS the device reports for a workgroup -- at most
    40 KB for the narrow ladder, B = 256, which every device gives; 80 KB for the fan at nvec = 4, which takes the
    single sweeps where the runtime reports 64 KB.)"""
    rp, ci, val, bp = sh.fixture(name)
    n = len(rp) - 1
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", block_ptr=bp)
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


# ---------------------------------------------------------------- additive Schwarz on the same matrices
WHOLE_MATRIX_FORM = 1


def schwarz_check(label, name, M, form):
    rp, ci, val, bp = sh.fixture(name)
    n = len(rp) - 1
    assert M.schwarz_info()["persistent"] == form and M.schwarz_info()["nsub"] == len(bp) - 1
    rows, lp, grp, gci, gv = M.export()
    assert np.array_equal(rows, np.arange(n)) and np.array_equal(lp, bp)      # overlap 0: the subdomains are the blocks
    check(label, name, 0, (grp, gci, gv), M.apply)


@pytest.mark.parametrize("name", ["narrow", "wide", "fan", "sub128"])
def test_schwarz_level_launches_on_the_blocks(gpu_ctx, name):
    """overlap 0 with the block size of the fixture: the same factors, one launch per dependency level"""
    rp, ci, val, bp = sh.fixture(name)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondSchwarz(gpu_ctx, A, level_of_fill=0, overlap=0, block_size=uniform_block(bp), level_launches=True)
    schwarz_check("schwarz level launches", name, M, 0)
    M.close(); A.close()


def test_schwarz_one_workgroup_per_subdomain(gpu_ctx):
    """40 subdomains of 128 rows: the default form is one workgroup per subdomain (schwarz_info persistent == 2)"""
    rp, ci, val, bp = sh.fixture("sub128")
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondSchwarz(gpu_ctx, A, level_of_fill=0, overlap=0, block_size=128)
    assert M.schwarz_info()["nsub"] >= 32
    schwarz_check("schwarz subdomain sweeps", "sub128", M, 2)
    M.close(); A.close()


@pytest.mark.parametrize("name", ["one_narrow", "one_wide"])
def test_schwarz_whole_matrix_form(gpu_ctx, name):
    """block_size 0, one subdomain = the whole matrix (one ladder block, narrow and wide rows).  create() reports form 1 for
    it, the persistent sweeps in which a row waits for the words it depends on: one subdomain is fewer than the 32 of
    the one-workgroup form, and 256 / 512 rows over some hundred levels are far from the 4096 rows per level at which
    create() goes back to a launch per level"""
    rp, ci, val, bp = sh.fixture(name)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondSchwarz(gpu_ctx, A, level_of_fill=0, overlap=0, block_size=0)
    print("\n%s: whole-matrix form %d" % (name, M.schwarz_info()["persistent"]))
    schwarz_check("schwarz whole matrix", name, M, WHOLE_MATRIX_FORM)
    M.close(); A.close()


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("combine", ["add", "zero"])
def test_schwarz_overlap_on_a_nonsymmetric_pattern(gpu_ctx, combine, fill):
    """"Overlap Level" 1 where "the rows its columns reference" is one-directional: the extended row lists and loc_ptr exact
    (against the oracle and against ilu_shapes.extended_rows), factor pattern exact, factor and application with the
    tolerances of test_schwarz_overlap_matches_oracle"""
    rp, ci, val, bp = sh.fixture("sub128c3")
    n = len(rp) - 1
    ref = orc.Schwarz(rp, ci, val, fill, bp, 1, combine)
    orow, olp, orp, oci, ov = ref.export()
    erow, elp = sh.extended_rows(rp, ci, bp, 1)
    assert np.array_equal(orow, erow) and np.array_equal(olp, elp)
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M = hip.PrecondSchwarz(gpu_ctx, A, level_of_fill=fill, overlap=1, combine=combine, block_size=128)
    rows, lp, grp, gci, gv = M.export()
    assert np.array_equal(rows, orow) and np.array_equal(lp, olp)
    assert np.array_equal(grp, orp) and np.array_equal(gci, oci)
    r = rhs(n)
    z, zo = M.apply(r), ref.apply(r)
    print("\nschwarz overlap 1 %s fill %d: form %d, factor entrywise device vs oracle %.2e, apply %.2e" %
          (combine, fill, M.schwarz_info()["persistent"], entrywise(gv, ov), np.linalg.norm(z - zo) / np.linalg.norm(zo)))
    assert entrywise(gv, ov) < 1e-10
    assert np.linalg.norm(z - zo) / np.linalg.norm(zo) < 1e-11
    M.close(); A.close()
