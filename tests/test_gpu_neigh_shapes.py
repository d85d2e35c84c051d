"""-m gpu: every branch of the neighbour-list layout (csrc/assemble.hpp: build_neigh_ell_t, k_neigh_sort, k_neigh_transpose)
and of what reads it (k_asm_count, the diagonal-slot rule of the Poisson / Helmholtz / block Helmholtz row kernels, the
duplicate merge, the choice of the SELL row sort) on the constructed lists of tests/neigh_shapes.py.

tests/test_neigh_shapes_host.py shows, without a GPU, WHICH branch each fixture reaches (the table in its docstring) and that
the lists are valid: nothing here can index out of range.  The reference is always the oracle GIVEN THE SAME LIST; the
tolerances are the project's own (pattern exact, values and right-hand sides 1e-12 of the largest, volumes 1e-13 relative).
Above 32 768 rows the order k_neigh_sort leaves is the order of the matrix row (no SELL row sort behind it).  The exports
sort the rows they return, so that order does not show in export_csr: it shows in the bit-for-bit tests (the sums follow
the list order) and in the block-ILU set-up, which reads the rows as stored and refuses unsorted ones
(device_rows_ascend: called on every Poisson and Helmholtz matrix and on every block of the block Helmholtz system, so
that the copy of the slot rule in each row kernel is seen where it decides the stored order).

Found with these fixtures, and fixed: above 32 768 rows the three assemblies skipped the duplicate merge ("tiny boxes"),
but a box is thin as soon as ONE periodic direction is shorter than two cuts.  Shape: thin_dup-big, 8200 x 4 cells, cut =
3 dx, 32 800 rows -- the device returned 885 050 entries with repeated columns where the oracle has 688 662 (the first
assertion of check_matrix: the row pointers differ; Helmholtz and block Helmholtz alike).  The row kernels now raise a
device flag when a sorted row receives a column twice, and such rows are merged in one pass for every n
(merge_adjacent_row; thin_dup-big, thin_self-big); the unsorted layout above the threshold (overcap) goes through
k_sell_merge_duplicates like the small problems.

Symmetric family: G_i and L_i are inputs of the assembly.  Rows truncated to 0 .. 3 entries (short, p512) have singular
moment matrices, so the tensors that follow from the constructed list are nan or of order 1e33 there; both the oracle and
the device are given the tensors of the unedited list instead (particles()).  A design choice: for those few rows the
tensors are not the ones of the list under test, for all rows the comparison means something at 1e-12.

Bit for bit (test_bits_*): on a sorted layout the row kernels sum in column order whatever the caller's order and skip
out-of-cut entries, so a shuffled and padded list gives the bits of the same list pre-sorted without its padding; 32- and
64-bit offsets and host and device arrays reach the same kernels.
"""
import functools

import numpy as np
import pytest

from isph_amd import hip
import oracle as orc
import neigh_shapes as ns

pytestmark = pytest.mark.gpu

THETA = 0.5
HELMHOLTZ = [(name, size) for name in ("short", "p1024", "overcap", "thin_dup") for size in ("small", "big")]
UNSORTED = [(name, size) for name in ("short", "p1024", "overcap", "widths") for size in ("small", "big")]
SYMMETRIC = [(name, size) for name in ("short", "p512") for size in ("small", "big")]


# ---------------------------------------------------------------- references, computed once and left unchanged
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def particles(name, size, corrections=False):
    c, u, cm, notes = ns.fixture(name, size)
    P = orc.Particles(c, cm)
    P.precompute(corrections=corrections)
    if corrections:
        # G_i and L_i are inputs of the assembly, on the device and in the oracle alike.  A row truncated to 0 .. 3 entries
        # has a singular moment matrix: its tensors are nan or of order 1e33, and the entries formed with them are round-off
        # in either implementation.  Both sides are given the tensors of the unedited list (padding does not change them),
        # so that every row, the truncated ones included, has a reference that means something at 1e-12.
        Pu = orc.Particles(u, cm)
        Pu.precompute(corrections=True)
        P.Gc[:] = Pu.Gc
        P.Lc[:] = Pu.Lc
    return P


@functools.lru_cache(maxsize=None)
def ref_poisson(name, size, antisym=True):
    c, u, cm, notes = ns.fixture(name, size)
    P = particles(name, size, not antisym)
    return _frozen(*P.poisson(c["spec"].dt, c["rho"], c["v"], antisym=antisym))


def fields(c):
    """smooth pressure, force, viscosity and gravity for the Helmholtz assemblies; owners and images agree (periodic in x, y)"""
    x, nall = c["x"], c["nall"]
    box = c["spec"].dx * np.array(c["spec"].ncell[:2])
    kx, ky = 2 * np.pi / box[0], 2 * np.pi / box[1]
    pres = np.cos(kx * x[:, 0]) * np.sin(ky * x[:, 1])
    force = np.ascontiguousarray(0.01 * np.stack([np.sin(ky * x[:, 1]), np.cos(kx * x[:, 0]), np.zeros(nall)], axis=1))
    nu = c["nu"] * (1.0 + 0.1 * np.sin(kx * x[:, 0]))
    return pres, force, nu, np.array([0.05, -0.02, 0.0]), np.ascontiguousarray(c["v"])


@functools.lru_cache(maxsize=None)
def ref_helmholtz(name, size):
    c, u, cm, notes = ns.fixture(name, size)
    pres, force, nu, g, vel = fields(c)
    return _frozen(*particles(name, size).helmholtz(c["spec"].dt, THETA, nu, c["rho"], pres, force, g, vel))


@functools.lru_cache(maxsize=None)
def ref_block_helmholtz(name, size):
    c, u, cm, notes = ns.fixture(name, size)
    pres, force, nu, g, vel = fields(c)
    return _frozen(*particles(name, size).block_helmholtz(c["spec"].dt, THETA, 0.3, nu, c["rho"], pres, force, g, vel))


def scalar_field(c):
    x = c["x"]
    box = c["spec"].dx * np.array(c["spec"].ncell[:2])
    return np.cos(2 * np.pi / box[0] * x[:, 0]) + np.sin(4 * np.pi / box[1] * x[:, 1])


@functools.lru_cache(maxsize=None)
def ref_gradient(name, size):
    c, u, cm, notes = ns.fixture(name, size)
    return _frozen(particles(name, size).gradient(scalar_field(c), True))[0]


# ---------------------------------------------------------------- helpers
def check_matrix(A, rp, ci, val, label, vscale=None):
    """export_csr is the oracle's CSR: pattern exact, every row strictly ascending, info()["nnz"] the oracle's count, values
    within 1e-12 of the largest"""
    grp, gci, gv = A.export_csr()
    assert np.array_equal(grp, rp), (label, "row pointers", int(grp[-1]), int(rp[-1]))
    assert np.array_equal(gci, ci), (label, "columns")
    rows = ns.rows_of(grp)
    assert np.all(np.diff(gci)[np.diff(rows) == 0] > 0), (label, "rows not strictly ascending")
    assert A.info()["nnz"] == len(ci), (label, A.info()["nnz"], len(ci))
    scale = np.abs(val).max() if vscale is None else vscale
    err = np.max(np.abs(gv - val)) if len(val) else 0.0
    assert err <= 1e-12 * scale, (label, err / scale)


def device_rows_ascend(ctx, A):
    """export_csr and export_rows sort the rows they return (std::stable_sort), so the order the rows have ON THE DEVICE does
    not show there.  The block-ILU set-up reads the rows as they are stored and refuses, with an error and without harm,
    a row whose in-block columns are not strictly ascending ("duplicate or unsorted columns"): built here for that check."""
    hip.Precond(ctx, A, "bjacobi-ilu0", 512).close()


def check_rhs(bg, b, label):
    err = np.max(np.abs(np.asarray(bg) - b.ravel()))
    assert err <= 1e-12 * np.abs(b).max(), (label, err / np.abs(b).max())


def poisson(ctx, c, cm, vfrac, antisym=True, Gc=None, Lc=None):
    return hip.assemble_poisson(ctx, c, cm, c["spec"].dt, c["rho"], np.ascontiguousarray(c["v"]), antisym=antisym, vfrac=vfrac,
                                Gc=Gc, Lc=Lc)


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def device_list(c, cm, vfrac):
    """the particle arrays, the list and the operands of the Poisson assembly as device tensors"""
    d = dict(c)
    for k in ("x", "type", "neigh_ptr", "neigh_idx"):
        d[k] = to_dev(c[k])
    return d, to_dev(cm), to_dev(c["rho"]), to_dev(np.ascontiguousarray(c["v"])), to_dev(vfrac)


def device_poisson(ctx, c, cm, vfrac):
    d, cmd, rho, vstar, vf = device_list(c, cm, vfrac)
    A, b = hip.assemble_poisson(ctx, d, cmd, c["spec"].dt, rho, vstar, vfrac=vf)
    return A, b.cpu().numpy()


def bits(A, b):
    out = tuple(A.export_csr()) + (np.asarray(b),)
    A.close()
    return out


def same_bits(got, want, label):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (label, ("rowptr", "colidx", "val", "b")[k])


# ---------------------------------------------------------------- Poisson, every fixture, both row numberings
@pytest.mark.parametrize("fx", ns.FIXTURES, ids=ns.ident)
def test_poisson_matches_the_oracle_on_the_same_list(gpu_ctx_both, fx):
    """AntiSymmetric family: matrix, right-hand side, strictly ascending rows and the entry count, in the caller's row
    numbering and in the library's own"""
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    rp, ci, val, b = ref_poisson(name, size)
    A, bg = poisson(gpu_ctx_both, c, cm, particles(name, size).vfrac)
    check_matrix(A, rp, ci, val, fx)
    check_rhs(bg, b, fx)
    device_rows_ascend(gpu_ctx_both, A)
    A.close()


@pytest.mark.parametrize("fx", SYMMETRIC, ids=ns.ident)
def test_poisson_symmetric_family_matches_the_oracle(gpu_ctx_both, fx):
    """the corrected (Symmetric) family reads G_i / L_i and runs its own instantiation of the row kernel"""
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    P = particles(name, size, True)
    rp, ci, val, b = ref_poisson(name, size, False)
    A, bg = poisson(gpu_ctx_both, c, cm, P.vfrac, antisym=False, Gc=P.Gc, Lc=P.Lc)
    check_matrix(A, rp, ci, val, fx)
    check_rhs(bg, b, fx)
    device_rows_ascend(gpu_ctx_both, A)
    A.close()


# ---------------------------------------------------------------- the Helmholtz kernels carry their own slot rule and threshold
@pytest.mark.parametrize("fx", HELMHOLTZ, ids=ns.ident)
def test_helmholtz_matches_the_oracle_on_the_same_list(gpu_ctx_both, fx):
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    pres, force, nu, g, vel = fields(c)
    rp, ci, val, b = ref_helmholtz(name, size)
    A, bg = hip.assemble_helmholtz(gpu_ctx_both, c, cm, c["spec"].dt, THETA, nu, c["rho"], pres, force, g, vel,
                                   vfrac=particles(name, size).vfrac)
    check_matrix(A, rp, ci, val, fx)
    check_rhs(bg, b, fx)
    device_rows_ascend(gpu_ctx_both, A)                     # k_asm_helmholtz' own slot rule and row-sort choice
    A.close()


@pytest.mark.parametrize("fx", HELMHOLTZ, ids=ns.ident)
def test_block_helmholtz_diagonal_blocks_match_the_oracle(gpu_ctx_both, fx):
    """without wall normals: the diagonal blocks and the right-hand side (off-diagonal blocks, where the library returns
    them, hold the same pattern)"""
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    pres, force, nu, g, vel = fields(c)
    rp, ci, vals, b = ref_block_helmholtz(name, size)
    blocks, bg = hip.assemble_block_helmholtz(gpu_ctx_both, c, cm, c["spec"].dt, THETA, 0.3, nu, c["rho"], pres, force, g, vel,
                                              vfrac=particles(name, size).vfrac)
    dim = c["dim"]
    for ib in range(dim):
        for jb in range(dim):
            if blocks[ib][jb] is None:
                assert ib != jb and not vals[ib * dim + jb].any()
                continue
            check_matrix(blocks[ib][jb], rp, ci, vals[ib * dim + jb], (fx, ib, jb), vscale=np.abs(vals).max())
            device_rows_ascend(gpu_ctx_both, blocks[ib][jb])                  # k_asm_block_helmholtz' own slot rule, every block
            blocks[ib][jb].close()
    check_rhs(bg, b, fx)


# ---------------------------------------------------------------- bit for bit on the sorted layouts
@pytest.mark.parametrize("fx", ns.SORTED_UNIQUE, ids=ns.ident)
def test_bits_do_not_depend_on_order_padding_offset_width_or_side(gpu_ctx_both, fx):
    """the constructed list against (a) the same list with every row pre-sorted by column and the padding removed, (b) the
    same list with 64-bit offsets (neigh_ptr64), (c) the same list as device tensors: matrix and right-hand side equal bit
    for bit"""
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    assert ns.regimes(c, cm)["sorted"] and ns.regimes(c, cm)["duplicates"] == 0
    vfrac = particles(name, size).vfrac
    want = bits(*poisson(gpu_ctx_both, c, cm, vfrac))
    same_bits(bits(*poisson(gpu_ctx_both, ns.canonical(c, cm), cm, vfrac)), want, (fx, "pre-sorted, no padding"))
    c64 = dict(c)
    c64["neigh_ptr"] = c["neigh_ptr"].astype(np.int64)
    same_bits(bits(*poisson(gpu_ctx_both, c64, cm, vfrac)), want, (fx, "neigh_ptr64"))
    same_bits(bits(*device_poisson(gpu_ctx_both, c, cm, vfrac)), want, (fx, "device tensors"))


# ---------------------------------------------------------------- the layout without a column map
@pytest.mark.parametrize("fx", UNSORTED, ids=ns.ident)
def test_unsorted_layout_volumes_and_gradient(gpu_ctx_both, fx):
    """compute_volumes and the gradient read the list in the caller's order (no column map, no k_neigh_sort): rows of every
    length through k_numneigh / k_slicew_from_rowlen / k_neigh_transpose alone"""
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    P = particles(name, size)
    n = c["nlocal"]
    vg = hip.compute_volumes(gpu_ctx_both, c, cm)
    assert np.max(np.abs(vg - P.vfrac[:n]) / P.vfrac[:n]) < 1e-13
    want = ref_gradient(name, size)
    got = hip.gradient(gpu_ctx_both, c, cm, scalar_field(c), P.vfrac, antisym=True)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------- held list
@pytest.mark.parametrize("size", ["small", "big"])
def test_held_list_reuses_the_sorted_layout_bit_for_bit(gpu_ctx_both, size):
    """isph_ctx_hold_neighbours on p512: the second Poisson assembly and the second compute_volumes run on the layouts the
    first ones left in the context (sorted with a bitonic stride, and unsorted); all equal the un-held results"""
    c, u, cm, notes = ns.fixture("p512", size)
    ctx = gpu_ctx_both
    d, cmd, rho, vstar, vf = device_list(c, cm, particles("p512", size).vfrac)

    def run():
        vol = hip.compute_volumes(ctx, d, cmd).cpu().numpy()
        A, b = hip.assemble_poisson(ctx, d, cmd, c["spec"].dt, rho, vstar, vfrac=vf)
        return (vol,) + bits(A, b.cpu().numpy())

    free = run()
    ctx.hold_neighbours(True)
    try:
        first, second = run(), run()
    finally:
        ctx.hold_neighbours(False)
    for k, (a, b1, b2) in enumerate(zip(free, first, second)):
        assert np.array_equal(a, b1) and np.array_equal(a, b2), k
    rp, ci, val, b = ref_poisson("p512", size)
    assert np.array_equal(free[1], rp) and np.array_equal(free[2], ci)


# ---------------------------------------------------------------- downstream of the rows
@pytest.mark.parametrize("name", ["thin_dup", "p256", "p512", "p1024"])
def test_block_ilu0_on_the_assembled_rows_matches_the_oracle(gpu_ctx, name):
    """above the threshold: ILU extraction walks the rows as the assembly left them (one entry per column, ascending).
    Pattern of the factor exact, one application at the tolerance of test_ilu0_factor_and_apply_match_oracle."""
    c, u, cm, notes = ns.fixture(name, "big")
    rp, ci, val, b = ref_poisson(name, "big")
    n = c["nlocal"]
    A, bg = poisson(gpu_ctx, c, cm, particles(name, "big").vfrac)
    check_matrix(A, rp, ci, val, name)                      # first: the factorisation below is only defined on merged rows
    bs = 512
    bp = np.arange(0, n + bs, bs).clip(0, n).astype(np.int32)
    ref = orc.ILU(rp, ci, val, 0, bp)
    frp, fci, fv = ref.export()
    M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", bs)
    grp, gci, gv = M.export_ilu()
    assert np.array_equal(grp, frp) and np.array_equal(gci, fci)
    r = np.random.default_rng(5).standard_normal(n)
    z, zo = M.apply(r), ref.apply(r)
    # the ladders hold a row without neighbours: its Poisson row is a zero diagonal alone, the pivot of its block is 0 and
    # the oracle's application is not finite there.  The blocks are independent (block Jacobi): every other block is
    # compared at the tolerance, nothing is asked of the block with the zero pivot.
    rows = ns.rows_of(rp)
    zero_pivot = np.unique(rows[(ci == rows) & (val == 0.0)] // bs)
    assert len(zero_pivot) == (0 if name == "thin_dup" else 1)
    ok = ~np.isin(np.arange(n) // bs, zero_pivot)
    assert np.isfinite(zo[ok]).all() and np.isfinite(z[ok]).all()
    assert np.linalg.norm(z[ok] - zo[ok]) / np.linalg.norm(zo[ok]) < 1e-11
    M.close()
    A.close()
