"""-m gpu: every branch of the sliced-ELL layer (csrc/sell.hpp) and of the chunked host ingress (csrc/ingress.hpp) on the
constructed matrices of tests/sell_shapes.py.

tests/test_sell_shapes_host.py shows, without a GPU, WHICH branch each fixture reaches (the table in its docstring) and that
a misplaced entry changes what is compared here.  The matrices hold small integers and x an odd integer below 2^20 per
column, so every product and every export below is compared with np.array_equal: no tolerance anywhere.  The one
comparison on arbitrary doubles (test_product_bits_follow_the_documented_order) is bit for bit as well.

Found while writing these tests, and fixed: isph_mat_export_csr (and isph_mat_export_rows of a matrix in the library's own
numbering) re-sorted every exported row with std::sort, which does not keep equal keys in order: on a sorted row of 17 or
more entries libstdc++ exchanges the two entries of a duplicate column, so the export gave their values the wrong way
round although k_sell_sort_rows had ranked them by position (shape: any row of the unsorted ladder with more than 16
entries and a duplicate column).  The exports now use std::stable_sort.  The kernels themselves passed everything here.

Not reachable within the 560 000-entry limit: a 32-bit chunk in FRONT of a 16-bit one (chunk 0 decides for the whole matrix,
so it takes three chunks), hence the hand-over inside a row is exercised 16 -> 32 only.
"""
import functools

import numpy as np
import pytest

from isph_amd import hip
import sell_shapes as sh

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
PATHS = ["host", "device"]


# ---------------------------------------------------------------- shared references, computed once
@functools.lru_cache(maxsize=None)
def ref(name):
    """(sorted CSR, exact product, x, regimes) of a fixture; for a halo fixture the product of the folded square matrix
    on the owned part of x"""
    fx = sh.fixture(name)
    rp, ci, val, ncol = fx[:4]
    nrow = len(rp) - 1
    srp, sci, sval = sh.stable_sorted(rp, ci, val)
    if len(fx) == 5:
        x = sh.x_of(nrow)
        y = sh.exact_product(rp, sh.fold(ci, nrow, fx[4]["send_idx"]), val, x)
    else:
        x = sh.x_of(ncol)
        y = sh.exact_product(rp, ci, val, x)
    out = (srp, sci, sval, y, x, sh.regimes(rp, ci, ncol))
    for a in out[:5]:
        a.setflags(write=False)
    return out


def to_dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


def create(ctx, name, path, val=None):
    rp, ci, v, ncol = sh.fixture(name)[:4]
    v = v if val is None else val
    if path == "device":
        return hip.Matrix.from_csr(ctx, to_dev(rp), to_dev(ci), to_dev(v), ncol=ncol)
    return hip.Matrix.from_csr(ctx, rp, ci, v, ncol=ncol)


def check_export(name, A, label=""):
    """export_csr equals the stably sorted input, info() the host sums, export_rows the same rows on ranges that cross
    slice boundaries"""
    srp, sci, sval, y, x, r = ref(name)
    nrow = len(srp) - 1
    inf = A.info()
    assert inf["nrow"] == nrow and inf["nnz"] == len(sci) and inf["nslices"] == len(r["width"]), (name, label)
    assert inf["stored"] == 64 * int(r["width"].sum()), (name, label)
    grp, gci, gv = A.export_csr()
    assert np.array_equal(grp, srp) and np.array_equal(gci, sci) and np.array_equal(gv, sval), (name, label)
    for b, n in ((0, 1), (60, 10), (63, 66), (nrow - 70, 70), (nrow - 1, 1), (64 * (len(r["width"]) // 2) - 3, 131)):
        b = min(max(b, 0), nrow - 1)
        n = min(n, nrow - b)
        qrp, qci, qv = A.export_rows(b, n)
        lo, hi = srp[b], srp[b + n]
        assert np.array_equal(qrp, srp[b:b + n + 1].astype(np.int64) - lo), (name, label, b)
        assert np.array_equal(qci, sci[lo:hi]) and np.array_equal(qv, sval[lo:hi]), (name, label, b)


def check(name, A, label=""):
    check_export(name, A, label)
    srp, sci, sval, y, x, r = ref(name)
    assert np.array_equal(A.spmv(np.array(x)), y), (name, label)


def device_product(ctx, A, xd, y):
    """isph_spmv on device vectors: the production dispatch (16-bit columns where the matrix has them)"""
    import torch
    hip._check(hip.lib().isph_spmv(ctx.h, A.h, hip._ptr(xd), hip._ptr(y), 1))
    torch.cuda.synchronize()


def all_variants(ctx, A, x, nrow):
    """[production, variant 0 .. 6] on device vectors, y allocated with a guard of 64 elements behind the rows; rows and
    guard pre-filled with a sentinel: every row is overwritten, the guard is not"""
    import torch
    xd = to_dev(x)
    out = []
    for variant in [None] + list(range(7)):
        y = torch.full((nrow + 64,), SENTINEL, dtype=torch.float64, device="cuda")
        if variant is None:
            device_product(ctx, A, xd, y)
        else:
            A.spmv_time(xd, y, reps=1, variant=variant)
            torch.cuda.synchronize()
        yh = y.cpu().numpy()
        assert np.all(yh[nrow:] == SENTINEL), variant                         # rows >= nrow are never written
        assert not np.any(yh[:nrow] == SENTINEL), variant
        out.append(yh[:nrow])
    return out


# ---------------------------------------------------------------- round trip and product, every family
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sh.WIDTH_FIXTURES)
def test_width_ladder_round_trip_and_product(gpu_ctx, name, path):
    """npair 0 .. 25 around every unroll boundary, all-empty slices between and behind, nrow % 64 in {0, 1, 63}, nrow in
    {1, 63, 64, 65}"""
    A = create(gpu_ctx, name, path)
    check(name, A, path)
    assert A.column_bits() == 16
    A.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sh.WINDOW_FIXTURES)
def test_window_ladder_round_trip_product_and_column_bits(gpu_ctx, name, path):
    """1 / 2 / 63 / 64 windows, a full table from one start slot, a chain that wraps past slot 63, offsets 0 and 1023,
    window numbers beyond 3000: 16-bit columns; 32-bit as soon as ONE slice has 65 windows.  window_pad65 PINS TODAY'S
    BEHAVIOUR: the 65th window of its slice comes from the padding column 0 of an empty row alone (no entry reads it),
    and the matrix still falls back to 32-bit columns.  window_rect has ghost columns and no plan: the plain kernel
    reads all ncol values from the caller."""
    A = create(gpu_ctx, name, path)
    check(name, A, path)
    r = ref(name)[5]
    if name != "window_rect":
        assert A.column_bits() == r["bits"] == {"window_le64": 16, "window_w65": 32, "window_pad65": 32}[name]
        check(name, A, path + " after the query")
    A.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sh.UNSORTED_FIXTURES)
def test_unsorted_rows_are_sorted_stably(gpu_ctx, name, path):
    """k_sell_sort_rows with R = 64 .. 1, rows of up to 1024 entries (16 trips of the rank loop), rows unsorted in the last
    pair only, duplicate columns with distinct values (position breaks the tie), one unsorted row in a ragged last slice.
    Rows of more than 16 entries with a duplicate column: the export's own re-sort used to exchange such ties."""
    A = create(gpu_ctx, name, path)
    check(name, A, path)
    assert A.column_bits() == 16
    check(name, A, path + " 16-bit")
    A.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sh.SLICES_FIXTURES)
def test_many_slices_through_the_scan(gpu_ctx, name, path):
    """k_exclusive_scan_ll (device-pointer path) over 1023 / 1024 / 1025 / 2049 slices with zero-width slices in between;
    the host path, whose offsets come from the host row pointers, as the control"""
    A = create(gpu_ctx, name, path)
    check(name, A, path)
    A.close()


# ---------------------------------------------------------------- all SpMV variants
@pytest.mark.parametrize("name", sh.WIDTH_FIXTURES + sh.SQUARE_WINDOW_FIXTURES)
def test_every_spmv_variant_gives_the_exact_product(gpu_ctx, name):
    """isph_spmv_time variants 0 .. 6 (the 32-bit kernel with UNROLL 8 / 8 / 4 / 12 / 2 / 6 / 4, with and without
    non-temporal loads) and the production dispatch of isph_spmv: all equal the integer product; rows >= nrow untouched"""
    srp, sci, sval, y, x, r = ref(name)
    A = create(gpu_ctx, name, "host")
    for k, got in enumerate(all_variants(gpu_ctx, A, x, len(srp) - 1)):
        assert np.array_equal(got, y), (name, k)
    A.close()


# ---------------------------------------------------------------- bits
@pytest.mark.parametrize("name", sh.WIDTH_FIXTURES + sh.WINDOW_FIXTURES)
def test_product_bits_follow_the_documented_order(gpu_ctx, name):
    """values N(0,1) 10^U(-3,3), x standard normal: the production product equals every variant and sell_shapes.emulate_spmv
    (acc0 over the even positions, acc1 over the odd ones, one fused multiply-add per entry, acc0 + acc1) BIT FOR BIT --
    the order the exact-iterate Krylov tests rely on"""
    rp, ci, _, ncol = sh.fixture(name)
    nrow = len(rp) - 1
    val, x = sh.random_values(name)
    A = create(gpu_ctx, name, "host", val=val)
    want = sh.emulate_spmv(rp, ci, val, x)
    if name == "window_rect":                                                  # no plan: isph_spmv_time refuses, one kernel
        got = [A.spmv(x)]
    else:
        got = all_variants(gpu_ctx, A, x, nrow)
        assert np.array_equal(got[0], A.spmv(x))
    for k, g in enumerate(got):
        assert np.array_equal(g, got[0]), (name, k)
    differ = np.flatnonzero(got[0] != want)
    print("\n%s: %d of %d rows differ from the emulation" % (name, len(differ), nrow))
    assert len(differ) == 0
    A.close()


# ---------------------------------------------------------------- host ingress
@pytest.mark.parametrize("variant", sh.CHUNKED_VARIANTS)
def test_chunked_ingress_modes_bytes_and_fused_paths(gpu_ctx, variant):
    """two chunks, a row across (or on) their boundary, chunk modes 16/16, 16/32 and 32/32 (a 16-bit chunk handing a row
    over to a 32-bit one), differences of 65535 / 65536, a row start far below the previous row's end behind an empty row,
    the first-column table exactly full and one row too long, an unsorted row in chunk 1: the bytes on the link are the
    host count, export and product exact through the plain ingress, the ingress fused with block ILU(0), the ingress with
    coordinates (rows renumbered by the library) and the gathered ingress with coordinates and ILU(0)"""
    name = "chunked_" + variant
    rp, ci, val, ncol = sh.fixture(name)
    nrow = len(rp) - 1
    r = ref(name)[5]
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    sent = hip.ingress_info(gpu_ctx)["link_bytes"]
    print("\n%s: link bytes %d, host count %d, modes %s" % (name, sent, r["link_bytes"], [c["mode"] for c in r["chunks"]]))
    assert sent == r["link_bytes"]
    check(name, A, "plain")
    assert A.column_bits() == 16
    check(name, A, "plain 16-bit")
    A.close()
    coords = np.random.default_rng(3).uniform(0.0, 1.0, (nrow, 3))
    if np.any(np.diff(rp) == 0):
        # block ILU(0) is undefined for a row without a diagonal: the fused set-ups refuse these matrices, loudly (the *_diag
        # variants carry the same chunk shapes through them); the context goes on working
        for fused in (lambda: hip.Matrix.from_host_csr_with_bjacobi(gpu_ctx, rp, ci, val),
                      lambda: hip.Matrix.from_host_csr_with_coords(gpu_ctx, rp, ci, val, coords, with_bjacobi=True)):
            with pytest.raises(hip.IsphError, match="without a diagonal"):
                fused()
    else:
        A, M = hip.Matrix.from_host_csr_with_bjacobi(gpu_ctx, rp, ci, val)
        assert hip.ingress_info(gpu_ctx)["link_bytes"] == r["link_bytes"]
        check(name, A, "bjacobi")
        assert A.column_bits() == 16                                           # (unsorted_chunk1: rebuilt on first use)
        M.close(); A.close()
        A, M = hip.Matrix.from_host_csr_with_coords(gpu_ctx, rp, ci, val, coords, with_bjacobi=True)
        check(name, A, "coords + bjacobi")
        M.close(); A.close()
    A = hip.Matrix.from_host_csr_with_coords(gpu_ctx, rp, ci, val, coords)
    assert hip.ingress_info(gpu_ctx)["link_bytes"] == r["link_bytes"]
    check(name, A, "coords")
    A.close()


# ---------------------------------------------------------------- halo: the LIST / GHOST instantiations
@pytest.mark.parametrize("variant", sh.HALO_VARIANTS)
def test_self_halo_product_equals_the_folded_matrix(variant):
    """interior (LIST) and boundary (LIST + GHOST) launches through the self-peer plan: both lists, no interior slice, no
    boundary slice, with 16-bit columns and (fallback) with 32-bit columns; host- and device-pointer path"""
    import torch
    assert torch.cuda.is_available()
    name = "halo_" + variant
    rp, ci, val, ncol, plan = sh.fixture(name)
    srp, sci, sval, y, x, r = ref(name)
    ctx = hip.Context(0, rank=0, nranks=1, uid=hip.Context.unique_id())
    try:
        for path in PATHS:
            A = create(ctx, name, path)
            A.set_halo(plan["peers"], plan["send_ptr"], plan["send_idx"], plan["recv_ptr"])
            check_export(name, A, path)
            assert np.array_equal(A.spmv(np.array(x)), y), path
            assert A.column_bits() == r["bits"] == (32 if variant == "fallback" else 16)
            assert np.array_equal(A.spmv(np.array(x)), y), path
            A.close()
    finally:
        ctx.close()
