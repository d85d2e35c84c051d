"""-m "not gpu": the constructed matrices of tests/sell_shapes.py land on the branches they claim, their exact references
hold what they promise, and the comparisons of tests/test_gpu_sell_shapes.py would see a wrong kernel.  No GPU, no oracle.

Where each family lands according to sell_shapes.regimes() (which restates csrc/sell.hpp and csrc/ingress.hpp; the kernels
are the authority):

  width_tail0/1/63   18 slices of npair 1 2 3 4 5 7 8 9 0 11 12 13 15 16 17 24 25 0 (+ a ragged slice of npair 3): the main
                     loops of UNROLL 2 / 4 / 6 / 8 / 12 run 0, 1 and several trips with tails of 0 .. 11 pairs; all-empty
                     slices between and behind non-empty ones; nrow % 64 = 0, 1, 63; two windows, 16-bit columns
  tiny1/63/64/65     nrow below, one short of, equal to and one beyond a slice
  window_le64        slices of 1, 2, 63, 64 windows; 64 windows on one start slot (probe chains up to 63 steps, wrapping);
                     a 7-window chain from slots 62 / 63 into 0 .. 4; 64 windows with window 0 and an empty row (padding adds
                     nothing); the last of 49 888 slices reads the last column: 16-bit
  window_w65         + one slice of 65 windows: 32-bit
  window_pad65       + one slice of 64 entry windows and an empty row whose padding column 0 is the 65th: 32-bit
  window_rect        ncol > nrow without a plan: the plain 32-bit kernel on all ncol values
  unsorted<w>        widest slice w = 2 30 | 32 62 | 64 66 | 128 130 | 256 | 512 | 1024  ->  R = 64 | 32 | 16 | 8 | 4 | 2 | 1;
                     1 .. 16 trips of the rank loop; shuffled rows, rows unsorted in the last pair only, duplicate columns
  unsorted_ragged    one unsorted row, in the ragged last slice
  chunked_*          two chunks of 524 288 + 35 712 entries, a row across the boundary at offset 2 (row_on_boundary: a row
                     that starts on it); modes 16/16 (narrow, d65535, row_start_back, table_fits), 16/32 (d65536_chunk1,
                     unsorted_chunk1, table_too_long), 32/32 (d65536_chunk0); the *_diag variants replace the empty rows by
                     rows that hold their diagonal alone, for the ingress fused with block ILU(0).  With two chunks a 32-bit chunk in FRONT of a
                     16-bit one cannot occur (chunk 0 decides for the matrix): the hand-over inside a row is 16 -> 32 only
  slices1023..2049   1, 1, 2 and 3 trips of the scan's block, every fifth slice of width 0
  halo_*             interior and boundary slice lists: both, boundary only, interior only; 16-bit and (fallback: 66
                     windows in a boundary slice) 32-bit columns
"""
import numpy as np
import pytest

import sell_shapes as sh

LD = np.longdouble


def reg(name):
    rp, ci, val, ncol = sh.fixture(name)[:4]
    return sh.regimes(rp, ci, ncol)


# ---------------------------------------------------------------- 1. every generator lands where it claims
def test_values_are_integers_in_range_and_shapes_are_consistent():
    for name in sh.FIXTURES:
        rp, ci, val, ncol = sh.fixture(name)[:4]
        nrow = len(rp) - 1
        assert rp[0] == 0 and np.all(np.diff(rp) >= 0) and rp[-1] == len(ci) == len(val) and len(ci) > 0, name
        assert ci.min() >= 0 and ci.max() < ncol and ncol >= nrow, name
        assert np.all(val == np.round(val)) and np.all(val != 0) and np.abs(val).max() <= 1000, name
        assert np.diff(rp).max() <= 1024 and len(ci) <= 560000, name
    x = sh.x_of(1 << 16)
    assert np.all(x % 2 == 1) and x.max() < 2 ** 20 and len(np.unique(x)) > 60000


@pytest.mark.parametrize("tail", [0, 1, 63])
def test_width_ladder_places_npair_on_the_unroll_boundaries(tail):
    rp, ci, val, ncol = sh.fixture("width_tail%d" % tail)
    r = reg("width_tail%d" % tail)
    nrow = len(rp) - 1
    assert nrow % 64 == tail and ncol == nrow
    want = [2 * p for p in sh.NPAIRS] + ([6] if tail else [])
    assert list(r["width"]) == want
    npair = set(r["width"] // 2)
    for u in (2, 4, 6, 8, 12):       # one pair below and above a trip of every unrolled main loop, whole trips, two trips
        assert {u - 1, u + 1} <= npair and any(p and p % u == 0 for p in npair) and any(p >= 2 * u for p in npair), u
        assert {p % u for p in npair} >= {0, 1, u - 1}, u
    assert r["width"][8] == 0 and r["width"][7] > 0 and r["width"][9] > 0          # an empty slice between non-empty ones
    assert r["width"][17] == 0 and (tail == 0) == (r["width"][-1] == 0)
    lens = np.diff(rp)
    for s, w in enumerate(r["width"][:18]):
        got = set(lens[64 * s:64 * s + 64])
        assert got == ({0, 1, min(w - 1, (w // 2) | 1), w - 1, w} if w else {0}), s
    assert r["bits"] == 16 and r["windows"].max() <= 2 and not np.all(np.diff(ci) > 0)
    assert np.array_equal(sh.stable_sorted(rp, ci, val)[1], ci)                     # rows arrive sorted


@pytest.mark.parametrize("nrow", [1, 63, 64, 65])
def test_tiny_matrices(nrow):
    rp, ci, val, ncol = sh.fixture("tiny%d" % nrow)
    r = reg("tiny%d" % nrow)
    assert len(rp) - 1 == nrow == ncol and len(r["width"]) == (nrow + 63) // 64 and r["width"].min() >= 2 and r["bits"] == 16


def test_window_ladder_counts_and_table_shapes():
    nw, by_slot = sh._window_pool()
    assert max(len(b) for b in by_slot) == 64 and nw * 1024 < 5_000_000
    # the host restatement of amg_like_hash against values worked out by hand from its definition in csrc/sell.hpp
    assert int(sh.window_slot(0)) == 0
    for w in (1, 2, 1000, 2 ** 21):
        h = w
        h ^= h >> 16; h = (h * 0x7feb352d) & 0xFFFFFFFF; h ^= h >> 15; h = (h * 0x846ca68b) & 0xFFFFFFFF; h ^= h >> 16
        assert int(sh.window_slot(w)) == h & 63
    base = [1, 2, 63, 64, 64, 7, 64]
    for name, extra_e, extra_w, bits in (("window_le64", [], [], 16), ("window_w65", [65], [65], 32),
                                         ("window_pad65", [64], [65], 32)):
        rp, ci, val, ncol = sh.fixture(name)
        r = reg(name)
        k = len(base + extra_e)
        assert ncol == len(rp) - 1 == nw * 1024 and len(r["width"]) == nw * 16
        assert list(r["entry_windows"][:k]) == base + extra_e and list(r["windows"][:k]) == base + extra_w
        assert r["width"][k:-1].max() == 0 and r["windows"][-1] == 2 and r["bits"] == bits
        assert ci.max() == ncol - 1 and ci.max() // 1024 == nw - 1 and np.all(r["width"][:k] == 4)
        off = ci % 1024
        assert (off == 0).sum() > 100 and (off == 1023).sum() > 100
        win = lambda s: np.unique(ci[rp[64 * s]:rp[64 * s + 64]] // 1024)
        assert len(set(sh.window_slot(win(4)))) == 1                                # a full table from ONE start slot
        slots = sorted(sh.window_slot(win(5)))
        assert slots == [0, 1, 62, 62, 63, 63, 63]                                  # three windows pushed past slot 63
        assert 0 in win(6) and np.diff(rp)[64 * 6 + 5] == 0                         # padding column 0 inside the table
        if name == "window_pad65":
            assert 0 not in win(7) and np.diff(rp)[64 * 7 + 5] == 0                 # ... and as the 65th window
    rp, ci, val, ncol = sh.fixture("window_rect")
    r = reg("window_rect")
    assert len(rp) - 1 == 512 < ncol == nw * 1024 and list(r["windows"]) == base + [65]


@pytest.mark.parametrize("w", sh.SORT_WIDTHS)
def test_unsorted_ladder_reaches_every_R(w):
    rp, ci, val, ncol = sh.fixture("unsorted%d" % w)
    r = reg("unsorted%d" % w)
    assert r["width"].max() == r["width"][0] == w and r["sort_R"] == sh.SORT_R[w] and ncol == len(rp) - 1
    assert r["sort_trips"][0] == (w + 63) // 64 and r["bits"] == 16
    # the thresholds themselves: R * (wmax | 1) * 24 bytes within 48 KiB
    assert r["sort_R"] * (w | 1) * 24 <= 48 * 1024 and (r["sort_R"] == 64 or 2 * r["sort_R"] * (w | 1) * 24 > 48 * 1024)
    srp, sci, sval = sh.stable_sorted(rp, ci, val)
    lens = np.diff(rp)
    kinds = dict(sorted=0, last_pair=0, shuffled=0, dup=0)
    for i in range(len(rp) - 1):
        a, b = ci[rp[i]:rp[i + 1]], sci[rp[i]:rp[i + 1]]
        if len(a) >= 2 and np.any(np.diff(b) == 0):
            kinds["dup"] += 1
            q = np.flatnonzero(np.diff(b) == 0)[0]
            assert sval[rp[i] + q] != sval[rp[i] + q + 1]                           # a tie the wrong way round would show
        if np.array_equal(a, b):
            kinds["sorted"] += 1
        elif np.array_equal(a[:-2], b[:-2]):
            kinds["last_pair"] += 1
        else:
            kinds["shuffled"] += 1
    assert min(kinds.values()) >= (1 if w == 2 else 5) or (w == 2 and kinds["dup"] == 0), kinds
    assert lens.max() == w


def test_unsorted_ragged_has_one_unsorted_row_in_the_last_slice():
    rp, ci, val, ncol = sh.fixture("unsorted_ragged")
    nrow = len(rp) - 1
    bad = [i for i in range(nrow) if np.any(np.diff(ci[rp[i]:rp[i + 1]]) < 0)]
    assert nrow % 64 == 59 and bad == [sh.ragged_row(nrow)] and bad[0] >= nrow - 59


CHUNK_MODES = dict(narrow=(16, 16), d65535=(16, 16), d65536_chunk1=(16, 32), d65536_chunk0=(32, 32), row_start_back=(16, 16),
                   row_on_boundary=(16, 16), unsorted_chunk1=(16, 32), table_fits=(16, 16), table_too_long=(16, 32),
                   row_start_back_diag=(16, 16), table_fits_diag=(16, 16), table_too_long_diag=(16, 32))


@pytest.mark.parametrize("variant", sh.CHUNKED_VARIANTS)
def test_chunked_variants_have_the_intended_modes_and_bytes(variant):
    rp, ci, val, ncol = sh.fixture("chunked_" + variant)
    r = reg("chunked_" + variant)
    nrow = len(rp) - 1
    ch = r["chunks"]
    assert len(ci) == 560000 and [c["entries"] for c in ch] == [524288, 35712]
    assert tuple(c["mode"] for c in ch) == CHUNK_MODES[variant]
    for c in ch:
        assert c["bytes"] == (12 * c["entries"] if c["mode"] == 32 else ((10 * c["entries"] + 3) & ~3) + 4 * c["rows"])
    assert r["link_bytes"] == ch[0]["bytes"] + ch[1]["bytes"] + 4 * (nrow + 1)
    d = np.diff(ci.astype(np.int64))
    inside = np.ones(len(d), dtype=bool)
    inside[rp[1:-1][(rp[1:-1] > 0) & (rp[1:-1] < len(ci))] - 1] = False             # differences across a row start
    if variant == "row_on_boundary":
        assert r["straddlers"] == [None] and 524288 in rp and ch[0]["rows"] + ch[1]["rows"] == nrow
    elif variant.startswith("row_start_back"):
        assert r["straddlers"] == [(sh.STRADDLER + 1, 2)]
    else:
        assert r["straddlers"] == [(sh.STRADDLER, 2)]
    if variant == "d65535":
        assert d[inside].max() == 65535
    if variant.startswith("d65536"):
        q = int(np.flatnonzero(inside & (d == 65536))[0]) + 1
        assert d[inside].max() == 65536 and (q >= 524288) == (variant == "d65536_chunk1")
        assert [c["wide"] for c in ch] == ([0, 1] if variant == "d65536_chunk1" else [1, 0])
    if variant.startswith("row_start_back"):
        i = 72002
        assert rp[i] - rp[i - 1] == variant.endswith("_diag") and ci[rp[i - 1] - 1] - ci[rp[i]] > 65535
        assert d[inside].max() == 40000 and d[inside].min() > 0
    if variant == "unsorted_chunk1":
        assert d[inside].min() < 0 and [c["wide"] for c in ch] == [0, 1]
    if variant.startswith("table_"):
        assert ch[1]["rows"] == sh.TABLE_ROWS_FIT + variant.startswith("table_too_long") and d[inside].max() == 1
        lim = 12 * 35712 - ((10 * 35712 + 3) & ~3)
        assert 4 * sh.TABLE_ROWS_FIT <= lim < 4 * (sh.TABLE_ROWS_FIT + 1)
    # block ILU(0) of the fused ingress needs a dominant diagonal
    rows = sh.row_index(rp)
    diag = np.zeros(nrow)
    diag[rows[ci == rows]] = np.abs(val[ci == rows])
    off = np.bincount(rows, weights=np.abs(val) * (ci != rows), minlength=nrow)
    assert np.all(diag[np.diff(rp) > 0] > off[np.diff(rp) > 0])
    assert np.any(np.diff(rp) == 0) == (variant in ("row_start_back", "table_fits", "table_too_long"))


@pytest.mark.parametrize("ns", sh.MANY_SLICES)
def test_many_slices_cross_the_scan_block(ns):
    r = reg("slices%d" % ns)
    w = r["width"]
    assert len(w) == ns and r["scan_trips"] == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[ns]
    assert {0, 4} <= set(w) <= {0, 2, 4} and np.all(w[2::5][:-1] == 0) and w[-1] > 0
    zero = np.flatnonzero(w == 0)
    assert np.any(w[zero[zero > 0] - 1] > 0) and np.any(w[zero[zero < ns - 1] + 1] > 0)   # zero-width slices in between


@pytest.mark.parametrize("variant", sh.HALO_VARIANTS)
def test_self_halo_slices(variant):
    rp, ci, val, ncol, plan = sh.fixture("halo_" + variant)
    nrow = len(rp) - 1
    ns = (nrow + 63) // 64
    ghost = np.zeros(ns, dtype=bool)
    ghost[(sh.row_index(rp)[ci >= nrow]) // 64] = True
    want = dict(mixed=[1, 3, 4], no_interior=list(range(ns)), no_boundary=[], fallback=[1, 2, ns - 1])[variant]
    assert list(np.flatnonzero(ghost)) == want and ncol - nrow == 40 == plan["recv_ptr"][-1] == len(plan["send_idx"])
    assert len(np.unique(plan["send_idx"])) == 40 and plan["send_idx"].max() < nrow
    r = sh.regimes(rp, ci, ncol)
    assert r["bits"] == (32 if variant == "fallback" else 16) and (variant != "fallback" or r["windows"][2] == 66)
    f = sh.fold(ci, nrow, plan["send_idx"])
    assert f.max() < nrow and np.array_equal(f[ci < nrow], ci[ci < nrow])
    assert np.array_equal(f[ci >= nrow], plan["send_idx"][ci[ci >= nrow] - nrow])


# ---------------------------------------------------------------- 2. the emulation of the kernels' order
def test_emulation_stays_within_the_derived_bound_of_the_long_double_product():
    """per row |emulation - long double| <= (len / 2 + 2) 2^-53 sum|a||x|: each accumulator takes len / 2 fused steps of one
    rounding each, one more for acc0 + acc1, one for the rounding of the long-double reference to double"""
    for name in ("width_tail63", "window_w65"):
        rp, ci, _, ncol = sh.fixture(name)
        val, x = sh.random_values(name)
        y = sh.emulate_spmv(rp, ci, val, x)
        rows = sh.row_index(rp)
        nrow = len(rp) - 1
        yl = np.zeros(nrow, dtype=LD)
        np.add.at(yl, rows, val.astype(LD) * x[ci].astype(LD))
        mag = np.bincount(rows, weights=np.abs(val * x[ci]), minlength=nrow)
        bound = (np.diff(rp) / 2 + 2) * 2.0 ** -53 * mag
        assert np.all(np.abs(y.astype(LD) - yl) <= bound.astype(LD))
        assert np.any(y != sh.unfused_spmv(rp, ci, val, x))         # the fused order is not the rounded-product order
        assert np.array_equal(sh.emulate_spmv(rp, ci, sh.fixture(name)[2], sh.x_of(ncol)),
                              sh.exact_product(rp, ci, sh.fixture(name)[2], ncol=ncol))


def test_emulation_differs_from_the_unfused_sum_on_a_row_with_cancellation():
    """positions 0 and 2 share acc0: 1 * 1, then (1 + 2^-30) * -(1 - 2^-30) = -(1 - 2^-60): fused 2^-60, unfused 0"""
    rp, ci = np.array([0, 3]), np.array([0, 1, 2])
    val = np.array([1.0, 0.0, 1.0 + 2.0 ** -30])
    x = np.array([1.0, 5.0, -(1.0 - 2.0 ** -30)])
    assert sh.emulate_spmv(rp, ci, val, x)[0] == 2.0 ** -60 and sh.unfused_spmv(rp, ci, val, x)[0] == 0.0


# ---------------------------------------------------------------- 3. detection power
@pytest.mark.parametrize("family", sorted(sh.FAMILIES))
def test_every_mutation_changes_the_product_or_the_export(family):
    """what a subtly wrong kernel would do to one row -- two columns swapped, the last entry lost, a column off by one or
    by one window, an entry in the next row -- applied to the HOST reference of one fixture per family: the exact product
    (what spmv is compared with) or the sorted CSR (what the exports are compared with) must differ.  A column defect
    inside the 16-bit copy shows in the product alone, so the column mutations must change the product."""
    name = dict(width="width_tail63", window="window_w65", unsorted="unsorted66", chunked="chunked_d65536_chunk1",
                slices="slices1025", halo="halo_fallback")[family]
    fx = sh.fixture(name)
    ncol = fx[3]
    rp, ci, val = sh.stable_sorted(*fx[:3])
    nrow = len(rp) - 1
    cols = (lambda c: sh.fold(c, nrow, fx[4]["send_idx"])) if family == "halo" else (lambda c: c)
    x = sh.x_of(ncol)
    y = sh.exact_product(rp, cols(ci), val, x)
    for kind in sh.MUTATIONS:
        for seed in range(3):
            mrp, mci, mval = sh.mutate(rp, ci, val, ncol, kind, seed)
            product = not np.array_equal(sh.exact_product(mrp, cols(mci), mval, x), y)
            export = not (np.array_equal(mrp, rp) and np.array_equal(mci, ci) and np.array_equal(mval, val))
            assert product or export, (kind, seed)
            assert export, (kind, seed)
            if kind in ("swap_columns", "shift_1", "shift_1024", "drop_last", "next_row"):
                assert product, (kind, seed)


# ---------------------------------------------------------------- 4. exactness
def test_partial_sums_stay_exact_for_every_generator():
    for name in sh.FIXTURES:
        rp, ci, val, ncol = sh.fixture(name)[:4]
        assert sh.max_partial_sum(rp, ci, val, ncol) < 2.0 ** 41 < 2.0 ** 53, name
