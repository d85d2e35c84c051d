"""Constructed matrices for the branches of the sliced-ELL layer (csrc/sell.hpp: conversion, row sort, 16-bit column windows,
SpMV kernels) and of the chunked host ingress (csrc/ingress.hpp), exact references, and a classifier that restates the
thresholds of the two files on a CSR.

Host only: numpy, no GPU, no SPH, nothing from oracle/.  The SPH matrices of the other suites have sorted rows of 30-90
entries whose slices touch a few dozen column windows: they land on whichever branch the lattice gives.  The generators
here place slices ON the thresholds by design, each with the smallest shape that still reaches its branch.

Values are exact by construction: matrix entries are non-zero integers in [-1000, 1000], x[c] = fingerprint(c) is an odd
integer below 2^20, rows hold at most 1024 entries, so every partial sum of a row stays below 2^10 * 2^10 * 2^20 = 2^40 in
magnitude and every summation order gives the same double.  Products and exports are compared with np.array_equal; there
is no tolerance to choose.  (A misplaced entry, a column off by one or by a window, an entry in the wrong row all change
the product: tests/test_sell_shapes_host.py applies those mutations to the host data and checks that they show.)

What a branch depends on (restated in regimes(); the kernels are the authority, a change that moves a threshold there
updates regimes()):
  * a slice is 64 rows; its width is the longest row rounded up to even, npair = width / 2 is the trip count of the SpMV
    loops (main loop UNROLL pairs at a time, tail loop one pair at a time);
  * padding positions store value 0 and the row's first column AS IT ARRIVED (0 for a row without entries and for the
    rows of the last slice beyond nrow), so padding can add window 0 to a slice;
  * k_sell_compress_cols: a slice that touches at most 64 windows of 1024 columns (padding included) gets a 64-slot table,
    open addressing from amg_like_hash(window) & 63 with linear probing; one slice with 65 sends the whole matrix to the
    32-bit kernel;
  * sell_sort_rows: ONE R per launch from the matrix' widest slice (Ws = wmax | 1, R halved from 64 while R * Ws * 24 bytes
    exceed 48 KiB); the rank loop of a row takes ceil(width / 64) trips;
  * csr_ingress_host: the first chunk holds 524288 entries, the following ones 4194304; a chunk travels with 16-bit column
    differences (10 bytes per entry + a table of first columns, 4 bytes per row that starts in it) when the table fits
    into the 12 bytes per entry of its slot, chunk 0 said yes, and no difference inside a row lies outside [0, 65535];
    else with 32-bit columns (12 bytes per entry);
  * k_exclusive_scan_ll: one block of 1024 threads, the carry crosses a trip of the block beyond 1024 slices.
"""
import fractions
import functools

import numpy as np

SLICE = 64
WINDOW = 1024
FIRST_CHUNK = 524288          # HostStager::kChunk / 8
CHUNK = 4194304               # HostStager::kChunk
MAX_CHUNKS = 512              # 64 * kModeWords: more chunks travel with 32-bit columns
SCAN_BLOCK = 1024             # threads of the single block of k_exclusive_scan_ll


# ---------------------------------------------------------------- values
def fingerprint(c):
    """x[c]: an odd integer below 2^20 from a multiplicative hash of the column"""
    c = np.asarray(c, dtype=np.uint64)
    return ((((c * np.uint64(2654435761)) >> np.uint64(11)) & np.uint64(0xFFFFF)) | np.uint64(1)).astype(np.float64)


def x_of(ncol):
    return fingerprint(np.arange(ncol))


def _ints(rng, n, top=1000):
    return (rng.integers(1, top + 1, size=n) * rng.choice([-1, 1], size=n)).astype(np.float64)


def _distinct_ints(rng, n):
    """n <= 2000 distinct non-zero integers in [-1000, 1000]"""
    pool = np.concatenate([np.arange(-1000, 0), np.arange(1, 1001)])
    return rng.choice(pool, size=n, replace=False).astype(np.float64)


def _csr(rows, rng, vals=None):
    """CSR of a list of column arrays (in the order given)"""
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows])
    ci = (np.concatenate(rows) if len(rows) and rp[-1] else np.zeros(0)).astype(np.int32)
    val = _ints(rng, len(ci)) if vals is None else np.concatenate(vals).astype(np.float64)
    return rp, ci, val


def window_slot(w):
    """host restatement of amg_like_hash(w) & 63 (csrc/sell.hpp): the slot at which the probing for window w starts"""
    m = np.uint64(0xFFFFFFFF)
    h = np.asarray(w, dtype=np.uint64) & m
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7feb352d)) & m
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846ca68b)) & m
    h = h ^ (h >> np.uint64(16))
    return (h & np.uint64(63)).astype(np.int64)


# ---------------------------------------------------------------- width ladder: SpMV main and tail loops
NPAIRS = [1, 2, 3, 4, 5, 7, 8, 9, 0, 11, 12, 13, 15, 16, 17, 24, 25, 0]   # one slice each; 0: an all-empty slice


def _cycle_lengths(w, n=SLICE):
    """row lengths of a slice of width w: 0, 1, an odd one, w - 1, w, cyclically"""
    if w == 0:
        return [0] * n
    cyc = [0, 1, min(w - 1, (w // 2) | 1), w - 1, w]
    return [cyc[j % 5] for j in range(n)]


def width_ladder(tail=0, seed=11):
    """One slice per npair of NPAIRS (npair on and around the multiples of 2, 4, 6, 8 and 12 the SpMV variants unroll by), an
    all-empty slice in the middle and one at the end, then `tail` rows (0, 1 or 63) of a ragged last slice."""
    rng = np.random.default_rng(seed)
    lens = []
    for p in NPAIRS:
        lens += _cycle_lengths(2 * p)
    lens += [(5, 0, 3, 6, 1)[j % 5] for j in range(tail)]
    n = len(lens)
    rows = [np.sort(rng.choice(n, size=m, replace=False)) for m in lens]
    return _csr(rows, rng) + (n,)


def tiny(nrow, seed=12):
    """nrow in {1, 63, 64, 65}: less than a slice, one row short of it, exactly one, one row more"""
    rng = np.random.default_rng(seed)
    lens = [min(nrow, 1 + (5 * i) % 9) for i in range(nrow)]
    rows = [np.sort(rng.choice(nrow, size=m, replace=False)) for m in lens]
    return _csr(rows, rng) + (nrow,)


# ---------------------------------------------------------------- window ladder: the 64-slot table of a slice
@functools.lru_cache(maxsize=None)
def _window_pool():
    """(NW, windows by start slot): NW is the smallest number of windows among which 64 share one start slot"""
    count = np.zeros(64, dtype=np.int64)
    nw = 0
    while count.max() < 64:
        count[int(window_slot(nw))] += 1
        nw += 1
    slots = window_slot(np.arange(nw))
    return nw, [np.flatnonzero(slots == s) for s in range(64)]


def _window_rows(wins, rng, empty_row=None):
    """64 rows over the windows `wins` (k <= 65): row j reads the windows j, j + 21 and j + 42 (mod k), so every window is
    read; the offsets inside a window cycle through 0, 1023 and a random one.  Row `empty_row` has no entries."""
    wins = np.asarray(wins, dtype=np.int64)
    k = len(wins)
    rows = []
    for j in range(SLICE):
        if j == empty_row:
            rows.append(np.zeros(0, dtype=np.int64))
            continue
        w = wins[[j % k, (j + 21) % k, (j + 42) % k]]
        off = np.array([(0, WINDOW - 1, int(rng.integers(1, WINDOW - 1)))[(j + i) % 3] for i in range(3)])
        rows.append(np.unique(w * WINDOW + off))
    return rows


WINDOW_VARIANTS = ("le64", "w65", "pad65", "rect")


def window_ladder(variant="le64", seed=13):
    """Slices that touch exactly 1, 2, 63 and 64 windows, 64 windows that all start probing at ONE slot (a full table with
    the longest probe chains, wrapping past slot 63), a short chain that wraps from slot 63 to slot 0, and 64 windows with
    window 0 among them and an empty row (the padding column 0 adds nothing).  Columns at offsets 0 and 1023 of their
    windows; window numbers up to NW - 1 (the hash decides NW = 3118, ncol = 1024 NW); the last slice of the matrix
    reads the last column.
      le64 : the above; every slice within 64 windows
      w65  : + a slice that touches 65 windows
      pad65: + a slice whose entries touch 64 windows, none of them window 0, with one empty row: the padding column 0 is
             the 65th
      rect : the first 8 slices of w65 as a rectangular operator (ncol > nrow, no halo plan)"""
    assert variant in WINDOW_VARIANTS
    rng = np.random.default_rng(seed)
    nw, by_slot = _window_pool()
    full = int(np.argmax([len(b) for b in by_slot]))
    pick = lambda k, lo=1: np.sort(rng.choice(np.arange(lo, nw), size=k, replace=False))
    wrap = np.concatenate([by_slot[62][:2], by_slot[63][:3], by_slot[0][1:2], by_slot[1][:1]])
    with0 = np.concatenate([[0], pick(63)])
    content = [_window_rows([7], rng), _window_rows([3, nw - 1], rng), _window_rows(pick(63), rng), _window_rows(pick(64), rng),
               _window_rows(by_slot[full][:64], rng), _window_rows(wrap, rng), _window_rows(with0, rng, empty_row=5)]
    if variant in ("w65", "rect"):
        content.append(_window_rows(pick(65), rng))
    if variant == "pad65":
        content.append(_window_rows(pick(64), rng, empty_row=5))
    ncol = nw * WINDOW
    rows = [r for sl in content for r in sl]
    if variant == "rect":
        return _csr(rows, rng) + (ncol,)
    nrow = ncol
    last = _window_rows([nw - 1, 0], rng)
    head, tail = _csr(rows, rng), _csr(last, rng)
    lens = np.zeros(nrow, dtype=np.int64)
    lens[:len(rows)] = np.diff(head[0])
    lens[nrow - SLICE:] = np.diff(tail[0])
    rp = np.zeros(nrow + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    return rp, np.concatenate([head[1], tail[1]]), np.concatenate([head[2], tail[2]]), ncol


# ---------------------------------------------------------------- unsorted ladder: the LDS row sort
SORT_WIDTHS = (2, 30, 32, 62, 64, 66, 128, 130, 256, 512, 1024)
SORT_R = {2: 64, 30: 64, 32: 32, 62: 32, 64: 16, 66: 16, 128: 8, 130: 8, 256: 4, 512: 2, 1024: 1}
UNSORTED_NROW = 19 * SLICE


def ragged_row(nrow):
    """the one unsorted row of the ragged variant: the last row of full length"""
    return (nrow - 1) // 6 * 6


def unsorted_ladder(w, ragged=False, seed=14):
    """A square matrix of 19 slices whose widest slice is w (the host picks the sort's R from it): slices of width w, 2 and
    about w / 2, the others with rows of at most 4 entries.  Rows cycle through: shuffled; sorted but for the last pair;
    sorted; shuffled with two duplicate columns (distinct values: ties are broken by position).
    ragged: every row sorted except ONE in the last slice, which has 59 rows."""
    rng = np.random.default_rng(seed + w)
    nrow = UNSORTED_NROW - (5 if ragged else 0)
    widths = [w, 2, max(2, (w // 2 + 1) & ~1)] + [min(w, 4)] * 16
    rows, vals = [], []
    for i in range(nrow):
        ww = widths[i // SLICE]
        m = (ww, ww - 1, 1, 0, min(ww, 3), ww // 2 + 1)[i % 6]
        mode = i % 4
        if m >= 4 and mode == 3:
            c = np.sort(rng.choice(nrow, size=m - 2, replace=False))
            c = np.sort(np.concatenate([c, c[[0, len(c) // 2]]]))
        else:
            c = np.sort(rng.choice(nrow, size=m, replace=False))
        if ragged:
            if i == ragged_row(nrow):
                c = c[::-1].copy()
        elif mode in (0, 3) and m >= 2:
            c = rng.permutation(c)
        elif mode == 1 and m >= 2:
            c[[-1, -2]] = c[[-2, -1]]
        rows.append(c)
        vals.append(_distinct_ints(rng, m))
    return _csr(rows, rng, vals) + (nrow,)


# ---------------------------------------------------------------- chunked: the host ingress
CHUNKED_ROWS = 80000
CHUNKED_VARIANTS = ("narrow", "d65535", "d65536_chunk1", "d65536_chunk0", "row_start_back", "row_on_boundary", "unsorted_chunk1",
                    "table_fits", "table_too_long", "row_start_back_diag", "table_fits_diag", "table_too_long_diag")
STRADDLER = 74898            # 7 * 74898 = 524286: the row holds the entries 524286 .. 524292
TABLE_ROWS_FIT = 17856       # chunk 1 holds 35712 entries: 357120 + 4 rows <= 428544  <=>  rows <= 17856


def _band(lens, rng):
    """rows of consecutive columns around the diagonal (position 3 where the row is long enough and away from the ends);
    diagonal +-1000, the others +-[1, 100]: strictly diagonally dominant, so block ILU(0) of it exists"""
    n = len(lens)
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    r = np.repeat(np.arange(n), lens)
    start = np.clip(np.arange(n) - np.minimum(3, np.maximum(lens, 1) - 1), 0, n - np.maximum(lens, 1))
    ci = start[r] + (np.arange(rp[-1]) - rp[r])
    val = _ints(rng, len(ci), top=100)
    d = ci == r
    val[d] = 1000.0 * rng.choice([-1, 1], size=int(d.sum()))
    return rp.astype(np.int32), ci.astype(np.int32), val


def chunked(variant="narrow", seed=15):
    """560 000 entries in two chunks (524 288 + 35 712), 80 000 rows of 7; row 74 898 holds entries 524 286 .. 524 292 and
    so straddles the chunk boundary at its offset 2.  Variants:
      narrow          every difference inside a row is 1: both chunks with 16-bit differences
      d65535          one difference of exactly 65535 (row 70 000): still 16-bit
      d65536_chunk1   one difference of 65536 in chunk 1 (row 77 000): chunk 0 16-bit, chunk 1 32-bit; the straddling row
                      changes mode at its third entry
      d65536_chunk0   one difference of 65536 in chunk 0 (row 70 000): chunk 0 decides for the matrix, both 32-bit
      row_start_back  row 72 001 starts 70 000 columns below the end of row 72 000, an EMPTY row in between, differences of
                      40 000 and 30 000 inside the row: nothing is wide (a row start is not a difference), both 16-bit
      row_on_boundary two early rows of 8 entries (and two late ones of 6): row 74 898 starts exactly on entry 524 288
      unsorted_chunk1 one row of chunk 1 (78 000) with two entries swapped: chunk 1 32-bit, the matrix is sorted afterwards
      table_fits      12 755 empty rows between the rows of chunk 1: 17 856 rows start in it, the most whose first columns
                      fit behind the 16-bit differences
      table_too_long  one more empty row: chunk 1 travels with 32-bit columns
      *_diag          the same three with rows that hold their diagonal alone where the others have empty rows (block ILU(0),
                      which the fused ingress sets up, is undefined for a row without a diagonal); the table variants reach
                      17 856 / 17 857 row starts on the same 35 712 entries with 2975 rows of 7 entries between them"""
    assert variant in CHUNKED_VARIANTS
    rng = np.random.default_rng(seed)
    lens = np.full(CHUNKED_ROWS, 7, dtype=np.int64)
    if variant == "row_on_boundary":
        lens[[10, 20]] = 8
        lens[[79000, 79010]] = 6
    if variant == "row_start_back":
        lens = np.insert(lens, 72001, 0)
    if variant == "row_start_back_diag":
        lens = np.insert(lens, 72001, 1)
        lens[100] = 6                                             # the entry count and the straddling offset stay
    if variant in ("table_fits_diag", "table_too_long_diag"):
        # behind the straddling row: a rows of 7, b of 1, c of 2 with a + b + c row starts and 7 a + b + 2 c = 35 707 entries
        first = STRADDLER + 1
        a, b, c = (2975, 14880, 1) if variant == "table_fits_diag" else (2975, 14882, 0)
        per = np.full(a, b // a)
        per[:b % a] += 1
        pieces = [lens[:first]]
        for k in range(a):
            pieces += [np.ones(per[k], dtype=np.int64), np.array([7])]
        lens = np.concatenate(pieces + [np.full(c, 2, dtype=np.int64)])
    if variant in ("table_fits", "table_too_long"):
        first = STRADDLER + 1                                     # the first row that starts in chunk 1
        extra = TABLE_ROWS_FIT - (CHUNKED_ROWS - first) + (variant == "table_too_long")
        per = np.full(CHUNKED_ROWS - first, extra // (CHUNKED_ROWS - first))
        per[:extra % (CHUNKED_ROWS - first)] += 1
        pieces = [lens[:first]]
        for k in range(CHUNKED_ROWS - first):
            pieces += [np.zeros(per[k], dtype=np.int64), lens[first + k:first + k + 1]]
        lens = np.concatenate(pieces)
    rp, ci, val = _band(lens, rng)

    def low(r, gaps):                                             # the row's leading columns moved down: differences `gaps`
        b = rp[r]
        for k in range(len(gaps) - 1, -1, -1):
            ci[b + k] = ci[b + k + 1] - gaps[k]
    if variant == "d65535":
        low(70000, [65535])
    if variant == "d65536_chunk1":
        low(77000, [65536])
    if variant == "d65536_chunk0":
        low(70000, [65536])
    if variant.startswith("row_start_back"):
        low(72002, [40000, 30000])                               # (row 72 001 is the empty / diagonal-only one)
    if variant == "unsorted_chunk1":
        b = rp[78000]
        ci[[b + 4, b + 5]] = ci[[b + 5, b + 4]]
        val[[b + 4, b + 5]] = val[[b + 5, b + 4]]
    return rp, ci, val, len(rp) - 1


# ---------------------------------------------------------------- many slices: the single-block scan
MANY_SLICES = (1023, 1024, 1025, 2049)


def many_slices(ns, seed=16):
    """ns slices (the last one 59 rows), 0-3 entries per row, every fifth slice without entries: the offsets of the
    device-pointer path come from k_exclusive_scan_ll, whose carry crosses a trip of its block beyond 1024 slices"""
    rng = np.random.default_rng(seed + ns)
    nrow = ns * SLICE - 5
    lens = rng.integers(0, 4, size=nrow)
    lens[(np.arange(nrow) // SLICE) % 5 == 2] = 0
    lens[nrow - 3:] = (3, 0, 2)
    rp = np.zeros(nrow + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    r = np.repeat(np.arange(nrow), lens)
    ci = rng.integers(0, nrow, size=int(rp[-1]))
    ci = ci[np.lexsort((ci, r))].astype(np.int32)
    return rp, ci, _ints(rng, len(ci)), nrow


# ---------------------------------------------------------------- self halo: the LIST / GHOST instantiations
HALO_VARIANTS = ("mixed", "no_interior", "no_boundary", "fallback")


def self_halo(variant="mixed", seed=17):
    """(rowptr, colidx, val, ncol, plan): owned rows plus 40 ghost columns, ghost column nrow + g the image of the owned row
    plan["send_idx"][g]; plan holds the arrays of Matrix.set_halo for the single peer 0.
      mixed      : 300 rows; the slices 1, 3 and 4 (the ragged one) read ghost columns, 0 and 2 do not
      no_interior: every slice reads a ghost column
      no_boundary: none does (the ghost columns exist, the plan is exchanged, nothing reads it)
      fallback   : 66 620 rows, slice 2 touches 65 windows (and reads ghost columns): 32-bit columns for the matrix"""
    assert variant in HALO_VARIANTS
    rng = np.random.default_rng(seed)
    ng = 40
    nrow = 300 if variant != "fallback" else 65 * WINDOW + SLICE - 4
    ns = (nrow + SLICE - 1) // SLICE
    bnd = {"mixed": {1, 3, 4}, "no_interior": set(range(ns)), "no_boundary": set(), "fallback": {1, 2, ns - 1}}[variant]
    filled = set(range(5)) | ({500, ns - 1} if variant == "fallback" else set())
    rows = []
    for i in range(nrow):
        s, j = divmod(i, SLICE)
        if s not in filled:
            rows.append(np.zeros(0, dtype=np.int64))
            continue
        if variant == "fallback" and s == 2:
            c = np.unique(np.array([j, (j + 21) % 65, (j + 42) % 65]) * WINDOW + np.array([0, WINDOW - 1, 1 + 7 * j]))
        else:
            c = np.sort(rng.choice(min(nrow, 2 * WINDOW), size=1 + (3 * i) % 9, replace=False))
        if s in bnd and (j % 3 == 0 or j == SLICE - 1):
            c = np.concatenate([c, nrow + np.sort(rng.choice(ng, size=1 + j % 2, replace=False))])
        rows.append(c)
    send_idx = np.sort(rng.choice(nrow, size=ng, replace=False)).astype(np.int32)
    plan = dict(peers=np.array([0], dtype=np.int32), send_ptr=np.array([0, ng], dtype=np.int32), send_idx=send_idx,
                recv_ptr=np.array([0, ng], dtype=np.int32))
    return _csr(rows, rng) + (nrow + ng, plan)


def fold(colidx, nrow, send_idx):
    """the columns of the folded square matrix: a ghost column is the owned row it is an image of"""
    ci = np.asarray(colidx, dtype=np.int64).copy()
    g = ci >= nrow
    ci[g] = np.asarray(send_idx, dtype=np.int64)[ci[g] - nrow]
    return ci


# ---------------------------------------------------------------- the fixtures of the two test files
FIXTURES = {}
for _t in (0, 1, 63):
    FIXTURES["width_tail%d" % _t] = functools.partial(width_ladder, _t)
for _n in (1, 63, 64, 65):
    FIXTURES["tiny%d" % _n] = functools.partial(tiny, _n)
for _v in WINDOW_VARIANTS:
    FIXTURES["window_" + _v] = functools.partial(window_ladder, _v)
for _w in SORT_WIDTHS:
    FIXTURES["unsorted%d" % _w] = functools.partial(unsorted_ladder, _w)
FIXTURES["unsorted_ragged"] = functools.partial(unsorted_ladder, 30, True)
for _v in CHUNKED_VARIANTS:
    FIXTURES["chunked_" + _v] = functools.partial(chunked, _v)
for _n in MANY_SLICES:
    FIXTURES["slices%d" % _n] = functools.partial(many_slices, _n)
for _v in HALO_VARIANTS:
    FIXTURES["halo_" + _v] = functools.partial(self_halo, _v)

WIDTH_FIXTURES = ["width_tail0", "width_tail1", "width_tail63", "tiny1", "tiny63", "tiny64", "tiny65"]
WINDOW_FIXTURES = ["window_" + v for v in WINDOW_VARIANTS]
SQUARE_WINDOW_FIXTURES = ["window_le64", "window_w65", "window_pad65"]
UNSORTED_FIXTURES = ["unsorted%d" % w for w in SORT_WIDTHS] + ["unsorted_ragged"]
CHUNKED_FIXTURES = ["chunked_" + v for v in CHUNKED_VARIANTS]
SLICES_FIXTURES = ["slices%d" % n for n in MANY_SLICES]
HALO_FIXTURES = ["halo_" + v for v in HALO_VARIANTS]
FAMILIES = dict(width=WIDTH_FIXTURES, window=WINDOW_FIXTURES, unsorted=UNSORTED_FIXTURES, chunked=CHUNKED_FIXTURES,
                slices=SLICES_FIXTURES, halo=HALO_FIXTURES)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """the named matrix, built once per process, its arrays read-only"""
    out = FIXTURES[name]()
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------- references
def row_index(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(np.asarray(rowptr, dtype=np.int64)))


def exact_product(rowptr, colidx, val, x=None, ncol=None):
    """A x with the integer data of this module: exact in double whatever the order of the sum"""
    x = x_of(ncol) if x is None else x
    nrow = len(rowptr) - 1
    return np.bincount(row_index(rowptr), weights=np.asarray(val) * x[np.asarray(colidx, dtype=np.int64)], minlength=nrow)[:nrow]


def max_partial_sum(rowptr, colidx, val, ncol):
    """the largest magnitude any partial sum of a row's terms can reach: sum_j |a_ij| x_j"""
    return float(exact_product(rowptr, colidx, np.abs(val), ncol=ncol).max(initial=0.0))


def stable_sorted(rowptr, colidx, val):
    """every row sorted by column, entries of equal column in the order they came"""
    o = np.lexsort((np.asarray(colidx), row_index(rowptr)))
    return np.asarray(rowptr), np.asarray(colidx)[o], np.asarray(val)[o]


def _fma(a, b, c):
    """a * b + c rounded once (Python 3.10 has no math.fma): exact rational arithmetic, float() rounds to nearest even"""
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def emulate_spmv(rowptr, colidx, val, x):
    """the documented order of k_sell_spmv / k_sell_spmv16 on arbitrary doubles: acc0 takes the entries at the even positions
    of the (sorted) row and acc1 those at the odd ones, in position order, each step one fused multiply-add; the row's
    result is acc0 + acc1.  Padding entries (value 0) leave an accumulator as it is and are skipped."""
    nrow = len(rowptr) - 1
    y = np.zeros(nrow)
    for i in np.flatnonzero(np.diff(rowptr)):
        acc = [0.0, 0.0]
        b = int(rowptr[i])
        for k in range(int(rowptr[i + 1]) - b):
            acc[k & 1] = _fma(float(val[b + k]), float(x[colidx[b + k]]), acc[k & 1])
        y[i] = acc[0] + acc[1]
    return y


def unfused_spmv(rowptr, colidx, val, x):
    """the same order with the product rounded before the sum (what the kernels do NOT compute)"""
    nrow = len(rowptr) - 1
    y = np.zeros(nrow)
    for i in np.flatnonzero(np.diff(rowptr)):
        acc = [0.0, 0.0]
        b = int(rowptr[i])
        for k in range(int(rowptr[i + 1]) - b):
            acc[k & 1] = float(val[b + k]) * float(x[colidx[b + k]]) + acc[k & 1]
        y[i] = acc[0] + acc[1]
    return y


def random_values(name, seed=21):
    """(val, x) for the bit-level comparison: values N(0,1) * 10^U(-3,3) on the pattern of the fixture, x standard normal"""
    rp, ci, _, ncol = fixture(name)[:4]
    rng = np.random.default_rng(seed)
    return rng.standard_normal(len(ci)) * 10.0 ** rng.uniform(-3.0, 3.0, len(ci)), rng.standard_normal(ncol)


# ---------------------------------------------------------------- classifier
def sort_R(wmax):
    """sell_sort_rows: rows staged per pass of the LDS sort"""
    ws, r = wmax | 1, 64
    while r > 1 and r * ws * 24 > 48 * 1024:
        r >>= 1
    return r


def regimes(rowptr, colidx, ncol=None):
    """Which branches of csrc/sell.hpp and csrc/ingress.hpp the CSR reaches.  The thresholds are restated from the code's
    dispatch lines and comments; THE KERNELS ARE THE AUTHORITY, and a change that moves a threshold there updates this
    function.  Returns a dict:
      width [nslices]          stored width of each slice (even); npair = width // 2
      windows [nslices]        distinct 1024-column windows over the stored positions of the slice, padding included (the
                               padding column is the row's first column as it arrived, 0 for a row without entries and for
                               the rows of the last slice beyond nrow)
      entry_windows [nslices]  the same over the entries alone
      bits                     16 when every slice has at most 64 windows, else 32 (0 for a matrix without stored entries)
      sort_R                   rows per pass of k_sell_sort_rows: ONE value per launch, from the widest slice
      sort_trips [nslices]     trips of the rank loop for a row of the slice: ceil(width / 64)
      scan_trips               trips of the single block of k_exclusive_scan_ll over the slices
      chunks                   per chunk of the host ingress dict(entries, rows: row starts in it, wide: differences outside
                               [0, 65535] that are not row starts, mode: 16 | 32, bytes)
      link_bytes               sum of the chunks' bytes + 4 (nrow + 1)
      straddlers               per inner chunk boundary the row it cuts and the offset inside the row, or None"""
    rp = np.asarray(rowptr, dtype=np.int64)
    ci = np.asarray(colidx, dtype=np.int64)
    nrow = len(rp) - 1
    nnz = int(rp[-1])
    ns = (nrow + SLICE - 1) // SLICE
    lens = np.diff(rp)
    plen = np.zeros(ns * SLICE, dtype=np.int64)
    plen[:nrow] = lens
    width = (plen.reshape(ns, SLICE).max(axis=1) + 1) & ~1 if ns else np.zeros(0, dtype=np.int64)
    sl = row_index(rp) // SLICE
    big = int(ci.max(initial=0) // WINDOW) + 2

    def distinct(keys):
        u = np.unique(keys)
        return np.bincount(u // big, minlength=ns)[:ns] if len(u) else np.zeros(ns, dtype=np.int64)
    ekeys = sl * big + ci // WINDOW
    first = np.zeros(ns * SLICE, dtype=np.int64)
    has = np.flatnonzero(lens > 0)
    first[has] = ci[rp[has]]
    padded = np.flatnonzero(plen < np.repeat(width, SLICE))
    pkeys = (padded // SLICE) * big + first[padded] // WINDOW
    out = dict(width=width, entry_windows=distinct(ekeys), windows=distinct(np.concatenate([ekeys, pkeys])))
    out["bits"] = 0 if width.sum() == 0 else (16 if out["windows"].max() <= 64 else 32)
    out["sort_R"] = sort_R(int(width.max(initial=0)))
    out["sort_trips"] = (width + 63) // 64
    out["scan_trips"] = (ns + SCAN_BLOCK - 1) // SCAN_BLOCK
    # ---- host ingress
    cstart = [0]
    if nnz > 0:
        cstart.append(min(nnz, FIRST_CHUNK))
    while cstart[-1] < nnz:
        cstart.append(min(nnz, cstart[-1] + CHUNK))
    nch = len(cstart) - 1
    crow = np.searchsorted(rp, cstart, side="left")                # first row that starts at or behind the chunk's first entry
    d = np.diff(ci)
    wide = np.concatenate([[False], (d < 0) | (d > 65535)])        # entry q against q - 1, as the flat staging pass counts
    start = np.zeros(max(nnz, 1), dtype=bool)
    start[rp[has]] = True
    wide = wide & ~start[:len(wide)] if nnz else wide              # the chunk's finisher takes the row starts back
    chunks, verdict = [], None
    for c in range(nch):
        p0, p1 = cstart[c], cstart[c + 1]
        cnt, nr = p1 - p0, int(crow[c + 1] - crow[c])
        off_rf = (10 * cnt + 3) & ~3
        fits = nch <= MAX_CHUNKS and off_rf + 4 * nr <= 12 * cnt
        try16 = fits and (c == 0 or verdict)
        nw = int(wide[p0:p1].sum())
        m16 = bool(try16 and nw == 0)
        if c == 0:
            verdict = m16
        chunks.append(dict(entries=cnt, rows=nr, wide=nw, mode=16 if m16 else 32, bytes=off_rf + 4 * nr if m16 else 12 * cnt))
    out["chunks"] = chunks
    out["link_bytes"] = sum(c["bytes"] for c in chunks) + 4 * (nrow + 1)
    strad = []
    for c in range(1, nch):
        r = int(np.searchsorted(rp, cstart[c], side="right")) - 1
        strad.append((r, cstart[c] - int(rp[r])) if rp[r] < cstart[c] < rp[r + 1] else None)
    out["straddlers"] = strad
    return out


# ---------------------------------------------------------------- mutations (host data only: what a wrong kernel would do)
MUTATIONS = ("swap_columns", "drop_last", "shift_1", "shift_1024", "next_row")


def mutate(rowptr, colidx, val, ncol, kind, seed=0):
    """the sorted CSR with one defect applied to one row (chosen by seed among the rows that can show it):
      swap_columns  two entries of a row exchange their columns (values stay)
      drop_last     the row's last entry is lost
      shift_1       one column is off by one
      shift_1024    one column is off by one window
      next_row      the row's last entry lands in the next row"""
    rp, ci, val = np.array(rowptr, dtype=np.int64), np.array(colidx, dtype=np.int64), np.array(val, dtype=np.float64)
    rng = np.random.default_rng(seed)
    nrow = len(rp) - 1
    lens = np.diff(rp)
    cand = np.flatnonzero(lens >= 2) if kind == "swap_columns" else np.flatnonzero(lens >= 1)
    if kind == "next_row":
        cand = cand[cand < nrow - 1]
    rng.shuffle(cand)
    for r in cand:
        b, e = int(rp[r]), int(rp[r + 1])
        if kind == "swap_columns":
            k = [q for q in range(b + 1, e) if ci[q] != ci[b] and val[q] != val[b]]
            if not k:
                continue
            ci[[b, k[0]]] = ci[[k[0], b]]
            return rp, ci, val
        if kind in ("drop_last", "next_row"):
            if kind == "drop_last":
                ci, val = np.delete(ci, e - 1), np.delete(val, e - 1)
                rp[r + 1:] -= 1
            else:                                                  # the entry stays where it is in the arrays: the row ends before it
                rp[r + 1] -= 1
            return rp, ci, val
        step = 1 if kind == "shift_1" else WINDOW
        q = int(rng.integers(b, e))
        new = ci[q] + step if ci[q] + step < ncol else ci[q] - step
        if new < 0:
            continue
        ci[q] = new
        return rp, ci, val
    raise ValueError("no row can show " + kind)
