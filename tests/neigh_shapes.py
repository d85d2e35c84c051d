"""Constructed neighbour lists for the branches of the neighbour-list layout (csrc/assemble.hpp: build_neigh_ell_t with
k_numneigh, k_slicew_from_rowlen, k_neigh_sort, k_neigh_transpose) and of what sits downstream of it (k_asm_count, the
diagonal-slot rule of the row kernels, the duplicate merge, the choice of the SELL row sort), and a classifier that restates
the thresholds of that code on a list.

Host only: numpy, the particle generator and nothing else.  The generator's own lists hold no out-of-cut entry (skin 0),
23-28 entries per row in 2-D and about 113 in 3-D, always in the generator's order: they land on the counting branch of the
sort with one slice width and never on the length edges.  The lists here are edits of such lists -- what a caller with a
skin, a binned list builder or a thin periodic box hands over:

  * pad(row, L): the row gets entries until its raw length is L.  The added entries are particle indices < nall, never the
    row's own, distinct where the cloud has enough candidates, each farther than sqrt(1.0001) * cut from the row's
    particle: the strict `rsq < cutsq` test of every kernel and of the oracle skips them, they only lengthen the list;
  * truncate(row, L): the row keeps its first L entries (L = 0: the row is its diagonal alone).  The oracle is given the
    same list, so its row follows;
  * permute: entries reordered inside rows -- shuffled, reversed, ascending by column, or left as they are.  Entries of one
    row whose columns are equal keep their relative order (periodic images of one particle are summed in list order by
    the oracle and by the stable sort of the device).

What a branch depends on (restated in regimes(); the kernels are the authority, a change that moves a threshold there
updates regimes()):
  * a slice is 64 rows; its width is the longest raw row rounded up to even (k_slicew_from_rowlen); wmax is the widest;
  * with a column map the lists are ordered by column when wmax <= kNeighSortCap = 1024, else the whole layout stays in
    the caller's order (T.sorted = 0);
  * k_neigh_sort, one wave per row: a row whose keys (column << 10 | position) ascend is copied through; else a row of
    len <= 128 is ranked by counting (two keys per lane: the second one, kb, serves positions 64 .. 127); else a bitonic
    network over P = 256 / 512 / 1024 >= len; the LDS stride per row is max(wmax + 2, P(wmax)) rounded up to even;
  * k_neigh_transpose moves 16 columns of a slice per trip: widths that are no multiple of 16 end in a partial tile;
  * the row kernels put the diagonal where the first in-cut column above the row's own arrives (sorted lists), else last;
  * the assemblies sort the rows again (sell_sort_rows) unless the lists were sorted and n > 32768; duplicate columns of a
    row (two periodic images of one particle in cut: a box thinner than 2 cut) are merged for every n.
"""
import functools

import numpy as np

import isph_amd  # noqa: F401
from isph_amd import workload

SLICE = 64                    # kSlice
TILE = 16                     # k_neigh_transpose: `for (int c0 = 0; c0 < w; c0 += 16)`
SORT_CAP = 1024               # kNeighSortCap: `if (wmax <= kNeighSortCap)`
COUNT_MAX = 128               # k_neigh_sort: `if (len > 128)` -> bitonic
BITONIC_MIN = 256             # k_neigh_sort: `int P = 256; while (P < len) P <<= 1;`
ROW_SORT_MAX = 32768          # kMergeAllRowsMax: T.dup is set for `T.sorted && n > kMergeAllRowsMax`, and the assemblies run
                              # `T.dup ? sell_set_wmax : sell_sort_rows`
OUT_OF_CUT = 1.0001           # padded entries lie outside OUT_OF_CUT * cut^2

KEEP, SHUFFLE, REVERSE, ASCEND = 0, 1, 2, 3

SIZES = {"small": (34, 34), "big": (182, 182)}
THIN_DUP = {"small": (64, 4), "big": (8200, 4)}
THIN_SELF = {"small": (64, 2), "big": (16400, 2)}
SHORT = [0, 1, 2, 3, 63, 64, 65, 127, 128]
LONG = {"p256": [129, 255, 256], "p512": [257, 511, 512], "p1024": [513, 1023, 1024]}
WIDTHS = [15, 16, 17, 31, 32, 33, 47, 48]


# ---------------------------------------------------------------- clouds
@functools.lru_cache(maxsize=None)
def cloud(ncell, brick=None):
    """(parts, colmap) of the generator, JITTER mode; arrays read-only: every fixture is a copy-on-edit of these"""
    dim = len(ncell)
    if dim == 2:
        spec = workload.TGVSpec(dim=2, ncell=tuple(ncell), brick=brick or (8, 8), origin=(0.5, 0.5), mode=workload.JITTER)
    else:
        spec = workload.TGVSpec(dim=3, ncell=tuple(ncell), brick=brick or (8, 8, 8), mode=workload.JITTER)
    parts = workload.make_tgv(spec)
    colmap = workload.single_rank_colmap(parts)
    for a in list(parts.values()) + [colmap]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return parts, colmap


def rows_of(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def rsq(parts, rows, idx):
    """|x_row - x_idx|^2 in the kernels' operation order (rsq_nofma: squares summed from the left, no fma)"""
    x = parts["x"]
    d = x[rows] - x[idx]
    s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if parts["dim"] == 3:
        s = s + d[:, 2] * d[:, 2]
    return s


def in_cut(parts):
    """mask over neigh_idx: the entries the strict cut test keeps"""
    return rsq(parts, rows_of(parts["neigh_ptr"]), parts["neigh_idx"]) < float(parts["cut"]) ** 2


# ---------------------------------------------------------------- the three edits
def _with_list(parts, lens, idx):
    out = dict(parts)
    ptr = np.zeros(len(lens) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(lens)
    out["neigh_ptr"] = ptr.astype(np.int32)
    out["neigh_idx"] = np.ascontiguousarray(idx, dtype=np.int32)
    return out


def _pads(parts, row, count, rng):
    x, dim = parts["x"], parts["dim"]
    d = x[:, :dim] - x[row, :dim]
    far = np.flatnonzero((d * d).sum(axis=1) > 1.0002 * float(parts["cut"]) ** 2)   # inside the OUT_OF_CUT bound with room
    far = far[far != row]
    assert len(far) > 0
    return rng.choice(far, size=count, replace=len(far) < count)


def resize(parts, lengths, seed):
    """rows of `lengths` ({row: raw length}) truncated or padded to exactly that length; the other rows untouched"""
    rng = np.random.default_rng(seed)
    ptr, idx = parts["neigh_ptr"], parts["neigh_idx"]
    rows = np.split(idx, ptr[1:-1])
    for r in sorted(lengths):
        L, have = lengths[r], len(rows[r])
        rows[r] = rows[r][:L] if L <= have else np.concatenate([rows[r], _pads(parts, r, L - have, rng)])
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    return _with_list(parts, lens, np.concatenate(rows) if lens.sum() else np.zeros(0, dtype=np.int32))


def disordered(parts, colmap):
    """per row: some key (column << 10 | position) is below its predecessor -- k_neigh_sort's `disorder |= kw[k + 1] < kw[k]`"""
    ptr, idx = parts["neigh_ptr"], parts["neigh_idx"]
    row = rows_of(ptr)
    key = (colmap[idx].astype(np.int64) << 10) | (np.arange(len(idx)) - ptr[:-1].astype(np.int64)[row])
    out = np.zeros(len(ptr) - 1, dtype=bool)
    out[row[1:][(np.diff(row) == 0) & (np.diff(key) < 0)]] = True
    return out


def permute(parts, colmap, mode, seed, force=True):
    """entries reordered inside rows; mode: one of KEEP / SHUFFLE / REVERSE / ASCEND or an array of them per row.  Entries of
    a row with equal columns keep their relative order.  A shuffled row that came out ascending by chance (rows of two or
    three entries) is reversed, so that every shuffled row with two different columns is out of order."""
    rng = np.random.default_rng(seed)
    ptr, idx = parts["neigh_ptr"], parts["neigh_idx"]
    n, total = len(ptr) - 1, len(idx)
    row = rows_of(ptr)
    m = np.broadcast_to(np.asarray(mode), (n,))[row]
    pos = np.arange(total, dtype=np.float64)
    col = colmap[idx].astype(np.float64)
    key = np.where(m == SHUFFLE, rng.random(total) * total, np.where(m == REVERSE, -pos, np.where(m == ASCEND, col, pos)))
    s = np.lexsort((pos, key, row))                       # s[t]: the old position of the entry now at t
    # equal columns of a row: the places they occupy now, taken in order, get the entries in their old order
    c = colmap[idx[s]]
    places = np.lexsort((np.arange(total), c, row))
    olds = np.lexsort((s, c, row))
    fixed = np.empty(total, dtype=np.int64)
    fixed[places] = s[olds]
    out = _with_list(parts, np.diff(ptr), idx[fixed])
    if force:
        again = (np.broadcast_to(np.asarray(mode), (n,)) == SHUFFLE) & ~disordered(out, colmap)
        if again.any():
            out = permute(out, colmap, np.where(again, REVERSE, KEEP), seed, force=False)
    return out


def canonical(parts, colmap):
    """the same list with the out-of-cut padding removed and every row ascending by column (stable)"""
    keep = rsq(parts, rows_of(parts["neigh_ptr"]), parts["neigh_idx"]) <= 1.00005 * float(parts["cut"]) ** 2
    row = rows_of(parts["neigh_ptr"])[keep]
    idx = parts["neigh_idx"][keep]
    lens = np.bincount(row, minlength=int(parts["nlocal"]))
    out = _with_list(parts, lens, idx)
    return permute(out, colmap, ASCEND, 0)


# ---------------------------------------------------------------- fixtures
def _spread(n, count, seed):
    """`count` distinct rows: row 0 (diagonal first in its row), row n - 1 (diagonal last) and the last slice's first row
    first, then rows spread over the slices, two of them neighbours inside one slice"""
    rng = np.random.default_rng(seed)
    fixed = [0, n - 1, (n - 1) // SLICE * SLICE, SLICE + 5, SLICE + 6]
    rest = rng.permutation(np.arange(2 * SLICE, (n - 1) // SLICE * SLICE))
    rows = fixed + [int(r) for r in rest[:max(0, count - len(fixed))]]
    return rows[:count]


def _assign(n, lengths, seed):
    """{row: length}: the longest lengths go to rows 0 and n - 1 (padding keeps their in-cut entries: their diagonals stay
    first and last), truncations never do"""
    order = sorted(lengths, reverse=True)
    return dict(zip(_spread(n, len(order), seed), order))


def _ladder(size, short, long=(), once=(), seed=1):
    """rows of the lengths `short` (once each), `long` (twice each: one row shuffled, one reversed) and `once`; every other
    row unedited; every row shuffled"""
    parts, colmap = cloud(SIZES[size])
    n = parts["nlocal"]
    where = _assign(n, list(short) + list(long) + list(long) + list(once), seed)
    edited = resize(parts, where, seed + 1)
    mode = np.full(n, SHUFFLE)
    seen = set()
    for r in sorted(where):
        if where[r] in long and where[r] not in seen:
            seen.add(where[r])
            mode[r] = REVERSE
    return permute(edited, colmap, mode, seed + 2), parts, colmap, dict(where=where, pads_only=False)


def _short(size):
    return _ladder(size, SHORT)


def _long(name, size):
    return _ladder(size, SHORT, LONG[name], seed=3 + len(name))


def _overcap(size):
    return _ladder(size, SHORT, LONG["p1024"], once=[1025], seed=9)


ALL_LENGTHS = SHORT + LONG["p256"] + LONG["p512"] + LONG["p1024"] + [1025]      # the 19 raw lengths of the ladders


@functools.lru_cache(maxsize=None)
def pads_only(size):
    """rows padded to every length of ALL_LENGTHS that is above the generator's own, nothing truncated, every row shuffled:
    the in-cut entries are those of the unedited list, so the oracle must give the unedited system"""
    parts, colmap = cloud(SIZES[size])
    have = int(np.diff(parts["neigh_ptr"]).max())
    where = _assign(parts["nlocal"], [L for L in ALL_LENGTHS if L > have], 51)
    return permute(resize(parts, where, 52), colmap, SHUFFLE, 53), parts, colmap, dict(where=where, pads_only=True)


def _inorder(size):
    parts, colmap = cloud(SIZES[size])
    n = parts["nlocal"]
    where = _assign(n, [64, 64, 128, 128, 256, 256], 11)
    edited = resize(parts, where, 12)
    return permute(edited, colmap, ASCEND, 13), parts, colmap, dict(where=where, pads_only=True)


def _widths(size):
    """slices 1 .. 8: the widest raw row is WIDTHS[s - 1] (rows truncated for 15 / 16 / 17: the generator's rows are longer;
    one or two rows padded for the others); the ragged last slice gets one row of 33"""
    parts, colmap = cloud(SIZES[size])
    n = parts["nlocal"]
    assert n % SLICE != 0
    have = np.diff(parts["neigh_ptr"])
    where = {}
    for s, w in enumerate(WIDTHS, start=1):
        rows = range(s * SLICE, (s + 1) * SLICE)
        if w < have[list(rows)].max():
            cyc = [w, w - 1, w // 2, 1, w, 0, w - 2]
            for k, r in enumerate(rows):
                where[r] = cyc[k % len(cyc)]
        else:
            where[s * SLICE + 7] = w
            where[s * SLICE + 63] = w - (s % 2)
    where[(n - 1) // SLICE * SLICE + 1] = 33
    edited = resize(parts, where, 21)
    return permute(edited, colmap, SHUFFLE, 22), parts, colmap, dict(where=where, pads_only=False)


def _thin(ncell, brick):
    parts, colmap = cloud(ncell, brick)
    return permute(parts, colmap, SHUFFLE, 31), parts, colmap, dict(where={}, pads_only=True)


def _shuffled3d():
    parts, colmap = cloud((33, 33, 33))
    n = parts["nlocal"]
    where = _assign(n, [129, 129, 300, 300], 41)
    edited = resize(parts, where, 42)
    return permute(edited, colmap, SHUFFLE, 43), parts, colmap, dict(where=where, pads_only=True)


FIXTURES = [(name, size) for name in ("short", "inorder", "p256", "p512", "p1024", "overcap", "widths", "thin_dup")
            for size in ("small", "big")] + [("thin_self", "small"), ("thin_self", "big"), ("shuffled3d", "big")]
SORTED_UNIQUE = [(name, size) for name in ("short", "inorder", "p256", "p512", "p1024", "widths")
                 for size in ("small", "big")] + [("shuffled3d", "big")]
PADS_ONLY = [(name, size) for (name, size) in FIXTURES if name in ("inorder", "thin_dup", "thin_self", "shuffled3d")]


def ident(f):
    return "%s-%s" % f


@functools.lru_cache(maxsize=None)
def fixture(name, size):
    """(constructed parts, unedited parts, colmap, notes); notes["where"]: {row: raw length} of the resized rows,
    notes["pads_only"]: the in-cut entries of every row are those of the unedited list (no truncation)"""
    if name == "short":
        out = _short(size)
    elif name in LONG:
        out = _long(name, size)
    elif name == "overcap":
        out = _overcap(size)
    elif name == "inorder":
        out = _inorder(size)
    elif name == "widths":
        out = _widths(size)
    elif name == "thin_dup":
        out = _thin(THIN_DUP[size], (8, 4))
    elif name == "thin_self":
        out = _thin(THIN_SELF[size], (8, 2))
    elif name == "shuffled3d":
        assert size == "big"
        out = _shuffled3d()
    else:
        raise KeyError(name)
    for k in ("neigh_ptr", "neigh_idx"):
        out[0][k].setflags(write=False)
    return out


# ---------------------------------------------------------------- classifier
def regimes(parts, colmap):
    """the branches a list reaches, from the thresholds of csrc/assemble.hpp (constants at the top of this file)"""
    ptr, idx = parts["neigh_ptr"], parts["neigh_idx"]
    n = int(parts["nlocal"])
    lens = np.diff(ptr).astype(np.int64)
    nslices = (n + SLICE - 1) // SLICE
    padded = np.zeros(nslices * SLICE, dtype=np.int64)
    padded[:n] = lens
    width = (padded.reshape(nslices, SLICE).max(axis=1) + 1) & ~1          # k_slicew_from_rowlen: (w + 1) & ~1
    wmax = int(width.max())
    is_sorted = wmax <= SORT_CAP                                           # build_neigh_ell_t: wmax <= kNeighSortCap
    need = wmax + 2                                                        # `long long need = wmax + 2`
    if wmax > COUNT_MAX:                                                   # `if (wmax > 128)`: p2 = 256; while (p2 < wmax) ...
        p2 = BITONIC_MIN
        while p2 < wmax:
            p2 <<= 1
        need = max(need, p2)
    stride = (need + 1) & ~1
    row = rows_of(ptr)
    col = colmap[idx].astype(np.int64)
    disorder = disordered(parts, colmap)
    path = {"copy": 0, "count": 0, "P256": 0, "P512": 0, "P1024": 0, "count_lens": [], "bitonic_lens": []}
    if is_sorted:
        path["copy"] = int(np.sum(~disorder))
        path["count"] = int(np.sum(disorder & (lens <= COUNT_MAX)))
        path["count_lens"] = sorted(set(lens[disorder & (lens <= COUNT_MAX)].tolist()))
        path["copy_lens"] = sorted(set(lens[~disorder].tolist()))
        for P in (256, 512, 1024):
            path["P%d" % P] = int(np.sum(disorder & (lens > max(COUNT_MAX, P // 2)) & (lens <= P)))
        path["bitonic_lens"] = sorted(set(lens[disorder & (lens > COUNT_MAX)].tolist()))
    # the matrix rows: in-cut entries, the diagonal's slot, duplicate columns
    cut = in_cut(parts)
    r_in, c_in = row[cut], col[cut]
    own = colmap[:n].astype(np.int64)
    below = np.bincount(r_in, weights=(c_in <= own[r_in]), minlength=n).astype(np.int64)   # slot rule: first cj > ci_own
    count = np.bincount(r_in, minlength=n)
    diag = {"alone": int(np.sum(count == 0)), "first": int(np.sum((count > 0) & (below == 0))),
            "last": int(np.sum((count > 0) & (below == count))), "inside": int(np.sum((below > 0) & (below < count)))}
    pairs = np.unique(r_in * (int(colmap.max()) + 1) + c_in)
    dup = len(r_in) - len(pairs)
    own_image = int(np.sum(c_in == own[r_in]))
    return dict(n=n, nslices=nslices, width=width, wmax=wmax, sorted=bool(is_sorted), stride=int(stride), lds_bytes=int(8 * stride * 4),
                path=path, diag=diag, duplicates=int(dup), own_images=own_image,
                merge="merge_adjacent_row under the flag" if (is_sorted and n > ROW_SORT_MAX) else "k_sell_merge_duplicates",
                row_sort="sell_set_wmax" if (is_sorted and n > ROW_SORT_MAX) else "sell_sort_rows",
                tail_tiles=sorted(set((width[width % TILE != 0] % TILE).tolist())), ragged=n % SLICE,
                raw_lens=sorted(set(lens.tolist())), nnz=len(pairs) + int(n - np.sum(np.bincount(r_in[c_in == own[r_in]], minlength=n) > 0)))
