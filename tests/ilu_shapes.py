"""Constructed matrices for the row-shape branches of block ILU(k) (csrc/ilu.hpp), a long-double reference factorisation
that shares no code with oracle/, and a classifier that restates the kernels' thresholds on a factor pattern.

Host only: numpy, no GPU, no SPH.  The SPH Poisson matrices of the other suites reach whichever branch the kernel support
and the lattice happen to give; the generators here place rows ON the thresholds (64/65 lower entries, pivot rows of 64/65
and 128/129 upper entries, a longest row of 128, 129 and 130 entries) by design, with patterns that are structurally
nonsymmetric and values of mixed sign with a negative diagonal on about a fifth of the rows.

What a branch depends on (restated in regimes(); csrc/ilu.hpp is the authority):
  * the width `wmax` the host dispatches on -- ILU(0): the longest row of the MATRIX (the sliced-ELL width, entries outside
    the row's block included); ILU(k > 0): the longest row of the factor (k_iluk_merge).  ladder() therefore hands the
    columns outside a block only to rows that stay within the longest in-block row: matrix and factor width coincide;
  * k_ilu_factor<WIDE>: wmax > 128; k_ilu_schedule<NARROW>: wmax <= 129;
  * inside the narrow factor template a row takes the loop without branches when it has at most 64 lower entries and none
    of its pivot rows has more than 64 upper entries; else the general loop, whose steps >= 64 read the LDS tables and
    whose tail loop handles the part of a pivot row beyond 64 (WIDE: beyond 128) entries.
"""
import functools

import numpy as np

LD = np.longdouble

# (a, b): row i of an m-row block gets min(i, a) lower and min(m - 1 - i, b) upper in-block columns
TAB_N = [(0, 0), (1, 0), (0, 1), (15, 16), (16, 15), (17, 31), (32, 33), (63, 64), (64, 63), (65, 62), (62, 65), (100, 27),
         (27, 100), (127, 0), (0, 127), (48, 48), (5, 70), (70, 5)]
TAB_W = TAB_N + [(64, 129), (65, 128), (129, 64), (128, 128), (200, 10), (10, 200), (130, 130)]
TAB_FILL = [(6, 2), (0, 8), (9, 0), (4, 4), (2, 10), (8, 6), (12, 1)]


# ---------------------------------------------------------------- generators
def _values(rng, rows, n):
    """CSR of the column lists `rows` (each sorted, diagonal included): off-diagonals N(0,1) * 10^U(-2,0), the diagonal
    (1 + U(0,1)) * sum|offdiag| + 0.1 with a negative sign on about a fifth of the rows (strict diagonal dominance)"""
    rp = np.zeros(n + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows])
    ci = np.concatenate(rows).astype(np.int32)
    val = np.zeros(len(ci))
    for i, c in enumerate(rows):
        off = rng.standard_normal(len(c)) * 10.0 ** rng.uniform(-2.0, 0.0, len(c))
        d = int(np.searchsorted(c, i))
        off[d] = 0.0
        dv = (1.0 + rng.uniform()) * np.abs(off).sum() + 0.1
        off[d] = -dv if rng.uniform() < 0.2 else dv
        val[rp[i]:rp[i + 1]] = off
    return rp, ci, val


def ladder(blocks, table, seed=7, coupling=2):
    """(rowptr, colidx, val, block_ptr): blocks of the given sizes; consecutive rows cycle through `table`, the in-block
    columns drawn without replacement; `coupling` columns in other blocks (which block Jacobi drops) for every row that
    stays within the longest in-block row with them (see the module docstring)."""
    rng = np.random.default_rng(seed)
    bp = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int32)
    n = int(bp[-1])
    rows, g = [], 0
    for b in range(len(blocks)):
        lo, m = int(bp[b]), int(blocks[b])
        for i in range(m):
            a, u = table[g % len(table)]
            g += 1
            nl, nu = min(i, a), min(m - 1 - i, u)
            low = lo + np.sort(rng.choice(i, nl, replace=False)) if nl else np.zeros(0, dtype=np.int64)
            upp = lo + i + 1 + np.sort(rng.choice(m - 1 - i, nu, replace=False)) if nu else np.zeros(0, dtype=np.int64)
            rows.append(np.concatenate([low, [lo + i], upp]).astype(np.int64))
    lmax = max(len(c) for c in rows)
    for b in range(len(blocks)):
        lo, m = int(bp[b]), int(blocks[b])
        for i in range(lo, lo + m):
            nc = min(coupling, lmax - len(rows[i]), n - m)
            if nc > 0:
                out = rng.choice(n - m, nc, replace=False)
                out = np.where(out < lo, out, out + m)
                rows[i] = np.sort(np.concatenate([rows[i], out]))
    return _values(rng, rows, n) + (bp,)


def fan(m=512, seed=7, roots=24, small=12):
    """One block with WIDE dependency levels in both directions.  With a = roots + m // 2:  rows [0, roots) have no lower
    entries; rows [roots, a) have 1..small lower entries, all among the roots (ONE L-level of m // 2 rows); rows [a, m)
    have 65 to 127 lower entries drawn from [0, a) (the next L-level, every row with more than 64 dependencies).  The upper
    parts are the mirror image from the last row down.  No row exceeds 128 entries and some have exactly 128."""
    rng = np.random.default_rng(seed)
    a = roots + m // 2
    assert m - a >= 130 and 2 * a > m and roots < 65

    def side(j, other):          # j: distance from this direction's first row; other: entries the row has the other way
        if j < roots:
            return np.zeros(0, dtype=np.int64)
        if j < a:
            return np.sort(rng.choice(roots, int(rng.integers(1, small + 1)), replace=False))
        top = 127 - other
        cnt = (65, top, int(rng.integers(65, top + 1)))[min(j % 8, 2)]
        return np.sort(rng.choice(a, cnt, replace=False))

    low, upp = [None] * m, [None] * m
    for i in range(m):           # the small sides first: the long side of a row fills what is left of its 128 entries
        if i < a:
            low[i] = side(i, 0)
        if m - 1 - i < a:
            upp[i] = m - 1 - side(m - 1 - i, 0)[::-1]
    for i in range(m):
        if low[i] is None:
            low[i] = side(i, len(upp[i]))
        if upp[i] is None:
            upp[i] = m - 1 - side(m - 1 - i, len(low[i]))[::-1]
    rows = [np.concatenate([low[i], [i], upp[i]]).astype(np.int64) for i in range(m)]
    return _values(rng, rows, m) + (np.array([0, m], dtype=np.int32),)


# ---------------------------------------------------------------- the fixtures of the two test files
# Seed 7 throughout, except where PLAIN DOUBLE arithmetic in the sequential IKJ order (the oracle) is itself further than
# half the project's entrywise bound (relative 1e-10 above a floor of 1e-10 max|f|) from the long-double factor: a handful
# of entries near the floor that come out of cancellation (seed 7: 2.3e-10 for "sub128", 5.9e-11 for "fill1024" at K = 3;
# typical seeds give 1e-11).  A fixture on which double arithmetic uses up the bound cannot tell a wrong kernel from a right
# one; tests/test_ilu_shapes_host.py holds every fixture to that condition, whatever the device does.
FIXTURES = {
    "narrow": lambda: ladder([256, 256, 100], TAB_N),
    "w128": lambda: ladder([256, 200], TAB_N),
    # 129: rows of 64 + 64 and of 128 dependencies in ONE direction, the most two column loads per lane hold (NARROW schedule);
    # 130: rows of 64 + 65 and of 129 dependencies in one direction, which the NARROW schedule would cut short
    "w129": lambda: ladder([256, 200], TAB_N + [(64, 64), (128, 0), (0, 128)]),
    "w130": lambda: ladder([256, 200], TAB_N + [(64, 65), (129, 0), (0, 129)]),
    "wide": lambda: ladder([512, 300], TAB_W),
    "fan": lambda: fan(512),
    "ragged": lambda: ladder([1, 63, 64, 65, 1024, 1, 200], TAB_N),
    "fill64": lambda: ladder([64, 64, 64, 64, 30], TAB_FILL),
    "fill256": lambda: ladder([256, 256, 77], TAB_FILL),
    "fill512": lambda: ladder([512, 130], TAB_FILL),
    "fill1024": lambda: ladder([1024, 200], TAB_FILL, seed=8),
    "sub128": lambda: ladder([128] * 40, TAB_N, seed=9),         # 40 uniform subdomains: Schwarz, one workgroup each
    "sub128c3": lambda: ladder([128] * 40, TAB_N, coupling=3),   # ... with three columns outside for the overlap layer
    "one_narrow": lambda: ladder([256], TAB_N),                  # a single block: Schwarz on the whole matrix
    "one_wide": lambda: ladder([512], TAB_W),
}
ILU0_FIXTURES = ["narrow", "w128", "w129", "w130", "wide", "fan", "ragged"]
ILUK_FIXTURES = ["fill64", "fill256", "fill512", "fill1024"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    out = FIXTURES[name]()
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- long-double reference
def _block_dense(rp, ci, val, lo, hi):
    m = hi - lo
    W = np.zeros((m, m), dtype=LD)
    P = np.zeros((m, m), dtype=bool)
    for r in range(m):
        c = ci[rp[lo + r]:rp[lo + r + 1]]
        keep = (c >= lo) & (c < hi)
        W[r, c[keep] - lo] = val[rp[lo + r]:rp[lo + r + 1]][keep]
        P[r, c[keep] - lo] = True
    return W, P


def _symbolic(P, K):
    """Ifpack_IlukGraph's rule on one block: lev_ij = min(lev_ij, lev_ik + lev_kj + 1) over the pivots k < min(i, j) in
    ascending order, an entry kept (and used as a pivot or in a pivot row) while its level is <= K.  Pivot by pivot over
    all rows at once: when pivot k is applied, row k and column k have seen every pivot below k, exactly as in the
    row-by-row order, so the operations are the same ones.  Returns the final pattern."""
    m = P.shape[0]
    big = np.int16(1 << 12)
    lev = np.where(P, np.int16(0), big).astype(np.int16)
    for k in range(m - 1):
        rows = np.flatnonzero(lev[k + 1:, k] <= K) + k + 1
        cols = np.flatnonzero(lev[k, k + 1:] <= K) + k + 1
        if rows.size == 0 or cols.size == 0:
            continue
        ix = np.ix_(rows, cols)
        new = lev[rows, k][:, None] + lev[k, cols][None, :] + np.int16(1)
        new[new > K] = big
        lev[ix] = np.minimum(lev[ix], new)
    return lev <= K


def _numeric(W, P):
    """IKJ on the FINAL pattern P, in long double: strict L (unit diagonal implied), D and strict U in one dense array"""
    m = W.shape[0]
    for i in range(m):
        w = W[i]
        for k in np.flatnonzero(P[i, :i]):
            lik = w[k] / W[k, k]
            w[k] = lik
            w[k + 1:] -= lik * W[k, k + 1:]
        # what the pivots added outside the row's pattern is dropped: no step above read it (the pivots are taken from P)
        w[~P[i]] = 0.0
    return W


@functools.lru_cache(maxsize=None)
def _ref_cached(name, K):
    rp, ci, val, bp = fixture(name)
    return _ref_iluk(rp, ci, val, bp, K)


def _ref_iluk(rp, ci, val, bp, K):
    n = len(rp) - 1
    cols, vals, dense = [], [], []
    for b in range(len(bp) - 1):
        lo, hi = int(bp[b]), int(bp[b + 1])
        W, P = _block_dense(rp, ci, val, lo, hi)
        if not P.diagonal().all():
            raise ValueError("row without a diagonal entry")
        if K > 0:
            P = _symbolic(P, K)
        W = _numeric(W, P)
        dense.append((W, P))
        for r in range(hi - lo):
            c = np.flatnonzero(P[r])
            cols.append(c + lo)
            vals.append(W[r, c])
    frp = np.zeros(n + 1, dtype=np.int32)
    frp[1:] = np.cumsum([len(c) for c in cols])
    fci = np.concatenate(cols).astype(np.int32)
    fv = np.concatenate(vals)
    for a in (frp, fci, fv):
        a.setflags(write=False)
    return frp, fci, fv, dense


def ref_iluk(rp, ci, val, bp, K):
    """block ILU(K) of the CSR matrix over the blocks `bp`: (frp, fci, fval) with fval in long double -- symbolic pass with
    Ifpack_IlukGraph's level rule, THEN the numeric IKJ pass on the final pattern (a one-pass factorisation with dynamic
    insertion skips the updates of entries whose level only drops to K at a later pivot)"""
    return _ref_iluk(rp, ci, val, bp, K)[:3]


def ref_iluk_of(name, K):
    """ref_iluk of a named fixture, computed once per process"""
    return _ref_cached(name, K)[:3]


def _apply(dense, bp, r):
    z = np.zeros(len(r), dtype=LD)
    for b, (W, P) in enumerate(dense):
        lo, hi = int(bp[b]), int(bp[b + 1])
        y = np.asarray(r[lo:hi], dtype=LD).copy()
        for i in range(hi - lo):
            y[i] -= np.dot(W[i, :i], y[:i])
        for i in range(hi - lo - 1, -1, -1):
            y[i] = (y[i] - np.dot(W[i, i + 1:], y[i + 1:])) / W[i, i]
        z[lo:hi] = y
    return z


def ref_apply(rp, ci, val, bp, K, r):
    """z = U^-1 D^-1 L^-1 r block by block, in long double"""
    return _apply(_ref_iluk(rp, ci, val, bp, K)[3], bp, r)


def ref_apply_of(name, K, r):
    return _apply(_ref_cached(name, K)[3], fixture(name)[3], r)


# ---------------------------------------------------------------- classifier
def _levels(n, frp, fci, direction):
    lev = np.zeros(n, dtype=np.int64)
    order = range(n) if direction == 0 else range(n - 1, -1, -1)
    for i in order:
        c = fci[frp[i]:frp[i + 1]]
        d = c[c < i] if direction == 0 else c[c > i]
        if len(d):
            lev[i] = lev[d].max() + 1
    return lev


def regimes(frp, fci, bp, wmax=None):
    """Which branches of csrc/ilu.hpp the factor pattern (frp, fci) over the blocks bp reaches.  wmax: the width the host
    dispatches on when it is not the factor's longest row (ILU(0) of a matrix with longer rows than its in-block part).
    The thresholds are the ones of the code's dispatch lines and comments; a change that moves one updates this function."""
    n = len(frp) - 1
    rows = np.repeat(np.arange(n), np.diff(frp))
    dg = np.bincount(rows[fci < rows], minlength=n)
    up = np.bincount(rows[fci > rows], minlength=n)
    out = dict(wmax=int((dg + up + 1).max()) if wmax is None else int(wmax))
    out["factor"] = "wide" if out["wmax"] > 128 else "narrow"          # ilu_launch_factor: wide = F->wmax > 128
    out["schedule"] = "narrow" if out["wmax"] <= 129 else "general"    # ilu_launch_schedule: F->wmax <= 129
    pmax = np.zeros(n, dtype=np.int64)                                 # longest upper part among a row's pivot rows
    low = fci < rows
    np.maximum.at(pmax, rows[low], up[fci[low]])
    if out["factor"] == "narrow":
        fast = (dg <= 64) & (pmax <= 64)                               # k_ilu_factor: narrow_row
        out["fast"] = int(np.sum(fast & (dg > 0)))
        out["general_dg"] = int(np.sum(dg > 64))                       # steps s >= 64: the LDS tables
        out["general_pivot"] = int(np.sum(pmax > 64))                  # the pnq[u] > 64 tail loop
        out["wide_dg"] = out["wide_pivot"] = 0
    else:
        out["fast"] = out["general_dg"] = out["general_pivot"] = 0
        out["wide_dg"] = int(np.sum(dg > 64))
        out["wide_pivot"] = int(np.sum(pmax > 128))                    # the pnq[u] > 128 tail loop
    for t in (64, 65, 128, 129):
        out["dg%d" % t] = int(np.sum(dg == t))
        out["up%d" % t] = int(np.sum(up == t))
    blk = np.repeat(np.arange(len(bp) - 1), np.diff(bp))
    for d, (name, dep) in enumerate((("L", dg), ("U", up))):
        lev = _levels(n, frp, fci, d)
        out[name + "_65_128"] = int(np.sum((dep >= 65) & (dep <= 128)))   # k_ilu_schedule<true>: the second column load
        out[name + "_gt128"] = int(np.sum(dep > 128))
        sched = lev > 0                                                 # rows without dependencies are not in the stream
        key = blk[sched] * (n + 1) + lev[sched]
        uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        out[name + "_widest_level"] = int(cnt.max()) if len(cnt) else 0
        out[name + "_one_row_levels"] = int(np.sum(cnt == 1))
        has64 = np.zeros(len(uniq), dtype=bool)
        has64[inv[dep[sched] > 64]] = True
        out[name + "_widest_level_with_gt64"] = int(cnt[has64].max()) if has64.any() else 0
    return out


def matrix_wmax(rp):
    return int(np.diff(rp).max())


# ---------------------------------------------------------------- overlapping subdomains (additive Schwarz)
def extended_rows(rp, ci, bp, overlap=1):
    """Ifpack's overlapping subdomains restated with numpy sets: the owned rows of a block first, then, layer by layer, the
    rows that the COLUMNS of the previous layer's rows reference and the subdomain does not hold yet, ascending.  On a
    structurally nonsymmetric matrix that relation is one-directional: a row that references the subdomain without being
    referenced by it stays outside.  Returns (rows [nloc], loc_ptr [nsub + 1])."""
    out, lp = [], [0]
    for s in range(len(bp) - 1):
        rows = np.arange(bp[s], bp[s + 1], dtype=np.int64)
        layer = rows
        for _ in range(overlap if len(bp) > 2 else 0):
            cols = np.unique(np.concatenate([ci[rp[i]:rp[i + 1]] for i in layer]))
            layer = np.setdiff1d(cols, rows)
            rows = np.concatenate([rows, layer])
        out.append(rows)
        lp.append(lp[-1] + len(rows))
    return np.concatenate(out).astype(np.int32), np.array(lp, dtype=np.int32)


def local_matrix(rp, ci, val, rows):
    """the matrix restricted to the rows and columns `rows` of one subdomain, in the subdomain's own numbering (position in
    `rows`), columns ascending: (rowptr, colidx, val)"""
    n = len(rp) - 1
    loc = np.full(n, -1, dtype=np.int64)
    loc[rows] = np.arange(len(rows))
    cols, vals = [], []
    for i in rows:
        c = loc[ci[rp[i]:rp[i + 1]]]
        keep = c >= 0
        o = np.argsort(c[keep], kind="stable")
        cols.append(c[keep][o])
        vals.append(val[rp[i]:rp[i + 1]][keep][o])
    lrp = np.zeros(len(rows) + 1, dtype=np.int32)
    lrp[1:] = np.cumsum([len(c) for c in cols])
    return lrp, np.concatenate(cols).astype(np.int32), np.concatenate(vals)
