"""Constructed matrices for the branches of the additive-Schwarz layer (csrc/schwarz.hpp), a long-double reference of the
whole preconditioner (subdomain row lists, local matrices, ILU(k) factor, the two triangular solves, the combine mode) in
a sparse row-wise form, and a model that restates on an exported factor which branch of schwarz.hpp a matrix reaches.

Host only: numpy, no GPU.  Built on tests/ilu_shapes.py (value rule, ladder, fan, extended_rows, local_matrix); the
reference here does what ilu_shapes._numeric does, row by row on a work vector instead of a dense m x m array, so that a
subdomain of 4096 or 8192 rows fits.

What a branch depends on (restated in model(); csrc/schwarz.hpp is the authority):
  * form: one workgroup per subdomain (>= 32 subdomains, the largest <= 4096 extended rows, the longest factor row <= 1024);
    else persistent launches unless nloc / min(L levels, U levels) >= 4096; else one launch per dependency level;
  * persistent factorisation: 4 waves per row when (nnz - nloc) / 2 / nloc > 64 (integer division), else 1; the column
    look-up is a hash table of 2^hbits slots (the smallest power of two >= twice the longest row) while 12 maxrow + 16 +
    6 2^hbits + 8 bytes fit 64 KiB -- a longest row of 2048 -- and a binary search beyond; a longest row above 5000 is refused;
  * persistent sweeps: the level orders (ascending row inside a level) padded to multiples of 4 positions and cut into runs
    of at most 64 positions, whole levels unless a level is longer; 16 lanes per row, lane `sub` holds the entries
    sub, sub + 16, ... of the row's side; a dependency whose position lies inside the row's run goes on the lane's near list
    (6 entries, then the overflow loop); with long_rows (more than one row in twenty has more than 96 entries on a side:
    the SPLIT = true kernels) one at most 128 positions before the run goes on the far list (6 entries, then its overflow
    loop).
"""
import functools

import numpy as np

import ilu_shapes as sh

LD = np.longdouble

K_RUN, K_RECENT, K_NEAR, K_FAR, K_CHUNK = 64, 128, 6, 6, 96
K_LONG_WINDOW = 4
WIDE_LEVEL, MAX_ROW = 4096, 5000
SUB_MAX_ROWS, SUB_MIN_SUBS, SUB_FACTOR_MAX_ROW = 4096, 32, 1024
SYM_CAP, SUB_HASH = 2048, 8192


# ---------------------------------------------------------------- generators
def rows_of(rp, ci):
    return [ci[rp[i]:rp[i + 1]].astype(np.int64) for i in range(len(rp) - 1)]


def _finish(rng, rows, n, bp=None):
    return sh._values(rng, rows, n) + (np.array([0, n], dtype=np.int32) if bp is None else bp,)


def comb(window, n=1024, seed=7):
    """Chain rows at the ids that are 0 modulo 16: the lower part of such a row is the `window` ids below it, so that the
    chain rows among them sit 16 entries apart -- ONE sub-lane of the sweep holds all of them.  The rows at 15 modulo 16
    are the mirror image (upper part: the `window` ids above); every other row is a level-0 filler in both directions.
    Each chain row is a level of its own (4 padded positions): a run holds 16 of them."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        if i % 16 == 0:
            c = np.arange(max(0, i - window), i + 1)
        elif i % 16 == 15:
            c = np.arange(i, min(n, i + window + 1))
        else:
            c = np.array([i])
        rows.append(c.astype(np.int64))
    return _finish(rng, rows, n)


def from_counts(counts, seed=7):
    """one block; row i has min(i, a) lower and min(m - 1 - i, u) upper columns for counts[i] = (a, u), drawn without replacement"""
    rng = np.random.default_rng(seed)
    m = len(counts)
    rows = []
    for i, (a, u) in enumerate(counts):
        nl, nu = min(i, a), min(m - 1 - i, u)
        low = np.sort(rng.choice(i, nl, replace=False)) if nl else np.zeros(0, dtype=np.int64)
        upp = i + 1 + np.sort(rng.choice(m - 1 - i, nu, replace=False)) if nu else np.zeros(0, dtype=np.int64)
        rows.append(np.concatenate([low, [i], upp]).astype(np.int64))
    return _finish(rng, rows, m)


TAB_S = [(0, 0), (1, 0), (0, 1), (15, 16), (96, 3), (3, 96), (48, 48), (95, 0), (0, 95), (64, 31), (31, 64), (96, 0), (0, 96),
         (17, 31), (5, 70), (70, 5)]


def short(nlong, m=400):
    """a ladder whose rows have at most 96 entries on a side (one chunk of the sweeps), except `nlong` rows of 97"""
    counts = [TAB_S[g % len(TAB_S)] for g in range(m)]
    for t, i in enumerate(np.linspace(120, 279, nlong).astype(int) if nlong else []):
        counts[i] = (97, 3) if t % 2 == 0 else (3, 97)
    return from_counts(counts)


def dense_upper(extra, m=400):
    """130 m + extra off-diagonal entries: (nnz - m) / 2 / m is 65 for extra = 0 and 64 for extra = -1.  The first 48 rows
    have 300 upper entries (more than one round of the 256 threads of k_gilu_factor_sf<4>)."""
    up = [min(m - 1 - i, 300 if i < 48 else 70 + (i * 7) % 40) for i in range(m)]
    lo = [min(i, 3 + (i * 5) % 30) for i in range(m)]
    target, total, i = 130 * m + extra, sum(up) + sum(lo), m - 1
    assert total < target
    while total < target:
        assert lo[i] < i
        lo[i] += 1
        total += 1
        i = i - 1 if i > m // 2 else m - 1
    return from_counts(list(zip(lo, up)))


def long_row(length, m):
    """a 15-entries-a-row ladder whose last row has `length` entries (length - 1 of the m - 1 ids below it: its pivot rows'
    columns hit and miss its pattern)"""
    rp, ci, val, bp = sh.ladder([m], sh.TAB_FILL)
    rows = rows_of(rp, ci)
    rng = np.random.default_rng(1000 + length)
    rows[m - 1] = np.concatenate([np.sort(rng.choice(m - 1, length - 1, replace=False)), [m - 1]]).astype(np.int64)
    return _finish(rng, rows, m)


def wide(h, seed=7):
    """2 h rows in two levels per direction: row i < h has the one upper column h + p(i), row h + j the one lower column q(j)"""
    rng = np.random.default_rng(seed)
    p, q = rng.permutation(h), rng.permutation(h)
    rows = [np.array([i, h + p[i]], dtype=np.int64) for i in range(h)] + [np.array([q[j], h + j], dtype=np.int64) for j in range(h)]
    return _finish(rng, rows, 2 * h)


def ext(n, B=128, seed=7):
    """B-row subdomains of a 15-entries-a-row ladder with one column outside per row; the rows of subdomain 0 reference,
    31 columns each (row 0: the remainder too), the first 31 B + (n - 32 B > 0) rows outside it: its extended list has
    exactly 4096 rows for n = 4096 and 4097 for n = 4224"""
    rp, ci, val, bp = sh.ladder([B] * (n // B), sh.TAB_FILL, seed, coupling=1)
    rows = rows_of(rp, ci)
    nout = 31 * B + (1 if n > 32 * B else 0)
    for r in range(B):
        add = np.arange(B + 31 * r, B + 31 * (r + 1))
        if r == 0 and nout > 31 * B:
            add = np.concatenate([add, [B + 31 * B]])
        c = rows[r]
        rows[r] = np.concatenate([c[c < B], add]).astype(np.int64)
    return _finish(np.random.default_rng(seed + 1), rows, n, bp)


def zero_pivot(name, z):
    """the fixture `name` of ilu_shapes with a stored 0.0 on the diagonal of row z, which no other row references"""
    rp, ci, val, bp = sh.fixture(name)
    rows = [c if i == z else c[c != z] for i, c in enumerate(rows_of(rp, ci))]
    rp, ci, val = sh._values(np.random.default_rng(11), rows, len(rows))
    val[rp[z] + int(np.searchsorted(ci[rp[z]:rp[z + 1]], z))] = 0.0
    return rp, ci, val, np.array(bp)


def knuth(c, bits):
    """the multiplicative hash of the LDS tables of schwarz.hpp: the top `bits` bits of c * 2654435761 mod 2^32"""
    return ((np.asarray(c, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def collide(n, bits, lo):
    """the ids in [lo, n) whose home slot is one of the last 8 or the first 16 of a 2^bits table: a probe chain that starts
    at the end of the table, wraps round slot 2^bits - 1 and runs on through the first slots"""
    c = np.arange(lo, n)
    h = knuth(c, bits)
    return c[(h >= (1 << bits) - 8) | (h < 16)]


def _spread(rng, cols, npiv, extra):
    """`cols` dealt to npiv pivot rows (every column to one of them, so that the union is exact), plus `extra` more each"""
    deal = [cols[k::npiv] for k in range(npiv)]
    return [np.unique(np.concatenate([d, rng.choice(cols, min(extra, len(cols)), replace=False)])) for d in deal]


def sym_edge(size, n=1200, npiv=40, seed=7):
    """fill 1: the level-1 pattern of the last row has exactly `size` entries -- its npiv lower columns 0 .. npiv - 1, the
    diagonal, and the union of those pivot rows' upper parts, which are dealt from a set of size - npiv - 1 columns.  The
    other rows are a 15-entries-a-row ladder: no other row's pattern comes near the table's capacity."""
    rp, ci, val, bp = sh.ladder([n], sh.TAB_FILL, seed)
    rows = rows_of(rp, ci)
    rng = np.random.default_rng(seed + 1)
    T = np.sort(rng.choice(np.arange(npiv, n - 1), size - npiv - 1, replace=False))
    for k, up in enumerate(_spread(rng, T, npiv, 30)):
        c = rows[k]
        rows[k] = np.concatenate([c[c <= k], up]).astype(np.int64)
    rows[n - 1] = np.concatenate([np.arange(npiv), [n - 1]]).astype(np.int64)
    return _finish(rng, rows, n)


def sym_collide(n=8192, npiv=8, seed=7):
    """fill 1: the level-1 pattern of the last row holds every column of collide(n, 11, npiv): keys that share their bucket of
    the 11-bit table of k_gilu_symbolic1 and a chain that wraps past slot 2047"""
    rp, ci, val, bp = sh.ladder([n], sh.TAB_FILL, seed)
    rows = rows_of(rp, ci)
    rng = np.random.default_rng(seed + 1)
    C = collide(n - 1, 11, npiv)
    for k, up in enumerate(_spread(rng, C, npiv, 10)):
        c = rows[k]
        rows[k] = np.concatenate([c[c <= k], up]).astype(np.int64)
    rows[n - 1] = np.concatenate([np.arange(npiv), [n - 1]]).astype(np.int64)
    return _finish(rng, rows, n)


def nodiag1(base, z, k0):
    """`base` without the stored diagonal of row z, with the entries (z, k0) and (k0, z), k0 < z: the pivot of row z is
    the fill - l(z, k0) u(k0, z)"""
    rp, ci, val, bp = base
    rows = rows_of(rp, ci)
    assert k0 < z
    rows[z] = np.unique(np.concatenate([rows[z], [k0]]))
    rows[k0] = np.unique(np.concatenate([rows[k0], [z]]))
    rp, ci, val = sh._values(np.random.default_rng(13), rows, len(rows))
    # entries of size one on both sides of the fill: the pivot is not small
    for i, j in ((z, k0), (k0, z)):
        val[rp[i] + int(np.searchsorted(ci[rp[i]:rp[i + 1]], j))] = 1.0
    val[rp[k0] + int(np.searchsorted(ci[rp[k0]:rp[k0 + 1]], k0))] = 2.0 + np.abs(val[rp[k0]:rp[k0 + 1]]).sum()
    return _drop(rp, ci, val, bp, z)


def ext_few(seed=7):
    """32 subdomains of 128 rows; subdomain 3 has NO column outside itself and subdomain 4 exactly one"""
    rp, ci, val, bp = sh.ladder([128] * 32, sh.TAB_FILL, seed, coupling=1)
    rows = rows_of(rp, ci)
    for i in range(3 * 128, 5 * 128):
        c = rows[i]
        rows[i] = c[(c >= i // 128 * 128) & (c < i // 128 * 128 + 128)]
    rows[4 * 128 + 5] = np.sort(np.concatenate([rows[4 * 128 + 5], [77]]))
    rows[4 * 128 + 90] = np.sort(np.concatenate([rows[4 * 128 + 90], [77]]))
    return _finish(np.random.default_rng(seed + 1), rows, len(rows), bp)


def ext_collide(nsub=128, B=128, seed=7):
    """the rows of subdomain 0 reference every column of collide(n, 13, B): keys that share their bucket of the 13-bit set of
    k_gilu_sub_rows and a chain that wraps past slot 8191"""
    rp, ci, val, bp = sh.ladder([B] * nsub, sh.TAB_FILL, seed, coupling=1)
    rows = rows_of(rp, ci)
    C = collide(nsub * B, 13, B)
    for r in range(B):
        rows[r] = np.unique(np.concatenate([rows[r], C[r::B], C[(r + 7) % B::B]])).astype(np.int64)
    return _finish(np.random.default_rng(seed + 1), rows, len(rows), bp)


def subrow(length, B=128, seed=7):
    """32 subdomains of B rows; the upper half of subdomain 0 has long rows -- 70 lower and 100 upper columns -- and its last
    row all B - 1 ids below it and length - B columns outside the subdomain: under overlap 1 those rows come in, and the
    row's `length` entries are the longest factor row (more than 64 pivots, pivot rows of more than 64 upper entries)"""
    rp, ci, val, bp = sh.ladder([B] * 32, sh.TAB_FILL, seed, coupling=1)
    rows = rows_of(rp, ci)
    rng = np.random.default_rng(seed + 1)
    out = np.sort(rng.choice(np.arange(B, 32 * B), length - B, replace=False))
    for i in range(B // 2, B - 1):
        rows[i] = np.concatenate([np.sort(rng.choice(i, min(i, 70), replace=False)), [i], np.arange(i + 1, B),
                                  np.sort(rng.choice(out, 100 - (B - 1 - i), replace=False))]).astype(np.int64)
    rows[B - 1] = np.concatenate([np.arange(B), out]).astype(np.int64)
    return _finish(rng, rows, 32 * B, bp)


def _drop(rp, ci, val, bp, z):
    p = int(rp[z] + np.searchsorted(ci[rp[z]:rp[z + 1]], z))
    assert ci[p] == z
    rp = rp.copy()
    rp[z + 1:] -= 1
    return rp, np.delete(ci, p), np.delete(val, p), np.array(bp)


def no_diagonal(name, z):
    """the fixture `name` of ilu_shapes without the stored diagonal of row z"""
    rp, ci, val, bp = sh.fixture(name)
    p = int(rp[z] + np.searchsorted(ci[rp[z]:rp[z + 1]], z))
    assert ci[p] == z
    rp = rp.copy()
    rp[z + 1:] -= 1
    return rp, np.delete(ci, p), np.delete(val, p), np.array(bp)


# name -> (generator, block_size handed to the library: 0 = the whole matrix)
FILL1 = {
    "sym1023": (lambda: sym_edge(1023), 0),
    "sym1024": (lambda: sym_edge(1024), 0),
    "sym_collide": (lambda: sym_collide(), 0),
    "nodiag1_dev": (lambda: nodiag1(sh.ladder([256], sh.TAB_FILL), 100, 40), 0),
    "nodiag1_host": (lambda: nodiag1(sym_edge(1024), 600, 300), 0),     # the same kind of row, the pattern built on the host
}
FIXTURES = {
    "comb_near": (lambda: comb(112), 0),
    "comb_far": (lambda: comb(640), 0),
    "fan": (lambda: sh.fixture("fan"), 0),
    "short96": (lambda: short(0), 0),
    "short97lo": (lambda: short(20), 0),        # 20 of 400 rows: exactly one in twenty, long_rows stays false
    "short97hi": (lambda: short(21), 0),
    "dense_upper64": (lambda: dense_upper(-1), 0),
    "dense_upper": (lambda: dense_upper(0), 0),
    "row2048": (lambda: long_row(2048, 2304), 0),
    "row2049": (lambda: long_row(2049, 2304), 0),
    "row5000": (lambda: long_row(5000, 5200), 0),
    "row5001": (lambda: long_row(5001, 5200), 0),
    "wide4095": (lambda: wide(4095), 0),
    "wide4096": (lambda: wide(4096), 0),
    "subs31": (lambda: sh.ladder([128] * 31, sh.TAB_N, seed=9), 128),
    "subs32": (lambda: sh.ladder([128] * 32, sh.TAB_N, seed=9), 128),
    "ext4096": (lambda: ext(4096), 128),
    "ext4097": (lambda: ext(4224), 128),
    "ext0_1": (ext_few, 128),
    "ext_collide": (ext_collide, 128),
    "subrow1024": (lambda: subrow(1024), 128),
    "subrow1025": (lambda: subrow(1025), 128),
}
WHOLE = [k for k, v in FIXTURES.items() if v[1] == 0 and k != "row5001"]
SUBS = [k for k, v in FIXTURES.items() if v[1] > 0]
FIXTURES.update(FILL1)
# (name, level of fill, overlap) of every case that builds
CASES = [(k, 0, 0) for k in WHOLE] + [(k, 0, ov) for k in SUBS for ov in (0, 1)] + [(k, 1, 0) for k in FILL1]
# the refusals: name -> (generator, block_size, level_launches, text of the error)
REFUSALS = {
    "row5001": (FIXTURES["row5001"][0], 0, False, "exceeds the LDS row image"),
    "zero_pivot level launches": (lambda: zero_pivot("one_narrow", 0), 0, True, "zero pivot"),
    "zero_pivot persistent": (lambda: zero_pivot("one_narrow", 0), 0, False, "zero pivot"),
    "zero_pivot one workgroup": (lambda: zero_pivot("sub128", 640), 128, False, "zero pivot"),
    "nodiag0 host": (lambda: no_diagonal("one_narrow", 100), 0, False, "missing diagonal"),
    "nodiag0 device": (lambda: no_diagonal("sub128", 700), 128, False, "missing diagonal"),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    out = tuple(np.array(a) for a in FIXTURES[name][0]())
    for a in out:
        a.setflags(write=False)
    return out


def block_size(name):
    return FIXTURES[name][1]


# ---------------------------------------------------------------- long-double reference, sparse and row-wise
def ref_pattern(lrp, lci, K):
    """the ILU(K) pattern of one local matrix, K = 0 | 1, by the level-of-fill rule: level 1 = the columns right of the
    diagonal of the level-0 pivot rows.  K = 1 inserts a structurally missing diagonal (as Ifpack does); K = 0 refuses it."""
    m = len(lrp) - 1
    a = rows_of(lrp, lci)
    if K == 0:
        for i, c in enumerate(a):
            if i not in c:
                raise ValueError("row without a diagonal entry")
        return a
    assert K == 1
    upper = [c[c > i] for i, c in enumerate(a)]
    return [np.unique(np.concatenate([c, [i]] + [upper[k] for k in c[c < i]])) for i, c in enumerate(a)]


def ref_factor(lrp, lci, lv, K):
    """(frp, fci, fval long double, diagonal position per row): IKJ on the final pattern, as ilu_shapes._numeric"""
    m = len(lrp) - 1
    pat = ref_pattern(lrp, lci, K)
    frp = np.zeros(m + 1, dtype=np.int64)
    frp[1:] = np.cumsum([len(c) for c in pat])
    fci = np.concatenate(pat).astype(np.int32)
    fv = np.zeros(len(fci), dtype=LD)
    fdg = np.zeros(m, dtype=np.int64)
    w = np.zeros(m, dtype=LD)
    U = [None] * m
    D = np.zeros(m, dtype=LD)
    for i, c in enumerate(pat):
        w[:] = 0.0
        w[lci[lrp[i]:lrp[i + 1]]] = lv[lrp[i]:lrp[i + 1]]
        d = int(np.searchsorted(c, i))
        for k in c[:d]:
            lik = w[k] / D[k]
            w[k] = lik
            uc, uv = U[k]
            w[uc] -= lik * uv          # what lands outside the row's pattern is never read: the pivots are taken from c
        fv[frp[i]:frp[i + 1]] = w[c]
        fdg[i], D[i], U[i] = d, w[i], (c[d + 1:], w[c[d + 1:]])
    return frp, fci, fv, fdg


def ref_solve(frp, fci, fv, fdg, r):
    m = len(frp) - 1
    y = np.array(r, dtype=LD)
    for i in range(m):
        b, d = frp[i], fdg[i]
        if d:
            y[i] -= np.dot(fv[b:b + d], y[fci[b:b + d]])
    for i in range(m - 1, -1, -1):
        b, d, e = frp[i], fdg[i], frp[i + 1]
        y[i] = (y[i] - np.dot(fv[b + d + 1:e], y[fci[b + d + 1:e]])) / fv[b + d]
    return y


def ref_schwarz(rp, ci, val, B, K, overlap):
    """rows, loc_ptr, and the factor of the block-diagonal local matrix in the library's numbering (columns = position in
    `rows`), values in long double; per subdomain the pieces for ref_apply"""
    n = len(rp) - 1
    bp = np.array([0, n] if B == 0 else list(range(0, n, B)) + [n], dtype=np.int32)
    rows, lp = sh.extended_rows(rp, ci, bp, overlap)
    frps, fcis, fvs, subs = [np.zeros(1, dtype=np.int64)], [], [], []
    for s in range(len(bp) - 1):
        mine = rows[lp[s]:lp[s + 1]]
        lrp, lci, lv = (rp, ci, val) if len(bp) == 2 else sh.local_matrix(rp, ci, val, mine)
        f = ref_factor(lrp, lci, lv, K)
        frps.append(f[0][1:] + frps[-1][-1])
        fcis.append(f[1] + lp[s])
        fvs.append(f[2])
        subs.append((mine, int(bp[s + 1] - bp[s]), f))
    out = (rows, lp, np.concatenate(frps), np.concatenate(fcis).astype(np.int32), np.concatenate(fvs), subs)
    for a in out[:5]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_schwarz_of(name, K, overlap):
    rp, ci, val, bp = fixture(name)
    return ref_schwarz(rp, ci, val, block_size(name), K, overlap)


def ref_apply(ref, combine, r):
    """z = sum over the subdomains of R^T (LU)^-1 R r (add) or of its owned part (zero), in long double"""
    z = np.zeros(len(r), dtype=LD)
    for mine, nown, f in ref[5]:
        y = ref_solve(f[0], f[1], f[2], f[3], np.asarray(r)[mine])
        if combine == "add":
            np.add.at(z, mine, y)
        else:
            z[mine[:nown]] = y[:nown]
    return z


# ---------------------------------------------------------------- regime model
def _levels(n, frp, fci, dg, upper):
    lev = np.zeros(n, dtype=np.int64)
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        c = fci[frp[i] + dg[i] + 1:frp[i + 1]] if upper else fci[frp[i]:frp[i] + dg[i]]
        if len(c):
            lev[i] = lev[c].max() + 1
    return lev


def _runs(sizes):
    """runs_of: run starts over the padded positions of the levels of the given sizes"""
    rs, pos, cur = [0], 0, 0
    for sz in sizes:
        sz = (int(sz) + 3) // 4 * 4
        if cur > 0 and cur + sz > K_RUN:
            rs.append(pos)
            cur = 0
        while sz > 0:
            take = min(sz, K_RUN - cur)
            pos += take
            cur += take
            sz -= take
            if cur == K_RUN:
                rs.append(pos)
                cur = 0
    if cur > 0:
        rs.append(pos)
    return np.array(rs, dtype=np.int64)


def model(frp, fci, lp, level_launches=False, fill=0, wmax=0):
    """What create() decides and what the persistent sweeps meet on the factor pattern (frp, fci) (the library's numbering:
    M.export()) of the subdomains lp, for overlap <= 1.  wmax: the longest row of the MATRIX (the device-local set-up of
    many subdomains takes rows up to 1024 entries).  Keys as schwarz_info() / paths() where they have one."""
    frp, fci = np.asarray(frp, dtype=np.int64), np.asarray(fci, dtype=np.int64)
    nloc, nsub = len(frp) - 1, len(lp) - 1
    rows = np.repeat(np.arange(nloc), np.diff(frp))
    dg = np.bincount(rows[fci < rows], minlength=nloc)
    up = np.bincount(rows[fci > rows], minlength=nloc)
    out = dict(nloc=nloc, nnz=int(frp[-1]), nsub=nsub, maxrow=int(np.diff(frp).max()), sub_maxrows=int(np.diff(lp).max()))
    lev = [_levels(nloc, frp, fci, dg, False), _levels(nloc, frp, fci, dg, True)]
    nl, nu = int(lev[0].max()) + 1, int(lev[1].max()) + 1
    out["levels_l"], out["levels_u"] = nl, nu
    sub = not level_launches and nsub >= SUB_MIN_SUBS and out["sub_maxrows"] <= SUB_MAX_ROWS and out["maxrow"] <= SUB_FACTOR_MAX_ROW
    persistent = not level_launches and not sub and nloc // min(nl, nu) < WIDE_LEVEL
    out["persistent"] = 2 if sub else 1 if persistent else 0
    out["refused"] = out["maxrow"] > MAX_ROW
    out["rows_gt96"] = int(np.sum((dg > K_CHUNK) | (up > K_CHUNK)))
    out["max_side"] = int(max(dg.max(), up.max()))
    out["mean_upper"] = (out["nnz"] - nloc) // 2 // nloc
    out["max_upper"] = int(up.max())
    out["max_lower"] = int(dg.max())
    # row lists and local matrices on the device: many subdomains, no fill, none beyond the capacity of the one-workgroup form
    out["rows_on_device"] = int(not level_launches and fill == 0 and nsub >= SUB_MIN_SUBS and wmax <= SUB_FACTOR_MAX_ROW and
                                out["sub_maxrows"] <= SUB_MAX_ROWS)
    # level-1 pattern on the device: the whole matrix, every row below the 1024 entries that half the 11-bit table holds
    out["symbolic1_on_device"] = int(fill == 1 and nsub == 1 and out["maxrow"] < SYM_CAP // 2)
    # long_rows is evaluated by the host set-up only
    out["long_rows"] = int(out["rows_gt96"] * 20 > nloc) if not out["rows_on_device"] else 0
    out["factor_waves"] = (4 if out["mean_upper"] > 64 else 1) if persistent else 0
    hbits = 0
    while (1 << hbits) < 2 * out["maxrow"]:
        hbits += 1
    fits = out["maxrow"] * 12 + 16 + (6 << hbits) + 8 <= 64 * 1024
    out["hbits"] = hbits if persistent and fits else 0
    if not persistent:
        out.update(nrun_l=0, nrun_u=0, n4l=0, n4u=0)
        return out
    for d, name in enumerate("lu"):
        order = np.argsort(lev[d], kind="stable")                 # bucket(): ascending row inside a level
        sizes = np.bincount(lev[d])
        start4 = np.concatenate([[0], np.cumsum((sizes + 3) // 4 * 4)])
        first = np.concatenate([[0], np.cumsum(sizes)])
        pos4 = np.zeros(nloc, dtype=np.int64)
        pos4[order] = start4[lev[d][order]] + np.arange(nloc) - first[lev[d][order]]
        rs = _runs(sizes)
        out["n4" + name], out["nrun_" + name] = int(start4[-1]), len(rs) - 1
        out["runs_near_" + name] = max(K_LONG_WINDOW if out["long_rows"] else 2, 2 * -(-(len(rs) - 1) // len(sizes)))
        base = rs[np.searchsorted(rs, pos4, side="right") - 1]   # first position of every row's run
        side = fci > rows if d else fci < rows
        r, c = rows[side], fci[side]
        t = np.arange(len(fci))[side] - (frp[r] + dg[r] + 1 if d else frp[r])
        sl = pos4[c] - base[r]
        assert np.all(pos4[c] < pos4[r])
        nn = np.zeros((nloc, 16), dtype=np.int64)
        nr = np.zeros((nloc, 16), dtype=np.int64)
        np.add.at(nn, (r, t % 16), sl >= 0)
        if out["long_rows"]:
            np.add.at(nr, (r, t % 16), (sl < 0) & (sl >= -K_RECENT))
        out["near_max_" + name], out["far_max_" + name] = int(nn.max()), int(nr.max())
        out["near_overflow_rows_" + name] = int(np.sum(nn.max(axis=1) > K_NEAR))
        out["far_overflow_rows_" + name] = int(np.sum(nr.max(axis=1) > K_FAR))
        out["chunks_max_" + name] = int(-(-(up if d else dg).max() // K_CHUNK))
        out["rows_2chunks_" + name] = int(np.sum((up if d else dg) > K_CHUNK))
        run_lo = np.searchsorted(rs, start4[:-1], side="right")
        run_hi = np.searchsorted(rs, start4[:-1] + np.maximum(sizes, 1) - 1, side="right")
        out["cut_levels_" + name] = int(np.sum(run_hi > run_lo))
        out["widest_level_" + name] = int(sizes.max())
    return out
