"""No GPU: the constructed neighbour lists of tests/neigh_shapes.py reach the branches they are built for, their padding
is inert and can never index out of range, and the oracle is a usable reference on them.

Which fixture reaches which branch (regimes() restates the thresholds of csrc/assemble.hpp; "small" is 34 x 34 = 1 156
rows, "big" 182 x 182 = 33 124 rows, the smallest square cloud above the 32 768 rows below which sell_sort_rows re-sorts
every matrix row and hides a wrong order out of k_neigh_sort):

  fixture      raw row lengths                                  branch
  short        0 1 2 3 63 64 65 127 128, rest 23-28, shuffled   k_neigh_sort: counting rank only (first key of a lane up to
                                                                64, second key kb for 65 .. 128), copy-through for 0 and 1;
                                                                stride = wmax + 2 = 130; a row that is its diagonal alone
  inorder      every row ascending, some padded to 64 128 256   copy-through only, also for rows > 128 under the stride 258
                                                                of a layout sized for the bitonic network
  p256         short + 129 255 256 (shuffled and reversed)      bitonic network, P = 256, beside counted rows in one launch
  p512         short + 257 511 512                              bitonic, P = 512
  p1024        short + 513 1023 1024                            bitonic, P = 1024 = kNeighSortCap, stride 1026
  overcap      p1024 + one row of 1025                          wmax = 1026 > kNeighSortCap: the layout stays unsorted
                                                                (T.sorted = 0), sell_sort_rows also above 32 768 rows
  widths       slices whose widest row is 15 16 17 31 32 33     k_neigh_transpose: whole 16-column tiles, tails of 2 and 12
               47 48, n % 64 != 0                               columns, the ragged last slice
  thin_dup     box 4 dx wide, cut 3 dx: 64 x 4 and 8200 x 4     duplicate columns in a row, merged below and above 32 768 rows
  thin_self    box 2 dx wide, 64 x 2 and 16400 x 2              a particle's own image in its row (cj == ci_own), twice
  shuffled3d   33^3 = 35 937 rows shuffled, rows of 129 and 300 k_asm_poisson<3, 1> with packed records above the threshold,
                                                                P = 256 and 512 beside counted rows of ~113

Every fixture above the threshold has rows whose diagonal comes first, inside and last in the row (the slot rule
`cj > ci_own` of the row kernels), `short` rows that hold the diagonal alone.
"""
import time

import numpy as np
import pytest

import oracle as orc
import neigh_shapes as ns

SHORT_COUNTED = {2, 3, 63, 64, 65, 127, 128}


def even(w):
    return (w + 1) & ~1


@pytest.mark.parametrize("fx", ns.FIXTURES, ids=ns.ident)
def test_fixture_lands_in_its_regime(fx):
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    r = ns.regimes(c, cm)
    path = r["path"]
    big = size == "big"
    assert (r["n"] > ns.ROW_SORT_MAX) == big
    if name not in ("thin_dup", "thin_self"):
        assert r["ragged"] != 0                                               # a ragged last slice
    lens = np.diff(c["neigh_ptr"])
    for row, L in notes["where"].items():
        assert lens[row] == L
    bitonic = path["P256"] + path["P512"] + path["P1024"]
    if name == "short":
        assert r["sorted"] and r["wmax"] == 128 and r["stride"] == 130 and bitonic == 0
        assert SHORT_COUNTED <= set(path["count_lens"]) and {0, 1} <= set(path["copy_lens"])
        assert r["diag"]["alone"] >= 1
    elif name == "inorder":
        assert r["sorted"] and r["wmax"] == 256 and r["stride"] == 258
        assert path["copy"] == r["n"] and path["count"] == 0 and bitonic == 0
        assert {64, 128, 256} <= set(path["copy_lens"])
    elif name in ns.LONG:
        P = int(name[1:])
        assert r["sorted"] and r["wmax"] == P and r["stride"] == P + 2
        assert path["P%d" % P] == 6 and bitonic == 6 and path["bitonic_lens"] == ns.LONG[name]
        assert SHORT_COUNTED <= set(path["count_lens"])
        assert r["lds_bytes"] <= 65536
    elif name == "overcap":
        assert not r["sorted"] and r["wmax"] == 1026 > ns.SORT_CAP
        assert r["row_sort"] == "sell_sort_rows" and r["merge"] == "k_sell_merge_duplicates"    # above the threshold too
        assert 1025 in r["raw_lens"] and {513, 1023, 1024} <= set(r["raw_lens"])
    elif name == "widths":
        assert r["sorted"] and bitonic == 0
        assert r["width"][1:9].tolist() == [even(w) for w in ns.WIDTHS]
        assert [int(lens[64 * s:64 * s + 64].max()) for s in range(1, 9)] == ns.WIDTHS
        assert {2, 12} <= set(r["tail_tiles"]) and np.any(r["width"] % ns.TILE == 0)
        assert lens[(r["n"] - 1) // 64 * 64 + 1] == 33
    elif name == "thin_dup":
        assert r["sorted"] and r["duplicates"] > 0 and r["own_images"] == 0
        assert r["merge"] == ("merge_adjacent_row under the flag" if big else "k_sell_merge_duplicates")
        assert r["nnz"] == {"small": 5362, "big": 688662}[size]
    elif name == "thin_self":
        assert r["sorted"] and r["own_images"] == 2 * r["n"] and r["duplicates"] > 0
    elif name == "shuffled3d":
        assert r["n"] == 35937 and r["sorted"] and path["P256"] == 2 and path["P512"] == 2 and path["copy"] == 0
        assert path["count"] == r["n"] - 4
    if name != "overcap":
        assert r["row_sort"] == ("sell_set_wmax" if big else "sell_sort_rows")
    if big:                       # (thin_self: every row holds its own column in front of the diagonal's slot, none comes first)
        assert (r["diag"]["first"] >= 1 or name == "thin_self") and r["diag"]["inside"] >= 1 and r["diag"]["last"] >= 1


def test_every_branch_of_the_layer_is_reached_by_some_fixture():
    seen = dict(copy=0, count=0, P256=0, P512=0, P1024=0)
    unsorted_big = merged_big = 0
    count_lens, bitonic_lens = set(), set()
    for name, size in ns.FIXTURES:
        c, u, cm, notes = ns.fixture(name, size)
        r = ns.regimes(c, cm)
        for k in seen:
            seen[k] += r["path"][k]
        count_lens |= set(r["path"]["count_lens"])
        bitonic_lens |= set(r["path"]["bitonic_lens"])
        unsorted_big += (not r["sorted"]) and size == "big"
        merged_big += r["duplicates"] > 0 and size == "big"
    assert all(v > 0 for v in seen.values()), seen
    assert {2, 3, 63, 64, 65, 127, 128} <= count_lens
    assert {129, 255, 256, 257, 511, 512, 513, 1023, 1024} <= bitonic_lens
    assert unsorted_big and merged_big


@pytest.mark.parametrize("fx", ns.FIXTURES + [("pads_only", "small"), ("pads_only", "big")], ids=ns.ident)
def test_lists_are_valid_and_padding_is_out_of_cut(fx):
    """no index out of range, no row lists itself, offsets ascend from 0 to the list's length, and every entry that the
    unedited list does not hold lies outside 1.0001 cut^2: a constructed list can never fault a kernel, and its padding
    never enters a row"""
    name, size = fx
    c, u, cm, notes = ns.pads_only(size) if name == "pads_only" else ns.fixture(name, size)
    ptr, idx = c["neigh_ptr"], c["neigh_idx"]
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    assert ptr[0] == 0 and ptr[-1] == len(idx) and np.all(np.diff(ptr) >= 0) and len(ptr) == c["nlocal"] + 1
    assert idx.min() >= 0 and idx.max() < c["nall"]
    row = ns.rows_of(ptr)
    assert not np.any(idx == row)
    r2 = ns.rsq(c, row, idx)
    cutsq = float(c["cut"]) ** 2
    inside = r2 < cutsq
    assert np.all(r2[~inside] > ns.OUT_OF_CUT * cutsq)
    # the in-cut entries of a row are entries of the unedited row (all of them unless the row was truncated)
    big = np.int64(c["nall"])
    got = np.bincount(row[inside], minlength=c["nlocal"])
    have = np.diff(u["neigh_ptr"])
    assert np.all(np.isin(row[inside] * big + idx[inside], ns.rows_of(u["neigh_ptr"]) * big + u["neigh_idx"]))
    shorter = np.flatnonzero(got != have)
    assert all(notes["where"].get(int(r), 1 << 30) < have[r] for r in shorter)
    if notes["pads_only"]:
        assert len(shorter) == 0
    # padded entries are distinct inside a row
    pad_keys = row[~inside] * big + idx[~inside]
    assert len(np.unique(pad_keys)) == len(pad_keys)


def test_permutation_keeps_equal_columns_in_list_order():
    for name, size in (("thin_dup", "small"), ("thin_self", "small"), ("thin_dup", "big"), ("thin_self", "big")):
        c, u, cm, notes = ns.fixture(name, size)
        row = ns.rows_of(c["neigh_ptr"])
        out = []
        for p in (c, u):
            order = np.lexsort((np.arange(len(row)), cm[p["neigh_idx"]], row))       # stable: by row, column, list position
            out.append(p["neigh_idx"][order])
        assert np.array_equal(out[0], out[1])
        assert not np.array_equal(c["neigh_idx"], u["neigh_idx"])
    c, u, cm, notes = ns.fixture("p256", "small")
    lens = np.diff(c["neigh_ptr"])
    long_rows = [r for r in notes["where"] if notes["where"][r] in ns.LONG["p256"]]
    assert len(long_rows) == 6 and all(lens[r] > 128 for r in long_rows)
    # canonical(): the list the bit-for-bit tests compare with -- no padding, every row ascending, the same in-cut entries
    can = ns.canonical(c, cm)
    assert not ns.disordered(can, cm).any() and ns.in_cut(can).all()
    assert np.array_equal(np.diff(can["neigh_ptr"]), np.bincount(ns.rows_of(c["neigh_ptr"])[ns.in_cut(c)], minlength=c["nlocal"]))


def _system(parts, cm, corrections=False):
    P = orc.Particles(parts, cm)
    P.precompute(corrections=corrections)
    sp = parts["spec"]
    return P, P.poisson(sp.dt, parts["rho"], parts["v"])


@pytest.mark.parametrize("fx", ns.PADS_ONLY + [("pads_only", "small"), ("pads_only", "big")], ids=ns.ident)
def test_padding_and_order_are_inert_for_the_oracle(fx):
    """lists that were only padded and permuted: the oracle gives the pattern of the unedited list, values and right-hand
    side within 1e-12 of the largest, volumes within 1e-13 relative"""
    name, size = fx
    c, u, cm, notes = ns.pads_only(size) if name == "pads_only" else ns.fixture(name, size)
    assert notes["pads_only"]
    Pc, (rp, ci, val, b) = _system(c, cm)
    Pu, (rpu, ciu, valu, bu) = _system(u, cm)
    assert np.array_equal(rp, rpu) and np.array_equal(ci, ciu)
    dv = np.max(np.abs(val - valu)) / np.abs(valu).max()
    db = np.max(np.abs(b - bu)) / np.abs(bu).max()
    dvol = np.max(np.abs(Pc.vfrac - Pu.vfrac) / Pu.vfrac)
    print("\n%s-%s: values %.1e, b %.1e, volumes %.1e" % (name, size, dv, db, dvol))
    assert dv <= 1e-12 and db <= 1e-12 and dvol < 1e-13


@pytest.mark.parametrize("fx", ns.FIXTURES, ids=ns.ident)
def test_oracle_rows_are_merged_ascending_and_quick(fx):
    """the reference of the GPU suite: every row strictly ascending (duplicates merged) with its diagonal, the count
    regimes() predicts, and a run of under a second on the 2-D fixtures (the 3-D one has 4.4 times the entries: 5 s)"""
    name, size = fx
    c, u, cm, notes = ns.fixture(name, size)
    t0 = time.perf_counter()
    P, (rp, ci, val, b) = _system(c, cm)
    dt = time.perf_counter() - t0
    n = c["nlocal"]
    rows = ns.rows_of(rp)
    assert np.all(np.diff(ci)[np.diff(rows) == 0] > 0)
    assert np.array_equal(np.bincount(rows[ci == rows], minlength=n), np.ones(n, dtype=np.int64))
    assert len(ci) == ns.regimes(c, cm)["nnz"]
    print("\n%s-%s: oracle %.2f s, %d entries" % (name, size, dt, len(ci)))
    assert dt < (5.0 if name == "shuffled3d" else 1.0)


def test_own_image_rows_sum_to_zero_in_the_oracle():
    """thin_self: two in-cut entries of every row are the row particle's own periodic images (256 and 65 600 in all); the oracle adds them to the diagonal, and
    the constant vector stays in the null space: |A 1| <= 32 eps max|A| (rows of at most 28 terms, each rounded once)"""
    for size in ("small", "big"):
        c, u, cm, notes = ns.fixture("thin_self", size)
        assert ns.regimes(c, cm)["own_images"] == (256 if size == "small" else 65600)
        P, (rp, ci, val, b) = _system(c, cm)
        rows = ns.rows_of(rp)
        s = np.abs(np.bincount(rows, weights=val, minlength=c["nlocal"])).max() / np.abs(val).max()
        print("\nthin_self-%s: |A 1| / max|A| = %.1e" % (size, s))
        assert s <= 32 * np.finfo(float).eps
