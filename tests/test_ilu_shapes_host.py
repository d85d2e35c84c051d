"""Host side of the constructed block-ILU(k) fixtures (tests/ilu_shapes.py): every fixture that tests/test_gpu_ilu_shapes.py
hands to the device is checked HERE, without a GPU, for what it is meant to be -- deterministic, strictly diagonally dominant,
sorted, structurally nonsymmetric -- for the oracle's agreement with the long-double reference, and above all for the REGIME
it is named for: a fixture whose rows no longer reach the branch of csrc/ilu.hpp it was built for must fail in this file,
not pass silently on the device.

Regime table (ilu_shapes.regimes on the reference's factor pattern; f/s = factor / schedule template):

  fixture   K  wmax f/s            fast  dg>64  pivot>64 | WIDE: dg>64  pivot>128   widest level L/U (with a row of > 64 deps)
  narrow    0   128 narrow/narrow    55     92       453                            5/6
  w128      0   128 narrow/narrow    45     72       333                            5/6
  w129      0   129 wide/narrow                                     78          0   7/6    9 rows each of 128 lower / upper entries
  w130      0   130 wide/general                                    78        242   5/6    9 rows each of 129 lower / upper entries
  wide      0   261 wide/general                                   244        622   7/10
  fan       0   128 narrow/narrow     0    232       488                            256/256 (232/232)
  ragged    0   128 narrow/narrow   240    244       937                            17/15
  sub128    0   128 narrow/narrow   473    567      3767                            6/6
  one_wide  0   261 wide/general                                   161        389   7/10
  fill512   1    86 narrow/narrow   510      1        38   (pivot rows beyond 64 entries through fill alone)
  fill1024  1    95 narrow/narrow   977      1        69
  fill256   2   176 wide/general                                   133          0
  fill512   3   389 wide/general                                   297        400
  fill1024  3   714 wide/general                                   687        842

The oracle against the long-double reference on all of them: pattern exact; factor at most 1.6e-15 of max|f|, at most 4.1e-11
entrywise under the project's rule (relative, floor 1e-10 max|f|); application at most 1.1e-15."""
import numpy as np
import pytest

import oracle as orc
import ilu_shapes as sh

ILU0 = sh.ILU0_FIXTURES + ["sub128", "sub128c3", "one_narrow", "one_wide"]
CASES = [(name, 0) for name in ILU0] + [(name, k) for name in sh.ILUK_FIXTURES for k in (1, 2, 3)]

NARROW = dict(factor="narrow", schedule="narrow")
WIDE = dict(factor="wide", schedule="general")
AT_LEAST_8 = 8
# what each fixture is named for: strings and `exact` values must be equal, counts must reach the number given
NARROW_LADDER = dict(NARROW, exact=dict(wmax=128), fast=8, general_dg=8, general_pivot=8, L_65_128=8, U_65_128=8,
                     dg64=8, dg65=8, up64=8, up65=8)
WIDE_LADDER = dict(WIDE, wide_dg=8, wide_pivot=8, dg64=8, dg65=8, up64=8, up65=8, dg128=8, dg129=8, up128=8, up129=8,
                   L_65_128=8, U_65_128=8, L_gt128=8, U_gt128=8)
CONDITIONS = {
    ("narrow", 0): NARROW_LADDER,
    ("w128", 0): dict(NARROW, exact=dict(wmax=128), fast=8, general_dg=8, general_pivot=8),
    # WIDE factor kernel with the NARROW schedule: rows of 65..128 dependencies take the schedule's second column load
    ("w129", 0): dict(factor="wide", schedule="narrow", exact=dict(wmax=129), wide_dg=8, L_65_128=8, U_65_128=8, up64=8, up65=8,
                      dg128=8, up128=8, level0=dict(L_gt128=0, U_gt128=0)),
    # rows of 129 dependencies in one direction: one more than the NARROW schedule's two column loads per lane hold
    ("w130", 0): dict(WIDE, exact=dict(wmax=130), wide_dg=8, L_65_128=8, U_65_128=8, up64=8, up65=8, dg129=8, up129=8,
                      L_gt128=8, U_gt128=8),
    ("wide", 0): WIDE_LADDER,
    # in each direction a level of >= 130 rows (three runs of 64 ranks, the last one partial) with rows of > 64 dependencies
    ("fan", 0): dict(NARROW, exact=dict(wmax=128), general_dg=8, general_pivot=8, L_65_128=8, U_65_128=8, L_widest_level=130,
                     U_widest_level=130, L_widest_level_with_gt64=130, U_widest_level_with_gt64=130),
    ("ragged", 0): dict(NARROW_LADDER, blocks=(1, 63, 64, 65, 1024)),
    ("sub128", 0): dict(NARROW_LADDER, blocks=(128,), min_blocks=32),
    ("sub128c3", 0): dict(NARROW_LADDER, blocks=(128,), min_blocks=32),
    ("one_narrow", 0): dict(NARROW_LADDER, one_block=True),
    ("one_wide", 0): dict(WIDE_LADDER, one_block=True),
    # 64-row blocks: one wave walks both directions of the schedule's level walk
    ("fill64", 1): dict(NARROW, fast=8, blocks=(64,)), ("fill64", 2): dict(NARROW, fast=8), ("fill64", 3): dict(NARROW, fast=8),
    ("fill256", 1): dict(NARROW, fast=8, grown_past=64),
    ("fill256", 2): dict(WIDE, wide_dg=8, grown_past=128, L_65_128=8, U_65_128=8),
    ("fill256", 3): dict(WIDE, wide_dg=8, wide_pivot=8, grown_past=128, L_gt128=8, U_gt128=8),
    # the tail loop of the narrow template reached through fill alone
    ("fill512", 1): dict(NARROW, fast=8, general_pivot=8, grown_past=64, level0=dict(general_pivot=0, general_dg=0)),
    ("fill512", 2): dict(WIDE, wide_dg=8, wide_pivot=8, grown_past=128, L_gt128=8, U_gt128=8),
    ("fill512", 3): dict(WIDE, wide_dg=8, wide_pivot=8, grown_past=128, L_gt128=8, U_gt128=8),
    ("fill1024", 1): dict(NARROW, fast=8, general_pivot=8, grown_past=64, level0=dict(general_pivot=0, general_dg=0), blocks=(1024,)),
    ("fill1024", 2): dict(WIDE, wide_dg=8, wide_pivot=8, grown_past=128, L_gt128=8, U_gt128=8),
    ("fill1024", 3): dict(WIDE, wide_dg=8, wide_pivot=8, grown_past=128, L_gt128=8, U_gt128=8),
}


def check_conditions(cond, R, R0, bp):
    """cond: an entry of CONDITIONS; R: regimes of the factor; R0: regimes of the level-0 pattern of the same matrix"""
    for key, want in cond.items():
        if key == "exact":
            for k2, v in want.items():
                assert R[k2] == v, (k2, R[k2], v)
        elif key == "level0":
            for k2, v in want.items():
                assert R0[k2] == v, (k2, R0[k2], v)
        elif key == "grown_past":
            assert R0["wmax"] <= want < R["wmax"], (R0["wmax"], R["wmax"], want)
        elif key == "blocks":
            assert set(want) <= set(np.diff(bp).tolist()), (want, np.diff(bp))
        elif key == "min_blocks":
            assert len(bp) - 1 >= want
        elif key == "one_block":
            assert len(bp) == 2
        elif isinstance(want, str):
            assert R[key] == want, (key, R[key], want)
        else:
            assert want >= AT_LEAST_8 and R[key] >= want, (key, R[key], want)


def test_every_case_has_its_conditions():
    assert set(CONDITIONS) == set(CASES)


@pytest.mark.parametrize("name", sorted(sh.FIXTURES))
def test_fixture_is_deterministic_dominant_sorted_and_nonsymmetric(name):
    rp, ci, val, bp = sh.fixture(name)
    for a, b in zip(sh.FIXTURES[name](), (rp, ci, val, bp)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    n = len(rp) - 1
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and bp.dtype == np.int32 and val.dtype == np.float64
    assert bp[0] == 0 and bp[-1] == n and np.all(np.diff(bp) >= 1) and np.diff(bp).max() <= 1024
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert ci.min() >= 0 and ci.max() < n
    assert np.all(np.diff(ci)[np.diff(rows) == 0] > 0)                          # strictly ascending inside every row
    diag = ci == rows
    assert np.array_equal(np.bincount(rows[diag], minlength=n), np.ones(n, dtype=np.int64))
    off = np.bincount(rows[~diag], weights=np.abs(val[~diag]), minlength=n)
    assert np.all(np.abs(val[diag]) > off)                                     # strictly diagonally dominant
    neg = np.mean(val[diag] < 0)
    assert 0.1 < neg < 0.3 or n < 300 and 0.05 < neg < 0.4                     # about a fifth of the diagonals negative
    assert np.sum(val[~diag] > 0) > 0.4 * np.sum(~diag) and np.sum(val[~diag] < 0) > 0.4 * np.sum(~diag)
    blk = np.repeat(np.arange(len(bp) - 1), np.diff(bp))
    inb = (blk[rows] == blk[ci]) & ~diag
    if len(bp) > 2:
        assert np.sum(blk[rows] != blk[ci]) >= n // 2                          # columns that block Jacobi must drop
    keys = set((rows[inb].astype(np.int64) * n + ci[inb]).tolist())
    lone = sum(1 for r, c in zip(rows[inb].tolist(), ci[inb].tolist()) if c * n + r not in keys)
    assert lone > 0.25 * len(keys)                                             # structurally nonsymmetric, not by accident


@pytest.mark.parametrize("name,K", CASES)
def test_oracle_matches_long_double_reference_and_fixture_reaches_its_regime(name, K):
    rp, ci, val, bp = sh.fixture(name)
    n = len(rp) - 1
    frp, fci, fv = sh.ref_iluk_of(name, K)
    O = orc.ILU(rp, ci, val, K, bp)
    orp, oci, ov = O.export()
    assert np.array_equal(orp, frp) and np.array_equal(oci, fci)               # pattern: exact
    fmax = np.abs(fv).max()
    dev_max = float(np.max(np.abs(ov - fv)) / fmax)
    dev_entry = float(np.max(np.abs(ov - fv) / np.maximum(np.abs(fv), 1e-300 + 1e-10 * fmax)))
    r = np.random.default_rng(5).standard_normal(n)
    z = sh.ref_apply_of(name, K, r)
    dev_apply = float(np.linalg.norm(O.apply(r) - z) / np.linalg.norm(z))
    R = sh.regimes(frp, fci, bp, sh.matrix_wmax(rp) if K == 0 else None)
    print("\n%s K=%d: oracle vs long double: factor %.1e of max|f|, %.1e entrywise, apply %.1e\n  %s" %
          (name, K, dev_max, dev_entry, dev_apply, R))
    # double round-off of at most 1024 updates per entry / per solved row, each of relative size 1.1e-16, on factors of
    # diagonally dominant matrices (no growth): 1e-13.  The entrywise figure: see the note on the seeds in ilu_shapes.py
    assert dev_max <= 1e-13 and dev_apply <= 1e-13
    assert dev_entry <= 0.5e-10
    if K == 0:   # ILU(0) dispatches on the matrix' longest row: it must be the factor's, or regimes() describes another kernel
        assert sh.matrix_wmax(rp) == int(np.diff(frp).max())
        R0 = R
    else:
        f0 = sh.ref_iluk_of(name, 0)
        R0 = sh.regimes(f0[0], f0[1], bp)
        assert frp[-1] > f0[0][-1]
    check_conditions(CONDITIONS[(name, K)], R, R0, bp)


def test_one_pass_factorisation_is_not_the_reference():
    """the numeric pass runs on the FINAL pattern: a factorisation that inserts fill while it eliminates skips the updates
    of entries whose level only drops to K at a later pivot, and is 1e-3 away -- the reference must not be that one"""
    rp, ci, val, bp = sh.fixture("fill256")
    frp, fci, fv = sh.ref_iluk_of("fill256", 2)
    lo, hi = int(bp[0]), int(bp[1])
    W, P = sh._block_dense(rp, ci, val, lo, hi)
    m, K, big = hi - lo, 2, 1 << 20
    lev = np.where(P, 0, big)
    for i in range(m):                                   # dynamic insertion: update only what is in the pattern so far
        for k in range(i):
            if lev[i, k] > K:
                continue
            W[i, k] /= W[k, k]
            nl = lev[i, k] + lev[k, k + 1:] + 1
            have = lev[i, k + 1:] <= K
            take = have | (nl <= K)
            W[i, k + 1:] = np.where(take, np.where(have, W[i, k + 1:], 0) - W[i, k] * W[k, k + 1:], W[i, k + 1:])
            lev[i, k + 1:] = np.where(take, np.minimum(lev[i, k + 1:], nl), lev[i, k + 1:])
    sel = np.arange(frp[lo], frp[hi])
    rows = np.repeat(np.arange(lo, hi), np.diff(frp[lo:hi + 1]))
    assert np.array_equal(lev <= K, sh._symbolic(P, K))                        # same pattern ...
    one_pass = W[rows - lo, fci[sel] - lo]
    assert np.max(np.abs(one_pass - fv[sel])) / np.abs(fv[sel]).max() > 1e-6    # ... other values


def test_regimes_notice_a_table_without_long_pivot_rows():
    """the tail loop of the narrow template needs pivot rows of more than 64 upper entries: without the four table entries
    that make them the condition of the narrow ladder trips"""
    table = [t for t in sh.TAB_N if t not in ((5, 70), (62, 65), (27, 100), (0, 127))]
    rp, ci, val, bp = sh.ladder([256, 256, 100], table)
    frp, fci, fv = sh.ref_iluk(rp, ci, val, bp, 0)
    R = sh.regimes(frp, fci, bp, sh.matrix_wmax(rp))
    assert R["general_pivot"] == 0 and R["fast"] > 0
    with pytest.raises(AssertionError):
        check_conditions(CONDITIONS[("narrow", 0)], R, R, bp)


@pytest.mark.parametrize("fill", [0, 1])
def test_overlap_rows_are_one_directional_and_the_schwarz_oracle_matches_the_reference(fill):
    """the overlap fixture of tests/test_gpu_ilu_shapes.py: the oracle's extended row lists equal the plain restatement
    (rows referenced BY the subdomain's columns; a row that only references the subdomain stays outside), and its factors
    of every third extended subdomain equal the long-double ones"""
    rp, ci, val, bp = sh.fixture("sub128c3")
    n = len(rp) - 1
    rows, lp = sh.extended_rows(rp, ci, bp, 1)
    S = orc.Schwarz(rp, ci, val, fill, bp, 1, "add")
    orow, olp, orp, oci, ov = S.export()
    assert np.array_equal(orow, rows) and np.array_equal(olp, lp)
    r_of = np.repeat(np.arange(n), np.diff(rp))
    blk = np.repeat(np.arange(len(bp) - 1), np.diff(bp))
    worst = 0.0
    for s in range(0, len(bp) - 1, 3):
        mine = rows[lp[s]:lp[s + 1]]
        ext = mine[bp[s + 1] - bp[s]:]
        assert np.all(np.diff(ext) > 0) and len(ext) >= 128
        refs_in = np.unique(r_of[(blk[ci] == s) & (blk[r_of] != s)])      # rows outside that reference the subdomain
        assert len(np.setdiff1d(refs_in, ext)) >= 64                     # ... and were not pulled in: one direction only
        lrp, lci, lv = sh.local_matrix(rp, ci, val, mine)
        frp, fci, fv = sh.ref_iluk(lrp, lci, lv, np.array([0, len(mine)], dtype=np.int32), fill)
        a, b = orp[lp[s]], orp[lp[s + 1]]
        assert np.array_equal(orp[lp[s]:lp[s + 1] + 1] - a, frp) and np.array_equal(oci[a:b] - lp[s], fci)
        worst = max(worst, float(np.max(np.abs(ov[a:b] - fv) / np.maximum(np.abs(fv), 1e-300 + 1e-10 * np.abs(ov).max()))))
    print("\noverlap 1, fill %d: oracle vs long double entrywise %.1e" % (fill, worst))
    assert worst <= 0.5e-10
