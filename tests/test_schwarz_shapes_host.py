"""Host side of the constructed additive-Schwarz fixtures (tests/schwarz_shapes.py): every fixture that
tests/test_gpu_schwarz_shapes.py hands to the device is checked HERE, without a GPU, for what it is meant to be --
deterministic, strictly diagonally dominant, sorted -- for the oracle's agreement with the long-double reference, and for
the REGIME it is named for (schwarz_shapes.model on the reference's factor pattern): a fixture that no longer reaches the
branch of csrc/schwarz.hpp it was built for fails in this file, and on the device against M.paths().

Regime table (fill 0; form 2 = one workgroup per subdomain, 1 = persistent launches, 0 = one launch per level;
near / far = rows on which one 16-lane sub-lane holds more than 6 dependencies inside its run / within 128 positions before it):

  fixture        rows  form long_rows waves hbits  what it reaches
  comb_near      1024   1      1        1     8    near-list overflow loop: 35 rows in L, 36 in U (7 per sub-lane); rows of two chunks
  comb_far       1024   1      1        1    11    far-list overflow loop: 48 rows in L, 57 in U (up to 32 per sub-lane); near overflow
                                                   with up to 15 per sub-lane; rows of 7 chunks
  fan             512   1      1        1     8    levels of 232 and 256 rows cut across runs of 64 positions (2 cut levels a direction)
  short96         400   1      0        1     8    SPLIT = false kernels: no row beyond 96 entries on a side
  short97lo       400   1      0        1     8    20 rows of 97 on a side: 20 * 20 = 400 is not > 400, SPLIT = false with rows of two chunks
  short97hi       400   1      1        1     8    21 rows of 97: SPLIT = true
  dense_upper64   400   1      1        1    10    (nnz - n) / 2 / n = 64: k_gilu_factor_sf<1>, pivot rows of 300 upper entries
  dense_upper     400   1      1        4    10    one entry more, 65: k_gilu_factor_sf<4>, pivot rows beyond one round of 256 threads
  row2048        2304   1      0        1    12    longest row 2048: the hash table still fits 64 KiB
  row2049        2304   1      0        1     0    longest row 2049: binary search
  row5000        5200   1      0        1     0    longest row 5000: the largest row image
  row5001        5200   refused                    "row exceeds the LDS row image"
  wide4095       8190   1      0        1     2    two levels of 4095 rows, each cut into 64 runs (128 runs a direction)
  wide4096       8192   0                          4096 rows per level: level launches although not asked for
  subs31         3968   1                          31 subdomains of 128 rows (overlap 0 and 1): not the one-workgroup form
  subs32         4096   2                          32 subdomains: one workgroup each, row lists built on the device
  ext4096        4096   2                          overlap 1: subdomain 0 extends to exactly 4096 rows, lists built on the device
  ext4097        4224   1                          overlap 1: 4097 rows, the capacity flag is raised, lists built on the host
  ext0_1         4096   2                          overlap 1: subdomain 3 has no outside column, subdomain 4 exactly one (bitonic sort, np = 1)
  ext_collide   16384   2                          overlap 1: subdomain 0's outside columns share buckets of the 13-bit set, wrap past slot 8191
  subrow1024     4096   2                          overlap 1: longest factor row 1024 in the one-workgroup factorisation, 127 pivots,
                                                   pivot rows of 100 upper entries
  subrow1025     4096   1 (overlap 1)              a matrix row of 1025: host set-up; overlap 1: factor row 1025, not the one-workgroup form
  fill 1:
  sym1023        1200   1      1        1    11    level-1 pattern of the last row 1023 entries: built on the device
  sym1024        1200   1      1        1    11    1024 entries: the device table gives up, built on the host
  sym_collide    8192   1      0        1     9    the last row's keys share buckets of the 11-bit table and wrap past slot 2047
  nodiag1_dev     256   1      0        1     8    a row without stored diagonal, its pivot from fill alone: device pattern kernel
  nodiag1_host   1200   1      1        1    11    the same kind of row beside the 1024-entry one: host routine
  refusals: a stored 0.0 pivot in the three factorisation forms, a row without diagonal at fill 0 in both set-ups

The oracle in plain double against the long-double reference on all of them: row lists and pattern exact; factor at most
3.3e-11 entrywise under the project's rule (relative, floor 1e-10 max|f|; subs31 and subs32, seed 9 of ilu_shapes' sub128);
application at most 4.6e-16 (measured, printed by the tests; half the device bounds of 1e-10 and 1e-11 are required).
The device on the same fixtures (MI355X, tests/test_gpu_schwarz_shapes.py): factor at most 2.6e-11, application 2.4e-16.

A row without a stored diagonal: oracle/isph_oracle.c inserts it at every level of fill (ilu_symbolic, "structurally
missing diagonal: insert"); the library inserts it for fill >= 1 and refuses the matrix at fill 0."""
import numpy as np
import pytest

import oracle as orc
import ilu_shapes as sh
import schwarz_shapes as ss

CASES = ss.CASES
AT_LEAST_8 = 8
# what each fixture is named for: `exact` values must be equal, the other counts must reach the number given
CONDITIONS = {
    ("comb_near", 0, 0): dict(exact=dict(persistent=1, long_rows=1, chunks_max_l=2, chunks_max_u=2, near_max_l=7, near_max_u=7),
                           near_overflow_rows_l=8, near_overflow_rows_u=8, rows_2chunks_l=8, rows_2chunks_u=8),
    ("comb_far", 0, 0): dict(exact=dict(persistent=1, long_rows=1, chunks_max_l=7, chunks_max_u=7),
                          far_overflow_rows_l=8, far_overflow_rows_u=8, near_overflow_rows_l=8, near_overflow_rows_u=8),
    ("fan", 0, 0): dict(exact=dict(persistent=1, widest_level_l=256, widest_level_u=256, cut_levels_l=2, cut_levels_u=2)),
    ("short96", 0, 0): dict(exact=dict(persistent=1, long_rows=0, max_side=96, rows_gt96=0, nloc=400)),
    ("short97lo", 0, 0): dict(exact=dict(persistent=1, long_rows=0, max_side=97, rows_gt96=20, nloc=400), rows_2chunks_l=8, rows_2chunks_u=8),
    ("short97hi", 0, 0): dict(exact=dict(persistent=1, long_rows=1, max_side=97, rows_gt96=21, nloc=400)),
    ("dense_upper64", 0, 0): dict(exact=dict(persistent=1, mean_upper=64, factor_waves=1, nnz=131 * 400 - 1), max_upper=257),
    ("dense_upper", 0, 0): dict(exact=dict(persistent=1, mean_upper=65, factor_waves=4, nnz=131 * 400), max_upper=257),
    ("row2048", 0, 0): dict(exact=dict(persistent=1, maxrow=2048, hbits=12, factor_waves=1)),
    ("row2049", 0, 0): dict(exact=dict(persistent=1, maxrow=2049, hbits=0, factor_waves=1)),
    ("row5000", 0, 0): dict(exact=dict(persistent=1, maxrow=5000, hbits=0, refused=False)),
    ("wide4095", 0, 0): dict(exact=dict(persistent=1, nloc=8190, levels_l=2, levels_u=2, widest_level_l=4095, widest_level_u=4095,
                                     nrun_l=128, nrun_u=128, cut_levels_l=2, cut_levels_u=2)),
    ("wide4096", 0, 0): dict(exact=dict(persistent=0, nloc=8192, levels_l=2, levels_u=2)),
    ("subs31", 0, 0): dict(exact=dict(persistent=1, nsub=31, sub_maxrows=128, rows_on_device=0)),
    ("subs31", 0, 1): dict(exact=dict(persistent=1, nsub=31, rows_on_device=0)),
    ("subs32", 0, 0): dict(exact=dict(persistent=2, nsub=32, sub_maxrows=128, rows_on_device=1)),
    ("subs32", 0, 1): dict(exact=dict(persistent=2, nsub=32, rows_on_device=1)),
    ("ext4096", 0, 0): dict(exact=dict(persistent=2, nsub=32, rows_on_device=1)),
    ("ext4096", 0, 1): dict(exact=dict(persistent=2, nsub=32, sub_maxrows=4096, rows_on_device=1)),
    ("ext4097", 0, 0): dict(exact=dict(persistent=2, nsub=33, rows_on_device=1)),
    ("ext4097", 0, 1): dict(exact=dict(persistent=1, nsub=33, sub_maxrows=4097, rows_on_device=0)),
    ("ext0_1", 0, 0): dict(exact=dict(persistent=2, rows_on_device=1)),
    ("ext0_1", 0, 1): dict(exact=dict(persistent=2, rows_on_device=1)),
    ("ext_collide", 0, 0): dict(exact=dict(persistent=2, rows_on_device=1)),
    ("ext_collide", 0, 1): dict(exact=dict(persistent=2, rows_on_device=1)),
    ("subrow1024", 0, 0): dict(exact=dict(persistent=2, rows_on_device=1)),
    # the one-workgroup factorisation on a row of 1024 entries, 127 pivots, pivot rows of 100 upper entries
    ("subrow1024", 0, 1): dict(exact=dict(persistent=2, rows_on_device=1, maxrow=1024), max_lower=65, max_upper=65),
    ("subrow1025", 0, 0): dict(exact=dict(persistent=2, rows_on_device=0)),       # a matrix row of 1025: host set-up
    ("subrow1025", 0, 1): dict(exact=dict(persistent=1, rows_on_device=0, maxrow=1025)),
    ("sym1023", 1, 0): dict(exact=dict(persistent=1, symbolic1_on_device=1, maxrow=1023)),
    ("sym1024", 1, 0): dict(exact=dict(persistent=1, symbolic1_on_device=0, maxrow=1024)),
    ("sym_collide", 1, 0): dict(exact=dict(persistent=1, symbolic1_on_device=1)),
    ("nodiag1_dev", 1, 0): dict(exact=dict(persistent=1, symbolic1_on_device=1)),
    ("nodiag1_host", 1, 0): dict(exact=dict(persistent=1, symbolic1_on_device=0, maxrow=1024)),
}


def check_conditions(cond, R):
    for key, want in cond.items():
        if key == "exact":
            for k2, v in want.items():
                assert R[k2] == v, (k2, R[k2], v)
        else:
            assert want >= AT_LEAST_8 and R[key] >= want, (key, R[key], want)


def entrywise(gv, fv):
    fmax = np.abs(fv).max()
    return float(np.max(np.abs(gv - fv) / np.maximum(np.abs(fv), 1e-300 + 1e-10 * fmax)))


def own_ptr(name):
    n, B = len(ss.fixture(name)[0]) - 1, ss.block_size(name)
    return None if B == 0 else np.array(list(range(0, n, B)) + [n], dtype=np.int32)


def test_every_case_has_its_conditions():
    assert set(CONDITIONS) == set(CASES)


@pytest.mark.parametrize("name", sorted(ss.FIXTURES))
def test_fixture_is_deterministic_dominant_and_sorted(name):
    rp, ci, val, bp = ss.fixture(name)
    for a, b in zip(ss.FIXTURES[name][0](), (rp, ci, val, bp)):
        assert np.asarray(a).dtype == b.dtype and np.array_equal(a, b)
    n = len(rp) - 1
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and val.dtype == np.float64
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert ci.min() >= 0 and ci.max() < n
    assert np.all(np.diff(ci)[np.diff(rows) == 0] > 0)                          # strictly ascending inside every row
    diag = ci == rows
    have = np.bincount(rows[diag], minlength=n) == 1
    assert np.sum(~have) == (1 if name.startswith("nodiag") else 0)            # nodiag1: ONE row without a stored diagonal
    off = np.bincount(rows[~diag], weights=np.abs(val[~diag]), minlength=n)
    assert np.all(np.abs(val[diag]) > off[have])                               # strictly diagonally dominant
    assert 0.1 < np.mean(val[diag] < 0) < 0.3                                  # about a fifth of the diagonals negative
    assert np.sum(val[~diag] > 0) > 0.4 * np.sum(~diag) and np.sum(val[~diag] < 0) > 0.4 * np.sum(~diag)
    keys = set((rows[~diag].astype(np.int64) * n + ci[~diag]).tolist())
    lone = sum(1 for r, c in zip(rows[~diag].tolist(), ci[~diag].tolist()) if c * n + r not in keys)
    assert lone > 0.25 * len(keys)                                             # structurally nonsymmetric


@pytest.mark.parametrize("name,K,overlap", CASES)
def test_oracle_matches_long_double_reference_and_fixture_reaches_its_regime(name, K, overlap):
    rp, ci, val, bp = ss.fixture(name)
    n = len(rp) - 1
    rows, lp, frp, fci, fv, subs = ss.ref_schwarz_of(name, K, overlap)
    R = ss.model(frp, fci, lp, fill=K, wmax=int(np.diff(rp).max()))
    worst_apply = 0.0
    r = np.random.default_rng(5).standard_normal(n)
    for combine in ("add", "zero") if overlap else ("add",):
        O = orc.Schwarz(rp, ci, val, K, own_ptr(name), overlap, combine)
        orow, olp, orp, oci, ov = O.export()
        assert np.array_equal(orow, rows) and np.array_equal(olp, lp)          # row lists: exact
        assert np.array_equal(orp, frp) and np.array_equal(oci, fci)           # pattern: exact
        z = ss.ref_apply((rows, lp, frp, fci, fv, subs), combine, r)
        worst_apply = max(worst_apply, float(np.linalg.norm(O.apply(r) - z) / np.linalg.norm(z)))
    dev_entry = entrywise(ov, fv)
    print("\n%s fill %d overlap %d: oracle vs long double: factor %.1e entrywise, apply %.1e\n  %s" % (name, K, overlap, dev_entry, worst_apply, R))
    assert dev_entry <= 0.5e-10 and worst_apply <= 0.5e-11                     # half the device bounds
    # the model against what does not come from it: the oracle's factor and the level recurrence of ilu_shapes
    assert R["nnz"] == len(oci) and R["maxrow"] == int(np.diff(orp).max()) and R["nloc"] == len(orow)
    assert R["levels_l"] == int(sh._levels(len(orp) - 1, orp, oci, 0).max()) + 1
    assert R["levels_u"] == int(sh._levels(len(orp) - 1, orp, oci, 1).max()) + 1
    check_conditions(CONDITIONS[(name, K, overlap)], R)


def test_sparse_reference_is_the_dense_one():
    """the row-wise reference of schwarz_shapes and the dense one of ilu_shapes: same operations, same long-double bits"""
    rp, ci, val, bp = sh.fixture("fan")
    frp, fci, fv = sh.ref_iluk_of("fan", 0)
    ref = ss.ref_schwarz_of("fan", 0, 0)
    assert np.array_equal(ref[2], frp) and np.array_equal(ref[3], fci) and np.array_equal(ref[4], fv)
    r = np.random.default_rng(5).standard_normal(len(rp) - 1)
    assert np.max(np.abs(ss.ref_apply(ref, "add", r) - sh.ref_apply_of("fan", 0, r))) <= 1e-17 * np.abs(r).max()


def test_row5001_is_over_the_gate_and_row5000_is_not():
    for name, refused in (("row5000", False), ("row5001", True)):
        rp, ci, val, bp = ss.fixture(name)
        R = ss.model(rp, ci, np.array([0, len(rp) - 1]))
        assert R["maxrow"] == int(name[3:]) and R["refused"] == refused and R["persistent"] == 1


def test_model_notices_a_comb_that_fits_the_near_list():
    """a window of 96 ids holds 6 chain rows: the near list takes them all, no row reaches the overflow loop, and the
    condition of comb_near trips"""
    rp, ci, val, bp = ss.comb(96)
    R = ss.model(rp, ci, np.array([0, len(rp) - 1]))
    assert R["near_max_l"] == 6 and R["near_overflow_rows_l"] == 0
    with pytest.raises(AssertionError):
        check_conditions(CONDITIONS[("comb_near", 0, 0)], R)


def test_sym_edge_has_one_row_on_the_capacity_of_the_device_table():
    """k_gilu_symbolic1 gives a row up once its set reaches 1024 keys: 1023 stays on the device, 1024 goes to the host, and
    no other row of the two fixtures comes near"""
    for name, size in (("sym1023", 1023), ("sym1024", 1024)):
        rp, ci, val, bp = ss.fixture(name)
        lens = np.sort([len(c) for c in ss.ref_pattern(rp, ci, 1)])
        assert lens[-1] == size and lens[-2] < 700 and int(np.diff(rp).max()) < ss.SYM_CAP // 2


@pytest.mark.parametrize("name,bits,row", [("sym_collide", 11, 8191), ("ext_collide", 13, None)])
def test_collide_fixtures_share_buckets_and_wrap_round_the_table(name, bits, row):
    """the keys one workgroup (ext_collide: subdomain 0's outside columns) or one wave (sym_collide: the last row's level-1
    pattern) puts into its open-addressing table: more keys whose home is one of the last 8 slots than those slots hold
    (the chain wraps past the last slot whatever the order of insertion) and buckets with several keys"""
    rp, ci, val, bp = ss.fixture(name)
    if row is None:
        keys = np.setdiff1d(np.unique(ci[rp[0]:rp[128]]), np.arange(128))
    else:
        keys = ss.ref_pattern(rp, ci, 1)[row]
    h = ss.knuth(keys, bits).astype(np.int64)
    size = 1 << bits
    assert size == (ss.SYM_CAP if row is not None else ss.SUB_HASH)
    assert np.sum(h >= size - 8) >= 12 and np.sum(h < 16) >= 16
    assert np.bincount(h, minlength=size).max() >= 3


def test_ext0_1_has_a_subdomain_without_and_one_with_a_single_outside_column():
    rp, ci, val, bp = ss.fixture("ext0_1")
    rows, lp = sh.extended_rows(rp, ci, np.arange(0, len(rp), 128, dtype=np.int32), 1)
    sizes = np.diff(lp)
    assert sizes[3] == 128 and sizes[4] == 129 and np.all(np.delete(sizes, [3, 4]) > 200)


@pytest.mark.parametrize("name", ["nodiag1_dev", "nodiag1_host"])
def test_nodiag1_pivot_comes_from_fill_and_the_oracle_inserts_the_diagonal(name):
    rp, ci, val, bp = ss.fixture(name)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    z = int(np.flatnonzero(np.bincount(rows[ci == rows], minlength=n) == 0)[0])
    frp, fci, fv, fdg = ss.ref_schwarz_of(name, 1, 0)[5][0][2]
    assert fci[frp[z] + fdg[z]] == z and abs(fv[frp[z] + fdg[z]]) > 0.05       # inserted, and nonzero through fill
    orp, oci, ov = orc.ILU(rp, ci, val, 1, np.array([0, n], dtype=np.int32)).export()
    assert np.array_equal(orp, frp) and np.array_equal(oci, fci)
    with pytest.raises(ValueError):
        ss.ref_pattern(rp, ci, 0)                                              # fill 0: no diagonal, no pivot


@pytest.mark.parametrize("label", sorted(ss.REFUSALS))
def test_refusal_fixtures_are_what_they_say(label):
    make, B, level_launches, text = ss.REFUSALS[label]
    rp, ci, val, bp = make()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    diag = ci == rows
    have = np.bincount(rows[diag], minlength=n)
    if "zero_pivot" in label:
        z = int(np.flatnonzero(val[diag] == 0.0)[0])
        assert np.sum(val[diag] == 0.0) == 1 and have.all()
        lo, hi = (0, n) if B == 0 else (z // B * B, z // B * B + B)
        c = ci[rp[z]:rp[z + 1]]
        assert not np.any((c >= lo) & (c < z))                                 # level 0: no lower entry in its subdomain
        assert np.sum(ci == z) == 1                                            # no other row references it
        assert B == 0 or n // B >= ss.SUB_MIN_SUBS                             # the one-workgroup form
    elif "nodiag" in label:
        assert np.sum(have == 0) == 1 and (B == 0 or n // B >= ss.SUB_MIN_SUBS)
        # the oracle inserts the diagonal (Ifpack_IlukGraph): one entry more than the matrix has
        assert orc.ILU(rp, ci, val, 0, np.array([0, n], dtype=np.int32)).export()[0][-1] == len(ci) + 1
    else:
        assert int(np.diff(rp).max()) == ss.MAX_ROW + 1
