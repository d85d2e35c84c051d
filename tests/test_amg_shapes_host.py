"""-m "not gpu": the constructed graphs of tests/amg_shapes.py land in the regimes they claim, the restatement agrees with
itself (greedy roots == rounds, with and without the device's same-round shortcut) and with the oracle, and every
mutation a wrong kernel could make moves a compared quantity beyond its bound.

Oracle against restatement: aggregates and patterns equal, values within 4 k eps sum|terms| as far as the hierarchy
is decided beyond rounding (Hierarchy.decided).  The oracle's strength test at threshold 0 was a * a > 0, which drops an
entry of 1e-170 the device keeps (a != 0, AMG_STRONG); STRONG in oracle/isph_amg_oracle.c now follows the device's
documented rule, and edge_tiny_offdiag pins it.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import oracle as orc
import amg_shapes as S

ALL = sorted(S.FIXTURES)
THETAS = [(n, 0.0) for n in ALL] + [(n, S.THETA) for n in S.THETA_FIXTURES]


_gap = S.gap          # the value comparison of the GPU test


# ---------------------------------------------------------------- regimes
@pytest.mark.parametrize("name", ALL)
def test_fixture_lands_where_it_claims(name):
    H = S.fixture_reference(name)
    claim = S.FIXTURES[name][2]
    assert H.refusal is None and len(H.levels) >= 2
    assert {k: H.levels[0].path[k] for k in claim} == claim
    (rp, ci, v), nv, prm = S.fixture(name)
    assert S.regimes(rp, ci, v, prm, nv) == [L.path for L in H.levels]


def test_both_sides_of_every_threshold():
    p0 = lambda name: S.fixture_reference(name).levels[0]
    # prolongator rows: kProlong16 | +1, kProlong64 | +1, slot 7 of k_prolong (448 | 449), 64 * kProlongSlots | +1 (refusal)
    assert [p0("hub_%d" % k).p_widest for k in (16, 17, 64, 65, 448, 449, 512)] == [16, 17, 64, 65, 448, 449, 512]
    assert [p0("hub_%d" % k).path["prolong"] for k in (16, 17, 64, 65, 512)] == [16, 64, 64, 2, 2]
    H = S.fixture_reference("hub_513")
    assert H.refusal == S.REFUSED["hub_513"][2] and H.levels[0].p_widest == 513
    with pytest.raises(S.Refused, match="512 aggregates"):
        (rp, ci, v), nv, prm = S.fixture("hub_513")
        S.regimes(rp, ci, v, prm, nv)
    # A P: 64 | 65, 256 | 257, 1024 | 1025 distinct columns in the widest row
    names = ("hub_64", "hub_65", "hub_256", "hub_257", "hubs_3x341", "hubs_4x256")
    assert [p0(n).ap_widest for n in names] == [64, 65, 256, 257, 1024, 1025]
    assert [p0(n).path["ap"] for n in names] == [1, 2, 2, 4, 4, 5]
    # Galerkin product: kGalerkinTable coarse columns | more
    lo, hi = S.fixture_reference("long_chain_14700"), S.fixture_reference("long_chain_15200")
    assert lo.levels[1].n <= S.kGalerkinTable < hi.levels[1].n < S.kGalerkinTable + 128
    assert (lo.levels[0].path["galerkin"], hi.levels[0].path["galerkin"]) == (1, 2)
    # dense smoother blocks | the chunk stream on a coarse level: kSgsDenseMaxRows
    lo, hi = S.fixture_reference("long_chain_118000"), S.fixture_reference("long_chain_120000")
    assert lo.levels[1].n <= S.kSgsDenseMaxRows < hi.levels[1].n < S.kSgsDenseMaxRows + 512
    assert (lo.levels[1].path["smoother"], hi.levels[1].path["smoother"]) == (1, 2)
    assert lo.levels[1].path["coarse"] == hi.levels[1].path["coarse"] == 2          # more than kAmgDenseMax rows
    # direct solve | smoother on the coarsest level: kAmgDenseMax
    assert max(S.DENSE_SIZES) == S.kAmgDenseMax
    assert S.reference(*S.chain(S.kAmgDenseMax + 1), dict(max_levels=1)).levels[0].path["coarse"] == 2
    assert S.reference(*S.chain(S.kAmgDenseMax), dict(max_levels=1)).levels[0].path["coarse"] == 1
    # ... and below a coarsening step: the coarsest level of a 2-level hierarchy on kAmgDenseMax | + 1 rows
    lo, hi = S.fixture_reference("islands_2048"), S.fixture_reference("islands_2049")
    assert (lo.levels[1].n, hi.levels[1].n) == (S.kAmgDenseMax, S.kAmgDenseMax + 1)
    assert (lo.levels[1].path["coarse"], hi.levels[1].path["coarse"]) == (1, 2)
    assert (lo.levels[1].path["smoother"], hi.levels[1].path["smoother"]) == (0, 1)
    # the per-lane walk of k_spgemm_rows (more than kOwnCap products behind 64 entries) whose product is kept
    L = p0("shared_hubs_40x64")
    assert L.ap_round_products > S.kOwnCap and L.ap_widest <= S.kSpgemmRows64 and L.path["ap"] == 1
    assert all(p0(n).ap_round_products <= S.kOwnCap for n in ("hub_64", "grid_21x13", "chain_257"))
    # ragged last smoother block, ragged wave groups
    rows = sorted({L.n for name in ALL for L in S.fixture_reference(name).levels})
    for mod in (4, 16, 64):
        assert {0, 1, mod - 1} <= {n % mod for n in rows}, mod


def test_work_lists_and_the_mark_buffer():
    st = S.fixture_reference("star_1100").levels[0]
    # round 1 runs on a work list of ONE row, which brings kMarkBuf + 77 fresh rows: the flush inside a row
    assert st.stats["undecided"] == [1, 0] and st.path["mis_list_rounds"] == 1
    assert st.stats["mark_rows"] == [1101] and st.stats["mark_rows"][0] > S.kMarkBuf + 64
    # work-list rounds of different depth, and full sweeps after round 0 (more than n / 4 undecided)
    lists = {name: S.fixture_reference(name).levels[0].path for name in ALL}
    assert {p["mis_list_rounds"] for p in lists.values()} >= {0, 1, 2, 3}
    assert any(p["mis_rounds"] - 1 > p["mis_list_rounds"] for p in lists.values())
    # the staircases: a prescribed number of rounds, all but the first on work lists; the plain rounds need two per triple
    for name, length in (("staircase_12x4", 12), ("staircase_31x2", 31)):
        L = S.fixture_reference(name).levels[0]
        rounds = -(-length // 3)
        assert (L.path["mis_rounds"], L.path["mis_list_rounds"]) == (rounds, rounds - 1)
        assert len(L.stats["undecided_plain"]) >= 2 * rounds - 1
    # ... every round of which the shortcut helps to decide (the device needs half the plain rounds)
    for name in ("staircase_12x4", "staircase_31x2"):
        L = S.fixture_reference(name).levels[0]
        assert len(L.stats["shortcut_decided"]) == L.path["mis_rounds"]
        assert all(k > 0 for k in L.stats["shortcut_decided"][:-1])
    # the waiting staircases: after round 0 every round is a work-list round that leaves rows undecided or finishes, and
    # NONE of them is decided by the shortcut -- rows wait behind a row that is only being covered (the `else und = true`
    # branch of k_mis_decide_list) and are decided by the ordinary rules one round later
    for name, und in (("waiting_path7x3", [6, 3, 0]), ("waiting_tree24x2", [20, 8, 4, 2, 0])):
        L = S.fixture_reference(name).levels[0]
        assert L.stats["undecided"] == und
        assert (L.path["mis_rounds"], L.path["mis_list_rounds"]) == (len(und), len(und) - 1)
        assert L.stats["shortcut_decided"][0] > 0 and not any(L.stats["shortcut_decided"][1:])
        # the shortcut saves no round here (on the descending staircases it halves them); the roots are the greedy ones
        assert len(L.stats["undecided_plain"]) == len(und)
        assert L.stats["greedy_equals_rounds"] and L.stats["pass3_rows"] == 0
    L = S.fixture_reference("star_1100").levels[0]
    assert L.path["mis_list_rounds"] == 1 and L.stats["shortcut_decided"][1] == 0 and L.stats["undecided"] == [1, 0]
    # the same-round shortcut saves rounds somewhere (the only step the oracle does not share) and not everywhere
    saved = [len(L.stats["undecided_plain"]) - len(L.stats["undecided"])
             for name in ALL for L in S.fixture_reference(name).levels if L.agg is not None]
    assert min(saved) >= 0 and len(set(saved)) > 1


@pytest.mark.parametrize("name,theta", THETAS)
def test_greedy_roots_equal_the_rounds_and_pass3_is_never_reached(name, theta):
    H = S.fixture_reference(name, theta)
    for L in H.levels:
        if "pass3_rows" in L.stats:
            assert L.stats["greedy_equals_rounds"]
            assert L.stats["pass3_rows"] == 0


def test_aggregation_edges_are_present():
    st = lambda name, l=0: S.fixture_reference(name).levels[l].stats
    assert st("unsymmetric_150")["pass1_two_roots"] > 0
    for name in ("chain_257", "grid_21x13", "unsymmetric_150", "hub_16"):
        assert st(name)["pass2_ties"] > 0
    assert st("edge_empty")["isolated"] == 4 and st("edge_diag_only")["isolated"] == 4
    assert st("edge_tiny_offdiag")["isolated"] == 0 and st("edge_zero_offdiag")["isolated"] == 2
    # with a threshold the 1e-170 entry is weak (its square underflows to 0): the opposite of the threshold-0 rule
    assert S.fixture_reference("edge_tiny_offdiag", S.THETA).levels[0].stats["isolated"] == 4
    L = S.fixture_reference("edge_no_diag").levels[0]
    L.diagonal()
    assert np.count_nonzero(~L.has_diag) == 4 and np.all(L.diagonal()[~L.has_diag] == 1.0)
    L = S.fixture_reference("edge_zero_diag").levels[0]
    assert np.count_nonzero(L.diagonal() == 0.0) == 4
    # a masked null vector: zero columns of P, rows of explicit zeros with a stored zero pivot on level 1
    H = S.fixture_reference("masked_grid_21x13")
    L1 = H.levels[1]
    zero_rows = np.flatnonzero(np.asarray(H.nv[1]) == 0.0)
    assert len(zero_rows) >= 4 and H.coarse_smooth
    A1 = L1.csr()
    assert all(A1[i, i] == 0.0 and A1[i].nnz > 0 and not A1[i].data.any() for i in zero_rows)
    # aggregate counts on 2^k - 1 and 2^k with rows outside every aggregate (the key bits of the member sort)
    counts = {(L.nagg, L.stats["unaggregated"] > 0) for name in ALL for L in S.fixture_reference(name).levels if L.agg is not None}
    assert {(15, True), (16, True), (255, True), (256, True)} <= counts


@pytest.mark.parametrize("name", S.THETA_FIXTURES)
def test_strength_tests_keep_a_factor_two_from_equality(name):
    (rp, ci, v), _, _ = S.fixture(name)
    assert S.strength_margin(rp, ci, v, S.THETA) >= 2.0
    if name.startswith("thresholded"):
        A = sps.csr_matrix((v, ci, rp))
        strong = abs(A) > 0.5
        assert (strong != strong.T).nnz > 0          # a_ij strong with a_ji weak


@pytest.mark.parametrize("name", ALL)
def test_the_cycle_runs_on_every_fixture_that_is_decided_beyond_rounding(name):
    assert (name in S.CYCLE_FIXTURES) != (name in S.NOT_CYCLED)
    decided = S.fixture_reference(name).fully_decided
    if name in S.CYCLE_FIXTURES:
        assert decided
    else:
        assert not decided or name in S.NO_SMOOTHER


def test_the_thresholded_cycle_runs_at_its_threshold():
    assert S.fixture_reference("thresholded_20x13", S.THETA).fully_decided


@pytest.mark.parametrize("n", S.DENSE_SIZES)
@pytest.mark.parametrize("kind", S.DENSE_KINDS)
def test_dense_fixtures(n, kind):
    rp, ci, v, x, b = S.dense_direct(n, kind)
    A = sps.csr_matrix((v, ci, rp), shape=(n, n))
    assert S.dense_cond(n, kind) <= 1e4
    assert np.array_equal(A @ x, b)
    d = A.diagonal()
    if kind == "nodiag" and n > 1:
        assert not d.any()
    if kind != "nodiag" and n >= 63:
        assert np.count_nonzero(d == 0.0) > n // 2           # the stored diagonal is no pivot


def test_dense_singular_is_singular():
    rp, ci, v = S.dense_singular()
    assert np.linalg.matrix_rank(sps.csr_matrix((v, ci, rp)).toarray()) == len(rp) - 2


# ---------------------------------------------------------------- oracle against restatement
@pytest.mark.parametrize("name,theta", THETAS)
def test_oracle_builds_the_restated_hierarchy(name, theta):
    (rp, ci, v), nv, prm = S.fixture(name)
    H = S.fixture_reference(name, theta)
    G = orc.AMG(rp, ci, v, nullvec=nv, theta=theta, **prm)
    if H.fully_decided:
        assert G.levels == len(H.levels)
    for l in range(H.decided):
        L = H.levels[l]
        ro, co, vo = G.export(l, "A")
        assert np.array_equal(ro, L.rp) and np.array_equal(co, L.ci)
        assert _gap(vo, L.f64, L.bound()) <= 1.0
        if l + 1 < H.decided:
            assert np.array_equal(G.aggregates(l), L.agg)
            prp, pci, pv, pa, pk = L.P
            ro, co, vo = G.export(l, "P")
            assert np.array_equal(ro, prp) and np.array_equal(co, pci)
            assert _gap(vo, pv.astype(np.float64), 4.0 * pk * S.EPS * pa.astype(np.float64)) <= 1.0


@pytest.mark.parametrize("smoother", [0, 1])
@pytest.mark.parametrize("name", [n for n in S.CYCLE_FIXTURES if not n.startswith("long") and n not in S.NO_GAUSS_SEIDEL])
def test_oracle_cycle_is_the_restated_cycle(name, smoother):
    (rp, ci, v), nv, prm = S.fixture(name)
    r = np.random.default_rng(4).standard_normal(len(rp) - 1)
    zr = S.fixture_reference(name, 0.0, smoother).vcycle(r)
    zo = orc.AMG(rp, ci, v, nullvec=nv, smoother=smoother, **prm).apply(r)
    assert np.linalg.norm(zo - zr) <= 1e-9 * np.linalg.norm(zr)


# ---------------------------------------------------------------- mutations
# Aggregates and patterns are compared with np.array_equal, so for "an aggregate id off by one", "a pass-2 tie broken the
# other way" and "a dropped structural zero" what has to be shown is the PREMISE: the fixtures hold rows on which the wrong
# rule gives another array.  "A dropped singleton" has no fixture: pass 3 is never reached (see
# test_greedy_roots_equal_the_rounds_and_pass3_is_never_reached and the module docstring of amg_shapes).
def test_premise_pass2_ties_exist_and_the_other_choice_is_another_aggregate():
    for name in ("chain_257", "grid_16x16", "hub_16"):
        L = S.fixture_reference(name).levels[0]
        assert len(L.tie_rows) == L.stats["pass2_ties"] > 0
        assert all(alt != L.agg[i] and alt >= 0 for i, alt in L.tie_rows)
        (rp, ci, v), nv, prm = S.fixture(name)
        assert np.array_equal(orc.AMG(rp, ci, v, **prm).aggregates(0), L.agg)      # first in the row, not the other one


def test_premise_structural_zeros_of_p_exist_and_the_first_diagonal_differs_from_the_sum():
    L = S.fixture_reference("edge_zero_offdiag").levels[0]
    prp, pci, pv, pa, pk = L.P
    assert np.count_nonzero(pv == 0) >= 2           # entries of P behind the explicit zeros of A: dropped, the pattern differs
    L = S.fixture_reference("edge_dup_diag", 0.0, 2).levels[0]
    dup = np.flatnonzero(np.bincount(L.rows[L.ci == L.rows], minlength=L.n) == 2)
    assert len(dup) == 4 and np.all(L.diagonal()[dup] == L.csr().diagonal()[dup] + 1.0)


def test_mutation_summed_diagonal_instead_of_the_first():
    """edge_dup_diag: d_i taken as the sum of the two stored entries moves P beyond its bound"""
    (rp, ci, v), nv, prm = S.fixture("edge_dup_diag")
    L = S.fixture_reference("edge_dup_diag", 0.0, 2).levels[0]
    prp, pci, pv, pa, pk = L.P
    bound = 4.0 * pk * S.EPS * pa.astype(np.float64)
    A = sps.csr_matrix((v.copy(), ci.copy(), rp.copy()))
    A.sum_duplicates()                               # in place: on copies, the fixture is shared
    bad = S.reference(A.indptr, A.indices, A.data, prm).levels[0]
    assert np.array_equal(bad.agg, L.agg) and np.array_equal(bad.P[1], pci)
    assert _gap(bad.P[2], pv, bound) > 1e6


def test_mutation_unit_diagonal_replaced_by_zero():
    """d = 0 where 1.0 belongs (a row without a stored diagonal): the row of P loses its smoothing terms"""
    L = S.fixture_reference("edge_no_diag").levels[0]
    prp, pci, pv, pa, pk = L.P
    r, c, t = L.P_terms
    rows = np.flatnonzero(~L.has_diag)
    hit = np.isin(r, rows) & (np.arange(len(r)) >= np.count_nonzero(L.agg >= 0))     # the -(f a pt) terms of those rows
    assert np.count_nonzero(hit & (t != 0)) >= 4
    bound = 4.0 * pk * S.EPS * pa.astype(np.float64)
    key = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(np.repeat(np.arange(L.n), np.diff(prp)), pci))}
    bad = pv.astype(np.float64).copy()
    for k in np.flatnonzero(hit & (t != 0)):
        bad[key[(int(r[k]), int(c[k]))]] -= float(t[k])           # f = 0: the term is gone
    assert _gap(bad, pv, bound) > 1e6


@pytest.mark.parametrize("name", ["grid_21x13", "hub_65", "unsymmetric_150", "star_1100", "masked_grid_21x13"])
def test_mutation_one_term_missing_from_an_entry(name):
    """every non-zero term of every entry of P is larger than twice the entry's bound: a sum that loses one shows; the
    same for one product p_ki (A P)_kj of an entry of A_c, on the dense recomputation"""
    H = S.fixture_reference(name)
    L = H.levels[0]
    prp, pci, pv, pa, pk = L.P
    r, c, t = L.P_terms
    bound = 4.0 * pk * S.EPS * pa.astype(np.float64)
    pos = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(np.repeat(np.arange(L.n), np.diff(prp)), pci))}
    nz = np.flatnonzero(t != 0)
    for k in nz[:: max(1, len(nz) // 200)]:                        # one term at a time through the GPU test's comparison
        bad = pv.astype(np.float64).copy()
        bad[pos[(int(r[k]), int(c[k]))]] -= float(t[k])
        assert _gap(bad, pv, bound) > 2.0
    Lc = H.levels[1]
    P = sps.csr_matrix((pv.astype(np.float64), pci, prp), shape=(L.n, L.nagg))
    AP = (L.csr() @ P).tocsr()
    k = int(np.argmax(np.diff(P.indptr)))                          # drop row k's contribution to one entry
    i, j = P[k].indices[np.argmax(np.abs(P[k].data))], AP[k].indices[np.argmax(np.abs(AP[k].data))]
    e = np.flatnonzero((Lc.rows == i) & (Lc.ci == j))[0]
    bad = Lc.f64.copy()
    bad[e] -= P[k, i] * AP[k, j]
    assert _gap(bad, Lc.f64, Lc.bound()) > 2.0


def test_mutation_row_pivot_skipped():
    """Gauss-Jordan that takes the stored diagonal as pivot: the bidiag fixture has zeros there"""
    n = 63
    rp, ci, v, x, b = S.dense_direct(n, "bidiag")
    A = sps.csr_matrix((v, ci, rp), shape=(n, n)).toarray()
    with np.errstate(all="ignore"):
        M = np.hstack([A, b[:, None]])
        for k in range(n):
            M[k] = M[k] / M[k, k]
            for r in range(n):
                if r != k:
                    M[r] = M[r] - M[r, k] * M[k]
    bad = M[:, -1]
    tol = 8 * n * S.EPS * S.dense_cond(n, "bidiag")
    assert not (np.all(np.isfinite(bad)) and np.linalg.norm(bad - x) <= tol * np.linalg.norm(x))
    assert np.linalg.norm(np.linalg.solve(A, b) - x) <= tol * np.linalg.norm(x)


def test_mutation_last_row_of_the_ragged_block_ignored():
    H = S.fixture_reference("long_chain_118000")
    l = 1
    n = H.levels[l].n
    assert n % 64 not in (0, 1) and H.levels[l].path["smoother"] == 1
    r = np.random.default_rng(3).standard_normal(n)
    z = H.smooth_apply(l, r)
    r2 = r.copy()
    r2[n - 1] = 0.0
    z2 = H.smooth_apply(l, r2)
    z2[n - 1] = 0.0
    assert np.linalg.norm(z - z2) > 1e-9 * 100 * np.linalg.norm(z)


def test_smoother_zero_pivot_convention():
    """a zero pivot keeps its unknown at zero and passes nothing on"""
    H = S.fixture_reference("masked_grid_21x13")
    zero_rows = np.flatnonzero(np.asarray(H.nv[1]) == 0.0)
    r = np.ones(H.levels[1].n)
    for part in (0, 1, 2):
        z = H.smooth_apply(1, r, part)
        assert np.all(z[zero_rows] == 0.0) and np.all(np.isfinite(z)) and np.count_nonzero(z) == len(z) - len(zero_rows)
