"""The numpy restatement of a value update (tests/pattern_hold_reference.py) on constructed rows, against
scipy.sparse's sort_indices.  Host only; tests/test_gpu_pattern_hold.py compares the library with the restatement."""
import numpy as np
import pytest
import scipy.sparse as sp

import pattern_hold_reference as ph


def csr_of(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rp[-1] else np.zeros(0, np.int32)
    return rp, ci


ROWS = {
    "descending": ([[7, 5, 3, 1, 0], [9, 8], [6, 4, 2]], 10),
    "single_entry_row": ([[3], [0, 2], [1]], 4),
    "empty_row": ([[2, 0], [], [1, 2], []], 3),
    "ghost_columns": ([[5, 0, 4], [1, 3], [2, 6, 1]], 7),        # 3 rows, columns 3 .. 6 are ghosts
    "already_sorted": ([[0, 1], [1, 2], [0, 2]], 3),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_updated_csr_is_scipys_sorted_matrix_with_the_new_values(name):
    rows, ncol = ROWS[name]
    rp, ci = csr_of(rows)
    old = np.arange(1, len(ci) + 1, dtype=np.float64)
    new = ph.new_values(rp, old, seed=3)
    urp, uci, uv = ph.updated_csr(rp, ci, new)
    m = sp.csr_matrix((new.copy(), ci.copy(), rp.copy()), shape=(len(rows), ncol))
    m.sort_indices()
    assert np.array_equal(urp, m.indptr) and np.array_equal(uci, m.indices)
    assert np.array_equal(uv.view(np.uint64), m.data.view(np.uint64))       # zeros keep their place: nothing is eliminated
    row, rank = ph.entry_map(rp, ci)
    assert np.array_equal(row, ph.row_of_entry(rp))
    for e in range(len(ci)):                                                 # the map by its definition, entry by entry
        seg = ci[rp[row[e]]:rp[row[e] + 1]]
        assert rank[e] == np.sum(seg < ci[e])
        assert uci[urp[row[e]] + rank[e]] == ci[e] and uv[urp[row[e]] + rank[e]] == new[e]


def test_descending_row_reverses():
    rp, ci = csr_of([[4, 3, 2, 1, 0]])
    _, rank = ph.entry_map(rp, ci)
    assert list(rank) == [4, 3, 2, 1, 0]
    assert list(ph.updated_csr(rp, ci, [10., 11., 12., 13., 14.])[2]) == [14., 13., 12., 11., 10.]


def test_repeated_column_is_unmappable():
    rp, ci = csr_of([[0, 1], [2, 0, 2], [1]])
    assert not ph.mappable(rp, ci)
    with pytest.raises(ph.Unmappable, match="row 1 holds column 2 twice"):
        ph.entry_map(rp, ci)
    with pytest.raises(ph.Unmappable):
        ph.updated_csr(rp, ci, np.ones(len(ci)))
    rp2, ci2 = csr_of([[0, 1], [2, 0], [2]])                                 # the same column in two ROWS is fine
    assert ph.mappable(rp2, ci2)


def test_new_values_cannot_be_met_by_a_stale_image():
    rp, ci = csr_of(ROWS["empty_row"][0])
    old = np.array([5.0, 4242.0, 7.0, 9.0])
    new = ph.new_values(rp, old, seed=1)
    for r in range(len(rp) - 1):
        if rp[r + 1] > rp[r]:
            assert new[rp[r]] != old[rp[r]]
    big = ph.new_values(np.array([0, 2000]), np.arange(1.0, 2001.0), seed=2)
    assert (big == 0.0).any() and (big == -np.arange(1.0, 2001.0)).any()
