"""What a matrix whose pattern is kept must export after a value update, restated in numpy (no GPU, no library call).

isph_mat_update_values moves values without arithmetic: the updated matrix is the CSR the caller created it from, with
the new values, every row's columns ascending and the values carried along (Epetra's OptimizeStorage order, which is what
isph_mat_export_csr returns).  The entry map the library keeps for that is restated here as "source entry -> (row, rank
of its column in the row)"; a row that holds a column twice has no such map (a search cannot tell the two apart) and
is reported as unmappable.
"""
import numpy as np


class Unmappable(ValueError):
    """a row holds the same column twice"""


def row_of_entry(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def entry_map(rowptr, colidx):
    """(row [nnz], rank [nnz]): source entry e lies in row row[e] and its column is the rank[e]-th smallest of that row.
    Raises Unmappable (naming the first such row) when a row holds a column twice."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    row = row_of_entry(rowptr)
    order = np.lexsort((colidx, row))                       # entries by (row, column); rows stay in place
    srow, scol = row[order], colidx[order]
    dup = (srow[1:] == srow[:-1]) & (scol[1:] == scol[:-1])
    if dup.any():
        raise Unmappable("row %d holds column %d twice" % (srow[1:][dup][0], scol[1:][dup][0]))
    rank = np.empty(len(colidx), dtype=np.int64)
    rank[order] = np.arange(len(colidx), dtype=np.int64) - rowptr[srow]
    return row, rank


def mappable(rowptr, colidx):
    try:
        entry_map(rowptr, colidx)
        return True
    except Unmappable:
        return False


def updated_csr(rowptr, colidx, newval):
    """(rowptr, colidx, val) an updated matrix exports: the columns of every row ascending, newval carried along"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    row, rank = entry_map(rowptr, colidx)
    dst = rowptr[row] + rank
    ci = np.empty(len(dst), dtype=np.int32)
    v = np.empty(len(dst), dtype=np.float64)
    ci[dst] = np.asarray(colidx, dtype=np.int32)
    v[dst] = np.asarray(newval, dtype=np.float64)
    return rowptr.astype(np.int32), ci, v


def new_values(rowptr, val, seed=0):
    """values no stale image can pass for: every row with entries gets at least one value that differs from the old one
    (its first entry), about a fifth of the rest are exact zeros, a fifth change sign, the others are fresh integers"""
    rng = np.random.default_rng(seed)
    val = np.asarray(val, dtype=np.float64)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    kind = rng.integers(0, 5, size=len(val))
    fresh = rng.integers(1, 1000, size=len(val)).astype(np.float64) * rng.choice([-1.0, 1.0], size=len(val))
    out = np.where(kind == 0, 0.0, np.where(kind == 1, -val, fresh))
    first = rowptr[:-1][np.diff(rowptr) > 0]
    out[first] = np.where(val[first] == 4242.0, 4243.0, 4242.0)
    return out
