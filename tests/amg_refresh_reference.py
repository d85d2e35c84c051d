"""The hierarchy of GIVEN values on GIVEN aggregates: what isph_prec_refactor of an "sa-amg" computes (csrc/amg.hpp
amg_refactor), restated on the host.

Host only: numpy.  Nothing is decided here -- no strength test, no independent set, no passes: the aggregates of every
level come from the caller (PrecondAMG.aggregates(l), or the reference's own), and so does the rule for the damping.
Level by level:
    d_i     the FIRST stored diagonal entry of row i, 1.0 when the row stores none
    rho     max_i sum_j |a_ij| / |d_i| over the rows with d_i != 0 (columns >= n do not count) -- or lambda[l] when the
            caller hands the estimates of eig_type = 1 over
    P_tent  pt_i = nv_i / |nv restricted to the aggregate of i| (0 for a row outside every aggregate, or a zero norm)
    P_l     (I - omega / rho D^-1 A_l) P_tent: the term pt_i in column agg_i, and -(omega / rho / d_i) a_ij pt_j in column
            agg_j for every stored a_ij with j < n and agg_j >= 0, whatever its value (a stored zero keeps its slot)
    nv_c    the norms above
    A_{l+1} P_l^T (A_l P_l), every structural product kept
Rows come out with ascending columns, values in float64; products are expanded term by term and summed per (row, column),
so an entry whose terms cancel stays in the pattern, as on the device.
"""
import numpy as np


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _group(nrows, ncols, r, c, t):
    """CSR (ascending columns) of the sums of t over equal (r, c)"""
    key = r.astype(np.int64) * max(ncols, 1) + c.astype(np.int64)
    uk, inv = np.unique(key, return_inverse=True)
    v = np.zeros(len(uk))
    np.add.at(v, inv, t)
    rr = uk // max(ncols, 1)
    rp = np.zeros(nrows + 1, dtype=np.int64)
    np.add.at(rp, rr + 1, 1)
    return np.cumsum(rp), (uk % max(ncols, 1)).astype(np.int64), v


def _product(nrows, ncols, xrp, xci, xv, yrp, yci, yv, yrows):
    """X * Y with every structural product kept; entries of X in columns >= yrows are skipped"""
    xr = _rows_of(xrp)
    e = np.flatnonzero(xci < yrows)
    ln = np.diff(yrp)[xci[e]]
    src = np.repeat(e, ln)
    off = np.arange(len(src)) - np.repeat(np.cumsum(ln) - ln, ln)
    q = yrp[xci[src]] + off
    return _group(nrows, ncols, xr[src], yci[q], xv[src] * yv[q])


def diagonal(rp, ci, v):
    n = len(rp) - 1
    rows = _rows_of(rp)
    dg = np.ones(n)
    isd = np.flatnonzero(ci == rows)[::-1]          # reversed: the first one is written last
    dg[rows[isd]] = v[isd]
    return dg


def rho_anorm(rp, ci, v):
    n = len(rp) - 1
    rows = _rows_of(rp)
    dg = diagonal(rp, ci, v)
    s = np.zeros(n)
    inside = ci < n
    np.add.at(s, rows[inside], np.abs(v[inside]))
    nz = dg != 0
    return float((s[nz] / np.abs(dg[nz])).max()) if nz.any() else 0.0


def hierarchy(rp, ci, val, aggs, nullvec=None, omega=4.0 / 3.0, lambdas=None):
    """levels: a list of dicts A = (rp, ci, v), nv, and below the coarsest level P = (rp, ci, v), rho, damp.
    aggs[l]: the aggregate of every row of level l (-1: none); len(aggs) + 1 levels.  lambdas[l] (eig_type 1) replaces
    rho of level l in the damping."""
    rp, ci, v = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(val, dtype=np.float64)
    n = len(rp) - 1
    nv = np.ones(n) if nullvec is None else np.asarray(nullvec, dtype=np.float64)
    levels = []
    for l, agg in enumerate(aggs):
        agg = np.asarray(agg, dtype=np.int64)
        assert len(agg) == n
        nagg = int(agg.max()) + 1
        inn = agg >= 0
        nvc2 = np.zeros(nagg)
        np.add.at(nvc2, agg[inn], nv[inn] * nv[inn])
        nvc = np.sqrt(nvc2)
        pt = np.zeros(n)
        ok = inn.copy()
        ok[inn] = nvc[agg[inn]] > 0
        pt[ok] = nv[ok] / nvc[agg[ok]]
        dg = diagonal(rp, ci, v)
        rho = rho_anorm(rp, ci, v)
        lam = float(lambdas[l]) if lambdas is not None else 0.0
        damp = omega / lam if lam > 0 else (omega / rho if rho > 0 else 0.0)
        f = np.where(dg != 0, damp / np.where(dg != 0, dg, 1.0), 0.0)
        rows = _rows_of(rp)
        e = np.flatnonzero((ci < n) & (agg[np.minimum(ci, n - 1)] >= 0))
        r = np.concatenate([np.flatnonzero(inn), rows[e]])
        c = np.concatenate([agg[inn], agg[ci[e]]])
        t = np.concatenate([pt[inn], -(f[rows[e]] * v[e] * pt[ci[e]])])
        P = _group(n, nagg, r, c, t)
        AP = _product(n, nagg, rp, ci, v, P[0], P[1], P[2], n)
        # R = P^T as a CSR, then R (A P)
        prow = _rows_of(P[0])
        o = np.lexsort((prow, P[1]))
        rrp = np.zeros(nagg + 1, dtype=np.int64)
        np.add.at(rrp, P[1] + 1, 1)
        Ac = _product(nagg, nagg, np.cumsum(rrp), prow[o], P[2][o], AP[0], AP[1], AP[2], n)
        levels.append(dict(A=(rp, ci, v), P=P, nv=nv, rho=rho, damp=damp, agg=agg))
        rp, ci, v = Ac
        n, nv = nagg, nvc
    levels.append(dict(A=(rp, ci, v), nv=nv))
    return levels
