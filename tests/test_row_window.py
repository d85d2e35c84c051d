"""tests/row_window.py against the full oracle assembly: the rows a window assembles must be the full system's rows bit for
bit (pattern, values, right-hand side, volumes), and a window one hop too shallow must not be."""
import numpy as np
import pytest

from isph_amd import workload
import oracle as orc
import row_window as rw
from problems import Problem, tgv_spec

THETA, BETA = 1.0, 0.1


def _sample(parts, nrows, seed):
    """random rows plus the rows the generators' edges and the lists' ends give: the first and last rows, rows whose list
    reaches a periodic image, and the owners of some row's first and last neighbour (rows that are each other's
    neighbours inside one window)"""
    n = int(parts["nlocal"])
    rng = np.random.default_rng(seed)
    nptr, nidx, own = parts["neigh_ptr"], parts["neigh_idx"], parts["owner_index"]
    rows = list(rng.choice(n, size=nrows, replace=False)) + [0, 1, n - 2, n - 1]
    img = np.flatnonzero(np.maximum.reduceat(nidx, nptr[:-1]) >= n)           # a list with a ghost (periodic image)
    assert img.size > 0
    rows += list(rng.choice(img, size=min(8, img.size), replace=False))
    r = int(rows[0])
    rows += [int(own[nidx[nptr[r]]]), int(own[nidx[nptr[r + 1] - 1]])]
    return np.unique(np.asarray(rows, dtype=np.int64))


def _first_fluid_row(parts, kinds):
    kind = np.asarray([0] + list(kinds if kinds is not None else [orc.FLUID] * int(parts["type"].max())))
    return int(np.flatnonzero(kind[parts["type"][:parts["nlocal"]]] == orc.FLUID)[0])


def _assert_rows_equal(full, win_out, rows, drop=()):
    """full = (rowptr, colidx, val, b) of the full system (val [nnz] or [k, nnz], b [n] or [k, n]); win_out the window's"""
    rp, ci, val, b = full
    wrp, wci, wval, wb = win_out
    keep = ~np.isin(rows, drop)
    sel = rows[keep]
    frp, fci, fval = rw.rows_of(rp, ci, val, sel)
    grp, gci, gval = rw.rows_of(wrp, wci, wval, np.flatnonzero(keep))
    assert np.array_equal(grp, frp) and np.array_equal(gci, fci)
    assert np.array_equal(gval, fval)
    assert np.array_equal(np.asarray(wb)[..., keep], np.asarray(b)[..., sel])


def _rows_differ(full, win_out, rows, drop=()):
    try:
        _assert_rows_equal(full, win_out, rows, drop)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("antisym", [True, False])
def test_window_tgv3d_jitter_poisson(antisym):
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER), antisym=antisym)
    p = pr.parts
    full = pr.poisson()
    skip = [_first_fluid_row(p, None)]
    for seed in (1, 2):
        rows = _sample(p, 40, seed)
        win, P, out = rw.poisson(p, pr.colmap, rows, pr.spec.dt, p["rho"], p["v"], antisym=antisym)
        assert win.nrows == len(rows) and win.parts["nlocal"] > win.nrows and win.parts["nall"] > win.parts["nlocal"]
        _assert_rows_equal(full, out, rows, skip)
        assert np.array_equal(P.vfrac[:win.nrows], pr.P.vfrac[rows])
        if not antisym:
            assert np.array_equal(P.Gc[:win.nrows], pr.P.Gc[rows]) and np.array_equal(P.Lc[:win.nrows], pr.P.Lc[rows])
    # one hop short: the neighbours' volumes are missing
    _, _, short = rw.poisson(p, pr.colmap, rows, pr.spec.dt, p["rho"], p["v"], antisym=antisym, depth=rw.DEPTH["poisson"] - 1)
    assert _rows_differ(full, short, rows, skip)


def test_window_with_64bit_list_offsets_and_a_single_row():
    pr = Problem(tgv_spec(dim=3, n=12, mode=workload.JITTER), antisym=False)
    p64 = dict(pr.parts)
    p64["neigh_ptr"] = pr.parts["neigh_ptr"].astype(np.int64)
    full = pr.poisson()
    n = pr.n
    for rows in ([n - 1], [0, n // 2, n - 1]):
        rows = np.asarray(rows)
        _, _, out = rw.poisson(p64, pr.colmap, rows, pr.spec.dt, p64["rho"], p64["v"], antisym=False)
        _assert_rows_equal(full, out, rows, [_first_fluid_row(pr.parts, None)])


@pytest.mark.parametrize("antisym", [True, False])
def test_window_cavity_block_helmholtz_and_wall_neumann_poisson(antisym):
    p = workload.make_cavity(8, wall=4, brick=(4, 4, 4), lid_inset=1, jitter=0.02)
    colmap = workload.single_rank_colmap(p)
    n, nall = p["nlocal"], p["nall"]
    typ = p["type"][:n]
    P = orc.Particles(p, colmap, kinds=p["kinds"])
    P.precompute(corrections=True)
    zeros3, g, pres = np.zeros((nall, 3)), np.zeros(3), np.zeros(nall)
    rng = np.random.default_rng(3)
    walls = np.flatnonzero((typ == 2) & (np.abs(p["normal"][:n]).sum(axis=1) > 0))
    rows = np.unique(np.r_[_sample(p, 40, 4), rng.choice(np.flatnonzero(typ == 1), 24, replace=False),
                           rng.choice(walls, 24, replace=False), rng.choice(np.flatnonzero(typ == 3), 8, replace=False)])
    assert all(np.any(typ[rows] == t) for t in (1, 2, 3))
    full_h = P.block_helmholtz(p["dt"], THETA, BETA, p["nu"], p["rho"], pres, zeros3, g, p["v"], normal=p["normal"],
                               antisym=antisym)
    win, Pw, out_h = rw.block_helmholtz(p, colmap, rows, p["dt"], THETA, BETA, p["nu"], p["rho"], pres, zeros3, g, p["v"],
                                        normal=p["normal"], antisym=antisym, kinds=p["kinds"])
    _assert_rows_equal(full_h, out_h, rows)
    assert np.array_equal(Pw.vfrac[:win.nrows], P.vfrac[rows]) and np.array_equal(Pw.Gc[:win.nrows], P.Gc[rows])
    # the pressure Poisson system with the wall Neumann rows
    vstar = np.ascontiguousarray((0.1 * rng.standard_normal((n, 3)) * (typ[:, None] == 1))[colmap])
    full_p = P.poisson(p["dt"], p["rho"], vstar, antisym=antisym, singular=orc.NULLSPACE, normal=p["normal"])
    skip = [_first_fluid_row(p, p["kinds"])]
    _, _, out_p = rw.poisson(p, colmap, rows, p["dt"], p["rho"], vstar, antisym=antisym, kinds=p["kinds"],
                             normal=p["normal"])
    _assert_rows_equal(full_p, out_p, rows, skip)
    _, _, short_h = rw.block_helmholtz(p, colmap, rows, p["dt"], THETA, BETA, p["nu"], p["rho"], pres, zeros3, g, p["v"],
                                       normal=p["normal"], antisym=antisym, kinds=p["kinds"], depth=0)
    _, _, short_p = rw.poisson(p, colmap, rows, p["dt"], p["rho"], vstar, antisym=antisym, kinds=p["kinds"],
                               normal=p["normal"], depth=0)
    assert _rows_differ(full_h, short_h, rows) and _rows_differ(full_p, short_p, rows, skip)


def test_window_porous_quintic_morris_holmes_not_singular():
    p = workload.make_porous_cylinder(28, brick=(4, 4, 4), jitter=0.02)
    colmap = workload.single_rank_colmap(p)
    n, nall = p["nlocal"], p["nall"]
    P0 = orc.Particles(p, colmap, kernel="quintic", kinds=p["kinds"])
    P0.precompute(corrections=False)
    pnd = np.ascontiguousarray(1.0 / P0.vfrac)
    P = orc.Particles(p, colmap, kernel="quintic", kinds=p["kinds"], pnd=pnd, morris_safe_coeff=0.43301)
    P.precompute(corrections=False)
    vstar = np.zeros((nall, 3))
    xw = p["x"]
    vstar[:, 1] = 1e-3 * np.cos(xw[:, 0]) * (p["type"] <= 2)
    vstar[:, 0] = 1e-3 * np.sin(xw[:, 1]) * (p["type"] <= 2)
    full = P.poisson(p["dt"], p["rho"], vstar, singular=orc.NOT_SINGULAR, morris=1)
    rows = _sample(p, 24, 6)
    typ = p["type"][:n]
    rng = np.random.default_rng(7)
    rows = np.unique(np.r_[rows, [rng.choice(np.flatnonzero(typ == t)) for t in (1, 2, 3, 4)]])
    kw = dict(kernel="quintic", kinds=p["kinds"], singular=orc.NOT_SINGULAR, morris=1, pnd_from_volumes=True)
    win, Pw, out = rw.poisson(p, colmap, rows, p["dt"], p["rho"], vstar, **kw)
    _assert_rows_equal(full, out, rows)                           # NOT_SINGULAR: no row is edited
    assert np.array_equal(Pw.vfrac[:win.nrows], P.vfrac[rows])
    _, _, short = rw.poisson(p, colmap, rows, p["dt"], p["rho"], vstar, depth=0, **kw)
    assert _rows_differ(full, short, rows)
