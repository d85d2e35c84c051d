"""Row-window oracle: the unchanged CPU oracle assembles a few rows of a system far too large for it, bit for bit.

A window holds the requested rows plus the OWNERS of every particle within `depth` neighbour hops of them, each with
its full neighbour list (original order) renumbered into the window.  The further particles those lists reach become
ghosts: a ghost keeps the window index of its owner when the owner is in the window and gets -1 otherwise.  Columns
are the caller's own global ids (colmap carried over), so every sum the oracle forms runs over the same operands in
the same order as on the full system, and the window's rows equal the full assembly's rows exactly.

The rows come first in the window.  The oracle forms the volumes of all window particles; G_i, L_i and the assembly
are then restricted to the rows (`WindowParticles.precompute`): the other window particles act as ghosts that already
hold their volumes, and no row but the requested ones is assembled.

Depth a row needs (read off oracle/isph_oracle.c):
  volumes V_i, pnd_i (orc_compute_volumes, orc_compute_pnd)    0: positions of the row's own neighbours only
  G_i, L_i (orc_compute_gradient/laplacian_correction)        1: V_j of every neighbour
  Poisson rows + RHS, both families (orc_poisson)             1: V_j; the Symmetric family G_i, L_i (the row's own);
                                                                 MorrisHolmes pnd_j V_j; wall Neumann rows G_i, V_j
                                                                 and the row's normal (an input array)
  block Helmholtz rows + RHS (orc_block_helmholtz)            1: V_j, G_i of the slip term, normals (input arrays)
No operator reads G_j, L_j or any neighbour's neighbour directly, so depth 1 suffices everywhere; depth 0 leaves V_j
of most neighbours at 0 (their owners are not in the window) and the rows differ.

The helper never copies the whole neighbour list: only the lists of the window particles are gathered, with 64-bit
offsets when the caller's list has them."""
import types

import numpy as np

import oracle as orc

DEPTH = {"volumes": 0, "pnd": 0, "corrections": 1, "poisson": 1, "block_helmholtz": 1}


def _owner(parts):
    own = np.asarray(parts["owner_index"])
    if "owner_rank" in parts:
        assert np.all(np.asarray(parts["owner_rank"]) == parts["spec"].rank), "row_window: single rank only"
    return own


def _lists(nptr, nidx, who):
    """concatenated neighbour lists of the particles `who` (in that order), and their lengths"""
    lo = np.asarray(nptr[who], dtype=np.int64)
    ln = np.asarray(nptr[who + 1], dtype=np.int64) - lo
    tot = int(ln.sum())
    start = np.zeros(len(who), dtype=np.int64)
    np.cumsum(ln[:-1], out=start[1:])
    src = np.repeat(lo - start, ln) + np.arange(tot, dtype=np.int64)
    return np.asarray(nidx[src]), ln


class Window:
    """Window of `rows` (local indices into `parts`, unique, any order kept sorted) at `depth` neighbour hops.

    parts    the window as a make_tgv-style dict (x, type, neigh_ptr int32, neigh_idx, owner_index, ...)
    colmap   the caller's column ids of the window particles
    src      original particle index of every window particle; take(a) gathers a per-particle array [nall, ...]
    rows     the requested rows (sorted); they are the window's particles 0 .. nrows-1"""

    def __init__(self, parts, colmap, rows, depth):
        rows = np.unique(np.asarray(rows, dtype=np.int64))
        n, nall_full = int(parts["nlocal"]), int(parts["nall"])
        assert rows.size and rows[0] >= 0 and rows[-1] < n
        own = _owner(parts)
        nptr, nidx = parts["neigh_ptr"], parts["neigh_idx"]
        # hop k: the owners of the particles the lists of hop k-1 reach (a ghost is continued through its owner)
        have = np.zeros(n, dtype=bool)
        have[rows] = True
        front = rows
        for _ in range(int(depth)):
            reach, _ = _lists(nptr, nidx, front)
            new = np.zeros(n, dtype=bool)
            new[own[reach]] = True
            new &= ~have
            have |= new
            front = np.flatnonzero(new)
        have[rows] = False
        loc = np.concatenate([rows, np.flatnonzero(have)])      # the rows first, then the other owners
        nidx_w, ln = _lists(nptr, nidx, loc)
        # window numbering: locals 0..nloc-1, then every further particle the lists reach (ghosts), in ascending order
        g = np.zeros(nall_full, dtype=bool)
        g[nidx_w] = True
        g[loc] = False
        src = np.concatenate([loc, np.flatnonzero(g)])
        nloc, nall = len(loc), len(src)
        to_window = np.full(nall_full, -1, dtype=np.int64)
        to_window[src] = np.arange(nall)
        wptr = np.zeros(nloc + 1, dtype=np.int64)
        np.cumsum(ln, out=wptr[1:])
        assert wptr[-1] < 2 ** 31 - 1, "row_window: window too large for the oracle's 32-bit list"
        wown = to_window[own[src]]
        wown[wown >= nloc] = -1                                   # an owner that is only a ghost here holds no values
        x = np.ascontiguousarray(np.asarray(parts["x"])[src])
        typ = np.ascontiguousarray(np.asarray(parts["type"])[src], dtype=np.int32)
        self.src, self.rows, self.nrows, self.depth = src, rows, len(rows), int(depth)
        self.colmap = np.ascontiguousarray(np.asarray(colmap)[src], dtype=np.int32)
        self.parts = dict(spec=types.SimpleNamespace(rank=0), dim=int(parts["dim"]), nlocal=nloc, nall=nall, x=x,
                          type=typ, owner_rank=np.zeros(nall, dtype=np.int32), owner_index=wown.astype(np.int32),
                          neigh_ptr=wptr.astype(np.int32), neigh_idx=to_window[nidx_w].astype(np.int32),
                          h=float(parts["h"]), cut=float(parts["cut"]))

    def take(self, a):
        """a per-particle array of the full system [nall, ...] restricted to the window"""
        return np.ascontiguousarray(np.asarray(a)[self.src])


class WindowParticles(orc.Particles):
    """orc.Particles over a window.  precompute() forms the volumes of all window particles, then restricts the view to
    the requested rows (the window's first nrows particles): G_i, L_i and every assembly run over those rows alone, the
    other window particles serve as ghosts that hold their volumes already."""

    def __init__(self, win, **kw):
        self.win = win
        super().__init__(win.parts, win.colmap, **kw)

    def restrict(self):
        self.nlocal = self.win.nrows
        self.c.nlocal = self.win.nrows
        return self

    def precompute(self, corrections=True):
        assert self.nlocal == self.win.parts["nlocal"], "precompute before restrict"
        orc.lib().orc_compute_volumes(self.ref())
        self.restrict()
        if corrections:
            orc.lib().orc_compute_gradient_correction(self.ref())
            orc.lib().orc_compute_laplacian_correction(self.ref())
        return self


def rows_of(rp, ci, val, rows):
    """the CSR rows `rows` of a matrix: (rowptr, colidx, val) of the stacked rows (val may be [k, nnz])"""
    rows = np.asarray(rows, dtype=np.int64)
    rp = np.asarray(rp, dtype=np.int64)
    ln = rp[rows + 1] - rp[rows]
    out = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(ln, out=out[1:])
    src = np.repeat(rp[rows] - out[:-1], ln) + np.arange(int(out[-1]), dtype=np.int64)
    return out, np.asarray(ci)[src], np.asarray(val)[..., src]


def poisson(parts, colmap, rows, dt, rho, vstar, depth=DEPTH["poisson"], antisym=True, singular=orc.NULLSPACE,
            kernel="wendland", kinds=None, normal=None, morris=0, pnd_from_volumes=False, morris_safe_coeff=0.43301,
            solid_normal_diag=1.0):
    """Poisson rows `rows` of the system orc.Particles(parts, colmap).poisson(...) builds (rank0=False: the singular-mode
    edit of the first fluid row is not made).  pnd_from_volumes: the mirror's particle number density is 1 / V, from the
    oracle's own volumes.  Returns (window, particles, (rowptr, colidx, val, b)) with the rows in sorted order."""
    win = Window(parts, colmap, rows, depth)
    corr = (not antisym) or normal is not None
    P = WindowParticles(win, kernel=kernel, kinds=kinds, pnd=np.zeros(win.parts["nall"]) if pnd_from_volumes else None,
                        morris_safe_coeff=morris_safe_coeff)
    P.precompute(corrections=corr)
    if pnd_from_volumes:                                          # in place: the oracle's view points at this buffer
        with np.errstate(divide="ignore"):
            P.pnd[:] = 1.0 / P.vfrac                              # ghosts without an owner in the window: inf, never read
    out = P.poisson(dt, win.take(rho), win.take(vstar), antisym=antisym, singular=singular, rank0=False,
                    normal=None if normal is None else win.take(normal), morris=morris,
                    solid_normal_diag=solid_normal_diag)
    return win, P, out


def block_helmholtz(parts, colmap, rows, dt, theta, beta, nu, rho, p, f, g, vall, normal=None, antisym=True,
                    depth=DEPTH["block_helmholtz"], kernel="wendland", kinds=None, incremental=True):
    """block Helmholtz rows `rows` (orc.Particles.block_helmholtz on the full system): (window, particles,
    (rowptr, colidx, vals[dim*dim, nnz], b[dim, nrows]))"""
    win = Window(parts, colmap, rows, depth)
    P = WindowParticles(win, kernel=kernel, kinds=kinds)
    P.precompute(corrections=True)
    t = win.take
    out = P.block_helmholtz(dt, theta, beta, t(nu), t(rho), t(p), t(f), g, t(vall),
                            normal=None if normal is None else t(normal), antisym=antisym, incremental=incremental)
    return win, P, out


def runs(n, nruns, length=64, seed=0, starts=()):
    """rows of `nruns` runs of `length` consecutive rows spread over [0, n) (seeded), plus runs starting at `starts`"""
    rng = np.random.default_rng(seed)
    s = np.r_[rng.integers(0, n - length + 1, size=nruns), np.minimum(np.asarray(starts, dtype=np.int64), n - length)]
    return np.unique((s[:, None] + np.arange(length)).ravel())


def device_rows(A, rows):
    """the rows `rows` (sorted, unique) of a device matrix in the caller's numbering, through isph_mat_export_rows (one
    call per run of consecutive rows): (rowptr int64, colidx, val)"""
    rows = np.asarray(rows, dtype=np.int64)
    cut = np.flatnonzero(np.diff(rows) != 1) + 1
    parts = []
    for r in np.split(rows, cut):
        parts.append(A.export_rows(int(r[0]), len(r)))
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(np.concatenate([np.diff(p[0]) for p in parts]), out=rp[1:])
    return rp, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def assert_rows_match(dev, win, tol, scale=None):
    """device rows (rowptr, colidx, val) against the window's: pattern exact, |dval| <= tol * scale (default max|val| of
    the window's rows).  Returns max|dval| / scale."""
    rp, ci, v = dev
    wrp, wci, wv = win
    assert np.array_equal(np.asarray(rp, dtype=np.int64), np.asarray(wrp, dtype=np.int64)), "row lengths differ"
    assert np.array_equal(ci, wci), "columns differ"
    scale = float(np.abs(wv).max()) if scale is None else float(scale)
    err = float(np.abs(v - wv).max()) / scale
    assert err <= tol, (err, tol)
    return err
