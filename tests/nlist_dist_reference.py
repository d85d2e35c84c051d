"""numpy restatement of include/isph_hip.h "the same step on a brick of ranks": the decomposition, the wrap, the border rule,
the ghost order, the list, prune, column map, halo plan and the migration order -- the same formulas, all ranks at once in
one process.  tests/test_nlist_dist_host.py pins it to workload.make_cloud + dist.make_plan; tests/test_gpu_nlist_dist.py
compares the device build with it bit for bit."""
import itertools

import numpy as np


def nl_wrap(x, lo, period):
    """fmod + the two fix-ups (csrc/neighbours.hpp nl_wrap)"""
    r = np.fmod(np.asarray(x, dtype=np.float64) - lo, period)
    r = np.where(r < 0.0, r + period, r)
    r = np.where(r >= period, 0.0, r)
    return r + lo


class Decomp:
    def __init__(self, dim, lo, hi, periodic, pgrid, faces=None):
        self.dim = int(dim)
        pad = lambda v, fill: (list(v) + [fill] * 3)[:3]
        self.lo = np.array(pad(lo, 0.0), dtype=np.float64)
        self.hi = np.array(pad(hi, 0.0), dtype=np.float64)
        self.lo[self.dim:] = 0.0
        self.hi[self.dim:] = 0.0
        self.periodic = [int(bool(v)) for v in pad(periodic, 0)]
        self.pgrid = [int(v) for v in pad(pgrid, 1)]
        for a in range(self.dim, 3):
            self.periodic[a], self.pgrid[a] = 0, 1
        self.period = self.hi - self.lo
        self.user_faces = faces
        self.faces = []
        for a in range(3):
            pg = self.pgrid[a]
            if a < self.dim and faces is not None and faces[a] is not None:
                f = np.array(faces[a], dtype=np.float64)
                assert len(f) == pg + 1 and f[0] == self.lo[a] and f[-1] == self.hi[a]
            else:
                w = (self.hi[a] - self.lo[a]) / pg
                f = np.array([self.lo[a] + c * w for c in range(pg)] + [self.hi[a]], dtype=np.float64)
            self.faces.append(f)

    @property
    def nranks(self):
        return self.pgrid[0] * self.pgrid[1] * self.pgrid[2]

    def coords(self, rank):
        c, r = [], int(rank)
        for a in range(3):
            c.append(r % self.pgrid[a])
            r //= self.pgrid[a]
        return c

    def rank_of(self, c):
        return c[0] + self.pgrid[0] * (c[1] + self.pgrid[1] * c[2])

    def wrap(self, x):
        xw = np.array(x, dtype=np.float64, copy=True).reshape(-1, 3)
        for a in range(self.dim):
            if self.periodic[a]:
                xw[:, a] = nl_wrap(xw[:, a], self.lo[a], self.period[a])
        return xw

    def cell(self, a, x):
        """grid cell of axis a: faces[c] <= x < faces[c + 1]; beyond an outer face the outer cell"""
        return np.clip(np.searchsorted(self.faces[a], x, side="right") - 1, 0, self.pgrid[a] - 1)

    def owner(self, xw):
        c = [self.cell(a, xw[:, a]) if a < self.dim else np.zeros(len(xw), dtype=np.int64) for a in range(3)]
        return (c[0] + self.pgrid[0] * (c[1] + self.pgrid[1] * c[2])).astype(np.int64)

    def check(self, cut):
        for a in range(self.dim):
            w = np.diff(self.faces[a])
            if self.pgrid[a] > 1 and np.any(w < cut):
                raise ValueError("a sub-box is narrower than the cut")
            if self.pgrid[a] == 1 and self.periodic[a] and self.hi[a] - self.lo[a] < 2.0 * cut:
                raise ValueError("a periodic axis is shorter than two cuts")

    def slots(self, rank):
        """[(d, s, receiver rank)] of the rank's grid offsets in ascending (sz, sy, sx)"""
        c = self.coords(rank)
        opt = []
        for a in range(3):
            o = []
            for d in ((-1, 0, 1) if a < self.dim else (0,)):
                tc, s = c[a] + d, 0
                if tc < 0:
                    if not self.periodic[a]:
                        continue
                    tc, s = self.pgrid[a] - 1, 1
                if tc >= self.pgrid[a]:
                    if not self.periodic[a]:
                        continue
                    tc, s = 0, -1
                o.append((d, s, tc))
            opt.append(sorted(o, key=lambda t: t[1]))
        out = []
        for oz, oy, ox in itertools.product(opt[2], opt[1], opt[0]):
            if ox[0] == 0 and oy[0] == 0 and oz[0] == 0:
                continue
            out.append(((ox[0], oy[0], oz[0]), (ox[1], oy[1], oz[1]), self.rank_of([ox[2], oy[2], oz[2]])))
        return out


def split(dc, x_global):
    """ownership by the faces: per rank the global ids (ascending) of the particles it owns"""
    own = dc.owner(dc.wrap(x_global))
    return [np.flatnonzero(own == r) for r in range(dc.nranks)]


def _records(dc, rank, xw, cut):
    """the records rank `rank` sends: {receiver: (positions [m, 3], owner index [m], shift [m, 3])}, per receiver in
    ascending (owner index, shift)"""
    c = dc.coords(rank)
    n = len(xw)
    low, high = np.zeros((n, 3), dtype=bool), np.zeros((n, 3), dtype=bool)
    bad = np.zeros(n, dtype=bool)
    for a in range(dc.dim):
        flo, fhi = dc.faces[a][c[a]], dc.faces[a][c[a] + 1]
        open_lo = not dc.periodic[a] and c[a] == 0
        open_hi = not dc.periodic[a] and c[a] == dc.pgrid[a] - 1
        if not open_lo:
            bad |= xw[:, a] < flo
        if not open_hi:
            bad |= ~(xw[:, a] < fhi)
        low[:, a] = xw[:, a] - flo < cut
        high[:, a] = xw[:, a] >= fhi - cut
    if bad.any():
        raise ValueError("%d owned particles lie outside the rank's sub-box" % int(bad.sum()))
    per = {}
    for k, (d, s, rcv) in enumerate(dc.slots(rank)):
        ok = np.ones(n, dtype=bool)
        for a in range(3):
            if d[a] < 0:
                ok &= low[:, a]
            elif d[a] > 0:
                ok &= high[:, a]
        i = np.flatnonzero(ok)
        pos = xw[i].copy()
        for a in range(3):
            pos[:, a] = xw[i, a] + float(s[a]) * dc.period[a]
        if dc.dim == 2:
            pos[:, 2] = 0.0
        per.setdefault(rcv, []).append((pos, i, np.tile(np.array(s, dtype=np.int64), (len(i), 1)), np.full(len(i), k)))
    out = {}
    for rcv, parts in per.items():
        pos, idx, sh, slot = (np.concatenate([p[j] for p in parts]) for j in range(4))
        o = np.lexsort((slot, idx))           # by particle, then by slot = ascending shift for one receiver
        out[rcv] = (pos[o], idx[o], sh[o])
    return out


def _rows(x_all, n, cut):
    """j != i with ((d0 d0) + d1 d1) + d2 d2 < cut cut, ascending j"""
    cutsq = cut * cut
    ptr, idx = np.zeros(n + 1, dtype=np.int64), []
    for i in range(n):
        d = x_all[i] - x_all
        r = d[:, 0] * d[:, 0]
        r = r + d[:, 1] * d[:, 1]
        r = r + d[:, 2] * d[:, 2]
        hit = r < cutsq
        hit[i] = False
        j = np.flatnonzero(hit)
        idx.append(j)
        ptr[i + 1] = ptr[i] + len(j)
    return ptr, (np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)).astype(np.int32)


def build(dc, x_owned, cut, prune):
    """x_owned: per rank [nlocal, 3].  Returns per rank a dict: nlocal, nall, x, owner_rank, owner_index, shift [nall, 3],
    neigh_ptr (int64), neigh_idx, colmap, ncol, peers, send_ptr, send_idx, recv_ptr (int32 like the library's)."""
    dc.check(cut)
    R = dc.nranks
    assert len(x_owned) == R
    xw = [dc.wrap(x) for x in x_owned]
    rec = [_records(dc, r, xw[r], cut) for r in range(R)]
    out = []
    for me in range(R):
        n = len(xw[me])
        gx, gr, gi, gs = [np.zeros((0, 3))], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 3), np.int64)]
        for src in range(R):                                   # ghosts by owner rank, this rank's images in its place
            if me in rec[src]:
                pos, idx, sh = rec[src][me]
                gx.append(pos); gi.append(idx); gs.append(sh); gr.append(np.full(len(idx), src, dtype=np.int64))
        x_all = np.concatenate([xw[me]] + gx)
        orank = np.concatenate([np.full(n, me, dtype=np.int64)] + gr)
        oidx = np.concatenate([np.arange(n, dtype=np.int64)] + gi)
        shift = np.concatenate([np.zeros((n, 3), dtype=np.int64)] + gs)
        ptr, idx = _rows(x_all, n, cut)
        nall = len(x_all)
        if prune:
            keep = np.zeros(nall, dtype=bool)
            keep[:n] = True
            keep[idx] = True
            newidx = np.cumsum(keep) - 1
            x_all, orank, oidx, shift = x_all[keep], orank[keep], oidx[keep], shift[keep]
            idx = newidx[idx].astype(np.int32)
            nall = len(x_all)
        out.append(dict(nlocal=n, nall=nall, x=x_all, owner_rank=orank.astype(np.int32), owner_index=oidx.astype(np.int32),
                        shift=shift, neigh_ptr=ptr, neigh_idx=idx))
    # column map and plan: the receiver's distinct (owner rank, owner index) pairs; the sender lists the same pairs
    want = []
    for me in range(R):
        o, n = out[me], out[me]["nlocal"]
        colmap = np.arange(o["nall"], dtype=np.int64)
        g = np.arange(n, o["nall"])
        img = o["owner_rank"][g] == me
        colmap[g[img]] = o["owner_index"][g[img]]
        rem = g[~img]
        key = o["owner_rank"][rem].astype(np.int64) * (1 << 32) + o["owner_index"][rem]
        ukey, inv = np.unique(key, return_inverse=True)
        colmap[rem] = n + inv
        o["colmap"], o["ncol"] = colmap.astype(np.int32), n + len(ukey)
        want.append({int(r): (ukey[(ukey >> 32) == r] & 0xFFFFFFFF).astype(np.int32) for r in np.unique(ukey >> 32)})
    for me in range(R):
        sends = {p: want[p][me] for p in range(R) if p != me and me in want[p]}
        peers = sorted(set(want[me]) | set(sends))
        sp, rp, si = [0], [0], []
        for p in peers:
            s = sends.get(p, np.zeros(0, np.int32))
            si.append(s)
            sp.append(sp[-1] + len(s))
            rp.append(rp[-1] + len(want[me].get(p, ())))
        out[me].update(peers=np.asarray(peers, np.int32), send_ptr=np.asarray(sp, np.int32), recv_ptr=np.asarray(rp, np.int32),
                       send_idx=np.concatenate(si).astype(np.int32) if si else np.zeros(0, np.int32))
    return out


FAR = "moved farther than one sub-box"


def migrate(dc, x_owned, fd, fi):
    """per rank x [n, 3], fd [n, nd], fi [n, ni] -> per rank (x, fd, fi, sent, received): positions wrapped, the stayers in
    their old order, then the arrivals by (source rank, source index).  ValueError(FAR) when a target is no grid neighbour."""
    R = dc.nranks
    xw = [dc.wrap(x) for x in x_owned]
    dest = []
    for r in range(R):
        c = dc.coords(r)
        t = dc.owner(xw[r])
        for a in range(dc.dim):
            ta = dc.cell(a, xw[r][:, a])
            d = ta - c[a]
            pg = dc.pgrid[a]
            if dc.periodic[a] and pg > 1:
                d = np.where((ta == (c[a] + 1) % pg) | (ta == (c[a] - 1) % pg), 0, d)
            if np.any(np.abs(d) > 1):
                raise ValueError(FAR)
        dest.append(t)
    out = []
    for me in range(R):
        px, pd, pi = [], [], []
        stay = dest[me] == me
        px.append(xw[me][stay]); pd.append(fd[me][stay]); pi.append(fi[me][stay])
        nrecv = 0
        for src in range(R):
            if src == me:
                continue
            go = dest[src] == me
            nrecv += int(go.sum())
            px.append(xw[src][go]); pd.append(fd[src][go]); pi.append(fi[src][go])
        out.append((np.concatenate(px), np.concatenate(pd), np.concatenate(pi), int((~stay).sum()), nrecv))
    return out


# ---- the cases of tests/test_nlist_dist_host.py and tests/test_gpu_nlist_dist.py -------------------------------------------
# 2-D and 3-D: Wendland, h = 1.5 dx, cut = 3 dx, the box [0, 2 pi)^dim with the lattice at multiples of dx -- particles ON
# the faces of an even pgrid and pairs ON the cut radius.

# dim, lattice, pgrid, periodic, non-uniform faces
CASES = [
    (2, 16, (1, 1), (1, 1), False),
    (2, 16, (2, 1), (1, 1), False),
    (2, 16, (3, 1), (1, 1), False),
    (2, 16, (2, 2), (1, 1), False),
    (2, 16, (4, 1), (1, 1), False),
    (2, 16, (2, 1), (1, 0), False),
    (2, 16, (2, 1), (1, 1), True),
    (3, 12, (2, 2, 2), (1, 1, 1), False),
    (3, 12, (3, 2, 1), (1, 1, 1), False),
]
CLOUDS = ["jitter0.05-s1", "jitter0.05-s2", "jitter0.3-s1", "jitter0.3-s2", "lattice", "at-hi", "void"]


def case_id(c):
    return "%dd-%s%s%s" % (c[0], "x".join(str(v) for v in c[2]), "" if all(c[3]) else "-p" + "".join(str(v) for v in c[3]),
                           "-faces" if c[4] else "")


def geometry(case):
    dim, nlat, pgrid, periodic, nonuni = case
    dx = 2.0 * np.pi / nlat
    L = nlat * dx
    faces = None
    if nonuni:                                   # 7 + 9 cells: both sub-boxes at least the cut (3 dx) wide
        faces = [np.array([0.0, 7.0 * dx + 0.25 * dx, L]), None, None]
    dc = Decomp(dim, [0.0] * dim, [L] * dim, periodic, pgrid, faces)
    return dc, dx, L, 1.5 * dx, 3.0 * dx


def cloud(case, kind):
    """the global positions [N, 3] BEFORE the wrap"""
    dim, nlat, pgrid, periodic, _ = case
    dc, dx, L, h, cut = geometry(case)
    ax = [np.arange(nlat) * dx] * dim
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, dim)[:, ::-1]     # x fastest
    x = np.zeros((len(g), 3))
    x[:, :dim] = g
    if kind.startswith("jitter"):
        amp, seed = float(kind[6:].split("-s")[0]), int(kind.split("-s")[1])
        rng = np.random.default_rng(1000 * seed + nlat)
        x[:, :dim] += amp * dx * rng.uniform(-1.0, 1.0, size=(len(x), dim))
        if not all(periodic):                    # a non-periodic axis is not wrapped: stay inside the box
            for a in range(dim):
                if not periodic[a]:
                    x[:, a] = np.clip(x[:, a], 0.0, L - 1e-9)
    elif kind == "at-hi":
        x[:, :dim] += 0.05 * dx * np.random.default_rng(5).uniform(-1.0, 1.0, size=(len(x), dim))
        if not all(periodic):
            for a in range(dim):
                if not periodic[a]:
                    x[:, a] = np.clip(x[:, a], 0.0, L - 1e-9)
        x[3, 0] = L                              # wraps to 0
    elif kind == "void":                         # nothing in the last rank's sub-box
        x[:, :dim] += 0.05 * dx * np.random.default_rng(6).uniform(-1.0, 1.0, size=(len(x), dim))
        if not all(periodic):
            for a in range(dim):
                if not periodic[a]:
                    x[:, a] = np.clip(x[:, a], 0.0, L - 1e-9)
        own = dc.owner(dc.wrap(x))
        if dc.nranks > 1:
            x = x[own != dc.nranks - 1]
    return np.ascontiguousarray(x)


def global_rows(case, x):
    """rows of the whole cloud as sets of (global id, sx, sy, sz), from workload.make_cloud (fully periodic; the images
    across a non-periodic axis are dropped)"""
    dim, nlat, pgrid, periodic, _ = case
    dc, dx, L, h, cut = geometry(case)
    from isph_amd import workload
    p = workload.make_cloud(x, [L] * dim, h, cut, dim=dim)
    n = p["nlocal"]
    own = p["owner_index"].astype(np.int64)
    sh = np.rint((p["x"] - p["x"][own]) / L).astype(np.int64)
    sh[:, dim:] = 0
    rows = []
    for i in range(n):
        j = p["neigh_idx"][p["neigh_ptr"][i]:p["neigh_ptr"][i + 1]]
        ok = np.ones(len(j), dtype=bool)
        for a in range(dim):
            if not periodic[a]:
                ok &= sh[j, a] == 0
        rows.append(sorted(zip(own[j[ok]].tolist(), *(sh[j[ok], a].tolist() for a in range(3)))))
    return p, rows
