"""numpy restatement of the device neighbour-list builder (isph_nlist_build, include/isph_hip.h) and the seeded clouds its
tests share: wrap, periodic images and a brute-force O(N^2) search with the formulas of the header, for any box origin and
any subset of periodic axes.  For lo = 0 and a fully periodic box it reproduces workload.make_cloud exactly
(tests/test_neighbours_host.py), which pins the expected values of the cases make_cloud cannot produce."""
import functools

import numpy as np

import isph_amd  # noqa: F401
from isph_amd import workload


def wrap(x, lo, hi, periodic, dim):
    """r = fmod(x - lo, P); r < 0: r += P; r >= P: r = 0; x = r + lo -- on the periodic axes"""
    x = np.array(x, dtype=np.float64, copy=True)
    for a in range(dim):
        if not periodic[a]:
            continue
        P = float(hi[a]) - float(lo[a])
        r = np.fmod(x[:, a] - float(lo[a]), P)
        r = np.where(r < 0.0, r + P, r)
        r = np.where(r >= P, 0.0, r)
        x[:, a] = r + float(lo[a])
    return x


def images(xw, lo, hi, periodic, cut, dim):
    """ghost positions [nghost, 3] and owners [nghost]: owners ascending, shifts in the loop order sz, sy, sx"""
    n = xw.shape[0]
    slo, shi = np.zeros((n, 3), dtype=np.int64), np.zeros((n, 3), dtype=np.int64)
    P = np.zeros(3)
    for a in range(dim):
        if not periodic[a]:
            continue
        P[a] = float(hi[a]) - float(lo[a])
        shi[xw[:, a] - float(lo[a]) < cut, a] = 1
        slo[xw[:, a] >= float(hi[a]) - cut, a] = -1
    gx, gown = [], []
    for i in np.nonzero(np.any(slo != 0, axis=1) | np.any(shi != 0, axis=1))[0]:
        p = xw[i]
        for sz in range(slo[i, 2], shi[i, 2] + 1):
            for sy in range(slo[i, 1], shi[i, 1] + 1):
                for sx in range(slo[i, 0], shi[i, 0] + 1):
                    if not (sx or sy or sz):
                        continue
                    gx.append((p[0] + sx * P[0], p[1] + sy * P[1], p[2] + sz * P[2] if dim == 3 else 0.0))
                    gown.append(i)
    return np.array(gx, dtype=np.float64).reshape(-1, 3), np.array(gown, dtype=np.int32)


def search(x_all, nlocal, cut, dim, chunk=256):
    """full list of the owned rows by brute force: rsq = ((d0 d0) + d1 d1) + d2 d2, every product and sum rounded (numpy
    rounds each array operation), rsq < cut cut, self excluded, rows ascending"""
    cutsq = float(cut) * float(cut)
    ptr = np.zeros(nlocal + 1, dtype=np.int64)
    rows = []
    for i0 in range(0, nlocal, chunk):
        xi = x_all[i0:min(nlocal, i0 + chunk)]
        d = xi[:, None, 0] - x_all[None, :, 0]
        rsq = d * d
        for a in range(1, dim):
            d = xi[:, None, a] - x_all[None, :, a]
            rsq = rsq + d * d
        hit = rsq < cutsq
        hit[np.arange(xi.shape[0]), i0 + np.arange(xi.shape[0])] = False
        r, c = np.nonzero(hit)                      # row-major: every row ascending
        ptr[i0 + 1:i0 + 1 + xi.shape[0]] = np.bincount(r, minlength=xi.shape[0])
        rows.append(c.astype(np.int32))
    np.cumsum(ptr, out=ptr)
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32))


def build(x_owned, lo, hi, periodic, cut, dim, do_wrap=True):
    """dict(x, owner_index, neigh_ptr (int64), neigh_idx, nlocal, nghost)"""
    lo, hi, periodic = (list(lo) + [0.0] * 3)[:3], (list(hi) + [1.0] * 3)[:3], (list(periodic) + [0] * 3)[:3]
    x = np.ascontiguousarray(x_owned, dtype=np.float64)
    n = x.shape[0]
    xw = wrap(x, lo, hi, periodic, dim) if do_wrap else x.copy()
    gx, gown = images(xw, lo, hi, periodic, cut, dim)
    x_all = np.ascontiguousarray(np.vstack([xw, gx]))
    own = np.concatenate([np.arange(n, dtype=np.int32), gown])
    ptr, idx = search(x_all, n, cut, dim)
    return dict(x=x_all, owner_index=own, neigh_ptr=ptr, neigh_idx=idx, nlocal=n, nghost=len(gown))


# ---- the seeded clouds of the tests -----------------------------------------------------------------------------------
TWO_PI = 2.0 * np.pi


def _tgv(dim, n, mode, cut_over_h, origin=None):
    if dim == 3:
        spec = workload.TGVSpec(dim=3, ncell=(n, n, n), mode=mode, cut_over_h=cut_over_h)
    else:
        spec = workload.TGVSpec(dim=2, ncell=(n, n), brick=(8, 8), origin=origin or (0.5, 0.5), mode=mode, cut_over_h=cut_over_h)
    p = workload.make_tgv(spec)
    return p, np.ascontiguousarray(p["x"][:p["nlocal"]])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(x [nlocal, 3], box (dim edges of the periodic box at the origin), h, cut, dim, like) of a periodic case"""
    if name == "lattice12":                                   # 3-D lattice 12^3, Wendland: 51 840 pairs on the cut radius
        p, x = _tgv(3, 12, workload.LATTICE, 2.0)
        return dict(x=x, box=(TWO_PI,) * 3, h=p["h"], cut=p["cut"], dim=3, like=p)
    if name in ("advect16", "wrap16"):                        # 3-D 16^3 ADVECT, Quintic cut 3 h, shuffled atom order
        p, x = _tgv(3, 16, workload.ADVECT, 3.0)
        rng = np.random.default_rng(20240611)
        x = np.ascontiguousarray(x[rng.permutation(x.shape[0])])
        if name == "wrap16":                                  # every coordinate moved by a multiple of L, a few special values
            x = x + TWO_PI * rng.integers(-3, 4, size=x.shape)
            x[5, 0], x[6, 1], x[7, 2], x[8, 0] = TWO_PI, -1e-17, -0.0, 3.0 * TWO_PI
            x[9] = (TWO_PI, -1e-17, -0.0)
        return dict(x=x, box=(TWO_PI,) * 3, h=p["h"], cut=p["cut"], dim=3, like=None)
    if name in ("jitter24_wendland", "jitter24_quintic"):     # 2-D 24^2 JITTER, origin 0.5
        p, x = _tgv(2, 24, workload.JITTER, 2.0 if name.endswith("wendland") else 3.0)
        return dict(x=x, box=(TWO_PI,) * 2, h=p["h"], cut=p["cut"], dim=2, like=p)
    if name in ("lattice7", "lattice5"):                      # L = 7 dx (5 dx: too short), cut = 3 dx
        m = 7 if name == "lattice7" else 5
        dx = 1.0
        g = np.arange(m) * dx
        x = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1])
        return dict(x=x, box=(m * dx,) * 3, h=1.5 * dx, cut=3.0 * dx, dim=3, like=None)
    if name == "clump":                                       # 6 000 particles in a ball of radius cut / 4 + 2 000 uniform
        rng = np.random.default_rng(77)
        cut, L = 1.0, 8.0
        d = rng.normal(size=(6000, 3))
        d *= (0.25 * cut * rng.random(6000) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
        x = np.vstack([np.array([0.1, 4.0, 4.0]) + d, L * rng.random((2000, 3))])
        x = np.ascontiguousarray(x[rng.permutation(8000)])
        return dict(x=x, box=(L,) * 3, h=0.5 * cut, cut=cut, dim=3, like=None)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def host_cloud(name):
    """workload.make_cloud of a periodic case (computed once, shared, never modified)"""
    c = case(name)
    return workload.make_cloud(c["x"], c["box"], c["h"], c["cut"], dim=c["dim"], like=c["like"])


@functools.lru_cache(maxsize=None)
def open_case(name):
    """the cases make_cloud cannot produce: non-periodic axes and a box that does not start at the origin"""
    if name == "open2d":
        rng = np.random.default_rng(5)
        lo, hi, per, cut = (0.0, 0.0), (1.0, 1.0), (1, 0), 0.08
        x = np.zeros((1500, 3))
        x[:, :2] = rng.random((1500, 2))
        x[:40, 0] += rng.integers(-2, 3, size=40)             # some outside along the periodic axis: wrapped
        x[40:60, 1] = -0.3 * rng.random(20)                   # some outside along the open axis: stay where they are
        x[60:80, 1] = 1.0 + 0.3 * rng.random(20)
        dim = 2
    elif name == "open3d":
        rng = np.random.default_rng(6)
        lo, ext, per, cut = (-1.0, 0.5, 2.0), np.array([2.0, 1.5, 1.0]), (1, 1, 0), 0.16
        hi = tuple(np.array(lo) + ext)
        x = np.array(lo) + ext * rng.random((3000, 3))
        x[:60, :2] += ext[:2] * rng.integers(-2, 3, size=(60, 2))
        x[60:90, 2] = lo[2] - 0.4 * rng.random(30)
        x[90:120, 2] = hi[2] + 0.4 * rng.random(30)
        x[120, 0], x[121, 1] = hi[0], lo[1]                   # on the faces
        dim = 3
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x)
    return dict(x=x, lo=lo, hi=hi, periodic=per, cut=cut, dim=dim, ref=build(x, lo, hi, per, cut, dim))


def assert_same(got, want):
    """x, owner_index, neigh_ptr and neigh_idx, every entry (pairs on the cut radius included)"""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items() if k in ("x", "owner_index", "neigh_ptr", "neigh_idx")}
    assert g["x"].shape == want["x"].shape and np.array_equal(g["x"], want["x"])
    assert np.array_equal(g["owner_index"], want["owner_index"])
    assert np.array_equal(g["neigh_ptr"].astype(np.int64), np.asarray(want["neigh_ptr"]).astype(np.int64))
    assert np.array_equal(g["neigh_idx"], want["neigh_idx"])
