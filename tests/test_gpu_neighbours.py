"""The device builder of ghost atoms and the full neighbour list (isph_nlist_build, hip.NeighbourList,
workload.make_cloud_device) against workload.make_cloud -- bit for bit: the same ghosts in the same order, the same
positions, owners, offsets and list entries, pairs on the cut radius included -- and against the numpy restatement
(tests/neighbours_reference.py) where make_cloud does not apply (non-periodic axes, a box away from the origin)."""
import ctypes as C

import numpy as np
import pytest
import torch

import isph_amd  # noqa: F401
from isph_amd import hip, workload
import neighbours_reference as nref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_list(ctx, c, x=None, **kw):
    dim = c["dim"]
    nl = hip.NeighbourList(ctx, c["x"] if x is None else x, (0.0,) * dim, c["box"], (1,) * dim, c["cut"], dim, **kw)
    got, info = nl.get(), nl.info
    nl.close()
    return got, info


def check_periodic(ctx, name, x=None):
    c, want = nref.case(name), nref.host_cloud(name)
    got, info = device_list(ctx, c, x=x)
    assert (info["nlocal"], info["nghost"], info["entries"]) == (want["nlocal"], want["nall"] - want["nlocal"], len(want["neigh_idx"]))
    assert str(got["neigh_ptr"].dtype).endswith("int32") and info["fits32"] == 1
    nref.assert_same(got, want)
    return got, info


def test_lattice_with_pairs_on_the_cut_radius(gpu_ctx):
    """12^3 lattice at the Wendland cut: 51 840 pairs lie on the cut radius, a fused rsq decides 288 of them differently"""
    _, info = check_periodic(gpu_ctx, "lattice12")
    assert (info["nlocal"], info["nghost"], info["entries"]) == (1728, 4104, 177392)


@pytest.mark.parametrize("side", ["host", "device"])
def test_shuffled_advected_cloud_quintic(gpu_ctx, side):
    c = nref.case("advect16")
    got, _ = check_periodic(gpu_ctx, "advect16", x=None if side == "host" else T(c["x"]))
    assert all(hip._is_torch(v) and v.is_cuda for v in got.values()) == (side == "device")


@pytest.mark.parametrize("name", ["jitter24_wendland", "jitter24_quintic"])
def test_two_dimensions(gpu_ctx, name):
    got, _ = check_periodic(gpu_ctx, name)
    n = nref.case(name)["x"].shape[0]
    assert np.all(got["x"][n:, 2] == 0.0)


def test_largest_ghost_multiplicity_and_the_box_that_is_too_short(gpu_ctx):
    _, info = check_periodic(gpu_ctx, "lattice7")
    assert info["nghost"] == 13 ** 3 - 7 ** 3
    c = nref.case("lattice5")                                    # L = 5 dx < 2 cut = 6 dx
    h = C.c_void_p()
    x = np.ascontiguousarray(c["x"])
    rc = hip.lib().isph_nlist_build(gpu_ctx.h, 3, x.shape[0], hip._ptr(x), (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(*c["box"]),
                                    (C.c_int * 3)(1, 1, 1), c["cut"], 1, 0, C.byref(h))
    assert rc == -1 and not h and b"two cuts" in hip.lib().isph_last_error()
    with pytest.raises(ValueError):
        workload.make_cloud_device(gpu_ctx, T(x), c["box"], c["h"], c["cut"], dim=3)


def test_wrap(gpu_ctx):
    """every coordinate displaced by a multiple of L in -3 .. 3, and L, -1e-17, -0.0 and 3 L themselves"""
    c = nref.case("wrap16")
    assert np.abs(c["x"]).max() > 3 * nref.TWO_PI and c["x"][5, 0] == nref.TWO_PI and c["x"][6, 1] == -1e-17
    got, _ = check_periodic(gpu_ctx, "wrap16")
    n = c["x"].shape[0]
    assert np.all(got["x"][:n] >= 0.0) and np.all(got["x"][:n] < nref.TWO_PI) and not np.any(np.signbit(got["x"][:n]))


def test_dense_clump_takes_the_long_row_path(gpu_ctx):
    """6 000 particles within a quarter of the cut of one point: a neighbourhood no LDS staging holds, rows of about 6 000
    entries that are sorted in global memory, beside rows short enough for the LDS sort"""
    want = nref.host_cloud("clump")
    lens = np.diff(want["neigh_ptr"].astype(np.int64))
    assert lens.max() > 5999 and (lens > 1024).sum() >= 6000 and (lens <= 1024).sum() >= 1500 and len(want["neigh_idx"]) > 3.5e7
    check_periodic(gpu_ctx, "clump")


@pytest.mark.parametrize("name", ["open2d", "open3d"])
def test_open_axes_and_a_box_away_from_the_origin(gpu_ctx, name):
    c = nref.open_case(name)
    nl = hip.NeighbourList(gpu_ctx, c["x"], c["lo"], c["hi"], c["periodic"], c["cut"], c["dim"])
    got, info = nl.get(), nl.info
    nl.close()
    assert info["nghost"] == c["ref"]["nghost"]
    nref.assert_same(got, c["ref"])


def test_without_wrap_the_positions_are_taken_as_they_are(gpu_ctx):
    c = nref.open_case("open3d")
    xw = nref.wrap(c["x"], list(c["lo"]), list(c["hi"]), list(c["periodic"]), 3)
    nl = hip.NeighbourList(gpu_ctx, xw, c["lo"], c["hi"], c["periodic"], c["cut"], 3, wrap=False)
    got = nl.get()
    nl.close()
    nref.assert_same(got, c["ref"])


def test_edges(gpu_ctx):
    c = nref.case("advect16")
    dim, box = 3, c["box"]
    nl = hip.NeighbourList(gpu_ctx, np.zeros((0, 3)), (0.0,) * 3, box, (1,) * 3, c["cut"], dim)       # no particles
    g, info = nl.get(), nl.info
    nl.close()
    assert info == dict(nlocal=0, nghost=0, entries=0, fits32=1)
    assert g["x"].shape == (0, 3) and g["owner_index"].shape == (0,) and list(g["neigh_ptr"]) == [0] and g["neigh_idx"].shape == (0,)
    one = np.array([[0.1, 3.0, nref.TWO_PI - 0.1]])                                                  # one particle: images, no neighbours
    nl = hip.NeighbourList(gpu_ctx, one, (0.0,) * 3, box, (1,) * 3, c["cut"], dim)
    g, info = nl.get(), nl.info
    nl.close()
    want = workload.make_cloud(one, box, c["h"], c["cut"], dim=3)
    assert info["nghost"] == 3 and info["entries"] == 0
    nref.assert_same(g, want)
    a, ia = device_list(gpu_ctx, c)                                                                  # deterministic
    b, ib = device_list(gpu_ctx, c)
    assert ia == ib and all(np.array_equal(a[k], b[k]) for k in a)
    nl = hip.NeighbourList(gpu_ctx, c["x"], (0.0,) * 3, box, (1,) * 3, c["cut"], dim)                # both offset widths
    assert nl.info["fits32"] == 1
    g32, g64 = nl.get(), nl.get(ptr64=True)
    nl.close()
    assert g32["neigh_ptr"].dtype == np.int32 and g64["neigh_ptr"].dtype == np.int64
    assert np.array_equal(g32["neigh_ptr"], g64["neigh_ptr"]) and g64["neigh_ptr"][-1] == len(g64["neigh_idx"])


def _poisson(ctx, d, vstar_owned):
    colmap = d["owner_index"]
    own = colmap.to(torch.int64)
    vfrac = hip.compute_volumes(ctx, d, colmap)[own].contiguous()
    A, b = hip.assemble_poisson(ctx, d, colmap, d["dt"], d["rho"], vstar_owned[own].contiguous(), vfrac=vfrac)
    rp, ci, v = A.export_csr()
    A.close()
    return rp, ci, v, b.cpu().numpy()


@pytest.mark.parametrize("which", ["caller", "bricks"])
def test_downstream_the_poisson_system_is_the_same(gpu_ctx, gpu_ctx_bricks, which):
    """the matrix and the right-hand side assembled from the device-built dict equal, bit for bit, those assembled from
    the uploaded host dict"""
    ctx = gpu_ctx if which == "caller" else gpu_ctx_bricks
    c, host = nref.case("jitter24_wendland"), nref.host_cloud("jitter24_wendland")
    like = c["like"]
    n = host["nlocal"]
    hd = dict(host)
    for k in ("x", "type", "neigh_ptr", "neigh_idx", "owner_index", "rho", "nu"):
        hd[k] = T(host[k])
    dd = workload.make_cloud_device(ctx, T(c["x"]), c["box"], c["h"], c["cut"], dim=2, like=like)
    assert set(dd) == set(host)
    for k, v in host.items():
        if isinstance(v, np.ndarray):
            assert hip._is_torch(dd[k]) and dd[k].is_cuda and str(dd[k].dtype) == "torch." + str(v.dtype), k
            assert np.array_equal(dd[k].cpu().numpy(), v), k
        else:
            assert dd[k] == v or dd[k] is v, k
    vstar = T(like["v"][:n])
    want, got = _poisson(ctx, hd, vstar), _poisson(ctx, dd, vstar)
    assert len(want[2]) > 20 * n and np.abs(want[3]).max() > 0.0
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
