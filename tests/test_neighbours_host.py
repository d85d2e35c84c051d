"""-m "not gpu": the C ABI of the device neighbour-list builder (isph_nlist_*) is exported, the binding refuses bad
arguments before any library call, and tests/neighbours_reference.py -- the numpy restatement the GPU tests compare the
non-periodic cases with -- reproduces workload.make_cloud exactly where make_cloud applies."""
import ctypes

import numpy as np
import pytest

import isph_amd  # noqa: F401
from isph_amd import build, hip, workload
import neighbours_reference as nref

NLIST = ["isph_nlist_build", "isph_nlist_info", "isph_nlist_get", "isph_nlist_destroy"]


def test_the_library_exports_the_nlist_entry_points():
    lib = ctypes.CDLL(build.build_hip())
    for name in NLIST:
        assert hasattr(lib, name), "missing export: " + name
        assert name in hip.EXPORTS


def test_bad_arguments_are_refused_before_any_library_call():
    x = np.zeros((10, 3))
    box = dict(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), periodic=(1, 1, 1))
    for bad in (dict(x=np.zeros((10, 2))), dict(x=np.zeros(30)), dict(cut=0.0), dict(cut=-1.0), dict(cut=0.6),
                dict(hi=(1.0, 0.3, 1.0), cut=0.2), dict(dim=4)):
        kw = dict(dict(x=x, cut=0.2, dim=3, **box), **bad)
        with pytest.raises(ValueError):
            hip.NeighbourList(None, kw["x"], kw["lo"], kw["hi"], kw["periodic"], kw["cut"], kw["dim"])   # ctx None: never reached
    with pytest.raises(ValueError):                              # the third axis is not looked at in 2-D, the second is
        hip.NeighbourList(None, x, (0.0, 0.0), (1.0, 0.3), (1, 1), 0.2, 2)
    with pytest.raises(ValueError):
        workload.make_cloud_device(None, x, (1.0, 1.0, 0.3), 0.1, 0.2, dim=3)


@pytest.mark.parametrize("name", ["lattice12", "advect16", "wrap16", "jitter24_wendland", "jitter24_quintic", "lattice7"])
def test_the_reference_reproduces_make_cloud(name):
    c, want = nref.case(name), nref.host_cloud(name)
    dim = c["dim"]
    got = nref.build(c["x"], (0.0,) * dim, c["box"], (1,) * dim, c["cut"], dim)
    assert got["nghost"] == want["nall"] - want["nlocal"]
    nref.assert_same(got, want)


def test_the_lattice_has_the_counts_the_rounding_rule_was_checked_on():
    want = nref.host_cloud("lattice12")
    assert (want["nlocal"], want["nall"] - want["nlocal"], len(want["neigh_idx"])) == (1728, 4104, 177392)
    want = nref.host_cloud("lattice7")                            # six of seven planes per axis have an image
    assert want["nall"] - want["nlocal"] == 13 ** 3 - 7 ** 3
    c = nref.case("lattice5")
    with pytest.raises(ValueError):
        workload.make_cloud(c["x"], c["box"], c["h"], c["cut"], dim=3)


def test_the_open_cases_are_what_they_claim():
    for name, nper in (("open2d", 1), ("open3d", 2)):
        c = nref.open_case(name)
        r = c["ref"]
        x, n = r["x"], r["nlocal"]
        for a in range(c["dim"]):
            if c["periodic"][a]:
                assert np.all(x[:n, a] >= c["lo"][a]) and np.all(x[:n, a] < c["hi"][a])
            else:
                assert np.array_equal(x[:n, a], c["x"][:, a]) and np.array_equal(x[n:, a], x[r["owner_index"][n:], a])
                assert np.any(x[:n, a] < c["lo"][a]) and np.any(x[:n, a] > c["hi"][a])
        assert 0 < r["nghost"] and sum(c["periodic"]) == nper
        lens = np.diff(r["neigh_ptr"])
        assert lens.min() >= 0 and lens.max() > 8
