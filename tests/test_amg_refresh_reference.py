"""-m "not gpu": tests/amg_refresh_reference.py, the helper the refresh tests of the SA-AMG compare the device with, against
the restatement of the whole set-up in tests/amg_shapes.py -- fed that restatement's own aggregates, it must give that
restatement's prolongators and operators within the rounding bounds that module keeps beside every entry
(4 k eps sum|terms|, the bound of a k-term float64 sum in any order)."""
import numpy as np
import pytest

import amg_refresh_reference as arr
import amg_shapes as S


@pytest.mark.parametrize("name", ["grid_21x13", "hub_17", "unsymmetric_150", "masked_grid_21x13"])
def test_helper_on_the_references_aggregates_gives_the_references_hierarchy(name):
    (rp, ci, v), nv, prm = S.fixture(name)
    H = S.fixture_reference(name)
    assert H.refusal is None and len(H.levels) >= 2
    aggs = [L.agg for L in H.levels[:-1]]
    omega = dict(S.DEFAULTS, **prm)["omega"]
    got = arr.hierarchy(rp, ci, v, aggs, nullvec=nv, omega=omega)
    assert len(got) == len(H.levels)
    for l, (g, L) in enumerate(zip(got, H.levels)):
        grp, gci, gv = g["A"]
        assert np.array_equal(grp, L.rp) and np.array_equal(gci, L.ci), (name, l)
        gapA = S.gap(gv, L.f64, L.bound())
        print("%s level %d: A gap %.3g" % (name, l, gapA))
        assert gapA <= 1.0, (name, l, gapA)
        assert np.allclose(g["nv"], H.nv[l], rtol=1e-14, atol=0)
        if l < len(H.levels) - 1:
            prp, pci, pv, pa, pk = L.P
            qrp, qci, qv = g["P"]
            assert np.array_equal(qrp, prp) and np.array_equal(qci, pci), (name, l)
            gapP = S.gap(qv, pv.astype(np.float64), 4.0 * pk * S.EPS * pa.astype(np.float64))
            print("%s level %d: P gap %.3g" % (name, l, gapP))
            assert gapP <= 1.0, (name, l, gapP)
            assert abs(g["rho"] - float(L.rho)) <= 4 * S.EPS * float(L.rho)


def test_helper_takes_given_lambdas_in_the_place_of_rho():
    (rp, ci, v), nv, prm = S.fixture("grid_21x13")
    H = S.fixture_reference("grid_21x13")
    aggs = [L.agg for L in H.levels[:-1]]
    a = arr.hierarchy(rp, ci, v, aggs)
    b = arr.hierarchy(rp, ci, v, aggs, lambdas=[lv["rho"] for lv in a[:-1]])
    c = arr.hierarchy(rp, ci, v, aggs, lambdas=[0.5 * lv["rho"] for lv in a[:-1]])
    for x, y in zip(a, b):
        assert np.array_equal(x["A"][2], y["A"][2])
    assert not np.array_equal(a[1]["A"][2], c[1]["A"][2]) and c[0]["damp"] == 2.0 * a[0]["damp"]
