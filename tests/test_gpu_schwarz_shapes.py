"""-m gpu: the branches of the additive-Schwarz layer (csrc/schwarz.hpp) on the constructed fixtures of
tests/schwarz_shapes.py against its long-double reference.

tests/test_schwarz_shapes_host.py shows, without a GPU, WHICH branch each fixture reaches (the regime table in its
docstring) and that the oracle agrees with the reference.  Here the device first confirms the branch -- schwarz_info() and
paths() against schwarz_shapes.model on the factor it exported -- and then the values: row lists, loc_ptr and factor
pattern exact; factor values under the project's entrywise rule (relative 1e-10, floor 1e-10 max|f|); application within
1e-11; the default form against level_launches=True on the same matrix: factor bit for bit, application within 1e-13 of
max|z|; a second application with the bits of the first.

Every test prints the device's deviation from the reference beside the oracle's."""
import numpy as np
import pytest

from isph_amd import hip
import oracle as orc
import ilu_shapes as sh
import schwarz_shapes as ss
from test_gpu_ilu_shapes import entrywise, rel, rhs
from test_schwarz_shapes_host import CASES, CONDITIONS, check_conditions, own_ptr

pytestmark = pytest.mark.gpu


def check_paths(label, M, R):
    """the device's own account of the way it went against the model on the factor it exported"""
    info, p = M.schwarz_info(), M.paths()
    print("%s: %s %s" % (label, info, p))
    for k in ("nloc", "nnz", "nsub", "levels_l", "levels_u", "maxrow", "persistent"):
        assert info[k] == R[k], (label, k, info[k], R[k])
    for k in ("sub_maxrows", "long_rows", "factor_waves", "hbits", "nrun_l", "nrun_u", "n4l", "n4u", "rows_on_device", "symbolic1_on_device"):
        assert p[k] == R[k], (label, k, p[k], R[k])
    if R["persistent"] == 1:
        assert p["runs_near_l"] == R["runs_near_l"] and p["runs_near_u"] == R["runs_near_u"], label


@pytest.mark.parametrize("name,K,overlap", CASES)
def test_schwarz_on_every_constructed_shape(gpu_ctx, name, K, overlap):
    rp, ci, val, bp = ss.fixture(name)
    n, B = len(rp) - 1, ss.block_size(name)
    ref = ss.ref_schwarz_of(name, K, overlap)
    rows, lp, frp, fci, fv, subs = ref
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    r = rhs(n)
    for combine in ("add", "zero") if overlap else ("add",):
        O = orc.Schwarz(rp, ci, val, K, own_ptr(name), overlap, combine)
        zo = ss.ref_apply(ref, combine, r)
        out = {}
        for form in ("level launches", "default"):
            M = hip.PrecondSchwarz(gpu_ctx, A, level_of_fill=K, overlap=overlap, combine=combine, block_size=B,
                                   level_launches=form == "level launches")
            label = "%s fill %d overlap %d %s, %s" % (name, K, overlap, combine, form)
            grow, glp, grp, gci, gv = M.export()
            R = ss.model(grp, gci, glp, level_launches=form == "level launches", fill=K, wmax=int(np.diff(rp).max()))
            check_paths(label, M, R)
            if form == "default":
                check_conditions(CONDITIONS[(name, K, overlap)], R)
            assert np.array_equal(grow, rows) and np.array_equal(glp, lp)      # row lists, loc_ptr: exact
            assert np.array_equal(grp, frp) and np.array_equal(gci, fci)       # factor pattern: exact
            z = M.apply(r)
            z2 = M.apply(r)
            print("  factor entrywise device %.2e (oracle %.2e), apply device %.2e (oracle %.2e)" %
                  (entrywise(gv, fv), entrywise(O.export()[4], fv), rel(z, zo), rel(O.apply(r), zo)))
            assert entrywise(gv, fv) < 1e-10
            assert rel(z, zo) < 1e-11
            assert np.array_equal(z, z2), label                                # second application: same bits
            out[form] = (gv, z)
            M.close()
        assert np.array_equal(out["default"][0], out["level launches"][0])     # factor: bit for bit
        zl, z = out["level launches"][1], out["default"][1]
        assert np.max(np.abs(z - zl)) <= 1e-13 * np.max(np.abs(zl))
    A.close()


@pytest.mark.parametrize("label", sorted(ss.REFUSALS))
def test_refusals_by_their_text_and_the_context_stays_usable(gpu_ctx, label):
    make, B, level_launches, text = ss.REFUSALS[label]
    rp, ci, val, bp = make()
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    with pytest.raises(hip.IsphError, match=text):
        hip.PrecondSchwarz(gpu_ctx, A, level_of_fill=0, overlap=0, block_size=B, level_launches=level_launches)
    A.close()
    grp, gci, gval, gbp = sh.fixture("one_narrow")
    G = hip.Matrix.from_csr(gpu_ctx, grp, gci, gval)
    M = hip.PrecondSchwarz(gpu_ctx, G, level_of_fill=0, overlap=0, block_size=0, level_launches=level_launches)
    r = rhs(len(grp) - 1)
    assert rel(M.apply(r), sh.ref_apply_of("one_narrow", 0, r)) < 1e-11
    M.close(); G.close()
