"""Host checks behind tests/test_gpu_basis_f32.py (no GPU): what GMRES with the Krylov basis stored in single precision
(isph_solver_params::basis_bits = 32) is expected to compute, from the numpy restatement tests/krylov_cb_reference.py.

  * bits = 64: the restatement (Givens recurrence, DGKS or ICGS with the device's norm formula) returns the iterates of
    krylov_reference.gmres_iterates (dense least squares, two full passes) to round-off.
  * bits = 32: every stored vector is its own float rounding, and the Arnoldi relation holds for the STORED vectors up to
    the one rounding per column: |Op Z_j - V_{j+1} Hbar_j| <= 2^-24 |h_{j+1,j}| |v_{j+1}| (+ fp64 round-off) -- and is
    not zero, which is the error term behind the residual floor.
  * the table of the feature: FGMRES(50), two passes (ICGS), tol 1e-8, zero start.  The recurrence converges in the
    iteration count of the fp64 basis; without the confirmation the true residual is left above tol wherever the solve did
    not restart anyway, with it the true residual is at or below tol at the cost of one restart and 0-4 iterations.
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import chebyshev_reference as cr
import krylov_cb_reference as cb
import krylov_reference as kr

TOL = 1e-8
KS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 61, 62]


@functools.lru_cache(maxsize=None)
def fixture(name):
    rp, ci, val, b, singular = cr.system(name)
    n = len(rp) - 1
    A = sps.csr_matrix((val, ci, rp), shape=(n, n))
    return rp, ci, val, A, b, (kr.unit_null(None, n) if singular else None)


@functools.lru_cache(maxsize=None)
def tgv(singular):
    rp, ci, val = kr.tgv_rows(None if singular else kr.SHIFT)
    n = len(rp) - 1
    A = sps.csr_matrix((val, ci, rp), shape=(n, n))
    return rp, ci, val, A, np.random.default_rng(7).standard_normal(n), (kr.unit_null(None, n) if singular else None)


@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("prec", ["none", "jacobi"])
@pytest.mark.parametrize("ortho", [cb.DGKS, cb.ICGS])
@pytest.mark.parametrize("flexible", [True, False])
def test_64_bits_are_the_plain_iterates(singular, prec, ortho, flexible):
    rp, ci, val, A, b, null = tgv(singular)
    n = A.shape[0]
    minv = kr.minv_for(prec, rp, ci, val)
    ref = kr.gmres_iterates(A, b, np.zeros(n), KS, 62, minv, null)
    got = cb.iterates(A, b, np.zeros(n), KS, 62, 64, ortho, minv, null, flexible)
    worst = 0.0
    for k in KS:
        if ref[k].rel_res < 1e-10:
            continue
        gap = kr.iterate_gap(got[k].x, ref[k].x)
        worst = max(worst, gap)
        assert gap <= 1e-11, (k, gap)
        assert abs(got[k].rec_res - ref[k].rel_res) <= 1e-12, (k, got[k].rec_res, ref[k].rel_res)
        if ortho == cb.ICGS:
            assert got[k].reorth == k
        elif ref[k].dgks_margin() > 1e-6:
            assert got[k].reorth == ref[k].dgks_second_passes(), (k, got[k].reorth)
    print("cb-reference bits 64 s%d %s o%d f%d: worst gap to krylov_reference %.2e" % (singular, prec, ortho, flexible, worst))


@pytest.mark.parametrize("m", [1, 5])
def test_64_bits_restarted(m):
    rp, ci, val, A, b, null = tgv(True)
    n = A.shape[0]
    x0 = np.random.default_rng(8).standard_normal(n)
    minv = kr.minv_for("jacobi", rp, ci, val)
    ref = kr.gmres_iterates(A, b, x0, [13], m, minv, null)[13]
    got = cb.iterates(A, b, x0, [13], m, 64, cb.DGKS, minv, null)[13]
    assert kr.iterate_gap(got.x, ref.x) <= 1e-12 and got.restarts == 12 // m


@pytest.mark.parametrize("singular", [True, False])
@pytest.mark.parametrize("ortho", [cb.DGKS, cb.ICGS])
def test_32_bits_store_rounded_vectors_and_keep_the_arnoldi_relation(singular, ortho):
    rp, ci, val, A, b, null = tgv(singular)
    n = A.shape[0]
    res = cb.gmres_cb(A, b, np.zeros(n), 30, 32, ortho, kr.minv_for("jacobi", rp, ci, val), null, tol=0.0, max_iters=45,
                      keep_cycles=True)
    assert res.iters == 45 and res.restarts == 1 and len(res.cycles) == 2
    worst, least = 0.0, np.inf
    for cyc in res.cycles:
        assert np.array_equal(cyc.V, cyc.V.astype(np.float32).astype(np.float64))
        assert np.max(np.abs(np.linalg.norm(cyc.V, axis=1) - 1.0)) <= 2e-7
        for j, (defect, hv) in enumerate(cb.arnoldi_defects(cyc)):
            worst, least = max(worst, defect / hv), min(least, defect / hv)
            assert defect <= 2.0 ** -24 * hv + 1e-13 * np.linalg.norm(cyc.AZ[j]), (j, defect, hv)
            assert defect > 0.0
    print("cb-reference bits 32 s%d o%d: Arnoldi defect / (|h| |v|) in [%.2e, %.2e], 2^-24 = %.2e" %
          (singular, ortho, least, worst, 2.0 ** -24))
    assert least >= 1e-9      # the rounding is there: a defect at fp64 round-off would mean nothing was rounded
    r64 = cb.gmres_cb(A, b, np.zeros(n), 30, 64, ortho, kr.minv_for("jacobi", rp, ci, val), null, tol=0.0, max_iters=45,
                      keep_cycles=True)
    for cyc in r64.cycles:
        for j, (defect, hv) in enumerate(cb.arnoldi_defects(cyc)):
            assert defect <= 1e-13 * max(hv, np.linalg.norm(cyc.AZ[j]))


def test_32_bit_iterates_differ_from_the_64_bit_ones_at_the_float_level():
    rp, ci, val, A, b, null = tgv(False)
    n = A.shape[0]
    i32 = cb.iterates(A, b, np.zeros(n), [17], 62, 32, cb.DGKS, None, None)[17]
    i64 = cb.iterates(A, b, np.zeros(n), [17], 62, 64, cb.DGKS, None, None)[17]
    sep = kr.iterate_gap(i32.x, i64.x)
    print("cb-reference separation of the 32- and 64-bit iterates at k = 17: %.2e" % sep)
    assert 1e-10 <= sep <= 1e-5


# system, preconditioner -> (fp64: iterations, restarts), (f32 recurrence only), (f32 confirmed)
TABLE = {
    ("tgv16", "jacobi"): ((30, 0), (30, 0), (31, 1)),
    ("tgv16", "bjacobi-ilu0"): ((28, 0), (28, 0), (29, 1)),
    ("wall42", "jacobi"): ((109, 2), (109, 2), (109, 2)),
    ("stencil", "jacobi"): ((40, 0), (40, 0), (42, 1)),
    ("spd", "jacobi"): ((53, 1), (55, 1), (55, 1)),
}


@pytest.mark.parametrize("name,prec", sorted(TABLE))
def test_the_table_of_the_feature(name, prec):
    rp, ci, val, A, b, null = fixture(name)
    n = A.shape[0]
    minv = kr.minv_for(prec, rp, ci, val)
    want64, want_rec, want_conf = TABLE[(name, prec)]

    def run(bits, confirm):
        return cb.gmres_cb(A, b, np.zeros(n), 50, bits, cb.ICGS, minv, null, tol=TOL, max_iters=500, max_restarts=15,
                           confirm=confirm)
    r64, rec, conf = run(64, True), run(32, False), run(32, True)
    for label, r in (("fp64 basis", r64), ("f32 recurrence only", rec), ("f32 confirmed", conf)):
        print("cb-table %-8s %-13s %-20s iters %3d restarts %d (residual %d) true rel. residual %.2e" %
              (name, prec, label, r.iters, r.restarts, r.residual_restarts, r.true_res))
    assert (r64.iters, r64.restarts) == want64 and r64.converged and r64.true_res <= TOL
    assert (rec.iters, rec.restarts) == want_rec and rec.converged and rec.residual_restarts == 0
    assert (conf.iters, conf.restarts) == want_conf and conf.converged
    assert conf.true_res <= TOL
    if want_conf == want_rec:      # the solve restarts anyway: the confirmation passes at once
        assert conf.residual_restarts == 0 and rec.true_res <= TOL
    else:                          # one cycle: the float basis leaves the true residual above tol
        assert conf.residual_restarts == 1 and TOL < rec.true_res <= 5e-8
    assert r64.residual_restarts == 0
