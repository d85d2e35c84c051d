"""-m "not gpu": tests/ins_reference.py against hand-computed cases, and the bindings of the step primitives refusing
operands shorter than the ABI reads (the check comes before any library call: no device needed)."""
import math

import numpy as np
import pytest

import isph_amd  # noqa: F401
from isph_amd import hip
import ins_reference as R


def test_zero_mean_pressure_by_hand():
    # owned: fluid 1, solid NaN, fluid 3, buffers 5 and 7; ghosts: solid 9, fluid 11
    kinds = [R.FLUID, R.SOLID, R.BUFFER_DIRICHLET, R.BUFFER_NEUMANN]
    typ = np.array([1, 2, 1, 3, 4, 2, 1])
    f = np.array([1.0, np.nan, 3.0, 5.0, 7.0, 9.0, 11.0])
    g, mean, count, abs_sum = R.zero_mean_pressure(f, 5, typ, kinds, True)
    assert (mean, count, abs_sum) == (4.0, 4, 16.0)
    assert g.tolist() == [-3.0, 0.0, -1.0, 1.0, 3.0, 9.0, 7.0]              # the Solid ghost keeps its 9
    g, mean, _, _ = R.zero_mean_pressure(f, 5, typ, kinds, False)
    assert mean == 4.0 and g.tolist() == [1.0, 0.0, 3.0, 5.0, 7.0, 9.0, 11.0]
    g, mean, count, _ = R.zero_mean_pressure([2.0, 1e300, 5.0], 2, [1, 1, 1], [R.SOLID], True)
    assert (mean, count) == (0.0, 0) and g.tolist() == [0.0, 0.0, 5.0]       # nothing enters: mean 0, nothing subtracted


def test_status_by_hand():
    x = np.array([[0.0, 0, 0], [3.0, 4.0, 0], [1.0, 0, 0], [0, 0, 9.0]])
    v = np.array([[1.0, 2.0, 2.0], [0, 0, 10.0], [0, 3.0, 4.0], [100.0, 0, 0]])
    typ = np.array([1, 1, 2, 3])
    vfrac = np.array([0.5, 0.25, 2.0, 1.0])
    rho = np.array([2.0, 4.0, 1.0, 1.0])
    st, ab = R.status(x, typ, vfrac, v, rho, 4, type_mask=0b011, centre=(0, 0, 0), radius=5.0)
    # rows 0, 1, 2: masses 1, 1, 2; |v|^2 = 9, 100, 25
    assert st.tolist() == [3.0, 1.0, 5.0, 16.0, 2.75, 4.0, 0.5 * 9 + 0.5 * 100 + 25.0, 10.0]
    assert ab[1] == 1.0 and ab[3] == 16.0
    st, _ = R.status(x, typ, vfrac, v, rho, 4, type_mask=0b011, centre=(0, 0, 0), radius=4.999)
    assert st[7] == 5.0                                                     # row 1 sits at r = 5 exactly: outside now
    st, _ = R.status(x, typ, vfrac, v, rho, 4, type_mask=-1, centre=(0, 0, 0), radius=0.0)
    assert st[0] == 4.0 and st[7] == 0.0                                     # radius 0: no maximum is taken
    st, _ = R.status(x, typ, vfrac, v, rho, 2, type_mask=0b100)
    assert st.tolist() == [0.0] * 8                                         # owned rows only; none of type 3 among them


def test_tgv_error_by_hand():
    umax, nu, rho, t = 0.5, 0.25, 2.0, 1.0
    x = np.array([[0.0, 0.0, 0.0], [math.pi / 2, 0.0, 0.0]])
    # exact: p = 0.25 rho (cos 2x + cos 2y) umax^2 e^{-4 nu t} -> (0.25 e^-1, 0);  u = (0, 0) and (umax e^{-1/2}, 0)
    e1, eh = math.exp(-1.0), math.exp(-0.5)
    uex, pex = R.tgv_exact(x, t, umax, np.full(2, nu), np.full(2, rho))
    assert np.allclose(pex, [0.25 * e1, 0.0], atol=1e-17) and np.allclose(uex[1], [umax * eh, 0, 0], atol=1e-16)
    # the state: the exact pressure plus a constant (removed with the mean) and a velocity off by (0, 0, 0.1) in row 0
    p = pex + 3.0
    p_mean_dev = 3.0 + pex.mean()                                          # what the reference subtracts
    vn = uex.copy()
    vn[0, 2] = 0.1
    got = R.tgv_error(x, vn, p, np.full(2, rho), np.full(2, nu), t, umax, 2)
    want_p = math.sqrt(((3.0 - p_mean_dev) ** 2 * 2) / 2)
    assert abs(got[0] - want_p) < 1e-15
    assert abs(got[1] - math.sqrt((0.25 * e1) ** 2 / 2)) < 1e-16
    assert abs(got[2] - math.sqrt(0.01 / 2)) < 1e-16
    assert abs(got[3] - math.sqrt((umax * eh) ** 2 / 2)) < 1e-16


def test_step_primitives_are_declared_and_exported():
    for name in ("isph_ghost_fill", "isph_zero_mean_pressure", "isph_status", "isph_tgv_error"):
        assert name in hip.EXPORTS
        assert hasattr(hip.lib(), name)


def test_driver_entry_points_are_declared_and_ins_params_mirrors_the_defaults():
    for name in ("isph_ins_params_default", "isph_ins_create", "isph_ins_destroy", "isph_ins_set_state", "isph_ins_set_list",
                 "isph_ins_rebuild", "isph_ins_sizes", "isph_ins_get", "isph_ins_pre", "isph_ins_view", "isph_ins_force",
                 "isph_ins_add_force", "isph_ins_solve", "isph_ins_advance", "isph_ins_shift", "isph_ins_diagnostics",
                 "isph_ins_run"):
        assert name in hip.EXPORTS and hasattr(hip.lib(), name)
    p = hip.InsParams(2, 0.01, 0.3, 0.6, kinds=[99, 12], box=([0, 0, 0], [6, 6, 1], [1, 1, 0]), theta=0.25, g=(0, -9.81, 0),
                      prec_poisson="sa-amg", shift=0.05, shiftcut=0.6)
    c = p.c
    # what isph_ins_params_default wrote, behind the fields set here: a wrong struct layout would scramble them
    assert (c.dim, c.antisym, c.incremental_pressure, c.singular_mode, c.ntypes) == (2, 1, 1, hip.NULLSPACE, 2)
    assert (c.theta, c.dt, c.cut, c.shift, c.shiftcut, c.nonfluidweight, c.tgv_umax) == (0.25, 0.01, 0.6, 0.05, 0.6, 0.1, 0.1)
    assert (c.prec_helmholtz, c.helmholtz_block_size, c.prec_poisson, c.poisson_block_size) == (b"bjacobi-ilu0", 512, b"sa-amg", 512)
    assert (c.solver.num_blocks, c.solver.max_iters, c.solver.tol, c.solver.basis_bits) == (50, 500, 1e-8, 64)
    assert list(c.g) == [0.0, -9.81, 0.0] and list(c.hi) == [6.0, 6.0, 1.0] and list(c.periodic) == [1, 1, 0]
    assert (c.block_helmholtz, c.morris_holmes, c.normals_bd_coord, c.normals_use_part, c.recycle) == (0, 0, 0, 0, None)
    assert c.status_type_mask == -1 and c.status_radius == 0.0
    assert list(p._kind) == [0, 99, 12] and p._h.shape == (3, 3) and p._cutsq[1, 2] == 0.36
    with pytest.raises(TypeError):
        hip.InsParams(2, 0.01, 0.3, 0.6, thetta=0.5)


def test_bindings_refuse_operands_shorter_than_the_abi_reads():
    own = np.arange(10, dtype=np.int32) % 6
    with pytest.raises(ValueError):
        hip.ghost_fill(None, 6, own, np.zeros((9, 3)))                       # a row short
    with pytest.raises(ValueError):
        hip.ghost_fill(None, 6, own, np.zeros(9))
    with pytest.raises(ValueError):
        hip.ghost_fill(None, 11, own, np.zeros((10, 3)))                     # nlocal > nall
    with pytest.raises(ValueError):
        hip.ghost_fill(None, 6, own, np.zeros((10, 3), dtype=np.float32))    # would be converted, not updated in place
    typ = np.ones(10, dtype=np.int32)
    with pytest.raises(ValueError):
        hip.zero_mean_pressure(None, 6, typ, [99], np.zeros(9))
    with pytest.raises(ValueError):
        hip.zero_mean_pressure(None, 11, typ, [99], np.zeros(10))
    ok = dict(x=np.zeros((10, 3)), type=typ, vfrac=np.ones(10), v=np.zeros((10, 3)), rho=np.ones(10))
    for k, short in (("x", np.zeros((9, 3))), ("type", typ[:9]), ("vfrac", np.ones(9)), ("v", np.zeros((10, 2))), ("rho", np.ones(3))):
        with pytest.raises(ValueError):
            hip.status(None, 10, **dict(ok, **{k: short}))
    ok = dict(x=np.zeros((10, 3)), vnp1=np.zeros((10, 3)), p=np.zeros(10), rho=np.ones(10), nu=np.ones(10))
    for k, short in (("x", np.zeros((10, 2))), ("vnp1", np.zeros((9, 3))), ("p", np.zeros(9)), ("rho", np.ones(9)), ("nu", np.ones(0))):
        with pytest.raises(ValueError):
            hip.tgv_error(None, 10, t=0.0, umax=0.1, **dict(ok, **{k: short}))
