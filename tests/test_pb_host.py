"""-m "not gpu": the Poisson-Boltzmann parameter defaults of the C ABI are the reference's (SolverNOX_Stratimikos,
solver_nox_impl.h:78-145, solver_nox_stratimikos.h:84-122; PairISPH pb defaults, pair_isph.cpp:1680-1698), and the
Python mirror agrees.  No GPU calls."""
import ctypes

from isph_amd import build, hip


def test_pb_params_default_are_the_reference_defaults():
    lib = ctypes.CDLL(build.build_hip())
    p = hip.PBParams.__new__(hip.PBParams)
    ctypes.Structure.__init__(p)
    lib.isph_pb_params_default.argtypes = [ctypes.c_void_p]
    lib.isph_pb_params_default.restype = None
    lib.isph_pb_params_default(ctypes.byref(p))
    assert (p.kappasq, p.gamma, p.linearized) == (1.0, 0.0, 0)
    assert (p.max_iters, p.f_tol, p.update_tol) == (100, 1e-8, 1e-5)
    assert (p.prec_max_age, p.prec_kind) == (10, 0)
    assert p.linear.solver_type == 0 and p.linear.flexible == 1
    assert (p.linear.tol, p.linear.max_iters) == (1e-6, 80)
    a = hip.AmgParams()
    assert [getattr(p.amg, f) for f, _ in hip.AmgParams._fields_] == [getattr(a, f) for f, _ in hip.AmgParams._fields_]


def test_python_pb_params_agree_with_the_c_defaults():
    lib = ctypes.CDLL(build.build_hip())
    c = hip.PBParams.__new__(hip.PBParams)
    ctypes.Structure.__init__(c)
    lib.isph_pb_params_default.argtypes = [ctypes.c_void_p]
    lib.isph_pb_params_default(ctypes.byref(c))
    p = hip.PBParams()
    assert ctypes.sizeof(p) == ctypes.sizeof(hip.PBParams)
    assert bytes(p) == bytes(c)
    q = hip.PBParams(kappasq=100.0, prec_max_age=1, linear=dict(tol=1e-13, max_iters=400))
    assert (q.kappasq, q.prec_max_age, q.linear.tol, q.linear.max_iters, q.linear.num_blocks) == (100.0, 1, 1e-13, 400, 50)
