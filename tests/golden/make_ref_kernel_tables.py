"""Regenerates ref_kernel_tables.npz: what the reference's own KernelFuncWendland / Quintic / Cubic, kind filters,
sphOperator and MirrorNothing return (oracle/_ref/libisph_refkernels.so, built by oracle/build.py where the reference
sources are present) on the inputs of

  tests/test_oracle.py::test_oracle_kernels_equal_the_reference_kernel_classes
  tests/test_gpu_reference_tables.py::test_device_kernel_values_equal_the_reference_kernel_classes

The inputs are rebuilt here from the same seeds and stored beside the outputs, so the tests need neither the reference
nor oracle/_ref.  Run from the repo root where oracle/_ref can be built:  python tests/golden/make_ref_kernel_tables.py
"""
import ctypes
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_kernel_tables.npz")

KINDS = [99, 12, 127, 1, 2, 4, 8, 32, 64]            # every particle kind of pair_isph.h:113-138 and the filters in use
FILTERS = [99, 12, 127]
MATCH_FI = [99, 12]
MATCH_FJ = [99, 99 - 64, 127]
OPERATOR_ARGS = [(1.5, -0.25), (0.0, 3.0), (-2.0, -2.0), (1e-300, 1e300)]
KERNELS = ((0, "wendland", 2.0), (1, "quintic", 3.0), (2, "cubic", 2.0))
ORACLE_H = (1.5 * 2 * np.pi / 100, 0.037, 1.0)
DEVICE_H = 0.0942


def oracle_radii():
    """the radii of the oracle test, in its loop order: {(kernel, dim, index of h): r}"""
    rng = np.random.default_rng(1)
    out = {}
    for kernel, _, support in KERNELS:
        for dim in (2, 3):
            for hi, h in enumerate(ORACLE_H):
                s = np.concatenate([rng.uniform(0.0, support + 0.3, 400), np.arange(0.0, support + 0.51, 0.5),
                                    np.nextafter(np.arange(1.0, support + 0.1, 1.0), 0.0)])
                out[(kernel, dim, hi)] = np.ascontiguousarray(s * h)
    return out


def device_pairs(support, h=DEVICE_H):
    """the isolated particle pairs of the device test: (pair distances handed over, positions along x, the distance the
    device sees)"""
    s = np.concatenate([np.random.default_rng(2).uniform(0.02, support, 500), np.arange(0.5, support, 0.5),
                        support + np.array([1e-9, 0.1, 0.4])])     # the last three: listed neighbours outside the cut
    r = np.ascontiguousarray(s * h)
    npair = len(r)
    x = np.zeros((2 * npair, 3))
    x[0::2, 0] = 10.0 * np.arange(npair)                              # pairs far apart from each other
    x[1::2, 0] = x[0::2, 0] + r
    rr = np.ascontiguousarray(x[1::2, 0] - x[0::2, 0])
    return r, x, rr


def load_ref():
    spec = importlib.util.spec_from_file_location("_oracle_build", os.path.join(ROOT, "oracle", "build.py"))
    ob = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ob)
    path = ob.build_ref()
    if not (path and os.path.exists(path)):
        raise SystemExit("oracle/_ref/libisph_refkernels.so could not be built here: the reference sources are needed")
    ref = ctypes.CDLL(path)
    ref.ref_kernel_table.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]
    ref.ref_kernel_val.restype = ctypes.c_double
    ref.ref_kernel_val.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    ref.ref_sph_operator.restype = ctypes.c_double
    ref.ref_sph_operator.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double]
    ref.ref_mirror_nothing.restype = ctypes.c_double
    ref.ref_mirror_nothing.argtypes = [ctypes.c_double]
    return ref


def table(ref, kernel, dim, h, r):
    w, dw = np.zeros_like(r), np.zeros_like(r)
    ref.ref_kernel_table(kernel, dim, h, len(r), r.ctypes.data, w.ctypes.data, dw.ctypes.data)
    return w, dw


def main():
    ref = load_ref()
    out = {}
    nk, nf = len(KINDS), len(FILTERS)
    yes1 = np.zeros((nf, nk), np.int8)
    yes2 = np.zeros((nf, nf, nk, nk), np.int8)
    for a, fi in enumerate(FILTERS):
        for i, ik in enumerate(KINDS):
            yes1[a, i] = ref.ref_filter_yes1(fi, ik)
            for b, fj in enumerate(FILTERS):
                for j, jk in enumerate(KINDS):
                    yes2[a, b, i, j] = ref.ref_filter_yes2(fi, fj, ik, jk)
    myes1 = np.zeros((len(MATCH_FI), nk), np.int8)
    myes2 = np.zeros((len(MATCH_FI), len(MATCH_FJ), nk, nk), np.int8)
    for a, fi in enumerate(MATCH_FI):
        for i, ik in enumerate(KINDS):
            myes1[a, i] = ref.ref_filter_match_yes1(fi, ik)
            for b, fj in enumerate(MATCH_FJ):
                for j, jk in enumerate(KINDS):
                    myes2[a, b, i, j] = ref.ref_filter_match_yes2(fi, fj, ik, jk)
    out.update(filter_yes1=yes1, filter_yes2=yes2, filter_match_yes1=myes1, filter_match_yes2=myes2)
    out["sph_operator"] = np.array([[ref.ref_sph_operator(a, fi, fj) for a in (0, 1)] for fi, fj in OPERATOR_ARGS])
    out["mirror_nothing_0.3"] = np.array(ref.ref_mirror_nothing(0.3))
    for (kernel, dim, hi), r in oracle_radii().items():
        w, dw = table(ref, kernel, dim, ORACLE_H[hi], r)
        key = "oracle_%d_%d_%d" % (kernel, dim, hi)
        out[key + "_r"], out[key + "_w"], out[key + "_dw"] = r, w, dw
    for kernel, _, support in KERNELS:
        r, _, rr = device_pairs(support)
        for dim in (2, 3):
            w, dw = table(ref, kernel, dim, DEVICE_H, rr)
            key = "device_%d_%d" % (kernel, dim)
            out[key + "_rr"], out[key + "_w"], out[key + "_dw"] = rr, w, dw
            out[key + "_w0"] = np.array(ref.ref_kernel_val(kernel, dim, 0.0, DEVICE_H))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "%d arrays" % len(out))


if __name__ == "__main__":
    main()
