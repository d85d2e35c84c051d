"""-m "not gpu": the GMRES-polynomial entry points are declared in include/isph_hip.h, exported and bound in hip.py, and the
type strings "gmres-poly<d>" are parsed for d = 1 .. 25 and refused otherwise (no "-f32" form).  No device: isph_prec_type_kind is the
library's own parse_prec_type behind a host-only entry point, and the objects below have no context and no handle."""
import os
import re

import numpy as np
import pytest

import isph_amd  # noqa: F401
from isph_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("isph_poly_params_default", "isph_prec_create_gmres_poly", "isph_prec_poly_info", "isph_prec_type_kind")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "isph_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS and hasattr(hip.lib(), name)
    assert re.search(r"typedef struct \{\s*int degree;\s*\} isph_poly_params;", header)
    for name in ("PolyParams", "PrecondGmresPoly", "prec_type_kind"):
        assert hasattr(hip, name)
    assert issubclass(hip.PrecondGmresPoly, hip.Precond)
    assert callable(hip.Precond.roots) and callable(hip.Precond.hessenberg)
    p = hip.PolyParams()
    assert p.degree == 4 and [f for f, _ in hip.PolyParams._fields_] == ["degree"]
    assert hip.PolyParams(degree=7).degree == 7


def test_type_strings():
    for d in range(1, 26):
        assert hip.prec_type_kind("gmres-poly%d" % d) == 7
    for bad in ("gmres-poly0", "gmres-poly26", "gmres-poly4-f32", "gmres-poly", "gmres-poly04", "gmres-poly-4", "gmres-poly4 ",
                "gmres-poly100", "gmrespoly4"):
        assert hip.prec_type_kind(bad) == -1, bad
    # the kinds that were there keep their numbers
    assert [hip.prec_type_kind(k) for k in ("none", "jacobi", "bjacobi-ilu0", "sa-amg", "ilu1", "chebyshev3", "chebyshev16-f32")] == \
        [0, 1, 2, 3, 4, 6, 6]
    assert hip.prec_type_kind("chebyshev17") == -1


def test_nullvec_is_checked_before_the_call():
    class FakeA:
        h = None

        def info(self):
            return dict(nrow=10)

    with pytest.raises(hip.OperandError):
        hip.PrecondGmresPoly(None, FakeA(), 4, nullvec=np.ones(9))
