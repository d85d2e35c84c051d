"""-m "not gpu": hip.Precond.apply_multi checks the element counts of its operands before the C ABI sees a pointer (the
ABI reads lda (nvec - 1) + n elements of R and writes as many of Z).  No device: the object below has no context and no
handle, so anything that got past the checks would fail with another error than the one asserted."""
import numpy as np
import pytest

from isph_amd import hip


def bare(n):
    M = object.__new__(hip.Precond)
    M.ctx, M.h, M.n, M.A = None, None, n, None
    return M


def test_apply_multi_refuses_missized_operands_before_any_call():
    n = 10
    M = bare(n)
    for R, kw in ((np.zeros((3, n - 1)), {}),                              # lda below n
                  (np.zeros(3 * n - 1), dict(nvec=3)),                     # flat and one element short
                  (np.zeros(2 * (n + 7) + n - 1), dict(nvec=3, lda=n + 7)),
                  (np.zeros(3 * n), {}),                                   # flat without nvec
                  (np.zeros(3 * n), dict(nvec=0)),
                  (np.zeros((3, n)), dict(nvec=4)),                        # a shape that is not [nvec, lda]
                  (np.zeros((3, n + 2)), dict(lda=n))):
        with pytest.raises(hip.OperandError):
            M.apply_multi(R, **kw)
    with pytest.raises(hip.OperandError):                                  # Z shorter than R
        M.apply_multi(np.zeros((3, n)), np.zeros((2, n)))
    with pytest.raises(hip.OperandError):
        M.apply_multi(np.zeros(2 * (n + 7) + n), np.zeros(3 * n), nvec=3, lda=n + 7)
    assert issubclass(hip.OperandError, ValueError)
    # the last column may end at its n-th row
    with pytest.raises(AttributeError):                                    # past the checks: the missing context
        M.apply_multi(np.zeros(2 * (n + 7) + n), nvec=3, lda=n + 7)


def test_the_new_entry_points_are_exported():
    assert "isph_prec_apply_multi" in hip.EXPORTS and "isph_prec_multi_path" in hip.EXPORTS
