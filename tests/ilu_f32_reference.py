"""Expected values of the value_bits = 32 mode of the block ILU (host only, not a test module).

The mode is defined in one sentence (include/isph_hip.h, isph_ilu_params): the fp64 triangular solves z = U^-1 D^-1 L^-1 r
with every strict-L and strict-U entry of the factor replaced by its float rounding; the diagonal (the pivots) keeps its
doubles.  So everything here is ilu_shapes._apply -- the block triangular solves in long double -- on a factor CSR whose
off-diagonal values went through np.float32 once; nothing shares code with the device.

The GPU tests hand in the DEVICE'S OWN exported factor (which the mode leaves bit for bit as the 64-bit build makes it):
rounding the long-double reference factor instead could differ by one float ulp on an entry near a rounding boundary.
"""
import numpy as np

import ilu_shapes as sh

LD = np.longdouble


def round_factor(frp, fci, fv, single=True):
    """the factor values as the solves see them, in long double: strict L and strict U through np.float32 (round to
    nearest even, subnormals kept, a value that rounds to 0 stays in the pattern), the diagonal untouched"""
    fv = np.asarray(fv, dtype=LD).copy()
    if single:
        rows = np.repeat(np.arange(len(frp) - 1), np.diff(frp))
        off = np.asarray(fci) != rows
        fv[off] = fv[off].astype(np.float32).astype(LD)
    return fv


def dense_blocks(frp, fci, fv, bp):
    """[(W, P)] per block for ilu_shapes._apply: the factor of a block as a dense long-double array and its pattern"""
    out = []
    for b in range(len(bp) - 1):
        lo, hi = int(bp[b]), int(bp[b + 1])
        m = hi - lo
        W = np.zeros((m, m), dtype=LD)
        P = np.zeros((m, m), dtype=bool)
        for r in range(m):
            s = slice(int(frp[lo + r]), int(frp[lo + r + 1]))
            W[r, np.asarray(fci[s]) - lo] = fv[s]
            P[r, np.asarray(fci[s]) - lo] = True
        out.append((W, P))
    return out


def operator(frp, fci, fv, bp, single=True):
    """r -> z (long double) for the factor CSR (frp, fci, fv) over the blocks bp; single = False: the unrounded factor,
    from the same lines"""
    dense = dense_blocks(frp, fci, round_factor(frp, fci, fv, single), bp)
    return lambda r: sh._apply(dense, bp, r)


def apply(frp, fci, fv, bp, r, single=True):
    return operator(frp, fci, fv, bp, single)(r)


def rel(z, zo):
    """||z - zo|| / ||zo|| in long double (test_gpu_ilu_shapes.rel)"""
    zo = np.asarray(zo, dtype=LD)
    return float(np.linalg.norm(np.asarray(z, dtype=LD) - zo) / np.linalg.norm(zo))
