"""numpy restatement of the reference's smoothed field, electrostatic force and random stress, written from the functors
line by line, and of the Philox4x32-10 stream the device draws the random stress from: the expected values of
tests/test_gpu_body_force.py.  tests/test_body_force_reference.py pins it to the oracle and to published known answers.

Every neighbour sum runs in the caller's list order (surface_tension_reference.Pairs).  One smoothing length and one cut
for all type pairs.  Citations are file:line of the reference sources.  Test code only.
"""
import numpy as np

from surface_tension_reference import ALL, FLUID, ISPH_EPSILON, SOLID, Pairs, fill_ghosts, kernel_dval, kernel_val  # noqa: F401

BUFFER_DIRICHLET, BUFFER_NEUMANN = 32, 64  # pair_isph.h:113-124


def smooth_field(parts, kinds, f, vfrac, kernel="wendland", filt=None, out=None, pairs=None):
    """FunctorOuterSmoothField, scalar form (functor_smooth_field.h:43-106), one pass.  Rows that fail the filter keep
    what `out` holds (:53-54 returns before anything is stored)."""
    P = pairs or Pairs(parts, kinds, kernel)
    f, V = np.asarray(f, dtype=np.float64), np.asarray(vfrac, dtype=np.float64)
    row = np.ones(P.n, dtype=bool) if filt is None else (P.kind[:P.n] & filt[0]) != 0
    m = P.incut & row[P.i]
    if filt is not None:
        m = m & ((P.kind[P.j] & filt[1]) != 0)                                       # :76
    w0 = kernel_val(P.kernel, P.dim, 0.0, P.h)                                       # :60
    sf = f[:P.n] * (w0 * V[:P.n])                                                    # :61-64
    w = kernel_val(P.kernel, P.dim, P.r, P.h)
    # bincount adds in list order starting from 0; the functor starts from the self term: add it first, as row 0 of the list
    idx = np.r_[np.arange(P.n), P.i[m]]
    sf = np.bincount(idx, weights=np.r_[sf, (f[P.j] * (w * V[P.j]))[m]], minlength=P.n)   # :89-93
    res = np.zeros(P.n) if out is None else np.array(out, dtype=np.float64)
    res[row] = sf[row]
    return res


def mirror_coeff(P, pnd, vfrac, safe):
    """MirrorMorrisHolmes::computeMirrorCoefficient(sqrt(cutsq)) per pair (mirror_morris_holmes.h:39-52)"""
    pnd, V = np.asarray(pnd), np.asarray(vfrac)
    cut = np.sqrt(P.cut * P.cut)
    di = 2.0 * cut * (pnd[P.i] * V[P.i] - 0.5) + ISPH_EPSILON
    dj = 2.0 * cut * (pnd[P.j] * V[P.j] - 0.5) + ISPH_EPSILON
    di = np.maximum(di, safe * P.h)
    return 1.0 + dj / di


def gradient(parts, kinds, f, vfrac, Gc=None, antisym=False, filt=(FLUID, ALL), pnd=None, safe=0.43301, kernel="wendland",
             pairs=None, with_coeff=False):
    """Corrected::FunctorOuterGradient (functor_gradient.h:80-169) of a scalar field with FilterBinary(filt); pnd given:
    FunctorOuterGradient_MorrisHolmes (functor_boundary_morris_holmes.h:99-102).  [nlocal, 3], exact zeros on the rows
    that fail the filter."""
    P = pairs or Pairs(parts, kinds, kernel)
    f, V = np.asarray(f, dtype=np.float64), np.asarray(vfrac, dtype=np.float64)
    ik, jk = P.kind[P.i], P.kind[P.j]
    m = P.incut & ((ik & filt[0]) != 0) & ((jk & filt[1]) != 0)                      # :100, :114, :125
    coeff = np.ones(len(P.i))
    mirrored = ((ik & SOLID) == 0) & ((jk & SOLID) != 0)                             # :128
    if pnd is not None:
        coeff = np.where(mirrored, mirror_coeff(P, pnd, V, safe), 1.0)               # :129
    dwdr = kernel_dval(P.kernel, P.dim, P.r, P.h)
    vf = np.sqrt(V[P.i] * V[P.j]) if antisym else V[P.j]                             # :137
    vjtmp = dwdr / P.r * vf * coeff                                                  # :138
    gr = P.rij if antisym else P.gt_r(Gc)                                            # :107, :140-142 (Gi = identity)
    op = (f[P.i] + f[P.j]) if antisym else (f[P.j] - f[P.i])                         # sphOperator
    g = np.zeros((P.n, 3))
    for k in range(P.dim):
        g[:, k] = P.sum(gr[:, k] * vjtmp * op, m)                                    # :144-147
    if with_coeff:
        return g, coeff, m & mirrored
    return g


def phi_gradient(parts, kinds, phi, vfrac, ae_e, Gc=None, antisym=False, kernel="wendland", pairs=None):
    """PairISPH_Corrected::computePhiGradient (pair_isph_corrected.cpp:621-651): (Fluid, Fluid), MirrorNothing, then the
    rows whose kind IS BufferDirichlet or BufferNeumann hold -ae.e in all three components"""
    P = pairs or Pairs(parts, kinds, kernel)
    g = gradient(parts, kinds, phi, vfrac, Gc, antisym, (FLUID, FLUID), None, kernel=kernel, pairs=P)
    k = P.kind[:P.n]
    g[(k == BUFFER_DIRICHLET) | (k == BUFFER_NEUMANN)] = -np.asarray(ae_e, dtype=np.float64)      # :643-650
    return g


def electrostatic_increment(dim, psi, psigrad, e, ezcb, psiref, gamma):
    """FunctorOuterElectrostaticForce (functor_electrostatic_force.h:39-56): what is added to f on every owned particle;
    e [3] (pb.e) or [nlocal, 3] (-phigrad)"""
    n = len(psigrad)
    psi = np.asarray(psi, dtype=np.float64)[:n]
    e = np.broadcast_to(np.asarray(e, dtype=np.float64), (n, 3))
    c = ezcb * 2.0 * np.sinh(psi) / (1.0 + 2.0 * gamma * np.sinh(psi / 2.0) ** 2)
    df = np.zeros((n, 3))
    for k in range(dim):
        df[:, k] = -(c * (-psiref * psigrad[:, k] + e[:, k]))
    return df


def electrostatic_force(parts, kinds, psi, vfrac, prm, phi=None, Gc=None, antisym=False, pnd=None, safe=0.43301,
                        kernel="wendland", pairs=None):
    """computePsiGradient + computePhiGradient + computeElectrostaticForce; prm: dict(ezcb, psiref, gamma, pb_e, ae_e).
    Returns (psigrad, phigrad or None, increment of f)."""
    P = pairs or Pairs(parts, kinds, kernel)
    gpsi = gradient(parts, kinds, psi, vfrac, Gc, antisym, (FLUID, ALL), pnd, safe, kernel, P)
    gphi = None if phi is None else phi_gradient(parts, kinds, phi, vfrac, prm["ae_e"], Gc, antisym, kernel, P)
    e = np.asarray(prm["pb_e"], dtype=np.float64) if phi is None else -gphi
    return gpsi, gphi, electrostatic_increment(P.dim, psi, gpsi, e, prm["ezcb"], prm["psiref"], prm["gamma"])


# ---- the random stream: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) ------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two; returns four uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]                       # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def uniform53(hi, lo):
    """(((hi 2^32 + lo) >> 11) + 0.5) 2^-53, in (0, 1]"""
    w = (hi << np.uint64(32)) | lo
    return ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(tag, seed, step, dim):
    """the dim^2 standard normals of every tag: [len(tag), dim^2] (Box-Muller on the draw blocks b = 0 .. ceil(dim^2 / 2))"""
    tag = np.asarray(tag, dtype=np.int64).astype(np.uint64) & _MASK
    seed, step = int(seed), int(step)
    nblock = (dim * dim + 1) // 2
    g = np.zeros((len(tag), 2 * nblock))
    for b in range(nblock):
        o = philox4x32_10((tag, b, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        u1, u2 = uniform53(o[0], o[1]), uniform53(o[2], o[3])
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
        g[:, 2 * b], g[:, 2 * b + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return g[:, :dim * dim]


PACK = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))


def random_stress_tensor(parts, kinds, tag, seed, step):
    """computeRandomStressTensor (pair_isph.cpp:710-758) on the owned rows with kind & Fluid, packed [nlocal, 6]"""
    dim, n = int(parts["dim"]), int(parts["nlocal"])
    kind = np.asarray([0] + list(kinds), dtype=np.int64)[np.asarray(parts["type"])[:n]]
    g = normals(np.asarray(tag)[:n], seed, step, dim)
    R = g.reshape(n, dim, dim)                                                       # :736-738, R[k2][k1]
    T = 0.5 * (R + R.transpose(0, 2, 1))                                             # :742
    tr = np.zeros(n)
    for k in range(dim):
        tr = tr + T[:, k, k]                                                         # :744-745
    for k in range(dim):
        T[:, k, k] -= tr / dim                                                       # :747-748
    rs = np.zeros((n, 6))
    for s, (a, b) in enumerate(PACK):
        if b < dim:
            rs[:, s] = T[:, a, b]
    rs[(kind & FLUID) == 0] = 0.0                                                    # :733
    return rs


def unpack_column(rs, c):
    """column c of the packed tensors as a vector field [., 3]: rstress_{x,y,z}[i][k] = T[k][c] (:751-757)"""
    rs = np.asarray(rs)
    col = np.zeros((len(rs), 3))
    for k in range(3):
        a, b = min(k, c), max(k, c)
        col[:, k] = rs[:, PACK.index((a, b))]
    return col


def random_stress_force(parts, kinds, dt, kBT, nu, rho, rs_all, vfrac, kernel="wendland", pairs=None):
    """FunctorOuterRandomStress<FunctorOuterDivergenceAntiSymmetric> (functor_random_stress.h:54-74; the divergence is
    functor_divergence.h:54-124 with alpha = -1): the increment of f [nlocal, 3]; rs_all [nall, 6], ghosts filled"""
    P = pairs or Pairs(parts, kinds, kernel)
    V = np.asarray(vfrac, dtype=np.float64)
    m = P.incut & ((P.kind[P.i] & FLUID) != 0) & ((P.kind[P.j] & FLUID) != 0)
    dwdr = kernel_dval(P.kernel, P.dim, P.r, P.h)
    vjtmp = dwdr / P.r * np.sqrt(V[P.i] * V[P.j])
    i = P.i[m]
    df = np.zeros((P.n, 3))
    fl = (P.kind[:P.n] & FLUID) != 0
    sq = np.zeros(P.n)
    sq[fl] = np.sqrt(2.0 * kBT * np.asarray(nu)[:P.n][fl] * np.asarray(rho)[:P.n][fl] / dt / V[:P.n][fl])      # :65
    for c in range(P.dim):
        col = unpack_column(rs_all, c)
        # the divergence adds the dim terms of one pair to the running sum one by one (functor_divergence.h:114)
        terms = np.stack([P.rij[m, k] * (col[P.i[m], k] + col[P.j[m], k]) * vjtmp[m] for k in range(P.dim)], axis=1)
        d = np.bincount(np.repeat(i, P.dim), weights=terms.ravel(), minlength=P.n) * -1.0
        df[:, c] = np.where(fl, d * sq, 0.0)                                         # :61, :66-71
    return df
