"""numpy restatement of the three reductions of a time step, straight from the reference's loops:
PairISPH::computeZeroMeanPressure (pair_isph.cpp:422-464), ComputeISPH_Status::compute_vector
(compute_isph_status.cpp:141-175) and FixISPH_TGV::compute_error (fix_isph_tgv.cpp:76-116).  The terms are formed as
the loops form them (one rounding per product and per sum); the sums themselves are math.fsum, i.e. exact, so that a
device result can be held against the any-order summation bound."""
import math

import numpy as np

FLUID, SOLID, BUFFER_DIRICHLET, BUFFER_NEUMANN = 99, 12, 32, 64
EPS = float(np.finfo(np.float64).eps)


def kind_of(type_, kinds):
    """kinds[t - 1] = kind of the 1-based type t"""
    return np.asarray(kinds, dtype=np.int64)[np.asarray(type_, dtype=np.int64) - 1]


def zero_mean_pressure(f, nlocal, type_, kinds, update=True):
    """returns (f_new, mean, count, abs_sum): owned Solid rows -> 0 and left out; mean over the other owned rows; with
    update the mean leaves every row of [0, nall) that is not Solid.  count 0: mean 0, nothing subtracted (the declared
    departure; the reference divides by zero)."""
    f = np.array(f, dtype=np.float64)
    kd = kind_of(type_, kinds)
    own_solid = np.zeros(len(f), dtype=bool)
    own_solid[:nlocal] = kd[:nlocal] == SOLID
    f[own_solid] = 0.0
    enter = np.zeros(len(f), dtype=bool)
    enter[:nlocal] = kd[:nlocal] != SOLID
    terms = f[enter]
    count = int(enter.sum())
    mean = math.fsum(terms) / count if count else 0.0
    if update and count:
        f[kd != SOLID] -= mean
    return f, mean, count, math.fsum(np.abs(terms))


def status(x, type_, vfrac, v, rho, nlocal, type_mask=-1, centre=(0.0, 0.0, 0.0), radius=0.0):
    """returns (stat[8], abs_sums[7]): count, sum vx, vy, vz, V, rho V, 1/2 rho V |v|^2, max |v| within radius of centre"""
    x, v = np.asarray(x, dtype=np.float64)[:nlocal], np.asarray(v, dtype=np.float64)[:nlocal]
    vfrac, rho = np.asarray(vfrac, dtype=np.float64)[:nlocal], np.asarray(rho, dtype=np.float64)[:nlocal]
    t = np.asarray(type_, dtype=np.int64)[:nlocal]
    sel = ((int(type_mask) & 0xFFFFFFFF) >> (t - 1)) & 1 == 1
    vx, vy, vz = v[sel, 0], v[sel, 1], v[sel, 2]
    vmagsq = (vx * vx + vy * vy) + vz * vz
    mass = rho[sel] * vfrac[sel]
    ke = (0.5 * mass) * vmagsq
    cols = [np.ones(int(sel.sum())), vx, vy, vz, vfrac[sel], mass, ke]
    stat = [math.fsum(c) for c in cols]
    vmax = 0.0
    if radius > 0:
        xx = x[sel] - np.asarray(centre, dtype=np.float64)
        r = np.sqrt((xx[:, 0] * xx[:, 0] + xx[:, 1] * xx[:, 1]) + xx[:, 2] * xx[:, 2])
        inside = r <= radius
        if inside.any():
            vmax = float(np.sqrt(vmagsq[inside]).max())
    return np.array(stat + [vmax]), np.array([math.fsum(np.abs(c)) for c in cols])


def tgv_exact(x, t, umax, nu, rho):
    """the exact fields of fix_isph_tgv.cpp:87-91 with per-particle nu and rho"""
    x = np.asarray(x, dtype=np.float64)
    p = 0.25 * rho * (np.cos(2 * x[:, 0]) + np.cos(2 * x[:, 1])) * umax * umax * np.exp(-4.0 * nu * t)
    u = np.zeros((len(x), 3))
    u[:, 0] = umax * np.exp(-2.0 * nu * t) * np.sin(x[:, 0]) * np.cos(x[:, 1])
    u[:, 1] = -umax * np.exp(-2.0 * nu * t) * np.cos(x[:, 0]) * np.sin(x[:, 1])
    return u, p


def tgv_error(x, vnp1, p, rho, nu, t, umax, nlocal):
    """(p_err, p_norm, u_err, u_norm): the mean of p over the owned rows is removed, sums over nlocal, square root"""
    x, vnp1 = np.asarray(x, dtype=np.float64)[:nlocal], np.asarray(vnp1, dtype=np.float64)[:nlocal]
    p, rho, nu = (np.asarray(a, dtype=np.float64)[:nlocal] for a in (p, rho, nu))
    uex, pex = tgv_exact(x, t, umax, nu, rho)
    pavg = math.fsum(p) / nlocal
    errorp = math.fsum((p - pex - pavg) ** 2)
    normp = math.fsum(pex ** 2)
    erroru = math.fsum(np.sum((vnp1 - uex) ** 2, axis=1))
    normu = math.fsum(np.sum(uex ** 2, axis=1))
    return tuple(math.sqrt(s / nlocal) for s in (errorp, normp, erroru, normu))
