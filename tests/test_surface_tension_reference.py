"""-m "not gpu": pins tests/surface_tension_reference.py (the numpy restatement of the reference's wall-normal and
surface-tension functors that tests/test_gpu_surface_tension.py compares the device with) to things known without it,
and checks that the binding refuses short operands before any library call."""
import math

import numpy as np
import pytest

import isph_amd  # noqa: F401
from isph_amd import hip, workload
import oracle as orc
import surface_tension_reference as stref


def _pre(parts):
    cm = workload.single_rank_colmap(parts)
    return cm, orc.Particles(parts, cm, kernel=parts["spec"].kernel, kinds=parts["kinds"]).precompute()


@pytest.mark.parametrize("dim", [2, 3])
def test_flat_wall_normals_are_axis_vectors_and_pnd_is_the_oracles(dim):
    """Lattice cavity: a particle within two layers of a wall face and farther than one cut from every edge of the cavity
    has the unit normal of that face, pointing into the fluid (+e_a at the lower wall, -e_a at the upper one, on the solid
    and on the fluid side alike), to 1e-12; every other component vanishes by the symmetry of the lattice.  The particle
    number density of the same sweep is the oracle's."""
    nfluid, wall = (16, 6) if dim == 2 else (8, 6)
    p = workload.make_cavity(nfluid, wall=wall, dim=dim)
    cm, P = _pre(p)
    n, ncell = p["nlocal"], nfluid + 2 * wall
    nrm, pnd = stref.normals(p, p["kinds"], P.vfrac, P.Gc)
    ref = P.compute_pnd()[:n]
    assert np.max(np.abs(pnd - ref)) <= 1e-12 * np.abs(ref).max()
    tag0 = p["tag"][:n].astype(np.int64) - 1
    idx = np.stack([tag0 % ncell, (tag0 // ncell) % ncell, tag0 // (ncell * ncell)], axis=1)[:, :dim]
    reach = int(math.ceil(p["cut"] / p["spec"].dx))
    checked = 0
    for a in range(dim):
        away = np.ones(n, dtype=bool)
        for b in range(dim):
            if b != a:
                away &= (idx[:, b] >= wall + reach) & (idx[:, b] < wall + nfluid - reach)
        for face, sgn in ((wall, 1.0), (wall + nfluid, -1.0)):
            sel = away & (idx[:, a] >= face - 2) & (idx[:, a] < face + 2)
            e = np.zeros(3)
            e[a] = sgn
            assert sel.sum() > 0
            assert np.max(np.abs(nrm[sel] - e)) <= 1e-12
            checked += int(sel.sum())
    assert checked > 0
    fluid_deep = np.all((idx >= wall + reach) & (idx < wall + nfluid - reach), axis=1)
    assert np.all(nrm[fluid_deep] == 0.0)                                   # no solid neighbour: no normal


@pytest.mark.parametrize("N", [18, 36])
def test_circular_drop_interface_measure_and_laplace_force(N):
    """Circular drop of radius R = 0.6 of the box half width on the exact lattice, Corrected colour, default parameters.
      sum V_i mag_i / (2 pi R)        the smeared interface integrates to one:   1.01274 (N = 18), 1.00844 (N = 36)
      -sum V_i f_i . rhat_i / (2 pi)  Laplace, sigma kappa 2 pi R = 2 pi:        0.96295 (N = 18), 0.96108 (N = 36)
    (measured with this restatement; pointwise SPH curvature at fixed h/dx does not converge, so only the bounds below
    are asserted).  The net force vanishes by the symmetry of the lattice, and both sides of the interface are pushed
    towards the drop's centre."""
    p = workload.make_droplet(N, dim=2, shape="circle")
    cm, P = _pre(p)
    n = p["nlocal"]
    prs = stref.Pairs(p, p["kinds"])
    grad, nmag, ratio = stref.csf_phase_normal(p, p["kinds"], p["phase"], P.vfrac, P.Gc, pairs=prs)
    df, kap = stref.csf_force(p, p["kinds"], p["phase"], P.vfrac, P.Gc, stref.fill_ghosts(p, nmag), pairs=prs)
    V, R = P.vfrac[:n], p["rdrop"]
    d = p["x"][:n, :2] - p["centre"]
    rhat = d / np.sqrt((d ** 2).sum(1))[:, None]
    measure = (V * nmag[:, 3]).sum() / (2 * math.pi * R)
    laplace = -(V * (df[:, :2] * rhat).sum(1)).sum() / (2 * math.pi)
    print("N = %d: interface measure %.5f, Laplace integral %.5f" % (N, measure, laplace))
    assert abs(measure - 1.0) <= 0.02
    assert 0.9 <= laplace <= 1.05
    assert np.all(np.isfinite(df))
    assert np.max(np.abs((V[:, None] * df).sum(0))) <= 1e-12 * (V * np.abs(df).sum(1)).sum()
    act = nmag[:, 3] > stref.ISPH_EPSILON
    for t in (1, 2):
        m = act & (p["type"][:n] == t)
        assert m.sum() > 0 and (df[m, :2] * rhat[m]).sum() < 0.0


def test_zero_curvature_on_an_active_particle_adds_nothing():
    parts, nmag, Gc, V = stref.two_active_particles()
    df, kap = stref.csf_force(parts, parts["kinds"], parts["phase"], V, Gc, nmag)
    assert np.all(kap == 0.0) and np.all(nmag[:, 3] > stref.ISPH_EPSILON)
    assert np.all(np.isfinite(df)) and np.all(df == 0.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_pairwise_force_functions_closed_form(dim):
    c, s = 0.7, 1.3
    q = 3.5 / 3.0                                     # (c/3) / eps with eps = c / 3.5
    for r, tm in ((0.0, -s), (c / 3, 0.0), (c, 0.0), (c * (1 + 1e-9), 0.0)):
        assert abs(stref.pairwise_f(0, dim, s, r, c) - tm) <= 1e-14 * s
    assert stref.pairwise_f(0, dim, s, c * (1 + 1e-9), c) == 0.0        # outside the support: exactly nothing
    for model, A in ((1, 4.0 if dim == 2 else 8.0), (2, 8.0 if dim == 2 else 16.0)):
        for r, e in ((0.0, 0.0), (c / 3, q), (c, 3.5), (c * (1 + 1e-9), 3.5 * (1 + 1e-9))):
            v = s * (-A * math.exp(-2.0 * e * e) + math.exp(-0.5 * e * e))      # psi(r, eps/2) = exp(-2 (r/eps)^2)
            want = v if model == 1 else r * v
            assert abs(stref.pairwise_f(model, dim, s, r, c) - want) <= 1e-13 * abs(s * A)
        assert stref.pairwise_f(model, dim, s, 0.0, c) == (s * (1.0 - A) if model == 1 else 0.0)


@pytest.mark.parametrize("dim,N", [(2, 18), (3, 6)])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_pairwise_forces_sum_to_zero_for_symmetric_s(dim, N, model):
    p = workload.make_droplet(N, dim=dim, jitter=0.1)
    s = np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 0.7], [0.0, 0.7, 1.5]])
    df, fsum = stref.pairwise_force(p, p["kinds"], p["phase"], model, s)
    assert np.abs(df).max() > 0.0
    assert np.max(np.abs(fsum)) <= 1e-12 * np.abs(df).sum()


def test_binding_refuses_operands_shorter_than_the_abi_reads():
    """every new wrapper checks the element counts the C ABI reads before the library is touched (ctx is None here)"""
    p = workload.make_droplet(6, dim=2, jitter=0.1)
    n, nall = p["nlocal"], p["nall"]
    assert nall > n
    cm = workload.single_rank_colmap(p)
    V, G = np.ones(nall), np.zeros((n, 4))
    prm = hip.CsfParams(p["phase"])
    assert issubclass(hip.OperandError, hip.IsphError) and issubclass(hip.OperandError, ValueError)
    with pytest.raises(hip.IsphError):
        hip.compute_normals(None, p, cm, V[:n], G, kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.compute_normals(None, p, cm, V, G[:-1], kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.compute_normals(None, p, cm, V, None, kinds=p["kinds"])                  # Gc is required
    with pytest.raises(hip.IsphError):
        hip.csf_phase_normal(None, p, cm, prm, V, G, rho=np.ones(n), kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.csf_phase_normal(None, p, cm, prm, V, G, wall_normal=np.zeros((n - 1, 3)), pnd=V, kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.csf_phase_normal(None, p, cm, prm, V, G, wall_normal=np.zeros((n, 3)), kinds=p["kinds"])   # no pnd
    with pytest.raises(hip.IsphError):
        hip.csf_phase_normal(None, p, cm, hip.CsfParams([1]), V, G, kinds=p["kinds"])                 # phase table too short
    with pytest.raises(hip.IsphError):
        hip.csf_force(None, p, cm, prm, V, G, np.zeros((n, 4)), np.zeros((n, 3)), kinds=p["kinds"])  # nmag without ghosts
    with pytest.raises(hip.IsphError):
        hip.csf_force(None, p, cm, prm, V, G, np.zeros((nall, 4)), np.zeros((n - 1, 3)), kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.surface_tension_csf(None, p, cm, prm, V, G, np.zeros((n, 2)), kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.pairwise_force(None, p, cm, 0, p["phase"], np.ones((3, 3)), np.zeros((n - 1, 3)), kinds=p["kinds"])
    with pytest.raises(hip.IsphError):
        hip.pairwise_force(None, p, cm, 0, p["phase"], np.ones((2, 2)), np.zeros((n, 3)), kinds=p["kinds"])   # phase 2 of 2
