"""-m gpu: wall normals, the two sweeps of the continuum surface force and the pairwise force on the device against the
numpy restatement of the reference functors (tests/surface_tension_reference.py).  Gate: the project's own for
streaming operators, max|dev - ref| <= 1e-12 max|ref| per output array, on seeded jittered inputs."""
import functools
import math

import numpy as np
import pytest

from isph_amd import dist, hip, workload
import oracle as orc
import surface_tension_reference as stref
import tgv_driver as T

pytestmark = pytest.mark.gpu

GATE = 1e-12
COLOR = {"corrected": stref.CORRECTED, "adami": stref.ADAMI}


def gate(dev, ref, what=""):
    dev, ref = np.asarray(dev), np.asarray(ref)
    err, scale = np.max(np.abs(dev - ref)), np.abs(ref).max()
    print("%s: max|dev - ref| = %.3e, max|ref| = %.3e" % (what, err, scale))
    assert scale > 0 and err <= GATE * scale, what


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def side(on_device, *arrays):
    """the operands as numpy arrays (on_device = 0) or as tensors on the GPU (on_device = 1)"""
    if not on_device:
        return arrays if len(arrays) > 1 else arrays[0]
    import torch
    out = tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)
    return out if len(out) > 1 else out[0]


def parts_side(on_device, parts):
    if not on_device:
        return parts
    d = dict(parts)
    for k in ("x", "type", "neigh_ptr", "neigh_idx"):
        d[k] = side(1, parts[k])
    return d


class Case:
    """a workload with the oracle's computePre (volumes, G_i) and the restatement's pair arrays"""

    def __init__(self, parts, kernel):
        self.p, self.kernel = parts, kernel
        self.n, self.nall, self.dim = parts["nlocal"], parts["nall"], parts["dim"]
        self.cm = workload.single_rank_colmap(parts)
        P = orc.Particles(parts, self.cm, kernel=kernel, kinds=parts["kinds"]).precompute()
        self.V, self.G = P.vfrac, np.ascontiguousarray(P.Gc[:self.n])
        self.kinds = parts["kinds"]
        self.pairs = stref.Pairs(parts, self.kinds, kernel)
        rng = np.random.default_rng(5)
        self.rho = np.ascontiguousarray((1.0 + 0.5 * rng.random(self.n))[parts["owner_index"]])

    def ghosts(self, owned):
        return stref.fill_ghosts(self.p, owned)

    def operands(self, on_device):
        return (parts_side(on_device, self.p),) + tuple(side(on_device, self.cm, self.V, self.G))


@functools.lru_cache(maxsize=None)
def droplet(dim, kernel, walls=False, shape="circle"):
    N = 36 if dim == 2 else 12
    return Case(workload.make_droplet(N, dim=dim, shape=shape, wall_layers=4 if walls else 0, jitter=0.1, seed=11,
                                      brick=(6, 6, 6)), kernel)


@functools.lru_cache(maxsize=None)
def cavity(dim, kernel):
    nfluid, wall = (24, 6) if dim == 2 else (10, 6)
    return Case(workload.make_cavity(nfluid, wall=wall, dim=dim, jitter=0.05, seed=7), kernel)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("kernel", ["wendland", "quintic"])
@pytest.mark.parametrize("case", ["drop-on-solid-2d", "cavity-2d", "cavity-3d"])
def test_normals_and_pnd_match_restatement(gpu_ctx, case, kernel, on_device):
    c = droplet(2, kernel, walls=True) if case == "drop-on-solid-2d" else cavity(int(case[-2]), kernel)
    nrm_ref, pnd_ref = stref.normals(c.p, c.kinds, c.V, c.G, kernel, pairs=c.pairs)
    assert (np.abs(nrm_ref).sum(1) > 0).sum() > 0 and (np.abs(nrm_ref).sum(1) == 0).sum() > 0
    parts, cm, V, G = c.operands(on_device)
    nrm, pnd = hip.compute_normals(gpu_ctx, parts, cm, V, G, kernel=kernel, kinds=c.kinds)
    gate(host(nrm), nrm_ref, "normal")
    gate(host(pnd), pnd_ref, "pnd")
    assert np.array_equal(np.abs(host(nrm)).sum(1) == 0, np.abs(nrm_ref).sum(1) == 0)     # no particle gains or loses a wall
    gate(host(pnd), host(hip.compute_pnd(gpu_ctx, parts, cm, kernel=kernel, kinds=c.kinds)), "pnd against isph_compute_pnd")
    only = hip.compute_normals(gpu_ctx, parts, cm, V, G, kernel=kernel, kinds=c.kinds, with_pnd=False)
    assert np.array_equal(host(only), host(nrm))


def sweep1_reference(c, color, theta=0.0, walls=False):
    """the restatement's sweep 1 with the conditions on the input that make the comparison meaningful"""
    wall = pnd = None
    if walls:
        wall, pnd = stref.normals(c.p, c.kinds, c.V, c.G, c.kernel, pairs=c.pairs)
        pnd = c.ghosts(pnd)
    eps = 0.01
    grad, nmag, ratio = stref.csf_phase_normal(c.p, c.kinds, c.p["phase"], c.V, c.G, c.kernel, COLOR[color], c.rho, eps, theta,
                                               wall, pnd, pairs=c.pairs)
    margin = np.minimum(np.abs(ratio - eps), np.abs(ratio - (1.0 - eps))).min()
    print("in-phase volume ratio: closest to a threshold %.3e" % margin)
    assert margin >= 1e-6                                  # no particle sits on the threshold of the `if`
    return grad, nmag, wall, pnd


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("color", ["corrected", "adami"])
@pytest.mark.parametrize("kernel", ["wendland", "quintic"])
@pytest.mark.parametrize("dim,walls", [(2, False), (3, False), (2, True)])
def test_csf_phase_normal_matches_restatement(gpu_ctx, dim, walls, kernel, color, on_device):
    """sweep 1.  The raw gradient and its length to the gate; the unit normal to 1e-12 max(mag) / mag_i (its error is
    the gradient's divided by mag_i), every particle included."""
    c = droplet(dim, kernel, walls=walls)
    theta = 1.0472 if walls else 0.0
    grad_ref, nmag_ref, wall, pnd = sweep1_reference(c, color, theta, walls)
    prm = hip.CsfParams(c.p["phase"], color=color, theta=theta)
    parts, cm, V, G = c.operands(on_device)
    rho, wl, pn = side(on_device, c.rho, wall, pnd)
    grad, nmag = hip.csf_phase_normal(gpu_ctx, parts, cm, prm, V, G, rho=rho, wall_normal=wl, pnd=pn, kernel=kernel,
                                      kinds=c.kinds)
    grad, nmag = host(grad), host(nmag)
    gate(grad, grad_ref, "phase gradient")
    gate(nmag[:, 3], nmag_ref[:, 3], "mag")
    mag = nmag_ref[:, 3]
    act = mag > 0
    assert act.sum() > 0 and np.array_equal(nmag[:, 3] > 0, act)
    assert np.all(nmag[~act, :3] == 0.0)
    err = np.abs(nmag[act, :3] - nmag_ref[act, :3]).max(axis=1)
    print("unit normal: worst error x mag_i / max mag = %.3e, smallest mag_i / max mag = %.3e"
          % ((err * mag[act]).max() / mag.max(), mag[act].min() / mag.max()))
    assert np.all(err <= GATE * mag.max() / mag[act])
    if walls:                                              # the contact-angle correction really acted
        plain = stref.csf_phase_normal(c.p, c.kinds, c.p["phase"], c.V, c.G, kernel, COLOR[color], c.rho, pairs=c.pairs)[1]
        assert np.abs(plain[:, :3] - nmag_ref[:, :3]).max() > 1e-3


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("kernel", ["wendland", "quintic"])
@pytest.mark.parametrize("dim,walls", [(2, False), (3, False), (2, True)])
def test_csf_force_matches_restatement(gpu_ctx, dim, walls, kernel, on_device):
    """sweep 2, fed the RESTATEMENT's records (ghosts included) so that ill-conditioned normals do not leak into the
    comparison: curvature and force to the gate, no particle left out."""
    c = droplet(dim, kernel, walls=walls)
    _, nmag_ref, _, _ = sweep1_reference(c, "corrected", 1.0472 if walls else 0.0, walls)
    nm_all = c.ghosts(nmag_ref)
    alpha, kappa = 0.8, 3.0                                # kappa small enough for the exponential to matter
    df_ref, kap_ref = stref.csf_force(c.p, c.kinds, c.p["phase"], c.V, c.G, nm_all, kernel, alpha, kappa, pairs=c.pairs)
    act = nmag_ref[:, 3] > stref.ISPH_EPSILON
    assert act.sum() > 0 and not np.any(kap_ref[act] == 0.0)
    prm = hip.CsfParams(c.p["phase"], alpha=alpha, kappa=kappa)
    parts, cm, V, G = c.operands(on_device)
    f = side(on_device, np.zeros((c.n, 3)))
    kap = hip.csf_force(gpu_ctx, parts, cm, prm, V, G, side(on_device, nm_all), f, kernel=kernel, kinds=c.kinds)
    gate(host(kap), kap_ref, "curvature")
    gate(host(f), df_ref, "surface force")


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("dim,walls", [(2, False), (3, False), (2, True)])
def test_one_call_equals_the_staged_calls_bit_for_bit_and_accumulates(gpu_ctx, dim, walls, on_device):
    c = droplet(dim, "wendland", walls=walls)
    theta = 1.0472 if walls else 0.0
    _, _, wall, pnd = sweep1_reference(c, "corrected", theta, walls)
    prm = hip.CsfParams(c.p["phase"], theta=theta)
    parts, cm, V, G = c.operands(on_device)
    rho, wl, pn = side(on_device, c.rho, wall, pnd)
    kw = dict(kernel="wendland", kinds=c.kinds)
    f0 = np.random.default_rng(2).standard_normal((c.n, 3))
    _, nmag = hip.csf_phase_normal(gpu_ctx, parts, cm, prm, V, G, rho=rho, wall_normal=wl, pnd=pn, **kw)
    nm_all = side(on_device, c.ghosts(host(nmag)))
    f_staged, f_zero = side(on_device, f0.copy()), side(on_device, np.zeros((c.n, 3)))
    hip.csf_force(gpu_ctx, parts, cm, prm, V, G, nm_all, f_staged, **kw)
    hip.csf_force(gpu_ctx, parts, cm, prm, V, G, nm_all, f_zero, **kw)
    f_one = side(on_device, f0.copy())
    nm_one = hip.surface_tension_csf(gpu_ctx, parts, cm, prm, V, G, f_one, rho=rho, wall_normal=wl, pnd=pn, with_nmag=True, **kw)
    assert np.array_equal(host(nm_one), host(nmag))
    assert np.array_equal(host(f_one), host(f_staged))
    df = host(f_zero)
    assert np.abs(df).max() > 0
    assert np.max(np.abs((host(f_one) - f0) - df)) <= GATE * np.abs(df).max()          # incremented, not overwritten
    untouched = np.abs(df).sum(1) == 0
    assert untouched.sum() > 0 and np.array_equal(host(f_one)[untouched], f0[untouched])


class _SoloTD:
    """dist.make_plan without a transport: the ghost numbering of a rank depends on its own particles only (the send
    lists, which do depend on the peers, are not used here)"""

    def __init__(self, rank, n):
        self.rank, self.n = rank, n

    def get_world_size(self):
        return self.n

    def all_gather_object(self, out, obj):
        for r in range(self.n):
            out[r] = obj if r == self.rank else {}


def test_two_ranks_with_ghosts_filled_from_the_other_half(gpu_ctx):
    """The periodic droplet box as pgrid (2, 1, 1): sweep 1 per half, each half's off-rank ghost records taken from the
    other half's sweep-1 output in numpy (owner_rank / owner_index through the plan's ghost columns), sweep 2 per half:
    the owned results are the single-rank run's."""
    N, kw = 36, dict(dim=2, shape="square", jitter=0.1, seed=11, brick=(6, 6, 6))
    one = Case(workload.make_droplet(N, **kw), "wendland")
    prm = hip.CsfParams(one.p["phase"])
    hk = dict(kernel="wendland", kinds=one.kinds)
    _, nm1 = hip.csf_phase_normal(gpu_ctx, one.p, one.cm, prm, one.V, one.G, **hk)
    f1 = np.zeros((one.n, 3))
    kap1 = hip.csf_force(gpu_ctx, one.p, one.cm, prm, one.V, one.G, one.ghosts(nm1), f1, **hk)
    by_tag = np.empty(one.n, dtype=np.int64)
    by_tag[one.p["tag"][:one.n] - 1] = np.arange(one.n)                       # lattice site -> single-rank particle
    halves = []
    for r in range(2):
        p = dist.prune_ghosts(workload.make_droplet(N, pgrid=(2, 1, 1), rank=r, **kw))
        plan = dist.make_plan(p, _SoloTD(r, 2))
        src = by_tag[p["tag"] - 1]
        assert np.max(np.abs(np.mod(p["x"][:, :2] - one.p["x"][src, :2] + np.pi, 2 * np.pi) - np.pi)) < 1e-12
        V, G = np.ascontiguousarray(one.V[src]), np.ascontiguousarray(one.G[src[:p["nlocal"]]])
        _, nm = hip.csf_phase_normal(gpu_ctx, p, plan.colmap, prm, V, G, **hk)
        halves.append(dict(p=p, plan=plan, V=V, G=G, nm=nm, src=src))
    assert sum(h["p"]["nlocal"] for h in halves) == one.n
    remote = 0
    for r, h in enumerate(halves):
        p, plan, other = h["p"], h["plan"], halves[1 - r]
        n = p["nlocal"]
        assert list(plan.peers) == [1 - r] and plan.ncol > n
        ghosts = other["nm"][plan.recv_idx]                                  # what isph_halo_forward(ncomp = 4) delivers
        nm_all = np.ascontiguousarray(np.concatenate([h["nm"], ghosts])[plan.colmap])
        remote += int((plan.colmap >= n).sum())
        f = np.zeros((n, 3))
        kap = hip.csf_force(gpu_ctx, p, plan.colmap, prm, h["V"], h["G"], nm_all, f, **hk)
        own = h["src"][:n]
        assert np.max(np.abs(kap - kap1[own])) <= GATE * np.abs(kap1).max()
        assert np.max(np.abs(f - f1[own])) <= GATE * np.abs(f1).max()
        assert np.max(np.abs(h["nm"][:, 3] - nm1[own, 3])) <= GATE * np.abs(nm1[:, 3]).max()
    assert remote > 0 and np.abs(f1).max() > 0


@pytest.mark.parametrize("on_device", [0, 1])
def test_zero_curvature_on_an_active_particle_leaves_the_force_alone(gpu_ctx, on_device):
    """the declared departure from the reference: kappa_i == 0 adds nothing (the reference would write NaN)"""
    parts, nmag, G, V = stref.two_active_particles()
    cm = np.arange(2, dtype=np.int32)
    f0 = np.array([[0.25, -1.5, 0.0], [3.0, 0.125, 0.0]])
    f = side(on_device, f0.copy())
    dparts, dcm, dV, dG = (parts_side(on_device, parts),) + tuple(side(on_device, cm, V, G))
    kap = hip.csf_force(gpu_ctx, dparts, dcm, hip.CsfParams(parts["phase"]), dV, dG, side(on_device, nmag), f,
                        kinds=parts["kinds"])
    assert np.all(host(kap) == 0.0)
    assert np.all(np.isfinite(host(f))) and np.array_equal(host(f), f0)


@functools.lru_cache(maxsize=None)
def three_phase_droplet(dim):
    """the square droplet with the outer fluid split at the box centre into two types / phases (x below / above)"""
    c = droplet(dim, "wendland", shape="square")
    p = dict(c.p)
    typ = p["type"].copy()
    typ[(typ == 2) & (p["site"][:, 0] >= p["N"])] = 3
    p.update(type=typ, kinds=[stref.FLUID] * 3, phase=[1, 2, 3])
    return p, c.cm, stref.Pairs(p, p["kinds"])


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("dim", [2, 3])
def test_pairwise_force_matches_restatement(gpu_ctx, dim, model, on_device):
    """Per-particle forces and f_sum to the gate, asymmetric s.  f_sum is a sum of all pair terms, and on a closed
    interface with a radial pair force they cancel: with two phases sum|F_ij| / |f_sum| is 1e4 to 6e4 here, so the
    half-ulp differences between two math libraries' cos / exp, one per pair term and of one sign, alone reach
    1.1e-16 * 6e4 = 7e-12 |f_sum|, above the gate whatever the kernel does.  The input therefore breaks the symmetry: the
    outer fluid is two phases split at the box centre and only one of them is attracted by the drop (s[2][1] = 3), which
    gives a net pull along x; the condition sum|F_ij| <= 1e3 |f_sum| is asserted on the restatement."""
    p, cm, pairs = three_phase_droplet(dim)
    s = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 0.3, 0.0, 0.0], [0.0, 3.0, 0.1, 0.0], [0.0, 0.0, 0.0, 0.2]])
    df_ref, sum_ref = stref.pairwise_force(p, p["kinds"], p["phase"], model, s, pairs=pairs)
    ph = np.asarray([0] + p["phase"])[pairs.type]
    terms = np.abs(stref.pairwise_f(model, dim, s[ph[pairs.i], ph[pairs.j]], pairs.r, pairs.cut)[pairs.incut]).sum()
    print("sum|F_ij| / max|f_sum| = %.3g" % (terms / np.abs(sum_ref).max()))
    assert terms <= 1e3 * np.abs(sum_ref).max()
    assert np.all(np.abs(df_ref).sum(1) > 0)                                  # every particle feels a force
    parts = parts_side(on_device, p)
    f0 = np.random.default_rng(4).standard_normal((p["nlocal"], 3))
    if dim == 2:
        f0[:, 2] = 0.0
    f = side(on_device, f0.copy())
    fsum = hip.pairwise_force(gpu_ctx, parts, side(on_device, cm), model, p["phase"], s, f, kinds=p["kinds"])
    gate(host(f), f0 + df_ref, "pairwise force")
    gate(host(f) - f0, df_ref, "pairwise increment")
    gate(fsum, sum_ref, "f_sum")


def test_device_normals_feed_the_block_helmholtz(gpu_ctx_both):
    """chain: isph_compute_normals -> isph_assemble_block_helmholtz on the cavity, against the oracle's block Helmholtz
    with the same normals (the gate of test_gpu_block_helmholtz.py)."""
    ctx = gpu_ctx_both
    c = cavity(2, "wendland")
    p, dim = c.p, 2
    P = orc.Particles(p, c.cm, kinds=c.kinds).precompute()
    nrm, _ = hip.compute_normals(ctx, p, c.cm, P.vfrac, c.G, kinds=c.kinds)
    normal = c.ghosts(nrm)
    assert (np.abs(normal).sum(1) > 0).sum() > 0
    x, nall = p["x"], p["nall"]
    pres = np.cos(x[:, 0]) * np.sin(x[:, 1])
    force = np.ascontiguousarray(0.01 * np.stack([np.sin(x[:, 1]), np.cos(x[:, 0]), np.zeros(nall)], axis=1))
    nu = p["nu"] * (1.0 + 0.1 * np.sin(x[:, 0]))
    g = np.array([0.05, -0.02, 0.0])
    vel = np.ascontiguousarray(p["v"])
    theta, beta, dt = 0.5, 0.3, p["dt"]
    rp, ci, vals, b = P.block_helmholtz(dt, theta, beta, nu, p["rho"], pres, force, g, vel, normal=normal, antisym=False)
    blocks, bg = hip.assemble_block_helmholtz(ctx, p, c.cm, dt, theta, beta, nu, p["rho"], pres, force, g, vel, normal=normal,
                                              antisym=False, vfrac=P.vfrac, Gc=P.Gc, Lc=P.Lc, kinds=c.kinds)
    scale, off = np.abs(vals).max(), 0.0
    for ib in range(dim):
        for jb in range(dim):
            rg, cg, vg = blocks[ib][jb].export_csr()
            assert np.array_equal(rg, rp) and np.array_equal(cg, ci)
            assert np.max(np.abs(vg - vals[ib * dim + jb])) <= 1e-12 * scale
            if ib != jb:
                off += np.abs(vals[ib * dim + jb]).sum()
    assert off > 0
    assert np.max(np.abs(bg - b.ravel())) <= 1e-12 * np.abs(b).max()


def droplet_chain(ctx, nsteps, device_force, N=16, block=256):
    """whole time steps of the jittered square droplet (computePre, surface tension, Helmholtz with that force, Poisson,
    corrections, advance) on the device; the CSF force from the device or from the restatement"""
    # seed 2: the smallest active |grad c| of the start configuration is 1e-2 of the largest (seeds 1..12 range from 8e-10
    # to 1e-2), so every unit normal carries thirteen digits and more into the curvature of its neighbours
    p0 = workload.make_droplet(N, dim=2, shape="square", jitter=0.1, seed=2)
    n, L = p0["nlocal"], 2 * np.pi
    kinds, phase = p0["kinds"], p0["phase"]
    h, cut, dt, nu0, rho0, theta = p0["h"], p0["cut"], p0["dt"], 0.1, 1.0, 0.5
    x, typ = p0["x"][:n].copy(), p0["type"][:n].copy()
    v, p = np.zeros((n, 3)), np.zeros(n)
    prm = hip.CsfParams(phase)
    fmax = 0.0
    for step in range(nsteps):
        parts, own = T.periodic_particles(x, L, cut)
        parts["h"], parts["cut"] = h, cut
        parts["type"] = np.ascontiguousarray(typ[own])
        nall = parts["nall"]
        colmap = own.astype(np.int32)
        ghost = lambda a: np.ascontiguousarray(a[own])
        rho, nuall = np.full(nall, rho0), np.full(nall, nu0)
        vfrac = ghost(hip.compute_volumes(ctx, parts, colmap))
        G, Lm = hip.compute_corrections(ctx, parts, colmap, vfrac)
        f = np.zeros((n, 3))
        if device_force:
            hip.surface_tension_csf(ctx, parts, colmap, prm, vfrac, G, f, kinds=kinds)
        else:
            _, nmag, ratio = stref.csf_phase_normal(parts, kinds, phase, vfrac, G)
            assert np.minimum(np.abs(ratio - 0.01), np.abs(ratio - 0.99)).min() >= 1e-6
            act = nmag[:, 3] > stref.ISPH_EPSILON
            print("step %d: smallest active mag / max mag = %.3e" % (step, nmag[act, 3].min() / nmag[:, 3].max()))
            if step == 0:      # a condition on the INPUT (later states are results: their figure is printed, not asserted)
                assert nmag[act, 3].min() >= 1e-6 * nmag[:, 3].max()          # the normals carry ten digits into the force
            f, _ = stref.csf_force(parts, kinds, phase, vfrac, G, ghost(nmag))
        fmax = max(fmax, np.abs(f).max())
        A_h, bh = hip.assemble_helmholtz(ctx, parts, colmap, dt, theta, nuall, rho, ghost(p), ghost(f), np.zeros(3), ghost(v),
                                         antisym=False, vfrac=vfrac, Gc=G, Lc=Lm)
        Mh = hip.Precond(ctx, A_h, "bjacobi-ilu0", block)
        xh = np.ascontiguousarray(np.concatenate([v[:, 0], v[:, 1]]))
        ih = hip.solve(ctx, A_h, np.ascontiguousarray(bh[:2 * n].copy()), xh, prec=Mh, singular=False, nvec=2, lda=n)
        assert ih.converged == 1
        vstar = np.zeros((n, 3))
        vstar[:, 0], vstar[:, 1] = xh[:n], xh[n:]
        A, b = hip.assemble_poisson(ctx, parts, colmap, dt, rho, ghost(vstar), antisym=False, vfrac=vfrac, Gc=G, Lc=Lm)
        M = hip.Precond(ctx, A, "bjacobi-ilu0", block)
        dp = np.zeros(n)
        info = hip.solve(ctx, A, b.copy(), dp, prec=M, singular=True)
        assert info.converged == 1
        dp -= dp.mean()
        vs_all, p_all = ghost(vstar), ghost(p)
        hip.correct_velocity_pressure(ctx, parts, colmap, dt, rho, ghost(dp), vs_all, p_all, vfrac, antisym=False, Gc=G)
        vstar, p = vs_all[:n].copy(), p_all[:n].copy()
        dpa = hip.advance_begin(ctx, parts, colmap, dt, ghost(p), ghost(v), ghost(vstar), vfrac, antisym=False, Gc=G)
        xa, va, pa = np.ascontiguousarray(x.copy()), np.ascontiguousarray(v.copy()), p.copy()
        hip.advance_end(ctx, n, 2, dt, dpa, np.ascontiguousarray(vstar), pa, xa, va)
        x, v, p = xa, va, pa
        x[:, :2] %= L
        for M_ in (Mh, M, A_h, A):
            M_.close()
    return dict(x=x, v=v, p=p, fmax=fmax)


def test_three_droplet_steps_with_the_device_force_match_the_restatement_force(gpu_ctx_both):
    """chain: three time steps of the jittered square droplet with the CSF force from the device against the same chain
    with the force from the restatement (positions <= 1e-8 L, velocities and pressure <= 1e-6 max: the gates of
    test_three_tgv_steps_on_device_match_oracle_driver); both solves converge in every step."""
    L = 2 * np.pi
    dev = droplet_chain(gpu_ctx_both, 3, True)
    ref = droplet_chain(gpu_ctx_both, 3, False)
    assert ref["fmax"] > 0 and np.abs(ref["v"]).max() > 0                     # the drop really moved the fluid
    dx = np.abs(np.mod(dev["x"] - ref["x"] + 0.5 * L, L) - 0.5 * L)
    print("droplet chain: max dx %.3e, dv %.3e of %.3e, dp %.3e of %.3e"
          % (dx.max(), np.abs(dev["v"] - ref["v"]).max(), np.abs(ref["v"]).max(), np.abs(dev["p"] - ref["p"]).max(),
             np.abs(ref["p"]).max()))
    assert dx[:, :2].max() <= 1e-8 * L
    assert np.max(np.abs(dev["v"] - ref["v"])) <= 1e-6 * np.abs(ref["v"]).max()
    assert np.max(np.abs(dev["p"] - ref["p"])) <= 1e-6 * np.abs(ref["p"]).max()
