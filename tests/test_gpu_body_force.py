"""-m gpu: the smoothed field, the fused electrokinetic sweep (psi gradient with the MorrisHolmes mirror, phi gradient with
the buffer-row override, electrostatic force) and the random stress on the device against the numpy restatement of the
reference functors (tests/body_force_reference.py, pinned to the C oracle by tests/test_body_force_reference.py).  Gate:
the project's own for streaming operators, max|dev - ref| <= 1e-12 max|ref| per output array."""
import functools

import numpy as np
import pytest

from isph_amd import dist, hip, workload
import oracle as orc
import pb_channel
import body_force_reference as bf
from problems import Problem, tgv_spec

pytestmark = pytest.mark.gpu

GATE = 1e-12
KINDS = [orc.FLUID, orc.BUFFER_DIRICHLET, orc.BUFFER_NEUMANN, orc.SOLID]   # types 1..4
SLAB = 1.2
CASES = [dict(dim=2, n=20, mode=workload.JITTER), dict(dim=3, n=12, mode=workload.JITTER),
         dict(dim=2, n=16, mode=workload.LATTICE, kernel="quintic", cut_over_h=3.0)]
IDS = ["2d-jitter-wendland", "3d-jitter-wendland", "2d-lattice-quintic"]
PRM = dict(ezcb=0.7, psiref=1.3, gamma=0.0, pb_e=(0.4, -0.3, 0.2), ae_e=(0.3, -0.2, 0.1))


def zone_types(parts):
    """x-slabs of buffer particles at both ends, a solid block in the middle, fluid elsewhere; images follow their owners
    (the zones of tests/test_scalar_callers.py)"""
    own = parts["owner_index"]
    x = parts["x"][:parts["nlocal"]] % (2 * np.pi)
    t = np.ones(parts["nlocal"], dtype=np.int32)
    t[x[:, 0] < SLAB] = 2
    t[x[:, 0] > 2 * np.pi - SLAB] = 3
    t[(np.abs(x[:, 0] - np.pi) < 0.5) & (np.abs(x[:, 1] - np.pi) < 0.9)] = 4
    return t[own]


def gate(dev, ref, what=""):
    dev, ref = np.asarray(dev), np.asarray(ref)
    err, scale = np.max(np.abs(dev - ref)), np.abs(ref).max()
    print("%s: max|dev - ref| = %.3e, max|ref| = %.3e" % (what, err, scale))
    assert scale > 0 and err <= GATE * scale, what


def host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


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
    """one of the three clouds with the oracle's computePre and pnd, the restatement's pair arrays and two smooth fields"""

    def __init__(self, k):
        pr = Problem(tgv_spec(**CASES[k]), antisym=False, kinds=KINDS, types=zone_types)
        self.p, self.cm, self.n, self.nall, self.dim = pr.parts, pr.colmap, pr.n, pr.parts["nall"], pr.parts["dim"]
        self.kernel = pr.spec.kernel
        self.V, self.G = pr.P.vfrac, np.ascontiguousarray(pr.P.Gc[:self.n])
        self.pnd = pr.P.compute_pnd()
        self.pairs = bf.Pairs(self.p, KINDS, self.kernel)
        x, own = self.p["x"], self.p["owner_index"]
        self.own = own
        self.psi = np.ascontiguousarray((0.8 * np.cos(x[:, 0]) * np.sin(x[:, 1]) + 0.3 * np.sin(2 * x[:, 2] + 0.5))[:self.n][own])
        self.phi = np.ascontiguousarray((np.cos(x[:, 0]) + 0.2 * x[:, 1] - 0.4 * np.sin(x[:, 2]))[:self.n][own])
        self.kind = np.asarray(KINDS)[self.p["type"][:self.n] - 1]
        self.fluid_bit = (self.kind & orc.FLUID) != 0
        self.buffer = (self.kind == orc.BUFFER_DIRICHLET) | (self.kind == orc.BUFFER_NEUMANN)
        self.tag = np.ascontiguousarray(self.p["tag"][:self.n])
        rng = np.random.default_rng(3)
        self.nu, self.rho = 0.1 * (1.0 + 0.5 * rng.random(self.n)), 1.0 + 0.5 * rng.random(self.n)
        self.dt, self.kBT = 1e-3, 0.5

    def ghosts(self, owned):
        return bf.fill_ghosts(self.p, owned)

    def operands(self, on_device):
        return (parts_side(on_device, self.p),) + tuple(side(on_device, self.cm, self.V, self.G))

    def ek_reference(self, antisym, morris, with_phi=True, gamma=0.0):
        prm = dict(PRM, gamma=gamma)
        return bf.electrostatic_force(self.p, KINDS, self.psi, self.V, prm, self.phi if with_phi else None,
                                      None if antisym else self.G, antisym, self.pnd if morris else None, kernel=self.kernel,
                                      pairs=self.pairs)


@functools.lru_cache(maxsize=None)
def case(k):
    return Case(k)


# ------------------------------------------------------------------------------------------------ 1. smoothed field
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_smooth_field_matches_restatement(gpu_ctx, k, on_device):
    c = case(k)
    parts, cm, V, _ = c.operands(on_device)
    ref = bf.smooth_field(c.p, KINDS, c.phi, c.V, c.kernel, pairs=c.pairs)
    sf = hip.smooth_field(gpu_ctx, parts, cm, side(on_device, c.phi), V, kernel=c.kernel, kinds=KINDS)
    gate(host(sf), ref, "smoothed field")
    # a row filter: the rows of other kinds are not written
    solid = c.kind == orc.SOLID
    ref_s = bf.smooth_field(c.p, KINDS, c.phi, c.V, c.kernel, filt=(bf.SOLID, bf.ALL), out=np.full(c.n, -7.0), pairs=c.pairs)
    out = side(on_device, np.full(c.n, -7.0))
    got = hip.smooth_field(gpu_ctx, parts, cm, side(on_device, c.phi), V, filt=(bf.SOLID, bf.ALL), out=out, kernel=c.kernel,
                           kinds=KINDS)
    assert got is out
    out = host(out)
    assert solid.sum() > 0 and np.all(out[~solid] == -7.0)
    gate(out[solid], ref_s[solid], "smoothed field on the Solid rows")
    # a neighbour filter changes the sum
    ref_f = bf.smooth_field(c.p, KINDS, c.phi, c.V, c.kernel, filt=(bf.ALL, bf.FLUID), pairs=c.pairs)
    assert np.abs(ref_f - ref).max() > 1e-3 * np.abs(ref).max()
    got = hip.smooth_field(gpu_ctx, parts, cm, side(on_device, c.phi), V, filt=(bf.ALL, bf.FLUID), kernel=c.kernel, kinds=KINDS)
    gate(host(got), ref_f, "smoothed field over Fluid neighbours")


# ------------------------------------------------------------------------------------------------ 2. both gradients
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("morris", [0, 1])
@pytest.mark.parametrize("antisym", [0, 1])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_both_gradients_match_restatement(gpu_ctx, k, antisym, morris, on_device):
    c = case(k)
    gpsi_ref, gphi_ref, _ = c.ek_reference(antisym, morris)
    if morris:      # conditions on the input: a kernel that ignores the mirror cannot pass
        _, coeff, which = bf.gradient(c.p, KINDS, c.psi, c.V, None if antisym else c.G, antisym, pnd=c.pnd, kernel=c.kernel,
                                      pairs=c.pairs, with_coeff=True)
        plain, _, _ = c.ek_reference(antisym, 0)
        npairs, diff = int((which & (coeff != 1.0)).sum()), np.abs(gpsi_ref - plain).max() / np.abs(plain).max()
        print("mirrored pairs %d, |mirrored - plain| / max = %.3g" % (npairs, diff))
        assert npairs > 0 and diff > 1e-3
    parts, cm, V, G = c.operands(on_device)
    psi, phi, pnd = side(on_device, c.psi, c.phi, c.pnd if morris else None)
    gpsi, gphi = hip.electrostatic_force(gpu_ctx, parts, cm, hip.EkParams(**PRM), psi, V, phi=phi, antisym=bool(antisym),
                                         Gc=None if antisym else G, pnd=pnd, kernel=c.kernel, kinds=KINDS)
    gpsi, gphi = host(gpsi), host(gphi)
    gate(gpsi, gpsi_ref, "psi gradient")
    gate(gphi, gphi_ref, "phi gradient")
    solid = c.kind == orc.SOLID
    assert solid.sum() > 0 and np.all(gpsi[solid] == 0.0) and np.all(gphi[solid] == 0.0)
    assert c.buffer.sum() > 0 and np.array_equal(gphi[c.buffer], np.tile(-np.asarray(PRM["ae_e"]), (c.buffer.sum(), 1)))
    if c.dim == 2:
        assert np.all(gpsi[:, 2] == 0.0) and np.all(gphi[~c.buffer, 2] == 0.0)


# ------------------------------------------------------------------------------------------------ 3. force
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("gamma", [0.0, 0.1])
@pytest.mark.parametrize("with_phi", [True, False])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_force_matches_restatement_and_accumulates(gpu_ctx, k, with_phi, gamma, on_device):
    c = case(k)
    gpsi_ref, gphi_ref, df_ref = c.ek_reference(0, 1, with_phi, gamma)
    prm = dict(PRM, gamma=gamma)
    f0 = np.random.default_rng(8).standard_normal((c.n, 3))
    parts, cm, V, G = c.operands(on_device)
    psi, phi, pnd = side(on_device, c.psi, c.phi if with_phi else None, c.pnd)
    kw = dict(phi=phi, Gc=G, pnd=pnd, kernel=c.kernel, kinds=KINDS)
    f = side(on_device, f0.copy())
    gpsi, gphi = hip.electrostatic_force(gpu_ctx, parts, cm, hip.EkParams(**prm), psi, V, f=f, **kw)
    f, gpsi, gphi = host(f), host(gpsi), host(gphi)
    assert (gphi is None) == (not with_phi)
    felt = np.abs(df_ref[:, :c.dim]).sum(1) > 0                             # no filter: with pb_e every owned row feels it,
    assert np.all(felt if not with_phi else felt[c.fluid_bit])              # Solid ones included (with phi their field is 0)
    gate(f, f0 + df_ref, "force")
    gate(f - f0, df_ref, "force increment")
    if c.dim == 2:
        assert np.array_equal(f[:, 2], f0[:, 2])
    # gradients only: the same gradients bit for bit
    g2psi, g2phi = hip.electrostatic_force(gpu_ctx, parts, cm, hip.EkParams(**prm), psi, V, **kw)
    assert np.array_equal(host(g2psi), gpsi) and (not with_phi or np.array_equal(host(g2phi), gphi))
    # force only: the same force bit for bit
    f2 = side(on_device, f0.copy())
    assert hip.electrostatic_force(gpu_ctx, parts, cm, hip.EkParams(**prm), psi, V, f=f2, with_gradients=False, **kw) is None
    assert np.array_equal(host(f2), f)
    # the force follows from the returned gradients
    e = np.asarray(prm["pb_e"]) if not with_phi else -gphi
    gate(f - f0, bf.electrostatic_increment(c.dim, c.psi, gpsi, e, prm["ezcb"], prm["psiref"], gamma), "force from the gradients")


# ------------------------------------------------------------------------------------------------ 4. closed form
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_constant_psi_has_no_gradient_and_feels_the_applied_field(gpu_ctx, k, on_device):
    """psi = const, Symmetric family: psi_j - psi_i = 0 in every pair term, so psigrad is exactly zero, and every owned
    row, Solid ones included, receives -2 ezcb g(psi) pb_e, g = sinh psi / (1 + 2 gamma sinh^2(psi / 2))"""
    c = case(k)
    psi0, gamma = 0.6, 0.1
    prm = dict(PRM, gamma=gamma)
    parts, cm, V, G = c.operands(on_device)
    f0 = np.random.default_rng(9).standard_normal((c.n, 3))
    f = side(on_device, f0.copy())
    gpsi, _ = hip.electrostatic_force(gpu_ctx, parts, cm, hip.EkParams(**prm), side(on_device, np.full(c.nall, psi0)), V, f=f,
                                      Gc=G, pnd=side(on_device, c.pnd), kernel=c.kernel, kinds=KINDS)
    assert np.all(host(gpsi) == 0.0)
    g = np.sinh(psi0) / (1.0 + 2.0 * gamma * np.sinh(psi0 / 2.0) ** 2)
    want = np.zeros((c.n, 3))
    want[:, :c.dim] = -2.0 * prm["ezcb"] * g * np.asarray(prm["pb_e"])[:c.dim]
    gate(host(f) - f0, want, "force of a constant potential")


# ------------------------------------------------------------------------------------------------ 5. tensors
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_tensors_match_restatement_and_follow_the_tag(gpu_ctx, k, on_device):
    c = case(k)
    seed, step = (7 << 32) + 12345, (3 << 32) + 11
    ref = bf.random_stress_tensor(c.p, KINDS, c.tag, seed, step)
    parts, cm, _, _ = c.operands(on_device)
    rs = host(hip.random_stress_tensor(gpu_ctx, parts, cm, side(on_device, c.tag), seed, step, kernel=c.kernel, kinds=KINDS))
    gate(rs, ref, "random stress tensor")
    assert (~c.fluid_bit).sum() > 0 and np.all(rs[~c.fluid_bit] == 0.0)
    if c.dim == 2:
        assert np.all(rs[:, 3:] == 0.0)
    # the same particles in a shuffled atom order: the same tensor per tag, bit for bit
    order = np.random.default_rng(12).permutation(c.n)
    q = workload.renumber(c.p, order)
    assert np.array_equal(q["tag"][:c.n], c.tag[order]) and not np.array_equal(q["tag"][:c.n], c.tag)
    rq = host(hip.random_stress_tensor(gpu_ctx, parts_side(on_device, q), side(on_device, workload.single_rank_colmap(q)),
                                       side(on_device, np.ascontiguousarray(q["tag"][:c.n])), seed, step, kernel=c.kernel,
                                       kinds=KINDS))
    assert np.array_equal(rq, rs[order])
    # another step, another seed (in the low or the high word): every fluid row changes
    for s2, t2 in ((seed, step + 1), (seed + 1, step), (seed + (1 << 32), step), (seed, step + (1 << 32))):
        other = host(hip.random_stress_tensor(gpu_ctx, parts, cm, side(on_device, c.tag), s2, t2, kernel=c.kernel, kinds=KINDS))
        assert np.all(np.any(other[c.fluid_bit] != rs[c.fluid_bit], axis=1))
        gate(other, bf.random_stress_tensor(c.p, KINDS, c.tag, s2, t2), "random stress tensor, other draw")


# ------------------------------------------------------------------------------------------------ 6. stress force
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_stress_force_matches_restatement_and_accumulates(gpu_ctx, k, on_device):
    c = case(k)
    rs_all = c.ghosts(bf.random_stress_tensor(c.p, KINDS, c.tag, 99, 3))
    df_ref = bf.random_stress_force(c.p, KINDS, c.dt, c.kBT, c.nu, c.rho, rs_all, c.V, c.kernel, pairs=c.pairs)
    assert np.all(np.abs(df_ref[c.fluid_bit]).sum(1) > 0)
    f0 = np.random.default_rng(6).standard_normal((c.n, 3))
    parts, cm, V, _ = c.operands(on_device)
    nu, rho, rs = side(on_device, c.nu, c.rho, rs_all)
    f = side(on_device, f0.copy())
    hip.random_stress_force(gpu_ctx, parts, cm, c.dt, c.kBT, nu, rho, rs, f, V, kernel=c.kernel, kinds=KINDS)
    f = host(f)
    gate(f - f0, df_ref, "random-stress force increment")
    gate(f, f0 + df_ref, "random-stress force")
    assert np.array_equal(f[~c.fluid_bit], f0[~c.fluid_bit])                # rows without a Fluid bit are untouched
    if c.dim == 2:
        assert np.array_equal(f[:, 2], f0[:, 2])


# ------------------------------------------------------------------------------------------------ 7. one call, two ranks
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_one_call_equals_the_staged_calls_bit_for_bit(gpu_ctx, k, on_device):
    c = case(k)
    seed, step = 2024, 5
    parts, cm, V, _ = c.operands(on_device)
    tag, nu, rho = side(on_device, c.tag, c.nu, c.rho)
    kw = dict(kernel=c.kernel, kinds=KINDS)
    f0 = np.random.default_rng(6).standard_normal((c.n, 3))
    rs = hip.random_stress_tensor(gpu_ctx, parts, cm, tag, seed, step, **kw)
    f_staged = side(on_device, f0.copy())
    hip.random_stress_force(gpu_ctx, parts, cm, c.dt, c.kBT, nu, rho, side(on_device, c.ghosts(host(rs))), f_staged, V, **kw)
    f_one = side(on_device, f0.copy())
    rs_one = hip.force_from_random_stress(gpu_ctx, parts, cm, tag, seed, step, c.dt, c.kBT, nu, rho, f_one, V, with_rs=True, **kw)
    assert np.array_equal(host(rs_one), host(rs))
    assert np.array_equal(host(f_one), host(f_staged))
    assert np.abs(host(f_one) - f0).max() > 0
    f_two = side(on_device, f0.copy())
    assert hip.force_from_random_stress(gpu_ctx, parts, cm, tag, seed, step, c.dt, c.kBT, nu, rho, f_two, V, **kw) is None
    assert np.array_equal(host(f_two), host(f_one))


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
    """The 2-D cloud as pgrid (2, 1, 1): tensors per half, each half's off-rank ghost records taken from the other half's
    tensors in numpy (what isph_halo_forward(ncomp = 6) delivers), the sweep per half: per tag the single-rank tensors
    bit for bit and the single-rank forces within the gate."""
    c = case(0)
    seed, step = 31, 8
    hk = dict(kernel=c.kernel, kinds=KINDS)
    rs1 = hip.random_stress_tensor(gpu_ctx, c.p, c.cm, c.tag, seed, step, **hk)
    f1 = np.zeros((c.n, 3))
    hip.random_stress_force(gpu_ctx, c.p, c.cm, c.dt, c.kBT, c.nu, c.rho, c.ghosts(rs1), f1, c.V, **hk)
    by_tag = np.empty(c.n, dtype=np.int64)
    by_tag[c.tag - 1] = np.arange(c.n)                                        # tag -> single-rank particle
    halves = []
    for r in range(2):
        spec = tgv_spec(**dict(CASES[0], pgrid=(2, 1, 1), rank=r))
        p = dist.prune_ghosts(workload.make_tgv(spec))
        plan = dist.make_plan(p, _SoloTD(r, 2))
        src = by_tag[p["tag"] - 1]
        assert np.max(np.abs(np.mod(p["x"][:, :2] - c.p["x"][src, :2] + np.pi, 2 * np.pi) - np.pi)) < 1e-12
        p["type"] = np.ascontiguousarray(c.p["type"][src])
        n = p["nlocal"]
        rs = hip.random_stress_tensor(gpu_ctx, p, plan.colmap, np.ascontiguousarray(p["tag"][:n]), seed, step, **hk)
        assert np.array_equal(rs, rs1[src[:n]])
        halves.append(dict(p=p, plan=plan, V=np.ascontiguousarray(c.V[src]), rs=rs, src=src))
    assert sum(h["p"]["nlocal"] for h in halves) == c.n
    remote = 0
    for r, h in enumerate(halves):
        p, plan, other = h["p"], h["plan"], halves[1 - r]
        n = p["nlocal"]
        assert list(plan.peers) == [1 - r] and plan.ncol > n
        ghosts = other["rs"][plan.recv_idx]
        rs_all = np.ascontiguousarray(np.concatenate([h["rs"], ghosts])[plan.colmap])
        remote += int((plan.colmap >= n).sum())
        own = h["src"][:n]
        f = np.zeros((n, 3))
        hip.random_stress_force(gpu_ctx, p, plan.colmap, c.dt, c.kBT, c.nu[own], c.rho[own], rs_all, f, h["V"], **hk)
        assert np.max(np.abs(f - f1[own])) <= GATE * np.abs(f1).max()
    assert remote > 0 and np.abs(f1).max() > 0


# ------------------------------------------------------------------------------------------------ 8. hand-over
def test_device_force_feeds_the_helmholtz_right_hand_side(gpu_ctx_both):
    """chain on the small channel of channel-edl-potential-2d.lmp: psi from isph_solve_poisson_boltzmann stays on the
    device, isph_electrostatic_force turns it into the body force there (on_device = 1, no host copy), and
    isph_assemble_helmholtz reads that force: its right-hand side equals the one assembled with the restatement's force
    from the same psi."""
    import torch
    ctx = gpu_ctx_both
    parts, own = pb_channel.channel(32)
    kinds = pb_channel.KINDS
    n, nall = parts["nlocal"], parts["nall"]
    colmap = own.astype(np.int32)
    vfrac = np.ascontiguousarray(hip.compute_volumes(ctx, parts, colmap)[own])
    pnd = np.ascontiguousarray(hip.compute_pnd(ctx, parts, colmap, kinds=kinds)[own])
    Gc, Lc = hip.compute_corrections(ctx, parts, colmap, vfrac)
    psi0 = (parts["type"] == 2).astype(float)
    J = hip.assemble_poisson_boltzmann(ctx, parts, colmap, psi0=psi0, antisym=False, vfrac=vfrac, Gc=Gc, Lc=Lc, kinds=kinds,
                                       pnd=pnd, morris_safe_coeff=0.0)
    psi_d = torch.from_numpy(psi0[:n].copy()).cuda()
    info = hip.solve_poisson_boltzmann(ctx, J, psi_d, None, params=hip.PBParams(kappasq=pb_channel.KAPPA ** 2))
    assert info.status == 1
    own_d = torch.from_numpy(own.astype(np.int64)).cuda()
    dparts = parts_side(1, parts)
    dcm, dV, dG, dL, dpnd = side(1, colmap, vfrac, Gc, Lc, pnd)
    prm = dict(ezcb=50.0, psiref=1.0, gamma=0.0, pb_e=(0.02, 0.01, 0.0), ae_e=(0.0, 0.0, 0.0))
    f_d = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    hip.electrostatic_force(ctx, dparts, dcm, hip.EkParams(**prm), psi_d[own_d].contiguous(), dV, f=f_d, Gc=dG, pnd=dpnd,
                            morris_safe_coeff=0.0, kinds=kinds, with_gradients=False)
    rng = np.random.default_rng(4)
    nu, rho, pres = np.full(nall, 0.1), np.full(nall, 1.0), np.ascontiguousarray(rng.random(n)[own])
    vel = np.ascontiguousarray((0.01 * rng.standard_normal((n, 3)))[own])
    vel[:, 2] = 0.0
    dt, theta, g = 1e-3, 0.5, np.zeros(3)
    hk = dict(antisym=False, kinds=kinds, rhs_only=True)
    dnu, drho, dpres, dvel = side(1, nu, rho, pres, vel)
    _, b_dev = hip.assemble_helmholtz(ctx, dparts, dcm, dt, theta, dnu, drho, dpres, f_d[own_d].contiguous(), g, dvel, vfrac=dV,
                                      Gc=dG, Lc=dL, pnd=dpnd, morris_safe_coeff=0.0, **hk)
    psi = psi_d.cpu().numpy()
    _, _, df = bf.electrostatic_force(parts, kinds, psi[own], vfrac, prm, None, Gc, False, pnd, safe=0.0)
    assert np.abs(df).max() > 0
    _, b_ref = hip.assemble_helmholtz(ctx, parts, colmap, dt, theta, nu, rho, pres, np.ascontiguousarray(df[own]), g, vel,
                                      vfrac=vfrac, Gc=Gc, Lc=Lc, pnd=pnd, morris_safe_coeff=0.0, **hk)
    _, b_zero = hip.assemble_helmholtz(ctx, parts, colmap, dt, theta, nu, rho, pres, np.zeros((nall, 3)), g, vel,
                                       vfrac=vfrac, Gc=Gc, Lc=Lc, pnd=pnd, morris_safe_coeff=0.0, **hk)
    assert np.abs(b_ref - b_zero).max() > 1e-6 * np.abs(b_ref).max()         # the force is visible in the right-hand side
    gate(b_dev.cpu().numpy(), b_ref, "Helmholtz right-hand side")
    J.close()
