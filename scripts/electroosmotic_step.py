"""An electro-osmotic step (applied field + Poisson-Boltzmann + Navier-Stokes, the switches of
sph-script/flow-charged-pore.xml) and a fluctuating Taylor-Green step on the device, device-resident arrays, Symmetric
operator family.

Channel: the periodic box of the TGV generator with Solid walls along y, a BufferDirichlet slab at the low-x end and a
BufferNeumann slab at the high-x end.  The chain of PairISPH::compute (pair_isph.cpp:1305-1339):
  1 conductivity smoothing (isph_smooth_field, two passes, ghosts refreshed in between)
  2 applied potential: isph_assemble_applied_potential + isph_solve (Solid taken as Fluid: ae.is_solid2fluid)
  3 Poisson-Boltzmann: isph_assemble_poisson_boltzmann + isph_solve_poisson_boltzmann (psi = 1 on the walls)
  4 body force: isph_electrostatic_force (psi gradient with the MorrisHolmes mirror, phi gradient, force: one sweep)
  5 Helmholtz with that force   6 Poisson   7 corrections
The Navier-Stokes and Poisson-Boltzmann builders know Fluid and Solid only; the buffer kinds carry the Fluid bits and
are handed to them as Fluid, which is what their bit-test filters see in the reference.

Then one fluctuating TGV step (isph_force_from_random_stress -> Helmholtz -> Poisson -> corrections), and the two new
sweeps beside the launches they replace on the same particles: HIP events around each call on the context's stream,
neighbour layout held, 3 warm-up calls, median and spread of --repeats calls.  Linear solves: FGMRES(50); block ILU(0) for
the Helmholtz system, --prec for the applied potential and the pressure Poisson equation.  --neighbours device: ghosts and
neighbour list of the fluctuating step are rebuilt from the particle positions on the device (workload.make_cloud_device)
instead of coming from the host generator.

    python scripts/electroosmotic_step.py --dim 2 --N 1024
    python scripts/electroosmotic_step.py --dim 3 --N 96"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import isph_amd  # noqa: F401
from isph_amd import hip, workload

ap = argparse.ArgumentParser()
ap.add_argument("--dim", type=int, default=2)
ap.add_argument("--N", type=int, default=1024, help="cells per box edge")
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--prec", default="sa-amg", choices=["sa-amg", "bjacobi-ilu0"], help="of the two scalar elliptic solves")
ap.add_argument("--max-iters", type=int, default=4000, help="of every linear solve (GMRES(50) + block ILU(0))")
ap.add_argument("--neighbours", default="host", choices=["host", "device"],
                help="where ghosts and neighbour list of the fluctuating step are built")
args = ap.parse_args()

FLUID, SOLID, BUF_D, BUF_N, ALL = 99, 12, 32, 64, 127
KINDS = [FLUID, BUF_D, BUF_N, SOLID]                 # types 1..4
KINDS_AE = [FLUID, BUF_D, BUF_N, FLUID]              # ae.is_solid2fluid
KINDS_NS = [FLUID, FLUID, FLUID, SOLID]              # buffers are Fluid to the builders that know two kinds
dim, N = args.dim, args.N
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = hip.Context(0, stream=stream.cuda_stream)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
L = 2.0 * np.pi


def elliptic_prec(A, nullvec=None):
    if args.prec == "sa-amg":
        return hip.PrecondAMG(ctx, A, nullvec=nullvec, params=hip.AmgParams(block=512))
    return hip.Precond(ctx, A, "bjacobi-ilu0", 512)


solver = lambda tol=1e-8: hip.SolverParams(tol=tol, max_iters=args.max_iters, max_restarts=args.max_iters // 50 + 1)


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def upload(parts):
    if hip._is_torch(parts["x"]):                   # built on the device: nothing to upload
        return parts, parts["owner_index"], parts["owner_index"].to(torch.int64)
    d = dict(parts)
    for k in ("x", "type", "neigh_ptr", "neigh_idx"):
        d[k] = T(parts[k])
    return d, T(parts["owner_index"].astype(np.int32)), T(parts["owner_index"].astype(np.int64))


def spec(mode):
    if dim == 3:
        return workload.TGVSpec(dim=3, ncell=(N, N, N), mode=mode)
    return workload.TGVSpec(dim=2, ncell=(N, N), brick=(8, 8), origin=(0.5, 0.5), mode=mode)


def momentum_step(dp, colmap, own, kinds, vfrac, G, Lc, f, v, p, rho, nu, dt, mask=None, normal=None):
    """Helmholtz with the body force f, Poisson, corrections; returns (vstar, p, text).  mask: 1 on the rows that span the
    null space of the pressure operator (the rows that are not Solid), None = all"""
    n = int(dp["nlocal"])
    ghost = lambda a: a[own].contiguous()
    kw = dict(kinds=kinds)
    t0 = sync()
    H, bh = hip.assemble_helmholtz(ctx, dp, colmap, dt, 0.5, nu, rho, ghost(p), ghost(f), np.zeros(3), ghost(v), antisym=False,
                                   vfrac=vfrac, Gc=G, Lc=Lc, **kw)
    MH = hip.Precond(ctx, H, "bjacobi-ilu0", 512)
    xh = torch.cat([v[:, k] for k in range(dim)]).contiguous()
    ih = hip.solve(ctx, H, bh[:dim * n].contiguous(), xh, prec=MH, singular=False, nvec=dim, lda=n, params=solver())
    MH.close(); H.close()
    vstar = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    for k in range(dim):
        vstar[:, k] = xh[k * n:(k + 1) * n]
    t1 = sync()
    A, b = hip.assemble_poisson(ctx, dp, colmap, dt, rho, ghost(vstar), antisym=False, vfrac=vfrac, Gc=G, Lc=Lc,
                                normal=None if normal is None else ghost(normal), **kw)
    M = elliptic_prec(A, None if mask is None else mask / np.sqrt(float(mask.sum())))
    dpv = torch.zeros(n, dtype=torch.float64, device=dev)
    ip = hip.solve(ctx, A, b, dpv, prec=M, singular=True, null_mask=mask, params=solver())
    M.close(); A.close()
    m = torch.ones(n, dtype=torch.float64, device=dev) if mask is None else T(mask.astype(np.float64))
    dpv -= m * ((dpv * m).sum() / m.sum())
    t2 = sync()
    vs_all, p_all = ghost(vstar), ghost(p)
    hip.correct_velocity_pressure(ctx, dp, colmap, dt, rho, ghost(dpv), vs_all, p_all, vfrac, antisym=False, Gc=G)
    t3 = sync()
    text = ("helmholtz %.2f [%d its, conv %d]  poisson %.2f [%d its, conv %d]  corrections %.2f"
            % ((t1 - t0) * 1e3, ih.iters, ih.converged, (t2 - t1) * 1e3, ip.iters, ip.converged, (t3 - t2) * 1e3))
    return vs_all[:n], p_all[:n], text


def timed(name, fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.sort(ts)
    print("  %-58s %8.1f [%8.1f .. %8.1f]" % (name, np.median(ts), ts[0], ts[-1]))
    return float(np.median(ts))


# ---- the electro-osmotic step ---------------------------------------------------------------------------------------
sp = spec(workload.LATTICE)
parts = workload.make_tgv(sp)
n, nall, dx = parts["nlocal"], parts["nall"], sp.dx
own_h = parts["owner_index"]
xo = parts["x"][:n] % L
wall, slab = 4.0 * dx, 0.15 * L
typ = np.ones(n, dtype=np.int32)
typ[xo[:, 0] < slab] = 2
typ[xo[:, 0] > L - slab] = 3
typ[(xo[:, 1] < wall) | (xo[:, 1] > L - wall)] = 4
parts["type"] = np.ascontiguousarray(typ[own_h])
dp, colmap, own = upload(parts)
ghost = lambda a: a[own].contiguous()
kind = np.asarray(KINDS)[typ - 1]
solid_all = T((kind == SOLID)[own_h])
buffer_all = T(((kind == BUF_D) | (kind == BUF_N))[own_h])
dt, e0 = sp.dt, 0.05                                 # applied field -dphi/dx = e0 between the two buffers
ezcb = 1.0
psiref = 2.0 * ezcb * (8.0 * dx) ** 2                # Debye length 8 dx: kappa^2 = 2 ezcb / psiref
ek = hip.EkParams(ezcb=ezcb, psiref=psiref, gamma=0.0, pb_e=(e0, 0.0, 0.0), ae_e=(e0, 0.0, 0.0))
rho = torch.full((nall,), 1.0, dtype=torch.float64, device=dev)
nu = torch.full((nall,), 0.1, dtype=torch.float64, device=dev)
print("electro-osmotic channel %d-D, %d particles (%d Solid, %d buffer), h = %.4g, cut = %.4g, dt = %.4g, kappa dx = 0.125"
      % (dim, n, int((kind == SOLID).sum()), int(((kind == BUF_D) | (kind == BUF_N)).sum()), parts["h"], parts["cut"], dt))
ctx.hold_neighbours(True)
t0 = sync()
vfrac = ghost(hip.compute_volumes(ctx, dp, colmap))
G, Lc = hip.compute_corrections(ctx, dp, colmap, vfrac)
nrm, pn = hip.compute_normals(ctx, dp, colmap, vfrac, G, kinds=KINDS_NS)      # wall normals for the Neumann rows of the Poisson equation
pnd = ghost(pn)
t1 = sync()
sigma = torch.ones(nall, dtype=torch.float64, device=dev)                     # 1 conductivity smoothing, ae.smooth_phi = 2
sigma[solid_all] = 0.01
for _ in range(2):
    sigma = ghost(hip.smooth_field(ctx, dp, colmap, sigma, vfrac, kinds=KINDS))
t2 = sync()
x_all = T(parts["x"][:, 0] % L)                                              # 2 applied potential, phi = -e0 x in the buffers
phi0 = torch.where(buffer_all, -e0 * x_all, torch.zeros_like(x_all))
A, b = hip.assemble_applied_potential(ctx, dp, colmap, sigma, phi0, antisym=False, vfrac=vfrac, Gc=G, Lc=Lc, kinds=KINDS_AE)
M = elliptic_prec(A)
phi = phi0[:n].clone()
ia = hip.solve(ctx, A, b, phi, prec=M, params=solver(1e-10))
M.close(); A.close()
t3 = sync()
psi0 = solid_all.to(torch.float64)                                           # 3 Poisson-Boltzmann, psi = 1 on the walls
J = hip.assemble_poisson_boltzmann(ctx, dp, colmap, psi0=psi0, antisym=False, vfrac=vfrac, Gc=G, Lc=Lc, kinds=KINDS_NS, pnd=pnd)
psi = psi0[:n].clone()
ib = hip.solve_poisson_boltzmann(ctx, J, psi, None, params=hip.PBParams(kappasq=2.0 * ezcb / psiref))
J.close()
t4 = sync()
f = torch.zeros((n, 3), dtype=torch.float64, device=dev)                     # 4 the body force
hip.electrostatic_force(ctx, dp, colmap, ek, ghost(psi), vfrac, phi=ghost(phi), f=f, Gc=G, pnd=pnd, kinds=KINDS,
                        with_gradients=False)
t5 = sync()
v = torch.zeros((n, 3), dtype=torch.float64, device=dev)
p = torch.zeros(n, dtype=torch.float64, device=dev)
vstar, p, text = momentum_step(dp, colmap, own, KINDS_NS, vfrac, G, Lc, f, v, p, rho, nu, dt,
                                mask=(kind != SOLID).astype(np.int32), normal=nrm)                  # 5, 6, 7
t6 = sync()
fluid = T(kind == FLUID)
print("computePre + normals + pnd %.2f  smoothing %.2f  applied potential %.2f [%d its, conv %d]  Poisson-Boltzmann %.2f [%d Newton, "
      "%d linear its, status %d]  force %.2f  %s  total %.2f ms"
      % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, ia.iters, ia.converged, (t4 - t3) * 1e3, ib.newton_iters,
         ib.linear_iters, ib.status, (t5 - t4) * 1e3, text, (t6 - t0) * 1e3))
moving = T(kind != SOLID)                            # the wall particles keep their velocity (the binding's correction has no kinds)
print("dt %.3g  max|f| %.3g  mean fluid u_x %.3g  max|v| off the walls %.3g"
      % (dt, float(f.abs().max()), float(vstar[fluid, 0].mean()), float(vstar[moving].abs().max())))

print("per call, HIP events, %d repeats after 3 warm-up calls: median [min .. max] us" % args.repeats)
psi_all, phi_all = ghost(psi), ghost(phi)
kw = dict(kinds=KINDS)
t_ek = timed("isph_electrostatic_force (k_ek_force), mirror + phi + force",
             lambda: hip.electrostatic_force(ctx, dp, colmap, ek, psi_all, vfrac, phi=phi_all, f=f, Gc=G, pnd=pnd, with_gradients=False, **kw))
timed("isph_electrostatic_force, gradients written too",
      lambda: hip.electrostatic_force(ctx, dp, colmap, ek, psi_all, vfrac, phi=phi_all, f=f, Gc=G, pnd=pnd, **kw))
t_g1 = timed("isph_gradient (k_gradient) of psi, (Fluid, All)",
             lambda: hip.gradient(ctx, dp, colmap, psi_all, vfrac, antisym=False, Gc=G, filt=(FLUID, ALL), **kw))
t_g2 = timed("isph_gradient (k_gradient) of phi, (Fluid, Fluid)",
             lambda: hip.gradient(ctx, dp, colmap, phi_all, vfrac, antisym=False, Gc=G, filt=(FLUID, FLUID), **kw))
timed("isph_smooth_field (k_smooth_field)", lambda: hip.smooth_field(ctx, dp, colmap, sigma, vfrac, **kw))
print("  fused electrokinetic sweep / two isph_gradient launches (which have no mirror and no force): %.2f" % (t_ek / (t_g1 + t_g2)))
ctx.hold_neighbours(False)

# ---- the fluctuating TGV step -----------------------------------------------------------------------------------------
sp = spec(workload.JITTER)
parts = workload.make_tgv(sp)
n = parts["nlocal"]
v0 = parts["v"][:n]
if args.neighbours == "device":                     # the same particles: ghosts and list rebuilt where the positions are
    tn = sync()
    parts = workload.make_cloud_device(ctx, T(parts["x"][:n]), (L,) * dim, sp.h, sp.cut, dim=dim, like=parts)
    print("ghosts + neighbour list on the device %.2f ms" % ((sync() - tn) * 1e3))
nall = parts["nall"]
dp, colmap, own = upload(parts)
ghost = lambda a: a[own].contiguous()
tag = parts["tag"][:n].contiguous() if hip._is_torch(parts["tag"]) else T(parts["tag"][:n])
rho = torch.full((nall,), 1.0, dtype=torch.float64, device=dev)
nu = torch.full((nall,), 0.1, dtype=torch.float64, device=dev)
dt, kBT, seed = sp.dt, 1e-6, 20240917
print("fluctuating TGV %d-D, %d particles, kBT = %g" % (dim, n, kBT))
ctx.hold_neighbours(True)
t0 = sync()
vfrac = ghost(hip.compute_volumes(ctx, dp, colmap))
G, Lc = hip.compute_corrections(ctx, dp, colmap, vfrac)
t1 = sync()
f = torch.zeros((n, 3), dtype=torch.float64, device=dev)
hip.force_from_random_stress(ctx, dp, colmap, tag, seed, 0, dt, kBT, nu[:n].contiguous(), rho[:n].contiguous(), f, vfrac)
t2 = sync()
v, p = T(v0), torch.zeros(n, dtype=torch.float64, device=dev)
vstar, p, text = momentum_step(dp, colmap, own, None, vfrac, G, Lc, f, v, p, rho, nu, dt)
t3 = sync()
print("computePre %.2f  random stress %.2f  %s  total %.2f ms   max|f| %.3g  net force / sum|f| %.2e"
      % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, text, (t3 - t0) * 1e3, float(f.abs().max()),
         float((f * vfrac[:n, None]).sum(0).abs().max() / (f.abs() * vfrac[:n, None]).sum())))

print("per call, HIP events, %d repeats after 3 warm-up calls: median [min .. max] us" % args.repeats)
rs = hip.random_stress_tensor(ctx, dp, colmap, tag, seed, 0)
rs_all = ghost(rs)
nu_o, rho_o = nu[:n].contiguous(), rho[:n].contiguous()
cols = [torch.rand((nall, 3), dtype=torch.float64, device=dev) for _ in range(dim)]
timed("isph_random_stress_tensor (k_random_stress_tensor)", lambda: hip.random_stress_tensor(ctx, dp, colmap, tag, seed, 1))
t_rs = timed("isph_random_stress_force (k_random_stress_force)",
             lambda: hip.random_stress_force(ctx, dp, colmap, dt, kBT, nu_o, rho_o, rs_all, f, vfrac))
timed("isph_force_from_random_stress (tensor + sweep)",
      lambda: hip.force_from_random_stress(ctx, dp, colmap, tag, seed, 1, dt, kBT, nu_o, rho_o, f, vfrac))
t_d = timed("isph_divergence (k_divergence), AntiSymmetric (Fluid, Fluid)",
            lambda: hip.divergence(ctx, dp, colmap, cols[0], vfrac, antisym=True, alpha=-1.0, filt=(FLUID, FLUID)))
print("  fused stress sweep / %d isph_divergence launches: %.2f" % (dim, t_rs / (dim * t_d)))
ctx.hold_neighbours(False)
ctx.close()
