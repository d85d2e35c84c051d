"""The two-phase droplet of sph-script/square-droplet-{2d,3d}.lmp (--walls: liquid-drop-on-solid-2d.lmp) through whole
pressure-correction time steps on the device, Symmetric operator family, device-resident arrays: computePre (volumes,
G_i, L_i) -> wall normals + particle number density (with walls) -> continuum surface force -> Helmholtz with that force
(theta = 1/2, dim right-hand sides, FGMRES + block ILU(0)) -> Poisson -> zero mean -> corrections -> advance.  The
neighbour list of every step comes from the host (LAMMPS' job): workload.make_cloud on the moved particles -- or, with
--neighbours device, from workload.make_cloud_device: the positions then never leave the GPU between two steps.

Then the four surface-tension sweeps beside gradient + divergence on the same particles, HIP events around each call on
the context's stream, neighbour layout held, warm, median and spread of --repeats calls.

    python scripts/droplet_step.py --dim 2 --N 512
    python scripts/droplet_step.py --dim 3 --N 64
    python scripts/droplet_step.py --dim 2 --N 512 --neighbours device"""
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
ap.add_argument("--N", type=int, default=512, help="the box is 2 N cells wide")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--walls", action="store_true", help="liquid drop on a solid slab (2-D)")
ap.add_argument("--jitter", type=float, default=0.05)
ap.add_argument("--neighbours", default="host", choices=["host", "device"],
                help="where ghosts and neighbour list of the moved particles are rebuilt between two steps")
args = ap.parse_args()

dim = args.dim
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = hip.Context(0, stream=stream.cuda_stream)
p0 = workload.make_droplet(args.N, dim=dim, shape="square", wall_layers=4 if args.walls else 0, jitter=args.jitter)
kinds, phase, h, cut, dt = p0["kinds"], p0["phase"], p0["h"], p0["cut"], p0["dt"]
n = p0["nlocal"]
L = 2.0 * np.pi
prm = hip.CsfParams(phase, theta=1.0472 if args.walls else 0.0)
fixed = np.array([k != workload.FLUID_KIND for k in kinds])
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
kw = dict(kinds=kinds)


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


parts = p0
like_d = dict(p0, **{k: T(p0[k]) for k in ("type", "rho", "nu")})
x_own, typ_own = p0["x"][:n].copy(), p0["type"][:n].copy()
v = torch.zeros((n, 3), dtype=torch.float64, device=dev)
p = torch.zeros(n, dtype=torch.float64, device=dev)
g = np.zeros(3)
print("droplet %d-D, %d particles, %d phases%s, h = %.4g, cut = %.4g, dt = %.4g"
      % (dim, n, 2, " + walls" if args.walls else "", h, cut, dt))
for step in range(args.steps):
    if step > 0 and args.neighbours == "device":   # ghosts and lists of the moved particles, rebuilt where they are
        tn = sync()
        parts = workload.make_cloud_device(ctx, x_own, (L,) * dim, h, cut, dim=dim, like=like_d)
        print("step %d: ghosts + neighbour list on the device %.2f ms" % (step, (sync() - tn) * 1e3))
    elif step > 0:                                 # the host rebuilds ghosts and lists from the moved particles
        like = dict(p0, type=np.r_[typ_own, p0["type"][n:]])
        parts = workload.make_cloud(x_own, (L,) * dim, h, cut, dim=dim, like=like)
    dp, colmap, own = upload(parts)
    nall = parts["nall"]
    rho = torch.full((nall,), 1.0, dtype=torch.float64, device=dev)
    nu = torch.full((nall,), 0.1, dtype=torch.float64, device=dev)
    ghost = lambda a: a[own].contiguous()
    ctx.hold_neighbours(True)
    t0 = sync()
    vfrac = ghost(hip.compute_volumes(ctx, dp, colmap))
    G, Lc = hip.compute_corrections(ctx, dp, colmap, vfrac)
    t1 = sync()
    normal = pnd = None
    if args.walls:
        nrm, pn = hip.compute_normals(ctx, dp, colmap, vfrac, G, **kw)
        normal, pnd = nrm, ghost(pn)
    t2 = sync()
    f = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    hip.surface_tension_csf(ctx, dp, colmap, prm, vfrac, G, f, wall_normal=normal, pnd=pnd, **kw)
    t3 = sync()
    H, bh = hip.assemble_helmholtz(ctx, dp, colmap, dt, 0.5, nu, rho, ghost(p), ghost(f), g, ghost(v), antisym=False,
                                   vfrac=vfrac, Gc=G, Lc=Lc, **kw)
    MH = hip.Precond(ctx, H, "bjacobi-ilu0", 512)
    xh = torch.cat([v[:, k] for k in range(dim)]).contiguous()
    ih = hip.solve(ctx, H, bh[:dim * n].contiguous(), xh, prec=MH, singular=False, nvec=dim, lda=n)
    MH.close(); H.close()
    vstar = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    for k in range(dim):
        vstar[:, k] = xh[k * n:(k + 1) * n]
    t4 = sync()
    A, b = hip.assemble_poisson(ctx, dp, colmap, dt, rho, ghost(vstar), antisym=False, vfrac=vfrac, Gc=G, Lc=Lc,
                                normal=None if normal is None else ghost(normal), **kw)
    M = hip.Precond(ctx, A, "bjacobi-ilu0", 512)
    dpv = torch.zeros(n, dtype=torch.float64, device=dev)
    info = hip.solve(ctx, A, b, dpv, prec=M, singular=True)
    M.close(); A.close()
    dpv -= dpv.mean()
    t5 = sync()
    vs_all, p_all = ghost(vstar), ghost(p)
    hip.correct_velocity_pressure(ctx, dp, colmap, dt, rho, ghost(dpv), vs_all, p_all, vfrac, antisym=False, Gc=G)
    dpa = hip.advance_begin(ctx, dp, colmap, dt, p_all, ghost(v), vs_all, vfrac, antisym=False, Gc=G)
    xd, pd, vd = dp["x"][:n].clone(), p_all[:n].clone(), v.clone()
    hip.advance_end(ctx, n, dim, dt, dpa, vs_all[:n].contiguous(), pd, xd, vd)
    t6 = sync()
    ctx.hold_neighbours(False)
    v, p = vd, pd
    x_own = xd if args.neighbours == "device" else xd.cpu().numpy()
    print("step %d: computePre %.2f  normals %.2f  surface tension %.2f  helmholtz %.2f [%d its, conv %d]  poisson %.2f [%d its, conv %d]"
          "  correct+advance %.2f  total %.2f ms   max|f| %.3g  max|v| %.3g"
          % (step, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, ih.iters, ih.converged, (t5 - t4) * 1e3,
             info.iters, info.converged, (t6 - t5) * 1e3, (t6 - t0) * 1e3, float(f.abs().max()), float(v.abs().max())))

# ---- the sweeps one by one, beside gradient + divergence on the same particles ---------------------------------------
dp, colmap, own = upload(parts)
ghost = lambda a: a[own].contiguous()
ctx.hold_neighbours(True)
vfrac = ghost(hip.compute_volumes(ctx, dp, colmap))
G, Lc = hip.compute_corrections(ctx, dp, colmap, vfrac)
nrm, pn = hip.compute_normals(ctx, dp, colmap, vfrac, G, **kw)
pnd = ghost(pn)
wall = nrm if args.walls else None
_, nmag = hip.csf_phase_normal(ctx, dp, colmap, prm, vfrac, G, wall_normal=wall, pnd=pnd if args.walls else None, **kw)
nm_all = ghost(nmag)
f = torch.zeros((n, 3), dtype=torch.float64, device=dev)
scal = torch.rand(parts["nall"], dtype=torch.float64, device=dev)
vec = torch.rand((parts["nall"], 3), dtype=torch.float64, device=dev)
s = np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 0.5], [0.0, 0.5, 1.5]])
calls = [
    ("isph_gradient (k_gradient)", lambda: hip.gradient(ctx, dp, colmap, scal, vfrac, antisym=False, Gc=G, **kw)),
    ("isph_divergence (k_divergence)", lambda: hip.divergence(ctx, dp, colmap, vec, vfrac, antisym=False, Gc=G, **kw)),
    ("isph_compute_normals (k_normals)", lambda: hip.compute_normals(ctx, dp, colmap, vfrac, G, **kw)),
    ("isph_csf_phase_normal (k_csf_phase_normal)",
     lambda: hip.csf_phase_normal(ctx, dp, colmap, prm, vfrac, G, wall_normal=wall, pnd=pnd if args.walls else None,
                                  with_grad=False, **kw)),
    ("isph_csf_force (k_csf_force)", lambda: hip.csf_force(ctx, dp, colmap, prm, vfrac, G, nm_all, f, with_kappa=False, **kw)),
    ("isph_pairwise_force (k_pairwise_force)", lambda: hip.pairwise_force(ctx, dp, colmap, 1, phase, s, f, **kw)),
]
print("per call, HIP events, %d repeats after 3 warm-up calls: median [min .. max] us" % args.repeats)
for name, fn in calls:
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
    print("  %-46s %8.1f [%8.1f .. %8.1f]" % (name, np.median(ts), ts[0], ts[-1]))
ctx.hold_neighbours(False)
ctx.close()
