"""The GMRES-polynomial preconditioner "gmres-poly<d>" (include/isph_hip.h, csrc/gmres_poly.hpp) beside point Jacobi and
"chebyshev3" on the bench system (100^3 TGV pressure system of bench.py, FGMRES(50), tol 1e-8, the preconditioner rebuilt
for every solve), all variants ALTERNATED repetition by repetition in this one process:

  * jacobi, chebyshev3 with lambda = rho and with eig_type = 1, gmres-poly of degree 3, 4, 6 and 8 (with the null vector):
    create ms, solve ms and iterations, median (min - max) of ISPH_REPS repeats after one warm-up;
  * operator sweeps per solve: the launches of the profile class "spmv" (the solver's products and every fused step of a
    polynomial) in one more, untimed solve with the profile on; the sweeps of the set-up (Arnoldi products) by count;
  * global reductions per solve, counted from the code (on one rank an all-reduce is a no-op: nothing to measure): 3 per
    FGMRES iteration of a singular system -- two in the Gram-Schmidt step, one in the null-vector dot of the product --,
    2 more for every second Gram-Schmidt pass (isph_solve_info::reorth), 2 at the start; the Arnoldi set-ups 5 per step
    with a null vector (the projection, two passes of two) and 4 without;
  * one fused step k_sell_poly_step in us beside its algorithmic bytes, beside ISPH_POLY_UNFUSED=1 and beside
    k_sell_cheby_step: (apply of degree 9 - apply of degree 1) / 8, device events, the three alternated.

    python scripts/time_gmres_poly.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import isph_amd  # noqa: F401
from isph_amd import hip, workload

n = int(os.environ.get("ISPH_NCELL", "100"))
REPS = int(os.environ.get("ISPH_REPS", "7"))
out_path = sys.argv[1] if len(sys.argv) > 1 else None
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = hip.Context(0, stream=st.cuda_stream, ordering="bricks")
spec = workload.TGVSpec(dim=3, ncell=(n, n, n), brick=(n, n, n), mode=workload.ADVECT)
parts = workload.make_tgv(spec)
dp = dict(parts)
for k in ("x", "type", "neigh_ptr", "neigh_idx"):
    dp[k] = torch.from_numpy(np.ascontiguousarray(parts[k])).to(dev)
own = torch.from_numpy(parts["owner_index"].astype(np.int64)).to(dev)
colmap = own.to(torch.int32).contiguous()
rho = torch.from_numpy(parts["rho"]).to(dev)
vs = torch.from_numpy(np.ascontiguousarray(parts["v"])).to(dev)
vf = hip.compute_volumes(ctx, dp, colmap)
A, b = hip.assemble_poisson(ctx, dp, colmap, spec.dt, rho, vs, vfrac=vf[own].contiguous())
N = n ** 3
nv = torch.full((N,), 1.0 / np.sqrt(float(N)), dtype=torch.float64, device=dev)
prm = hip.SolverParams(tol=1e-8)
x = torch.zeros(N, dtype=torch.float64, device=dev)
bw = b.clone()


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts):
    return "%8.2f (%.2f - %.2f)" % (med(ts), min(ts), max(ts))


# label, constructor, sweeps of the set-up, reductions of the set-up
VARIANTS = [
    ("jacobi", lambda: hip.Precond(ctx, A, "jacobi", 0), 0, 0),
    ("chebyshev3 (rho)", lambda: hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0), 0, 0),
    ("chebyshev3 (eig_type 1)", lambda: hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0, eig_type=1), 10, 41),
] + [("gmres-poly%d" % d, (lambda d=d: hip.PrecondGmresPoly(ctx, A, d, nullvec=nv)), d, 5 * d + 3) for d in (3, 4, 6, 8)]

acc = {v[0]: dict(setup=[], solve=[], its=0, conv=1, reorth=0) for v in VARIANTS}
for rep_ in range(REPS + 1):
    for label, make, _, _ in VARIANTS:
        bw.copy_(b); x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = make()
        ctx.sync()
        t1 = time.perf_counter()
        inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        M.close()
        a = acc[label]
        if rep_ > 0:
            a["setup"].append((t1 - t0) * 1e3); a["solve"].append((t2 - t1) * 1e3)
        a["its"], a["conv"], a["reorth"] = inf.iters, a["conv"] and inf.converged, inf.reorth

# one more solve each with the profile on: the sweeps of the solve (not timed)
ctx.set_profile(True)
for label, make, _, _ in VARIANTS:
    M = make()
    ctx.sync()
    ctx.profile_read()
    bw.copy_(b); x.zero_()
    hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
    ctx.sync()
    acc[label]["sweeps"] = ctx.profile_read()["spmv"][1]
    M.close()
ctx.set_profile(False)

say("# scripts/time_gmres_poly.py: %d^3 TGV pressure system, %d rows, FGMRES(50) tol 1e-8, preconditioner rebuilt per solve," % (n, N))
say("# the variants alternated repetition by repetition; 1 warm-up + %d repeats, host clock around calls that end in a device" % REPS)
say("# synchronise: median (min - max).  sweeps: launches of the profile class \"spmv\" in one more solve (+ the set-up's products);")
say("# reductions: counted from the code, 3 per iteration + 2 per second Gram-Schmidt pass + 2 (+ the set-up's)")
say("# device: %s" % torch.cuda.get_device_name(0))
for label, _, s_setup, r_setup in VARIANTS:
    a = acc[label]
    say("%-24s iterations %3d%s  create ms %s  solve ms %s  sum %7.2f  sweeps %3d + %2d  reductions %3d + %2d" %
        (label, a["its"], "" if a["conv"] else " (NOT converged)", stats(a["setup"]), stats(a["solve"]), med(a["setup"]) + med(a["solve"]),
         a["sweeps"], s_setup, 3 * a["its"] + 2 * a["reorth"] + 2, r_setup))
base = acc["jacobi"]
for label, _, _, r_setup in VARIANTS[1:]:
    a = acc[label]
    say("%-24s against jacobi: sum %.3f  reductions %.3f" %
        (label, (med(a["setup"]) + med(a["solve"])) / (med(base["setup"]) + med(base["solve"])),
         (3 * a["its"] + 2 * a["reorth"] + 2 + r_setup) / float(3 * base["its"] + 2 * base["reorth"] + 2)))


# ---- one fused step beside the unfused composition and the Chebyshev step --------------------------------------------
def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def pair(make):
    return make(9), make(1)


os.environ["ISPH_POLY_UNFUSED"] = "1"
unfused = pair(lambda d: hip.PrecondGmresPoly(ctx, A, d, nullvec=nv))
os.environ.pop("ISPH_POLY_UNFUSED", None)
STEPS = [("k_sell_poly_step (fused)", pair(lambda d: hip.PrecondGmresPoly(ctx, A, d, nullvec=nv))),
         ("ISPH_POLY_UNFUSED=1", unfused),
         ("k_sell_cheby_step", pair(lambda d: hip.PrecondChebyshev(ctx, A, degree=d)))]
rr = torch.randn(N, dtype=torch.float64, device=dev)
zz = torch.empty_like(rr)
for _ in range(3):
    for _, (M9, M1) in STEPS:
        M9.apply(rr, zz); M1.apply(rr, zz)
ts = {label: [] for label, _ in STEPS}
for _ in range(30):
    for label, (M9, M1) in STEPS:
        t9 = event_ms(lambda: M9.apply(rr, zz))
        t1 = event_ms(lambda: M1.apply(rr, zz))
        ts[label].append((t9 - t1) / 8.0 * 1e3)
i, cb = A.info(), A.column_bits()
per_slice = i["nslices"] * (16 + (256 if cb == 16 else 0))
# per row: the polynomial reads x (every x counted once: gathers beyond that are cache hits), dinv and z and writes out and z
# (5 x 8 B; the second half of a pair reads out as well: 6 x 8); Chebyshev b, dinv, w in, w out, y in, y out (6 x 8)
bytes_of = {"k_sell_poly_step (fused)": i["stored"] * (8 + cb // 8) + N * 40 + per_slice,
            "ISPH_POLY_UNFUSED=1": i["stored"] * (8 + cb // 8) + N * 24 + per_slice + N * 48,
            "k_sell_cheby_step": i["stored"] * (8 + cb // 8) + N * 48 + per_slice}
say()
say("# one step with a matrix product, us: (apply of degree 9 - apply of degree 1) / 8 of the same repetition, 30 repeats, device")
say("# events, the three forms alternated; the roots at degree 9: %s" % ("".join("p" if abs(t.imag) > 0 else "r" for t in STEPS[0][1][0].roots())))
say("# bytes = stored x (8 + column %d) + rows x (40: x, dinv, z in, z out, out | Chebyshev 48: b, dinv, w in, w out, y in, y out) + slices;" % (cb // 8))
say("# unfused: the product's 24 per row (x, dinv, y out) + the update's 48 (x, y, out, z in, z out and out read by pairs)")
ref = med(ts["k_sell_cheby_step"])
for label, _ in STEPS:
    t = ts[label]
    say("%-26s %8.1f (%.1f - %.1f) us  %7.1f MB  %5.0f GB/s   against k_sell_cheby_step %.3f" %
        (label, med(t), min(t), max(t), bytes_of[label] / 1e6, bytes_of[label] / med(t) / 1e3, med(t) / ref))
for _, (M9, M1) in STEPS:
    M9.close(); M1.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
