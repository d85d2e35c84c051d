"""Block ILU(k) as the smoother of the SA-AMG (isph_amg_params::smoother = 4, ML's "IFPACK" smoother) on the bench system
(100^3 TGV pressure system of bench.py, tol 1e-8, the preconditioner rebuilt for every solve): create ms, solve ms and
iterations of the SA-AMG with smoother 0, with smoother 2 of degree 2, with smoother 4 at fill 0 and 1 and sweeps 1 and
3, and of the stand-alone "bjacobi-ilu0" beside them -- the configurations ALTERNATED repetition by repetition in this
one process.  Then one V cycle of every configuration in us from device events, and the coarse levels of smoother 4 as
dense 64-row block inverses (k_ilu_dense_build) against the chunk stream (ISPH_AMG_COARSE_STREAM=1): create ms and cycle us.

    python scripts/time_amg_ilu.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
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


def amg(**kw):
    return lambda: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, **kw))


CONFIGS = [("SA-AMG smoother 0 (symmetric Gauss-Seidel), 1 sweep", amg(block=512, smoother=0)),
           ("SA-AMG smoother 2 (Chebyshev), degree 2", amg(smoother=2, sweeps=2))]
for fill in (0, 1):
    for sweeps in (1, 3):
        CONFIGS.append(("SA-AMG smoother 4 (ILU(%d)), %d sweep%s" % (fill, sweeps, "" if sweeps == 1 else "s"),
                        amg(block=512, smoother=4, ilu_fill=fill, sweeps=sweeps)))
CONFIGS.append(("block ILU(0) alone, library bricks", lambda: hip.Precond(ctx, A, "bjacobi-ilu0", 0)))

say("# scripts/time_amg_ilu.py: %d^3 TGV pressure system, %d rows, FGMRES(50) tol 1e-8, preconditioner rebuilt per solve," % (n, N))
say("# 1 warm-up + %d repeats, the configurations alternated repetition by repetition; host clock around calls that end in a" % REPS)
say("# device synchronise: median (min - max)")
say("# device: %s" % torch.cuda.get_device_name(0))
acc = [dict(create=[], solve=[], its=0, conv=1) for _ in CONFIGS]
for rep in range(REPS + 1):
    for a, (label, make) in zip(acc, CONFIGS):
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
        if rep > 0:
            a["create"].append((t1 - t0) * 1e3); a["solve"].append((t2 - t1) * 1e3)
        a["its"], a["conv"] = inf.iters, a["conv"] and inf.converged
for a, (label, _) in zip(acc, CONFIGS):
    say("%-52s iterations %3d%s  create ms %s  solve ms %s  sum %7.2f" %
        (label, a["its"], "" if a["conv"] else " (NOT converged)", stats(a["create"]), stats(a["solve"]),
         med(a["create"]) + med(a["solve"])))


def cycle_us(M, r, z, reps=30):
    for _ in range(3):
        M.apply(r, z)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        M.apply(r, z)
        e1.record(st)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


r = torch.randn(N, dtype=torch.float64, device=dev)
z = torch.empty_like(r)
say()
say("# one application (one V cycle), us, 30 repeats, device events: median (min - max)")
for label, make in CONFIGS:
    M = make()
    t = cycle_us(M, r, z)
    extra = ""
    if isinstance(M, hip.PrecondAMG):
        extra = "   levels %s smoother paths %s" % ([M.level_info(l)["rows"] for l in range(M.levels)],
                                                   [M.path(l)["smoother"] for l in range(M.levels)])
    say("%-52s %9.1f (%.1f - %.1f)%s" % (label, med(t), min(t), max(t), extra))
    M.close()

say()
say("# smoother 4: coarse levels as dense 64-row block inverses against the chunk stream (ISPH_AMG_COARSE_STREAM=1),")
say("# alternated; create ms (host clock, %d repeats) and one V cycle in us (device events, 30 repeats)" % REPS)
for fill in (0, 1):
    make = amg(block=512, smoother=4, ilu_fill=fill, sweeps=1)
    tc, cyc, paths = {"dense": [], "stream": []}, {}, {}
    for rep in range(REPS + 1):
        for mode in ("dense", "stream"):
            if mode == "stream":
                os.environ["ISPH_AMG_COARSE_STREAM"] = "1"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = make()
            ctx.sync()
            t1 = time.perf_counter()
            os.environ.pop("ISPH_AMG_COARSE_STREAM", None)
            if rep > 0:
                tc[mode].append((t1 - t0) * 1e3)
            if rep == REPS:
                cyc[mode] = cycle_us(M, r, z)
                paths[mode] = [M.path(l)["smoother"] for l in range(M.levels)]
            M.close()
    for mode in ("dense", "stream"):
        say("ILU(%d) coarse levels %-6s paths %-16s create ms %s   cycle us %9.1f (%.1f - %.1f)" %
            (fill, mode, paths[mode], stats(tc[mode]), med(cyc[mode]), min(cyc[mode]), max(cyc[mode])))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
