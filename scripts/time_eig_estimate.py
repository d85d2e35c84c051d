"""The eigenvalue estimate (eig_type = 1: Arnoldi on D^-1 A, include/isph_hip.h) against the bound rho (eig_type = 0) on the
bench system (100^3 TGV pressure system of bench.py, FGMRES(50), tol 1e-8, the preconditioner rebuilt for every solve),
the two rules ALTERNATED repetition by repetition in this one process:

  * "chebyshev3" (ratio 30), SA-AMG with Chebyshev degree 2 (ratio 20), SA-AMG with symmetric Gauss-Seidel: create ms,
    solve ms and iterations, median (min - max) of ISPH_REPS repeats after one warm-up;
  * lambda_used beside rho and the Arnoldi steps of every level of the two hierarchies and of the stand-alone polynomial;
  * the estimate's own time per level: create of a degree-1 polynomial with eig_type 1 minus the same create with
    eig_type 0, with the fused product (k_sell_dinv_spmv) and with ISPH_EIG_UNFUSED=1 (product + scaling kernel);
    level l > 0: the level operator exported from the hierarchy and set up as a matrix of its own.

    python scripts/time_eig_estimate.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
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


def solve_pair(label, make):
    """make(eig_type); 0 and 1 alternated, one warm-up each; returns the last pair of preconditioners' estimates"""
    acc = {e: dict(setup=[], solve=[], its=0, conv=1, est=None) for e in (0, 1)}
    for rep_ in range(REPS + 1):
        for e in (0, 1):
            bw.copy_(b); x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = make(e)
            ctx.sync()
            t1 = time.perf_counter()
            inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            a = acc[e]
            if rep_ == REPS:
                a["est"] = [M.eig_estimate(l) for l in range(getattr(M, "levels", 1))]
            M.close()
            if rep_ > 0:
                a["setup"].append((t1 - t0) * 1e3); a["solve"].append((t2 - t1) * 1e3)
            a["its"], a["conv"] = inf.iters, a["conv"] and inf.converged
    for e in (0, 1):
        a = acc[e]
        say("%-36s eig_type %d  iterations %3d%s  create ms %s  solve ms %s  sum %7.2f" %
            (label, e, a["its"], "" if a["conv"] else " (NOT converged)", stats(a["setup"]), stats(a["solve"]),
             med(a["setup"]) + med(a["solve"])))
    say("%-36s 1 / 0: solve %.3f  create %.3f  sum %.3f  (the estimates: %+.2f ms of create)" %
        (label, med(acc[1]["solve"]) / med(acc[0]["solve"]), med(acc[1]["setup"]) / med(acc[0]["setup"]),
         (med(acc[1]["setup"]) + med(acc[1]["solve"])) / (med(acc[0]["setup"]) + med(acc[0]["solve"])),
         med(acc[1]["setup"]) - med(acc[0]["setup"])))
    for l, est in enumerate(acc[1]["est"]):
        say("%-36s level %d  lambda_used %.6f  rho %.6f  Arnoldi steps %d" % (label, l, est["lambda_used"], est["rho"], est["steps"]))


say("# scripts/time_eig_estimate.py: %d^3 TGV pressure system, %d rows, FGMRES(50) tol 1e-8, preconditioner rebuilt per solve," % (n, N))
say("# eig_type 0 (lambda = rho = ||D^-1 A||_inf) and 1 (10 Arnoldi steps, clipped by rho) alternated repetition by repetition;")
say("# 1 warm-up + %d repeats, host clock around calls that end in a device synchronise: median (min - max)" % REPS)
say("# device: %s" % torch.cuda.get_device_name(0))
solve_pair("chebyshev3 (ratio 30)", lambda e: hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0, eig_type=e))
solve_pair("SA-AMG Chebyshev degree 2 ratio 20",
           lambda e: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2, cheb_ratio=20.0, eig_type=e)))
solve_pair("SA-AMG symmetric Gauss-Seidel",
           lambda e: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(block=512, theta=0.0, smoother=0, eig_type=e)))

say()
say("# the estimate alone, ms: create of a degree-1 polynomial with eig_type 1 minus the create with eig_type 0 of the same")
say("# repetition (host clock, create + synchronise), %d repetitions, fused product and ISPH_EIG_UNFUSED=1 alternated" % (2 * REPS))
G = hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2, eig_type=1))
mats = [(A, N, A.info()["nnz"])]
for l in range(1, G.levels):
    rp, ci, v = G.export(l, "A")
    mats.append((hip.Matrix.from_csr(ctx, rp, ci, v), len(rp) - 1, len(v)))
G.close()


def create_ms(Am, eig_type, unfused):
    if unfused:
        os.environ["ISPH_EIG_UNFUSED"] = "1"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M = hip.PrecondChebyshev(ctx, Am, degree=1, eig_type=eig_type)
    ctx.sync()
    t1 = time.perf_counter()
    os.environ.pop("ISPH_EIG_UNFUSED", None)
    M.close()
    return (t1 - t0) * 1e3


for l, (Am, nrow, nnz) in enumerate(mats):
    ts = {False: [], True: []}
    try:
        for rep_ in range(2 * REPS + 1):
            for unfused in (False, True):
                t = create_ms(Am, 1, unfused) - create_ms(Am, 0, unfused)
                if rep_ > 0:
                    ts[unfused].append(t)
    except hip.IsphError as e:      # (a coarse operator with an empty row has no stand-alone polynomial)
        say("level %d  rows %8d  entries %10d   not measured: %s" % (l, nrow, nnz, e))
        continue
    say("level %d  rows %8d  entries %10d   fused %s   unfused %s   fused / unfused %.3f" %
        (l, nrow, nnz, stats(ts[False]), stats(ts[True]), med(ts[False]) / med(ts[True])))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
