"""Refresh of the SA-AMG on new matrix values with the hierarchy kept (isph_prec_refactor of "sa-amg", csrc/amg.hpp
amg_refactor) against the create call, on the bench system (100^3 TGV pressure system of bench.py, tol 1e-8).  The matrix
is brought in from its CSR while isph_ctx_hold_pattern is on (the caller's row numbering), so that its values can be
updated in place.  Per smoother -- 0, 2 of degree 2 with rho and with eig_type = 1, 4 at fill 0 -- and ALTERNATED repetition
by repetition in this one process:
  * create with the mode off (what the commit before this feature does), create with the mode on, refactor, and refactor
    with ISPH_AMG_REFRESH_TWO_PASS=1 (the two-pass kernels of the create call in the place of the refresh kernels), ms;
  * create + solve against update_values + refactor + solve, ms and iterations;
  * the bytes the hierarchy holds after create with the mode off and on, and the pool peak of a refactor.
Then the Poisson-Boltzmann harmonic case (ISPH_PB_N, default 256; prec_max_age = 1) with prec_refresh 0 and 1.

    python scripts/time_amg_refresh.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import torch
import isph_amd  # noqa: F401
from isph_amd import hip, workload

n = int(os.environ.get("ISPH_NCELL", "100"))
REPS = int(os.environ.get("ISPH_REPS", "7"))
PB_N = int(os.environ.get("ISPH_PB_N", "256"))
out_path = sys.argv[1] if len(sys.argv) > 1 else None
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = hip.Context(0, stream=st.cuda_stream, ordering="caller")
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
A0, b = hip.assemble_poisson(ctx, dp, colmap, spec.dt, rho, vs, vfrac=vf[own].contiguous())
rp, ci, val = A0.export_csr()
A0.close()
N = n ** 3
rp_d, ci_d = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
val_d = torch.from_numpy(val).to(dev)
# the second values: the off-diagonal entries x 2.5, the diagonal x 2.75 -- rows stay diagonally dominant, the order of a row's
# couplings stands, so a fresh create aggregates as the kept hierarchy does (README); the matrix is regular
diag = torch.from_numpy(ci == np.repeat(np.arange(N), np.diff(rp))).to(dev)
val2_d = torch.where(diag, 2.75 * val_d, 2.5 * val_d).contiguous()
ctx.hold_pattern(True)
A = hip.Matrix.from_csr(ctx, rp_d, ci_d, val_d)
ctx.hold_pattern(False)
nv = torch.full((N,), 1.0 / np.sqrt(float(N)), dtype=torch.float64, device=dev)
prm = hip.SolverParams(tol=1e-8)
x = torch.zeros(N, dtype=torch.float64, device=dev)
bw = b.clone()


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts):
    return "%8.2f (%.2f - %.2f)" % (med(ts), min(ts), max(ts))


def timed(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


CONFIGS = [("smoother 0 (symmetric Gauss-Seidel)", dict(block=512, smoother=0)),
           ("smoother 2 (Chebyshev), degree 2, rho", dict(smoother=2, sweeps=2)),
           ("smoother 2 (Chebyshev), degree 2, eig_type 1", dict(smoother=2, sweeps=2, eig_type=1)),
           ("smoother 4 (block ILU(0))", dict(block=512, smoother=4, ilu_fill=0))]


def create(kw, hold):
    ctx.hold_pattern(hold)
    try:
        return hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, **kw))
    finally:
        ctx.hold_pattern(False)


def solve(M):
    x.zero_()
    bw.copy_(b)
    return hip.solve(ctx, A, bw, x, prec=M, params=prm)


def refactor_two_pass(M):
    os.environ["ISPH_AMG_REFRESH_TWO_PASS"] = "1"
    try:
        M.refactor(A)
    finally:
        del os.environ["ISPH_AMG_REFRESH_TWO_PASS"]


say("# scripts/time_amg_refresh.py: %d^3 TGV pressure system, %d rows, %d entries, FGMRES(50) tol 1e-8, 1 warm-up + %d repeats," % (n, N, len(ci), REPS))
say("# the configurations and the calls alternated repetition by repetition; host clock around calls that end in a device")
say("# synchronise: median (min - max) ms")
say("# device: %s" % torch.cuda.get_device_name(0))
keys = ("create_off", "create_on", "refactor", "refactor_two_pass", "create_solve", "update_refactor_solve")
acc = [dict({k: [] for k in keys}, its_create=0, its_refresh=0, conv=1) for _ in CONFIGS]
for rep in range(REPS + 1):
    for c, (name, kw) in enumerate(CONFIGS):
        a = acc[c]
        A.update_values(val_d)
        t_off, M0 = timed(lambda: create(kw, False))
        M0.close()
        t_on, M = timed(lambda: create(kw, True))
        t_ref, _ = timed(lambda: M.refactor(A))
        t_two, _ = timed(lambda: refactor_two_pass(M))
        # create + solve on the second values against update + refactor + solve of the kept hierarchy
        A.update_values(val2_d)
        t_cs, (Mc, ic) = timed(lambda: (lambda m: (m, solve(m)))(create(kw, False)))
        Mc.close()
        A.update_values(val_d)
        M.refactor(A)

        def held_cycle():
            A.update_values(val2_d)
            M.refactor(A)
            return solve(M)
        t_urs, ir = timed(held_cycle)
        M.close()
        if rep > 0:
            for k, t in zip(keys, (t_off, t_on, t_ref, t_two, t_cs, t_urs)):
                a[k].append(t)
            a["its_create"], a["its_refresh"] = ic.iters, ir.iters
            a["conv"] = a["conv"] and ic.converged == 1 and ir.converged == 1
say()
say("%-46s %26s %26s %26s %26s" % ("SA-AMG set-up, ms", "create, mode off", "create, mode on", "refactor", "refactor, two-pass kernels"))
for (name, _), a in zip(CONFIGS, acc):
    say("%-46s %26s %26s %26s %26s" % (name, stats(a["create_off"]), stats(a["create_on"]), stats(a["refactor"]), stats(a["refactor_two_pass"])))
say()
say("%-46s %26s %5s %30s %5s %s" % ("one system solved, ms", "create + solve", "its", "update + refactor + solve", "its", "converged"))
for (name, _), a in zip(CONFIGS, acc):
    say("%-46s %26s %5d %30s %5d %d" % (name, stats(a["create_solve"]), a["its_create"], stats(a["update_refactor_solve"]), a["its_refresh"], a["conv"]))
say()
say("%-46s %16s %16s %16s %22s" % ("device bytes", "held, mode off", "held, mode on", "the mode adds", "pool peak of a refactor"))
for name, kw in CONFIGS:
    ctx.sync(); hip.pool_trim()
    base = hip.pool_info()["live"]
    M0 = create(kw, False)
    off = hip.pool_info()["live"] - base
    M0.close()
    ctx.sync(); hip.pool_trim()
    M = create(kw, True)
    on = hip.pool_info()["live"] - base
    hip.pool_info(reset_peak=True)
    M.refactor(A)
    peak = hip.pool_info()["peak_live"] - base
    M.close()
    say("%-46s %16d %16d %16d %22d" % (name, off, on, on - off, peak))

# ---- the Newton driver of the Poisson-Boltzmann solve
import test_gpu_poisson_boltzmann as tpb  # noqa: E402
h = tpb._harmonic(ctx, PB_N)
say()
say("Poisson-Boltzmann harmonic case, N = %d (%d rows), SA-AMG, prec_max_age = 1: median (min - max) ms of the solve" % (PB_N, h["n"]))
pb = {0: [], 1: []}
last = {}
for rep in range(REPS + 1):
    for refresh in (0, 1):
        J = tpb._assemble_harmonic(ctx, h)
        psi = np.zeros(h["n"])
        p = hip.PBParams(prec_max_age=1, prec_refresh=refresh)
        t, info = timed(lambda: hip.solve_poisson_boltzmann(ctx, J, psi, h["f"], params=p))
        J.close()
        if rep > 0:
            pb[refresh].append(t)
        last[refresh] = info
for refresh in (0, 1):
    i = last[refresh]
    say("prec_refresh = %d: %s   status %d, Newton steps %d, linear iterations %d, builds %d of which refreshes %d"
        % (refresh, stats(pb[refresh]), i.status, i.newton_iters, i.linear_iters, i.prec_builds, i.prec_refreshes))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
A.close()
ctx.close()
