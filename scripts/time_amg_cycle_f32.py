"""cycle_bits = 32 (the whole V cycle of the Chebyshev-smoothed SA-AMG in single-precision storage) against 64 on the bench
system (100^3 TGV pressure system of bench.py, FGMRES(50), tol 1e-8, the preconditioner rebuilt for every solve).  The two
widths are ALTERNATED repetition by repetition in this one process; one warm-up and ISPH_REPS timed repeats per line:
median (min - max).

  * one V cycle (degree 2), device events, us;
  * the fine-level Chebyshev step with a product, us: a one-level hierarchy with a null vector applies the polynomial of the
    fine level from a zero guess, so (apply of degree 9 - apply of degree 1) / 8 of one repetition is one step; beside it
    the bytes the step streams (per stored entry the value 8|4 B and the 16-bit column 2 B; per row b, dinv, w in, w out,
    y in once, y out at 8|4 B) and the bytes it gathers through L2 (8|4 B of y per stored entry);
  * the set-up cost of the float planes (create + synchronise, host clock);
  * create plus solve and iterations for degree 2 with rho and with eig_type = 1;
  * the pool's peak of live bytes over a create plus solve.

    python scripts/time_amg_cycle_f32.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
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
WIDTHS = (64, 32)


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
r = torch.randn(N, dtype=torch.float64, device=dev)
z = torch.empty_like(r)


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts, fmt="%8.2f (%.2f - %.2f)"):
    return fmt % (med(ts), min(ts), max(ts))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def amg(bits, sweeps=2, **kw):
    return hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=sweeps, cheb_ratio=20.0,
                                                                   cycle_bits=bits, **kw))


say("# scripts/time_amg_cycle_f32.py: %d^3 TGV pressure system, %d rows, FGMRES(50) tol 1e-8, preconditioner rebuilt per solve," % (n, N))
say("# cycle_bits 64 and 32 alternated repetition by repetition, 1 warm-up + %d repeats per line: median (min - max)" % REPS)
say("# device: %s" % torch.cuda.get_device_name(0))

# ---- one cycle ----------------------------------------------------------------------------------------------------------
say()
say("# one V cycle (all levels, Chebyshev degree 2, ratio 20), us, 30 repetitions, device events")
for eig_type in (0, 1):
    Ms = {bits: amg(bits, eig_type=eig_type) for bits in WIDTHS}
    for _ in range(3):
        for bits in WIDTHS:
            Ms[bits].apply(r, z)
    ts = {bits: [] for bits in WIDTHS}
    for _ in range(30):
        for bits in WIDTHS:
            ts[bits].append(event_ms(lambda: Ms[bits].apply(r, z)) * 1e3)
    z64, z32 = torch.empty_like(r), torch.empty_like(r)
    Ms[64].apply(r, z64); Ms[32].apply(r, z32)
    torch.cuda.synchronize()
    say("eig_type %d  levels %s  64 bits %s   32 bits %s   32 / 64: %.3f   ||z32 - z64|| / ||z64|| = %.2e" %
        (eig_type, [Ms[64].level_info(l)["rows"] for l in range(Ms[64].levels)], stats(ts[64], "%8.1f (%.1f - %.1f)"),
         stats(ts[32], "%8.1f (%.1f - %.1f)"), med(ts[32]) / med(ts[64]), float((z32 - z64).norm() / z64.norm())))
    for M in Ms.values():
        M.close()

# ---- the fine-level step --------------------------------------------------------------------------------------------------
say()
say("# the fine-level Chebyshev step with a product, us: a one-level hierarchy applies the fine level's polynomial from a zero")
say("# guess; (apply of degree 9 - apply of degree 1) / 8 of one repetition, 30 repetitions, device events")
say("# streamed = stored x (value 8|4 + column 2) + rows x 6 vectors x 8|4 B + slices x (16 + 256); gathered = stored x 8|4 B of y")
Ms = {bits: (amg(bits, 9, max_levels=1), amg(bits, 1, max_levels=1)) for bits in WIDTHS}
for _ in range(3):
    for bits in WIDTHS:
        for M in Ms[bits]:
            M.apply(r, z)
ts = {bits: [] for bits in WIDTHS}
for _ in range(30):
    for bits in WIDTHS:
        t9 = event_ms(lambda: Ms[bits][0].apply(r, z))
        t1 = event_ms(lambda: Ms[bits][1].apply(r, z))
        ts[bits].append((t9 - t1) / 8.0 * 1e3)
for bits in WIDTHS:
    for M in Ms[bits]:
        M.close()
info = A.info()
byt = {}
for bits in WIDTHS:
    w = bits // 8
    streamed = info["stored"] * (w + A.column_bits() // 8) + N * 6 * w + info["nslices"] * (16 + (256 if A.column_bits() == 16 else 0))
    byt[bits] = (streamed, info["stored"] * w)
    say("%2d bits  %s us   streamed %7.1f MB (%5.0f GB/s)   gathered %7.1f MB   streamed + gathered %5.0f GB/s   (%d + %d B per stored entry)" %
        (bits, stats(ts[bits], "%8.1f (%.1f - %.1f)"), streamed / 1e6, streamed / med(ts[bits]) / 1e3, byt[bits][1] / 1e6,
         (streamed + byt[bits][1]) / med(ts[bits]) / 1e3, w + A.column_bits() // 8, w))
say("32 / 64: time %.3f   streamed bytes %.3f   streamed + gathered bytes %.3f" %
    (med(ts[32]) / med(ts[64]), byt[32][0] / byt[64][0], sum(byt[32]) / sum(byt[64])))


# ---- create plus solve ----------------------------------------------------------------------------------------------------
def solve_pair(label, make):
    acc = {bits: dict(setup=[], solve=[], its=0, conv=1, peak=0) for bits in WIDTHS}
    for rep_ in range(REPS + 1):
        for bits in WIDTHS:
            bw.copy_(b); x.zero_()
            torch.cuda.synchronize()
            hip.pool_info(reset_peak=True)
            t0 = time.perf_counter()
            M = make(bits)
            ctx.sync()
            t1 = time.perf_counter()
            inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            a = acc[bits]
            a["peak"] = max(a["peak"], hip.pool_info()["peak_live"])
            M.close()
            if rep_ > 0:
                a["setup"].append((t1 - t0) * 1e3); a["solve"].append((t2 - t1) * 1e3)
            a["its"], a["conv"] = inf.iters, a["conv"] and inf.converged
    for bits in WIDTHS:
        a = acc[bits]
        say("%-40s %2d bits  iterations %3d%s  create ms %s  solve ms %s  sum %7.2f  pool peak %7.1f MB" %
            (label, bits, a["its"], "" if a["conv"] else " (NOT converged)", stats(a["setup"]), stats(a["solve"]),
             med(a["setup"]) + med(a["solve"]), a["peak"] / 1e6))
    say("%-40s 32 / 64: solve %.3f  create %.3f  sum %.3f  (float planes: %+.2f ms of create)" %
        (label, med(acc[32]["solve"]) / med(acc[64]["solve"]), med(acc[32]["setup"]) / med(acc[64]["setup"]),
         (med(acc[32]["setup"]) + med(acc[32]["solve"])) / (med(acc[64]["setup"]) + med(acc[64]["solve"])),
         med(acc[32]["setup"]) - med(acc[64]["setup"])))


say()
say("# create plus solve, host clock around calls that end in a device synchronise, ms; pool peak = the pool's high-water mark")
say("# of live bytes over the create and the solve (matrix, Krylov workspace and hierarchy)")
solve_pair("SA-AMG Chebyshev degree 2, rho", lambda bits: amg(bits))
solve_pair("SA-AMG Chebyshev degree 2, eig_type 1", lambda bits: amg(bits, eig_type=1))

say()
say("# create alone (create + synchronise, host clock, %d repetitions alternated), ms: what the float planes cost" % (4 * REPS))
tset = {bits: [] for bits in WIDTHS}
for rep_ in range(4 * REPS + 1):
    for bits in WIDTHS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = amg(bits)
        ctx.sync()
        t1 = time.perf_counter()
        M.close()
        if rep_ > 0:
            tset[bits].append((t1 - t0) * 1e3)
say("64 bits %s   32 bits %s   the float planes of A_l, P_l, R_l, A_l P_l and D^-1: %+.3f ms" %
    (stats(tset[64]), stats(tset[32]), med(tset[32]) - med(tset[64])))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
