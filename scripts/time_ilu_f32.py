"""value_bits = 32 of the block ILU against 64 on the bench matrix: the 3-D TGV pressure system (ISPH_NCELL^3 rows) on the
library's bricks, ONE process, the two widths alternated repetition by repetition.

  * one application of "bjacobi-ilu0" and "bjacobi-ilu1", us: HIP events on the library's stream around the solve kernel
    alone (the prec_apply class of isph_ctx_set_profile, what the k_ilu_solve_stream line of bench.py --full reports),
    beside the bytes one application streams -- chunks in use (isph_prec_info) x 64 x (8 | 4 B value + 2 B word) plus a
    byte per chunk, and per row r, z, the pivot and the two 16-bit order tables;
  * the create call, ms (host clock, create + synchronise): the rounding pass runs on every create, and the benchmark
    protocol rebuilds the preconditioner for every solve;
  * a solve with the benchmark's settings (FGMRES(50), default tolerance, singular), the preconditioner created inside
    the timed region: ms and iterations.
One warm-up, then ISPH_REPS repetitions per line: median (min - max).  No speed-up is assumed anywhere: the only figure
known in advance is the byte ratio of the stream, 6 / 10.

    python scripts/time_ilu_f32.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
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
prm = hip.SolverParams()      # bench.py's
x = torch.zeros(N, dtype=torch.float64, device=dev)
bw = b.clone()
KIND = {64: "", 32: "-f32"}


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts, fmt="%.2f"):
    ts = sorted(ts)
    return (fmt + " (" + fmt + " - " + fmt + ")") % (ts[len(ts) // 2], ts[0], ts[-1])


def make(fill, bits):
    return hip.Precond(ctx, A, "bjacobi-ilu%d%s" % (fill, KIND[bits]), 0)


def apply_bytes(M, bits):
    """what one application streams: per chunk in use 64 x (value + 16-bit word) and the info byte; per row r in, z out,
    the pivot and the row's two positions (2 x 2 B)"""
    i = M.info()
    return i["stream_chunks"] * (64 * (bits // 8 + 2) + 1) + N * (8 + 8 + 8 + 4), i


def apply_pair_us(fill, reps=30):
    Ms = {bits: make(fill, bits) for bits in (64, 32)}
    rr = torch.randn(N, dtype=torch.float64, device=dev)
    zz = torch.empty_like(rr)
    for _ in range(3):
        for bits in (64, 32):
            Ms[bits].apply(rr, zz)
    ctx.sync()
    ts = {64: [], 32: []}
    ctx.set_profile(True)
    ctx.profile_read()
    for _ in range(reps):
        for bits in (64, 32):
            Ms[bits].apply(rr, zz)
            ms, calls = ctx.profile_read()["prec_apply"]
            assert calls == 1
            ts[bits].append(ms * 1e3)
    ctx.set_profile(False)
    by = {bits: apply_bytes(Ms[bits], bits) for bits in (64, 32)}
    assert Ms[32].value_bits == 32 and Ms[64].value_bits == 0
    for M in Ms.values():
        M.close()
    return ts, by


def create_pair_ms(fill, reps):
    ts = {64: [], 32: []}
    for rep_ in range(reps + 1):
        for bits in (64, 32):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = make(fill, bits)
            ctx.sync()
            t1 = time.perf_counter()
            M.close()
            if rep_ > 0:
                ts[bits].append((t1 - t0) * 1e3)
    return ts


def solve_pair(fill):
    """the benchmark's protocol: create + solve in the timed region, 64 and 32 alternated, one warm-up each; the solve
    kernel's time inside the solve from one more, untimed, profiled pass per width"""
    acc = {bits: dict(total=[], its=0, conv=1) for bits in (64, 32)}
    for rep_ in range(REPS + 1):
        for bits in (64, 32):
            bw.copy_(b); x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = make(fill, bits)
            inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            M.close()
            a = acc[bits]
            if rep_ > 0:
                a["total"].append((t1 - t0) * 1e3)
            a["its"], a["conv"] = inf.iters, a["conv"] and inf.converged
    for bits in (64, 32):
        bw.copy_(b); x.zero_()
        M = make(fill, bits)
        ctx.sync()
        ctx.set_profile(True)
        ctx.profile_read()
        hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
        ms, calls = ctx.profile_read()["prec_apply"]
        ctx.set_profile(False)
        M.close()
        acc[bits]["in_solve_us"] = ms / max(calls, 1) * 1e3
    for bits in (64, 32):
        a = acc[bits]
        say("bjacobi-ilu%d %2d bits  iterations %3d%s  create + solve ms %s   application inside the solve %.1f us" %
            (fill, bits, a["its"], "" if a["conv"] else " (NOT converged)", stats(a["total"]), a["in_solve_us"]))
    say("bjacobi-ilu%d 32 / 64: create + solve %.3f  (%+.2f ms)" %
        (fill, med(acc[32]["total"]) / med(acc[64]["total"]), med(acc[32]["total"]) - med(acc[64]["total"])))


say("# scripts/time_ilu_f32.py: %d^3 TGV pressure system, %d rows, block ILU on the library's bricks, value_bits 64 and 32" % (n, N))
say("# alternated repetition by repetition in one process; median (min - max)")
say("# device: %s" % torch.cuda.get_device_name(0))
say()
say("# one application, us: HIP events around the solve kernel alone, 30 repetitions.  bytes = chunks in use x (64 x (8|4 + 2) + 1)")
say("# + rows x 28: the stream goes from 10 to 6 B per entry")
for fill in (0, 1):
    ts, by = apply_pair_us(fill)
    m64, m32 = med(ts[64]), med(ts[32])
    (b64, i64), (b32, _) = by[64], by[32]
    say("bjacobi-ilu%d  blocks %d  factor entries %d  chunks in use %d (capacity %d)" %
        (fill, i64["nblocks"], i64["factor_nnz"], i64["stream_chunks"], i64["stream_capacity"]))
    say("    64 bits %s us  %6.1f MB  %5.0f GB/s" % (stats(ts[64], "%.1f"), b64 / 1e6, b64 / m64 / 1e3))
    say("    32 bits %s us  %6.1f MB  %5.0f GB/s" % (stats(ts[32], "%.1f"), b32 / 1e6, b32 / m32 / 1e3))
    say("    32 / 64: time %.3f  bytes %.3f" % (m32 / m64, b32 / b64))
say()
say("# the create call, ms (create + synchronise, host clock, %d repetitions): the rounding pass and its host check are in the 32-bit figure" % (4 * REPS))
for fill in (0, 1):
    ts = create_pair_ms(fill, 4 * REPS)
    say("bjacobi-ilu%d  64 bits %s   32 bits %s   the float plane: %+.3f ms" %
        (fill, stats(ts[64], "%.3f"), stats(ts[32], "%.3f"), med(ts[32]) - med(ts[64])))
say()
say("# a solve with the benchmark's settings (FGMRES(50), preconditioner created inside the timed region), %d repetitions" % REPS)
for fill in (0, 1):
    solve_pair(fill)
say()
A.close()
ctx.close()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
