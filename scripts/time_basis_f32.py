"""basis_bits = 32 of GMRES against 64 on the bench matrix: the 3-D TGV pressure system (ISPH_NCELL^3 rows) on the
library's bricks with the benchmark's settings (FGMRES(50), DGKS, tol 1e-8, singular), ONE process, the two widths
alternated repetition by repetition.  Per preconditioner ("bjacobi-ilu0" on the library's bricks, "jacobi",
"chebyshev3"), built once outside the timed region:

  * the whole solve, ms (host clock around isph_solve, synchronised): one warm-up, then ISPH_REPS repetitions per
    width, median (min - max); iterations, restarts, residual_restarts and rel_res_explicit of the solve;
  * the three Gram-Schmidt sweeps of a DGKS step, us per launch: profile classes [2] k_multi_dot, [3] k_multi_axpy_dot,
    [4] k_multi_axpy_norm of isph_ctx_profile_read over one more, untimed, profiled solve per width and repetition,
    beside their algorithmic bytes per launch at the mean number of basis vectors nk of that solve --
        multi_dot       N (s nk + 8 ceil(nk / 16))             V once, w once per batch of 16
        multi_axpy_dot  N (s nk + 16)                          V once, w read and written
        multi_axpy_norm N (s nk p + 8 + (p ? 8 : 0) + o)       V and the write of w only when the second pass runs
                                                               (share p of the steps); o = the new vector: 8, or 4 + 8
    with s = 8 | 4 bytes per basis entry (a singular system at 64 bits carries the null vector as one more column);
  * the pool's peak above the matrix and the preconditioner during one solve in a fresh context.
The yardstick of the 32-bit leg is the 64-bit leg of the same run.  No speed-up is assumed anywhere: the only figures
known in advance are the byte ratios.

    python scripts/time_basis_f32.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
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
spec = workload.TGVSpec(dim=3, ncell=(n, n, n), brick=(n, n, n), mode=workload.ADVECT)
parts = workload.make_tgv(spec)
N, M_BLOCKS = n ** 3, 50


def assemble(ctx):
    dp = dict(parts)
    for k in ("x", "type", "neigh_ptr", "neigh_idx"):
        dp[k] = torch.from_numpy(np.ascontiguousarray(parts[k])).to(dev)
    own = torch.from_numpy(parts["owner_index"].astype(np.int64)).to(dev)
    colmap = own.to(torch.int32).contiguous()
    rho = torch.from_numpy(parts["rho"]).to(dev)
    vs = torch.from_numpy(np.ascontiguousarray(parts["v"])).to(dev)
    vf = hip.compute_volumes(ctx, dp, colmap)
    return hip.assemble_poisson(ctx, dp, colmap, spec.dt, rho, vs, vfrac=vf[own].contiguous())


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts, fmt="%.2f"):
    ts = sorted(ts)
    return (fmt + " (" + fmt + " - " + fmt + ")") % (ts[len(ts) // 2], ts[0], ts[-1])


def sweep_bytes(bits, nk, p):
    """algorithmic bytes per launch of the three sweeps at nk basis vectors, second-pass share p"""
    s = bits // 8
    new = 8 if bits == 64 else 4 + 8
    return (N * (s * nk + 8 * np.ceil(nk / 16.0)), N * (s * nk + 16), N * (s * nk * p + 8 + 8 * p + new))


ctx = hip.Context(0, stream=st.cuda_stream, ordering="bricks")
A, b = assemble(ctx)
x = torch.zeros(N, dtype=torch.float64, device=dev)
bw = b.clone()
CLASSES = ("multi_dot", "multi_axpy_dot", "multi_axpy_norm")


def solve_pair(prec):
    M = hip.Precond(ctx, A, prec, 0)
    acc = {bits: dict(total=[], info=None, us={c: [] for c in CLASSES}, nk=0.0, p=0.0) for bits in (64, 32)}
    for rep_ in range(REPS + 1):
        for bits in (64, 32):
            prm = hip.SolverParams(basis_bits=bits)      # bench.py's otherwise
            bw.copy_(b); x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            a = acc[bits]
            if rep_ > 0:
                a["total"].append((t1 - t0) * 1e3)
            a["info"] = inf
            # the same solve once more, profiled and untimed
            bw.copy_(b); x.zero_()
            ctx.set_profile(True)
            ctx.profile_read()
            hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            prof = ctx.profile_read()
            ctx.set_profile(False)
            if rep_ > 0:
                for c in CLASSES:
                    a["us"][c].append(prof[c][0] / max(prof[c][1], 1) * 1e3)
    for bits in (64, 32):
        a, inf = acc[bits], acc[bits]["info"]
        # basis vectors per Gram-Schmidt step, averaged over the solve: the cycles' lengths follow from iters, restarts
        # and residual_restarts only approximately, so the mean takes full cycles of 50 and one remainder
        its, full = inf.iters, inf.iters // M_BLOCKS
        lens = [M_BLOCKS] * full + ([its - full * M_BLOCKS] if its % M_BLOCKS else [])
        nk = sum(sum(range(1, L + 1)) for L in lens) / float(max(its, 1)) + (1.0 if bits == 64 else 0.0)
        p = inf.reorth / float(max(its, 1))
        a["nk"], a["p"] = nk, p
        say("%-13s %2d bits  iterations %3d restarts %d residual_restarts %d%s  rel_res_explicit %.3e  solve ms %s" %
            (prec, bits, inf.iters, inf.restarts, inf.residual_restarts, "" if inf.converged else " (NOT converged)",
             inf.rel_res_explicit, stats(a["total"])))
        by = sweep_bytes(bits, nk, p)
        for c, nb in zip(CLASSES, by):
            m = med(a["us"][c])
            say("    %-16s %s us per launch   %6.1f MB at nk %.1f (second pass in %.0f %% of the steps)  %5.0f GB/s" %
                (c, stats(a["us"][c], "%.1f"), nb / 1e6, nk, 100.0 * p, nb / m / 1e3))
    say("%-13s 32 / 64: solve %.3f (%+.2f ms)" % (prec, med(acc[32]["total"]) / med(acc[64]["total"]),
                                                  med(acc[32]["total"]) - med(acc[64]["total"])))
    for c, b64, b32 in zip(CLASSES, sweep_bytes(64, acc[64]["nk"], acc[64]["p"]), sweep_bytes(32, acc[32]["nk"], acc[32]["p"])):
        say("    %-16s 32 / 64: time %.3f  bytes %.3f" % (c, med(acc[32]["us"][c]) / med(acc[64]["us"][c]), b32 / b64))
    M.close()


say("# scripts/time_basis_f32.py: %d^3 TGV pressure system, %d rows, FGMRES(50) DGKS tol 1e-8, basis_bits 64 and 32" % (n, N))
say("# alternated repetition by repetition in one process; %d repetitions after one warm-up; median (min - max)" % REPS)
say("# device: %s" % torch.cuda.get_device_name(0))
say()
for prec in ("bjacobi-ilu0", "jacobi", "chebyshev3"):
    solve_pair(prec)
    say()
A.close()
ctx.close()

say("# pool peak during one solve above the matrix and the preconditioner (fresh context per width, jacobi)")
ld = (N + 63) // 64 * 64
for bits in (64, 32):
    c2 = hip.Context(0, stream=st.cuda_stream, ordering="bricks")
    A2, b2 = assemble(c2)
    M2 = hip.Precond(c2, A2, "jacobi", 0)
    x2 = torch.zeros(N, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip.pool_trim()
    base = hip.pool_info(reset_peak=True)["live"]
    hip.solve(c2, A2, b2.clone(), x2, prec=M2, singular=True, params=hip.SolverParams(basis_bits=bits))
    peak = hip.pool_info()["peak_live"] - base
    basis = 8 * ld * (M_BLOCKS + 2) if bits == 64 else 4 * ld * (M_BLOCKS + 1) + 8 * ld
    say("%2d bits  peak %7.1f MB   of which the basis %7.1f MB, Z %7.1f MB" % (bits, peak / 1e6, basis / 1e6, 8 * ld * M_BLOCKS / 1e6))
    M2.close(); A2.close(); c2.close()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
