"""The Chebyshev smoother / preconditioner on the bench system (100^3 TGV pressure system of bench.py, tol 1e-8, the
preconditioner rebuilt for every solve): iterations, set-up ms and solve ms of block ILU(0), SA-AMG with the Gauss-Seidel
smoothers 0 and 1, SA-AMG with Chebyshev of degree 1..4 at ratio 20 and 30, stand-alone chebyshev<d> beside point Jacobi;
then the fused step (k_sell_cheby_step) against the unfused composition (ISPH_CHEB_UNFUSED=1: SpMV + vector update),
level by level, from device events.  One warm-up and ISPH_REPS timed repeats per line: median (min - max).

Last section: value_bits = 32 (the polynomial of fl32(A), sweeps over a float plane of the values) against 64, the two
forms ALTERNATED repetition by repetition in this one process: the fused step per level with the bytes it moves,
chebyshev3 and the SA-AMG with Chebyshev degree 2 (set-up, solve, iterations), the set-up cost of the float plane, and
one application of each form against the other.  ISPH_CHEB_SECTIONS=f32 prints only that section and the block ILU(0)
and point Jacobi lines beside it.

    python scripts/time_chebyshev.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7, ISPH_CHEB_SECTIONS=all|f32)
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
ALL = os.environ.get("ISPH_CHEB_SECTIONS", "all") != "f32"
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


def stats(ts):
    ts = sorted(ts)
    return "%8.2f (%.2f - %.2f)" % (ts[len(ts) // 2], ts[0], ts[-1])


def solve_line(label, make, solver_params=prm):
    setup, solve, its, conv = [], [], 0, 1
    for r in range(REPS + 1):
        bw.copy_(b); x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = make()
        ctx.sync()
        t1 = time.perf_counter()
        inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=solver_params)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        M.close()
        if r > 0:
            setup.append((t1 - t0) * 1e3); solve.append((t2 - t1) * 1e3)
        its, conv = inf.iters, conv and inf.converged
    say("%-44s iterations %3d%s  set-up ms %s  solve ms %s  sum %7.2f" %
        (label, its, "" if conv else " (NOT converged)", stats(setup), stats(solve), sorted(setup)[len(setup) // 2] + sorted(solve)[len(solve) // 2]))


say("# scripts/time_chebyshev.py: %d^3 TGV pressure system, %d rows, FGMRES(50) tol 1e-8, preconditioner rebuilt per solve," % (n, N))
say("# 1 warm-up + %d repeats per line, host clock around calls that end in a device synchronise: median (min - max)" % REPS)
say("# device: %s" % torch.cuda.get_device_name(0))
solve_line("block ILU(0), library bricks", lambda: hip.Precond(ctx, A, "bjacobi-ilu0", 0))
for sm in (0, 1) if ALL else ():
    solve_line("SA-AMG Gauss-Seidel smoother %d, 1 sweep" % sm,
               lambda: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(block=512, theta=0.0, smoother=sm)))
for ratio in (20.0, 30.0) if ALL else ():
    for d in (1, 2, 3, 4):
        solve_line("SA-AMG Chebyshev degree %d ratio %2.0f" % (d, ratio),
                   lambda: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=d, cheb_ratio=ratio)))
solve_line("point Jacobi", lambda: hip.Precond(ctx, A, "jacobi", 0))
for d in (1, 2, 3, 4) if ALL else ():
    solve_line("chebyshev%d (ratio 30)" % d, lambda: hip.Precond(ctx, A, "chebyshev%d" % d, 0))
if ALL:
    solve_line("Block CG + SA-AMG Chebyshev degree 2 ratio 20",
               lambda: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2, cheb_ratio=20.0)),
               hip.SolverParams(solver_type=1, tol=1e-8))


# ---- the fused step against the unfused composition, level by level --------------------------------------------------
def apply_ms(M, r, z, reps=30):
    for _ in range(3):
        M.apply(r, z)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        M.apply(r, z)
        e1.record(st)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)


def step_us(Am, nrow, unfused):
    """time of one step with a product = (apply at degree 9 - apply at degree 1) / 8, device events"""
    if unfused:
        os.environ["ISPH_CHEB_UNFUSED"] = "1"
    M9, M1 = hip.PrecondChebyshev(ctx, Am, degree=9), hip.PrecondChebyshev(ctx, Am, degree=1)
    os.environ.pop("ISPH_CHEB_UNFUSED", None)
    r = torch.randn(nrow, dtype=torch.float64, device=dev)
    z = torch.empty_like(r)
    t9, t1 = apply_ms(M9, r, z), apply_ms(M1, r, z)
    M9.close(); M1.close()
    med = lambda t: t[len(t) // 2]
    return (med(t9) - med(t1)) / 8.0 * 1e3, (t9[0] - med(t1)) / 8.0 * 1e3, (t9[-1] - med(t1)) / 8.0 * 1e3


say()
say("# one Chebyshev step with a matrix product, us: (apply of degree 9 - apply of degree 1) / 8, 30 repeats, device events;")
say("# level l > 0: the level operator exported from the hierarchy and applied as a matrix of its own (16-bit columns where")
say("# they exist; inside the cycle the coarse operators keep 32-bit columns)")
G = hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2))
mats = [(A, N, A.info()["nnz"])]
for l in range(1, G.levels):
    rp, ci, v = G.export(l, "A")
    mats.append((hip.Matrix.from_csr(ctx, rp, ci, v), len(rp) - 1, len(v)))
for l, (Am, nrow, nnz) in enumerate(mats if ALL else []):
    try:
        f, u = step_us(Am, nrow, False), step_us(Am, nrow, True)
    except hip.IsphError as e:      # (a coarse operator with an empty row has no stand-alone polynomial)
        say("level %d  rows %8d  entries %10d   not measured: %s" % (l, nrow, nnz, e))
        continue
    say("level %d  rows %8d  entries %10d   fused %8.1f (%.1f - %.1f)   unfused %8.1f (%.1f - %.1f)   fused / unfused %.3f" %
        (l, nrow, nnz, f[0], f[1], f[2], u[0], u[1], u[2], f[0] / u[0]))
r = torch.randn(N, dtype=torch.float64, device=dev)
z = torch.empty_like(r)
if ALL:
    say()
    say("# one V cycle (all levels, Chebyshev degree 2, ratio 20), ms, 30 repeats, device events")
    tf = apply_ms(G, r, z)
    os.environ["ISPH_CHEB_UNFUSED"] = "1"
    Gu = hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2))
    os.environ.pop("ISPH_CHEB_UNFUSED", None)
    tu = apply_ms(Gu, r, z)
    say("fused %.3f (%.3f - %.3f)   unfused %.3f (%.3f - %.3f)   levels %s" %
        (tf[len(tf) // 2], tf[0], tf[-1], tu[len(tu) // 2], tu[0], tu[-1], [G.level_info(l)["rows"] for l in range(G.levels)]))
    Gu.close()
    G0 = hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(block=512, theta=0.0, smoother=0))
    t0 = apply_ms(G0, r, z)
    say("the symmetric Gauss-Seidel cycle (smoother 0, 1 sweep) beside it: %.3f (%.3f - %.3f)" % (t0[len(t0) // 2], t0[0], t0[-1]))
    G0.close()


# ---- value_bits = 32 against 64, alternated in this process -----------------------------------------------------------
def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def step_pair_us(Am, nrow, reps=30):
    """one step with a product, us, for 64 and 32 bits: (apply of degree 9 - apply of degree 1) / 8 of the same repetition,
    the four applications of a repetition back to back, 64 and 32 alternating"""
    Ms = {bits: (hip.PrecondChebyshev(ctx, Am, degree=9, value_bits=bits), hip.PrecondChebyshev(ctx, Am, degree=1, value_bits=bits))
          for bits in (64, 32)}
    rr = torch.randn(nrow, dtype=torch.float64, device=dev)
    zz = torch.empty_like(rr)
    for _ in range(3):
        for bits in (64, 32):
            for M in Ms[bits]:
                M.apply(rr, zz)
    ts = {64: [], 32: []}
    for _ in range(reps):
        for bits in (64, 32):
            t9 = event_ms(lambda: Ms[bits][0].apply(rr, zz))
            t1 = event_ms(lambda: Ms[bits][1].apply(rr, zz))
            ts[bits].append((t9 - t1) / 8.0 * 1e3)
    for bits in (64, 32):
        for M in Ms[bits]:
            M.close()
    return ts


def step_bytes(Am, nrow, bits):
    """algorithmic bytes of one fused step: per stored entry the value (8 or 4 B) and the column (2 B windowed, 4 B
    otherwise); per row b, dinv, w in, w out, y in (every y counted once: gathers beyond that are cache hits), y out
    = 6 x 8 B; per slice of 64 rows two 8-B offsets and, with 16-bit columns, the 64 x 4 B window table"""
    i, cb = Am.info(), Am.column_bits()
    per_entry = bits // 8 + cb // 8
    return i["stored"] * per_entry + nrow * 48 + i["nslices"] * (16 + (256 if cb == 16 else 0)), per_entry, cb


def solve_pair(label, make):
    """make(bits); 64 and 32 alternated, one warm-up each"""
    acc = {bits: dict(setup=[], solve=[], its=0, conv=1) for bits in (64, 32)}
    for rep_ in range(REPS + 1):
        for bits in (64, 32):
            bw.copy_(b); x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = make(bits)
            ctx.sync()
            t1 = time.perf_counter()
            inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            M.close()
            a = acc[bits]
            if rep_ > 0:
                a["setup"].append((t1 - t0) * 1e3); a["solve"].append((t2 - t1) * 1e3)
            a["its"], a["conv"] = inf.iters, a["conv"] and inf.converged
    for bits in (64, 32):
        a = acc[bits]
        say("%-36s %2d bits  iterations %3d%s  set-up ms %s  solve ms %s  sum %7.2f" %
            (label, bits, a["its"], "" if a["conv"] else " (NOT converged)", stats(a["setup"]), stats(a["solve"]),
             med(a["setup"]) + med(a["solve"])))
    say("%-36s 32 / 64: solve %.3f  set-up %.3f  (float plane: %+.2f ms of set-up)" %
        (label, med(acc[32]["solve"]) / med(acc[64]["solve"]), med(acc[32]["setup"]) / med(acc[64]["setup"]),
         med(acc[32]["setup"]) - med(acc[64]["setup"])))


say()
say("# value_bits = 32 (sweeps over fl32 of the values, 4 B each) against 64, alternated repetition by repetition")
say("# bytes of one fused step = stored x (value 8|4 + column 2|4) + rows x 48 (b, dinv, w in, w out, y in once, y out)")
say("#                           + slices x (16 + 256 with 16-bit columns): 10 -> 6 or 12 -> 8 B per stored entry")
say("# step us = (apply of degree 9 - apply of degree 1) / 8 of one repetition, 30 repetitions, device events: median (min - max)")
for l, (Am, nrow, nnz) in enumerate(mats):
    try:
        ts = step_pair_us(Am, nrow)
    except hip.IsphError as e:      # (a coarse operator with an empty row has no stand-alone polynomial)
        say("level %d  rows %8d  entries %10d   not measured: %s" % (l, nrow, nnz, e))
        continue
    by64, pe64, cb = step_bytes(Am, nrow, 64)
    by32, pe32, _ = step_bytes(Am, nrow, 32)
    m64, m32 = med(ts[64]), med(ts[32])
    say("level %d  rows %8d  stored %10d  %2d-bit columns   64 bits %8.1f (%.1f - %.1f) us  %6.1f MB  %5.0f GB/s   "
        "32 bits %8.1f (%.1f - %.1f) us  %6.1f MB  %5.0f GB/s   32 / 64: time %.3f  bytes %.3f  (%d -> %d B per entry)" %
        (l, nrow, Am.info()["stored"], cb, m64, min(ts[64]), max(ts[64]), by64 / 1e6, by64 / m64 / 1e3,
         m32, min(ts[32]), max(ts[32]), by32 / 1e6, by32 / m32 / 1e3, m32 / m64, by32 / by64, pe64, pe32))
say()
solve_pair("chebyshev3 (ratio 30)", lambda bits: hip.PrecondChebyshev(ctx, A, degree=3, ratio=30.0, value_bits=bits))
solve_pair("SA-AMG Chebyshev degree 2 ratio 20",
           lambda bits: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2, cheb_ratio=20.0,
                                                                                cheb_value_bits=bits)))
say()
say("# set-up of the stand-alone polynomial alone (create + synchronise, host clock, %d repetitions alternated), ms" % (4 * REPS))
tset = {64: [], 32: []}
for rep_ in range(4 * REPS + 1):
    for bits in (64, 32):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = hip.PrecondChebyshev(ctx, A, degree=3, value_bits=bits)
        ctx.sync()
        t1 = time.perf_counter()
        M.close()
        if rep_ > 0:
            tset[bits].append((t1 - t0) * 1e3)
say("64 bits %s   32 bits %s   the float plane (%.1f MB written, %.1f MB read): %+.3f ms" %
    (stats(tset[64]), stats(tset[32]), A.info()["stored"] * 4 / 1e6, A.info()["stored"] * 8 / 1e6, med(tset[32]) - med(tset[64])))
say()
say("# one application of each form against the other (expected ~1e-8: the values differ by 2^-24 relative), max norm")
for label, make in (("chebyshev3", lambda bits: hip.PrecondChebyshev(ctx, A, degree=3, value_bits=bits)),
                    ("SA-AMG Chebyshev degree 2 cycle",
                     lambda bits: hip.PrecondAMG(ctx, A, nullvec=nv, params=hip.AmgParams(theta=0.0, smoother=2, sweeps=2,
                                                                                          cheb_value_bits=bits)))):
    M64, M32 = make(64), make(32)
    z64, z32 = torch.empty_like(r), torch.empty_like(r)
    M64.apply(r, z64); M32.apply(r, z32)
    torch.cuda.synchronize()
    say("%-34s max|z32 - z64| / max|z64| = %.2e   cycle / application ms: 64 bits %.3f  32 bits %.3f" %
        (label, float((z32 - z64).abs().max() / z64.abs().max()), med(apply_ms(M64, r, z64)), med(apply_ms(M32, r, z32))))
    M64.close(); M32.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
