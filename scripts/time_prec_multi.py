"""One preconditioner applied to K = 2, 3, 4 vectors per sweep (isph_prec_apply_multi: cheb_apply_multi, amg_apply_multi)
against K single applications -- the route every caller took before the one-sweep forms existed, and still takes under
ISPH_PREC_MULTI_SINGLE=1 -- on the bench system (100^3 TGV: the pressure system for the applications, the Helmholtz system
with its three right-hand sides for the lockstep solve).  The two routes are ALTERNATED repetition by repetition in this
one process; one warm-up round, then the repeats: median (min - max).

  * one application to K vectors, device events, us: chebyshev3 and the SA-AMG with Chebyshev degree 2, matrix values of
    64 and 32 bits;
  * per level of that hierarchy, one Chebyshev step with a product on the level's operator: the operator A_l is exported
    and set up as a matrix of its own (so it is swept with 16-bit columns where they exist; inside the hierarchy levels
    >= 1 have 32-bit columns), (apply of degree 9 - apply of degree 1) / 8 of one repetition is one step, the K-vector
    step against K single steps, beside their algorithmic bytes: the matrix stream (value 8 B + column 2|4 B per stored
    entry) once for the K-vector step and K times for the singles; gathers (8 B per stored entry) and the vector traffic
    (b, w in, w out, y in, y out; dinv once | K times) K-fold in both;
  * the 3-RHS Helmholtz lockstep solve (FGMRES(50), tol 1e-8), preconditioner created with and without
    ISPH_PREC_MULTI_SINGLE=1, create excluded, host clock around calls that end in a device synchronise, ms;
  * the pool's peak of live bytes over such a solve.

    python scripts/time_prec_multi.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
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
APPLY_REPS = 30
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prec_multi_100cubed.txt")
lines = []
KS = (2, 3, 4)


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
vfrac = vf[own].contiguous()
A, b = hip.assemble_poisson(ctx, dp, colmap, spec.dt, rho, vs, vfrac=vfrac)
N = n ** 3
nv = torch.full((N,), 1.0 / np.sqrt(float(N)), dtype=torch.float64, device=dev)


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts, fmt="%8.1f (%.1f - %.1f)"):
    return fmt % (med(ts), min(ts), max(ts))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def amg(M_of, bits=64, sweeps=2, nullvec=None, **kw):
    return hip.PrecondAMG(ctx, M_of, nullvec=nullvec,
                          params=hip.AmgParams(theta=0.0, smoother=2, sweeps=sweeps, cheb_ratio=20.0, cheb_value_bits=bits, **kw))


def singles(M, R, Z, K, ld):
    for k in range(K):
        M.apply(R[k * ld:(k + 1) * ld], Z[k * ld:(k + 1) * ld])


def apply_pair(M, rows):
    """us of one application to K vectors: K single applications, then apply_multi, alternated"""
    R = torch.randn(4 * rows, dtype=torch.float64, device=dev)
    Z, Z1 = torch.zeros_like(R), torch.zeros_like(R)
    out = {}
    for K in KS:
        assert M.multi_path(K) == 1
        for _ in range(3):
            singles(M, R, Z1, K, rows)
            M.apply_multi(R, Z, nvec=K, lda=rows)
        torch.cuda.synchronize()
        assert torch.equal(Z[:K * rows], Z1[:K * rows]), "the K-vector application differs from K single ones"
        ts, tm = [], []
        for _ in range(APPLY_REPS):
            ts.append(event_ms(lambda: singles(M, R, Z1, K, rows)) * 1e3)
            tm.append(event_ms(lambda: M.apply_multi(R, Z, nvec=K, lda=rows)) * 1e3)
        out[K] = (ts, tm)
    return out


say("# scripts/time_prec_multi.py: %d^3 TGV, %d rows; K vectors per sweep (apply_multi) against K single applications (the route of" % (n, N))
say("# ISPH_PREC_MULTI_SINGLE=1), alternated repetition by repetition, 3 warm-ups + %d repeats per line: median (min - max)" % APPLY_REPS)
say("# device: %s" % torch.cuda.get_device_name(0))

# ---- one application ----------------------------------------------------------------------------------------------------
say()
say("# one application to K vectors, us, device events (pressure system, 16-bit columns on the fine level)")
for bits in (64, 32):
    for label, make in (("chebyshev3", lambda: hip.PrecondChebyshev(ctx, A, degree=3, value_bits=bits)),
                        ("sa-amg chebyshev degree 2", lambda: amg(A, bits, nullvec=nv))):
        M = make()
        res = apply_pair(M, N)
        for K in KS:
            ts, tm = res[K]
            say("%-26s value bits %2d  K %d  singles %s   multi %s   multi / singles %.3f" %
                (label, bits, K, stats(ts), stats(tm), med(tm) / med(ts)))
        M.close()

# ---- per level ------------------------------------------------------------------------------------------------------------
say()
say("# per level of the SA-AMG hierarchy: one Chebyshev step with a product on A_l (exported, set up as its own matrix), us;")
say("# (apply of degree 9 - apply of degree 1) / 8 of one repetition; algorithmic MB: matrix stream once | K times + K x (gathers + vectors)")
Mh = amg(A, 64, nullvec=nv)
level_mats = []
for l in range(Mh.levels):
    rows = Mh.level_info(l)["rows"]
    if l == 0:
        level_mats.append((rows, A))
    else:
        rp, ci, v = Mh.export(l, "A")
        keep = np.diff(rp) > 0
        if not keep.all() or rows < 2:            # (a level with empty rows has no polynomial of its own outside the hierarchy)
            say("level %d  rows %d: skipped (rows without entries)" % (l, rows))
            continue
        level_mats.append((rows, hip.Matrix.from_csr(ctx, rp, ci, v)))
say("# levels: %s" % [Mh.level_info(l)["rows"] for l in range(Mh.levels)])
Mh.close()
for rows, Al in level_mats:
    info = Al.info()
    cb = Al.column_bits() // 8
    try:
        M9, M1 = hip.PrecondChebyshev(ctx, Al, degree=9), hip.PrecondChebyshev(ctx, Al, degree=1)
    except hip.IsphError as e:
        say("rows %d: skipped (%s)" % (rows, e))
        continue
    R = torch.randn(4 * rows, dtype=torch.float64, device=dev)
    Z = torch.zeros_like(R)
    for K in KS:
        for _ in range(3):
            for M in (M9, M1):
                singles(M, R, Z, K, rows)
                M.apply_multi(R, Z, nvec=K, lda=rows)
        ts, tm = [], []
        for _ in range(APPLY_REPS):
            s9 = event_ms(lambda: singles(M9, R, Z, K, rows)); s1 = event_ms(lambda: singles(M1, R, Z, K, rows))
            m9 = event_ms(lambda: M9.apply_multi(R, Z, nvec=K, lda=rows)); m1 = event_ms(lambda: M1.apply_multi(R, Z, nvec=K, lda=rows))
            ts.append((s9 - s1) / 8.0 * 1e3)
            tm.append((m9 - m1) / 8.0 * 1e3)
        stream = info["stored"] * (8 + cb)
        gath = info["stored"] * 8
        mb_s = (K * stream + K * gath + K * rows * 6 * 8) / 1e6
        mb_m = (stream + K * gath + rows * (5 * K + 1) * 8) / 1e6
        say("rows %8d  stored %10d  column bits %2d  K %d  K single steps %s   multi step %s   multi / singles %.3f   MB %7.1f | %7.1f (%.3f)" %
            (rows, info["stored"], 8 * cb, K, stats(ts), stats(tm), med(tm) / med(ts), mb_s, mb_m, mb_m / mb_s))
    M9.close(); M1.close()
    if Al is not A:
        Al.close()

# ---- the lockstep solve ---------------------------------------------------------------------------------------------------
say()
say("# the 3-RHS Helmholtz lockstep solve (theta 0.5, FGMRES(50), tol 1e-8, guess: the current velocity), ms, host clock around a")
say("# call that ends in a device synchronise; preconditioner created once per route (create not timed); %d repeats alternated" % REPS)
nu = torch.from_numpy(np.ascontiguousarray(parts["nu"])).to(dev) if "nu" in parts else torch.full((parts["nall"],), 0.01, dtype=torch.float64, device=dev)
pall = torch.zeros(parts["nall"], dtype=torch.float64, device=dev)
H, bh = hip.assemble_helmholtz(ctx, dp, colmap, spec.dt, 0.5, nu, rho, pall, torch.zeros_like(vs), np.zeros(3), vs, vfrac=vfrac)
x0 = torch.cat([vs[:N, 0], vs[:N, 1], vs[:N, 2]]).contiguous()
prm = hip.SolverParams(tol=1e-8)
for label, make in (("chebyshev3", lambda: hip.PrecondChebyshev(ctx, H, degree=3)),
                    ("sa-amg chebyshev degree 2", lambda: amg(H, 64))):
    Mm = make()
    os.environ["ISPH_PREC_MULTI_SINGLE"] = "1"
    Ms = make()
    del os.environ["ISPH_PREC_MULTI_SINGLE"]
    assert Mm.multi_path(3) == 1 and Ms.multi_path(3) == 0
    acc = {0: [], 1: []}
    its, xs, peak, grown = {}, {}, {}, {}
    for rep_ in range(REPS + 1):
        for route, M in ((0, Ms), (1, Mm)):
            bw, x = bh.clone(), x0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf = hip.solve(ctx, H, bw, x, prec=M, singular=False, nvec=3, lda=N, params=prm)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep_ > 0:
                acc[route].append((t1 - t0) * 1e3)
            its[route], xs[route] = (inf.iters, inf.converged), x
    assert torch.equal(xs[0], xs[1]) and its[0] == its[1], "the lockstep solve differs between the two routes"
    Mm.close(); Ms.close()
    # the pool: one object alive at a time; peak of live bytes over the solve, and what the first application to K vectors takes
    for route in (0, 1):
        if route == 0:
            os.environ["ISPH_PREC_MULTI_SINGLE"] = "1"
        M = make()
        os.environ.pop("ISPH_PREC_MULTI_SINGLE", None)
        bw, x = bh.clone(), x0.clone()
        torch.cuda.synchronize()
        hip.pool_info(reset_peak=True)
        hip.solve(ctx, H, bw, x, prec=M, singular=False, nvec=3, lda=N, params=prm)
        torch.cuda.synchronize()
        peak[route] = hip.pool_info()["peak_live"]
        M.close()
    M = make()
    R = torch.randn(4 * N, dtype=torch.float64, device=dev)
    Z = torch.zeros_like(R)
    live = hip.pool_info()["live"]
    for K in KS:
        M.apply_multi(R, Z, nvec=K, lda=N)
        torch.cuda.synchronize()
        grown[K] = hip.pool_info()["live"] - live
    M.close()
    say("%-26s iterations %3d%s  singles %s   multi %s   multi / singles %.3f" %
        (label, its[1][0], "" if its[1][1] else " (NOT converged)", stats(acc[0], "%8.2f (%.2f - %.2f)"),
         stats(acc[1], "%8.2f (%.2f - %.2f)"), med(acc[1]) / med(acc[0])))
    say("%-26s pool peak over the solve, MB: singles %.1f   multi %.1f   (%+.1f);   K-fold work vectors after the first application to" %
        (label, peak[0] / 1e6, peak[1] / 1e6, (peak[1] - peak[0]) / 1e6))
    say("%-26s K = 2, 3, 4 vectors, MB of live pool bytes: %s" % ("", ", ".join("%.1f" % (grown[K] / 1e6) for K in KS)))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
