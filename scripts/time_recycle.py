"""Recycling GMRES with the recycle space carried from one solve to the next (isph_solve_recycle) on the bench system:
consecutive pressure systems of the 100^3 TGV step workload (the particles advected by advect_dt = dt (1 + 0.1 s),
s = 0..3, like the sequences of tests/gcrodr_recycle_reference.py), solved in turn by

  * the default solver, flexible GMRES(50),
  * GCRO-DR(50, 10) without a handle (solver_type 2 as it always was: every solve starts from nothing),
  * GCRO-DR(50, 10) with a handle,

with jacobi, chebyshev3 and bjacobi-ilu0, the three routes ALTERNATED system by system in this one process; one warm-up
round, then the repeats: median (min - max).  Per solve: iterations, the operator applications that rebuilt C, and
preconditioner create + solve in ms (host clock around calls that end in a device synchronise); the bytes the handle holds.

Then the two kernels of the handle path, k_tall_gemm and k_block_gram, against the per-column launches they replace
(isph_dense_tall_gemm mode 3, isph_dense_block_gram per_column) on blocks of the sizes of a restart, beside their
algorithmic bytes; and the 3-RHS Helmholtz solve: lockstep FGMRES(50), GCRO-DR without a handle, and GCRO-DR with a
handle whose columns share the space.

    python scripts/time_recycle.py [output file]          (ISPH_NCELL=100, ISPH_REPS=3)
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
REPS = int(os.environ.get("ISPH_REPS", "3"))
STEPS = 4
M_BLOCKS, K_REC = 50, 10
KERNEL_REPS = 10
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "recycle_100cubed.txt")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(t):
    t = sorted(t)
    return t[len(t) // 2]


def stats(ts, fmt="%8.2f (%.2f - %.2f)"):
    return fmt % (med(ts), min(ts), max(ts))


dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = hip.Context(0, stream=st.cuda_stream, ordering="bricks")
N = n ** 3
base = workload.TGVSpec(dim=3, ncell=(n, n, n), brick=(n, n, n), mode=workload.ADVECT)

say("# scripts/time_recycle.py: %d^3 TGV, %d rows; %d consecutive pressure systems (advect_dt = dt (1 + 0.1 s)); tol 1e-8;" % (n, N, STEPS))
say("# routes alternated system by system, 1 warm-up round + %d repeats: median (min - max)" % REPS)
say("# device: %s" % torch.cuda.get_device_name(0))


def assemble(s, helmholtz=False):
    spec = workload.TGVSpec(dim=3, ncell=(n, n, n), brick=(n, n, n), mode=workload.ADVECT, advect_dt=base.dt * (1.0 + 0.1 * s))
    parts = workload.make_tgv(spec)
    dp = dict(parts)
    for k in ("x", "type", "neigh_ptr", "neigh_idx"):
        dp[k] = torch.from_numpy(np.ascontiguousarray(parts[k])).to(dev)
    own = torch.from_numpy(parts["owner_index"].astype(np.int64)).to(dev)
    colmap = own.to(torch.int32).contiguous()
    rho = torch.from_numpy(parts["rho"]).to(dev)
    vs = torch.from_numpy(np.ascontiguousarray(parts["v"])).to(dev)
    vfrac = hip.compute_volumes(ctx, dp, colmap)[own].contiguous()
    if not helmholtz:
        return hip.assemble_poisson(ctx, dp, colmap, spec.dt, rho, vs, vfrac=vfrac)
    nu = torch.from_numpy(np.ascontiguousarray(parts["nu"])).to(dev) if "nu" in parts else torch.full((parts["nall"],), 0.01, dtype=torch.float64, device=dev)
    pall = torch.zeros(parts["nall"], dtype=torch.float64, device=dev)
    H, bh = hip.assemble_helmholtz(ctx, dp, colmap, spec.dt, 0.5, nu, rho, pall, torch.zeros_like(vs), np.zeros(3), vs, vfrac=vfrac)
    return H, bh, torch.cat([vs[:N, 0], vs[:N, 1], vs[:N, 2]]).contiguous()


systems = [assemble(s) for s in range(STEPS)]

PRECS = (("jacobi", lambda A: hip.Precond(ctx, A, "jacobi", 0)),
         ("chebyshev3", lambda A: hip.PrecondChebyshev(ctx, A, degree=3)),
         ("bjacobi-ilu0", lambda A: hip.Precond(ctx, A, "bjacobi-ilu0", 0)))
ROUTES = (("fgmres(50)", hip.SolverParams(tol=1e-8), False),
          ("gcro-dr(%d,%d)" % (M_BLOCKS, K_REC), hip.SolverParams(solver_type=2, num_blocks=M_BLOCKS, num_recycled=K_REC, tol=1e-8), False),
          ("gcro-dr + handle", hip.SolverParams(solver_type=2, num_blocks=M_BLOCKS, num_recycled=K_REC, tol=1e-8), True))

# ---- the sequences -------------------------------------------------------------------------------------------------------
say()
say("# per system s: iterations (+ applications that rebuilt C), create + solve ms")
for pname, make in PRECS:
    ms = {(r, s): [] for r in range(len(ROUTES)) for s in range(STEPS)}
    its, held = {}, 0
    for rep_ in range(REPS + 1):
        spaces = [hip.RecycleSpace(ctx) if handle else None for _, _, handle in ROUTES]
        for s, (A, b) in enumerate(systems):
            for r, (rname, prm, handle) in enumerate(ROUTES):
                bw, x = b.clone(), torch.zeros(N, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M = make(A)
                info = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm, recycle=spaces[r])
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                M.close()
                apps = spaces[r].info()["applications"] if handle else 0
                its[(r, s)] = (info.iters, apps, info.converged)
                if rep_ > 0:
                    ms[(r, s)].append((t1 - t0) * 1e3)
        for sp in spaces:
            if sp is not None:
                held = sp.info()["bytes"]
                sp.close()
    for r, (rname, _, handle) in enumerate(ROUTES):
        say("%-13s %-17s %s" % (pname, rname, "   ".join(
            "s%d %3d%s%s %s" % (s, its[(r, s)][0], "+%-2d" % its[(r, s)][1] if handle else "   ", "" if its[(r, s)][2] else " (NOT converged)",
                                stats(ms[(r, s)])) for s in range(STEPS))))
    tot = [sum(med(ms[(r, s)]) for s in range(1, STEPS)) for r in range(len(ROUTES))]
    say("%-13s systems 1..%d, sum of medians, ms: %s;  handle / fgmres %.3f, handle / gcro-dr %.3f;  the handle holds %.1f MB" %
        (pname, STEPS - 1, ", ".join("%s %.2f" % (ROUTES[r][0], tot[r]) for r in range(len(ROUTES))), tot[2] / tot[0], tot[2] / tot[1],
         held / 1e6))

# ---- the kernels ---------------------------------------------------------------------------------------------------------
say()
say("# the two kernels against the per-column launches, ms per product (host clock, the calls end synchronised; coefficient upload")
say("# included), %d repeats alternated; algorithmic MB: every vector of the block once + outputs | once per output column" % KERNEL_REPS)
ld = (N + 63) // 64 * 64
for pa, pb, q, what in ((10, 41, 10, "restart of (50,10): C = W Q / U = Vh P R^-1"), (20, 31, 20, "restart of (50,20)"),
                        (10, 0, 10, "Cholesky-QR, 10 vectors")):
    A_ = torch.randn(ld * pa, dtype=torch.float64, device=dev)
    B_ = torch.randn(ld * pb, dtype=torch.float64, device=dev) if pb else None
    Y_ = torch.randn(ld * q, dtype=torch.float64, device=dev)
    O1, O2 = torch.zeros(ld * q, dtype=torch.float64, device=dev), torch.zeros(ld * q, dtype=torch.float64, device=dev)
    coef = np.random.default_rng(1).standard_normal((pa + pb, q))
    tf, tu, gf, gu = [], [], [], []
    for rep_ in range(KERNEL_REPS + 1):
        for mode, acc, O in ((0, tf, O1), (3, tu, O2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hip.dense_tall_gemm(ctx, N, A_, ld, B_, ld, coef, O, ld, mode=mode)
            t1 = time.perf_counter()
            if rep_ > 0:
                acc.append((t1 - t0) * 1e3)
        for per, acc in ((False, gf), (True, gu)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            G = hip.dense_block_gram(ctx, N, A_, ld, B_, ld, Y_, ld, per_column=per)
            t1 = time.perf_counter()
            if rep_ > 0:
                acc.append((t1 - t0) * 1e3)
    assert torch.equal(O1, O2), "k_tall_gemm differs from the per-column launches"
    p = pa + pb
    say("%-46s p %2d q %2d  tall_gemm %s   per column %s   ratio %.3f   MB %7.1f | %7.1f" %
        (what, p, q, stats(tf), stats(tu), med(tf) / med(tu), (p + q) * N * 8 / 1e6, q * (p + 2) * N * 8 / 1e6))
    say("%-46s p %2d q %2d  block_gram %s   per column %s   ratio %.3f   MB %7.1f | %7.1f" %
        ("", p, q, stats(gf), stats(gu), med(gf) / med(gu), (p + q) * N * 8 / 1e6, q * (p + (2 if pb else 1)) * N * 8 / 1e6))
    del A_, B_, Y_, O1, O2

# ---- the 3-RHS Helmholtz solve ---------------------------------------------------------------------------------------------
say()
say("# the 3-RHS Helmholtz solve (theta 0.5, tol 1e-8, guess: the current velocity) of systems 0 and 1, chebyshev3, create + solve ms;")
say("# with a handle the columns of one call share the space and system 1 starts from the space system 0 left")
del systems
hsys = [assemble(s, helmholtz=True) for s in range(2)]
ms = {(r, s): [] for r in range(len(ROUTES)) for s in range(2)}
its = {}
for rep_ in range(REPS + 1):
    spaces = [hip.RecycleSpace(ctx) if handle else None for _, _, handle in ROUTES]
    for s, (H, bh, x0) in enumerate(hsys):
        for r, (rname, prm, handle) in enumerate(ROUTES):
            bw, x = bh.clone(), x0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = hip.PrecondChebyshev(ctx, H, degree=3)
            info = hip.solve(ctx, H, bw, x, prec=M, singular=False, nvec=3, lda=N, params=prm, recycle=spaces[r])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            M.close()
            its[(r, s)] = (info.iters, spaces[r].info()["applications"] if handle else 0, info.converged)
            if rep_ > 0:
                ms[(r, s)].append((t1 - t0) * 1e3)
    for sp in spaces:
        if sp is not None:
            sp.close()
for r, (rname, _, handle) in enumerate(ROUTES):
    say("%-17s %s" % (rname, "   ".join("s%d iterations (3 columns) %3d%s%s %s" % (
        s, its[(r, s)][0], "+%-2d" % its[(r, s)][1] if handle else "   ", "" if its[(r, s)][2] else " (NOT converged)", stats(ms[(r, s)]))
        for s in range(2))))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
