"""Keeping a matrix' pattern against building everything anew, on the 3-D TGV pressure system (ISPH_NCELL^3 rows).  Both
ways of each pair alternate repetition by repetition in ONE process; median (min - max) over ISPH_REPS repetitions behind
one warm-up.  Nothing is assumed about the outcome: a leg where the kept pattern is not faster is printed like any other.

  * drop-in: the matrix in lexicographic atom order on the host, through the C++ mirror (SolverLin_HIP +
    PrecondWrapper_Ifpack with setCoordinates, "bjacobi-ilu0": tests/cpp/test_pattern_hold_wrappers.cpp, "timed"):
    a solve without hold (full ingress + create), the first solve under holdPattern(true) (full ingress + entry map +
    create: what building the map costs) and a second one (value update + refactor); ingress / set-up / Krylov ms, link
    bytes, map bytes;
  * native: isph_prec_create_ilu against isph_prec_refactor on the assembled matrix in the library's numbering, level of
    fill 0 and 1, value_bits 64 and 32 (create + synchronise against refactor + synchronise, host clock), and create +
    solve against refactor + solve with the benchmark's settings (FGMRES(50), default tolerance, singular).

    python scripts/time_pattern_hold.py [output file]          (ISPH_NCELL=100, ISPH_REPS=7)
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import isph_amd  # noqa: F401
from isph_amd import build, hip, workload

n = int(os.environ.get("ISPH_NCELL", "100"))
REPS = int(os.environ.get("ISPH_REPS", "7"))
out_path = sys.argv[1] if len(sys.argv) > 1 else None
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stats(ts, fmt="%.2f"):
    ts = sorted(ts)
    return (fmt + " (" + fmt + " - " + fmt + ")") % (ts[len(ts) // 2], ts[0], ts[-1])


def med(ts):
    return sorted(ts)[len(ts) // 2]


N = n ** 3
spec = workload.TGVSpec(dim=3, ncell=(n, n, n), brick=(n, n, n), mode=workload.ADVECT)   # one brick: lexicographic atoms
parts = workload.make_tgv(spec)
say("# scripts/time_pattern_hold.py: %d^3 TGV pressure system, %d rows; pairs alternated in one process, %d repetitions, "
    "median (min - max)" % (n, N, REPS))
say("# device: %s" % torch.cuda.get_device_name(0))
say()

# ---------------------------------------------------------------- drop-in
exe = build.build_cpp_pattern_hold_test()
ctx = hip.Context(0, ordering="caller")
colmap = workload.single_rank_colmap(parts)
vf = hip.compute_volumes(ctx, parts, colmap)
A, b = hip.assemble_poisson(ctx, parts, colmap, spec.dt, parts["rho"], np.ascontiguousarray(parts["v"]),
                            vfrac=np.ascontiguousarray(vf[parts["owner_index"]]))
rp, ci, v = A.export_csr()
A.close()
ctx.close()
tmp = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
fin, fco = os.path.join(tmp, "isph_pattern_hold_sys.bin"), os.path.join(tmp, "isph_pattern_hold_xyz.bin")
with open(fin, "wb") as f:
    np.array([len(rp) - 1, len(v)], np.int32).tofile(f)
    rp.astype(np.int32).tofile(f); ci.astype(np.int32).tofile(f); v.tofile(f); np.asarray(b, dtype=np.float64).tofile(f)
with open(fco, "wb") as f:
    for a in range(3):
        np.ascontiguousarray(parts["x"][:N, a], dtype=np.float64).tofile(f)
say("# drop-in: host CSR in lexicographic atom order, SolverLin_HIP::solveProblem with PrecondWrapper_Ifpack + setCoordinates,")
say("# \"bjacobi-ilu0\" on the library's bricks; %d entries" % len(v))
try:
    r = subprocess.run([exe, fin, fco, "timed", str(REPS)], capture_output=True, text=True, timeout=900)
finally:
    for f_ in (fin, fco):
        if os.path.exists(f_):
            os.remove(f_)
for l in r.stdout.splitlines():
    if not l.startswith(">>"):
        say(l)
if r.returncode != 0:
    say("# the driver returned %d: %s" % (r.returncode, r.stderr[-500:]))
say()
del rp, ci, v

# ---------------------------------------------------------------- native
dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = hip.Context(0, stream=st.cuda_stream, ordering="bricks")
dp = dict(parts)
for k in ("x", "type", "neigh_ptr", "neigh_idx"):
    dp[k] = torch.from_numpy(np.ascontiguousarray(parts[k])).to(dev)
own = torch.from_numpy(parts["owner_index"].astype(np.int64)).to(dev)
colmap = own.to(torch.int32).contiguous()
rho = torch.from_numpy(parts["rho"]).to(dev)
vs = torch.from_numpy(np.ascontiguousarray(parts["v"])).to(dev)
vf = hip.compute_volumes(ctx, dp, colmap)
A, b = hip.assemble_poisson(ctx, dp, colmap, spec.dt, rho, vs, vfrac=vf[own].contiguous())
prm = hip.SolverParams()      # bench.py's
x = torch.zeros(N, dtype=torch.float64, device=dev)
bw = b.clone()
ctx.hold_pattern(True)        # an ILU(k > 0) keeps its fill levels (1 B per factor entry) for the refactor


def make(fill, bits):
    return hip.PrecondILU(ctx, A, level_of_fill=fill, block_size=0, value_bits=bits)


say("# native: the assembled matrix in the library's numbering, block ILU on its bricks; isph_prec_create_ilu against")
say("# isph_prec_refactor of a kept preconditioner on the same matrix, each followed by a synchronisation (host clock, ms)")
for fill in (0, 1):
    for bits in (64, 32):
        K = make(fill, bits)
        tc, tr = [], []
        for rep_ in range(2 * REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = make(fill, bits)
            ctx.sync()
            t1 = time.perf_counter()
            M.close()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            K.refactor(A)
            ctx.sync()
            t3 = time.perf_counter()
            if rep_ > 0:
                tc.append((t1 - t0) * 1e3); tr.append((t3 - t2) * 1e3)
        say("bjacobi-ilu%d %2d bits  create %s   refactor %s   refactor / create %.3f  (%+.2f ms)" %
            (fill, bits, stats(tc, "%.3f"), stats(tr, "%.3f"), med(tr) / med(tc), med(tr) - med(tc)))
        K.close()
say()
say("# a solve with the benchmark's settings, the preconditioner created / refactored inside the timed region")
for fill in (0, 1):
    K = make(fill, 64)
    tc, tr, its = [], [], {}
    for rep_ in range(REPS + 1):
        for how in ("create", "refactor"):
            bw.copy_(b); x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if how == "create":
                M = make(fill, 64)
            else:
                K.refactor(A)
                M = K
            inf = hip.solve(ctx, A, bw, x, prec=M, singular=True, params=prm)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if how == "create":
                M.close()
            its[how] = (inf.iters, inf.converged)
            if rep_ > 0:
                (tc if how == "create" else tr).append((t1 - t0) * 1e3)
    say("bjacobi-ilu%d  create + solve %s ms (%d iterations%s)   refactor + solve %s ms (%d iterations%s)   ratio %.3f  (%+.2f ms)" %
        (fill, stats(tc), its["create"][0], "" if its["create"][1] else ", NOT converged", stats(tr), its["refactor"][0],
         "" if its["refactor"][1] else ", NOT converged", med(tr) / med(tc), med(tr) - med(tc)))
    K.close()
say()
ctx.hold_pattern(False)
A.close()
ctx.close()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
