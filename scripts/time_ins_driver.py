"""The time step of the 3-D Taylor-Green vortex (ISPH_NCELL^3 particles, default 100; Wendland cut 2h, theta 1/2, NullSpace,
GMRES(50) + block ILU(0) on the library's bricks, fix isph/shift 0.05) through the two ways there are to run it:

  chain    bench.py's step_workload: the entry points of the C ABI chained in Python, torch indexing as the glue
  driver   isph_ins_run's phases (hip.InsStep), everything behind the C ABI

alternated in one process, ISPH_REPS times (default 3) ISPH_STEPS steps (default 3) after one warm-up step each, both from
the same initial state.  Compared is the device work of a step -- computePre ... shift, the scope of bench.py's `value`;
the chain's ghosts and neighbour list are made by the host (seconds, not counted), the driver's by isph_ins_rebuild
(reported on its own line).  Then the glue alone at the same size: the ghost fills, the two transposes and the zero mean
of one step, as torch indexing and as the library's primitives.

usage: python scripts/time_ins_driver.py [output file]      (default profiles/ins_driver_100cubed.txt)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import isph_amd  # noqa: F401
from isph_amd import hip, workload
import bench

nc = int(os.environ.get("ISPH_NCELL", "100"))
reps = int(os.environ.get("ISPH_REPS", "3"))
K = int(os.environ.get("ISPH_STEPS", "3"))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ins_driver_%dcubed.txt" % nc)

sys.argv = [sys.argv[0], "--workload", "step", "--ncell", str(nc), "--kernel", "wendland", "--theta", "0.5", "--singular", "nullspace",
            "--prec", "bjacobi-ilu0", "--steps", str(K), "--warmup", "1"]
args = bench.parse()
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = hip.Context(0, stream=stream.cuda_stream, ordering="bricks")
L = 2.0 * np.pi


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


spec = workload.TGVSpec(dim=3, ncell=(nc, nc, nc), brick=(nc, nc, nc), mode=workload.LATTICE, kernel="wendland", cut_over_h=2.0)
p0 = workload.make_tgv(spec)
N = p0["nlocal"]
dt = 0.125 * spec.h
state = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
         (p0["x"][:N], p0["v"][:N], np.zeros(N), p0["type"][:N].astype(np.int32), p0["rho"][:N], p0["nu"][:N])]
prm = hip.InsParams(3, dt, spec.h, spec.cut, box=([0.0] * 3, [L] * 3, [1] * 3), antisym=1, theta=0.5, singular_mode=hip.NULLSPACE,
                    prec_helmholtz="bjacobi-ilu0", helmholtz_block_size=0, prec_poisson="bjacobi-ilu0", poisson_block_size=0,
                    shift=0.05, shiftcut=spec.cut, nonfluidweight=0.1)
PHASES = ("rebuild", "pre", "solve", "advance", "shift")


def driver_steps(nwarm, nsteps):
    """per timed step: dict of phase times in ms"""
    S = hip.InsStep(ctx, prm)
    S.set_state(*state)
    rows, its = [], []
    for step in range(nwarm + nsteps):
        t = [sync()]
        S.rebuild(); t.append(sync())
        S.pre(); t.append(sync())
        info = S.solve(); t.append(sync())
        S.advance(); t.append(sync())
        S.shift(); t.append(sync())
        if step >= nwarm:
            rows.append({k: (t[i + 1] - t[i]) * 1e3 for i, k in enumerate(PHASES)})
            its.append((info.helmholtz.iters, info.poisson.iters))
    ke = 0.5 * float((S.get("v", device=True) ** 2).sum().item())
    S.close()
    return rows, its, ke


chain_ms, chain_recs, driver_ms, driver_steps_ms, driver_rebuild_ms = [], [], [], [], []
for rep in range(reps):
    rec = bench.step_workload(args, ctx=ctx, steps=K, warmup=1, quiet=True)
    chain_ms.append(rec["ms_per_step"])
    chain_recs.append(rec)
    rows, its, ke = driver_steps(1, K)
    per = [sum(r[k] for k in PHASES[1:]) for r in rows]
    driver_steps_ms += per
    driver_ms.append(float(np.mean(per)))
    driver_rebuild_ms += [r["rebuild"] for r in rows]
    print("rep %d: chain %.2f ms/step [its %s / %s, KE %.9g]   driver %.2f ms/step [its %s, KE %.9g]" %
          (rep, rec["ms_per_step"], rec["config"]["iterations_helmholtz_3rhs_total"], rec["config"]["iterations_poisson"],
           rec["config"]["kinetic_energy_sum_end"], driver_ms[-1], its, ke), flush=True)
    last_rows = rows

# ---- the glue alone ---------------------------------------------------------------------------------------------------------
nl = hip.NeighbourList(ctx, state[0], [0.0] * 3, [L] * 3, [1] * 3, spec.cut, 3)
own32 = nl.get()["owner_index"]
nl.close()
own64 = own32.long()
nall = int(own32.shape[0])
a1 = torch.rand(N, dtype=torch.float64, device=dev)
a3 = torch.rand((N, 3), dtype=torch.float64, device=dev)
b1 = torch.zeros(nall, dtype=torch.float64, device=dev)
b3 = torch.zeros((nall, 3), dtype=torch.float64, device=dev)
b1[:N], b3[:N] = a1, a3
typ = torch.ones(nall, dtype=torch.int32, device=dev)
cols = torch.rand(3 * N, dtype=torch.float64, device=dev)


def glue_torch():                       # what bench.py's step does between the library calls
    for _ in range(5):
        a3[own64].contiguous()
    for _ in range(5):
        a1[own64].contiguous()
    torch.cat([a3[:, 0], a3[:, 1], a3[:, 2]]).contiguous()
    torch.stack([cols[:N], cols[N:2 * N], cols[2 * N:]], dim=1).contiguous()
    d = a1.clone()
    d -= d.mean()


def glue_library():                     # the same fills through the primitives (the driver fuses the transposes into one kernel)
    for _ in range(5):
        hip.ghost_fill(ctx, N, own32, b3)
    for _ in range(5):
        hip.ghost_fill(ctx, N, own32, b1)
    hip.zero_mean_pressure(ctx, N, typ, [99], b1, want_mean=False)


def timed(fn, n=10):
    fn()
    ts = []
    for _ in range(n):
        t0 = sync()
        fn()
        ts.append((sync() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


g_t, g_l = timed(glue_torch), timed(glue_library)


def fmt(v):
    return "median %.2f  min %.2f  max %.2f" % (float(np.median(v)), float(min(v)), float(max(v)))


lines = [
    "time step of the 3-D Taylor-Green vortex, %d^3 = %d particles, %d ghosts, Wendland cut 2h, theta 0.5, NullSpace," % (nc, N, nall - N),
    "GMRES(50) + block ILU(0) on the library's bricks, shift 0.05; %s" % torch.cuda.get_device_name(0),
    "%d repetitions x %d steps after 1 warm-up step, chain and driver alternated in one process; ms per step" % (reps, K),
    "",
    "device work of a step (computePre ... shift), mean over the %d steps of a repetition:" % K,
    "  chain  (bench.py step_workload, Python + torch glue)   %s" % fmt(chain_ms),
    "  driver (isph_ins_* phases)                             %s" % fmt(driver_ms),
    "  driver, every single step                               %s" % fmt(driver_steps_ms),
    "  driver / chain (medians)                                %.3f" % (float(np.median(driver_ms)) / float(np.median(chain_ms))),
    "  spread of the chain (max - min) / median                %.3f" % ((max(chain_ms) - min(chain_ms)) / float(np.median(chain_ms))),
    "ghosts + neighbour list: driver isph_ins_rebuild          %s" % fmt(driver_rebuild_ms),
    "                         chain, on the host (not counted) %.0f ms" % chain_recs[-1]["host_lammps_side_ms_per_step"]["neighbour_list_and_ghosts"],
    "",
    "stages of the last repetition, ms per step:",
    "  chain : " + "  ".join("%s %.2f" % (k, v) for k, v in chain_recs[-1]["stages_ms_per_step"].items() if k not in ("neighbour_host", "upload")),
    "  driver: " + "  ".join("%s %.2f" % (k, float(np.mean([r[k] for r in last_rows]))) for k in PHASES[1:]),
    "  (the chain forms G_i and L_i in computePre although the momentum-preserving family never reads them; the driver does not)",
    "",
    "the glue of one step alone (5 ghost fills [n][3], 5 ghost fills [n], 2 transposes, zero mean), ms:",
    "  torch indexing                  median %.3f  min %.3f  max %.3f" % g_t,
    "  isph_ghost_fill / isph_zero_mean_pressure (transposes: fused into the driver's one kernel)  median %.3f  min %.3f  max %.3f" % g_l,
]
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
ctx.close()
