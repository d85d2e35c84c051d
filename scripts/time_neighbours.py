"""Ghost atoms + full neighbour list on the device (workload.make_cloud_device / isph_nlist_build) against the host rebuild
it replaces (workload.make_cloud, as bench.py --workload step runs it between two steps), in one process, alternated: the
3-D TGV cloud at ISPH_NCELL^3 after one advect step, at the Wendland cut (2 h) and at the Quintic cut (3 h).  The arrays of
the two sides are asserted equal.  The device side is warm (one untimed build first) and timed with a host clock around
a device synchronise, from positions on the device to the dict on the device; isph_nlist_build alone is timed too.
Median (min - max) of ISPH_REPS repetitions.

    python scripts/time_neighbours.py [output file]          (ISPH_NCELL=100, ISPH_REPS=5)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
import isph_amd  # noqa: F401
from isph_amd import hip, workload

n = int(os.environ.get("ISPH_NCELL", "100"))
REPS = int(os.environ.get("ISPH_REPS", "5"))
out_path = sys.argv[1] if len(sys.argv) > 1 else None
STEP_DEVICE_MS = {"wendland": 90.0, "quintic": 290.5}      # device stages of one step at 100^3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stats(ts):
    ts = sorted(ts)
    return "%9.2f (%.2f - %.2f)" % (ts[len(ts) // 2], ts[0], ts[-1])


med = lambda ts: sorted(ts)[len(ts) // 2]
dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = hip.Context(0, stream=st.cuda_stream)
L = 2.0 * np.pi
say("# scripts/time_neighbours.py: 3-D TGV cloud, %d^3 particles after one advect step, periodic box; one box, one run of this" % n)
say("# script, 1 warm-up + %d alternated repetitions per line, host clock (the device side ends in a synchronise): ms, median (min - max)" % REPS)
say("# device: %s; host rebuild on %s OpenMP threads" % (torch.cuda.get_device_name(0), os.environ.get("OMP_NUM_THREADS", "all")))
for kernel, cut_over_h in (("wendland", 2.0), ("quintic", 3.0)):
    spec = workload.TGVSpec(dim=3, ncell=(n, n, n), brick=(n, n, n), mode=workload.ADVECT, cut_over_h=cut_over_h, kernel=kernel)
    like = workload.make_tgv(spec)
    N = like["nlocal"]
    x_h = np.ascontiguousarray(like["x"][:N])
    x_d = torch.from_numpy(x_h).to(dev)
    like_d = dict(like)
    for k in ("rho", "nu", "type"):
        like_d[k] = torch.from_numpy(np.ascontiguousarray(like[k])).to(dev)
    t_host, t_dev, t_build = [], [], []
    peak = 0
    for r in range(REPS + 1):
        t0 = time.perf_counter()
        hc = workload.make_cloud(x_h, (L, L, L), spec.h, spec.cut, like=like)
        t1 = time.perf_counter()
        hip.pool_info(reset_peak=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dc = workload.make_cloud_device(ctx, x_d, (L, L, L), spec.h, spec.cut, like=like_d)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        peak = max(peak, hip.pool_info()["peak_live"])
        nl = hip.NeighbourList(ctx, x_d, (0.0,) * 3, (L,) * 3, (1,) * 3, spec.cut, 3)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        nl.close()
        if r == 0:                                          # the arrays of the two sides are equal at this size
            for k in ("x", "owner_index", "neigh_ptr", "neigh_idx", "type", "rho", "nu", "tag"):
                assert np.array_equal(dc[k].cpu().numpy(), hc[k]), k
            assert dc["neigh_ptr"].cpu().numpy().dtype == hc["neigh_ptr"].dtype and (dc["nlocal"], dc["nall"]) == (hc["nlocal"], hc["nall"])
        else:
            t_host.append((t1 - t0) * 1e3); t_dev.append((t3 - t2) * 1e3); t_build.append((t4 - t3) * 1e3)
        nall, nnz = hc["nall"], len(hc["neigh_idx"])
        del hc, dc
    written = 24 * nall + 4 * nall + 12 * (N + 1) + 4 * nnz
    say()
    say("%s cut %.4f: %d owned, %d ghosts, %d list entries (%.1f per row); the arrays of the two sides are equal"
        % (kernel, spec.cut, N, nall - N, nnz, nnz / N))
    say("  host   workload.make_cloud                         %s" % stats(t_host))
    say("  device workload.make_cloud_device                  %s" % stats(t_dev))
    say("  device isph_nlist_build alone                      %s" % stats(t_build))
    say("  host / device %.1f;  device build = %.1f %% of the step's device stages (%.1f ms);  %.3f GB written (x, owner, offsets, list)"
        " = %.1f GB/s over isph_nlist_build;  peak pool memory of the build %.3f GB"
        % (med(t_host) / med(t_dev), 100.0 * med(t_dev) / STEP_DEVICE_MS[kernel], STEP_DEVICE_MS[kernel], written / 1e9,
           written / 1e9 / (med(t_build) * 1e-3), peak / 1e9))
    assert med(t_dev) < med(t_host), "the device build is not faster than the host rebuild it replaces"
ctx.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
