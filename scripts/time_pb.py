"""The nonlinear Poisson-Boltzmann solve of conv-poisson-boltzmann-harmonic-2d-rev390.txt at N = 1024 (1 048 576
particles): the device-resident Newton solve (isph_solve_poisson_boltzmann: F, J, preconditioner, FGMRES and update on
the device, only the norms read back) against the host chain of tests/test_gpu_reference_tables.py device_chain
(Newton loop and sinh / cosh in numpy, a CSR export, a new matrix and a new SA-AMG hierarchy every step), alternating
the two in one process.  Both use the tight settings of tests/test_gpu_poisson_boltzmann.py (linear tol 1e-13).
Reports wall ms, Newton and GMRES iterations and preconditioner builds as one JSON line per run.

usage: python scripts/time_pb.py [N] [ROUNDS]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import isph_amd  # noqa: F401
from isph_amd import hip
from test_gpu_reference_tables import device_chain
from test_gpu_poisson_boltzmann import _assemble_harmonic, _harmonic, _harmonic_errors, _tight

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ctx = hip.Context(0, ordering="bricks")


def device_resident():
    t0 = time.perf_counter()
    h = _harmonic(ctx, N)
    J = _assemble_harmonic(ctx, h)
    psi = np.zeros(h["n"])
    info = hip.solve_poisson_boltzmann(ctx, J, psi, h["f"], params=_tight(h["n"]))
    J.close()
    ctx.sync()
    t2 = time.perf_counter()
    e = _harmonic_errors(ctx, h, psi)
    # ms: lattice + volumes + corrections + assembly + Newton, the span device_chain covers; solve_ms: the solve call alone
    return dict(path="device", N=N, ms=(t2 - t0) * 1e3, solve_ms=info.ms, status=info.status,
                newton=info.newton_iters, gmres=info.linear_iters, prec_builds=info.prec_builds, norm_f=info.norm_f,
                err_psi=e["err_psi"])


def host_chain():
    t0 = time.perf_counter()
    r = device_chain(ctx, N)      # lattice + volumes + corrections + assembly + the Newton loop
    ctx.sync()
    t1 = time.perf_counter()
    return dict(path="host_chain", N=N, ms=(t1 - t0) * 1e3, newton=r["newton"], gmres=int(sum(r["gmres"])),
                prec_builds=len(r["gmres"]), err_psi=r["err_psi"])


for rnd in range(ROUNDS):
    for fn in ((device_resident, host_chain) if rnd % 2 == 0 else (host_chain, device_resident)):
        print(json.dumps(dict(fn(), round=rnd)), flush=True)
ctx.close()
