"""Run by tests/test_gpu_ins_dist.py::test_two_ranks_run_clean_under_the_pool_canary in a child process with
ISPH_POOL_CANARY=1: create, two steps and destroy of the distributed driver on two rank threads.  The canary is read once,
when the library first touches its pool, so it cannot be switched on inside the test process; with it every pooled device
buffer carries a pattern behind its last element that is checked when the buffer is given back, and an overrun aborts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import isph_amd  # noqa: F401,E402
import test_gpu_ins_dist as M  # noqa: E402
from ranks import RankGroup  # noqa: E402


def main():
    case = M.D.tgv2d_case(16, False, 0.5)
    dc = M.make_decomp(2, (2, 1))
    G = RankGroup(2, timeout_s=60.0)
    try:
        res = G.run(M._rank_steps, case, dc, M.owner_of(dc, case.x), 2, M.JACOBI, False)
    finally:
        G.close()
    assert all(np.isfinite(o["p"]).all() and np.all(o["rows"][:, 14:] == 1) for o in res)
    print("two ranks, two steps: clean")


if __name__ == "__main__":
    main()
