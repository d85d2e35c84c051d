"""Level-by-level comparison of two smoothed-aggregation hierarchies: hip.PrecondAMG against oracle.AMG, or two device
builds.  Both expose levels, level_info(l), export(l, "A" | "P") and aggregates(l)."""
import numpy as np


def compare_levels(M, G, deep=None, ptol=1e-12, atol=1e-11):
    """Levels 0 .. deep-1 (all, and the same number of them, by default): A_l on each, P_l and the aggregates on all but the last compared level.
    Patterns, aggregates and level sizes exact; P values within ptol and A values within atol of their max.  When
    deep stops short of the last level, P_{deep-1} is not compared, nor its size.  Returns (max P gap, max A gap)."""
    if deep is None:
        assert M.levels == G.levels, (M.levels, G.levels)
        deep = G.levels
    gp = ga = 0.0
    for l in range(deep):
        im, ig = M.level_info(l), G.level_info(l)
        if l == deep - 1:
            im, ig = (im["rows"], im["nnz"]), (ig["rows"], ig["nnz"])
        assert im == ig, (l, im, ig)
        for what in ("A", "P") if l < deep - 1 else ("A",):
            rg, cg, vg = G.export(l, what)
            rm, cm, vm = M.export(l, what)
            assert np.array_equal(rg, rm) and np.array_equal(cg, cm), (l, what)
            gap = float(np.max(np.abs(vm - vg))) / np.abs(vg).max()
            if what == "P":
                gp = max(gp, gap)
            else:
                ga = max(ga, gap)
        if l < deep - 1:
            assert np.array_equal(G.aggregates(l), M.aggregates(l)), l
    assert gp <= ptol and ga <= atol, (gp, ga)
    return gp, ga
