"""-m gpu: keeping a matrix' pattern -- isph_ctx_hold_pattern, isph_mat_update_values, isph_mat_pattern_info and
isph_prec_refactor (csrc/pattern.hpp, csrc/ingress.hpp mat_update_values_host, csrc/ilu.hpp ilu_refactor).

Every comparison is bit for bit (np.array_equal; floating-point arrays through their uint64 view where a sign of zero or
a NaN could hide): the update moves values without arithmetic, and the refactor runs the deterministic kernels of the
create call in its order on the same input bits.  No tolerance anywhere.

The reference of an updated matrix is twofold: the numpy restatement of tests/pattern_hold_reference.py (what it must
export) and a FRESH create of the same route from (rowptr, colidx, new values) with the mode off, i.e. the code path every
other test of the suite exercises (export, product on a fixed vector, column bits).  The reference of a refactored
preconditioner is a fresh PrecondILU on that fresh matrix.
"""
import functools

import numpy as np
import pytest

from isph_amd import hip
import ilu_shapes as ish
import pattern_hold_reference as ph
import sell_shapes as sh

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def to_dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


class held:
    """the mode on for the duration of a with-block (the contexts are shared by the session)"""

    def __init__(self, ctx, on=True):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        self.ctx.hold_pattern(self.on)

    def __exit__(self, *exc):
        self.ctx.hold_pattern(False)


# ---------------------------------------------------------------- matrices
@functools.lru_cache(maxsize=None)
def rows130():
    """130 rows (two full slices and two rows of a third), slice widths 6, 10 and 4; row 3 is empty, row 70 holds its
    diagonal alone; every other row has its diagonal (the fused block-ILU routes need one) -- except the empty one, for
    which those routes are not run"""
    rng = np.random.default_rng(5)
    n = 130
    rows = []
    for i in range(n):
        top = 5 if i < 64 else 9 if i < 128 else 3
        m = int(rng.integers(1, top + 1))
        others = rng.choice(np.delete(np.arange(n), i), size=m, replace=False)
        rows.append(np.sort(np.concatenate([[i], others])))
    rows[3] = np.zeros(0, dtype=np.int64)
    rows[70] = np.array([70])
    rows[10] = np.sort(np.concatenate([[10], rng.choice(np.arange(11, n), size=5, replace=False)]))   # width 6 for sure
    rows[100] = np.sort(np.concatenate([[100], rng.choice(np.arange(0, 100), size=9, replace=False)]))  # width 10
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    val = rng.integers(1, 50, size=len(ci)).astype(np.float64) * rng.choice([-1.0, 1.0], size=len(ci))
    val[ci == np.repeat(np.arange(n), np.diff(rp))] = 1000.0
    xy = rng.uniform(0.0, 10.0, size=(n, 2))
    return rp, ci, val, n, xy


@functools.lru_cache(maxsize=None)
def rows130_diag():
    """rows130 with a diagonal in row 3 as well: block ILU is defined"""
    rp, ci, val, n, xy = rows130()
    rp2 = rp.copy()
    rp2[4:] += 1
    ci2 = np.insert(ci, rp[3], 3).astype(np.int32)
    val2 = np.insert(val, rp[3], 1000.0)
    return rp2, ci2, val2, n, xy


@functools.lru_cache(maxsize=None)
def lattice(nx=30, seed=9):
    """nx x nx lattice, 9-point stencil, strictly diagonally dominant, atoms in shuffled order: (rowptr, colidx, val, n, xy).
    Spans several of the library's 22 x 22 bricks."""
    rng = np.random.default_rng(seed)
    n = nx * nx
    order = rng.permutation(n)                 # atom a sits at lattice site order[a]
    atom_of = np.empty(n, dtype=np.int64)
    atom_of[order] = np.arange(n)
    rows, vals = [], []
    for a in range(n):
        ix, iy = divmod(int(order[a]), nx)
        cols = []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                jx, jy = ix + dx, iy + dy
                if 0 <= jx < nx and 0 <= jy < nx:
                    cols.append(int(atom_of[jx * nx + jy]))
        cols = np.sort(np.array(cols))
        v = -rng.integers(1, 9, size=len(cols)).astype(np.float64)
        v[cols == a] = 100.0
        rows.append(cols)
        vals.append(v)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    xy = np.stack([order // nx, order % nx], axis=1).astype(np.float64) + 0.5
    return rp, np.concatenate(rows).astype(np.int32), np.concatenate(vals), n, xy


@functools.lru_cache(maxsize=None)
def distinct(name):
    """a fixture of sell_shapes.UNSORTED_FIXTURES with the second occurrence of every repeated column moved to the next
    column the row does not hold, IN PLACE (the row stays as unsorted as it was).  All of them but "unsorted2" repeat a
    column in every fourth long row -- to pin the tie-breaking of the row sort --, which no map can describe: as they
    are they serve test_update_is_refused_without_a_map."""
    rp, ci, val, ncol = sh.fixture(name)[:4]
    ci = ci.copy()
    for i in range(len(rp) - 1):
        seg = ci[rp[i]:rp[i + 1]]
        seen = set()
        for k in range(len(seg)):
            c = int(seg[k])
            if c in seen:
                while c in seen or c in seg:
                    c = (c + 1) % ncol
                seg[k] = c
            seen.add(c)
    ci.setflags(write=False)
    assert ph.mappable(rp, ci) and not np.array_equal(ci, sh.stable_sorted(rp, ci, val)[1])
    return rp, ci, val, ncol, None


MATRICES = {"rows130": rows130, "rows130_diag": rows130_diag, "lattice30": lattice,
            "distinct30": functools.partial(distinct, "unsorted30"), "distinct66": functools.partial(distinct, "unsorted66"),
            "distinct_ragged": functools.partial(distinct, "unsorted_ragged")}


def matrix(name):
    """(rowptr, colidx, val, ncol, coordinates or None)"""
    if name in MATRICES:
        return MATRICES[name]()
    return tuple(sh.fixture(name)[:4]) + (None,)


TABLE130 = np.array([0, 50, 100, 130], dtype=np.int32)          # uneven, last block shorter than 64 rows


def create(ctx, name, route, val):
    """(Matrix, Precond or None) of a route from the named pattern and the given values"""
    rp, ci, _, ncol, xy = matrix(name)
    if route == "host":
        return hip.Matrix.from_csr(ctx, rp, ci, val, ncol=ncol), None
    if route == "device":
        return hip.Matrix.from_csr(ctx, to_dev(rp), to_dev(ci), to_dev(val), ncol=ncol), None
    if route == "bjacobi":
        return hip.Matrix.from_host_csr_with_bjacobi(ctx, rp, ci, val, block_size=64 if len(rp) < 1000 else 512, ncol=ncol)
    if route == "blocks":
        n = len(rp) - 1
        bp = TABLE130 if n == 130 else np.unique(np.append(np.arange(0, n, 500), n)).astype(np.int32)
        return hip.Matrix.from_host_csr_with_bjacobi(ctx, rp, ci, val, ncol=ncol, block_ptr=bp)
    if route == "coords":
        return hip.Matrix.from_host_csr_with_coords(ctx, rp, ci, val, xy, dim=2, ncol=ncol), None
    if route == "coords_bjacobi":
        return hip.Matrix.from_host_csr_with_coords(ctx, rp, ci, val, xy, dim=2, ncol=ncol, with_bjacobi=True)
    raise KeyError(route)


def close(*objs):
    for o in objs:
        if o is not None:
            o.close()


CHUNKED_DIAG = [n for n in sh.CHUNKED_FIXTURES if n.endswith("_diag")]
UPDATE_CASES = (
    [("rows130", r) for r in ("host", "device", "coords")] +
    [("rows130_diag", r) for r in ("host", "device", "bjacobi", "blocks", "coords", "coords_bjacobi")] +
    [("window_rect", r) for r in ("host", "device")] +                       # ghost columns: ncol > nrow
    [(n, r) for n in ("unsorted2", "distinct30", "distinct66", "distinct_ragged") for r in ("host", "device")] +
    [(n, "host") for n in sh.CHUNKED_FIXTURES] +                             # rows across the boundary at 524 288 entries
    [("chunked_unsorted_chunk1", "device")] +
    [(n, r) for n in CHUNKED_DIAG for r in ("bjacobi", "blocks")] +
    [("lattice30", r) for r in ("host", "coords", "coords_bjacobi")]
)


FUSED = ("bjacobi", "blocks", "coords_bjacobi")


def values_for(route, rp, ci, val, seed):
    """ph.new_values; the routes that factor the matrix on the way in keep a pivot (an exact zero on a diagonal is a zero
    pivot of the fresh create this test compares with, not something the update is about)"""
    new = ph.new_values(rp, val, seed=seed)
    if route in FUSED:
        d = np.asarray(ci) == ph.row_of_entry(rp)
        new[d] = 1000.0 + seed
    return new


def observe(A, x):
    rp, ci, v = A.export_csr()
    return rp, ci, v, np.array(A.spmv(np.array(x))), A.column_bits()


def assert_same_matrix(got, want, label):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), label
    assert same(got[2], want[2]), label
    assert same(got[3], want[3]), label
    assert got[4] == want[4], label


@pytest.mark.parametrize("name,route", UPDATE_CASES)
def test_value_update_is_a_fresh_create_of_the_new_values(gpu_ctx, name, route):
    """two updates in a row; after each the matrix exports what the host restatement says and is, in export, product and
    column width, the matrix the same route creates from the new values with the mode off"""
    rp, ci, val, ncol, xy = matrix(name)
    assert ncol > len(rp) - 1 if name == "window_rect" else True
    x = sh.x_of(ncol)
    with held(gpu_ctx):
        A, M = create(gpu_ctx, name, route, val)
    has, nbytes, count = A.pattern_info()
    assert (has, nbytes, count) == (1, 4 * len(ci), 0)
    if route.startswith("coords"):
        assert len(A.subdomains()) - 1 >= (2 if name == "lattice30" else 1)
    before = observe(A, x)
    for step, seed in enumerate((1, 2)):
        new = values_for(route, rp, ci, val, seed)
        A.update_values(new)
        assert A.pattern_info() == (1, 4 * len(ci), step + 1)
        got = observe(A, x)
        urp, uci, uv = ph.updated_csr(rp, ci, new)
        assert np.array_equal(got[0], urp) and np.array_equal(got[1], uci) and same(got[2], uv), (name, route, step)
        F, FM = create(gpu_ctx, name, route, new)                          # mode off
        assert F.pattern_info() == (0, 0, 0)
        assert_same_matrix(got, observe(F, x), (name, route, step))
        close(F, FM)
        assert not same(got[2], before[2])
    if route in ("host", "bjacobi", "blocks", "coords", "coords_bjacobi"):
        assert hip.ingress_info(gpu_ctx)["link_bytes"] > 0                  # the fresh create was the last ingress
        A.update_values(val)
        assert hip.ingress_info(gpu_ctx)["link_bytes"] == 8 * len(ci)
        assert_same_matrix(observe(A, x), before, (name, route, "back"))
    close(A, M)


def test_device_values_update(gpu_ctx):
    """on_device = 1: one scatter launch from a device tensor, for a matrix created from host arrays and for one created
    from device arrays (unsorted rows: the map is not the identity)"""
    name = "distinct_ragged"
    rp, ci, val, ncol, _ = matrix(name)
    x = sh.x_of(ncol)
    new = ph.new_values(rp, val, seed=4)
    F, _ = create(gpu_ctx, name, "host", new)
    want = observe(F, x)
    F.close()
    for route in ("host", "device"):
        with held(gpu_ctx):
            A, _ = create(gpu_ctx, name, route, val)
        A.update_values(to_dev(new))
        assert A.pattern_info()[2] == 1
        assert_same_matrix(observe(A, x), want, route)
        A.close()


# ---------------------------------------------------------------- refactor
def ilu_matrix(name):
    """(rowptr, colidx, val, table of uneven blocks whose last is shorter than 64 rows)"""
    if name == "ladder":
        rp, ci, val, _ = ish.fixture("narrow")                              # ladder([256, 256, 100], TAB_N)
        return rp, ci, val, np.array([0, 200, 500, 560, 612], dtype=np.int32)
    rp, ci, val, _ = ish.fixture("fan")
    return rp, ci, val, np.array([0, 200, 450, 512], dtype=np.int32)


def row_scaled(rp, val, seed=3):
    """D A with d_i in {-2, 1/2, 3, 5/4}: every value changes, signs change, and the ILU exists where A's does"""
    rng = np.random.default_rng(seed)
    d = rng.choice([-2.0, 0.5, 3.0, 1.25], size=len(rp) - 1)
    return np.asarray(val) * np.repeat(d, np.diff(rp)), d


def prec_state(M, r):
    frp, fci, fv = M.export_ilu()
    i = M.info()
    return frp, fci, fv, (i["factor_nnz"], i["stream_chunks"], i["stream_capacity"], i["nblocks"]), np.array(M.apply(np.array(r))), M.value_bits


def assert_same_prec(got, want, label):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), label
    assert same(got[2], want[2]), label
    assert got[3] == want[3] and got[5] == want[5], label
    assert same(got[4], want[4]), label


@pytest.mark.parametrize("vbits", [64, 32])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("route", ["bs512", "table"])
@pytest.mark.parametrize("name", ["ladder", "fan"])
def test_refactor_is_a_fresh_create(gpu_ctx, name, route, k, vbits):
    rp, ci, val, table = ilu_matrix(name)
    kw = dict(block_size=512) if route == "bs512" else dict(block_ptr=table)
    r = np.random.default_rng(1).standard_normal(len(rp) - 1)
    val2, _ = row_scaled(rp, val)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondILU(gpu_ctx, A, level_of_fill=k, value_bits=vbits, **kw)
    old = prec_state(M, r)
    A.update_values(val2)
    M.refactor(A)
    got = prec_state(M, r)
    A2 = hip.Matrix.from_csr(gpu_ctx, rp, ci, val2)
    M2 = hip.PrecondILU(gpu_ctx, A2, level_of_fill=k, value_bits=vbits, **kw)
    assert_same_prec(got, prec_state(M2, r), (name, route, k, vbits))
    assert np.array_equal(got[1], old[1]) and not same(got[2], old[2]) and not same(got[4], old[4])
    A.update_values(val)                                                    # and back: the first factor again
    M.refactor(A)
    assert_same_prec(prec_state(M, r), old, (name, route, k, vbits, "back"))
    close(M, M2, A, A2)


@pytest.mark.parametrize("vbits", [64, 32])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_refactor_on_the_librarys_bricks(gpu_ctx, k, vbits):
    """30 x 30 lattice in shuffled atom order through isph_mat_create_csr_coords; block_size 0 = the bricks"""
    rp, ci, val, n, xy = lattice()
    r = np.random.default_rng(2).standard_normal(n)
    val2, _ = row_scaled(rp, val)
    with held(gpu_ctx):
        A = hip.Matrix.from_host_csr_with_coords(gpu_ctx, rp, ci, val, xy, dim=2)
        M = hip.PrecondILU(gpu_ctx, A, level_of_fill=k, block_size=0, value_bits=vbits)
    assert M.info()["nblocks"] >= 2
    old = prec_state(M, r)
    A.update_values(val2)
    M.refactor(A)
    got = prec_state(M, r)
    A2 = hip.Matrix.from_host_csr_with_coords(gpu_ctx, rp, ci, val2, xy, dim=2)
    M2 = hip.PrecondILU(gpu_ctx, A2, level_of_fill=k, block_size=0, value_bits=vbits)
    assert_same_prec(got, prec_state(M2, r), (k, vbits))
    assert not same(got[2], old[2]) and not same(got[4], old[4])
    close(M, M2, A, A2)


@pytest.mark.parametrize("route", ["bjacobi", "blocks", "coords_bjacobi"])
def test_refactor_of_a_preconditioner_from_the_fused_ingress(gpu_ctx, route):
    name = "lattice30" if route == "coords_bjacobi" else "rows130_diag"
    rp, ci, val, ncol, xy = matrix(name)
    r = np.random.default_rng(3).standard_normal(len(rp) - 1)
    val2, _ = row_scaled(rp, val)
    with held(gpu_ctx):
        A, M = create(gpu_ctx, name, route, val)
    old = prec_state(M, r)
    A.update_values(val2)
    M.refactor(A)
    got = prec_state(M, r)
    A2, M2 = create(gpu_ctx, name, route, val2)
    assert_same_prec(got, prec_state(M2, r), route)
    assert not same(got[2], old[2]) and not same(got[4], old[4])
    close(M, M2, A, A2)


# ---------------------------------------------------------------- solve
def test_update_refactor_solve_equals_create_create_solve(gpu_ctx):
    """singular 12^3 TGV Poisson system, the second matrix scaled row-wise; FGMRES(50), DGKS, tol 1e-8"""
    from problems import Problem, tgv_spec
    pr = Problem(tgv_spec(dim=3, n=12))
    rp, ci, val, b = pr.poisson()
    rng = np.random.default_rng(6)
    d = rng.choice([0.5, 1.0, 2.0, 4.0], size=pr.n)
    val2, b2 = val * np.repeat(d, np.diff(rp)), b * d
    prm = hip.SolverParams(solver_type=0, flexible=1, num_blocks=50, tol=1e-8, ortho=0)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.Precond(gpu_ctx, A, "bjacobi-ilu0", 512)
    x0 = np.zeros(pr.n)
    i0 = hip.solve(gpu_ctx, A, b.copy(), x0, prec=M, singular=True, params=prm)
    A.update_values(val2)
    M.refactor(A)
    x1 = np.zeros(pr.n)
    i1 = hip.solve(gpu_ctx, A, b2.copy(), x1, prec=M, singular=True, params=prm)
    A2 = hip.Matrix.from_csr(gpu_ctx, rp, ci, val2)
    M2 = hip.Precond(gpu_ctx, A2, "bjacobi-ilu0", 512)
    x2 = np.zeros(pr.n)
    i2 = hip.solve(gpu_ctx, A2, b2.copy(), x2, prec=M2, singular=True, params=prm)
    assert i0.converged == 1 and i1.converged == 1 and i2.converged == 1
    assert same(x1, x2) and (i1.iters, i1.restarts) == (i2.iters, i2.restarts)
    assert not same(x1, x0)
    close(M, M2, A, A2)


# ---------------------------------------------------------------- refusals
def test_update_is_refused_without_a_map(gpu_ctx):
    rp, ci, val, ncol, _ = matrix("rows130")
    x = sh.x_of(ncol)
    A, _ = create(gpu_ctx, "rows130", "host", val)                          # mode off
    assert A.pattern_info() == (0, 0, 0)
    before = observe(A, x)
    with pytest.raises(hip.IsphError, match="no entry map"):
        A.update_values(ph.new_values(rp, val))
    assert A.pattern_info() == (0, 0, 0)
    assert_same_matrix(observe(A, x), before, "untouched")
    A.close()
    # a repeated column: created as without the mode
    rows = [[0, 1], [2, 0, 2], [1]]
    rp2 = np.array([0, 2, 5, 6], dtype=np.int32)
    ci2 = np.array(sum(rows, []), dtype=np.int32)
    v2 = np.arange(1.0, 7.0)
    assert not ph.mappable(rp2, ci2)
    for route in ("host", "device"):
        with held(gpu_ctx):
            D = (hip.Matrix.from_csr(gpu_ctx, rp2, ci2, v2) if route == "host" else
                 hip.Matrix.from_csr(gpu_ctx, to_dev(rp2), to_dev(ci2), to_dev(v2)))
        assert D.pattern_info()[0] == 0
        with pytest.raises(hip.IsphError, match="no entry map"):
            D.update_values(v2)
        assert same(np.array(D.spmv(np.ones(3))), np.array([3.0, 12.0, 6.0]))
        D.close()
    name = "unsorted30"                                                     # repeated columns in an unsorted row
    rp3, ci3, val3, ncol3, _ = matrix(name)
    assert not ph.mappable(rp3, ci3)
    F, _ = create(gpu_ctx, name, "host", val3)
    want = observe(F, sh.x_of(ncol3))
    F.close()
    for route in ("host", "device"):
        with held(gpu_ctx):
            D, _ = create(gpu_ctx, name, route, val3)
        assert D.pattern_info() == (0, 0, 0)
        with pytest.raises(hip.IsphError, match="no entry map"):
            D.update_values(val3)
        assert_same_matrix(observe(D, sh.x_of(ncol3)), want, route)        # created as without the mode
        D.close()
    # the context goes on working: a mapped matrix next
    with held(gpu_ctx):
        B, _ = create(gpu_ctx, "rows130", "host", val)
    B.update_values(val)
    assert B.pattern_info()[2] == 1
    assert_same_matrix(observe(B, x), before, "after the refusals")
    B.close()


def moved_column(rp, ci, lo, hi):
    """a copy of colidx with ONE off-diagonal column of a row of [lo, hi) moved to a free neighbouring column inside
    [lo, hi): same nrow, same nnz, rows still ascending.  Returns (colidx, row)."""
    for i in range(lo, hi):
        seg = ci[rp[i]:rp[i + 1]]
        for k, c in enumerate(seg):
            if c != i and lo <= c and c + 1 < hi and c + 1 != i and (k + 1 == len(seg) or seg[k + 1] > c + 1):
                out = ci.copy()
                out[rp[i] + k] = c + 1
                return out, i
    raise AssertionError("no movable column")


@pytest.mark.parametrize("k", [0, 1])
def test_refactor_refuses_another_pattern_and_recovers(gpu_ctx, k):
    rp, ci, val, _ = ilu_matrix("ladder")
    ci_bad, row = moved_column(rp, ci, 300, 512)
    r = np.random.default_rng(4).standard_normal(len(rp) - 1)
    val2, _ = row_scaled(rp, val)
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        M = hip.PrecondILU(gpu_ctx, A, level_of_fill=k, block_size=512)
        Mdead = hip.PrecondILU(gpu_ctx, A, level_of_fill=k, block_size=512)
    Abad = hip.Matrix.from_csr(gpu_ctx, rp, ci_bad, val)
    assert Abad.info()["nnz"] == A.info()["nnz"] and Abad.info()["nrow"] == A.info()["nrow"]
    for P in (M, Mdead):
        with pytest.raises(hip.IsphError, match=r"row %d \(" % row):
            P.refactor(Abad)
    Mdead.close()                                                           # valid for destroy
    A.update_values(val2)
    M.refactor(A)                                                           # ... and for another refactor
    A2 = hip.Matrix.from_csr(gpu_ctx, rp, ci, val2)
    M2 = hip.PrecondILU(gpu_ctx, A2, level_of_fill=k, block_size=512)
    assert_same_prec(prec_state(M, r), prec_state(M2, r), k)
    close(M, M2, A, A2, Abad)


def test_refactor_refuses_other_types_tables_and_sizes(gpu_ctx):
    rp, ci, val, n, xy = lattice()
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        Ao = hip.Matrix.from_host_csr_with_coords(gpu_ctx, rp, ci, val, xy, dim=2)
        Mo = hip.PrecondILU(gpu_ctx, Ao, block_size=0)
        Mp = hip.PrecondILU(gpu_ctx, A, block_size=512)
    for kind, word in (("chebyshev3", "chebyshev"), ("jacobi", "jacobi"), ("sa-amg", "sa-amg")):
        P = hip.Precond(gpu_ctx, A, kind, 512)
        z = np.array(P.apply(np.ones(n)))
        with pytest.raises(hip.IsphError, match=word):
            P.refactor(A)
        assert same(np.array(P.apply(np.ones(n))), z)                       # goes on working
        P.close()
    with pytest.raises(hip.IsphError, match="subdomain table differs"):     # the bricks against consecutive rows
        Mo.refactor(A)
    with pytest.raises(hip.IsphError, match="subdomain table differs"):
        Mp.refactor(Ao)
    rp3, ci3, val3, _, _ = matrix("rows130_diag")
    A3 = hip.Matrix.from_csr(gpu_ctx, rp3, ci3, val3)
    with pytest.raises(hip.IsphError, match="130 rows"):
        Mp.refactor(A3)
    Mo.refactor(Ao)                                                         # both still refactor on their own matrices
    Mp.refactor(A)
    close(Mo, Mp, A, Ao, A3)


def test_iluk_created_with_the_mode_off_is_refused(gpu_ctx):
    """the fill levels are kept only while the mode is on; ILU(0) needs none"""
    rp, ci, val, _ = ilu_matrix("ladder")
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
    M1 = hip.PrecondILU(gpu_ctx, A, level_of_fill=1, block_size=512)
    with pytest.raises(hip.IsphError, match="hold_pattern"):
        M1.refactor(A)
    M0 = hip.PrecondILU(gpu_ctx, A, level_of_fill=0, block_size=512)
    old = prec_state(M0, np.ones(len(rp) - 1))
    M0.refactor(A)
    assert_same_prec(prec_state(M0, np.ones(len(rp) - 1)), old, "ilu0")
    close(M0, M1, A)


# ---------------------------------------------------------------- memory
def test_pool_without_the_mode_and_over_many_cycles(gpu_ctx):
    rp, ci, val, _ = ilu_matrix("ladder")
    val2, _ = row_scaled(rp, val)
    gpu_ctx.sync()
    base = hip.pool_info()["live"]
    A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)                           # mode off: no map
    off = hip.pool_info()["live"] - base
    assert A.pattern_info() == (0, 0, 0)
    A.close()
    assert hip.pool_info()["live"] == base
    with held(gpu_ctx):
        A = hip.Matrix.from_csr(gpu_ctx, rp, ci, val)
        on = hip.pool_info()["live"] - base
        assert off < on <= off + int(1.25 * 4 * len(ci)) + 4096             # the map and the pool's slack, nothing else
        M32 = hip.PrecondILU(gpu_ctx, A, level_of_fill=1, block_size=512, value_bits=32)
        M64 = hip.PrecondILU(gpu_ctx, A, level_of_fill=0, block_size=512)
    A.update_values(val2); M32.refactor(A); M64.refactor(A)
    gpu_ctx.sync()
    live = hip.pool_info()["live"]
    total = live + hip.pool_info()["cached"]
    for c in range(20):
        A.update_values(val if c % 2 == 0 else val2)
        M32.refactor(A)
        M64.refactor(A)
    gpu_ctx.sync()
    p = hip.pool_info()
    assert p["live"] == live and p["live"] + p["cached"] == total
    assert A.pattern_info()[2] == 21
    close(M32, M64, A)
    assert hip.pool_info()["live"] == base
