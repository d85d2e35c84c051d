"""-m gpu: the device-resident Navier-Stokes time step (isph_ins_*, hip.InsStep) against
  1. the chain of C-ABI calls it replaces, written out below on device tensors (bit for bit: the driver issues the same
     launches on the same data),
  2. the oracle's driver (oracle/tgv_driver.py) at the tolerances of tests/test_gpu_tgv_step.py,
  3. the reference's own convergence table,
and its walls, force hook, refusals and pool hygiene."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from isph_amd import hip, workload
import ins_reference as R
import tgv_driver as T

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """one configuration: the owned particles at t = 0 and everything both the chain and the driver are told"""

    def __init__(self, dim, x, v, p, typ, rho, nu, h, cut, dt, box, kinds=None, kernel="wendland", antisym=True, theta=0.0,
                 block=256, shift=0.0, umax=0.1):
        self.dim, self.h, self.cut, self.dt, self.box = dim, h, cut, dt, box
        self.x, self.v, self.p, self.typ, self.rho, self.nu = x, v, p, typ.astype(np.int32), rho, nu
        self.kinds = [R.FLUID] if kinds is None else list(kinds)
        self.kernel, self.antisym, self.theta, self.block, self.shift, self.umax = kernel, antisym, theta, block, shift, umax
        self.n = len(x)

    def params(self, **kw):
        lo, hi, per = [0.0] * 3, list(self.box) + [1.0] * (3 - self.dim), [1] * self.dim + [0] * (3 - self.dim)
        args = dict(kinds=self.kinds, kernel=self.kernel, box=(lo, hi, per), antisym=int(self.antisym), theta=self.theta,
                    prec_helmholtz="bjacobi-ilu0", helmholtz_block_size=self.block, prec_poisson="bjacobi-ilu0",
                    poisson_block_size=self.block, shift=self.shift, shiftcut=self.cut, nonfluidweight=0.1, tgv_umax=self.umax)
        args.update(kw)
        return hip.InsParams(self.dim, self.dt, self.h, self.cut, **args)

    def driver(self, ctx, **kw):
        S = hip.InsStep(ctx, self.params(**kw))
        S.set_state(*[_dev(a) for a in (self.x, self.v, self.p, self.typ, self.rho, self.nu)])
        return S


def tgv2d_case(N, antisym, theta, kernel="wendland", cut_over_h=2.0, block=256):
    """the particles and settings of oracle/tgv_driver.py::run_tgv2d"""
    umax, nu, rho0 = 0.1, 0.1, 1.0
    L = 2 * np.pi
    dx = L / N
    h = 1.5 * dx
    g = (np.arange(N) + 0.5) * dx
    X, Y = np.meshgrid(g, g, indexing="xy")
    x = np.stack([X.ravel(), Y.ravel(), np.zeros(N * N)], axis=1)
    v, _ = T.tgv_exact(x, 0.0, umax, nu, rho0)
    n = N * N
    return Case(2, x, v, np.zeros(n), np.ones(n), np.full(n, rho0), np.full(n, nu), h, cut_over_h * h, 0.1 * h / umax, (L, L),
                kernel=kernel, antisym=antisym, theta=theta, block=block, umax=umax)


def tgv3d_case(ncell=8, shift=0.05):
    spec = workload.TGVSpec(dim=3, ncell=(ncell,) * 3, brick=(ncell,) * 3, mode=workload.LATTICE)
    p0 = workload.make_tgv(spec)
    n = p0["nlocal"]
    L = 2 * np.pi
    return Case(3, np.ascontiguousarray(p0["x"][:n]), np.ascontiguousarray(p0["v"][:n]), np.zeros(n), p0["type"][:n],
                p0["rho"][:n].copy(), p0["nu"][:n].copy(), spec.h, spec.cut, 0.125 * spec.h, (L, L, L), antisym=False, theta=0.5,
                shift=shift)


def chain(ctx, case, nsteps, zero_mean="reference", force=None, advance=True, rows=None):
    """PairISPH::compute + advanceTime (+ fix isph/shift) as a caller of the C ABI writes them, on device tensors, with
    hip.ghost_fill / hip.zero_mean_pressure as the glue.  zero_mean = "plain": the mean over ALL rows is subtracted (what
    scripts/droplet_step.py does).  rows: list that receives the diagnostics rows.  Returns the final state (numpy)."""
    c = case
    n, dim, dt, kinds = c.n, c.dim, c.dt, c.kinds
    kw = dict(kernel=c.kernel, kinds=kinds)
    x, v, p = _dev(c.x), _dev(c.v), _dev(c.p)
    typ_own, rho_own, nu_own = _dev(c.typ), _dev(c.rho), _dev(c.nu)
    kind_own = R.kind_of(c.typ, kinds)
    mask = (kind_own & R.SOLID) == 0
    solid = bool(np.any(kind_own == R.SOLID))
    fixed = np.array([0] + [int(k == R.SOLID) for k in kinds], dtype=np.int32)
    g = np.zeros(3)
    lo, hi, per = [0.0] * dim, list(c.box), [1] * dim
    out = {}
    for step in range(1, nsteps + 1):
        ctx.hold_neighbours(False)
        nl = hip.NeighbourList(ctx, x, lo, hi, per, c.cut, dim, wrap=True)
        lst = nl.get()
        nl.close()
        own = lst["owner_index"]
        nall = int(own.shape[0])
        fill = lambda a: hip.ghost_fill(ctx, n, own, a)

        def with_ghosts(a, dtype=torch.float64):
            full = torch.zeros((nall,) + tuple(a.shape[1:]), dtype=dtype, device=DEV)
            full[:n] = a
            return full
        xall = lst["x"]
        vall, pall, rho, nu = (fill(with_ghosts(a)) for a in (v, p, rho_own, nu_own))
        typ = with_ghosts(typ_own, torch.int32)
        typ[n:] = typ_own[own[n:].long()]
        parts = dict(dim=dim, nlocal=n, nall=nall, x=xall, type=typ, neigh_ptr=lst["neigh_ptr"], neigh_idx=lst["neigh_idx"],
                     h=c.h, cut=c.cut)
        # ---- computePre
        ctx.hold_neighbours(True)
        vfrac = fill(with_ghosts(hip.compute_volumes(ctx, parts, own, kernel=c.kernel)))
        Gc = Lc = normal = None
        if not c.antisym:
            Gc, Lc = hip.compute_corrections(ctx, parts, own, vfrac, kernel=c.kernel)
        if solid:
            nrm, pnd = hip.compute_normals(ctx, parts, own, vfrac, Gc, **kw)
            normal = fill(with_ghosts(nrm))
        f = torch.zeros((nall, 3), dtype=torch.float64, device=DEV)
        if force is not None:
            f[:n] += _dev(force)
        # ---- Helmholtz
        rhs_only = abs(c.theta) < 1e-24
        H, bh = hip.assemble_helmholtz(ctx, parts, own, dt, c.theta, nu, rho, pall, f, g, vall, antisym=c.antisym, vfrac=vfrac,
                                       Gc=Gc, Lc=Lc, rhs_only=rhs_only, **kw)
        if rhs_only:
            xh = bh.clone()
            ih = None
        else:
            MH = hip.Precond(ctx, H, "bjacobi-ilu0", c.block)
            xh = torch.cat([v[:, k] for k in range(dim)]).contiguous()
            ih = hip.solve(ctx, H, bh, xh, prec=MH, singular=False, nvec=dim, lda=n)
            MH.close(); H.close()
        vstar = torch.zeros((nall, 3), dtype=torch.float64, device=DEV)
        for k in range(dim):
            vstar[:n, k] = xh[k * n:(k + 1) * n]
        fill(vstar)
        # ---- Poisson
        A, b = hip.assemble_poisson(ctx, parts, own, dt, rho, vstar, antisym=c.antisym, vfrac=vfrac, Gc=Gc, Lc=Lc, normal=normal,
                                    singular=hip.NULLSPACE, **kw)
        M = hip.Precond(ctx, A, "bjacobi-ilu0", c.block)
        dpv = torch.zeros(nall, dtype=torch.float64, device=DEV)
        ip = hip.solve(ctx, A, b, dpv[:n], prec=M, singular=True, null_mask=mask.astype(np.int32))
        M.close(); A.close()
        fill(dpv)
        dp_raw = dpv[:n].cpu().numpy()
        if zero_mean == "reference":
            hip.zero_mean_pressure(ctx, n, typ, kinds, dpv, want_mean=False)
        else:
            dpv -= dpv[:n].mean()
        # ---- corrections (the wrapper of the binding has no `kinds`: the call itself)
        pv, dev, keep = hip.particles_view(parts, own, vfrac=vfrac, Gc=Gc, Lc=Lc, normal=normal, **kw)
        hip._check(hip.lib().isph_correct_velocity_pressure(ctx.h, C.byref(pv), int(c.antisym), float(dt), hip._ptr(rho),
                                                            hip._ptr(dpv), hip._ptr(vstar), hip._ptr(pall), 1, 1))
        fill(vstar)
        if rows is not None:
            t = step * dt
            e = hip.tgv_error(ctx, n, xall, vstar, pall, rho, nu, t, c.umax)
            s = hip.status(ctx, n, xall, typ, vfrac, vstar, rho)
            rows.append(np.array(list(e) + list(s) + [ih.iters if ih else 0, ip.iters, ih.converged if ih else 1, ip.converged]))
        out = dict(vstar=vstar[:n].cpu().numpy(), dp=dpv[:n].cpu().numpy(), p_corrected=pall[:n].cpu().numpy(), dp_raw=dp_raw)
        if not advance:
            x, v, p = xall[:n], vall[:n], pall[:n]
            break
        # ---- advanceTime, over owned particles and ghosts
        work = torch.zeros(nall, dtype=torch.float64, device=DEV)
        hip._check(hip.lib().isph_advance_begin(ctx.h, C.byref(pv), int(c.antisym), float(dt), hip._ptr(pall), hip._ptr(vall),
                                                hip._ptr(vstar), hip._ptr(work), 1))
        fill(work)
        hip.advance_end(ctx, nall, dim, dt, work, vstar, pall, xall, vall)
        # ---- fix isph/shift: computePre on the moved particles with the list of the step
        if c.shift > 0.0:
            vfrac = fill(with_ghosts(hip.compute_volumes(ctx, parts, own, kernel=c.kernel)))
            if not c.antisym:
                Gc, Lc = hip.compute_corrections(ctx, parts, own, vfrac, kernel=c.kernel)
            pv, dev, keep = hip.particles_view(parts, own, vfrac=vfrac, Gc=Gc, Lc=Lc, **kw)
            vmax = C.c_double(0.0)
            hip._check(hip.lib().isph_shift_particles(ctx.h, C.byref(pv), int(c.antisym), hip._ptr(fixed), float(c.shift),
                                                      float(c.cut), 0.1, float(dt), hip._ptr(xall), hip._ptr(vall),
                                                      hip._ptr(pall), C.byref(vmax), 1))
        x, v, p = xall[:n].contiguous(), vall[:n].contiguous(), pall[:n].contiguous()
    ctx.hold_neighbours(False)
    out.update(x=x.cpu().numpy(), v=v.cpu().numpy(), p=p.cpu().numpy())
    return out


def driver_phases(ctx, case, nsteps, rows=None, force=None, advance=True):
    S = case.driver(ctx)
    out = {}
    for step in range(1, nsteps + 1):
        S.rebuild()
        S.pre()
        if force is not None:
            S.add_force(_dev(force))
        info = S.solve()
        if rows is not None:
            rows.append(np.array(list(S.diagnostics(step * case.dt)) + [info.helmholtz.iters, info.poisson.iters,
                                                                         info.helmholtz.converged, info.poisson.converged]))
        out = dict(vstar=S.get("vstar"), dp=S.get("dp"), p_corrected=S.get("p"))
        if not advance:
            break
        S.advance()
        if case.shift > 0.0:
            S.shift()
    out.update(x=S.get("x"), v=S.get("v"), p=S.get("p"))
    S.close()
    return out


def driver_run(ctx, case, nsteps, want_rows=True):
    S = case.driver(ctx)
    rows = S.run(nsteps, diag=want_rows)
    out = dict(x=S.get("x"), v=S.get("v"), p=S.get("p"))
    S.close()
    return out, rows


def _same_bits(a, b, what):
    for k in ("x", "v", "p"):
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs, max |diff| %.3e" % (what, k, np.max(np.abs(a[k] - b[k])))


def _same_to_tolerance(a, b, L, umax):
    assert np.max(np.abs(a["x"] - b["x"])) < 1e-8 * L
    assert np.max(np.abs(a["v"] - b["v"])) < 1e-7 * umax
    assert np.max(np.abs(a["p"] - b["p"])) < 1e-6 * np.abs(b["p"]).max()


CASES_2D = [(True, 0.0), (False, 0.0), (False, 0.5)]
_chain_cache = {}


def chain_2d(ctx, antisym, theta):
    """the chain's three steps at N = 16, computed once per configuration and shared (never modified)"""
    key = (antisym, theta)
    if key not in _chain_cache:
        rows = []
        st = chain(ctx, tgv2d_case(16, antisym, theta), 3, rows=rows)
        _chain_cache[key] = (st, np.array(rows))
    return _chain_cache[key]


# ---- 1. against the chain ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("antisym,theta", CASES_2D)
def test_driver_equals_the_chain_2d(gpu_ctx, antisym, theta):
    case = tgv2d_case(16, antisym, theta)
    ref, ref_rows = chain_2d(gpu_ctx, antisym, theta)
    again = chain(gpu_ctx, case, 3)
    reproducible = all(ref[k].tobytes() == again[k].tobytes() for k in ("x", "v", "p"))
    rows = []
    by_phase = driver_phases(gpu_ctx, case, 3, rows=rows)
    by_run, run_rows = driver_run(gpu_ctx, case, 3)
    print("chain run-to-run reproducible: %s" % reproducible)
    if reproducible:
        _same_bits(by_phase, ref, "phases")
        _same_bits(by_run, ref, "isph_ins_run")
        assert np.array(rows).tobytes() == ref_rows.tobytes() and run_rows.tobytes() == ref_rows.tobytes()
    else:           # a stage of the chain is not reproducible on the device: the tolerances of the oracle comparison
        for st in (by_phase, by_run):
            _same_to_tolerance(st, ref, 2 * np.pi, 0.1)


def test_driver_equals_the_chain_3d_with_rebuild_and_shift(gpu_ctx):
    case = tgv3d_case(8, shift=0.05)
    ref = chain(gpu_ctx, case, 3)
    again = chain(gpu_ctx, case, 3)
    reproducible = all(ref[k].tobytes() == again[k].tobytes() for k in ("x", "v", "p"))
    by_phase = driver_phases(gpu_ctx, case, 3)
    by_run, _ = driver_run(gpu_ctx, case, 3, want_rows=False)
    print("chain run-to-run reproducible: %s" % reproducible)
    assert np.max(np.abs(ref["x"] - case.x)) > 0 and np.isfinite(ref["p"]).all()
    if reproducible:
        _same_bits(by_phase, ref, "phases")
        _same_bits(by_run, ref, "isph_ins_run")
    else:
        for st in (by_phase, by_run):
            _same_to_tolerance(st, ref, 2 * np.pi, 0.1)


@pytest.mark.parametrize("side", ["host", "device"])
@pytest.mark.parametrize("wide", [False, True])
def test_the_caller_s_list_then_run_equals_the_chain(gpu_ctx, side, wide):
    """isph_ins_set_list with the caller's ghosts, owners and full list (host or device arrays, 32- or 64-bit offsets):
    isph_ins_run takes it for the first step and rebuilds from the second on"""
    case = tgv2d_case(16, False, 0.5)
    ref, ref_rows = chain_2d(gpu_ctx, False, 0.5)
    up = _dev if side == "device" else (lambda a: np.ascontiguousarray(a))
    S = hip.InsStep(gpu_ctx, case.params())
    S.set_state(*[up(a) for a in (case.x, case.v, case.p, case.typ, case.rho, case.nu)])
    L = 2 * np.pi
    nl = hip.NeighbourList(gpu_ctx, up(case.x), [0.0, 0.0], [L, L], [1, 1], case.cut, 2)
    lst = nl.get(ptr64=wide)
    nl.close()
    S.set_list(lst["x"], lst["owner_index"], lst["neigh_ptr"], lst["neigh_idx"])
    sz = S.sizes()
    assert sz["nall"] == len(lst["owner_index"]) and sz["entries"] == len(lst["neigh_idx"]) and sz["step"] == 0
    own = np.asarray(lst["owner_index"].cpu() if side == "device" else lst["owner_index"])
    assert np.array_equal(S.get("owner", ghosts=True), own)
    assert S.get("v", ghosts=True).tobytes() == case.v[own].tobytes()              # gathered through the owner map
    rows = S.run(3)
    assert S.sizes()["step"] == 3
    got = dict(x=S.get("x"), v=S.get("v"), p=S.get("p"))
    S.close()
    _same_bits(got, ref, "set_list + run")
    assert rows.tobytes() == ref_rows.tobytes()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("antisym,theta", CASES_2D)
def test_driver_matches_the_oracle_driver(gpu_ctx, antisym, theta):
    N, nsteps, umax, L = 16, 3, 0.1, 2 * np.pi
    hist_o, state_o = T.run_tgv2d(N, nsteps, antisym=antisym, theta=theta, return_state=True)
    case = tgv2d_case(N, antisym, theta)
    S = case.driver(gpu_ctx)
    rows = S.run(nsteps)
    st = dict(x=S.get("x"), v=S.get("v"), p=S.get("p"))
    S.close()
    for k, ro in enumerate(hist_o):
        assert abs(rows[k, 0] - ro["p_err"]) <= 1e-6 * ro["p_err"]
        assert abs(rows[k, 2] - ro["u_err"]) <= 1e-6 * ro["u_err"]
        assert rows[k, 14] == 1 and rows[k, 15] == 1
    _same_to_tolerance(st, state_o, L, umax)
    # the diag rows against the errors computed on the host from the same fields (phases, so that the fields can be read)
    S = case.driver(gpu_ctx)
    for step in range(1, nsteps + 1):
        S.rebuild(); S.pre(); S.solve()
        d = S.diagnostics(step * case.dt)
        want = R.tgv_error(S.get("x"), S.get("vstar"), S.get("p"), case.rho, case.nu, step * case.dt, umax, case.n)
        for g_, w_ in zip(d[:4], want):
            assert abs(g_ - w_) <= 1e-12 * abs(w_)
        assert d.tobytes() == rows[step - 1, :12].tobytes()
        S.advance()
    S.close()


# ---- 3. against the reference's table --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [16, 32])
def test_run_reproduces_the_reference_tgv_table(gpu_ctx, N):
    """sph-script/conv-taylor-green-vortex-2d-rev390.txt, Wendland, with the pinned settings of oracle/tgv_driver.py
    (theta 1/2, incremental pressure, corrected family): both error columns to 2.5e-3 relative, read from diag -- no field
    is downloaded."""
    ref = T.known_answers()["conv_taylor_green_vortex_2d_rev390"]["rows"][str(N)]
    case = tgv2d_case(N, T.PINNED["antisym"], T.PINNED["theta"], block=512)
    S = case.driver(gpu_ctx)
    rows = S.run(ref["step"])
    S.close()
    last = rows[-1]
    assert abs(ref["step"] * case.dt - ref["time"]) < 1e-6
    assert abs(last[0] / ref["p_err"] - 1) < 2.5e-3, (last[0], ref["p_err"])
    assert abs(last[2] / ref["u_err"] - 1) < 2.5e-3, (last[2], ref["u_err"])
    assert np.all(rows[:, 14:] == 1)


# ---- 4. walls ----------------------------------------------------------------------------------------------------------------

def droplet_case():
    p0 = workload.make_droplet(6, dim=2, shape="square", wall_layers=4, jitter=0.1)
    n = p0["nlocal"]
    L = 2 * np.pi
    rng = np.random.default_rng(1)
    v = np.zeros((n, 3))
    fluid = R.kind_of(p0["type"][:n], p0["kinds"]) != R.SOLID
    v[fluid, :2] = 0.05 * rng.standard_normal((int(fluid.sum()), 2))
    return Case(2, np.ascontiguousarray(p0["x"][:n]), v, np.zeros(n), p0["type"][:n], np.ones(n), np.full(n, 0.1), p0["h"],
                p0["cut"], p0["dt"], (L, L), kinds=p0["kinds"], antisym=False, theta=0.5, block=512)


def test_walled_droplet_zero_mean_is_the_reference_s(gpu_ctx):
    case = droplet_case()
    solid = R.kind_of(case.typ, case.kinds) == R.SOLID
    assert solid.any() and (~solid).any()
    got = driver_phases(gpu_ctx, case, 1, advance=False)
    ref = chain(gpu_ctx, case, 1, advance=False)
    plain = chain(gpu_ctx, case, 1, zero_mean="plain", advance=False)
    dp, p = got["dp"], got["p_corrected"]
    assert np.all(dp[solid] == 0.0) and np.all(p[solid] == 0.0)
    fl, raw = dp[~solid], ref["dp_raw"][~solid]
    nf = len(fl)
    # the mean that was subtracted is within (nf - 1) eps sum|raw| / nf of the exact one (tests/test_gpu_step_ops.py); each
    # subtraction then rounds once, half an ulp of its result
    bound = (nf - 1) * R.EPS * math.fsum(np.abs(raw)) / nf + 0.5 * R.EPS * math.fsum(np.abs(fl)) / nf
    print("non-Solid rows %d: mean of dp %.3e, bound %.3e" % (nf, abs(math.fsum(fl) / nf), bound))
    assert abs(math.fsum(fl) / nf) <= bound
    for k in ("dp", "p_corrected", "vstar"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert not np.array_equal(got["dp"], plain["dp"])                       # the defect of the scripts: the mean over ALL rows
    assert np.abs(plain["dp"][solid]).max() > 0.0


# ---- 5. the force hook -----------------------------------------------------------------------------------------------------

def test_force_added_between_pre_and_solve_equals_the_chain(gpu_ctx):
    case = tgv2d_case(16, False, 0.5)
    force = np.tile(np.array([0.3, -0.2, 0.0]), (case.n, 1))
    got = driver_phases(gpu_ctx, case, 1, force=force)
    ref = chain(gpu_ctx, case, 1, force=force)
    _same_bits(got, ref, "force hook")
    assert not np.array_equal(got["v"], chain(gpu_ctx, case, 1)["v"])          # the force is felt
    S = case.driver(gpu_ctx)
    S.rebuild(); S.pre()
    assert S.force_ptr() != 0 and S.view().nlocal == case.n and S.view().vfrac
    S.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_by_name(gpu_ctx):
    case = tgv2d_case(16, True, 0.0)
    for kw, text in ((dict(morris_holmes=1), "MorrisHolmes"), (dict(block_helmholtz=1), "block Helmholtz"),
                     (dict(normals_bd_coord=1), "bd_coord"), (dict(normals_use_part=1), "use_part"),
                     (dict(recycle=C.c_void_p(8)), "recycle handle")):
        with pytest.raises(hip.IsphError, match=text):
            hip.InsStep(gpu_ctx, case.params(**kw))
    gpu_ctx.hold_pattern(True)
    try:
        with pytest.raises(hip.IsphError, match="hold-pattern"):
            hip.InsStep(gpu_ctx, case.params())
    finally:
        gpu_ctx.hold_pattern(False)
    S = case.driver(gpu_ctx)
    with pytest.raises(hip.IsphError, match="isph_ins_pre: no neighbour list"):
        S.pre()
    with pytest.raises(hip.IsphError, match="isph_ins_solve: isph_ins_pre comes first"):
        S.solve()
    S.rebuild()
    with pytest.raises(hip.IsphError, match="isph_ins_solve: isph_ins_pre comes first"):
        S.solve()
    S.close()
    wall = droplet_case()
    wall.antisym = True
    with pytest.raises(hip.IsphError, match="Solid particles need the corrected family"):
        wall.driver(gpu_ctx)


def test_a_context_with_a_communicator_is_refused_by_name():
    ctx = hip.Context(0, rank=0, nranks=1, uid=hip.Context.unique_id())
    try:
        case = tgv2d_case(16, True, 0.0)
        with pytest.raises(hip.IsphError, match="communicator"):
            hip.InsStep(ctx, case.params())
        own = _dev(np.arange(4, dtype=np.int32) % 2)
        with pytest.raises(hip.IsphError, match="isph_ghost_fill: a context with a communicator"):
            hip.ghost_fill(ctx, 2, own, _dev(np.zeros(4)))
        with pytest.raises(hip.IsphError, match="isph_zero_mean_pressure: a context with a communicator"):
            hip.zero_mean_pressure(ctx, 2, _dev(np.ones(4, dtype=np.int32)), [99], _dev(np.zeros(4)))
        with pytest.raises(hip.IsphError, match="isph_tgv_error: a context with a communicator"):
            hip.tgv_error(ctx, 2, *[_dev(np.zeros(s)) for s in ((2, 3), (2, 3), 2, 2, 2)], 0.0, 0.1)
        with pytest.raises(hip.IsphError, match="isph_status: a context with a communicator"):
            hip.status(ctx, 2, _dev(np.zeros((2, 3))), _dev(np.ones(2, dtype=np.int32)), _dev(np.ones(2)), _dev(np.zeros((2, 3))),
                       _dev(np.ones(2)))
    finally:
        ctx.close()


# ---- 7. the pool ---------------------------------------------------------------------------------------------------------------

def test_destroy_gives_every_buffer_back(gpu_ctx):
    """after a first pass has grown the context's own workspaces: create, run, destroy leaves no more live bytes in the
    pool than there were before create"""
    case = tgv2d_case(16, False, 0.5)
    driver_run(gpu_ctx, case, 1, want_rows=False)
    gpu_ctx.hold_neighbours(False)
    before = hip.pool_info()["live"]
    S = case.driver(gpu_ctx)
    S.run(2)
    during = hip.pool_info()["live"]
    S.close()
    after = hip.pool_info()["live"]
    assert during > before and after <= before, (before, during, after)
