"""-m gpu: the device-resident Poisson-Boltzmann Newton solve (isph_assemble_poisson_boltzmann, isph_pb_residual,
isph_pb_jacobian, isph_solve_poisson_boltzmann) against the oracle's Laplacian rows, numpy restatements of
functor_poisson_boltzmann_f.h / _jacobian.h, the reference's own convergence table and a scipy Newton."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from isph_amd import dist, hip, workload
import oracle as orc
import pb_channel
import pb_harmonic
from ranks import RankGroup

pytestmark = pytest.mark.gpu


def _harmonic(ctx, N, colmap=None, parts=None):
    """the lattice of conv-poisson-boltzmann-harmonic-2d-rev390.txt (as tests/test_gpu_reference_tables.py device_chain)"""
    if parts is None:
        spec = workload.TGVSpec(dim=2, ncell=(N, N), brick=(8, 8), origin=(0.0, 0.0), mode=workload.LATTICE)
        parts = workload.make_tgv(spec)
    n = parts["nlocal"]
    if colmap is None:
        colmap = workload.single_rank_colmap(parts)
    own = parts["owner_index"].astype(np.int64)
    xs, ys = parts["x"][:n, 0] - np.pi, parts["x"][:n, 1] - np.pi
    exact = np.sin(xs) * np.cos(ys)
    vf = hip.compute_volumes(ctx, parts, colmap)
    vfrac = np.ascontiguousarray(vf[own])
    Gc, Lc = hip.compute_corrections(ctx, parts, colmap, vfrac)
    return dict(parts=parts, colmap=colmap, n=n, exact=exact, vf=vf, vfrac=vfrac, Gc=Gc, Lc=Lc,
                f=-(2.0 * exact + np.sinh(exact)))                  # Extra F of poisson-boltzmann-harmonic.xml


def _harmonic_errors(ctx, h, psi):
    n, parts = h["n"], h["parts"]
    xs, ys = parts["x"][:n, 0] - np.pi, parts["x"][:n, 1] - np.pi
    gex = np.stack([np.cos(xs) * np.cos(ys), -np.sin(xs) * np.sin(ys)], axis=1)
    own = parts["owner_index"].astype(np.int64)
    grad = hip.gradient(ctx, parts, h["colmap"], np.ascontiguousarray(psi[own]), h["vfrac"], antisym=False, Gc=h["Gc"],
                        filt=(workload.FLUID_KIND, 127))[:, :2]
    return dict(volume=float(h["vf"][:n].sum()), err_psi=float(np.sqrt(np.sum((psi - h["exact"]) ** 2) / n)),
                err_grad=float(np.sqrt(np.sum((grad - gex) ** 2) / n)))


def _assemble_harmonic(ctx, h, eps=None):
    return hip.assemble_poisson_boltzmann(ctx, h["parts"], h["colmap"], eps=eps, antisym=False, vfrac=h["vfrac"], Gc=h["Gc"],
                                          Lc=h["Lc"])


def _channel(ctx, N, boundary):
    parts, own = pb_channel.channel(N)
    n, nall = parts["nlocal"], parts["nall"]
    colmap = own.astype(np.int32)
    kinds = pb_channel.KINDS
    vf = hip.compute_volumes(ctx, parts, colmap)
    vfrac = np.ascontiguousarray(vf[own])
    morris = boundary == "MorrisHolmes"
    pnd = np.ascontiguousarray(hip.compute_pnd(ctx, parts, colmap, kinds=kinds)[own]) if morris else None
    Gc, Lc = hip.compute_corrections(ctx, parts, colmap, vfrac)
    solid = parts["type"] == 2
    psi0 = solid.astype(float)                                   # isph_electric_potential_on_wall 1.0
    J = hip.assemble_poisson_boltzmann(ctx, parts, colmap, psi0=psi0, antisym=False, vfrac=vfrac, Gc=Gc, Lc=Lc, kinds=kinds,
                                       pnd=pnd, morris_safe_coeff=0.0)
    return J, parts, own, psi0, solid[:n]


def _oracle_laplacian(parts, colmap, kinds=None, eps=None, morris=False):
    """Laplacian(-1, eps) rows with FilterBinary(Fluid, All) (functor_poisson_boltzmann_jacobian.h:56-64) on the oracle"""
    nall = parts["nall"]
    pnd = None
    if morris:
        pnd = orc.Particles(parts, colmap, kernel="wendland", kinds=kinds).compute_pnd()
    P = orc.Particles(parts, colmap, kernel="wendland", kinds=kinds, pnd=pnd, morris_safe_coeff=0.0)
    P.precompute(corrections=True)
    rp, ci = P.graph()
    val = P.laplacian_matrix(rp, ci, antisym=False, alpha=-1.0, material=np.ones(nall) if eps is None else eps,
                             filt=(orc.FLUID, orc.ALL), morris=1 if morris else 0)
    n = len(rp) - 1
    return sps.csr_matrix((val, ci, rp), shape=(n, n))


def _g(psi, gamma, lin):
    if lin:
        return psi / (1.0 + 2.0 * gamma * (psi / 2) ** 2)
    return np.sinh(psi) / (1.0 + 2.0 * gamma * np.sinh(psi / 2.0) ** 2)


def _dg(psi, gamma, lin):
    if lin:
        return (4.0 - 2.0 * gamma * psi ** 2) / (gamma ** 2 * psi ** 4 + 4.0 * gamma * psi ** 2 + 4.0)
    num = 2.0 * gamma * np.cosh(0.5 * psi) * np.sinh(0.5 * psi) * np.sinh(psi)
    den = 2.0 * gamma * np.sinh(0.5 * psi) ** 2 + 1.0
    return np.cosh(psi) / den - num / den ** 2


def _csr(J):
    rp, ci, v = J.export_csr()
    n = len(rp) - 1
    return sps.csr_matrix((v, ci, rp), shape=(n, n)), rp, ci, v


def _check_rows(J, A_or, dirichlet):
    D, rp, ci, v = _csr(J)
    n = D.shape[0]
    fl = np.nonzero(~dirichlet)[0]
    scale = np.abs(A_or.data).max()
    assert abs(D[fl] - A_or[fl]).max() <= 1e-12 * scale
    rows = np.repeat(np.arange(n), np.diff(rp))
    on_d = dirichlet[rows]
    diag = on_d & (ci == rows)
    assert np.all(v[diag] == -1.0) and diag.sum() == dirichlet.sum()
    assert np.all(v[on_d & ~diag] == 0.0)                         # nothing else on a Dirichlet row


# ---------------------------------------------------------------- 1. Jacobian rows after assembly
@pytest.mark.parametrize("case", ["harmonic", "harmonic-eps", "MorrisHolmes", "ConstExtension"])
def test_jacobian_rows_equal_the_oracle_laplacian(gpu_ctx_both, case):
    ctx = gpu_ctx_both
    if case.startswith("harmonic"):
        h = _harmonic(ctx, 32)
        eps = None
        if case == "harmonic-eps":
            x = h["parts"]["x"]
            eps = 1.5 + 0.5 * np.sin(x[:, 0]) * np.cos(2.0 * x[:, 1])      # periodic: images carry their owner's value
        J = _assemble_harmonic(ctx, h, eps)
        A_or = _oracle_laplacian(h["parts"], h["colmap"], eps=eps)
        _check_rows(J, A_or, np.zeros(h["n"], bool))
    else:
        J, parts, own, psi0, solid = _channel(ctx, 64, case)
        A_or = _oracle_laplacian(parts, own, kinds=pb_channel.KINDS, morris=case == "MorrisHolmes")
        assert solid.sum() > 0
        _check_rows(J, A_or, solid)
    J.close()


# ---------------------------------------------------------------- 2. computeF and computeJacobian
@pytest.mark.parametrize("gamma,lin", [(0.0, 0), (0.3, 0), (0.3, 1)])
def test_residual_and_jacobian_diagonal(gpu_ctx_both, gamma, lin):
    ctx = gpu_ctx_both
    J, parts, own, psi0, solid = _channel(ctx, 64, "MorrisHolmes")
    n = parts["nlocal"]
    A_or = _oracle_laplacian(parts, own, kinds=pb_channel.KINDS, morris=True)
    rng = np.random.default_rng(7)
    psi = rng.uniform(-1.0, 1.0, n)
    f = rng.uniform(-1.0, 1.0, n)
    prm = hip.PBParams(kappasq=100.0, gamma=gamma, linearized=lin)
    # functor_poisson_boltzmann_f.h:60-85 + extra_f.h:79-81 (Solid rows: no Extra F)
    Fnp = np.where(solid, psi0[:n] - psi, A_or @ psi + prm.kappasq * _g(psi, gamma, lin) + f)
    F0 = hip.pb_residual(ctx, J, psi, f, params=prm)
    scale = np.abs(Fnp).max()
    assert np.max(np.abs(F0 - Fnp)) <= 1e-12 * scale
    D0 = _csr(J)[0].diagonal()
    hip.pb_jacobian(ctx, J, psi, params=prm)
    D1 = _csr(J)[0].diagonal()
    fl = ~solid
    want = prm.kappasq * _dg(psi, gamma, lin)
    assert np.max(np.abs((D1 - D0)[fl] - want[fl])) <= 1e-13 * np.abs(D1).max()
    assert np.all(D1[solid] == -1.0)
    F1 = hip.pb_residual(ctx, J, psi, f, params=prm)              # F does not depend on the diagonal J holds
    assert np.max(np.abs(F1 - F0)) <= 1e-12 * scale
    J.close()


# ---------------------------------------------------------------- 3. the reference's table through the solve alone
def _tight(n):
    return hip.PBParams(f_tol=1e-6, update_tol=4e-16 * n, max_iters=30, linear=dict(tol=1e-13, max_iters=400))


@pytest.mark.parametrize("N", [16, 32, 64, 128, 256, 512, 1024])
def test_solve_reproduces_reference_pb_harmonic_table(gpu_ctx, N):
    ref = pb_harmonic.known_answers()[N]
    h = _harmonic(gpu_ctx, N)
    J = _assemble_harmonic(gpu_ctx, h)
    psi = np.zeros(h["n"])
    info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, h["f"], params=_tight(h["n"]))
    J.close()
    assert info.status == 1, (info.status, info.newton_iters, info.norm_f, info.norm_update)
    r = _harmonic_errors(gpu_ctx, h, psi)
    assert abs(r["volume"] - ref["volume"]) <= 2e-12 * ref["volume"]
    tol = 1e-8 if N <= 512 else 1e-7
    assert abs(r["err_psi"] - ref["err_psi"]) <= tol * ref["err_psi"], (r, ref)
    assert abs(r["err_grad"] - ref["err_grad"]) <= tol * ref["err_grad"], (r, ref)


# ---------------------------------------------------------------- 4. the reference's defaults
@pytest.mark.parametrize("N", [16, 32, 64, 128, 256])
def test_reference_defaults_converge_to_the_table(gpu_ctx_bricks, N):
    """||F|| <= 1e-8 with lambda_min(J) >~ kappa^2 = 1 bounds the error of psi far below 1e-5 of err_psi"""
    ref = pb_harmonic.known_answers()[N]
    h = _harmonic(gpu_ctx_bricks, N)
    J = _assemble_harmonic(gpu_ctx_bricks, h)
    psi = np.zeros(h["n"])
    info = hip.solve_poisson_boltzmann(gpu_ctx_bricks, J, psi, h["f"])
    J.close()
    assert info.status == 1 and info.norm_f < 1e-8 and info.norm_update < 1e-5
    r = _harmonic_errors(gpu_ctx_bricks, h, psi)
    assert abs(r["err_psi"] - ref["err_psi"]) <= 1e-5 * ref["err_psi"], (r, ref)


# ---------------------------------------------------------------- 5. the nonlinear channel
def _scipy_newton(A, solid, psi0, kappasq):
    n = A.shape[0]
    fl = (~solid).astype(float)
    Af = sps.diags(fl) @ A
    psi = np.zeros(n)
    for _ in range(40):
        F = np.where(solid, psi0 - psi, A @ psi + kappasq * np.sinh(psi))
        Jm = (Af + sps.diags(np.where(solid, -1.0, kappasq * np.cosh(psi)))).tocsc()
        d = spla.spsolve(Jm, -F)
        psi += d
        if np.max(np.abs(d)) <= 1e-15:
            break
    return psi


@pytest.mark.parametrize("boundary", ["MorrisHolmes", "ConstExtension"])
@pytest.mark.parametrize("N", [64, 128])
def test_nonlinear_channel_matches_a_scipy_newton(gpu_ctx_both, N, boundary):
    """channel-edl-potential.xml: kappa^2 = 2 ezcb / psiref = 100, sinh, psi = 1 on the walls"""
    ctx = gpu_ctx_both
    J, parts, own, psi0, solid = _channel(ctx, N, boundary)
    n = parts["nlocal"]
    A_or = _oracle_laplacian(parts, own, kinds=pb_channel.KINDS, morris=boundary == "MorrisHolmes")
    want = _scipy_newton(A_or, solid, psi0[:n], pb_channel.KAPPA ** 2)
    psi = np.zeros(n)
    prm = hip.PBParams(kappasq=pb_channel.KAPPA ** 2, update_tol=1e-12, max_iters=30, linear=dict(tol=1e-13, max_iters=400))
    info = hip.solve_poisson_boltzmann(ctx, J, psi, None, params=prm)
    J.close()
    assert info.status == 1, (info.status, info.newton_iters, info.norm_f, info.norm_update)
    assert np.max(np.abs(psi - want)) <= 1e-10
    assert np.max(np.abs(psi[solid] - 1.0)) <= 1e-12             # the wall rows: psi0 to the linear solve's accuracy


# ---------------------------------------------------------------- 6. status tests and preconditioner reuse
def test_status_tests_and_preconditioner_reuse(gpu_ctx):
    h = _harmonic(gpu_ctx, 32)
    J = _assemble_harmonic(gpu_ctx, h)
    n = h["n"]

    psi = np.zeros(n)
    info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, h["f"], params=hip.PBParams(max_iters=1))
    assert info.status == 0 and info.newton_iters == 1

    bad = h["f"].copy()
    bad[n // 3] = np.nan
    psi = np.zeros(n)
    info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, bad)          # FiniteValue: reported, not raised
    assert info.status == -1 and info.newton_iters == 0

    psi = np.zeros(n)
    info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, h["f"], params=hip.PBParams(prec_max_age=1))
    assert info.status == 1 and info.newton_iters > 1 and info.prec_builds == info.newton_iters

    psi = np.zeros(n)
    info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, h["f"])
    assert info.status == 1 and info.newton_iters < 10 and info.prec_builds == 1
    assert info.linear_iters > 0 and info.ms > 0.0

    psi = np.zeros(n)
    info = hip.solve_poisson_boltzmann(gpu_ctx, J, psi, h["f"], params=hip.PBParams(prec_kind=1))   # block-Jacobi ILU(0)
    assert info.status == 1
    J.close()


# ---------------------------------------------------------------- 7. two ranks
def _pb_rank(rank, G, N):
    spec = workload.TGVSpec(dim=2, ncell=(N, N), brick=(8, 8), origin=(0.0, 0.0), mode=workload.LATTICE, pgrid=(2, 1),
                            rank=rank)
    parts = dist.prune_ghosts(workload.make_tgv(spec))
    plan = dist.make_plan(parts, G.td(rank))
    ctx = G.context(rank)
    try:
        nl = int(parts["nlocal"])
        fwd = hip.HaloForward(ctx, nl, plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        vf = hip.compute_volumes(ctx, parts, plan.colmap)
        vfrac = np.ascontiguousarray(dist.forward_scalar_rccl(fwd, plan, vf))
        fwd.close()
        Gc, Lc = hip.compute_corrections(ctx, parts, plan.colmap, vfrac)
        J = hip.assemble_poisson_boltzmann(ctx, parts, plan.colmap, antisym=False, vfrac=vfrac, Gc=Gc, Lc=Lc, ncol=plan.ncol)
        if plan.ncol > nl:
            J.set_halo(plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        xs, ys = parts["x"][:nl, 0] - np.pi, parts["x"][:nl, 1] - np.pi
        ex = np.sin(xs) * np.cos(ys)
        psi = np.zeros(nl)
        info = hip.solve_poisson_boltzmann(ctx, J, psi, -(2.0 * ex + np.sinh(ex)), params=_tight(N * N))
        J.close()
        return dict(tag=parts["tag"][:nl].astype(np.int64), psi=psi, status=info.status, newton=info.newton_iters)
    finally:
        ctx.close()


def test_two_ranks_match_one_rank(gpu_ctx):
    N = 64
    h = _harmonic(gpu_ctx, N)
    J = _assemble_harmonic(gpu_ctx, h)
    psi1 = np.zeros(h["n"])
    info1 = hip.solve_poisson_boltzmann(gpu_ctx, J, psi1, h["f"], params=_tight(h["n"]))
    J.close()
    assert info1.status == 1
    G = RankGroup(2)
    try:
        res = G.run(_pb_rank, N)
    finally:
        G.close()
    tags1 = h["parts"]["tag"][:h["n"]].astype(np.int64)
    by_tag = np.full(int(max(tags1.max(), max(r["tag"].max() for r in res))) + 1, np.nan)
    by_tag[tags1] = psi1
    assert sum(len(r["tag"]) for r in res) == h["n"]
    for r in res:
        assert r["status"] == 1 and r["newton"] == info1.newton_iters, (r["newton"], info1.newton_iters)
        assert np.max(np.abs(r["psi"] - by_tag[r["tag"]])) <= 1e-10


# ---------------------------------------------------------------- 8. device memory
def test_repeated_pb_cycles_do_not_raise_the_pool_peak(gpu_ctx_bricks):
    h = _harmonic(gpu_ctx_bricks, 64)

    def cycle():
        J = _assemble_harmonic(gpu_ctx_bricks, h)
        psi = np.zeros(h["n"])
        info = hip.solve_poisson_boltzmann(gpu_ctx_bricks, J, psi, h["f"])
        assert info.status == 1
        J.close()
        gpu_ctx_bricks.sync()

    cycle()
    peak = hip.pool_info()["peak_live"]
    cycle()
    cycle()
    assert hip.pool_info()["peak_live"] <= peak
