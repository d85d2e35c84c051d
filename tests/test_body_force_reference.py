"""-m "not gpu": pins tests/body_force_reference.py (the numpy restatement of the smoothed field, the electrostatic force
and the random stress that tests/test_gpu_body_force.py compares the device with) to the C oracle and to the published
known answers of Philox4x32-10, and checks that the binding refuses short operands before any library call.

Gate of the restatement against the oracle: the project's max|a - b| <= 1e-12 max|b| (measured: 2e-16 .. 5e-16)."""
import functools

import numpy as np
import pytest

import isph_amd  # noqa: F401
from isph_amd import hip, workload
import oracle as orc
import body_force_reference as bf
from problems import Problem, tgv_spec

GATE = 1e-12
KINDS = [orc.FLUID, orc.BUFFER_DIRICHLET, orc.BUFFER_NEUMANN, orc.SOLID]   # types 1..4
SLAB = 1.2
CASES = [dict(dim=2, n=20, mode=workload.JITTER), dict(dim=3, n=12, mode=workload.JITTER),
         dict(dim=2, n=16, mode=workload.LATTICE, kernel="quintic", cut_over_h=3.0)]
IDS = ["2d-jitter-wendland", "3d-jitter-wendland", "2d-lattice-quintic"]


def zone_types(parts):
    """x-slabs of buffer particles at both ends, a solid block in the middle, fluid elsewhere; images follow their owners
    (the zones of tests/test_scalar_callers.py)"""
    own = parts["owner_index"]
    x = parts["x"][:parts["nlocal"]] % (2 * np.pi)
    t = np.ones(parts["nlocal"], dtype=np.int32)
    t[x[:, 0] < SLAB] = 2
    t[x[:, 0] > 2 * np.pi - SLAB] = 3
    t[(np.abs(x[:, 0] - np.pi) < 0.5) & (np.abs(x[:, 1] - np.pi) < 0.9)] = 4
    return t[own]


@functools.lru_cache(maxsize=None)
def case(k):
    pr = Problem(tgv_spec(**CASES[k]), antisym=False, kinds=KINDS, types=zone_types)
    pr.pairs = bf.Pairs(pr.parts, KINDS, pr.spec.kernel)
    x = pr.parts["x"]
    own = pr.parts["owner_index"]
    pr.field = np.ascontiguousarray((np.cos(x[:, 0]) + 0.3 * np.sin(2 * x[:, 1]) + 0.2 * x[:, 2])[:pr.n][own])
    return pr


def gate(a, b, what=""):
    err, scale = np.max(np.abs(np.asarray(a) - np.asarray(b))), np.abs(b).max()
    print("%s: max|a - b| = %.3e, max|b| = %.3e" % (what, err, scale))
    assert scale > 0 and err <= GATE * scale, what


def test_workloads_hold_all_four_kinds_and_periodic_images():
    for k, (owned, buffers, solids) in enumerate(((400, 160, 24), (1728, 720, 52), (256, 96, 8))):
        pr = case(k)
        kind = np.asarray(KINDS)[pr.parts["type"][:pr.n] - 1]
        assert pr.n == owned and pr.parts["nall"] > pr.n
        assert ((kind == orc.BUFFER_DIRICHLET) | (kind == orc.BUFFER_NEUMANN)).sum() == buffers
        assert (kind == orc.SOLID).sum() == solids


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox4x32_10_known_answers(ctr, key, out):
    """the three known answers of the Random123 distribution (kat_vectors: philox4x32 10)"""
    got = bf.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(w[0]) for w in got) == out


def test_uniforms_and_normals_of_the_stream():
    """u in (0, 1] (so that ln u is finite) also for the all-ones words; the normals of 2e5 tags have mean 0 and variance
    1 to three standard errors; another step, seed or tag gives other numbers"""
    full = np.array([0xffffffff], dtype=np.uint64)
    zero = np.array([0], dtype=np.uint64)
    assert 0.0 < bf.uniform53(zero, zero)[0] == 2.0 ** -54 and bf.uniform53(full, full)[0] <= 1.0
    tags = np.arange(1, 200001)
    g = bf.normals(tags, 12345, 7, 3)
    assert g.shape == (200000, 9) and np.all(np.isfinite(g))
    n = g.size
    assert abs(g.mean()) <= 3.0 / np.sqrt(n) and abs(g.var() - 1.0) <= 3.0 * np.sqrt(2.0 / n)
    assert abs(np.mean(g[:, 0] * g[:, 1])) <= 3.0 / np.sqrt(len(g))       # the two outputs of one Box-Muller pair
    for other in (bf.normals(tags, 12345, 8, 3), bf.normals(tags, 12346, 7, 3), bf.normals(tags + 1, 12345, 7, 3),
                  bf.normals(tags, 12345 + (1 << 32), 7, 3), bf.normals(tags, 12345, 7 + (1 << 32), 3)):
        assert np.all(np.any(other != g, axis=1))
    assert np.array_equal(bf.normals(tags[:100], 12345, 7, 2), bf.normals(tags[:100], 12345, 7, 3)[:, :4])


@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_restated_gradients_equal_the_oracles(k):
    pr = case(k)
    p, f = pr.parts, pr.field
    kern = pr.spec.kernel
    sym = bf.gradient(p, KINDS, f, pr.P.vfrac, pr.P.Gc, False, (bf.FLUID, bf.ALL), kernel=kern, pairs=pr.pairs)
    gate(sym, pr.P.gradient(f, False, filt=(orc.FLUID, orc.ALL)), "Symmetric (Fluid, All)")
    anti = bf.gradient(p, KINDS, f, pr.P.vfrac, None, True, (bf.FLUID, bf.FLUID), kernel=kern, pairs=pr.pairs)
    gate(anti, pr.P.gradient(f, True, filt=(orc.FLUID, orc.FLUID)), "AntiSymmetric (Fluid, Fluid)")
    kind = np.asarray(KINDS)[p["type"][:pr.n] - 1]
    assert np.all(sym[kind == orc.SOLID] == 0.0) and np.all(anti[kind == orc.SOLID] == 0.0)


@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_mirror_and_buffer_override_act_on_these_workloads(k):
    """conditions on the inputs of the GPU tests: filtered pairs with a mirror coefficient other than 1 exist (measured
    296 / 4448 / 488), the mirrored gradient differs from the plain one (0.41 / 0.27 / 0.043 of the maximum), and the
    buffer rows of the phi gradient hold -ae_e exactly"""
    pr = case(k)
    p, f, kern = pr.parts, pr.field, pr.spec.kernel
    pnd = pr.P.compute_pnd()
    plain = bf.gradient(p, KINDS, f, pr.P.vfrac, pr.P.Gc, kernel=kern, pairs=pr.pairs)
    mir, coeff, which = bf.gradient(p, KINDS, f, pr.P.vfrac, pr.P.Gc, pnd=pnd, kernel=kern, pairs=pr.pairs, with_coeff=True)
    npairs = int((which & (coeff != 1.0)).sum())
    diff = np.abs(mir - plain).max() / np.abs(plain).max()
    print("mirrored pairs %d, |mirrored - plain| / max = %.3g" % (npairs, diff))
    assert npairs > 0 and diff > 1e-3
    ae = np.array([0.3, -0.2, 0.1])
    gphi = bf.phi_gradient(p, KINDS, f, pr.P.vfrac, ae, pr.P.Gc, kernel=kern, pairs=pr.pairs)
    kind = np.asarray(KINDS)[p["type"][:pr.n] - 1]
    buf = (kind == orc.BUFFER_DIRICHLET) | (kind == orc.BUFFER_NEUMANN)
    assert buf.sum() > 0 and np.array_equal(gphi[buf], np.tile(-ae, (buf.sum(), 1)))
    fluid = kind == orc.FLUID
    gate(gphi[fluid], pr.P.gradient(f, False, filt=(orc.FLUID, orc.FLUID))[fluid], "phi gradient on the fluid rows")


@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_restated_stress_columns_equal_the_oracles_divergence(k):
    pr = case(k)
    p, dim, n = pr.parts, pr.parts["dim"], pr.n
    rs = bf.random_stress_tensor(p, KINDS, p["tag"], 99, 3)
    rs_all = bf.fill_ghosts(p, rs)
    nu, rho, dt, kBT = np.full(n, 0.1), np.full(n, 1.0), 1e-3, 0.5
    df = bf.random_stress_force(p, KINDS, dt, kBT, nu, rho, rs_all, pr.P.vfrac, pr.spec.kernel, pairs=pr.pairs)
    kind = np.asarray(KINDS)[p["type"][:n] - 1]
    fl = (kind & orc.FLUID) != 0
    sq = np.sqrt(2.0 * kBT * nu * rho / dt / pr.P.vfrac[:n])
    for c in range(dim):
        col = bf.unpack_column(rs_all, c)
        div = pr.P.divergence(col, True, alpha=-1.0, filt=(orc.FLUID, orc.FLUID))
        gate(df[fl, c], (div * sq)[fl], "stress column %d" % c)
    assert np.all(df[~fl] == 0.0) and (~fl).sum() > 0
    if dim == 2:
        assert np.all(df[:, 2] == 0.0)


@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_tensors_are_symmetric_traceless_and_zero_off_the_fluid(k):
    pr = case(k)
    p, dim, n = pr.parts, pr.parts["dim"], pr.n
    rs = bf.random_stress_tensor(p, KINDS, p["tag"], 2024, 11)
    kind = np.asarray(KINDS)[p["type"][:n] - 1]
    fl = (kind & orc.FLUID) != 0
    assert np.all(rs[~fl] == 0.0) and np.all(np.any(rs[fl] != 0.0, axis=1))
    diag = [bf.PACK.index((a, a)) for a in range(dim)]
    trace = rs[:, diag].sum(axis=1)
    # 4 ulp of the largest entry of the tensors of the cloud (measured 0.5 .. 2 ulp).  Per tensor the figure does not
    # hold for the prescribed arithmetic: T[k][k] -= tr / dim leaves a residual of ulps of the DRAWN diagonal, and two
    # drawn diagonals that nearly cancel leave entries much smaller than that (measured up to 16 ulp of a tensor's own
    # largest entry)
    print("trace residual: %.2f ulp of the largest entry" % (np.abs(trace).max() / np.spacing(np.abs(rs).max())))
    assert np.all(np.abs(trace) <= 4 * np.spacing(np.abs(rs).max()))
    if dim == 2:
        assert np.all(rs[:, 3:] == 0.0)
    for c in range(dim):                                                   # column c, row k == column k, row c
        for q in range(dim):
            assert np.array_equal(bf.unpack_column(rs, c)[:, q], bf.unpack_column(rs, q)[:, c])
    # the off-diagonal entries are means of two normals (variance 1/2)
    off = rs[fl, 1]
    assert abs(off.var() - 0.5) <= 4.0 * 0.5 * np.sqrt(2.0 / len(off))


def test_smooth_field_reproduces_a_constant_up_to_the_partition_of_unity_and_keeps_unfiltered_rows():
    pr = case(0)
    p, n = pr.parts, pr.n
    one = np.ones(p["nall"])
    sf = bf.smooth_field(p, KINDS, one, pr.P.vfrac, pr.spec.kernel, pairs=pr.pairs)
    assert np.max(np.abs(sf - 1.0)) <= 0.15                                # sum_j W_ij V_j on a jittered cloud
    kind = np.asarray(KINDS)[p["type"][:n] - 1]
    out = bf.smooth_field(p, KINDS, pr.field, pr.P.vfrac, pr.spec.kernel, filt=(bf.SOLID, bf.ALL), out=np.full(n, -7.0),
                          pairs=pr.pairs)
    assert np.all(out[kind != orc.SOLID] == -7.0) and np.all(out[kind == orc.SOLID] != -7.0)
    every = bf.smooth_field(p, KINDS, pr.field, pr.P.vfrac, pr.spec.kernel, pairs=pr.pairs)
    assert np.array_equal(out[kind == orc.SOLID], every[kind == orc.SOLID])


def test_binding_refuses_operands_shorter_than_the_abi_reads():
    """every new wrapper checks the element counts the C ABI reads before the library is touched (ctx is None here)"""
    pr = case(0)
    p, cm, n, nall = pr.parts, pr.colmap, pr.n, pr.parts["nall"]
    assert nall > n
    V, G = np.ones(nall), np.zeros((n, 4))
    psi, tag = np.zeros(nall), np.arange(1, n + 1, dtype=np.int32)
    prm = hip.EkParams(ezcb=1.0)
    assert (prm.ezcb, prm.psiref, prm.gamma) == (1.0, 1.0, 0.0) and list(prm.pb_e) == [0.0] * 3 and list(prm.ae_e) == [0.0] * 3
    kw = dict(kinds=KINDS)
    with pytest.raises(hip.OperandError):
        hip.smooth_field(None, p, cm, psi[:n], V, **kw)                                   # f on owned particles only
    with pytest.raises(hip.OperandError):
        hip.smooth_field(None, p, cm, psi, V[:n], **kw)                                   # vfrac on owned particles only
    with pytest.raises(hip.OperandError):
        hip.smooth_field(None, p, cm, psi, V, out=np.zeros(n - 1), **kw)
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi[:n], V, Gc=G, **kw)                 # psi on owned particles only
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi, V, phi=psi[:n], Gc=G, **kw)        # phi on owned particles only
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi, V, Gc=G, morris_holmes=True, **kw)  # MorrisHolmes without pnd
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi, V, Gc=G, pnd=V[:n], **kw)          # pnd on owned particles only
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi, V, antisym=False, **kw)            # Symmetric family without Gc
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi, V, Gc=G[:-1], **kw)
    with pytest.raises(hip.OperandError):
        hip.electrostatic_force(None, p, cm, prm, psi, V, Gc=G, f=np.zeros((n - 1, 3)), **kw)
    with pytest.raises(hip.OperandError):
        hip.random_stress_tensor(None, p, cm, tag[:-1], 1, 0, **kw)                       # a short tag
    rs_all, nu, f = np.zeros((nall, 6)), np.ones(n), np.zeros((n, 3))
    with pytest.raises(hip.OperandError):
        hip.random_stress_force(None, p, cm, 0.1, 1.0, nu, nu, rs_all[:n], f, V, **kw)    # rs without ghosts
    with pytest.raises(hip.OperandError):
        hip.random_stress_force(None, p, cm, 0.1, 1.0, nu[:-1], nu, rs_all, f, V, **kw)
    with pytest.raises(hip.OperandError):
        hip.random_stress_force(None, p, cm, 0.1, 1.0, nu, nu, rs_all, f[:-1], V, **kw)
    with pytest.raises(hip.OperandError):
        hip.random_stress_force(None, p, cm, 0.1, 1.0, nu, nu, rs_all, f, V[:n], **kw)
    with pytest.raises(hip.OperandError):
        hip.force_from_random_stress(None, p, cm, tag[:-1], 1, 0, 0.1, 1.0, nu, nu, f, V, **kw)
    with pytest.raises(hip.OperandError):
        hip.force_from_random_stress(None, p, cm, tag, 1, 0, 0.1, 1.0, nu, nu[:-1], f, V, **kw)
    with pytest.raises(hip.OperandError):
        hip.force_from_random_stress(None, p, cm, tag, 1, 0, 0.1, 1.0, nu, nu, np.zeros((n, 2)), V, **kw)
