"""-m gpu: the four primitives a time step needs between its neighbour sweeps -- isph_ghost_fill, isph_zero_mean_pressure,
isph_status, isph_tgv_error -- against tests/ins_reference.py.

Bounds.  A sum of n terms taken in ANY order differs from the exact sum by at most (n - 1) eps sum|f_i| (to first order; the
device's tree is far inside it); ins_reference sums exactly (math.fsum).  The mean adds one division, which the slack of
the bound covers from n = 2 on and which is exact at n = 1.  The maximum is a selection: exact.  isph_tgv_error is a
streaming sweep of transcendental terms: 1e-12 relative, the project's bound for such sweeps."""
import numpy as np
import pytest
import torch

from isph_amd import hip
import ins_reference as R

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4097, 100003]          # straddle a wave, a block and the second stage


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- ghost_fill ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncomp", [1, 3, 4, 6])
@pytest.mark.parametrize("nghost", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("on_device", [False, True])
def test_ghost_fill_is_the_gather_by_owner(gpu_ctx, ncomp, nghost, on_device):
    rng = np.random.default_rng(100 * ncomp + nghost)
    nlocal = 37
    nall = nlocal + nghost
    own = np.concatenate([np.arange(nlocal), rng.integers(0, nlocal, size=nghost)]).astype(np.int32)
    a = rng.standard_normal((nall, ncomp)) if ncomp > 1 else rng.standard_normal(nall)
    a[nlocal:] = np.nan                                  # whatever the ghost rows held is overwritten
    want = a[own]
    if on_device:
        ad = _dev(a)
        hip.ghost_fill(gpu_ctx, nlocal, _dev(own), ad)
        got = ad.cpu().numpy()
    else:
        got = a.copy()
        hip.ghost_fill(gpu_ctx, nlocal, own, got)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("bad", [37, -1, 2 ** 31 - 1])
def test_ghost_fill_refuses_an_owner_that_is_not_owned(gpu_ctx, bad):
    nlocal, nall = 37, 300
    own = np.concatenate([np.arange(nlocal), np.zeros(nall - nlocal)]).astype(np.int32)
    own[211] = bad
    a = _dev(np.ones((nall, 3)))
    with pytest.raises(hip.IsphError, match="owner"):
        hip.ghost_fill(gpu_ctx, nlocal, _dev(own), a)
    own[211] = 5                                         # the context is usable afterwards
    hip.ghost_fill(gpu_ctx, nlocal, _dev(own), a)


# ---- zero_mean_pressure ------------------------------------------------------------------------------------------------

def _field(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, size=n))


def _check_zero_mean(ctx, f, nlocal, typ, kinds, update, on_device=True):
    want, mean, count, abs_sum = R.zero_mean_pressure(f, nlocal, typ, kinds, update)
    runs = []
    for _ in range(2):
        if on_device:
            fd = _dev(f)
            m = hip.zero_mean_pressure(ctx, nlocal, _dev(typ.astype(np.int32)), kinds, fd, update=update)
            runs.append((m, fd.cpu().numpy()))
        else:
            fh = f.copy()
            m = hip.zero_mean_pressure(ctx, nlocal, typ.astype(np.int32), kinds, fh, update=update)
            runs.append((m, fh))
    (m, got), (m2, got2) = runs
    print("zero mean: n=%d count=%d mean=%.17g reference=%.17g diff=%.3e bound=%.3e" %
          (nlocal, count, m, mean, abs(m - mean), (max(count, 1) - 1) * R.EPS * abs_sum / max(count, 1)))
    assert np.float64(m).tobytes() == np.float64(m2).tobytes() and got.tobytes() == got2.tobytes()    # run to run
    assert abs(m - mean) <= (max(count, 1) - 1) * R.EPS * abs_sum / max(count, 1)
    # the rows: Solid owned rows are 0, the others lost exactly the device's mean (or nothing)
    kd = R.kind_of(typ, kinds)
    base = np.array(f)
    base[:nlocal][kd[:nlocal] == R.SOLID] = 0.0
    expect = base.copy()
    if update and count:
        expect[kd != R.SOLID] = base[kd != R.SOLID] - m
    assert got.tobytes() == expect.tobytes()
    return m


@pytest.mark.parametrize("n", SIZES)
def test_zero_mean_pressure_all_fluid(gpu_ctx, n):
    nall = n + min(n, 50)
    f = _field(nall, n)
    _check_zero_mean(gpu_ctx, f, n, np.ones(nall, dtype=np.int64), [R.FLUID], True)


@pytest.mark.parametrize("n", SIZES)
def test_zero_mean_pressure_with_solid_rows(gpu_ctx, n):
    """Solid owned rows hold NaN and 1e300: zeroed, and outside the mean.  Solid ghosts are left alone.  BufferDirichlet
    and BufferNeumann count as non-Solid."""
    rng = np.random.default_rng(n)
    nall = n + 40
    kinds = [R.FLUID, R.SOLID, R.BUFFER_DIRICHLET, R.BUFFER_NEUMANN]
    typ = rng.integers(1, 5, size=nall)
    f = _field(nall, n + 1)
    solid_own = np.flatnonzero(typ[:n] == 2)
    f[solid_own[::2]] = np.nan
    f[solid_own[1::2]] = 1e300
    typ[n:n + 5] = 2                                     # Solid ghosts, with a value that must survive
    f[n:n + 5] = 7.25
    for update in (True, False):
        _check_zero_mean(gpu_ctx, f, n, typ, kinds, update)


def test_zero_mean_pressure_update_0_touches_only_the_solid_rows(gpu_ctx):
    n, nall = 257, 300
    typ = np.ones(nall, dtype=np.int32)
    typ[::7] = 2
    f = _field(nall, 5)
    fd = _dev(f)
    m = hip.zero_mean_pressure(gpu_ctx, n, _dev(typ), [R.FLUID, R.SOLID], fd, update=False)
    got = fd.cpu().numpy()
    own_solid = np.zeros(nall, dtype=bool)
    own_solid[:n] = typ[:n] == 2
    assert np.all(got[own_solid] == 0.0) and got[~own_solid].tobytes() == f[~own_solid].tobytes()
    assert m != 0.0


@pytest.mark.parametrize("on_device", [False, True])
def test_zero_mean_pressure_all_solid_gives_mean_0(gpu_ctx, on_device):
    """the declared departure: no row enters, mean 0, nothing subtracted (the reference divides by zero)"""
    n, nall = 65, 80
    typ = np.full(nall, 1, dtype=np.int64)
    f = _field(nall, 9)
    m = _check_zero_mean(gpu_ctx, f, n, typ, [R.SOLID], True, on_device=on_device)
    assert m == 0.0


def test_zero_mean_pressure_host_operands(gpu_ctx):
    n, nall = 4097, 4200
    typ = np.ones(nall, dtype=np.int64)
    typ[3::5] = 2
    _check_zero_mean(gpu_ctx, _field(nall, 11), n, typ, [R.FLUID, R.SOLID], True, on_device=False)


def test_zero_mean_pressure_without_read_back(gpu_ctx):
    n = 1000
    f = _field(n, 3)
    fd, fd2 = _dev(f), _dev(f)
    typ = _dev(np.ones(n, dtype=np.int32))
    assert hip.zero_mean_pressure(gpu_ctx, n, typ, [R.FLUID], fd, want_mean=False) is None
    hip.zero_mean_pressure(gpu_ctx, n, typ, [R.FLUID], fd2)
    gpu_ctx.sync()
    assert torch.equal(fd, fd2)


# ---- status ------------------------------------------------------------------------------------------------------------

def _particles(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 2 * np.pi, size=(n, 3))
    v = rng.standard_normal((n, 3))
    vfrac = rng.uniform(0.5, 1.5, size=n) * 1e-3
    rho = rng.uniform(0.9, 1.1, size=n)
    typ = rng.integers(1, 4, size=n).astype(np.int32)
    return x, typ, vfrac, v, rho


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mask,radius", [(-1, 0.0), (0b101, 2.0), (0b010, 0.0)])
def test_status_matches_the_reference_loop(gpu_ctx, n, mask, radius):
    x, typ, vfrac, v, rho = _particles(n, n + 17)
    centre = (3.0, 3.0, 3.0)
    want, abs_sums = R.status(x, typ, vfrac, v, rho, n, mask, centre, radius)
    args = [_dev(a) for a in (x, typ, vfrac, v, rho)]
    got = hip.status(gpu_ctx, n, *args, type_mask=mask, centre=centre, radius=radius)
    got2 = hip.status(gpu_ctx, n, *args, type_mask=mask, centre=centre, radius=radius)
    assert got.tobytes() == got2.tobytes()                                  # run to run
    cnt = int(want[0])
    print("status n=%d mask=%d: diff %s  bound %s" % (n, mask, np.abs(got[:7] - want[:7]), (max(cnt, 1) - 1) * R.EPS * abs_sums))
    assert got[0] == want[0]
    assert np.all(np.abs(got[:7] - want[:7]) <= (max(cnt, 1) - 1) * R.EPS * abs_sums)
    assert got[7] == want[7]                                                # exact
    if radius == 0.0:
        assert got[7] == 0.0
    elif n >= 63:
        assert got[7] > 0.0


def test_status_host_operands_give_the_device_bits(gpu_ctx):
    n = 4097
    x, typ, vfrac, v, rho = _particles(n, 4)
    a = hip.status(gpu_ctx, n, x, typ, vfrac, v, rho, type_mask=0b011, centre=(1.0, 2.0, 3.0), radius=2.5)
    b = hip.status(gpu_ctx, n, *[_dev(t) for t in (x, typ, vfrac, v, rho)], type_mask=0b011, centre=(1.0, 2.0, 3.0), radius=2.5)
    assert a.tobytes() == b.tobytes()


# ---- tgv_error ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [16 * 16, 1003])
@pytest.mark.parametrize("on_device", [False, True])
def test_tgv_error_matches_the_reference_loop(gpu_ctx, n, on_device):
    rng = np.random.default_rng(n)
    umax, t = 0.1, 0.37
    x = np.zeros((n, 3))
    x[:, :2] = rng.uniform(0, 2 * np.pi, size=(n, 2))
    nu = np.full(n, 0.1) * rng.uniform(0.9, 1.1, size=n)
    rho = rng.uniform(0.9, 1.1, size=n)
    uex, pex = R.tgv_exact(x, t, umax, nu, rho)
    vnp1 = uex + 1e-3 * umax * rng.standard_normal((n, 3))
    p = pex + 0.3 + 1e-4 * rng.standard_normal(n)                            # an offset: the mean is removed
    want = R.tgv_error(x, vnp1, p, rho, nu, t, umax, n)
    ops = (x, vnp1, p, rho, nu)
    if on_device:
        ops = tuple(_dev(a) for a in ops)
    got = hip.tgv_error(gpu_ctx, n, *ops, t, umax)
    print("tgv_error n=%d: %s against %s" % (n, got, want))
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w)
    assert got == hip.tgv_error(gpu_ctx, n, *ops, t, umax)
