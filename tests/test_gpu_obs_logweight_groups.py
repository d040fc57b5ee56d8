"""pp_obs_logweight_groups (csrc/obs_logweight.hip) on the device: the vector likelihood of the M n_per rows of a batched posterior
call, operands per particle or per group. Row i = g n_per + j must have the BITS pp_obs_logweight gives for the same element
values - for every width (lanes per row, the U = 4 trip, the slot wrap, cut groups), every group size (several groups inside one
wave, groups that straddle waves and workgroups) and every stride form; then float64, support, untouched memory and refusals."""
import numpy as np
import pytest

import obs_logweight_ref as OR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

KS = (1, 3, 4, 5, 127, 128, 129, 257, 400, 1030)
GROUPS = ((1, 7), (2, 1), (5, 3), (3, 64), (2, 67))      # (M, n_per)
NMAX, KMAX = 192, 1030
SENTINEL = -12345.5
X_BIT = 16


def bar(ref):
    """The project's bar for this kernel (tests/test_gpu_obs_logweight.py): rtol 1e-4, atol 1e-4 * max(1, |ref|max)."""
    return dict(rtol=1e-4, atol=1e-4 * max(1.0, float(np.max(np.abs(ref)))))


@pytest.fixture(scope='module')
def lib():
    from pyprob_amd import lib as L
    return L.load()


@pytest.fixture(scope='module')
def ops():
    from pyprob_amd.ops import ops
    return ops


def pool(kind):
    """Parameters p0..p3 and values x, [NMAX, KMAX] float32 on the host: ANY pairing of a value with parameters of other rows
    lies inside the support (a group's value row meets the parameters of all its particles) and every log-density is finite."""
    g = np.random.RandomState(77 + kind)
    u = lambda a, b: g.uniform(a, b, (NMAX, KMAX)).astype(np.float32)  # noqa: E731
    z = np.zeros((NMAX, KMAX), np.float32)
    table = {0: lambda: ([u(-2, 2), u(0.3, 2), z, z], u(-3, 3)),
             1: lambda: ([u(-2, -1), u(1, 3), z, z], u(-0.9, 0.9)),
             3: lambda: ([u(0.5, 6), z, z, z], np.floor(u(0, 9))),
             4: lambda: ([u(0.1, 0.9), z, z, z], np.floor(u(0, 2)).clip(0, 1)),
             6: lambda: ([u(0.5, 3), z, z, z], u(0.05, 3)),
             7: lambda: ([u(0.5, 4), u(0.5, 3), z, z], u(0.05, 4)),
             8: lambda: ([u(0.5, 4), u(0.5, 4), u(-2, -1), u(1, 2)], u(-0.9, 0.9)),
             9: lambda: ([u(-1, 1), u(0.3, 1.5), z, z], u(0.1, 4)),
             10: lambda: ([u(0.5, 2), u(0.5, 3), z, z], u(0.1, 3)),
             11: lambda: ([np.floor(u(10, 21)), u(-2, 2), z, z], np.floor(u(0, 11)).clip(0, 10)),
             12: lambda: ([u(-3, 3), u(0.2, 8), z, z], u(-3.1, 3.1)),
             13: lambda: ([u(-1, 1), u(0.5, 2), u(-3, -2), u(2, 3)], u(-1.9, 1.9))}
    return table[kind]()


_pools = {}


def dev_pool(kind):
    """The pool on the device, made once per family and left unchanged."""
    if kind not in _pools:
        p, x = pool(kind)
        _pools[kind] = ([torch.from_numpy(q).cuda() for q in p], torch.from_numpy(x).cuda())
    return _pools[kind]


def block(src, rows, k):
    """A contiguous [rows, k] copy of the pool's corner."""
    return src[:rows, :k].contiguous()


def fill(o, t, rs, es, row0=0):
    o.p, o.row_stride, o.elem_stride = t.data_ptr() + 4 * row0 * rs, rs, es


def single(lib, kind, ps, x, k, n, scale=1.0, lw=None, lp=None):
    """pp_obs_logweight: ps / x = (tensor, row stride, element stride, first row)."""
    from pyprob_amd import lib as L
    arr = (L.pp_obs_operand * 4)()
    for q in range(OR.N_PARAMS[kind]):
        fill(arr[q], *ps[q])
    xo = L.pp_obs_operand()
    fill(xo, *x)
    L.check(lib.pp_obs_logweight(kind, arr, xo, k, scale, L.ptr(lw), L.ptr(lp), None, n, n, L.stream_ptr()), 'pp_obs_logweight')


def grouped(lib, kind, ps, x, mask, k, M, n_per, scale=1.0, lw=None, lp=None, check=True):
    """pp_obs_logweight_groups straight through the C ABI on torch's current stream."""
    from pyprob_amd import lib as L
    arr = (L.pp_obs_operand * 4)()
    for q in range(OR.N_PARAMS.get(kind, 2)):      # (a refused kind: two slots are filled)
        if ps[q] is not None:
            fill(arr[q], *ps[q])
    xo = L.pp_obs_operand()
    if x is not None:
        fill(xo, *x)
    rc = lib.pp_obs_logweight_groups(kind, arr, xo, mask, k, scale, L.ptr(lw), L.ptr(lp), M, n_per, L.stream_ptr())
    if check:
        L.check(rc, 'pp_obs_logweight_groups')
    return rc


def both(lib, kind, k, M, n_per, scale=0.37):
    """(lp, lw) of the grouped call and of the M single-observation calls on the same values: per-particle parameters [M n_per, k],
    x [M, k] one row per group; the single call of group g reads the parameter rows [g n_per, (g + 1) n_per) and x row g as ONE
    SHARED ROW (0, 1)."""
    P, X = dev_pool(kind)
    n = M * n_per
    ps = [block(q, n, k) for q in P]
    x = block(X, M, k)
    start = torch.linspace(-3.0, 5.0, n, device='cuda')
    lw_g, lw_s = start.clone(), start.clone()
    lp_g, lp_s = torch.full((n,), SENTINEL, device='cuda'), torch.full((n,), SENTINEL, device='cuda')
    grouped(lib, kind, [(q, k, 1) for q in ps], (x, k, 1), X_BIT, k, M, n_per, scale=scale, lw=lw_g, lp=lp_g)
    for g in range(M):
        a, b = g * n_per, (g + 1) * n_per
        single(lib, kind, [(q, k, 1, a) for q in ps], (x[g], 0, 1), k, n_per, scale=scale,
               lw=lw_s[a:b], lp=lp_s[a:b])
    return [t.cpu().numpy() for t in (lp_g, lw_g, lp_s, lw_s)]


# ---- 1. bit identity with the single-observation kernel --------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_rows_have_the_bits_of_the_single_observation_kernel(lib, k):
    """Several groups inside one wave (k <= 128 with n_per 1 or 3), the U = 4 trip (k >= 257), the slot wrap (k > 1024), the cut
    group (k % 4 != 0) and group rows that are not 16-byte aligned (k % 4 != 0: the grouped call reads x by elements, and the
    slices of the single calls start at g n_per k floats)."""
    for M, n_per in GROUPS:
        lp_g, lw_g, lp_s, lw_s = both(lib, 0, k, M, n_per)
        assert np.all(np.isfinite(lp_s)) and not np.any(lp_s == SENTINEL), (k, M, n_per)
        assert np.array_equal(lp_g, lp_s), (k, M, n_per, np.flatnonzero(lp_g != lp_s)[:5])
        assert np.array_equal(lw_g, lw_s), (k, M, n_per, np.flatnonzero(lw_g != lw_s)[:5])


@pytest.mark.parametrize('kind', OR.KINDS)
def test_every_family_has_the_bits_of_the_single_observation_kernel(lib, kind):
    for k in (5, 400):
        for M, n_per in ((5, 3), (2, 67)):
            lp_g, lw_g, lp_s, lw_s = both(lib, kind, k, M, n_per)
            assert np.all(np.isfinite(lp_s)), (kind, k, M, n_per)
            assert np.array_equal(lp_g, lp_s) and np.array_equal(lw_g, lw_s), (kind, k, M, n_per)


# ---- 2. stride forms (through the operator) -----------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (5, 128, 400))
def test_stride_forms_deliver_the_same_bits(ops, k):
    """The mean shared [k], per particle [M n_per, 1] or a padded [M n_per, k] view, x a padded [M, k] view: the bits of the call
    that reads the same values from contiguous [M n_per, k] / [M, k] blocks."""
    P, X = dev_pool(0)
    M, n_per = 5, 13
    n = M * n_per
    sd = P[1][:1, :1].reshape(1).contiguous()
    x = block(X, M, k)

    def run(mean, xv):
        lp = torch.full((n,), SENTINEL, device='cuda')
        ops.obs_logweight_groups(None, 0, [mean, sd, None, None], xv, X_BIT, k, 1.0, lp, M, n_per)
        return lp.cpu().numpy()

    def padded(t, pad):
        buf = torch.full((t.shape[0], k + pad), float('nan'), device='cuda')
        buf[:, :k] = t
        return buf[:, :k]
    full = block(P[0], n, k)
    want = run(full, x)
    assert np.all(np.isfinite(want))
    for pad in (3, 4):       # (a row stride that is / is not a multiple of 4: the 4-byte and the 16-byte path)
        assert np.array_equal(run(padded(full, pad), x), want), ('padded mean', pad)
        assert np.array_equal(run(full, padded(x, pad)), want), ('padded x', pad)
        assert np.array_equal(run(padded(full, pad), padded(x, 7 - pad)), want), ('both padded', pad)
    row = full[0].contiguous()
    assert np.array_equal(run(row, x), run(row.reshape(1, k).expand(n, k).contiguous(), x))
    per = full[:, 0].contiguous().reshape(n, 1)
    assert np.array_equal(run(per, x), run(per.expand(n, k).contiguous(), x))
    # an image-shaped value block [M, *event] and per-particle block [M n_per, *event]
    if k == 400:
        assert np.array_equal(run(full.reshape(n, 1, 20, 20), x.reshape(M, 1, 20, 20)), want)
    # x NOT marked per group: one shared row [k], or one row per particle [M n_per, k]
    lp = torch.full((n,), SENTINEL, device='cuda')
    ops.obs_logweight_groups(None, 0, [full, sd, None, None], x[0].contiguous(), 0, k, 1.0, lp, M, n_per)
    lp2 = torch.full((n,), SENTINEL, device='cuda')
    ops.obs_logweight(None, 0, [full, sd, None, None], x[0].contiguous(), k, 1.0, None, lp2, n)
    assert np.array_equal(lp.cpu().numpy(), lp2.cpu().numpy())
    xn = x.repeat_interleave(n_per, 0).contiguous()
    ops.obs_logweight_groups(None, 0, [full, sd, None, None], xn, 0, k, 1.0, lp, M, n_per)
    assert np.array_equal(lp.cpu().numpy(), want)


# ---- 3. float64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', OR.KINDS)
def test_against_float64(lib, kind):
    hp, hx = pool(kind)
    for k, (M, n_per) in ((5, (5, 3)), (129, (3, 64)), (1030, (2, 67))):
        lp_g, lw_g, _, _ = both(lib, kind, k, M, n_per, scale=0.37)
        n = M * n_per
        xs = np.repeat(hx[:M, :k], n_per, 0)
        ref, _ = OR.row_lp(kind, [q[:n, :k] for q in hp], xs, n, k)
        np.testing.assert_allclose(lp_g, ref, **bar(ref))
        start = np.linspace(-3.0, 5.0, n)
        np.testing.assert_allclose(lw_g, start + 0.37 * ref, **bar(ref))


# ---- 4. support and untouched memory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (5, 400))
def test_support_nan_and_guards(lib, k):
    P, X = dev_pool(7)                      # Gamma(concentration, rate): x < 0 is outside, a NaN concentration gives NaN
    M, n_per, guard = 4, 9, 8
    n = M * n_per
    ps = [block(q, n, k) for q in P]
    x = block(X, M, k)
    x[2, k - 2] = -0.5                      # ONE element of ONE group outside the support
    ps[0][n_per + 4, 1] = float('nan')      # a NaN parameter in one particle row (group 1)
    buf = torch.full((n + 2 * guard,), SENTINEL, device='cuda')
    buf[guard:guard + n] = 0.25
    lpb = torch.full((n + 2 * guard,), SENTINEL, device='cuda')
    grouped(lib, 7, [(q, k, 1) for q in ps], (x, k, 1), X_BIT, k, M, n_per, scale=1.0, lw=buf[guard:guard + n],
            lp=lpb[guard:guard + n])
    for out in (buf.cpu().numpy(), lpb.cpu().numpy()):
        assert np.all(out[:guard] == SENTINEL) and np.all(out[guard + n:] == SENTINEL)
        rows = out[guard:guard + n].reshape(M, n_per)
        assert np.all(np.isneginf(rows[2])), rows[2]
        assert np.isnan(rows[1, 4])
        rest = np.ones((M, n_per), bool)
        rest[2] = False
        rest[1, 4] = False
        assert np.all(np.isfinite(rows[rest]))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_return_nonzero_and_write_nothing(lib):
    P, X = dev_pool(0)
    k, M, n_per = 5, 3, 4
    n = M * n_per
    ps = [block(q, n, k) for q in P]
    x = block(X, M, k)
    lw = torch.full((n,), SENTINEL, device='cuda')
    lp = torch.full((n,), SENTINEL, device='cuda')
    good = dict(kind=0, ps=[(q, k, 1) for q in ps], x=(x, k, 1), mask=X_BIT, k=k, M=M, n_per=n_per, lw=lw, lp=lp)
    bad = [dict(kind=5), dict(kind=2), dict(kind=99), dict(kind=-1), dict(k=0), dict(k=-3), dict(n_per=0), dict(n_per=-1),
           dict(M=-1), dict(mask=32), dict(mask=-1), dict(x=None), dict(ps=[None, (ps[1], k, 1), None, None]),
           dict(ps=[(ps[0], k, 1), None, None, None]), dict(lw=None, lp=None), dict(x=(x, -1, 1))]
    for kw in bad:
        a = dict(good, **kw)
        rc = grouped(lib, a['kind'], a['ps'], a['x'], a['mask'], a['k'], a['M'], a['n_per'], lw=a['lw'], lp=a['lp'], check=False)
        assert rc != 0, kw
        assert b'pp_obs_logweight_groups' in lib.pp_last_error(), kw
    torch.cuda.synchronize()
    assert bool((lw == SENTINEL).all()) and bool((lp == SENTINEL).all())
    # no group: nothing to do, nothing written
    assert grouped(lib, 0, good['ps'], good['x'], X_BIT, k, 0, n_per, lw=lw, lp=lp, check=False) == 0
    torch.cuda.synchronize()
    assert bool((lw == SENTINEL).all()) and bool((lp == SENTINEL).all())
    # and the good call is one
    assert grouped(lib, **{**good, 'check': False}) == 0
