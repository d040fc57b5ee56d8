"""pp_obs_logweight (csrc/obs_logweight.hip) on the device: the elementwise identity with pp_dist_logweight for every family,
stride form and row width, the float64 restatement and the reference's recorded values, the order contract (a row's bits do not
depend on n, rows, stride form, padding or alignment), support and untouched rows, refusals, and three lock-step runs end to end."""
import os

import numpy as np
import pytest

import obs_logweight_ref as OR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

KS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 784, 1025, 4099)
NS = (1, 7, 300)
NMAX, KMAX = 300, 4099
FORMS = ('scalar', 'row', 'per', 'full', 'pad')
SENTINEL = -12345.5


def bar(ref):
    """The project's log-weight bar (tests/test_gpu_cnn.py): rtol 1e-4, atol 1e-4 * max(1, |ref|max)."""
    return dict(rtol=1e-4, atol=1e-4 * max(1.0, float(np.max(np.abs(ref)))))


@pytest.fixture(scope='module')
def lib():
    from pyprob_amd import lib as L
    return L.load()


@pytest.fixture(scope='module')
def ops():
    from pyprob_amd.ops import ops
    return ops


def pool(kind, seed=0):
    """Parameters p0..p3 and values x, [NMAX, KMAX] float32 each on the host, drawn so that ANY pairing of a value with
    parameters of other rows or columns lies inside the support (every stride form pairs them differently) and every
    log-density is finite and of moderate size."""
    g = np.random.RandomState(1000 * kind + seed)
    u = lambda a, b: g.uniform(a, b, (NMAX, KMAX)).astype(np.float32)  # noqa: E731
    z = np.zeros((NMAX, KMAX), np.float32)
    if kind == 0:
        return [u(-2, 2), u(0.3, 2), z, z], u(-3, 3)
    if kind == 1:
        return [u(-2, -1), u(1, 3), z, z], u(-0.9, 0.9)
    if kind == 3:
        return [u(0.5, 6), z, z, z], np.floor(u(0, 9))
    if kind == 4:
        return [u(0.1, 0.9), z, z, z], np.floor(u(0, 2)).clip(0, 1)
    if kind == 6:
        return [u(0.5, 3), z, z, z], u(0.05, 3)
    if kind == 7:
        return [u(0.5, 4), u(0.5, 3), z, z], u(0.05, 4)
    if kind == 8:
        return [u(0.5, 4), u(0.5, 4), u(-2, -1), u(1, 2)], u(-0.9, 0.9)
    if kind == 9:
        return [u(-1, 1), u(0.3, 1.5), z, z], u(0.1, 4)
    if kind == 10:
        return [u(0.5, 2), u(0.5, 3), z, z], u(0.1, 3)
    if kind == 11:
        return [np.floor(u(10, 21)), u(-2, 2), z, z], np.floor(u(0, 11)).clip(0, 10)
    if kind == 12:
        return [u(-3, 3), u(0.2, 8), z, z], u(-3.1, 3.1)
    return [u(-1, 1), u(0.5, 2), u(-3, -2), u(2, 3)], u(-1.9, 1.9)


_pools = {}


def dev_pool(kind):
    """The pool on the device, made once per family and left unchanged."""
    if kind not in _pools:
        p, x = pool(kind)
        _pools[kind] = ([torch.from_numpy(q).cuda() for q in p], torch.from_numpy(x).cuda())
    return _pools[kind]


class Operand:
    """One operand in one stride form, cut from a [NMAX, KMAX] pool tensor: `t` keeps the storage alive, (ptr, rs, es) is what
    pp_obs_logweight reads, `full` the same values materialised to [n, k]."""

    def __init__(self, src, n, k, form, offset=False, pad=5):
        blk = src[:n, :k]
        shift = 1 if offset else 0      # base offset by one float: 4-byte alignment only
        if form == 'scalar':
            val, self.rs, self.es = blk[:1, :1].reshape(1), 0, 0
        elif form == 'row':
            val, self.rs, self.es = blk[0].reshape(k), 0, 1
        elif form == 'per':
            val, self.rs, self.es = blk[:, 0].reshape(n), 1, 0
        elif form == 'full':
            val, self.rs, self.es = blk.reshape(n * k), k, 1
        else:                  # rows padded by `pad` floats
            val, self.rs, self.es = None, k + pad, 1
        if val is None:
            self.t = torch.full((n * (k + pad) + shift,), float('nan'), device='cuda')
            view = self.t[shift:].reshape(n, k + pad)[:, :k]
            view.copy_(blk)
            self.full = view
        else:
            self.t = torch.empty(val.numel() + shift, device='cuda')
            self.t[shift:].copy_(val)
            self.full = {'scalar': lambda: blk[:1, :1].expand(n, k), 'row': lambda: blk[:1].expand(n, k),
                         'per': lambda: blk[:, :1].expand(n, k), 'full': lambda: blk}[form]()
        self.ptr = self.t.data_ptr() + 4 * shift
        assert self.ptr % 4 == 0

    def rows2d(self, n):
        """The operand's own storage as [n, row stride] (forms with one row per particle), for planting a value."""
        return self.t[(self.ptr - self.t.data_ptr()) // 4:].reshape(n, self.rs)

    def fill(self, o):
        o.p, o.row_stride, o.elem_stride = self.ptr, self.rs, self.es


def call(lib, kind, ps, x, k, n, scale=1.0, lw=None, lp=None, rows=None, check=True):
    """pp_obs_logweight straight through the C ABI on torch's current stream."""
    from pyprob_amd import lib as L
    arr = (L.pp_obs_operand * 4)()
    for q in range(OR.N_PARAMS[kind]):
        ps[q].fill(arr[q])
    xo = L.pp_obs_operand()
    x.fill(xo)
    m = n if rows is None else rows.numel()
    rc = lib.pp_obs_logweight(kind, arr, xo, k, scale, L.ptr(lw), L.ptr(lp), L.ptr(rows), m, n, L.stream_ptr())
    if check:
        L.check(rc, 'pp_obs_logweight')
    return rc


def run(lib, kind, ps, x, k, n, **kw):
    lp = torch.full((n,), SENTINEL, device='cuda')
    call(lib, kind, ps, x, k, n, lp=lp, **kw)
    return lp


def elementwise(ops, kind, ps, x, n, k, scale=None, lw=None):
    """pp_dist_logweight's lp_out on the same values flattened to n k single elements with materialised parameters: [n, k]."""
    flat = [q.full.reshape(-1).contiguous() if i < OR.N_PARAMS[kind] else None for i, q in enumerate(ps)]
    lp = torch.empty(n * k, device='cuda')
    ops.dist_logweight(None, [kind], flat, [0 if f is None else 1 for f in flat], [x.full.reshape(-1).contiguous()], [1.0], None, lp, n * k)
    if lw is not None:
        ops.dist_logweight(lw, [kind], flat, [0 if f is None else 1 for f in flat], [x.full.reshape(-1).contiguous()], [scale], None, None,
                           n * k)
    return lp.reshape(n, k)


# ---- 1. elementwise identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', OR.KINDS)
def test_elementwise_identity_with_dist_logweight(lib, ops, kind):
    """lp_out against the float64 sum of pp_dist_logweight's per-element values, for every width, row count and stride form.
    Bound: an element passes through at most ceil(k / 64) + 8 fp32 additions (the header's order has fewer: ceil(k / 256) + 8),
    each of relative error 2^-24 on a partial sum that is at most sum_e |lp_e|: (ceil(k / 64) + 8) 2^-24 sum_e |lp_e|."""
    P, X = dev_pool(kind)
    # every planted value is finite: the restatement on the CPU over the whole pool, as paired and with the rows and columns
    # of the parameters rolled against the values (the pairings the stride forms make come from the same ranges)
    hp, hx = pool(kind)
    for shift in (0, 1):
        e = OR.elem_lp(kind, [np.roll(q.astype(np.float64), shift, (0, 1)) for q in hp[:OR.N_PARAMS[kind]]], hx.astype(np.float64))
        assert np.all(np.isfinite(e)), kind
    worst = 0.0
    for k in KS:
        for n in NS:
            for i, form in enumerate(FORMS):
                xform = ('row', 'full', 'per', 'pad')[(i + k + n) % 4]
                ps = [Operand(q, n, k, form) for q in P]
                x = Operand(X, n, k, xform)
                got = run(lib, kind, ps, x, k, n).double()
                elem = elementwise(ops, kind, ps, x, n, k).double()
                assert bool(torch.isfinite(elem).all()), (kind, k, n, form)
                want, mag = elem.sum(1), elem.abs().sum(1)
                bound = (-(-k // 64) + 8) * 2.0 ** -24 * mag
                err = (got - want).abs()
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                assert bool((err <= bound).all()), (kind, k, n, form, xform, float(err.max()), float(bound.min()))
    print('kind %d: worst error / bound = %.3f' % (kind, worst))


@pytest.mark.parametrize('kind', OR.KINDS)
def test_k1_is_bit_identical_to_dist_logweight(lib, ops, kind):
    P, X = dev_pool(kind)
    n, k, scale = 300, 1, 0.37
    for form in ('scalar', 'per'):
        ps = [Operand(q, n, k, form) for q in P]
        x = Operand(X, n, k, 'per')
        start = torch.linspace(-3.0, 5.0, n, device='cuda')
        lw_a, lw_b = start.clone(), start.clone()
        lp_a = torch.full((n,), SENTINEL, device='cuda')
        call(lib, kind, ps, x, k, n, scale=scale, lw=lw_a, lp=lp_a)
        lp_b = elementwise(ops, kind, ps, x, n, k, scale=scale, lw=lw_b).reshape(n)
        assert np.array_equal(lp_a.cpu().numpy(), lp_b.cpu().numpy()), (kind, form)
        assert np.array_equal(lw_a.cpu().numpy(), lw_b.cpu().numpy()), (kind, form)


# ---- 2. float64 and the reference's recorded values ----------------------------------------------------------------------------
@pytest.mark.parametrize('kind', OR.KINDS)
def test_against_float64_and_the_fixture(lib, kind):
    P, X = dev_pool(kind)
    for k, n in ((5, 7), (257, 300), (784, 7), (4099, 7)):
        for form in ('full', 'row', 'per'):
            ps = [Operand(q, n, k, form) for q in P]
            x = Operand(X, n, k, 'row')
            want, _ = OR.row_lp(kind, [q.full.cpu().numpy() for q in ps], x.full.cpu().numpy(), n, k)
            assert np.all(np.isfinite(want))
            np.testing.assert_allclose(run(lib, kind, ps, x, k, n).cpu().numpy().astype(np.float64), want, **bar(want))
    g = np.load(os.path.join(GOLDEN, 'vec_lp.npz'))
    p, xs, want = g['k%d_p' % kind], g['k%d_x' % kind], g['k%d_lp' % kind]
    n, k = xs.shape
    ps = [Operand(torch.from_numpy(q).cuda(), n, k, 'full') for q in p]
    got = run(lib, kind, ps, Operand(torch.from_numpy(xs).cuda(), n, k, 'full'), k, n).cpu().numpy()
    np.testing.assert_allclose(got.astype(np.float64), want.astype(np.float64), **bar(want))


# ---- 3. invariance, bit-exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 7, 13])
@pytest.mark.parametrize('k', KS)
def test_a_rows_bits_depend_on_k_and_its_values_only(lib, kind, k):
    P, X = dev_pool(kind)
    n = 300
    ps = [Operand(q, n, k, 'full') for q in P]
    x = Operand(X, n, k, 'row')
    base = run(lib, kind, ps, x, k, n).cpu().numpy()
    assert np.array_equal(run(lib, kind, ps, x, k, n).cpu().numpy(), base)                    # two consecutive runs
    # the row alone (n = 1) and inside a rows subset
    for r in (0, 137, 299):
        one = [Operand(q[r:r + 1], 1, k, 'full') for q in P]
        assert np.array_equal(run(lib, kind, one, Operand(X, 1, k, 'row'), k, 1).cpu().numpy(), base[r:r + 1]), (k, r)
    rows = torch.tensor([0, 5, 64, 137, 298, 299], dtype=torch.int64, device='cuda')
    sub = run(lib, kind, ps, x, k, n, rows=rows).cpu().numpy()
    keep = np.zeros(n, bool)
    keep[rows.cpu().numpy()] = True
    assert np.array_equal(sub[keep], base[keep]) and np.all(sub[~keep] == SENTINEL)
    # a padded row stride and bases offset by one float against the contiguous, aligned copies
    pad = run(lib, kind, [Operand(q, n, k, 'pad') for q in P], Operand(X, n, k, 'pad'), k, n).cpu().numpy()
    assert np.array_equal(pad, run(lib, kind, ps, Operand(X, n, k, 'full'), k, n).cpu().numpy())
    off = run(lib, kind, [Operand(q, n, k, 'full', offset=True) for q in P], Operand(X, n, k, 'row', offset=True), k, n).cpu().numpy()
    assert np.array_equal(off, base)
    # a shared [k] parameter against the same values materialised to [n, k]
    shared = [Operand(q, n, k, 'row') for q in P]
    mat = [Operand(q[:1].expand(n, KMAX), n, k, 'full') for q in P]
    xb = Operand(X, n, k, 'full')
    assert np.array_equal(run(lib, kind, shared, xb, k, n).cpu().numpy(), run(lib, kind, mat, xb, k, n).cpu().numpy())


def takes_16_byte_loads(kind, ps, x):
    """The host's rule for the 16-byte instance (include/pyprob_amd.h, ADDRESSING), restated: p1..p3 constant along a row, p0 and
    x each constant along a row or a run with a 16-byte aligned base and a row stride that is a multiple of 4, one of them a run."""
    def run_ok(o):
        return o.es == 1 and o.ptr % 16 == 0 and o.rs % 4 == 0
    rest = all(ps[q].es == 0 for q in range(1, OR.N_PARAMS[kind]))
    return rest and (ps[0].es == 0 or run_ok(ps[0])) and (x.es == 0 or run_ok(x)) and (ps[0].es == 1 or x.es == 1)


def spread(src, n):
    """A pool tensor whose every row repeats its first element: a per-row value, to be delivered with element stride 1."""
    return src[:n, :1].expand(n, KMAX)


# k % 4 == 0: one group, one trip, exactly four trips' worth, more than one trip (k > 1024); k % 4 != 0: a cut group after 0, 1,
# many full groups and after more than one trip
FAST_KS = (4, 8, 64, 256, 784, 1028, 4096, 5, 63, 257, 1025, 4099)


@pytest.mark.parametrize('kind', [0, 6, 7, 11, 13])
@pytest.mark.parametrize('k', FAST_KS)
def test_the_16_byte_instance_gives_the_general_instances_bits(lib, kind, k):
    """Calls that take the 16-byte instance against the same values delivered so that the general instance runs: every base
    offset by one float, and p1..p3 with element stride 1 (the per-row value repeated along the row). Rows are padded to a
    multiple of 4 floats, so k % 4 != 0 ends a row in a cut group. Then the order contract on the 16-byte instance itself: the
    row alone, a rows subset, two runs, and a -inf / NaN row next to untouched ones."""
    P, X = dev_pool(kind)
    n, NP = 300, OR.N_PARAMS[kind]
    pad = 8 - k % 4 if k % 4 else 4                     # (k + pad) % 4 == 0

    def layouts(n_, Pr, Xr, offset=False):
        """Pr, Xr: where the per-row operands come from (the pool, or one row of it); shared rows and scalars are the pool's."""
        def op(src, form):
            return Operand(src, n_, k, form, offset=offset, pad=pad)
        return {'p0 run, x row': ([op(Pr[0], 'pad')] + [op(q, 'per') for q in Pr[1:]], op(X, 'row')),
                'p0 per row, x run': ([op(Pr[0], 'per')] + [op(q, 'scalar') for q in P[1:]], op(Xr, 'pad')),
                'p0 row, x run': ([op(P[0], 'row')] + [op(q, 'per') for q in Pr[1:]], op(Xr, 'pad'))}
    fast = layouts(n, P, X)
    shifted = layouts(n, P, X, offset=True)
    base = {}
    for name, (ps, x) in fast.items():
        assert takes_16_byte_loads(kind, ps, x), name
        base[name] = run(lib, kind, ps, x, k, n).cpu().numpy()
        assert np.all(np.isfinite(base[name])), (name, k)
        assert np.array_equal(run(lib, kind, ps, x, k, n).cpu().numpy(), base[name]), name              # two consecutive runs
        ps2, x2 = shifted[name]
        assert not takes_16_byte_loads(kind, ps2, x2)
        assert np.array_equal(run(lib, kind, ps2, x2, k, n).cpu().numpy(), base[name]), (name, k, 'offset by one float')
        if NP >= 2:
            form = 'scalar' if name == 'p0 per row, x run' else 'per'
            src = [(q[:1, :1].expand(n, KMAX) if form == 'scalar' else spread(q, n)) for q in P[1:]]
            ps3 = [ps[0]] + [Operand(q, n, k, 'full') for q in src]
            assert not takes_16_byte_loads(kind, ps3, x)
            assert np.array_equal(run(lib, kind, ps3, x, k, n).cpu().numpy(), base[name]), (name, k, 'p1..p3 with element stride 1')
    # the row alone and inside a rows subset
    for r in (0, 137, 299):
        for name, (ps, x) in layouts(1, [q[r:r + 1] for q in P], X[r:r + 1]).items():
            assert takes_16_byte_loads(kind, ps, x), name
            assert np.array_equal(run(lib, kind, ps, x, k, 1).cpu().numpy(), base[name][r:r + 1]), (name, k, r)
    rows = torch.tensor([0, 5, 64, 137, 298, 299], dtype=torch.int64, device='cuda')
    keep = np.zeros(n, bool)
    keep[rows.cpu().numpy()] = True
    for name, (ps, x) in fast.items():
        sub = run(lib, kind, ps, x, k, n, rows=rows).cpu().numpy()
        assert np.array_equal(sub[keep], base[name][keep]) and np.all(sub[~keep] == SENTINEL), name
    # one element outside the support / one NaN parameter: that row alone changes
    ps, x = fast['p0 run, x row']
    e = k - 1                                            # the row's last element: in the cut group when there is one
    if kind in (0, 7, 13):
        ps[0].rows2d(n)[5, e] = float('nan')
        got = run(lib, kind, ps, x, k, n).cpu().numpy()
        assert np.isnan(got[5]) and np.array_equal(np.delete(got, 5), np.delete(base['p0 run, x row'], 5))
    ps, x = fast['p0 row, x run']
    outside = {0: None, 6: -1.0, 7: -0.5, 11: 2.5, 13: 7.0}[kind]
    if outside is not None:
        x.rows2d(n)[3, e] = outside
        got = run(lib, kind, ps, x, k, n).cpu().numpy()
        assert got[3] == -np.inf and np.array_equal(np.delete(got, 3), np.delete(base['p0 row, x run'], 3))


# ---- 4. support and untouched rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,outside', [(0, None), (1, 5.0), (3, 2.5), (6, -1.0), (7, -0.5), (9, 0.0), (13, 7.0)])
def test_support_nan_and_untouched_rows(lib, kind, outside):
    P, X = dev_pool(kind)
    n, k = 7, 257
    ps = [Operand(q, n, k, 'full') for q in P]
    x = Operand(X, n, k, 'full')
    base = run(lib, kind, ps, x, k, n).cpu().numpy()
    assert np.all(np.isfinite(base))
    if outside is not None:          # one element outside the support: that row is -inf, the others keep their bits
        x.t.reshape(n, k)[3, 200] = outside
        got = run(lib, kind, ps, x, k, n).cpu().numpy()
        assert got[3] == -np.inf and np.array_equal(np.delete(got, 3), np.delete(base, 3))
        x.t.reshape(n, k)[3, 200] = X[3, 200]
    if kind in (0, 7, 9, 13):        # a NaN parameter (where scalar_log_prob gives NaN): that row is NaN
        ps[0].t.reshape(n, k)[5, 13] = float('nan')
        got = run(lib, kind, ps, x, k, n).cpu().numpy()
        assert np.isnan(got[5]) and np.array_equal(np.delete(got, 5), np.delete(base, 5))
        ps[0].t.reshape(n, k)[5, 13] = P[0][5, 13]
    # lw alone and lp_out alone; entries outside `rows` keep the sentinel
    rows = torch.tensor([1, 4, 6], dtype=torch.int64, device='cuda')
    keep = np.zeros(n, bool)
    keep[[1, 4, 6]] = True
    lw = torch.full((n,), SENTINEL, device='cuda')
    call(lib, kind, ps, x, k, n, scale=0.5, lw=lw, rows=rows)
    lw = lw.cpu().numpy()
    assert np.all(lw[~keep] == SENTINEL)
    assert np.array_equal(lw[keep], (np.float32(SENTINEL) + np.float32(0.5) * base[keep]).astype(np.float32))
    lp = torch.full((n,), SENTINEL, device='cuda')
    call(lib, kind, ps, x, k, n, lp=lp, rows=rows)
    lp = lp.cpu().numpy()
    assert np.all(lp[~keep] == SENTINEL) and np.array_equal(lp[keep], base[keep])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(lib):
    from pyprob_amd import lib as L
    n, k = 7, 5
    P, X = dev_pool(0)
    ps = [Operand(q, n, k, 'full') for q in P]
    x = Operand(X, n, k, 'row')
    lw = torch.full((n,), SENTINEL, device='cuda')
    lp = torch.full((n,), SENTINEL, device='cuda')
    rows = torch.tensor([1, 2], dtype=torch.int64, device='cuda')

    def raw(kind=0, k_=k, lw_=lw, lp_=lp, rows_=None, m=n, n_=n, drop=None, x_=True):
        arr = (L.pp_obs_operand * 4)()
        for q in range(OR.N_PARAMS.get(kind, 2)):
            if q != drop:
                ps[q].fill(arr[q])
        xo = L.pp_obs_operand()
        if x_:
            x.fill(xo)
        return lib.pp_obs_logweight(kind, arr, xo, k_, 1.0, L.ptr(lw_), L.ptr(lp_), L.ptr(rows_), m, n_, L.stream_ptr())
    for kw in (dict(kind=2), dict(kind=5), dict(kind=14), dict(kind=-1), dict(k_=0), dict(k_=-1), dict(n_=-1, m=-1), dict(m=-1),
               dict(m=n + 1, rows_=rows), dict(m=2), dict(drop=0), dict(drop=1), dict(kind=13, drop=3), dict(x_=False),
               dict(lw_=None, lp_=None)):
        assert raw(**kw) != 0, kw
        assert b'pp_obs_logweight' in lib.pp_last_error(), kw
    assert raw(rows_=rows, m=0) == 0                           # m == 0: nothing to do, no launch
    torch.cuda.synchronize()
    assert bool((lw == SENTINEL).all()) and bool((lp == SENTINEL).all())


# ---- the operator ---------------------------------------------------------------------------------------------------------------
def test_operator_classifies_shapes(lib, ops):
    P, X = dev_pool(0)
    n, k = 7, 400
    mean, sd, x = P[0][:n, :k].contiguous(), P[1][:n, :1].contiguous(), X[0, :k].contiguous()
    want, _ = OR.row_lp(0, [mean.cpu().numpy(), sd.cpu().numpy()], x.cpu().numpy(), n, k)
    for m_ in (mean, mean.reshape(n, 1, 20, 20), P[0][:n, :k]):          # [n, k], [n, C, H, W], a padded view
        lp = torch.empty(n, device='cuda')
        ops.obs_logweight(None, 0, [m_, sd, None, None], x, k, 1.0, None, lp, n)
        np.testing.assert_allclose(lp.cpu().numpy().astype(np.float64), want, **bar(want))
    with pytest.raises(RuntimeError, match='must be a scalar'):
        ops.obs_logweight(None, 0, [mean[:, :k - 1].contiguous(), sd, None, None], x, k, 1.0, None, torch.empty(n, device='cuda'), n)


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
H = W = 20


def _patterns():
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing='ij')
    return torch.stack([0.5 + 0.4 * torch.sin((yy * (1 + c % 3) + xx * (1 + c // 3)) * 0.35) for c in range(6)])


class _Counting:
    """is_engine's operator namespace with obs_logweight counted."""

    def __init__(self, ops):
        self._ops, self.calls = ops, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def obs_logweight(self, *a):
        self.calls += 1
        return self._ops.obs_logweight(*a)


@pytest.fixture()
def counted(monkeypatch):
    from pyprob_amd import is_engine
    c = _Counting(is_engine.ops)
    monkeypatch.setattr(is_engine, 'ops', c)
    return c


def normal_sum64(x, mean, sd):
    x, mean = np.asarray(x, np.float64), np.asarray(mean, np.float64)
    return np.sum(-0.5 * ((x - mean) / sd) ** 2 - np.log(sd) - 0.5 * np.log(2 * np.pi), axis=-1)


def _captcha():
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Categorical, Normal
    patterns = _patterns()

    class Captcha(Model):
        def forward(self):
            d = pyprob.sample(Categorical([1 / 6.] * 6))
            gain = pyprob.sample(Normal(1.0, 0.1))
            pyprob.observe(Normal(patterns.to(d.device)[d.long()] * gain.reshape(-1, 1, 1), 0.1), name='img')
            return d
    image = patterns[2] * 1.05 + 0.1 * torch.randn(H, W, generator=torch.Generator().manual_seed(6))
    return Captcha('captcha-like, lock step'), patterns, image


def _values(post, j):
    return next(iter(post.statement_log[j].values()))[0]


def test_end_to_end_prior_is(counted, monkeypatch):
    from pyprob_amd import InferenceEngine
    model, patterns, image = _captcha()
    n, m = 512, 64
    monkeypatch.delenv('PP_VEC_LIKELIHOOD', raising=False)
    post = model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, lock_step=True, observe={'img': image}, seed=5)
    assert counted.calls >= 1
    lw = post._all_log_weights.cpu().numpy().astype(np.float64)
    assert lw.shape == (n,) and np.all(np.isfinite(lw))
    d, gain = (_values(post, j).cpu().numpy().astype(np.float64) for j in range(2))
    want = normal_sum64(image.double().numpy().reshape(1, -1),
                        (patterns.double().numpy()[d[:m].astype(int)] * gain[:m, None, None]).reshape(m, -1), 0.1)
    np.testing.assert_allclose(lw[:m], want, **bar(want))
    monkeypatch.setenv('PP_VEC_LIKELIHOOD', 'torch')
    before = counted.calls
    ref = model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, lock_step=True, observe={'img': image}, seed=5)
    assert counted.calls == before
    assert torch.equal(_values(ref, 1), _values(post, 1))      # the same draws
    rl = ref._all_log_weights.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(lw, rl, **bar(rl))


def test_end_to_end_with_the_inference_network(counted, monkeypatch):
    from pyprob_amd import InferenceEngine, InferenceNetwork, ObserveEmbedding
    from pyprob_amd.is_engine import ISRunner
    IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
    model, patterns, image = _captcha()
    emb = {'img': {'dim': 32, 'embedding': ObserveEmbedding.FEEDFORWARD}}
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=640, observe_embeddings=emb, batch_size=64,
                                  lstm_dim=64, seed=1)
    net = model._inference_network
    assert net._engine.spec.obs_width == H * W
    n, m = 512, 64
    monkeypatch.delenv('PP_VEC_LIKELIHOOD', raising=False)
    post = model.posterior_results(n, IC, lock_step=True, observe={'img': image}, seed=5)
    assert counted.calls >= 1
    lw = post._all_log_weights.cpu().numpy().astype(np.float64)
    assert lw.shape == (n,) and np.all(np.isfinite(lw))
    (a0, (v0, id0)), = post.statement_log[0].items()
    (a1, (v1, id1)), = post.statement_log[1].items()
    d, gain = v0.cpu().numpy().astype(np.float64), v1.cpu().numpy().astype(np.float64)
    run_ = ISRunner(net._engine)          # log q of the same values on the per-trace path (batch-1 network calls)
    run_.init(image.reshape(-1).numpy())
    dev = net._engine.device
    pr0 = torch.tensor([[1 / 6., 1 / 6.]], dtype=torch.float32, device=dev)
    pr1 = torch.tensor([[1.0, 0.1]], dtype=torch.float32, device=dev)
    want = np.zeros(m)
    img64, pat64 = image.double().numpy(), patterns.double().numpy()
    for b in range(m):
        run_.begin(1)
        _, q0 = run_.step(int(id0), None, pr0, value_in=v0[b:b + 1].contiguous())
        _, q1 = run_.step(int(id1), int(id0), pr1, value_in=v1[b:b + 1].contiguous())
        like = normal_sum64(img64.reshape(-1), (pat64[int(d[b])] * gain[b]).reshape(-1), 0.1)
        prior = np.log(1 / 6.) + (-0.5 * ((gain[b] - 1.0) / 0.1) ** 2 - np.log(0.1) - 0.5 * np.log(2 * np.pi))
        want[b] = prior + like - float(q0.item()) - float(q1.item())
    np.testing.assert_allclose(lw[:m], want, **bar(want))
    monkeypatch.setenv('PP_VEC_LIKELIHOOD', 'torch')
    before = counted.calls
    ref = model.posterior_results(n, IC, lock_step=True, observe={'img': image}, seed=5)
    assert counted.calls == before and torch.equal(_values(ref, 1), _values(post, 1))
    rl = ref._all_log_weights.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(lw, rl, **bar(rl))


def test_end_to_end_two_paths(counted, monkeypatch):
    import pyprob_amd as pyprob
    from pyprob_amd import InferenceEngine, Model
    from pyprob_amd.distributions import Normal, Uniform
    row = torch.linspace(-1.0, 1.0, 37)
    vec = row * 0.9 + 0.2 * torch.randn(37, generator=torch.Generator().manual_seed(7))

    class TwoPath(Model):
        def forward(self):
            u = pyprob.sample(Uniform(0.0, 1.0))
            if u < 0.4:
                g = pyprob.sample(Normal(1.0, 0.3))
                pyprob.observe(Normal(row.to(u.device) * g.reshape(-1, 1), 0.2), name='vec')
            else:
                pyprob.observe(Normal(row.to(u.device) * 0.5, 0.4), name='vec')
            return u
    n, m = 512, 64
    monkeypatch.delenv('PP_VEC_LIKELIHOOD', raising=False)
    post = TwoPath('two paths').posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, lock_step=True, observe={'vec': vec}, seed=9)
    assert counted.calls >= 2 and post.num_paths == 2
    lw = post._all_log_weights.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(lw))
    u, g = (_values(post, j).cpu().numpy().astype(np.float64) for j in range(2))
    r64, v64 = row.double().numpy(), vec.double().numpy()
    want = np.where(u < 0.4, normal_sum64(v64[None], r64[None] * g[:, None], 0.2), normal_sum64(v64, r64 * 0.5, 0.4))
    assert 0 < (u[:m] < 0.4).sum() < m
    np.testing.assert_allclose(lw[:m], want[:m], **bar(want[:m]))
    monkeypatch.setenv('PP_VEC_LIKELIHOOD', 'torch')
    before = counted.calls
    ref = TwoPath('two paths').posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, lock_step=True, observe={'vec': vec}, seed=9)
    assert counted.calls == before and torch.equal(_values(ref, 0), _values(post, 0))
    rl = ref._all_log_weights.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(lw, rl, **bar(rl))
