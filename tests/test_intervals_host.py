"""HPD interval, cdf and low-variance resampling, on the host side: the entry points of csrc/is_hpd.hip and
pp_is_resample_scheme_groups are declared, prototyped and exported; the workspace size; bad arguments are rejected before anything
touches a device; the numpy reference of the HPD search against an O(n^2) loop written from the definition; the host route of
Empirical.hpd_interval / cdf / resample(scheme=) on hand-made cases; the properties of the two low-variance schemes on the reference;
and, through CPU doubles of the three operators (interval_ref.py) with Empirical._device_backed widened to tensors that are not on a
device, hpd_interval / marginal().hpd_interval / cdf / hpd_batch / cdf_batch / resample_batch(scheme=) on a two-statement
straight-line program and Marsaglia's branching program; credible_interval and the default resample unchanged. The kernels are the
GPU's: tests/test_gpu_intervals.py. Every test but the last FAILS WITHOUT THE FEATURE: the parent has neither the symbols nor the
methods."""
import os
import re
import warnings

import numpy as np
import pytest

import histogram_ref as H
import interval_ref as I
import order_stats_ref as R
import resample_ref as RR
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from is_helpers import _batch_of
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_hpd_workspace_bytes', 'pp_is_hpd_groups', 'pp_is_ecdf_groups', 'pp_is_resample_scheme_groups')
EINVAL, ENOSPACE = -1, -2


@pytest.fixture
def device_style(monkeypatch):
    """Empirical._device_backed without its is_cuda clauses: a from_device Empirical over CPU tensors takes the device route, whose
    operators are the CPU doubles."""
    from pyprob_amd.distributions import Empirical
    H.register_cpu_doubles()
    R.register_cpu_doubles()
    RR.register_cpu_doubles()
    I.register_cpu_doubles()

    def backed(self):
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.dtype == torch.float32 and
                lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and v.numel() == lw.numel() and v.numel() > 0 and
                v.is_contiguous() and lw.is_contiguous() and os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')
    monkeypatch.setattr(Empirical, '_device_backed', backed)


def _sorted_cdf(v, lw):
    """(sorted values, their cumulative weights) of the counted particles, from the definition in float64."""
    v, lw = np.asarray(v, np.float64), np.asarray(lw, np.float64)
    keep = np.nonzero(np.isfinite(lw) & ~np.isnan(v))[0]
    order = keep[np.argsort(v[keep], kind='stable')]
    return v[order], np.cumsum(np.exp(lw[order] - lw[np.isfinite(lw)].max()))


def _exact_hpd(v, lw, level):
    sv, cdf = _sorted_cdf(v, lw)
    i, j = I.hpd_brute(sv, cdf, len(sv), level)
    return float(sv[i]), float(sv[j])


def _exact_cdf(v, lw, x, strict=False):
    sv, cdf = _sorted_cdf(v, lw)
    k = int(np.sum(sv < x)) if strict else int(np.sum(sv <= x))
    return 0.0 if k == 0 else float(cdf[k - 1] / cdf[-1])


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.PROTOTYPES, name
        assert hasattr(lib, name), name
        decl = hdr[hdr.rindex('%s(' % name):]
        decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
        assert decl.count(',') + 1 == len(L.PROTOTYPES[name][1]), name
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15          # additions only
    assert int(re.search(r'#define PP_IS_HPD_TILE (\d+)', hdr).group(1)) == L.PP_IS_HPD_TILE == 2048
    for k, name in enumerate(('MULTINOMIAL', 'STRATIFIED', 'SYSTEMATIC')):
        assert int(re.search(r'#define PP_RESAMPLE_%s (\d+)' % name, hdr).group(1)) == getattr(L, 'PP_RESAMPLE_' + name) == k
    # the scheme call is the multinomial call with one int32 more
    assert len(L.PROTOTYPES['pp_is_resample_scheme_groups'][1]) == len(L.PROTOTYPES['pp_is_resample_groups'][1]) + 1
    block = hdr[hdr.index('The highest-posterior-density interval and the cdf'):hdr.index('#define PP_IS_HPD_TILE')]
    assert 'neither an HPD interval nor a cdf' in block and 'empirical.py:668-728' in block
    block = hdr[hdr.index('Low-variance resampling'):hdr.index('#define PP_RESAMPLE_MULTINOMIAL')]
    assert 'empirical.py:617-637' in block
    text = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    assert all(name in text for name in SYMBOLS) and text.count('pp_abi_version() == 15') == 1
    from pyprob_amd import build, ops as P
    assert 'is_hpd.hip' in build.SOURCES
    for op in ('is_hpd_groups', 'is_ecdf_groups', 'is_resample_scheme_groups'):
        assert hasattr(P.ops, op) and ('    %s ' % op) in P.__doc__, op
    import pyprob_amd
    assert callable(pyprob_amd.hpd_batch) and callable(pyprob_amd.cdf_batch)


# ---- 2. workspace ----------------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_are_monotone_and_zero_outside_the_envelope():
    fn = L.load().pp_is_hpd_workspace_bytes
    per = (1, 63, 2047, 2048, 2049, 4097, 70001, 10 ** 6)
    for nl in (0, 1, 4):
        for M in (0, 1, 3, 257, 70000):
            sizes = [fn(M, n, nl) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (M, sizes)
        for n in per:
            sizes = [fn(M, n, nl) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n, sizes)
    sizes = [fn(3, 70001, nl) for nl in (0, 1, 2, 5, 100)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    for bad in ((-1, 5, 1), (1, 0, 1), (1, -4, 1), (1, 5, -1), (2 ** 20, 2 ** 11, 1), (2 ** 16, 1, 2 ** 15)):
        assert fn(*bad) == 0, bad
    assert fn(1, 2 ** 31 - 1, 1) > 0 and fn(2 ** 30 - 1, 1, 1) > 0
    # a group of one tile is finished by the first launch; a longer one keeps 16 bytes per (level, tile)
    assert fn(66000, 2, 4) == fn(1, 2048, 4) == 256
    assert fn(1, 600001, 4) >= 16 * 4 * 293 > fn(1, 600001, 4) - 512


# ---- 3. bad arguments ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    M, N, Q = 3, 9000, 4
    value, cdf = torch.zeros(M * N), torch.zeros(M * N, dtype=torch.float64)
    counted = torch.zeros(M, 2, dtype=torch.int32)
    level, out = torch.zeros(Q, dtype=torch.float64), torch.zeros(M, Q, 2, dtype=torch.float64)
    index = torch.zeros(M, Q, 2, dtype=torch.int32)
    wb = lib.pp_is_hpd_workspace_bytes(M, N, Q)
    ws = torch.zeros(wb, dtype=torch.uint8)

    def hpd(vp=value.data_ptr(), cp=cdf.data_ptr(), kp=counted.data_ptr(), m=M, n=N, lp=level.data_ptr(), nl=Q, o=out.data_ptr(),
            io=index.data_ptr(), w=ws.data_ptr(), b=wb):
        return lib.pp_is_hpd_groups(vp, cp, kp, m, n, lp, nl, o, io, w, b, None)
    for kw in (dict(vp=None), dict(cp=None), dict(kp=None), dict(lp=None), dict(o=None), dict(w=None), dict(n=0), dict(n=-3),
               dict(m=-1), dict(nl=-1), dict(m=2 ** 20, n=2 ** 11, b=2 ** 40), dict(m=2 ** 16, n=1, nl=2 ** 15, b=2 ** 40)):
        assert hpd(**kw) == EINVAL, kw
    assert b'pp_is_hpd_groups' in lib.pp_last_error()
    assert hpd(b=wb - 1) == ENOSPACE and hpd(b=0) == ENOSPACE and b'workspace too small' in lib.pp_last_error()
    assert hpd(m=0) == 0 and hpd(nl=0) == 0 and hpd(m=0, io=None) == 0                 # nothing to compute: no launch

    x, eo = torch.zeros(M, Q, dtype=torch.float64), torch.zeros(M, Q, dtype=torch.float64)
    rank = torch.zeros(M, Q, dtype=torch.int32)

    def ecdf(vp=value.data_ptr(), cp=cdf.data_ptr(), kp=counted.data_ptr(), m=M, n=N, xp=x.data_ptr(), nx=Q, strict=0,
             o=eo.data_ptr(), ro=rank.data_ptr()):
        return lib.pp_is_ecdf_groups(vp, cp, kp, m, n, xp, nx, strict, o, ro, None)
    for kw in (dict(vp=None), dict(cp=None), dict(kp=None), dict(xp=None), dict(o=None), dict(n=0), dict(m=-1), dict(nx=-1),
               dict(m=2 ** 20, n=2 ** 11), dict(m=2 ** 16, n=1, nx=2 ** 15)):
        assert ecdf(**kw) == EINVAL, kw
    assert b'pp_is_ecdf_groups' in lib.pp_last_error()
    assert ecdf(m=0) == 0 and ecdf(nx=0) == 0 and ecdf(m=0, ro=None) == 0

    K = 5
    idx, val = torch.zeros(M * K, dtype=torch.int64), torch.zeros(M * K)

    def draw(cp=cdf.data_ptr(), vp=value.data_ptr(), m=M, n=N, lo=0, hi=N, k=K, scheme=1, io=idx.data_ptr(), vo=val.data_ptr()):
        return lib.pp_is_resample_scheme_groups(cp, vp, m, n, lo, hi, k, scheme, 7, 0, io, vo, None)
    for scheme in (0, 1, 2):
        for kw in (dict(cp=None), dict(n=0), dict(m=-1), dict(k=-1), dict(lo=-1), dict(lo=5, hi=5), dict(hi=N + 1),
                   dict(io=None, vo=None), dict(vp=None), dict(m=2 ** 20, n=2 ** 11, hi=5), dict(m=2 ** 16, n=1, hi=1, k=2 ** 15)):
            assert draw(scheme=scheme, **kw) == EINVAL, (scheme, kw)
        assert draw(scheme=scheme, m=0) == 0 and draw(scheme=scheme, k=0) == 0
    for scheme in (3, -1, 2 ** 20):
        assert draw(scheme=scheme) == EINVAL and draw(scheme=scheme, m=0) == EINVAL, scheme
    assert b'pp_is_resample_scheme_groups' in lib.pp_last_error()
    for t in (value, cdf, counted, level, out, index, ws, x, eo, rank, idx, val):
        assert float(t.double().abs().sum()) == 0.0


# ---- 4. the reference against brute force ----------------------------------------------------------------------------------------------------
def test_hpd_reference_equals_the_brute_force_loop():
    """hpd_ref (both of its routes: all groups at once, and numpy.searchsorted per group) against an O(n^2) loop written from the
    definition - 600 random cases of n <= 40 with heavy ties, zero weights in front and inside, +-inf values and a short count."""
    rng = np.random.default_rng(41)
    levels = [1e-12, 0.3, 0.5, 0.9, 1.0]
    wrong = 0
    for case in range(600):
        n = int(rng.integers(1, 41))
        kind = case % 4
        v = np.sort(rng.integers(-2, 3, n).astype(np.float32) if kind < 2 else rng.normal(size=n).astype(np.float32))
        w = rng.exponential(1.0, n)
        if kind in (1, 3):
            w[rng.random(n) < 0.3] = 0.0
            w[:int(rng.integers(0, 3))] = 0.0
        if case % 50 == 0:
            v[0], v[-1] = -np.inf, np.inf
        if case % 77 == 0 and n > 2:
            v[-2:] = np.inf
        cdf = np.cumsum(w)
        c = int(rng.integers(max(1, n - 2), n + 1))
        counted = np.array([[c, 0]], np.int32)
        out, idx = I.hpd_ref(v[None], cdf[None], counted, levels + [0.0, 1.5, np.nan])
        pad = 2 ** 24 // n + 1          # the same group, padded beyond its count: the per-group route
        wide_v = np.concatenate([v, np.zeros(pad, np.float32)])[None]
        wide_c = np.concatenate([cdf, np.full(pad, cdf[-1])])[None]
        if case % 20 == 0:
            out2, idx2 = I.hpd_ref(wide_v, wide_c, counted, levels + [0.0, 1.5, np.nan])
            assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(idx, idx2), case
        assert (idx[0, 5:] == -1).all() and np.isnan(out[0, 5:]).all()
        for l, level in enumerate(levels):
            want = I.hpd_brute(v, cdf, c, level)
            want = (-1, -1) if want is None else want
            wrong += tuple(idx[0, l]) != want
            if want[0] >= 0:
                assert out[0, l].tolist() == [float(v[want[0]]), float(v[want[1]])]
    assert wrong == 0


# ---- 5. the host route -----------------------------------------------------------------------------------------------------------------------
def test_host_route_on_hand_made_cases(monkeypatch):
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import Empirical

    def boom(*a, **k):
        raise AssertionError('a host-backed Empirical reached a device operator')
    for op in ('is_sort_groups', 'is_hpd_groups', 'is_ecdf_groups', 'is_cdf_groups', 'is_resample_scheme_groups', 'is_resample_groups'):
        monkeypatch.setattr(P.ops, op, boom, raising=False)
    # all-equal values: width 0 at the first particle
    emp = Empirical(values=[2.5] * 9, log_weights=np.zeros(9))
    assert emp.hpd_interval(0.5) == (2.5, 2.5) and isinstance(emp.hpd_interval()[0], float)
    # level 1: the first particle of positive weight up to the last
    emp = Empirical(values=[-5.0, -4.0, 1.0, 1.5, 2.0, 9.0], log_weights=[-np.inf, -800.0, 0.0, -np.inf, 0.0, 0.5])
    assert emp.hpd_interval(1.0) == (1.0, 9.0)
    got = emp.hpd_interval([0.3, 1.0])
    assert got.dtype == np.float64 and got.shape == (2, 2) and got[1].tolist() == [1.0, 9.0]
    assert got[0].tolist() == list(_exact_hpd([-5.0, -4.0, 1.0, 1.5, 2.0, 9.0], [-np.inf, -800.0, 0.0, -np.inf, 0.0, 0.5], 0.3))
    # a one-sided posterior: the interval starts at the minimum, the equal-tailed one does not
    rng = np.random.default_rng(42)
    x = rng.exponential(1.0, 20000)
    emp = Empirical(values=[float(t) for t in x], log_weights=np.zeros(len(x)))
    lo, hi = emp.hpd_interval(0.9)
    elo, ehi = emp.credible_interval(0.9)
    assert lo == x.min() and elo > lo and hi - lo < ehi - elo and abs(hi - np.log(10.0)) < 0.1
    assert (lo, hi) == _hpd_numpy(np.sort(x), 0.9)
    # random weights and ties against the brute-force loop
    v, lw = rng.integers(-3, 4, 200).astype(np.float64), rng.normal(0, 2, 200)
    lw[5], v[11] = -np.inf, np.nan
    emp = Empirical(values=[float(t) for t in v], log_weights=lw)
    for level in (1e-12, 0.3, 0.5, 0.9, 1.0):
        assert emp.hpd_interval(level) == _exact_hpd(v, lw, level)
    # cdf: ties, strict, the ends, NaN
    for xq in (-4.0, -3.0, -0.5, 0.0, 3.0, 10.0, np.inf, -np.inf):
        assert emp.cdf(xq) == _exact_cdf(v, lw, xq) and emp.cdf(xq, strict=True) == _exact_cdf(v, lw, xq, True)
    assert emp.cdf(0.0, strict=True) < emp.cdf(0.0) and emp.cdf(-4.0) == 0.0 and emp.cdf(3.0) == 1.0 and emp.cdf(-3.0, strict=True) == 0.0
    got = emp.cdf([0.0, np.nan, 1.0])
    assert got.dtype == np.float64 and got.shape == (3,) and np.isnan(got[1]) and got[0] == emp.cdf(0.0) and isinstance(emp.cdf(0.0), float)
    # cdf is the forward map of quantile: fl(q T) / T after two roundings
    for q in (0.0, 1e-9, 0.1, 0.5, 0.77, 1.0):
        assert emp.cdf(emp.quantile(q)) >= q * (1 - 2.0 ** -51)
    # nothing counted: NaN
    none = Empirical(values=[np.nan, np.nan], log_weights=np.zeros(2))
    assert np.isnan(none.hpd_interval(0.5)).all() and np.isnan(none.cdf(0.0))
    # arguments
    for bad in (0.0, -0.1, 1.5, [0.5, 2.0], np.nan, [[0.5]]):
        with pytest.raises(ValueError):
            emp.hpd_interval(bad)
    with pytest.raises(ValueError):
        emp.cdf([[0.5]])
    with pytest.raises(ValueError):
        emp.resample(5, scheme='residual')
    tensors = Empirical(values=[torch.zeros(2), torch.ones(2)], log_weights=np.zeros(2))
    for call in (lambda: tensors.hpd_interval(0.5), lambda: tensors.cdf(0.5)):
        with pytest.raises(ValueError):
            call()
    # resample(scheme=): sorted indices, counts within one of n w, torch's generator
    vals = [float(t) for t in range(50)]
    lw = rng.normal(0, 1.5, 50)
    emp = Empirical(values=vals, log_weights=lw)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    for scheme, slack in (('systematic', 1), ('stratified', 2)):
        torch.manual_seed(3)
        r = emp.resample(400, scheme=scheme)
        drawn = np.array(r.get_values())
        assert (np.diff(drawn) >= 0).all() and r.metadata['scheme'] == scheme and r.length == 400
        counts = np.bincount(drawn.astype(int), minlength=50)
        assert (np.abs(counts - 400 * w) <= slack).all()
        torch.manual_seed(3)
        assert np.array_equal(np.array(emp.resample(400, scheme=scheme).get_values()), drawn)
    uni = Empirical(values=vals, log_weights=np.zeros(50))
    assert sorted(uni.resample(50, scheme='systematic').get_values()) == vals          # uniform weights: every particle once
    # PP_EMPIRICAL_DEVICE=0 keeps tensors on the host route
    v32, lw32 = v.astype(np.float32), rng.normal(0, 2, 200).astype(np.float32)
    dev = Empirical.from_device(torch.from_numpy(v32), torch.from_numpy(lw32), None)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    assert dev.hpd_interval(0.5) == _exact_hpd(v32, lw32, 0.5) and dev.cdf(1.0) == _exact_cdf(v32, lw32, 1.0)
    assert dev.resample(9, scheme='stratified').metadata['scheme'] == 'stratified'


def _hpd_numpy(xs, level):
    """Uniform weights: the shortest window of sorted xs by the definition (cdf k + 1, target i + fl(level n))."""
    n = len(xs)
    cdf = np.arange(1, n + 1, dtype=np.float64)
    i, j = I.hpd_ref(xs.astype(np.float32)[None], cdf[None], np.array([[n, 0]]), [level])[1][0, 0]
    return float(xs[i]), float(xs[j])


# ---- 6. the schemes' properties, on the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_out', [1, 2, 7, 1000, 4099])
def test_scheme_reference_draws_in_order_and_close_to_the_expected_counts(n_out):
    rng = np.random.default_rng(43)
    N = 257
    w = rng.exponential(1.0, (2, N))
    w[rng.random((2, N)) < 0.2] = 0.0
    cdf = np.cumsum(w, 1)
    expect = n_out * w / cdf[:, -1:]
    for scheme in (I.STRATIFIED, I.SYSTEMATIC):
        index, _ = I.resample_scheme_ref(cdf, None, 0, N, n_out, scheme, 12345, 99)
        assert index.shape == (2, n_out) and (np.diff(index, axis=1) >= 0).all()
        for g in range(2):
            counts = np.bincount(index[g], minlength=N)
            assert (counts[w[g] == 0] == 0).all()
            if scheme == I.SYSTEMATIC:
                assert (counts >= np.floor(expect[g])).all() and (counts <= np.ceil(expect[g])).all()
            else:
                assert (np.abs(counts - expect[g]) <= 2).all()
    # group g of a call is the one-group call at offset + g (systematic) or offset + g n_out (stratified)
    for scheme, step in ((I.SYSTEMATIC, 1), (I.STRATIFIED, n_out)):
        both = I.resample_scheme_ref(cdf, None, 0, N, n_out, scheme, 12345, 99)[0]
        one = I.resample_scheme_ref(cdf[1:], None, 0, N, n_out, scheme, 12345, 99 + step)[0]
        assert np.array_equal(both[1], one[0])
    assert np.array_equal(I.resample_scheme_ref(cdf, None, 3, 200, n_out, I.MULTINOMIAL, 5, 6)[0],
                          RR.resample_ref(cdf, None, 3, 200, n_out, 5, 6)[0])


# ---- 7. end to end through the CPU doubles ---------------------------------------------------------------------------------------------------
def _reset():
    for c in (I.calls, R.calls, RR.calls):
        for k in c:
            c[k] = 0


def test_batch_calls_are_one_operator_call_each_and_equal_the_loop(device_style):
    import pyprob_amd
    rng = np.random.default_rng(44)
    M, N = 5, 130
    values = torch.from_numpy(rng.integers(-4, 5, M * N).astype(np.float32))
    lw = torch.from_numpy(rng.normal(0, 2, M * N).astype(np.float32))
    lw[N + 3] = -np.inf
    posts = _batch_of(values, lw, M, N)
    levels = [0.5, 0.9, 1.0]
    loop = np.stack([p.hpd_interval(levels) for p in posts])
    pts = rng.normal(0, 3, (M, 4))
    pts[:, 0] = values.numpy().reshape(M, N)[:, 7]          # (a particle's own value: ties decide)
    cloop = np.stack([p.cdf(pts[g]) for g, p in enumerate(posts)])
    sloop = np.stack([p.cdf(pts[g], strict=True) for g, p in enumerate(posts)])
    _reset()
    fast = pyprob_amd.hpd_batch(posts, levels)
    assert I.calls['is_hpd_groups'] == 1 and R.calls['is_sort_groups'] == 1 and RR.calls['is_cdf_groups'] == 1
    assert fast.shape == (M, 3, 2) and fast.dtype == np.float64 and np.array_equal(fast, loop)
    for g in range(M):
        sl = slice(g * N, (g + 1) * N)
        assert [tuple(r) for r in fast[g]] == [_exact_hpd(values[sl].numpy(), lw[sl].numpy(), level) for level in levels]
    assert np.array_equal(pyprob_amd.hpd_batch(posts, 0.9), loop[:, 1]) and pyprob_amd.hpd_batch(posts).shape == (M, 2)
    _reset()
    fast = pyprob_amd.cdf_batch(posts, pts)
    assert I.calls['is_ecdf_groups'] == 1 and R.calls['is_sort_groups'] == 1 and RR.calls['is_cdf_groups'] == 1
    assert fast.shape == (M, 4) and np.array_equal(fast, cloop) and (sloop[:, 0] < cloop[:, 0]).all()
    assert np.array_equal(pyprob_amd.cdf_batch(posts, pts, strict=True), sloop)
    assert np.array_equal(pyprob_amd.cdf_batch(posts, pts[:, 0]), cloop[:, 0])          # [M]: one truth per posterior
    for g in range(M):
        sl = slice(g * N, (g + 1) * N)
        assert fast[g].tolist() == [_exact_cdf(values[sl].numpy(), lw[sl].numpy(), t) for t in pts[g]]
    # anything that is not the M groups in order takes the loop
    _reset()
    assert np.array_equal(pyprob_amd.hpd_batch(posts[::-1], levels), loop[::-1]) and I.calls['is_hpd_groups'] == M
    assert np.array_equal(pyprob_amd.cdf_batch(posts[::-1], pts[::-1]), cloop[::-1]) and I.calls['is_ecdf_groups'] == M
    assert R.calls['is_sort_groups'] == 0                                               # (sorted before: kept)
    assert pyprob_amd.hpd_batch([], levels).shape == (0, 3, 2) and pyprob_amd.cdf_batch([], np.zeros((0, 2))).shape == (0, 2)
    for bad in (lambda: pyprob_amd.hpd_batch(posts, [0.5, 1.5]), lambda: pyprob_amd.cdf_batch(posts, pts[:2]),
                lambda: pyprob_amd.resample_batch(posts, 5, scheme='residual')):
        with pytest.raises(ValueError):
            bad()
    # resample_batch(scheme=) of posteriors without a batch runner: the loop at offset + g (systematic) / offset + g n (stratified)
    n = 40
    cdf = RR.cdf_ref(lw.numpy().reshape(M, N))
    for scheme, step in (('systematic', 1), ('stratified', n)):
        _reset()
        out = pyprob_amd.resample_batch(posts, n, seed=21, offset=1000, scheme=scheme)
        assert I.calls['is_resample_scheme_groups'] == M and RR.calls['is_resample_groups'] == 0
        want = I.resample_scheme_ref(cdf, values.numpy(), 0, N, n, I.SCHEMES[scheme], 21, 1000)[1]
        for g, r in enumerate(out):
            one = posts[g].resample(n, seed=21, offset=1000 + g * step, scheme=scheme)
            assert np.array_equal(r._values.numpy(), one._values.numpy()) and np.array_equal(r._values.numpy(), want[g])
            assert r.metadata['scheme'] == scheme and r._device_backed()
    _reset()
    out = pyprob_amd.resample_batch(posts, n, seed=21, offset=1000)
    assert RR.calls['is_resample_groups'] == M and I.calls['is_resample_scheme_groups'] == 0 and 'scheme' not in out[0].metadata


def test_two_statement_program_through_the_cpu_doubles(device_style, monkeypatch):
    import pyprob_amd
    from test_joint_moments_host import _register_cpu_double, _two_statement_model
    _register_cpu_double()
    model = _two_statement_model()
    n = 300
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
    A, B = 'a__Normal__1', 'b__Normal__1'
    lw = post._all_log_weights.numpy()
    a, b = post.statement_log[0][A][0].numpy(), post.statement_log[1][B][0].numpy()
    levels = [0.5, 0.9]
    _reset()
    got = post.hpd_interval(levels)
    assert [tuple(r) for r in got] == [_exact_hpd(b, lw, level) for level in levels]
    assert post.hpd_interval(0.9) == tuple(got[1]) and post.hpd_interval() == tuple(got[1])
    # sorted once per object: every call after the first is one operator call
    assert I.calls['is_hpd_groups'] == 3 and R.calls['is_sort_groups'] == 1 and RR.calls['is_cdf_groups'] == 1
    assert [tuple(r) for r in post.marginal('mu').hpd_interval(levels)] == [_exact_hpd(a, lw, level) for level in levels]
    lo, hi = post.hpd_interval(0.9)
    elo, ehi = post.credible_interval(0.9)
    assert hi - lo <= ehi - elo                                                         # no interval of the mass is shorter
    pts = [float(np.median(b)), float(b.min()), float(b.max()) + 1.0, float(b.min()) - 1.0]
    assert post.cdf(pts).tolist() == [_exact_cdf(b, lw, t) for t in pts] and post.cdf(pts[2]) == 1.0 and post.cdf(pts[3]) == 0.0
    assert post.cdf(pts[1], strict=True) == 0.0 < post.cdf(pts[1])
    assert post.marginal('mu').cdf(1.0) == _exact_cdf(a, lw, 1.0)
    assert post.cdf(post.quantile(0.3)) >= 0.3 * (1 - 2.0 ** -51)
    # posteriors that are not one batched execution: the loop
    both = pyprob_amd.hpd_batch([post, post], levels)
    assert both.shape == (2, 2, 2) and np.array_equal(both[0], got) and np.array_equal(both[1], got)
    assert np.array_equal(pyprob_amd.hpd_batch([post], 0.9, address='mu')[0], np.array(post.marginal('a').hpd_interval(0.9)))
    assert np.array_equal(pyprob_amd.cdf_batch([post, post], [[pts[0]], [pts[1]]]), [[post.cdf(pts[0])], [post.cdf(pts[1])]])
    assert pyprob_amd.cdf_batch([post], [1.0], address='mu')[0] == post.marginal('mu').cdf(1.0)
    # resample(scheme=): the drawn values are device-backed, in the index order of the reference
    cdf = RR.cdf_ref(post._log_weights.numpy()[None])
    for scheme in ('stratified', 'systematic'):
        r = post.resample(64, seed=5, offset=9, scheme=scheme)
        want = I.resample_scheme_ref(cdf, post._values.numpy(), 0, n, 64, I.SCHEMES[scheme], 5, 9)
        assert r._device_backed() and np.array_equal(r._values.numpy(), want[1][0]) and r.metadata['scheme'] == scheme
        j = post.resample_joint(64, seed=5, offset=9, scheme=scheme)
        assert np.array_equal(j['index'].numpy(), want[0][0]) and (np.diff(j['index'].numpy()) >= 0).all()
        assert np.array_equal(j[B].numpy(), want[1][0]) and np.array_equal(j[A].numpy(), a[want[0][0]])
    # PP_EMPIRICAL_DEVICE=0: the host route, the same particles
    calls = dict(I.calls)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    assert np.array_equal(post.hpd_interval(levels), got) and post.cdf(pts).tolist() == [_exact_cdf(b, lw, t) for t in pts]
    assert I.calls == calls


def test_marsaglia_through_the_cpu_doubles(device_style):
    """A branch's address: marginal(address) answers over the particles that executed it."""
    from is_helpers import lockstep_network
    from test_joint_moments_host import _register_cpu_double
    _register_cpu_double()
    model, net, meta, params = lockstep_network()
    n = 200
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=3, offset=0)
    log, addrs = post.statement_log, post.addresses
    lw = post._all_log_weights.numpy()
    x0, y0 = (log[k][addrs[k]][0].numpy() for k in (0, 1))
    rejected = np.nonzero(x0 * x0 + y0 * y0 >= 1)[0]
    assert 0 < len(rejected) < n
    levels = [0.5, 0.9, 1.0]
    assert [tuple(r) for r in post.marginal(addrs[0]).hpd_interval(levels)] == [_exact_hpd(x0, lw, level) for level in levels]
    m = post.marginal(addrs[2])
    x1 = log[2][addrs[2]][0].numpy()[rejected]
    assert m.length == len(rejected)
    assert [tuple(r) for r in m.hpd_interval(levels)] == [_exact_hpd(x1, lw[rejected], level) for level in levels]
    assert m.cdf(0.0) == _exact_cdf(x1, lw[rejected], 0.0)
    vals, plw = post._values.numpy(), post._log_weights.numpy()
    assert [tuple(r) for r in post.hpd_interval(levels)] == [_exact_hpd(vals, plw, level) for level in levels]
    assert post.cdf([8.0, 9.0]).tolist() == [_exact_cdf(vals, plw, 8.0), _exact_cdf(vals, plw, 9.0)]
    r = m.resample(30, seed=2, scheme='systematic')
    assert r._device_backed() and r.length == 30 and r.metadata['scheme'] == 'systematic'
    want = I.resample_scheme_ref(RR.cdf_ref(lw[rejected][None]), x1, 0, len(x1), 30, I.SYSTEMATIC, 2, 0)[1]
    assert np.array_equal(r._values.numpy(), want[0])


# ---- 8. unchanged behaviour ------------------------------------------------------------------------------------------------------------------
def test_credible_interval_and_default_resample_are_unchanged():
    """credible_interval and the default resample on a fixed seed against their values on the parent commit (recorded before the
    change); the default metadata carries no scheme."""
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(2025)
    v = rng.normal(1.0, 2.0, 101)
    lw = rng.normal(0.0, 1.0, 101)
    emp = Empirical(values=[float(t) for t in v], log_weights=lw)
    assert emp.credible_interval(0.9) == tuple(RECORDED['interval_90']) and emp.credible_interval(0.5) == tuple(RECORDED['interval_50'])
    torch.manual_seed(5)
    r = emp.resample(6)
    assert r.get_values() == RECORDED['resample_6'] and 'scheme' not in r.metadata and r.metadata['op'] == 'resample'
    torch.manual_seed(5)
    assert emp.resample(6, scheme='multinomial').get_values() == RECORDED['resample_6']
    torch.manual_seed(5)
    assert emp.resample(4, min_index=10, max_index=60).get_values() == RECORDED['resample_range']


RECORDED = {'interval_90': [-3.8249635321027773, 4.595170812472256], 'interval_50': [-0.7834290410833975, 2.147006823728745],
            'resample_6': [4.694504919560915, 1.3858848986384147, 2.5580033365549557, 2.5488538548379065, 1.3858848986384147,
                           -0.32311348567226084],
            'resample_range': [-0.8314234623658772, 0.2008530793484934, 1.3858848986384147, 1.3858848986384147]}
