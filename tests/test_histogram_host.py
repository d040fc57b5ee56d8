"""Weighted histograms and quantiles of latents, on the host side: the entry points of csrc/is_hist.hip are declared, prototyped
and exported; pp_is_hist_shift; the workspace sizes; bad arguments are rejected before anything touches a device; the Histogram
arithmetic on a hand-made row; the host route of Empirical.histogram against numpy.histogram; and, through CPU doubles of the two
operators registered here (histogram_ref.py, float64 numpy) with Empirical._device_backed widened to tensors that are not on a
device, histogram / marginal().histogram / histogram2d / histogram_batch / min / max on a two-statement straight-line program and
Marsaglia's branching program. The kernels are the GPU's: tests/test_gpu_histogram.py."""
import os
import re
import warnings

import numpy as np
import pytest

import histogram_ref as H
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_hist_shift', 'pp_is_hist_workspace_bytes', 'pp_is_hist_groups', 'pp_is_extent_workspace_bytes',
           'pp_is_extent_groups')
EINVAL, ENOSPACE = -1, -2


@pytest.fixture
def device_style(monkeypatch):
    """Empirical._device_backed without its is_cuda clauses: a from_device Empirical over CPU tensors takes the device route, whose
    operators are the CPU doubles."""
    from pyprob_amd.distributions import Empirical
    H.register_cpu_doubles()

    def backed(self):
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.dtype == torch.float32 and
                lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and v.numel() == lw.numel() and v.numel() > 0 and
                v.is_contiguous() and lw.is_contiguous() and os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')
    monkeypatch.setattr(Empirical, '_device_backed', backed)


def _weights(lw):
    lw = np.asarray(lw, np.float64)
    w = np.exp(lw - lw.max())
    return w / w.sum()


def test_entry_points_are_declared_prototyped_and_exported():
    """FAILS WITHOUT THE FEATURE: the parent has none of the symbols."""
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
    assert int(re.search(r'#define PP_IS_HIST_MAX_BINS (\d+)', hdr).group(1)) == L.PP_IS_HIST_MAX_BINS == 2048
    block = hdr[hdr.index('Weighted histograms of one latent'):hdr.index('#define PP_IS_HIST_MAX_BINS')]
    for ref in ('empirical.py:298-309', 'empirical.py:889-914'):
        assert ref in block, ref


def test_shift_keeps_a_group_total_below_two_to_the_62():
    lib = L.load()
    want = {1: 62, 2: 61, 3: 60, 2 ** 20: 42, 2 ** 20 + 1: 41, 2 ** 31 - 1: 31}
    for n, s in want.items():
        assert lib.pp_is_hist_shift(n) == s == H.shift(n), n
        assert n * 2 ** s <= 2 ** 62 < n * 2 ** (s + 2)           # (the largest shift that fits, up to the power of two above n)
    assert lib.pp_is_hist_shift(10 ** 6) == 42
    assert lib.pp_is_hist_shift(0) == -1 and lib.pp_is_hist_shift(-5) == -1


def test_workspace_bytes_are_monotone_and_zero_outside_the_envelope():
    lib = L.load()
    per = (1, 63, 8191, 8192, 8193, 70001, 10 ** 6)
    for bins in ((1, 1), (50, 1), (2048, 1), (32, 64)):
        for M in (0, 1, 3, 257, 70000):
            sizes = [lib.pp_is_hist_workspace_bytes(M, n, *bins) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (bins, M, sizes)
            sizes = [lib.pp_is_extent_workspace_bytes(M, n) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (M, sizes)
        for n in per:
            sizes = [lib.pp_is_hist_workspace_bytes(M, n, *bins) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (bins, n, sizes)
    assert lib.pp_is_hist_workspace_bytes(1, 10 ** 6, 2048, 1) > lib.pp_is_hist_workspace_bytes(1, 10 ** 6, 50, 1) > \
        lib.pp_is_hist_workspace_bytes(1, 8192, 50, 1)
    assert lib.pp_is_extent_workspace_bytes(4, 10 ** 6) > lib.pp_is_extent_workspace_bytes(1, 10 ** 6) > 0
    for bad in ((-1, 5, 4, 1), (1, 0, 4, 1), (1, 5, 0, 1), (1, 5, 4, 0), (1, 5, 2049, 1), (1, 5, 64, 33), (2 ** 20, 2 ** 11, 4, 1)):
        assert lib.pp_is_hist_workspace_bytes(*bad) == 0, bad
    for bad in ((-1, 5), (1, 0), (2 ** 20, 2 ** 11)):
        assert lib.pp_is_extent_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    M, N, bx, by = 3, 9000, 8, 4
    lw, x, y = torch.zeros(M * N), torch.zeros(M * N), torch.zeros(M * N)
    ex, ey = torch.arange(bx + 1, dtype=torch.float64), torch.arange(by + 1, dtype=torch.float64)
    stats = torch.zeros(M, 6, dtype=torch.float64)
    out = torch.zeros(M, 2, bx * by + 3, dtype=torch.int64)
    wb = lib.pp_is_hist_workspace_bytes(M, N, bx, by)
    ws = torch.zeros(wb, dtype=torch.uint8)

    def call(lw_p=lw.data_ptr(), xp=x.data_ptr(), yp=y.data_ptr(), m=M, n=N, exp=ex.data_ptr(), bins_x=bx, sx=0, eyp=ey.data_ptr(),
             bins_y=by, sy=0, o=out.data_ptr(), w=ws.data_ptr(), b=wb):
        return lib.pp_is_hist_groups(lw_p, xp, yp, m, n, exp, bins_x, sx, eyp, bins_y, sy, stats.data_ptr(), o, w, b, None)
    assert call(lw_p=None) == EINVAL and call(xp=None) == EINVAL and call(exp=None) == EINVAL and call(o=None) == EINVAL
    assert call(w=None) == EINVAL
    assert call(n=0) == EINVAL and call(n=-3) == EINVAL and call(m=-1) == EINVAL
    assert call(m=2 ** 20, n=2 ** 11, b=2 ** 40) == EINVAL                       # M n_per = 2^31
    assert call(bins_x=0) == EINVAL and call(bins_y=0) == EINVAL and call(bins_x=-1) == EINVAL
    assert call(bins_x=64, bins_y=33, b=2 ** 40) == EINVAL                       # 2112 bins
    assert call(yp=None, eyp=None, bins_y=1, bins_x=2049, b=2 ** 40) == EINVAL
    assert call(eyp=None) == EINVAL and call(yp=None) == EINVAL                  # y without edges_y, edges_y without y
    assert call(sx=bx) == EINVAL and call(sx=-1) == EINVAL and call(sy=by) == EINVAL and call(sy=1) == EINVAL
    assert b'pp_is_hist_groups' in lib.pp_last_error()
    assert call(b=wb - 1) == ENOSPACE and call(b=0) == ENOSPACE
    assert b'workspace too small' in lib.pp_last_error()
    assert call(m=0) == 0 and call(m=0, yp=None, eyp=None, bins_y=1) == 0        # no group: nothing to launch
    ob = torch.zeros(M, 4, dtype=torch.float64)
    eb = lib.pp_is_extent_workspace_bytes(M, N)
    ews = torch.zeros(eb, dtype=torch.uint8)

    def extent(lw_p=lw.data_ptr(), xp=x.data_ptr(), m=M, n=N, o=ob.data_ptr(), w=ews.data_ptr(), b=eb):
        return lib.pp_is_extent_groups(lw_p, xp, m, n, o, w, b, None)
    assert extent(lw_p=None) == EINVAL and extent(xp=None) == EINVAL and extent(o=None) == EINVAL and extent(w=None) == EINVAL
    assert extent(n=0) == EINVAL and extent(m=-1) == EINVAL and extent(m=2 ** 20, n=2 ** 11, b=2 ** 40) == EINVAL
    assert b'pp_is_extent_groups' in lib.pp_last_error()
    assert extent(b=eb - 1) == ENOSPACE and extent(m=0) == 0
    for t in (lw, x, y, out.double(), ob, ws.double(), ews.double()):
        assert float(t.double().abs().sum()) == 0.0


def test_histogram_arithmetic_on_a_hand_made_row():
    from pyprob_amd.empirical import Histogram, _histogram_rows
    edges = np.array([[0.0, 1.0, 3.0, 4.0, 6.0]])
    # slots: four bins, below, above, NaN - fixed-point masses 100, 300, 0, 400 | 50, 100, 50 (total 1000)
    row = np.array([[[100, 300, 0, 400, 50, 100, 50], [1, 3, 0, 2, 1, 1, 1]]], np.int64)
    h = _histogram_rows(edges, row)[0]
    assert isinstance(h, Histogram) and h.particles == 9 and h.count.dtype == np.int64 and h.count.tolist() == [1, 3, 0, 2]
    assert h.mass.tolist() == [0.1, 0.3, 0.0, 0.4] and (h.below, h.above, h.nan) == (0.05, 0.1, 0.05)
    assert h.mass.sum() + h.below + h.above + h.nan == pytest.approx(1.0, abs=1e-15)
    np.testing.assert_allclose(h.density, [0.1, 0.15, 0.0, 0.2], rtol=1e-15)
    np.testing.assert_allclose(h.cdf(), [0.05, 0.15, 0.45, 0.45, 0.85], rtol=1e-15)
    # at the edges' own cumulative masses, inside a bin, across the empty bin (the leftmost point), for an array
    assert h.quantile(0.15) == pytest.approx(1.0) and h.quantile(0.45) == pytest.approx(3.0) and h.quantile(0.85) == pytest.approx(6.0)
    assert h.quantile(0.30) == pytest.approx(2.0) and h.quantile(0.65) == pytest.approx(5.0) and h.quantile(0.05) == 0.0
    np.testing.assert_allclose(h.quantile([0.1, 0.3, 0.65]), [0.5, 2.0, 5.0], rtol=1e-14)
    lo, hi = h.credible_interval(0.5)
    assert lo == pytest.approx(1.0 + 2.0 * (0.25 - 0.15) / 0.3) and hi == pytest.approx(4.0 + 2.0 * (0.75 - 0.45) / 0.4)
    assert h.mode == 5.0                                          # the centre of the bin of highest DENSITY, not mass
    # mass below / above the edges: the edge, with a warning
    with pytest.warns(RuntimeWarning, match='outside'):
        assert h.quantile(0.01) == 0.0
    with pytest.warns(RuntimeWarning, match='outside'):
        assert h.quantile(0.95) == 6.0 and h.credible_interval(0.98) == (0.0, 6.0)
    with pytest.raises(ValueError):
        h.quantile(1.5)
    # a group without weight: NaN arrays and no particle
    e = _histogram_rows(edges, np.zeros((1, 2, 7), np.int64))[0]
    assert e.particles == 0 and np.isnan(e.mass).all() and np.isnan(e.density).all() and np.isnan(e.cdf()).all()
    assert np.isnan(e.below) and np.isnan(e.quantile(0.5)) and np.isnan(e.quantile([0.1, 0.9])).all() and np.isnan(e.mode)
    assert (e.count == 0).all()
    # all the mass inside, in fixed point near 2^62: quantile(1) is the last edge without a warning
    full = _histogram_rows(edges, np.array([[[2 ** 60 + 1, 2 ** 60, 2 ** 60 - 1, 2 ** 60, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0]]], np.int64))[0]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert full.quantile(1.0) == 6.0 and full.quantile(0.0) == 0.0 and full.quantile(0.5) == pytest.approx(3.0)


def test_host_route_against_numpy_histogram(monkeypatch):
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import Empirical

    def boom(*a, **k):
        raise AssertionError('a host-backed Empirical reached a device histogram operator')
    monkeypatch.setattr(P.ops, 'is_hist_groups', boom, raising=False)
    monkeypatch.setattr(P.ops, 'is_extent_groups', boom, raising=False)
    rng = np.random.default_rng(5)
    n = 700
    v = rng.normal(2.0, 1.5, n)
    lw = rng.normal(0, 2, n)
    w = _weights(lw)
    emp = Empirical(values=[float(t) for t in v], log_weights=lw)
    for bins, rg in ((50, None), (7, None), (1, None), (13, (0.0, 3.0)), (2048, None)):
        h = emp.histogram(bins, range=rg)
        c, e = np.histogram(v, bins, range=rg)
        m, _ = np.histogram(v, bins, range=rg, weights=w)
        assert np.array_equal(h.edges, e) and np.array_equal(h.count, c) and h.count.dtype == np.int64
        assert np.abs(h.mass - m).max() <= 1e-12 and h.particles == n and h.nan == 0
        if rg is None:
            assert h.below == 0 and h.above == 0 and h.count.sum() == n       # the extremes sit in the first and the last bin
        else:
            assert h.below == pytest.approx(w[v < rg[0]].sum(), abs=1e-12) and h.above == pytest.approx(w[v > rg[1]].sum(), abs=1e-12)
        assert h.mass.sum() + h.below + h.above + h.nan == pytest.approx(1.0, abs=1e-12)
    # non-uniform edges, values exactly on edges (the last edge belongs to the last bin)
    edges = np.array([-1.0, 0.0, 0.5, 2.0, 10.0])
    v2 = np.concatenate([v, [-1.0, 0.5, 10.0, 10.0, np.nextafter(10.0, 11.0)]])
    lw2 = np.concatenate([lw, np.zeros(5)])
    h = Empirical(values=[float(t) for t in v2], log_weights=lw2).histogram(edges=edges)
    c, _ = np.histogram(v2, edges)
    m, _ = np.histogram(v2, edges, weights=_weights(lw2))
    assert np.array_equal(h.count, c) and np.abs(h.mass - m).max() <= 1e-12 and h.above > 0
    # particles without a finite weight are in no slot; NaN and infinite values under a weight have their own
    v3, lw3 = v.copy(), lw.copy()
    lw3[:3] = -np.inf, np.nan, np.inf
    v3[:3] = np.nan
    v3[3:6] = np.nan, -np.inf, np.inf
    h = Empirical(values=[float(t) for t in v3], log_weights=np.where(np.isfinite(lw3), lw3, -np.inf)).histogram(20, range=(-3, 7))
    w3 = _weights(np.where(np.isfinite(lw3), lw3, -np.inf))
    assert h.particles == n - 3 and h.nan == pytest.approx(w3[3], abs=1e-15)
    assert h.below == pytest.approx(w3[(v3 < -3)].sum(), abs=1e-12) and h.above == pytest.approx(w3[(v3 > 7)].sum(), abs=1e-12)
    # a degenerate extent is widened by 0.5 on either side, as numpy does
    h = Empirical(values=[3.0] * 5, log_weights=np.zeros(5)).histogram(4)
    assert np.array_equal(h.edges, np.histogram([3.0] * 5, 4)[1]) and h.count.tolist() == [0, 0, 5, 0]
    # PP_EMPIRICAL_DEVICE=0 keeps tensors on the host route; so do tensors that are not on a device
    dev = Empirical.from_device(torch.from_numpy(v.astype(np.float32)), torch.from_numpy(lw.astype(np.float32)), None)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    h = dev.histogram(10)
    c, e = np.histogram(v.astype(np.float32).astype(np.float64), 10)
    assert np.array_equal(h.count, c) and np.array_equal(h.edges, e)
    assert dev.min == float(v.astype(np.float32).min()) and dev.max == float(v.astype(np.float32).max())


def test_bad_edges_and_bins_raise_value_error(device_style):
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(6)
    host = Empirical(values=[float(t) for t in rng.normal(size=30)], log_weights=rng.normal(size=30))
    dev = Empirical.from_device(torch.randn(30), torch.randn(30), None)
    for emp in (host, dev):
        for kw in (dict(bins=0), dict(bins=-3), dict(bins=2049), dict(bins=2.5), dict(edges=[0.0]), dict(edges=[0.0, 1.0, 1.0]),
                   dict(edges=[0.0, 2.0, 1.0]), dict(edges=[0.0, np.inf]), dict(edges=[0.0, np.nan, 1.0]), dict(edges=[[0.0, 1.0]]),
                   dict(edges=np.arange(2050.0)), dict(range=(1.0, 0.0)), dict(range=(0.0, np.inf)),
                   dict(bins=100, range=(1e20, 1e20 + 1e5))):
            with pytest.raises(ValueError):
                emp.histogram(**kw)
        assert emp.histogram(edges=np.arange(2049.0)).mass.shape == (2048,)
    inf = Empirical(values=[0.0, np.inf, 1.0], log_weights=np.zeros(3))
    with pytest.raises(ValueError, match='range'):
        inf.histogram(5)
    assert inf.histogram(5, range=(0, 1)).above == pytest.approx(1 / 3)


def test_min_and_max_of_a_device_style_empirical(device_style):
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(7)
    v = rng.normal(size=500).astype(np.float32)
    lw = rng.normal(size=500).astype(np.float32)
    emp = Empirical.from_device(torch.from_numpy(v), torch.from_numpy(lw), None)
    H.calls['is_extent_groups'] = 0
    assert emp.min == float(np.min(v.astype(np.float64))) and emp.max == float(np.max(v.astype(np.float64)))
    assert H.calls['is_extent_groups'] == 1 and not emp._host_weights_ready()      # one launch serves both, no read-back of weights
    v2 = v.copy()
    v2[17] = np.nan
    emp = Empirical.from_device(torch.from_numpy(v2), torch.from_numpy(lw), None)
    assert np.isnan(emp.min) and np.isnan(emp.max) and np.isnan(np.min(v2))          # as numpy.min over the values
    v3 = v.copy()
    v3[5], v3[6] = -np.inf, np.inf
    emp = Empirical.from_device(torch.from_numpy(v3), torch.from_numpy(lw), None)
    assert emp.min == -np.inf and emp.max == np.inf
    # a particle the kernel skips (no finite log-weight) is one numpy.min still sees: the host route answers, as before
    lw4 = lw.copy()
    lw4[int(np.argmin(v))] = -np.inf
    emp = Empirical.from_device(torch.from_numpy(v), torch.from_numpy(lw4), None)
    assert emp.min == float(v.min()) and emp.max == float(v.max())


def _histogram_against_numpy(h, v, lw, bins, rg=None):
    fin = np.isfinite(lw)
    v, w = v[fin].astype(np.float64), _weights(lw[fin])
    c, e = np.histogram(v, bins, range=rg)
    m, _ = np.histogram(v, bins, range=rg, weights=w)
    assert np.array_equal(h.edges, e) and np.array_equal(h.count, c) and h.particles == fin.sum()
    # (the CPU double rounds every weight to 2^-S of the heaviest: n 2^-(S+1) / W of mass, far below 1e-12 at these sizes)
    assert np.abs(h.mass - m).max() <= 1e-12


def test_two_statement_program_through_the_cpu_doubles(device_style):
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
    H.calls['is_hist_groups'] = H.calls['is_extent_groups'] = 0
    h = post.histogram()
    assert H.calls == {'is_hist_groups': 1, 'is_extent_groups': 1} and len(h.mass) == 50
    _histogram_against_numpy(h, b, lw, 50)
    _histogram_against_numpy(post.histogram(16, range=(0.0, 2.0)), b, lw, 16, (0.0, 2.0))
    assert H.calls == {'is_hist_groups': 2, 'is_extent_groups': 1}                 # an explicit range needs no extent
    ha = post.marginal('mu').histogram(20)
    _histogram_against_numpy(ha, a, lw, 20)
    assert ha.quantile(0.5) == pytest.approx(post.marginal('a').mean, abs=3 * np.diff(ha.edges)[0] + post.marginal('a').stddev)
    assert post.min == float(b.min()) and post.max == float(b.max())
    # 2-D: the two latents under the call's weights
    h2 = post.histogram2d('mu', 'b', bins=(6, 5))
    w = _weights(lw)
    c2, ex, ey = np.histogram2d(a.astype(np.float64), b.astype(np.float64), (6, 5))
    m2, _, _ = np.histogram2d(a.astype(np.float64), b.astype(np.float64), (6, 5), weights=w)
    assert h2.addresses == [A, B] and np.array_equal(h2.x_edges, ex) and np.array_equal(h2.y_edges, ey)
    assert np.array_equal(h2.count, c2.astype(np.int64)) and np.abs(h2.mass - m2).max() <= 1e-12 and h2.mass.shape == (6, 5)
    assert h2.outside == 0 and h2.nan == 0 and h2.particles == n
    np.testing.assert_allclose(h2.density, m2 / (np.diff(ex)[:, None] * np.diff(ey)[None, :]), atol=1e-11)
    np.testing.assert_allclose(h2.mass.sum(1), post.marginal('a').histogram(6).mass, atol=1e-12)
    h2 = post.histogram2d('a', 'b', bins=4, range=((0.0, 2.0), (0.5, 1.5)))
    inside = (a >= 0) & (a <= 2) & (b >= 0.5) & (b <= 1.5)
    assert h2.mass.shape == (4, 4) and h2.count.sum() == inside.sum() and h2.outside == pytest.approx(w[~inside].sum(), abs=1e-12)
    with pytest.raises(ValueError):
        post.histogram2d('a', 'b', bins=(64, 33))
    with pytest.raises(KeyError):
        post.histogram2d('a', 'nope')
    # histogram_batch of posteriors that are not one batched execution: the loop
    before = dict(H.calls)
    both = pyprob_amd.histogram_batch([post, post], 12)
    assert H.calls['is_hist_groups'] - before['is_hist_groups'] == 2 and len(both) == 2
    assert all(np.array_equal(q.mass, post.histogram(12).mass) and np.array_equal(q.edges, post.histogram(12).edges) for q in both)
    lat = pyprob_amd.histogram_batch([post], 12, range=(-1.0, 3.0), address='mu')
    assert np.array_equal(lat[0].mass, post.marginal('a').histogram(12, range=(-1.0, 3.0)).mass)
    assert pyprob_amd.histogram_batch([]) == []
    assert pyprob_amd.Histogram is type(h) and pyprob_amd.Histogram2D is type(h2)


def test_marsaglia_through_the_cpu_doubles(device_style):
    """A branch's address: marginal(address).histogram bins the particles that executed it; histogram2d refuses it as joint() does."""
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
    _histogram_against_numpy(post.marginal(addrs[0]).histogram(10), x0, lw, 10)
    m = post.marginal(addrs[2])
    x1 = log[2][addrs[2]][0].numpy()[rejected]
    hb = m.histogram(8)
    assert hb.particles == len(rejected)
    _histogram_against_numpy(hb, x1, lw[rejected], 8)
    h2 = post.histogram2d(addrs[0], addrs[1], bins=(5, 3))
    assert h2.count.sum() == n and h2.count.dtype == np.int64
    with pytest.raises(ValueError, match=re.escape(addrs[2])):
        post.histogram2d(addrs[0], addrs[2])
    vals = post.values_numpy()
    _histogram_against_numpy(post.histogram(9), vals.astype(np.float32), post._log_weights.numpy(), 9)


def test_empiricals_without_a_statement_log_refuse_histogram2d():
    from pyprob_amd.distributions import Empirical
    host = Empirical(values=[0.0, 1.0], log_weights=np.zeros(2))
    dev = Empirical.from_device(torch.zeros(20), torch.zeros(20), None)
    for emp in (host, dev):
        with pytest.raises(AttributeError, match='no statement log'):
            emp.histogram2d('a', 'b')
