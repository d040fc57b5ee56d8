"""Exact weighted quantiles and combine_duplicates, on the host side: the entry points of csrc/is_sort.hip are declared, prototyped
and exported; the workspace sizes; bad arguments are rejected before anything touches a device; the host route of Empirical.quantile
/ credible_interval / argsort / combine_duplicates on hand-made cases; and, through CPU doubles of the three operators registered
here (order_stats_ref.py, numpy) with Empirical._device_backed widened to tensors that are not on a device, quantile /
marginal().quantile / argsort / combine_duplicates / quantile_batch on a two-statement straight-line program and Marsaglia's
branching program; combine_duplicates against the live reference; median / mode / Histogram.quantile unchanged. The kernels are the
GPU's: tests/test_gpu_order_stats.py."""
import os
import re
import warnings

import numpy as np
import pytest

import histogram_ref as H
import order_stats_ref as R
import resample_ref as RR
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from is_helpers import _batch_of
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REFERENCE = os.path.isdir('/root/reference/pyprob')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_sort_workspace_bytes', 'pp_is_sort_groups', 'pp_is_quantile_groups', 'pp_is_unique_workspace_bytes',
           'pp_is_unique_groups')
EINVAL, ENOSPACE = -1, -2


@pytest.fixture
def device_style(monkeypatch):
    """Empirical._device_backed without its is_cuda clauses: a from_device Empirical over CPU tensors takes the device route, whose
    operators are the CPU doubles."""
    from pyprob_amd.distributions import Empirical
    H.register_cpu_doubles()
    R.register_cpu_doubles()
    RR.register_cpu_doubles()

    def backed(self):
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.dtype == torch.float32 and
                lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and v.numel() == lw.numel() and v.numel() > 0 and
                v.is_contiguous() and lw.is_contiguous() and os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')
    monkeypatch.setattr(Empirical, '_device_backed', backed)


def _weights(lw):
    lw = np.asarray(lw, np.float64)
    w = np.exp(lw - lw[np.isfinite(lw)].max())
    return np.where(np.isfinite(lw), w, 0.0)


def _exact_quantile(v, lw, q):
    """The inverted-cdf quantile restated once more, from the definition: particles in stable value order, the first whose
    cumulative weight reaches q T (q T == 0: the first with a positive one)."""
    v, lw = np.asarray(v, np.float64), np.asarray(lw, np.float64)
    keep = np.nonzero(np.isfinite(lw) & ~np.isnan(v))[0]
    order = keep[np.argsort(v[keep], kind='stable')]
    cum = np.cumsum(_weights(lw)[order])
    t = q * cum[-1]
    for k in range(len(order)):
        if (cum[k] >= t) if t > 0 else (cum[k] > 0):
            return v[order[k]]
    return v[order[-1]]


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
    assert int(re.search(r'#define PP_IS_SORT_TILE (\d+)', hdr).group(1)) == L.PP_IS_SORT_TILE == 2048
    block = hdr[hdr.index('Order statistics of one latent'):hdr.index('#define PP_IS_SORT_TILE')]
    for ref in ('empirical.py:714-728', 'empirical.py:809-834'):
        assert ref in block, ref
    from pyprob_amd import build, ops as P
    assert 'is_sort.hip' in build.SOURCES
    for op in ('is_sort_groups', 'is_quantile_groups', 'is_unique_groups'):
        assert hasattr(P.ops, op) and ('    %s ' % op) in P.__doc__, op


def test_workspace_bytes_are_monotone_and_zero_outside_the_envelope():
    lib = L.load()
    per = (1, 63, 2047, 2048, 2049, 4097, 70001, 10 ** 6)
    for fn in (lib.pp_is_sort_workspace_bytes, lib.pp_is_unique_workspace_bytes):
        for M in (0, 1, 3, 257, 70000):
            sizes = [fn(M, n) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (M, sizes)
        for n in per:
            sizes = [fn(M, n) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n, sizes)
        for bad in ((-1, 5), (1, 0), (1, -4), (2 ** 20, 2 ** 11)):
            assert fn(*bad) == 0, bad
        assert fn(1, 2 ** 31 - 1) > 0 and fn(2 ** 31 - 1, 1) > 0
    # a group of one tile is sorted in LDS; a longer one needs two key and two index buffers (16 bytes per particle)
    assert lib.pp_is_sort_workspace_bytes(66000, 2) == lib.pp_is_sort_workspace_bytes(1, 2048) == 256
    assert lib.pp_is_sort_workspace_bytes(1, 10 ** 6) >= 16 * 10 ** 6 > lib.pp_is_sort_workspace_bytes(1, 10 ** 6) // 2


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    M, N, Q = 3, 9000, 4
    lw, x = torch.zeros(M * N), torch.zeros(M * N)
    stats = torch.zeros(M, 6, dtype=torch.float64)
    value, lwo = torch.zeros(M * N), torch.zeros(M * N)
    index, counted = torch.zeros(M * N, dtype=torch.int32), torch.zeros(M, 2, dtype=torch.int32)
    wb = lib.pp_is_sort_workspace_bytes(M, N)
    ws = torch.zeros(wb, dtype=torch.uint8)

    def sort(lp=lw.data_ptr(), xp=x.data_ptr(), m=M, n=N, vo=value.data_ptr(), lo=lwo.data_ptr(), io=index.data_ptr(),
             co=counted.data_ptr(), w=ws.data_ptr(), b=wb, sp=stats.data_ptr()):
        return lib.pp_is_sort_groups(lp, xp, m, n, sp, vo, lo, io, co, w, b, None)
    for kw in (dict(lp=None), dict(xp=None), dict(vo=None), dict(lo=None), dict(io=None), dict(co=None), dict(w=None), dict(n=0),
               dict(n=-3), dict(m=-1), dict(m=2 ** 20, n=2 ** 11, b=2 ** 40)):
        assert sort(**kw) == EINVAL, kw
    assert b'pp_is_sort_groups' in lib.pp_last_error()
    assert sort(b=wb - 1) == ENOSPACE and sort(b=0) == ENOSPACE and b'workspace too small' in lib.pp_last_error()
    assert sort(m=0) == 0 and sort(m=0, sp=None) == 0                              # no group: nothing to launch

    cdf, q, out = torch.zeros(M * N, dtype=torch.float64), torch.zeros(Q, dtype=torch.float64), torch.zeros(M, Q, dtype=torch.float64)

    def quantile(vp=value.data_ptr(), cp=cdf.data_ptr(), kp=counted.data_ptr(), m=M, n=N, qp=q.data_ptr(), nq=Q, o=out.data_ptr()):
        return lib.pp_is_quantile_groups(vp, cp, kp, m, n, qp, nq, o, None)
    for kw in (dict(vp=None), dict(cp=None), dict(kp=None), dict(qp=None), dict(o=None), dict(n=0), dict(m=-1), dict(nq=-1),
               dict(m=2 ** 20, n=2 ** 11), dict(m=2 ** 16, n=1, nq=2 ** 15)):
        assert quantile(**kw) == EINVAL, kw
    assert b'pp_is_quantile_groups' in lib.pp_last_error()
    assert quantile(m=0) == 0 and quantile(nq=0) == 0                              # nothing to compute: no launch

    uv, mass = torch.zeros(M, N), torch.zeros(M, N, dtype=torch.int64)
    count, runs = torch.zeros(M, N, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    ub = lib.pp_is_unique_workspace_bytes(M, N)
    uws = torch.zeros(ub, dtype=torch.uint8)

    def unique(vp=value.data_ptr(), lp=lwo.data_ptr(), kp=counted.data_ptr(), m=M, n=N, vo=uv.data_ptr(), mo=mass.data_ptr(),
               co=count.data_ptr(), ro=runs.data_ptr(), w=uws.data_ptr(), b=ub):
        return lib.pp_is_unique_groups(vp, lp, kp, m, n, stats.data_ptr(), vo, mo, co, ro, w, b, None)
    for kw in (dict(vp=None), dict(lp=None), dict(kp=None), dict(vo=None), dict(mo=None), dict(co=None), dict(ro=None), dict(w=None),
               dict(n=0), dict(m=-1), dict(m=2 ** 20, n=2 ** 11, b=2 ** 40)):
        assert unique(**kw) == EINVAL, kw
    assert b'pp_is_unique_groups' in lib.pp_last_error()
    assert unique(b=ub - 1) == ENOSPACE and unique(b=0) == ENOSPACE and unique(m=0) == 0
    for t in (lw, x, value, lwo, index, counted, cdf, out, uv, mass, count, runs, ws, uws):
        assert float(t.double().abs().sum()) == 0.0


def test_reference_keys_order_like_the_values():
    """The uint32 keys of order_stats_ref order as the values do; -0.0 and +0.0 share a key; what is not counted sorts last."""
    x = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = R.keys_ref(np.zeros(8, np.float32), x)
    assert (np.diff(k.astype(np.int64)) >= 0).all() and k[3] == k[4] == 0x80000000 and (np.diff(k.astype(np.int64)) == 0).sum() == 1
    assert k.max() < 0xFFFFFFFF
    lw = np.array([0.0, np.inf, -np.inf, np.nan, 0.0], np.float32)
    assert (R.keys_ref(lw, np.array([1.0, 1.0, 1.0, 1.0, np.nan], np.float32)) == [0xBF800000, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]).all()
    v, l, i, c = R.sort_ref(lw[None], np.array([[2.0, 1.0, 1.0, 1.0, np.nan]], np.float32))
    assert i.tolist() == [[0, 1, 2, 3, 4]] and c.tolist() == [[1, 1]]


def test_host_route_on_hand_made_cases(monkeypatch):
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import Empirical

    def boom(*a, **k):
        raise AssertionError('a host-backed Empirical reached a device operator')
    for op in ('is_sort_groups', 'is_quantile_groups', 'is_unique_groups', 'is_cdf_groups'):
        monkeypatch.setattr(P.ops, op, boom, raising=False)
    # uniform weights, even and odd n: the lower middle value, and every order statistic at q = (k + 1) / n
    for n in (6, 7):
        v = [5.0, 1.0, 4.0, 2.0, 6.0, 3.0, 7.0][:n]
        emp = Empirical(values=v, log_weights=np.zeros(n))
        assert emp.quantile(0.5) == sorted(v)[(n - 1) // 2] and isinstance(emp.quantile(0.5), float)
        assert emp.quantile(0.0) == min(v) and emp.quantile(1.0) == max(v)
        got = emp.quantile([0.0, 0.2, 0.5, 1.0])
        assert got.dtype == np.float64 and got.tolist() == [_exact_quantile(v, np.zeros(n), q) for q in (0.0, 0.2, 0.5, 1.0)]
        assert emp.argsort().tolist() == np.argsort(v, kind='stable').tolist() and emp.argsort().dtype == np.int64
        assert emp.credible_interval(0.5) == (emp.quantile(0.25), emp.quantile(0.75))
        assert emp.credible_interval() == (emp.quantile(0.05), emp.quantile(0.95)) == (min(v), max(v))
    # a single heavy particle takes every quantile above its left tail
    emp = Empirical(values=[0.0, 1.0, 2.0, 3.0], log_weights=[0.0, 0.0, 20.0, 0.0])
    assert emp.quantile(0.5) == 2.0 and emp.quantile([1e-6, 0.999]).tolist() == [2.0, 2.0] and emp.quantile(0.0) == 0.0
    assert emp.quantile(1.0) == 3.0
    # leading particles of weight 0 are not the 0-quantile; weight 0 in the middle is never returned
    emp = Empirical(values=[-5.0, -4.0, 1.0, 1.5, 2.0], log_weights=[-np.inf, -np.inf, 0.0, -np.inf, 0.0])
    assert emp.quantile(0.0) == 1.0 and emp.quantile(0.5) == 1.0 and emp.quantile(0.75) == 2.0 and emp.quantile(1.0) == 2.0
    assert emp.argsort().tolist() == [2, 4]                                      # (particles without a finite log-weight are not counted)
    # -0.0 and +0.0 are one value: particle order decides, the original sign survives
    emp = Empirical(values=[0.0, -0.0, 1.0, -0.0, -1.0], log_weights=np.zeros(5))
    assert emp.argsort().tolist() == [4, 0, 1, 3, 2]
    assert emp.quantile(0.4) == 0.0 and not np.signbit(emp.quantile(0.4)) and np.signbit(emp.quantile(0.6))
    d = emp.combine_duplicates()
    assert d.get_values() == [-1.0, 0.0, 1.0] and np.allclose(d.weights_numpy(), [0.2, 0.6, 0.2], atol=1e-15)
    # NaN values are not counted; nothing counted: NaN
    emp = Empirical(values=[np.nan, 2.0, 1.0, np.nan], log_weights=[5.0, 0.0, 0.0, 0.0])
    assert emp.quantile(0.5) == 1.0 and emp.quantile(1.0) == 2.0 and emp.argsort().tolist() == [2, 1]
    assert emp.combine_duplicates().get_values() == [1.0, 2.0]
    assert np.isnan(Empirical(values=[np.nan, np.nan], log_weights=np.zeros(2)).quantile(0.5))
    # infinite values under a weight are the two ends
    emp = Empirical(values=[np.inf, 0.0, -np.inf], log_weights=np.zeros(3))
    assert emp.quantile([0.0, 0.5, 1.0]).tolist() == [-np.inf, 0.0, np.inf]
    # random weights against the definition
    rng = np.random.default_rng(11)
    v, lw = rng.integers(-3, 4, 200).astype(np.float64), rng.normal(0, 2, 200)
    emp = Empirical(values=[float(t) for t in v], log_weights=lw)
    for q in (0.0, 0.01, 0.3, 0.5, 0.77, 1.0):
        assert emp.quantile(q) == _exact_quantile(v, lw, q)
    d = emp.combine_duplicates()
    w = _weights(lw) / _weights(lw).sum()
    assert d.get_values() == sorted(set(v.tolist())) and d.metadata['op'] == 'combine_duplicates' and d.length == 7
    assert np.abs(d.weights_numpy() - [w[v == t].sum() for t in sorted(set(v.tolist()))]).max() <= 1e-14
    assert abs(d.mean - emp.mean) <= 1e-13
    # arguments
    for bad in (-0.1, 1.5, [0.5, 2.0], np.nan, [[0.5]]):
        with pytest.raises(ValueError):
            emp.quantile(bad)
    for bad in (0.0, -1.0, 1.5):
        with pytest.raises(ValueError):
            emp.credible_interval(bad)
    with pytest.raises(RuntimeError, match='not hashable'):
        Empirical(values=[torch.zeros(2), torch.ones(2)], log_weights=np.zeros(2)).combine_duplicates()
    with pytest.raises(RuntimeError, match='not hashable'):
        Empirical(values=[[1, 2], [1, 2]], log_weights=np.zeros(2)).combine_duplicates()
    with pytest.raises(ValueError):
        Empirical(values=[torch.zeros(2), torch.ones(2)], log_weights=np.zeros(2)).quantile(0.5)
    # PP_EMPIRICAL_DEVICE=0 keeps tensors on the host route; so do tensors that are not on a device
    v32, lw32 = v.astype(np.float32), lw.astype(np.float32)
    dev = Empirical.from_device(torch.from_numpy(v32), torch.from_numpy(lw32), None)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    assert dev.quantile(0.3) == _exact_quantile(v32, lw32, 0.3) and isinstance(dev.argsort(), np.ndarray)
    assert [float(t) for t in dev.combine_duplicates().get_values()] == sorted(set(v.tolist()))


def test_device_style_empirical_through_the_cpu_doubles(device_style):
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(12)
    n = 500
    v = rng.integers(-2, 3, n).astype(np.float32)
    v[:40] = rng.normal(size=40).astype(np.float32)
    lw = rng.normal(0, 2, n).astype(np.float32)
    lw[7], v[9] = -np.inf, np.nan
    emp = Empirical.from_device(torch.from_numpy(v), torch.from_numpy(lw), None)
    for k in R.calls:
        R.calls[k] = 0
    RR.calls['is_cdf_groups'] = 0
    qs = [0.0, 0.1, 0.5, 0.9, 1.0]
    got = emp.quantile(qs)
    assert got.tolist() == [_exact_quantile(v, lw, q) for q in qs]
    assert emp.quantile(0.5) == got[2] and emp.credible_interval(0.8) == (got[1], got[3])
    # sorted once per object: every call after the first is one quantile launch
    assert R.calls == {'is_sort_groups': 1, 'is_quantile_groups': 3, 'is_unique_groups': 0} and RR.calls['is_cdf_groups'] == 1
    assert not emp._host_weights_ready()
    order = emp.argsort()
    assert torch.is_tensor(order) and order.dtype == torch.int64 and order.numel() == n - 2
    keep = np.nonzero(np.isfinite(lw) & ~np.isnan(v))[0]
    assert order.tolist() == keep[np.argsort(v[keep], kind='stable')].tolist() and R.calls['is_sort_groups'] == 1
    d = emp.combine_duplicates()
    assert R.calls['is_unique_groups'] == 1 and R.calls['is_sort_groups'] == 1
    distinct = np.unique(v[keep])
    w = _weights(lw)
    want = np.array([w[keep][v[keep] == t].sum() for t in distinct])
    assert d._device_backed() and d.metadata['op'] == 'combine_duplicates' and d.length == len(distinct)
    assert np.array_equal(d._values.numpy(), distinct) and d._log_weights.dtype == torch.float32
    # (the CPU double rounds every weight to 2^-S of the heaviest: n 2^-(S+1) / W of mass, far below 1e-12 at this size)
    assert np.abs(d.weights_numpy() - want / want.sum()).max() <= 1e-12
    top = float(lw[np.isfinite(lw)].max())
    assert np.abs(np.exp(d._lw - top) - want).max() <= 1e-12 * want.max()      # log_weight = log(mass) - S ln 2 + max lw
    assert np.abs(d._log_weights.numpy() - d._lw).max() <= 1e-6 * max(1.0, np.abs(d._lw).max())
    assert abs(d.mean - float((want * distinct).sum() / want.sum())) <= 1e-6
    # growing the Empirical drops what was sorted
    emp.add(0.25, 0.0)
    emp.finalize()
    assert '_dev_sorted' not in emp.__dict__ and emp.quantile(1.0) == float(v[keep].max()) and emp.length == n + 1


def test_quantile_batch_fast_path_equals_the_loop(device_style):
    import pyprob_amd
    rng = np.random.default_rng(13)
    M, N = 5, 130
    values = torch.from_numpy(rng.integers(-4, 5, M * N).astype(np.float32))
    lw = torch.from_numpy(rng.normal(0, 2, M * N).astype(np.float32))
    lw[N + 3] = -np.inf
    posts = _batch_of(values, lw, M, N)
    qs = [0.05, 0.5, 0.95]
    loop = np.stack([p.quantile(qs) for p in posts])
    for k in R.calls:
        R.calls[k] = 0
    RR.calls['is_cdf_groups'] = 0
    fast = pyprob_amd.quantile_batch(posts, qs)
    assert R.calls == {'is_sort_groups': 1, 'is_quantile_groups': 1, 'is_unique_groups': 0} and RR.calls['is_cdf_groups'] == 1
    assert fast.shape == (M, 3) and np.array_equal(fast, loop)
    for g in range(M):
        sl = slice(g * N, (g + 1) * N)
        assert fast[g].tolist() == [_exact_quantile(values[sl].numpy(), lw[sl].numpy(), q) for q in qs]
    assert np.array_equal(pyprob_amd.quantile_batch(posts, 0.5), loop[:, 1:2])
    # anything that is not the M groups in order takes the loop
    before = dict(R.calls)
    assert np.array_equal(pyprob_amd.quantile_batch(posts[::-1], qs), loop[::-1])
    assert R.calls['is_quantile_groups'] - before['is_quantile_groups'] == M and R.calls['is_sort_groups'] == before['is_sort_groups']
    assert pyprob_amd.quantile_batch([], qs).shape == (0, 3)
    with pytest.raises(ValueError):
        pyprob_amd.quantile_batch(posts, [0.5, 1.5])


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
    qs = [0.025, 0.5, 0.975]
    assert post.quantile(qs).tolist() == [_exact_quantile(b, lw, q) for q in qs]
    assert post.marginal('mu').quantile(qs).tolist() == [_exact_quantile(a, lw, q) for q in qs]
    assert post.credible_interval(0.95) == (_exact_quantile(b, lw, 0.025), _exact_quantile(b, lw, 0.975))
    order = post.argsort()
    assert order.tolist() == np.argsort(b, kind='stable').tolist()
    # the intended use: another latent of the statement log in the order of this one
    assert np.array_equal(post.statement_log[0][A][0][order].numpy(), a[np.argsort(b, kind='stable')])
    d = post.combine_duplicates()                                                # continuous draws: nothing to combine
    assert d.length == len(np.unique(b)) and abs(d.mean - post.mean) <= 1e-5
    # quantile_batch of posteriors that are not one batched execution: the loop
    both = pyprob_amd.quantile_batch([post, post], qs)
    assert both.shape == (2, 3) and np.array_equal(both[0], post.quantile(qs)) and np.array_equal(both[1], both[0])
    lat = pyprob_amd.quantile_batch([post], qs, address='mu')
    assert np.array_equal(lat[0], post.marginal('a').quantile(qs))
    # PP_EMPIRICAL_DEVICE=0: the host route, the same particles
    want = post.quantile(qs)
    calls = dict(R.calls)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    assert np.array_equal(post.quantile(qs), want) and R.calls == calls
    assert post.argsort().tolist() == order.tolist() and isinstance(post.argsort(), np.ndarray)


def test_marsaglia_through_the_cpu_doubles(device_style):
    """A branch's address: marginal(address) orders the particles that executed it."""
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
    qs = [0.1, 0.5, 0.9]
    assert post.marginal(addrs[0]).quantile(qs).tolist() == [_exact_quantile(x0, lw, q) for q in qs]
    m = post.marginal(addrs[2])
    x1 = log[2][addrs[2]][0].numpy()[rejected]
    assert m.length == len(rejected) and m.quantile(qs).tolist() == [_exact_quantile(x1, lw[rejected], q) for q in qs]
    assert m.argsort().tolist() == np.argsort(x1, kind='stable').tolist()
    vals, plw = post._values.numpy(), post._log_weights.numpy()
    assert post.quantile(qs).tolist() == [_exact_quantile(vals, plw, q) for q in qs]
    d = post.combine_duplicates()
    assert d.length == len(np.unique(vals)) and np.array_equal(d._values.numpy(), np.unique(vals))


@pytest.mark.skipif(not HAVE_REFERENCE, reason='needs the live reference')
def test_combine_duplicates_against_the_live_reference():
    """{value: normalised weight} of a small Categorical-valued Empirical to 1e-12. The reference keeps its log-weights in FLOAT32
    (util.to_tensor's default dtype) and combines two of them by a float32 logsumexp, so its own result carries ~1e-8 wherever that
    arithmetic rounds; the two cases below are those in which it is exact: (a) every category drawn equally often under uniform
    weights - every category goes through the same float32 operations, and the normalisation (in float64) gives exactly 1 / k;
    (b) one weighted draw per category next to draws of weight 0 (rejected traces): logsumexp(a, -inf) = a without rounding, the
    log-weights themselves being float32 numbers. The order differs as documented: first occurrence there, ascending here."""
    import sys
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, '/root/reference')
    from pyprob.distributions import Empirical as RefEmpirical
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(14)
    cases = []
    v = np.repeat(np.arange(5), 6)
    rng.shuffle(v)
    cases.append((v, np.zeros(len(v))))
    v, lw = [], []
    for k, l in enumerate([0.0, -0.5, -1.25, 0.75, -2.0]):
        zeros = int(rng.integers(1, 4))
        v += [k] * (zeros + 1)
        part = [-np.inf] * zeros
        part.insert(int(rng.integers(0, zeros + 1)), l)
        lw += part
    perm = rng.permutation(len(v))
    cases.append((np.asarray(v)[perm], np.asarray(lw)[perm]))
    for v, lw in cases:
        ref = RefEmpirical(values=[int(t) for t in v], log_weights=[float(t) for t in lw]).combine_duplicates()
        rw = ref.weights.double().numpy() if torch.is_tensor(ref.weights) else np.asarray(ref.weights, np.float64)
        want = {int(k): float(w) for k, w in zip(ref.get_values(), rw)}
        mine = Empirical(values=[int(t) for t in v], log_weights=lw).combine_duplicates()
        got = {int(k): float(w) for k, w in zip(mine.get_values(), mine.weights_numpy())}
        assert sorted(got) == sorted(want) == list(range(5)) and list(got) == sorted(got)
        assert max(abs(got[k] - want[k]) for k in want) <= 1e-12, (got, want)
        assert mine.metadata['op'] == 'combine_duplicates'
    assert len(set(round(w, 6) for w in got.values())) == 5                      # (case b: five different weights)


def test_median_mode_and_histogram_quantile_are_unchanged():
    """median, mode and Histogram.quantile on a fixed seed against their values on the parent commit (recorded before the change)."""
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(2024)
    v = rng.normal(1.0, 2.0, 101)
    lw = rng.normal(0.0, 1.0, 101)
    uni = Empirical(values=[float(t) for t in v], log_weights=np.zeros(101))
    assert uni.median == RECORDED['uniform_median'] and uni.mode == RECORDED['uniform_mode']
    ten = Empirical(values=[torch.tensor(float(t)) for t in v[:100]], log_weights=np.zeros(100))
    assert ten.median == RECORDED['tensor_median']
    wei = Empirical(values=[float(t) for t in v], log_weights=lw)
    assert wei.mode == RECORDED['weighted_mode']
    torch.manual_seed(5)
    assert wei.median == RECORDED['weighted_median']                             # (still the median of 1000 resampled values)
    h = wei.histogram(20)
    assert h.quantile(0.5) == RECORDED['hist_q50'] and h.quantile([0.1, 0.9]).tolist() == RECORDED['hist_q10_q90']
    assert h.credible_interval(0.9) == tuple(RECORDED['hist_interval'])


RECORDED = {'uniform_median': 1.0978248061390683, 'uniform_mode': 3.0577137479038026, 'tensor_median': 1.0978248119354248,
            'weighted_mode': 0.5762682629085283, 'weighted_median': 1.1343927101421944, 'hist_q50': 0.90925404594868,
            'hist_q10_q90': [-0.8067017596355197, 3.427143433507882], 'hist_interval': [-1.4821862713446374, 4.42598058181426]}
