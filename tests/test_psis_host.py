"""Pareto-smoothed importance sampling above and below the C ABI without a device: the symbols and their argument checks, the numpy
restatement (tests/psis_ref.py) against a plain loop and against scipy's generalised Pareto distribution, the host route of
Empirical.pareto_k / psis, and the device route and the batch calls through the CPU doubles of the operators."""
import os
import re
import warnings

import numpy as np
import pytest

import histogram_ref as H
import interval_ref as I
import order_stats_ref as R
import psis_ref as PR
import resample_ref as RR
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from is_helpers import _batch_of
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_psis_workspace_bytes', 'pp_is_psis_groups')
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
    PR.register_cpu_doubles()

    def backed(self):
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.dtype == torch.float32 and
                lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and v.numel() == lw.numel() and v.numel() > 0 and
                v.is_contiguous() and lw.is_contiguous() and os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')
    monkeypatch.setattr(Empirical, '_device_backed', backed)


def _reset():
    for c in (PR.calls, R.calls, RR.calls):
        for k in c:
            c[k] = 0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _pareto_lw(rng, n, k):
    return -k * np.log(1.0 - rng.random(n))          # weights U^-k: a Pareto tail of shape k


# ---- 1. symbols and the ABI ------------------------------------------------------------------------------------------------------------------
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
    assert int(re.search(r'#define PP_IS_PSIS_WIDTH (\d+)', hdr).group(1)) == L.PP_IS_PSIS_WIDTH == PR.WIDTH == 8
    block = hdr[hdr.index('Pareto-smoothed importance weights'):hdr.index('#define PP_IS_PSIS_WIDTH')]
    assert 'The reference has no counterpart' in block and 'empirical.py:758-766' in block
    text = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    assert all(name in text for name in SYMBOLS) and text.count('pp_abi_version() == 15') == 1
    from pyprob_amd import build, ops as P
    assert 'is_psis.hip' in build.SOURCES
    assert hasattr(P.ops, 'is_psis_groups') and '    is_psis_groups ' in P.__doc__
    import pyprob_amd
    assert callable(pyprob_amd.pareto_k_batch) and callable(pyprob_amd.psis_batch) and pyprob_amd.PsisFit is not None


def test_workspace_bytes_follow_the_largest_tail_and_are_zero_outside_the_envelope():
    fn = L.load().pp_is_psis_workspace_bytes
    per = (1, 20, 24, 257, 2048, 2049, 70001, 600001, 10 ** 6)
    for tail in (0, 5, 10000):
        for M in (0, 1, 3, 257, 70000):
            sizes = [fn(M, n, tail) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (M, tail, sizes)
        for n in per:
            sizes = [fn(M, n, tail) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n, tail, sizes)
    for bad in ((-1, 5, 0), (1, 0, 0), (1, -4, 0), (1, 5, -1), (2 ** 20, 2 ** 11, 0)):
        assert fn(*bad) == 0, bad
    assert fn(1, 2 ** 31 - 1, 0) > 0 and fn(2 ** 31 - 1, 1, 0) > 0
    # 8 bytes per exceedance of the longest tail a group can have (3 sqrt(10^6) = 3000) and 16 per grid point (30 + 54)
    assert 8 * 3000 + 16 * 84 <= fn(1, 10 ** 6, 0) <= 8 * 3000 + 16 * 84 + 32 + 5 * 256
    assert fn(1, 10 ** 6, 100000) >= 8 * 100000 > fn(1, 10 ** 6, 0)
    assert fn(1, 50, 100000) <= 8 * 50 + 16 * 37 + 32 + 5 * 256          # (a tail is never longer than the group)


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    M, N = 3, 9000
    ls, index = torch.zeros(M * N), torch.zeros(M * N, dtype=torch.int32)
    counted = torch.zeros(M, 2, dtype=torch.int32)
    lw_out, out = torch.zeros(M * N), torch.zeros(M, 8, dtype=torch.float64)
    wb = lib.pp_is_psis_workspace_bytes(M, N, 0)
    ws = torch.zeros(wb, dtype=torch.uint8)

    def psis(lp=ls.data_ptr(), ip=index.data_ptr(), kp=counted.data_ptr(), m=M, n=N, sp=None, tail=0, wo=lw_out.data_ptr(),
             o=out.data_ptr(), w=ws.data_ptr(), b=wb):
        return lib.pp_is_psis_groups(lp, ip, kp, m, n, sp, tail, wo, o, w, b, None)
    for kw in (dict(lp=None), dict(ip=None), dict(kp=None), dict(o=None), dict(w=None), dict(n=0), dict(n=-3), dict(m=-1),
               dict(tail=-1), dict(m=2 ** 20, n=2 ** 11, b=2 ** 40)):
        assert psis(**kw) == EINVAL, kw
        assert b'pp_is_psis_groups' in lib.pp_last_error()
    assert psis(tail=-1) == EINVAL and b'tail >= 0' in lib.pp_last_error()
    assert psis(b=wb - 1) == ENOSPACE and psis(b=0) == ENOSPACE and b'workspace too small' in lib.pp_last_error()
    assert psis(tail=5000, b=wb) == ENOSPACE                                            # (a longer tail needs more)
    assert psis(m=0) == 0 and psis(m=0, wo=None) == 0                                   # nothing to compute: no launch
    for t in (ls, index, counted, lw_out, out, ws):
        assert float(t.double().abs().sum()) == 0.0


# ---- 2. the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_plain_loop():
    rng = np.random.default_rng(11)
    cases = [np.sort(_pareto_lw(rng, n, k).astype(np.float32)) for n in (24, 40, 150) for k in (0.3, 1.1)]
    cases.append(np.sort(rng.integers(0, 5, 60).astype(np.float32)))                    # ties at the cutoff
    cases.append(np.sort(rng.integers(0, 40, 60).astype(np.float32)))
    cases.append(np.full(30, 2.5, np.float32))                                          # all equal: no fit
    cases.append(np.sort(rng.normal(0, 1, 20).astype(np.float32)))                      # n_t = 4: no fit
    cases.append(np.zeros(0, np.float32))
    fitted = 0
    for s in cases:
        for tail in (0, 7):
            row = PR.fit_group(s, tail, np.float64)[0]
            loop = np.array(PR.fit_loop(s, tail), np.float64)
            assert np.array_equal(_bits(row), _bits(loop)), (len(s), tail, row, loop)
            fitted += int(row[3] > 0)
    assert fitted >= 10
    row = PR.fit_group(np.full(30, 2.5, np.float32), 0)[0]
    assert row[0] == np.inf and np.isnan(row[1]) and row[3] == 0 and row[6] == 30 and row[7] == 2.5
    row = PR.fit_group(np.sort(rng.normal(0, 1, 20).astype(np.float32)), 0)[0]
    assert row[0] == np.inf and row[2] == 4 and row[4] == 16                            # (n = 4 <= 4)
    assert PR.fit_group(np.sort(rng.normal(0, 1, 24).astype(np.float32)), 0)[0][2] == 5


@pytest.mark.parametrize('k,seed', [(-0.3, 1), (0.3, 2), (0.7, 3), (1.2, 4)])
def test_restatement_recovers_the_shape_of_scipys_generalised_pareto(k, seed):
    """kappa (before the prior) within four asymptotic standard deviations (1 + k) / sqrt(n) of the maximum-likelihood shape
    estimator, on exceedances drawn directly."""
    from scipy.stats import genpareto
    n = 3000
    y = np.sort(genpareto.rvs(k, scale=1.0, size=n, random_state=np.random.default_rng(seed)))
    kappa, sigma, m = PR.gpd_fit(y, np.float64)
    print('k %.1f: kappa %.4f sigma %.4f m %d bound %.4f' % (k, kappa, sigma, m, 4 * (1 + k) / np.sqrt(n)))
    assert m == 30 + 54 and abs(kappa - k) <= 4 * (1 + k) / np.sqrt(n) and abs(sigma - 1.0) < 0.2
    kL, sL, _ = PR.gpd_fit(y, np.longdouble)
    assert abs(float(kL) - kappa) <= 1e-11 and abs(float(sL) - sigma) <= 1e-11


# ---- 3. the host route -----------------------------------------------------------------------------------------------------------------------
def test_host_route_of_pareto_k_and_psis(monkeypatch):
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import Empirical, PsisFit

    def boom(*a):
        raise AssertionError('the host route calls no operator')
    monkeypatch.setattr(P.ops, 'is_psis_groups', boom, raising=False)
    rng = np.random.default_rng(5)
    n = 2000
    for k, warns in ((0.2, False), (1.2, True)):
        lw = _pareto_lw(rng, n, k).astype(np.float32).astype(np.float64)
        lw[7], lw[11] = -np.inf, -np.inf
        vals = rng.normal(size=n)
        e = Empirical(values=list(vals), log_weights=list(lw))
        ls, idx, cnt = PR.sort_by_lw(lw.astype(np.float32)[None])
        want_lw, want = PR.psis_ref(ls, idx, cnt, 0, np.float64)
        khat = e.pareto_k()
        assert isinstance(khat, float) and khat == want[0, 0] and (khat > 0.7) == warns
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            sm = e.psis()
        said = [str(w.message) for w in caught if issubclass(w.category, UserWarning) and 'Pareto smoothing' in str(w.message)]
        assert len(said) == (1 if warns else 0) and all('%.3f' % khat in s and '0.7' in s for s in said)
        f = sm.fit
        assert isinstance(f, PsisFit) and (f.khat, f.sigma, f.tail, f.grid, f.log_cutoff, f.count) == \
            (want[0, 0], want[0, 1], int(want[0, 2]), int(want[0, 3]), want[0, 5], n - 2)
        assert f.tail == 135 and f.grid == 41 and f.ess_before == e.effective_sample_size and f.ess_after == sm.effective_sample_size
        assert sm.metadata['op'] == 'psis' and sm.metadata['khat'] == khat and sm.length == n
        got = sm.log_weights_numpy()
        assert np.array_equal(_bits(got.astype(np.float32)), _bits(want_lw[0]))
        changed = np.nonzero(_bits(got) != _bits(lw))[0]
        assert 0 < len(changed) <= f.tail and (lw[changed] > f.log_cutoff).all()          # non-tail bits unchanged
        assert got[7] == -np.inf and got[11] == -np.inf and np.array_equal(sm.values_numpy(), vals)
        assert got[np.isfinite(got)].max() <= lw[np.isfinite(lw)].max()
        assert e.pareto_k(50) == PR.psis_ref(ls, idx, cnt, 50, np.float64)[1][0, 0] and e.psis(50).fit.tail == 50
    # no fit: +inf, the weights unchanged, the warning says so
    for lw in (np.full(100, 0.5), rng.normal(size=20), np.array([0.0])):
        e = Empirical(values=list(np.arange(len(lw), dtype=np.float64)), log_weights=list(lw))
        assert e.pareto_k() == np.inf
        with pytest.warns(UserWarning, match='no tail could be fitted'):
            sm = e.psis()
        assert sm.fit.khat == np.inf and np.isnan(sm.fit.sigma) and np.array_equal(sm.log_weights_numpy(), lw)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            e.pareto_k(bad)
        with pytest.raises(ValueError):
            e.psis(bad)


# ---- 4. the device route and the batch calls through the CPU doubles -------------------------------------------------------------------------
def test_batch_calls_are_one_operator_call_each_and_equal_the_loop(device_style):
    import pyprob_amd
    rng = np.random.default_rng(44)
    M, N = 5, 400
    values = torch.from_numpy(rng.normal(size=M * N).astype(np.float32))
    lw = torch.from_numpy(np.concatenate([_pareto_lw(rng, N, k) for k in (0.1, 0.5, 0.9, 1.3, 0.3)]).astype(np.float32))
    lw[N + 3] = -np.inf
    posts = _batch_of(values, lw, M, N)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loop_k = np.array([p.pareto_k() for p in posts])
        loop = [p.psis() for p in posts]
        assert R.calls['is_sort_groups'] >= M and '_dev_lw_sorted' in posts[0].__dict__
        _reset()
        fast_k = pyprob_amd.pareto_k_batch(posts)
        assert PR.calls['is_psis_groups'] == 1 and R.calls['is_sort_groups'] == 1
        assert fast_k.dtype == np.float64 and fast_k.shape == (M,) and np.array_equal(_bits(fast_k), _bits(loop_k))
        ls, idx, cnt = PR.sort_by_lw(lw.numpy().reshape(M, N))
        assert np.array_equal(fast_k, PR.psis_ref(ls, idx, cnt, 0)[1][:, 0]) and (fast_k > 0.7).any() and (fast_k < 0.7).any()
        _reset()
        fast = pyprob_amd.psis_batch(posts)
        assert PR.calls['is_psis_groups'] == 1 and R.calls['is_sort_groups'] == 1 and len(fast) == M
        for f, l, p in zip(fast, loop, posts):
            assert np.array_equal(_bits(f._log_weights.numpy()), _bits(l._log_weights.numpy())) and f._device_backed()
            assert (f.fit.khat, f.fit.sigma, f.fit.tail, f.fit.ess_after) == (l.fit.khat, l.fit.sigma, l.fit.tail, l.fit.ess_after)
            assert f.metadata['op'] == 'psis' and f.length == p.length
        assert np.array_equal(pyprob_amd.pareto_k_batch(posts, tail=30), np.array([p.pareto_k(30) for p in posts]))
        # anything that is not the M groups in order takes the loop
        _reset()
        assert np.array_equal(pyprob_amd.pareto_k_batch(posts[::-1]), loop_k[::-1]) and PR.calls['is_psis_groups'] == M
        assert R.calls['is_sort_groups'] == 0                                           # (sorted before: kept)
        _reset()
        mixed = pyprob_amd.psis_batch([posts[1], posts[1], posts[0]])
        assert PR.calls['is_psis_groups'] == 3 and np.array_equal(_bits(mixed[2]._log_weights.numpy()), _bits(loop[0]._log_weights.numpy()))
    assert pyprob_amd.pareto_k_batch([]).shape == (0,) and pyprob_amd.psis_batch([]) == []
    with pytest.raises(ValueError):
        pyprob_amd.pareto_k_batch(posts, tail=0)


def test_two_statement_program_keeps_its_statement_log(device_style, monkeypatch):
    import pyprob_amd
    from test_joint_moments_host import _register_cpu_double, _two_statement_model
    _register_cpu_double()
    model = _two_statement_model()
    n = 300
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
        A = 'a__Normal__1'
        lw = post._all_log_weights.numpy()
        a = post.statement_log[0][A][0].numpy().astype(np.float64)
        ls, idx, cnt = PR.sort_by_lw(lw[None])
        want_lw, want = PR.psis_ref(ls, idx, cnt, 0)
        _reset()
        assert post.pareto_k() == want[0, 0] and post.pareto_k() == want[0, 0]
        sm = post.psis()
        # sorted by log-weight once per object: every call is one operator call
        assert PR.calls['is_psis_groups'] == 3 and R.calls['is_sort_groups'] == 1
    assert sm.fit.khat == want[0, 0] and sm.fit.tail == int(want[0, 2]) and sm.metadata['op'] == 'psis' and sm.name == post.name
    assert np.array_equal(_bits(sm._all_log_weights.numpy()), _bits(want_lw[0]))
    assert sm._all_log_weights.data_ptr() == sm._log_weights.data_ptr() and sm._all_values is post._all_values
    assert sm.statement_log is post.statement_log and sm.statement_names == post.statement_names and sm.num_paths == post.num_paths
    assert (_bits(want_lw[0]) != _bits(lw)).any()
    w = np.exp(want_lw[0].astype(np.float64) - want_lw[0].astype(np.float64).max())
    w0 = np.exp(lw.astype(np.float64) - lw.astype(np.float64).max())
    ma = sm.marginal('mu')
    assert abs(ma.mean - float((w * a).sum() / w.sum())) <= 1e-6 * max(1.0, abs(ma.mean))
    assert abs(post.marginal('mu').mean - float((w0 * a).sum() / w0.sum())) <= 1e-6
    assert ma.mean != post.marginal('mu').mean and sm.joint().count == n
    # not one batched execution: the loop
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.array_equal(pyprob_amd.pareto_k_batch([post, post]), [want[0, 0]] * 2)
        # PP_EMPIRICAL_DEVICE=0: the host route, the same particles
        calls = dict(PR.calls)
        monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
        assert post.pareto_k() == want[0, 0]
        assert np.array_equal(_bits(post.psis().log_weights_numpy().astype(np.float32)), _bits(want_lw[0]))
    assert PR.calls == calls


def test_a_call_that_dropped_particles_is_smoothed_over_all_of_them(device_style):
    from pyprob_amd.distributions import Empirical
    RR.register_cpu_doubles()
    rng = np.random.default_rng(9)
    n = 500
    all_lw = _pareto_lw(rng, n, 0.6).astype(np.float32)
    all_lw[[3, 77]] = [-np.inf, np.nan]
    all_values = rng.normal(size=n).astype(np.float32)
    ok = np.isfinite(all_lw)
    post = Empirical.from_device(torch.from_numpy(all_values[ok]), torch.from_numpy(all_lw[ok]), None)
    post._all_values, post._all_log_weights = torch.from_numpy(all_values), torch.from_numpy(all_lw)
    ls, idx, cnt = PR.sort_by_lw(all_lw[None])
    want_lw, want = PR.psis_ref(ls, idx, cnt, 0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sm = post.psis()
    assert sm.length == n - 2 and sm.fit.count == n - 2 and sm.fit.khat == want[0, 0]
    assert np.array_equal(_bits(sm._all_log_weights.numpy()), _bits(want_lw[0]))            # (the dropped set is unchanged)
    assert np.array_equal(_bits(sm._log_weights.numpy()), _bits(want_lw[0][ok])) and np.array_equal(sm._values.numpy(), all_values[ok])


def test_add_drops_the_sort_by_log_weight(device_style):
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(2)
    n = 200
    lw = _pareto_lw(rng, n, 0.4).astype(np.float32)
    e = Empirical.from_device(torch.from_numpy(rng.normal(size=n).astype(np.float32)), torch.from_numpy(lw), None)
    k = e.pareto_k()
    assert '_dev_lw_sorted' in e.__dict__
    top = np.float32(lw.max() + np.float32(3.0))
    e.add(0.25, log_weight=float(top))
    assert '_dev_lw_sorted' not in e.__dict__
    e.finalize()
    ls, idx, cnt = PR.sort_by_lw(np.append(lw, top)[None])
    assert e.pareto_k() == PR.psis_ref(ls, idx, cnt, 0)[1][0, 0] != k
