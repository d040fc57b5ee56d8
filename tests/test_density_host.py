"""Empirical.density_estimate (weighted Gaussian-mixture EM), on the host side: the entry points of csrc/is_gmm.hip are declared,
prototyped and exported and PP_IS_GMM_WIDTH agrees between header and binding; the workspace grows with the call; bad arguments are
rejected before anything touches a device; gmm_ref.py reproduces scikit-learn's fit of the recorded golden; the host route (float64
numpy) of density_estimate on hand-made cases - overrides, num_samples, the non-convergence warning; and, through a CPU double of the
operator registered here (gmm_ref.py) with Empirical._device_backed widened to tensors that are not on a device, density_estimate /
marginal().density_estimate / density_estimate_batch on a two-statement straight-line program and Marsaglia's branching program;
the fitted Mixture as the prior of a second lock-step call. The kernel is the GPU's: tests/test_gpu_density.py."""
import os
import re
import warnings

import numpy as np
import pytest

import gmm_ref as G
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from is_helpers import _batch_of
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_gmm_workspace_bytes', 'pp_is_gmm_groups')
EINVAL, ENOSPACE = -1, -2
# gmm_ref against scikit-learn 1.7.2 on the golden, measured on the build machine: at most 4.1e-13 absolute over the parameters of
# the four cases (K = 5), 4.0e-15 on the lower bound; the bound is 100 times the larger
GOLDEN_BOUND = 4.1e-11


@pytest.fixture
def device_style(monkeypatch):
    """Empirical._device_backed without its is_cuda clauses: a from_device Empirical over CPU tensors takes the device route, whose
    operators are the CPU doubles."""
    import histogram_ref as H
    import order_stats_ref as R
    import resample_ref as RR
    from pyprob_amd.distributions import Empirical
    H.register_cpu_doubles()
    R.register_cpu_doubles()
    RR.register_cpu_doubles()
    G.register_cpu_doubles()

    def backed(self):
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.dtype == torch.float32 and
                lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and v.numel() == lw.numel() and v.numel() > 0 and
                v.is_contiguous() and lw.is_contiguous() and os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')
    monkeypatch.setattr(Empirical, '_device_backed', backed)


def _fit_row(mix):
    f = mix.fit
    return np.concatenate([f.weights, f.means, f.stddevs ** 2, [f.lower_bound, f.n_iter, f.converged]])


def _close(mix, row, K, rel):
    """The MixtureFit against a gmm_ref row: parameters and lower bound to `rel`, n_iter / converged / count equal."""
    f = mix.fit
    got = np.concatenate([f.weights, f.means, f.stddevs ** 2, [f.lower_bound]])
    np.testing.assert_allclose(got, row[:3 * K + 1], rtol=rel, atol=0)
    assert (f.n_iter, float(f.converged), f.count) == (int(row[3 * K + 1]), row[3 * K + 2], int(row[3 * K + 4]))
    assert f.metadata['op'] == 'density_estimate' and len(mix.distributions) == K
    np.testing.assert_allclose(mix.probs.numpy(), f.weights, rtol=1e-6)


def test_entry_points_are_declared_prototyped_and_exported():
    """FAILS WITHOUT THE FEATURE: the parent has neither symbol."""
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
    block = hdr[hdr.index('Weighted Gaussian-mixture EM over one latent'):hdr.index('#define PP_IS_GMM_MAX_K')]
    for needle in ('empirical.py:795-807', '10 DBL_EPSILON', 'lb_0 = -inf', 'reg_covar'):
        assert needle in block, needle
    import pyprob_amd
    from pyprob_amd import build, ops as P
    assert 'is_gmm.hip' in build.SOURCES
    assert hasattr(P.ops, 'is_gmm_groups') and '    is_gmm_groups ' in P.__doc__
    assert callable(pyprob_amd.density_estimate_batch)


def test_width_macro_agrees_between_header_and_binding():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    assert int(re.search(r'#define PP_IS_GMM_MAX_K (\d+)', hdr).group(1)) == L.PP_IS_GMM_MAX_K == 16
    body = re.search(r'#define PP_IS_GMM_WIDTH\(K\) (.*)', hdr).group(1)
    for K in range(1, 17):
        assert eval(body, {'K': K}) == L.PP_IS_GMM_WIDTH(K) == G.width(K) == 3 * K + 6
    assert L.PP_IS_GMM_WIDTH(16) == 54


def test_workspace_bytes_are_monotone():
    lib = L.load()
    fn = lib.pp_is_gmm_workspace_bytes
    per = (1, 63, 2047, 2048, 2049, 4097, 70001, 10 ** 6)
    for K in (1, 3, 5, 16):
        for M in (0, 1, 3, 257, 70000):
            sizes = [fn(M, n, K) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (K, M, sizes)
        for n in per:
            sizes = [fn(M, n, K) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (K, n, sizes)
    for M, n in ((1, 1), (3, 2049), (256, 10000), (1, 10 ** 6)):
        sizes = [fn(M, n, K) for K in range(1, 17)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (M, n, sizes)
    assert fn(4, 10 ** 6, 3) > fn(1, 10 ** 6, 3) > fn(1, 2048, 3)
    for bad in ((-1, 5, 2), (1, 0, 2), (1, 5, 0), (1, 5, 17), (2 ** 20, 2 ** 11, 2)):
        assert fn(*bad) == 0, bad
    assert fn(1, 2 ** 31 - 1, 16) > 0


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    M, N, K = 3, 5000, 5
    lw, x = torch.zeros(M * N), torch.zeros(M * N)
    stats = torch.zeros(M, 6, dtype=torch.float64)
    init = torch.zeros(M, 3 * K, dtype=torch.float64)
    out = torch.zeros(M, L.PP_IS_GMM_WIDTH(K), dtype=torch.float64)
    wb = lib.pp_is_gmm_workspace_bytes(M, N, K)
    ws = torch.zeros(wb, dtype=torch.uint8)

    def call(lp=lw.data_ptr(), xp=x.data_ptr(), k=K, m=M, n=N, sp=stats.data_ptr(), ip=init.data_ptr(), it=10, tol=1e-3, reg=1e-6,
             every=8, o=out.data_ptr(), w=ws.data_ptr(), b=wb):
        return lib.pp_is_gmm_groups(lp, xp, k, m, n, sp, ip, it, tol, reg, every, o, w, b, None)
    for kw in (dict(lp=None), dict(xp=None), dict(ip=None), dict(o=None), dict(w=None), dict(k=0), dict(k=-1), dict(k=17, b=2 ** 40),
               dict(n=0), dict(n=-2), dict(m=-1), dict(m=2 ** 20, n=2 ** 11, b=2 ** 40), dict(it=0), dict(it=-5), dict(tol=-1e-9),
               dict(reg=-1e-9), dict(tol=float('nan')), dict(reg=float('nan'))):
        assert call(**kw) == EINVAL, kw
        assert b'pp_is_gmm_groups' in lib.pp_last_error()
    assert call(b=wb - 1) == ENOSPACE and call(b=0) == ENOSPACE and b'workspace too small' in lib.pp_last_error()
    assert call(m=0) == 0 and call(m=0, sp=None) == 0                            # no group: nothing to launch
    for t in (lw, x, stats, init, out, ws):
        assert float(t.double().abs().sum()) == 0.0


def test_gmm_ref_reproduces_scikit_learn_on_the_golden():
    """The reference's own density_estimate (scikit-learn's EM) on values repeated by integer weights, against gmm_ref on the
    distinct values under log(weight): equal n_iter, parameters and lower bound within 100 times the measured deviation."""
    z = np.load(os.path.join(REPO, 'tests', 'golden', 'gmm_sklearn.npz'))
    assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', 'gmm_sklearn.npz')) < 200 * 1024
    assert GOLDEN_BOUND <= 1e-9
    seen = []
    for c in ('k1', 'k2', 'k3', 'k5'):
        values, mult, init, fit = z[c + '_values'], z[c + '_mult'], z[c + '_init'], z[c + '_fit']
        K = len(init) // 3
        assert len(values) <= 4000 and mult.min() == 1 and mult.max() == 5 and values.dtype == np.float32
        row, _ = G.em_ref(np.log(mult.astype(np.float64)), values, init)
        dev = max(np.abs(row[:3 * K] - fit).max(), abs(row[3 * K] - float(z[c + '_lower_bound'])))
        print(c, 'K', K, 'n_iter', int(row[3 * K + 1]), 'deviation', dev)
        assert int(row[3 * K + 1]) == int(z[c + '_n_iter']) and row[3 * K + 2] == 1.0
        assert dev <= GOLDEN_BOUND, (c, dev)
        seen.append(K)
    assert seen == [1, 2, 3, 5]


def _bimodal(rng, n):
    x = np.where(rng.random(n) < 0.35, rng.normal(-2.0, 0.4, n), rng.normal(1.5, 0.7, n)).astype(np.float32)
    lw = rng.normal(0.0, 1.0, n).astype(np.float32)
    return x, lw


def test_host_route_on_hand_made_cases(monkeypatch):
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import Empirical, Mixture, MixtureFit

    def boom(*a, **k):
        raise AssertionError('a host-backed Empirical reached a device operator')
    for op in ('is_gmm_groups', 'is_sort_groups', 'is_quantile_groups', 'is_cdf_groups'):
        monkeypatch.setattr(P.ops, op, boom, raising=False)
    rng = np.random.default_rng(21)
    n = 1500
    x, lw = _bimodal(rng, n)
    lw[5], x[5] = -np.inf, np.nan                                               # a skipped particle: its value enters nothing
    emp = Empirical(values=[float(v) for v in x], log_weights=lw.astype(np.float64))
    for K in (1, 2, 3):
        mix = emp.density_estimate(K)
        assert isinstance(mix, Mixture) and isinstance(mix.fit, MixtureFit) and mix.fit.converged and mix.fit.count == n - 1
        row, _ = G.em_ref(lw, x, G.init_ref(lw, x, K))
        _close(mix, row, K, 1e-9)
    two = emp.density_estimate(2).fit
    assert abs(two.means[0] + 2.0) < 0.1 and abs(two.means[1] - 1.5) < 0.1 and abs(two.weights[0] - 0.35) < 0.05
    assert abs(two.stddevs[0] - 0.4) < 0.08 and abs(two.stddevs[1] - 0.7) < 0.08
    # K = 1 is the weighted mean and variance (+ reg_covar)
    one = emp.density_estimate(1).fit
    w = G.weights_ref(lw)[0]
    mean = (w[w > 0] * x[w > 0].astype(np.float64)).sum() / w.sum()
    var = (w[w > 0] * (x[w > 0] - mean) ** 2).sum() / w.sum()
    assert one.means[0] == pytest.approx(mean, rel=1e-9) and one.stddevs[0] ** 2 == pytest.approx(var + 1e-6, rel=1e-9)
    # the overrides are honoured: a start of their own, against gmm_ref from exactly that start
    init = np.array([0.2, 0.8, -1.0, 1.0, 0.3 ** 2, 0.9 ** 2])
    mix = emp.density_estimate(2, tol=0.0, max_iter=3, weights_init=[0.2, 0.8], means_init=[-1.0, 1.0], stddevs_init=[0.3, 0.9])
    row, _ = G.em_ref(lw, x, init, max_iter=3, tol=0.0)
    _close(mix, row, 2, 1e-12)
    assert mix.fit.n_iter == 3 and not mix.fit.converged
    only_sd = emp.density_estimate(2, tol=0.0, max_iter=1, stddevs_init=[2.0, 2.0])
    start = G.init_ref(lw, x, 2)
    start[4:] = 4.0
    _close(only_sd, G.em_ref(lw, x, start, max_iter=1, tol=0.0)[0], 2, 1e-9)
    # a fit that does not converge warns
    with pytest.warns(RuntimeWarning, match='did not converge'):
        emp.density_estimate(2, max_iter=1)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        emp.density_estimate(2)
    # num_samples: the reference's route - resample, then fit the draws
    torch.manual_seed(3)
    drawn = emp.density_estimate(2, num_samples=1000)
    assert drawn.fit.count == 1000 and drawn.fit.metadata['length'] == 1000
    assert abs(drawn.fit.means[0] + 2.0) < 0.3 and abs(drawn.fit.means[1] - 1.5) < 0.3
    # arguments
    for bad in (dict(num_mixture_components=0), dict(num_mixture_components=17), dict(num_mixture_components=2.0), dict(max_iter=0),
                dict(tol=-1.0), dict(reg_covar=-1e-6), dict(num_mixture_components=2, means_init=[0.0]),
                dict(num_mixture_components=2, weights_init=[0.0, 1.0]), dict(num_mixture_components=2, stddevs_init=[0.0, 1.0])):
        with pytest.raises(ValueError):
            emp.density_estimate(**bad)
    with pytest.raises(ValueError, match='scalar values'):
        Empirical(values=[torch.zeros(2), torch.ones(2)], log_weights=np.zeros(2)).density_estimate(1, means_init=[0.0],
                                                                                                    stddevs_init=[1.0])
    with pytest.raises(ValueError, match='no particle with a finite log-weight'):
        Empirical(values=[1.0, 2.0], log_weights=[-np.inf, -np.inf]).density_estimate(1, means_init=[0.0], stddevs_init=[1.0])
    # tensors that are not on a device, and every object under PP_EMPIRICAL_DEVICE=0, take the numpy route
    dev = Empirical.from_device(torch.from_numpy(x), torch.from_numpy(lw), None)
    want = _fit_row(emp.density_estimate(2))
    np.testing.assert_allclose(_fit_row(dev.density_estimate(2)), want, rtol=1e-9)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    np.testing.assert_allclose(_fit_row(dev.density_estimate(2)), want, rtol=1e-9)


def test_device_style_empirical_through_the_cpu_double(device_style):
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(22)
    n = 2500
    x, lw = _bimodal(rng, n)
    lw[::97], x[::97] = -np.inf, np.nan
    emp = Empirical.from_device(torch.from_numpy(x), torch.from_numpy(lw), None)
    G.calls['is_gmm_groups'] = 0
    mix = emp.density_estimate(2)
    assert G.calls['is_gmm_groups'] == 1
    _close(mix, G.em_ref(lw, x, G.init_ref(lw, x, 2))[0], 2, 1e-9)
    # what the device route returns for its other device-backed objects: a resample and a combine_duplicates result
    re = emp.resample(800, seed=4)
    assert re._device_backed() and re.density_estimate(2).fit.count == 800
    x_int = rng.integers(-3, 4, n).astype(np.float32)
    dup = Empirical.from_device(torch.from_numpy(x_int), torch.from_numpy(lw), None).combine_duplicates()
    assert dup._device_backed() and dup.length == 7
    fit = dup.density_estimate(1).fit
    assert fit.count == 7 and fit.means[0] == pytest.approx(dup.mean, rel=1e-6)
    assert G.calls['is_gmm_groups'] == 3
    torch.manual_seed(0)
    assert emp.density_estimate(2, num_samples=500).fit.count == 500 and G.calls['is_gmm_groups'] == 4


def test_density_estimate_batch_equals_the_loop(device_style):
    import order_stats_ref as R
    import pyprob_amd
    rng = np.random.default_rng(23)
    M, N, K = 5, 400, 2
    x = np.concatenate([_bimodal(rng, N)[0] + g for g in range(M)])
    values = torch.from_numpy(x)
    lw = torch.from_numpy(rng.normal(0, 1, M * N).astype(np.float32))
    posts = _batch_of(values, lw, M, N)
    loop = [p.density_estimate(K) for p in posts]
    G.calls['is_gmm_groups'] = 0
    for k in R.calls:
        R.calls[k] = 0
    fast = pyprob_amd.density_estimate_batch(posts, K)
    assert G.calls['is_gmm_groups'] == 1 and R.calls['is_sort_groups'] == 1 and R.calls['is_quantile_groups'] == 1
    assert len(fast) == M and all(np.array_equal(_fit_row(a), _fit_row(b)) for a, b in zip(fast, loop))
    assert len({f.fit.n_iter for f in fast}) >= 1 and all(f.fit.converged and f.fit.count == N for f in fast)
    assert all(abs(f.fit.means[1] - f.fit.means[0] - 3.5) < 0.4 for f in fast)
    # overrides reach every group; anything that is not the M groups in order takes the loop
    kw = dict(tol=0.0, max_iter=2, means_init=[0.0, 3.0], stddevs_init=[1.0, 1.0])
    a, b = pyprob_amd.density_estimate_batch(posts, K, **kw), [p.density_estimate(K, **kw) for p in posts]
    assert all(np.array_equal(_fit_row(u), _fit_row(v)) for u, v in zip(a, b)) and all(u.fit.n_iter == 2 for u in a)
    before = G.calls['is_gmm_groups']
    rev = pyprob_amd.density_estimate_batch(posts[::-1], K)
    assert G.calls['is_gmm_groups'] - before == M and all(np.array_equal(_fit_row(u), _fit_row(v)) for u, v in zip(rev, loop[::-1]))
    assert pyprob_amd.density_estimate_batch([], K) == []
    with pytest.raises(ValueError):
        pyprob_amd.density_estimate_batch(posts, 0)


@pytest.mark.parametrize('style', ['host', 'device'])
def test_two_statement_program_and_its_marginal(style, request):
    """The posterior and a marginal of the two-statement program on the CPU device: the numpy route (tensors that are not on a
    device) and the device route through the CPU double give gmm_ref's fit."""
    import pyprob_amd
    from test_joint_moments_host import _register_cpu_double, _two_statement_model
    if style == 'device':
        request.getfixturevalue('device_style')
    _register_cpu_double()
    model = _two_statement_model()
    n = 300
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
    A, B = 'a__Normal__1', 'b__Normal__1'
    lw = post._all_log_weights.numpy()
    a, b = post.statement_log[0][A][0].numpy(), post.statement_log[1][B][0].numpy()
    kw = dict(tol=0.0, max_iter=4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        own, lat = post.density_estimate(2, **kw), post.marginal('mu').density_estimate(2, **kw)
        both = pyprob_amd.density_estimate_batch([post, post], 2, address='mu', **kw)      # not one batched execution: the loop
    # (the default start takes the variance from the call's statistics - an fp32 exponent of the weights: ~1e-7 on the start)
    _close(own, G.em_ref(lw, b, G.init_ref(lw, b, 2), **kw)[0], 2, 1e-5)
    _close(lat, G.em_ref(lw, a, G.init_ref(lw, a, 2), **kw)[0], 2, 1e-5)
    assert len(both) == 2 and all(np.array_equal(_fit_row(m), _fit_row(lat)) for m in both)
    assert own.fit.count == n and own.fit.metadata['length'] == n and lat.fit.metadata['address'] == A


def test_marsaglia_branch_address(device_style):
    """Rows some particles executed only: marginal(address).density_estimate fits THOSE particles."""
    from is_helpers import lockstep_network
    from test_joint_moments_host import _register_cpu_double
    _register_cpu_double()
    model, net, meta, params = lockstep_network()
    n = 400
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=3, offset=0)
    log, addrs = post.statement_log, post.addresses
    lw = post._all_log_weights.numpy()
    x0, y0 = (log[k][addrs[k]][0].numpy() for k in (0, 1))
    rejected = np.nonzero(x0 * x0 + y0 * y0 >= 1)[0]
    assert 0 < len(rejected) < n
    x1 = log[2][addrs[2]][0].numpy()[rejected]
    init = dict(means_init=[-0.5, 0.5], stddevs_init=[0.4, 0.4])
    start = np.array([0.5, 0.5, -0.5, 0.5, 0.16, 0.16])
    m = post.marginal(addrs[2]).density_estimate(2, tol=0.0, max_iter=3, **init)
    _close(m, G.em_ref(lw[rejected], x1, start, max_iter=3, tol=0.0)[0], 2, 1e-12)
    assert m.fit.count == len(rejected)
    whole = post.density_estimate(2, tol=0.0, max_iter=3, **init)
    _close(whole, G.em_ref(post._log_weights.numpy(), post._values.numpy(), start, max_iter=3, tol=0.0)[0], 2, 1e-12)


def test_the_fitted_mixture_is_the_prior_of_a_second_lock_step_call():
    """Posterior in, prior out: the Mixture density_estimate returns feeds a second prior-IS call in lock step and scores finite."""
    import pyprob_amd
    from pyprob_amd import Model
    from pyprob_amd import distributions as D
    from test_dist_families import _register_dist_cpu_doubles
    import mixture_cases as MC
    oracle_ops.register()
    _register_dist_cpu_doubles()
    MC.register_mix_cpu_doubles()

    class First(Model):
        def forward(self):
            mu = pyprob_amd.sample(D.Normal(0.0, 2.0))
            pyprob_amd.observe(D.Mixture([D.Normal(mu, 0.5), D.Normal(-mu, 0.5)], probs=[0.3, 0.7]), name='y')
            return mu

    n = 2000
    post = First()._traces_prior_lockstep(n, {'y': 1.5}, seed=3, device='cpu')
    mix = post.density_estimate(2)
    f = mix.fit
    assert f.converged and f.count == n and f.means[0] < -1.0 < 1.0 < f.means[1] and f.weights[0] > f.weights[1]

    class Second(Model):
        def forward(self):
            mu = pyprob_amd.sample(mix)
            pyprob_amd.observe(D.Normal(mu, 0.5), name='y')
            return mu

    again = Second()._traces_prior_lockstep(n, {'y': 1.4}, seed=4, device='cpu')
    lw2 = again._all_log_weights.double().numpy()
    assert again.length == n and np.isfinite(lw2).all() and np.isfinite(again.mean)
    x2 = again._all_values.double().numpy()
    assert ((x2 < 0).mean() > 0.5) and (x2 > 0).any()                           # draws from both modes of the fitted prior
    np.testing.assert_allclose(mix.log_prob(torch.tensor([0.0, 1.5, -1.5])).double().numpy(),
                               G.mixture_logpdf([0.0, 1.5, -1.5], f.weights, f.means, f.stddevs), rtol=1e-4, atol=1e-4)
