"""CPU tests of the Mixture family (pyprob/distributions/mixture.py): the mirror class against the reference's values recorded in
tests/golden/mixture_lp.npz (tests/golden/make_mixture_golden.py), the pp_mix_* entry points' argument checks (they precede any
launch, so no device is needed), per-trace prior IS against a float64 quadrature, and the lock-step host logic on CPU test
doubles of the two operators."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import mixture_cases as MC
import pyprob_amd
from pyprob_amd import distributions as D
from pyprob_amd.model import Model
from pyprob_amd.state import InferenceEngine

IS = InferenceEngine.IMPORTANCE_SAMPLING


# ---- the mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MC.cases())
def test_mirror_against_reference(case):
    g = MC.golden()
    mix = MC.mirror(case)
    names = [str(s) for s in g[case + '_names']]
    assert mix.name == 'Mixture' and len(mix) == len(names) == len(mix.distributions)
    assert mix._address_suffix == str(g[case + '_suffix']) == 'Mixture({})'.format(', '.join(names))
    x, ref = g[case + '_x'], g[case + '_lp']
    lp = torch.stack([mix.log_prob(torch.as_tensor(v)) for v in x]).numpy()
    assert lp.shape == ref.shape                       # [V] for 1-D probs (a scalar per value), [V, B] for 2-D
    np.testing.assert_allclose(lp, ref, rtol=1e-5, atol=1e-5, err_msg=case)
    assert np.array_equal(np.isneginf(lp), np.isneginf(ref))
    assert float(mix.log_prob(torch.as_tensor(x[0]), sum=True)) == pytest.approx(float(np.sum(ref[0])), rel=1e-5, abs=1e-5) \
        or np.isneginf(ref[0]).any()
    assert mix.mean.shape == g[case + '_mean'].shape and mix.stddev.shape == g[case + '_stddev'].shape
    np.testing.assert_allclose(mix.mean.numpy(), g[case + '_mean'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(mix.stddev.numpy(), g[case + '_stddev'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(mix.variance.numpy(), g[case + '_stddev'].astype(np.float64) ** 2, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(mix.probs.sum(-1).numpy(), 1.0, rtol=1e-6)
    assert 'Mixture(distributions=[' in repr(mix)
    assert mix.to('cpu').log_prob(torch.as_tensor(x[1])).shape == ref[1].shape


def test_default_probs_are_uniform_and_bad_arguments_raise():
    mix = D.Mixture([D.Normal(0.0, 1.0), D.Normal(3.0, 1.0)])
    assert mix.probs.tolist() == [0.5, 0.5] and mix._address_suffix == 'Mixture(Normal, Normal)'
    with pytest.raises(ValueError):
        D.Mixture([D.Normal(0.0, 1.0)], probs=torch.ones(1, 1, 1))
    with pytest.raises(ValueError):
        D.Mixture([D.Normal(0.0, 1.0)], probs=[0.5, 0.5])


@pytest.mark.parametrize('case', MC.cases())
def test_sample_lies_in_the_support_of_some_component(case):
    torch.manual_seed(3)
    g = MC.golden()
    mix = MC.mirror(case)
    probs = g[case + '_probs']
    for _ in range(20):
        s = mix.sample()
        assert s.shape == (torch.Size([]) if probs.ndim == 1 else torch.Size([probs.shape[0]]))
        lps = torch.stack([d.log_prob(s).reshape(s.shape) for d in mix.distributions])
        assert bool((lps > -math.inf).any(0).all()), (case, s)
        assert bool((mix.log_prob(s) > -math.inf).all())


def test_sample_n_follows_the_weights():
    torch.manual_seed(0)
    mix = D.Mixture([D.Normal(-50.0, 0.1), D.Exponential(1.0), D.Uniform(100.0, 101.0)], probs=[1.0, 2.0, 1.0])
    v = mix.sample_n(40000).numpy()
    frac = np.array([(v < -40).mean(), ((v >= 0) & (v < 90)).mean(), (v >= 100).mean()])
    assert frac.sum() == 1.0
    np.testing.assert_allclose(frac, [0.25, 0.5, 0.25], atol=5 * math.sqrt(0.25 / 40000))


@pytest.mark.skipif(not os.path.isdir('/root/reference/pyprob'), reason='needs the live reference')
def test_convert_maps_pyprob_mixture():
    import sys
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, '/root/reference')
    import pyprob.distributions as R
    from pyprob_amd.pyprob_host import convert
    ref = R.Mixture([R.Normal(0.0, 1.0), R.Gamma(2.0, 3.0), R.Uniform(1.0, 4.0)], probs=[2.0, 1.0, 1.0])
    m = convert(ref)
    assert isinstance(m, D.Mixture) and m._address_suffix == ref._address_suffix == 'Mixture(Normal, Gamma, Uniform)'
    assert [d.name for d in m.distributions] == ['Normal', 'Gamma', 'Uniform']
    for x in (1.2, 2.5, 3.9):       # (inside every support: the reference's torch validates its arguments)
        assert float(m.log_prob(x)) == pytest.approx(float(ref.log_prob(x)), rel=1e-5, abs=1e-5)
    ref2 = R.Mixture([R.Normal([0.0, 1.0], [0.1, 1.0]), R.Normal([2.0, 5.0], [0.1, 1.0])], probs=[[0.7, 0.3], [0.1, 0.9]])
    x = torch.tensor([0.1, 4.0])
    np.testing.assert_allclose(convert(ref2).log_prob(x).numpy(), ref2.log_prob(x).numpy(), rtol=1e-5, atol=1e-5)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from pyprob_amd import build as B
    B.build()
    from pyprob_amd import lib as L
    return L.load()


def test_abi_exports_the_mixture_entry_points(lib):
    from pyprob_amd import lib as L
    assert lib.pp_abi_version() == 15 == L.PP_ABI_VERSION
    assert hasattr(lib, 'pp_mix_logweight') and hasattr(lib, 'pp_mix_draw')
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    assert int(re.search(r'#define PP_MIX_MAX_COMPONENTS (\d+)', hdr).group(1)) == L.PP_MIX_MAX_COMPONENTS == 16
    assert C.sizeof(L.pp_mixture) == 16 + 16 * C.sizeof(L.pp_dist)
    assert C.sizeof(L.pp_dist) == 24 + 4 * 8 and C.sizeof(L.pp_dist_term) == C.sizeof(L.pp_dist) + 16       # unchanged
    import pyprob_amd.ops  # noqa: F401
    assert hasattr(torch.ops.pyprob_hip, 'mix_logweight') and hasattr(torch.ops.pyprob_hip, 'mix_draw')


EINVAL = -1      # PP_EINVAL


def _mixture(L, buf, kinds=(0, 0), stride=0, count=None, probs=True, drop=None):
    """A pp_mixture over a host buffer. Every call below has m = n = 0: a call that passes the checks returns before any launch,
    so the pointers are never read."""
    mx = L.pp_mixture()
    mx.count = len(kinds) if count is None else count
    mx.probs_stride = stride
    mx.probs = buf.ctypes.data if probs else None
    npar = {0: 2, 1: 2, 3: 1, 4: 1, 6: 1, 7: 2, 8: 4, 9: 2, 10: 2, 11: 2, 12: 2, 13: 4}
    for k, kind in enumerate(kinds):
        mx.comp[k].kind = kind
        for q in range(npar.get(kind, 2)):
            if drop != (k, q):
                mx.comp[k].p[q] = buf.ctypes.data
    return mx


def test_argument_checks_come_before_any_launch(lib):
    from pyprob_amd import lib as L
    buf = np.ones(64, np.float32)
    rows = np.zeros(4, np.int64)
    ptr, rp = buf.ctypes.data, rows.ctypes.data

    def lw(mx, x=ptr, sx=1, lwp=ptr, lp=None, rows_=None, m=0, n=0):
        return lib.pp_mix_logweight(C.byref(mx), x, sx, 1.0, lwp, lp, rows_, m, n, None)

    def dr(mx, rows_=None, m=0, n=0, stream=7, out=ptr):
        return lib.pp_mix_draw(C.byref(mx), rows_, m, n, 1, 0, stream, out, None)
    good = _mixture(L, buf)
    assert lw(good) == 0 and dr(good) == 0
    assert lw(_mixture(L, buf, kinds=(0, 7, 13), stride=3)) == 0 and dr(_mixture(L, buf, kinds=(6,) * 16)) == 0
    bad = [('K = 0', _mixture(L, buf, count=0)), ('K = 17', _mixture(L, buf, count=17)),
           ('Factor', _mixture(L, buf, kinds=(0, 2))), ('Categorical', _mixture(L, buf, kinds=(5, 0))),
           ('unknown kind', _mixture(L, buf, kinds=(0, 14))), ('negative kind', _mixture(L, buf, kinds=(-1,))),
           ('missing second parameter', _mixture(L, buf, kinds=(0, 7), drop=(1, 1))),
           ('missing fourth parameter', _mixture(L, buf, kinds=(13,), drop=(0, 3))),
           ('no probs', _mixture(L, buf, probs=False)), ('stride 1', _mixture(L, buf, stride=1)),
           ('stride 3 of K = 2', _mixture(L, buf, stride=3))]
    for what, mx in bad:
        for call in (lw, dr):
            assert call(mx) == EINVAL, what
            assert lib.pp_last_error(), what
    # the m / n / rows rules of pp_dist_*
    for kw in (dict(m=1, n=0), dict(m=-1, n=0), dict(m=0, n=-1), dict(m=0, n=4), dict(rows_=rp, m=5, n=4)):
        assert lw(good, **kw) == EINVAL and dr(good, **kw) == EINVAL, kw
    assert lw(good, rows_=rp, m=0, n=4) == 0 and dr(good, rows_=rp, m=0, n=4) == 0
    assert lw(good, x=None) == EINVAL and lw(good, sx=-1) == EINVAL and lw(good, lwp=None, lp=None) == EINVAL and dr(good, out=None) == EINVAL
    assert lw(good, lwp=None, lp=ptr) == 0
    assert dr(good, stream=0x80000000) == EINVAL and b'stream_id' in lib.pp_last_error()
    assert dr(good, stream=0x80000007) == EINVAL and dr(good, stream=0x7FFFFFFF) == 0
    assert lib.pp_mix_logweight(None, ptr, 1, 1.0, ptr, None, None, 0, 0, None) == EINVAL


# ---- per-trace prior IS ----------------------------------------------------------------------------------------------------
S_OBS = 0.5
PROBS = [0.3, 0.7]


class MirroredGMM(Model):
    """mu ~ Normal(0, 2); y ~ 0.3 Normal(mu, s) + 0.7 Normal(-mu, s): the posterior of mu is bimodal, that of |mu| is not."""
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(0.0, 2.0))
        pyprob_amd.observe(D.Mixture([D.Normal(mu, S_OBS), D.Normal(-mu, S_OBS)], probs=PROBS), name='y')
        return abs(mu)


def gmm_abs_mean_quadrature(y):
    """E[|mu| | y] by float64 quadrature on a grid of 400 001 points over [-20, 20] (10 prior standard deviations)."""
    mu = np.linspace(-20.0, 20.0, 400001)
    lp = MC.comp_lp64('Normal', [0.0, 2.0], mu) + MC.mix_lp64(['Normal', 'Normal'], [[mu, S_OBS], [-mu, S_OBS]], PROBS, np.full_like(mu, y))
    w = np.exp(lp - lp.max())
    return float((w * np.abs(mu)).sum() / w.sum())


def test_per_trace_prior_is_with_a_mixture_likelihood():
    torch.manual_seed(0)
    n = 3000
    post = MirroredGMM().posterior_results(n, IS, observe={'y': 1.5})
    # |mu| | y is close to Normal(1.41, 0.49); prior draws from Normal(0, 2) leave an effective sample size of ~ n / 4, so the
    # standard error of the estimate is ~ 0.49 / sqrt(750) = 0.018: the bound is 5 of them
    assert float(post.mean) == pytest.approx(gmm_abs_mean_quadrature(1.5), abs=0.09)
    assert post.effective_sample_size > n / 10


# ---- the lock-step host logic on CPU test doubles ----------------------------------------------------------------------------
class MixturePriorAndLikelihood(Model):
    def forward(self):
        z = pyprob_amd.sample(D.Mixture([D.Normal(-3.0, 0.5), D.Gamma(4.0, 2.0)], probs=[1.0, 3.0]))
        mu = pyprob_amd.sample(D.Normal(0.0, 2.0))
        pyprob_amd.observe(D.Mixture([D.Normal(mu, S_OBS), D.Exponential(torch.exp(0.3 * z))], probs=torch.stack([z * 0 + 1.0, torch.exp(0.1 * mu)], 1)),
                           name='y')
        return mu


@pytest.fixture()
def cpu_doubles():
    import oracle_ops
    from test_dist_families import _register_dist_cpu_doubles
    oracle_ops.register()
    _register_dist_cpu_doubles()
    MC.register_mix_cpu_doubles()


def test_runner_builds_the_mixture_term(cpu_doubles):
    from pyprob_amd.is_engine import DistRunner, MixTerm
    r = DistRunner.__new__(DistRunner)
    r.dev = torch.device('cpu')
    r._consts = {}
    r._const = lambda v: torch.tensor([v], dtype=torch.float32)
    n = 5
    mix = D.Mixture([D.Normal(torch.arange(n).float(), 1.0), D.TruncatedNormal(0.0, 1.0, -1.0, 2.0), D.Exponential(2.0)], probs=torch.rand(n, 3))
    term = r.dist_term(mix)
    assert len(term) == 6 and term[0] == 'Mixture' and term[1] == [0, 13, 6] and term[5] == 3
    assert len(term[2]) == 12 and term[3] == [1, 1, 0, 0] + [0] * 4 + [0] * 4      # (the shared stddev comes broadcast)
    assert term[2][0].numel() == n and term[2][9] is None and term[4].numel() == 3 * n
    assert type(term) is MixTerm and not term.fused
    assert (term.tag, term.kinds, term.K) == ('Mixture', [0, 13, 6], 3) and term.params is term[2] and term.probs is term[4]
    r.accumulate(torch.zeros(n), term, torch.zeros(n))
    with pytest.raises(RuntimeError, match='lock-step Mixture'):        # the size check of every route: the weights hold n rows
        r.accumulate(torch.zeros(n + 1), term, torch.zeros(n + 1))
    with pytest.raises(RuntimeError, match='lock-step Mixture'):
        r.draw(mix, torch.zeros(n + 1), None, 1, 7)
    # Categorical, Factor and nested mixtures are no components
    assert r.dist_term(D.Mixture([D.Categorical([0.5, 0.5])])) is None
    assert r.dist_term(D.Mixture([D.Mixture([D.Normal(0.0, 1.0)])])) is None


def test_lock_step_prior_is_on_cpu_doubles(cpu_doubles):
    torch.manual_seed(1)
    n = 2000
    model = MixturePriorAndLikelihood()
    post = model._traces_prior_lockstep(n, {'y': 1.2}, seed=3, device='cpu')
    assert post.num_paths == 1 and post.length == n
    log = post.statement_log
    z, mu = (next(iter(log[j].values()))[0].double().numpy() for j in range(2))
    assert np.array_equal(mu, post._all_values.double().numpy())
    assert ((z < -1) | (z > 0)).all() and 0.2 < (z < -1).mean() < 0.3          # the Mixture prior: weights 1 : 3, no weight term
    ref = MC.mix_lp64(['Normal', 'Exponential'], [[mu.astype(np.float32), S_OBS], [np.exp(np.float32(0.3) * z.astype(np.float32))]],
                      np.stack([np.ones(n), np.exp(np.float32(0.1) * mu.astype(np.float32))], 1), np.full(n, 1.2))
    np.testing.assert_allclose(post._all_log_weights.double().numpy(), ref, rtol=1e-4, atol=1e-4)


def test_prior_traces_packed_with_a_mixture_likelihood_on_cpu():
    torch.manual_seed(2)
    n = 20000
    lens, table, ids, vals, prior, obs = MirroredGMM().prior_traces_packed(n, ['y'])
    assert lens.tolist() == [1] * n and table[0][1] == 'Normal' and obs.shape == (n, 1)
    # y - mu is Normal(0, s) with weight 0.3; y + mu with weight 0.7: the residual to the nearer of +-mu is within 5 s for all
    r = np.minimum(np.abs(obs[:, 0] - vals), np.abs(obs[:, 0] + vals))
    assert (r < 5 * S_OBS).all()
    far = np.abs(vals) > 3 * S_OBS          # where the two components are told apart
    took_first = np.abs(obs[far, 0] - vals[far]) < np.abs(obs[far, 0] + vals[far])
    assert abs(took_first.mean() - 0.3) < 5 * math.sqrt(0.21 / far.sum())


def test_controlled_mixture_sample_is_refused_with_the_reference_wording():
    class Controlled(Model):
        def forward(self):
            z = pyprob_amd.sample(D.Mixture([D.Normal(0.0, 1.0), D.Normal(3.0, 1.0)]))
            pyprob_amd.observe(D.Normal(z, 1.0), name='y')
            return z
    with pytest.raises(RuntimeError, match='Distribution currently unsupported: Mixture'):
        Controlled().prior_traces_packed(8, ['y'])


# ---- the one host route of a log-weight term (DistRunner.accumulate) on the CPU doubles -------------------------------------------
ROUTE_N = 37
ROUTE_ROWS = [0, 3, 4, 9, 15, 16, 22, 28, 31, 35, 36]       # 11 ascending particles, the first and the last among them


def _route_case(name):
    """(mirror distribution with at least one per-particle parameter, values [n]) of one term shape; deterministic per name."""
    n = ROUTE_N
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    u, z = (lambda: torch.rand(n, generator=g)), (lambda: torch.randn(n, generator=g))
    if name == 'Normal':
        return D.Normal(z(), 1.7), z()
    if name == 'Uniform':
        return D.Uniform(-1.0 - u(), 2.0), 6.0 * u() - 3.0                    # (values on both sides of the support)
    if name == 'Poisson':
        return D.Poisson(0.5 + 3.0 * u()), torch.floor(8.0 * u())
    if name == 'Bernoulli':
        return D.Bernoulli(0.1 + 0.8 * u()), (u() < 0.5).float()
    if name == 'Categorical':
        return D.Categorical(0.1 + torch.rand(n, 3, generator=g)), torch.floor(3.0 * u())
    if name == 'Exponential':
        return D.Exponential(0.5 + u()), 3.0 * u()
    if name == 'Gamma':
        return D.Gamma(1.0 + 2.0 * u(), 1.5), 0.1 + 3.0 * u()
    if name == 'Beta':
        return D.Beta(1.0 + 2.0 * u(), 2.0, low=-1.0, high=3.0), -1.0 + 4.0 * (0.05 + 0.9 * u())
    if name == 'LogNormal':
        return D.LogNormal(0.3 * z(), 0.8), 0.1 + 3.0 * u()
    if name == 'Weibull':
        return D.Weibull(1.0 + u(), 1.5), 0.1 + 3.0 * u()
    if name == 'Binomial':
        return D.Binomial(total_count=12, logits=z()), torch.floor(13.0 * u())
    if name == 'VonMises':
        return D.VonMises(z(), 2.0), z()
    if name == 'TruncatedNormal':
        return D.TruncatedNormal(z(), 1.0, -2.0, 3.0), -2.0 + 5.0 * u()
    if name == 'Factor':
        x = z()
        return D.Factor(log_prob=x), x                                        # (the term is the value itself)
    assert name == 'Mixture'
    return D.Mixture([D.Normal(z(), 1.0), D.TruncatedNormal(0.0, 1.0, -1.0, 2.0), D.Exponential(2.0)], probs=0.1 + torch.rand(n, 3, generator=g)), 1.5 * u()


ROUTE_CASES = ['Normal', 'Uniform', 'Poisson', 'Bernoulli', 'Categorical'] + sorted(D.DIST_KINDS) + ['Mixture']


@pytest.mark.parametrize('route', ['full', 'path'])
@pytest.mark.parametrize('name', ROUTE_CASES)
def test_accumulate_adds_the_mirror_log_prob_on_every_route(cpu_doubles, name, route):
    """DistRunner.accumulate for every term shape - the five ScalarTerm kinds, every DistTerm family and Factor, a 3-component
    MixTerm - at full width and on a path of 11 of 37 particles: exactly the path's particles gain scale * log_prob of the
    mirror class, the others keep their bits. A path reaches the DistTerm / MixTerm launches as its row list; the ScalarTerm
    rows kernel has no CPU double, so a ScalarTerm takes the mask route here (tests/test_gpu_rows.py compares the two).
    Tolerance: the doubles evaluate in float64 (the five) or with the mirror classes themselves and round once to fp32, the mirror
    evaluates in fp32 (a few ulp of a log-density below ~20: < 1e-5), and lw + scale * lp rounds once more at |lw| < ~10."""
    from pyprob_amd.is_engine import DistRunner, DistTerm, MixTerm, ScalarTerm
    r = DistRunner.__new__(DistRunner)
    r.dev = torch.device('cpu')
    r._consts = {}
    r._const = lambda v: torch.tensor([v], dtype=torch.float32)
    n, scale = ROUTE_N, 0.5
    dist, x = _route_case(name)
    term = r.dist_term(dist)
    assert type(term) is (MixTerm if name == 'Mixture' else DistTerm if name in D.DIST_KINDS else ScalarTerm)
    ref = (x if name == 'Factor' else dist.log_prob(x)).reshape(-1).float()
    assert ref.numel() == n and bool(torch.isfinite(ref).any())
    rows = torch.tensor(ROUTE_ROWS, dtype=torch.int64)
    touched = torch.ones(n, dtype=torch.bool) if route == 'full' else torch.zeros(n, dtype=torch.bool).index_fill_(0, rows, True)
    lw0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    lw = lw0.clone()
    if route == 'full':
        r.accumulate(lw, term, x, scale)
    else:
        r.accumulate(lw, term, x, scale, rows=rows, mask=touched if type(term) is ScalarTerm else None)
    assert torch.equal(lw[~touched], lw0[~touched])
    torch.testing.assert_close(lw[touched], (lw0 + scale * ref)[touched], rtol=1e-5, atol=1e-5)
    lp = r.log_prob(term, x, n)                       # the same dispatch without accumulation
    torch.testing.assert_close(lp, ref, rtol=1e-5, atol=1e-5)
