"""CPU tests of the distribution families beyond the inference network's five (pyprob_amd/distributions.py: Beta, Gamma,
Exponential, LogNormal, Weibull, Binomial, VonMises, TruncatedNormal, Factor) and of pyprob.factor: the mirror classes against
the reference's own values recorded in tests/golden/dist_lp.npz (tests/golden/make_dist_golden.py), per-trace prior IS on the
host, and the ABI 15 entry points of the library."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

import pyprob_amd
from pyprob_amd import distributions as D
from pyprob_amd.model import Model
from pyprob_amd.state import InferenceEngine

FAMILIES = ['Exponential', 'Gamma', 'Beta', 'LogNormal', 'Weibull', 'Binomial', 'VonMises', 'TruncatedNormal']


def _golden():
    return dict(np.load(os.path.join(GOLDEN, 'dist_lp.npz')))


def _make(name, p):
    """The mirror object of a golden parameter row (pp_dist order p0..p3)."""
    if name == 'Exponential':
        return D.Exponential(p[0])
    if name == 'Gamma':
        return D.Gamma(p[0], p[1])
    if name == 'Beta':
        return D.Beta(p[0], p[1], low=p[2], high=p[3])
    if name == 'LogNormal':
        return D.LogNormal(p[0], p[1])
    if name == 'Weibull':
        return D.Weibull(p[0], p[1])
    if name == 'Binomial':
        return D.Binomial(total_count=p[0], logits=p[1])
    if name == 'VonMises':
        return D.VonMises(p[0], p[1])
    return D.TruncatedNormal(p[0], p[1], p[2], p[3])


@pytest.mark.parametrize('name', FAMILIES)
def test_mirror_log_prob_mean_stddev_against_reference(name):
    g = _golden()
    for i, p in enumerate(g[name + '_params']):
        d = _make(name, [float(v) for v in p])
        assert d.name == name and d._address_suffix == name
        lp = d.log_prob(torch.from_numpy(g[name + '_x'][i])).numpy()
        np.testing.assert_allclose(lp, g[name + '_lp'][i], rtol=1e-5, atol=1e-5, err_msg='%s %s' % (name, p))
        assert float(d.mean) == pytest.approx(float(g[name + '_mean'][i]), rel=1e-5, abs=1e-6)
        # (TruncatedNormal's variance formula cancels in fp32: its stddev agrees to ~3e-5)
        assert float(d.stddev) == pytest.approx(float(g[name + '_stddev'][i]), rel=1e-4, abs=1e-6)
        s = d.sample()
        assert torch.is_tensor(s) and s.shape == torch.Size([]) and bool(torch.isfinite(s))
        assert float(d.log_prob(s, sum=True)) > -math.inf


def test_truncated_normal_clamps_its_mean_like_pyprob():
    d = D.TruncatedNormal(5.0, 1.0, 0.0, 2.0, clamp_mean_between_low_high=True)
    assert float(d.mean_non_truncated) == 2.0
    assert float(D.TruncatedNormal(5.0, 1.0, 0.0, 2.0).mean_non_truncated) == 5.0


def test_factor_log_prob():
    assert float(D.Factor(log_prob=-1.5).log_prob()) == -1.5
    assert float(D.Factor(log_prob_func=lambda x: -x * 2).log_prob(torch.tensor(3.0))) == -6.0
    assert D.Factor(log_prob=0.0).sample() is None
    with pytest.raises(RuntimeError):
        D.Factor()
    with pytest.raises(RuntimeError):
        D.Factor(log_prob=1.0, log_prob_func=lambda x: x)


class _GammaPoisson(Model):
    def forward(self):
        rate = pyprob_amd.sample(D.Gamma(3.0, 1.5))
        pyprob_amd.observe(D.Poisson(rate), name='k0')
        pyprob_amd.observe(D.Poisson(rate), name='k1')
        return rate


class _BetaBinomial(Model):
    def forward(self):
        p = pyprob_amd.sample(D.Beta(2.0, 2.0))
        pyprob_amd.observe(D.Binomial(total_count=20, probs=p), name='k')
        return p


class _FactorModel(Model):
    """reference tests/test_state.py:33-45"""
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(1.0, math.sqrt(5)))
        likelihood = D.Normal(mu, math.sqrt(2))
        pyprob_amd.factor(log_prob_func=lambda x: likelihood.log_prob(x), name='obs0')
        pyprob_amd.factor(log_prob_func=lambda x: likelihood.log_prob(x), name='obs1')
        return mu


def test_per_trace_prior_is_with_new_families():
    torch.manual_seed(0)
    post = _GammaPoisson().posterior_results(3000, InferenceEngine.IMPORTANCE_SAMPLING, observe={'k0': 4, 'k1': 6})
    # Gamma(3, 1.5) prior, two Poisson counts: Gamma(3 + 10, 1.5 + 2) posterior, mean 13 / 3.5
    assert float(post.mean) == pytest.approx(13 / 3.5, abs=0.15)
    post = _BetaBinomial().posterior_results(3000, InferenceEngine.IMPORTANCE_SAMPLING, observe={'k': 15})
    assert float(post.mean) == pytest.approx(17 / 24, abs=0.03)        # Beta(2 + 15, 2 + 5)


def test_per_trace_prior_is_with_factor():
    torch.manual_seed(0)
    post = _FactorModel().posterior_results(4000, InferenceEngine.IMPORTANCE_SAMPLING, observe={'obs0': 8, 'obs1': 9})
    assert float(post.mean) == pytest.approx(7.25, abs=0.25)
    assert float(post.stddev) == pytest.approx(math.sqrt(1 / 1.2), abs=0.25)


def test_abi_15_exports_the_distribution_entry_points():
    from pyprob_amd import build as B
    B.build()
    from pyprob_amd import lib as L
    lib = L.load()
    assert lib.pp_abi_version() == 15 == L.PP_ABI_VERSION
    assert hasattr(lib, 'pp_dist_logweight') and hasattr(lib, 'pp_dist_draw')
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    assert int(re.search(r'#define PP_DIST_MAX_TERMS (\d+)', hdr).group(1)) == L.PP_DIST_MAX_TERMS
    import ctypes as C
    assert C.sizeof(L.pp_dist) == 24 + 4 * 8          # kind + 4 strides, padded to the pointers
    assert C.sizeof(L.pp_dist_term) == C.sizeof(L.pp_dist) + 8 + 4 + 4


def test_runner_maps_every_family_to_its_kind():
    from pyprob_amd.is_engine import DistRunner, DistTerm, ScalarTerm
    r = DistRunner.__new__(DistRunner)
    r.dev = torch.device('cpu')
    r._consts = {}
    r._const = lambda v: torch.tensor([v], dtype=torch.float32)
    kinds = {'Exponential': 6, 'Gamma': 7, 'Beta': 8, 'LogNormal': 9, 'Weibull': 10, 'Binomial': 11, 'VonMises': 12,
             'TruncatedNormal': 13}
    g = _golden()
    for name, k in kinds.items():
        term = r.dist_term(_make(name, [float(v) for v in g[name + '_params'][0]]))
        assert len(term) == 9 and term[0] == k
        assert type(term) is DistTerm and not term.fused and term.kind == k and len(term.params) == 4 and term.wide() is term
    assert r.dist_term(D.Factor(log_prob=0.0))[0] == 2
    normal = r.dist_term(D.Normal(0.0, 1.0))
    assert len(normal) == 5 and type(normal) is ScalarTerm and normal.fused      # the five keep their pp_logweight_* route
    wide = normal.wide()       # ... and draw through pp_dist_draw with four parameter slots
    assert type(wide) is DistTerm and wide.kind == 0 and len(wide.params) == 4 and wide.params[2:] == [None, None]


def test_coroutine_params_take_the_new_families():
    from pyprob_amd.coroutine import _Params
    p = _Params('Gamma', [D.Gamma(2.0, 3.0), D.Gamma(1.0, 0.5)])
    np.testing.assert_array_equal(p.concentration, [2.0, 1.0])
    np.testing.assert_array_equal(p.rate, [3.0, 0.5])
    assert set(p.columns()) == {'concentration', 'rate'}


@pytest.mark.skipif(not os.path.isdir('/root/reference/pyprob'), reason='needs the live reference')
def test_convert_maps_every_new_pyprob_class_and_factor():
    import sys
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, '/root/reference')
    import pyprob.distributions as R
    from pyprob_amd.pyprob_host import convert
    cases = [(R.Exponential(2.0), 0.7), (R.Gamma(2.0, 3.0), 0.4), (R.Beta(2.0, 3.0, low=1.0, high=3.0), 2.2),
             (R.LogNormal(0.5, 0.8), 1.3), (R.Weibull(2.0, 1.5), 1.1), (R.Binomial(total_count=12, probs=torch.tensor(0.3)), 4.0),
             (R.VonMises(0.5, 2.0), 0.1), (R.TruncatedNormal(5.0, 1.0, 0.0, 2.0, clamp_mean_between_low_high=True), 1.5)]
    for d, x in cases:
        m = convert(d)
        assert m.name == d.name and m._address_suffix == d._address_suffix
        assert float(m.log_prob(x)) == pytest.approx(float(d.log_prob(x)), rel=1e-5, abs=1e-5), d.name
    f = convert(R.Factor(log_prob=torch.tensor(-2.0)))
    assert f.name == 'Factor' and float(f.log_prob()) == -2.0
    g = convert(R.Factor(log_prob_func=lambda v: v * 3))
    assert float(g.log_prob(torch.tensor(2.0))) == 6.0


_DIST_CPU_REGISTERED = []


def _register_dist_cpu_doubles():
    """TEST DOUBLES: "CPU" kernels for pyprob_hip::dist_logweight / dist_draw (the product registers the device kernels only),
    restated with the mirror classes' log_prob (torch, -inf outside the support) and torch's samplers - enough to run the host
    logic of a lock-step call without a device."""
    if _DIST_CPU_REGISTERED:
        return
    from pyprob_amd import ops as P

    def dist(kind, ps, q):
        p = [None if t is None else t.reshape(-1) for t in ps[4 * q:4 * q + 4]]
        ctor = {6: lambda: D.Exponential(p[0]), 7: lambda: D.Gamma(p[0], p[1]), 8: lambda: D.Beta(p[0], p[1], p[2], p[3]),
                9: lambda: D.LogNormal(p[0], p[1]), 10: lambda: D.Weibull(p[0], p[1]),
                11: lambda: D.Binomial(total_count=p[0], logits=p[1]), 12: lambda: D.VonMises(p[0], p[1]),
                13: lambda: D.TruncatedNormal(p[0], p[1], p[2], p[3]), 0: lambda: D.Normal(p[0], p[1]),
                1: lambda: D.Uniform(p[0], p[1]), 3: lambda: D.Poisson(p[0]), 4: lambda: D.Bernoulli(p[0])}
        return ctor[int(kind)]()

    def logweight_cpu(lw, kinds, params, strides, x, scales, rows, lp_out, n):
        idx = torch.arange(n) if rows is None else rows
        for q, kind in enumerate(kinds):
            xv = x[q].reshape(-1).expand(n)[idx]
            if int(kind) == 2:
                lp = xv.clone()
            else:
                ps = [None if t is None else t.reshape(-1).expand(n)[idx] for t in params[4 * q:4 * q + 4]]
                lp = dist(kind, ps, 0).log_prob(xv).reshape(-1).float()
            if lp_out is not None:
                lp_out[idx] = lp
            if lw is not None:
                lw[idx] += float(scales[q]) * lp

    def draw_cpu(kind, params, strides, rows, out, seed, offset, stream_id):
        n = out.numel()
        idx = torch.arange(n) if rows is None else rows
        ps = [None if t is None else t.reshape(-1).expand(n)[idx] for t in params]
        out[idx] = torch.as_tensor(dist(kind, ps, 0).sample(), dtype=torch.float32).reshape(-1).expand(idx.numel())

    P._lib.impl('dist_logweight', logweight_cpu, 'CPU')
    P._lib.impl('dist_draw', draw_cpu, 'CPU')
    _DIST_CPU_REGISTERED.append(True)


@pytest.mark.skipif(not os.path.isdir('/root/reference/pyprob'), reason='needs the live reference')
def test_pyprob_program_with_gamma_likelihood_and_factor_takes_the_lockstep_executor(monkeypatch):
    """pyprob's own Model with a Gamma likelihood and pyprob.factor, IC posterior through the binding (install()): the program
    takes the lock-step executor (pyprob.factor forwarded to the mirror's factor, no longer refused), and the two terms add to
    each particle's log-weight exactly what pyprob's own classes give, evaluated one particle at a time on the host."""
    import sys
    import warnings
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, '/root/reference')
    import pyprob
    from pyprob import InferenceEngine as PIE, InferenceNetwork as PIN
    from pyprob.distributions import Gamma as PGamma, Normal as PNormal
    import oracle_ops
    import pyprob_amd.binding as hip

    def cpu_engine(spec, device):
        eng = oracle_ops.CpuBufferEngine(spec)
        eng._use_ops = True
        return eng
    _register_dist_cpu_doubles()
    monkeypatch.setattr(hip._HipNetworkMixin, '_hip_device', 'cpu')
    monkeypatch.setattr(hip._HipNetworkMixin, '_hip_engine_factory', staticmethod(cpu_engine))
    monkeypatch.setenv('PP_PYTHON_LOOP', '1')
    monkeypatch.setenv('PYPROB_HIP_FAST_TRAIN', '0')
    monkeypatch.setenv('PYPROB_HIP_LOCKSTEP', '1')

    class GammaFactor(pyprob.Model):
        def __init__(self):
            self.extra = True
            super().__init__('Gaussian with a Gamma likelihood and a factor')

        def forward(self):
            mu = pyprob.sample(PNormal(1, math.sqrt(5)))
            likelihood = PNormal(mu, math.sqrt(2))
            pyprob.observe(likelihood, name='obs0')
            pyprob.observe(likelihood, name='obs1')
            if self.extra:
                pyprob.observe(PGamma(3.0, torch.exp(0.2 * mu)), name='y')
                pyprob.factor(log_prob=-0.05 * mu * mu)
            return mu

    hip.install()
    try:
        pyprob.seed(2)
        model = GammaFactor()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model.learn_inference_network(num_traces=64, batch_size=32, inference_network=PIN.LSTM, lstm_dim=16,
                                          observe_embeddings={'obs0': {'dim': 8}, 'obs1': {'dim': 8}})
            obs = {'obs0': 8.0, 'obs1': 9.0, 'y': 2.5}
            n = 64
            model.posterior_results(4, inference_engine=PIE.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe=obs)   # (the probe)
            pyprob.seed(5)
            a = model.posterior_results(n, inference_engine=PIE.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe=obs)
            model.extra = False
            pyprob.seed(5)
            b = model.posterior_results(n, inference_engine=PIE.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe=obs)
    finally:
        hip.uninstall()
    assert a._hip_executor['executor'] == 'lock step' and b._hip_executor['executor'] == 'lock step'
    mu_a, mu_b = a._hip._all_values, b._hip._all_values
    assert torch.equal(mu_a, mu_b)                   # same seed, same proposal: the runs differ only by the two terms
    extra = (a._hip._all_log_weights.double() - b._hip._all_log_weights.double()).numpy()
    host = [float(PGamma(3.0, torch.exp(0.2 * m)).log_prob(torch.tensor(2.5))) + float(-0.05 * m * m) for m in mu_a.reshape(-1)]
    np.testing.assert_allclose(extra, host, rtol=1e-4, atol=1e-4)
