"""posterior_results(IMPORTANCE_SAMPLING, lock_step=True): the prior-proposal engine with all particles in lock step on the
device (state.PriorISState + is_engine.DistRunner; draws by pp_dist_draw, terms by pp_dist_logweight / the rows kernels).
Every particle's log-weight is re-scored in float64 from the values it returns; the posteriors are checked against closed
forms, the reference's thresholds and the per-trace engine."""
import math

import numpy as np
import pytest
import torch

import pyprob_amd
from pyprob_amd import distributions as D
from pyprob_amd.model import Model
from pyprob_amd.state import InferenceEngine
from models import GaussianWithUnknownMean, GaussianWithUnknownMeanMarsagliaLockStep

pytestmark = pytest.mark.gpu
IS = InferenceEngine.IMPORTANCE_SAMPLING


@pytest.fixture(scope='module', autouse=True)
def built():
    from pyprob_amd import build as B
    B.build()
    torch.cuda.set_device(0)


def _lp_normal(x, m, s):
    return -0.5 * ((x - m) / s) ** 2 - math.log(s) - 0.5 * math.log(2 * math.pi)


def _host(t):
    return t.detach().double().cpu().numpy()


def _weighted(post):
    v, lw = _host(post._values), _host(post._log_weights)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    m = float((w * v).sum())
    return m, math.sqrt(float((w * (v - m) ** 2).sum())), 1.0 / float((w * w).sum())


def test_gum_lockstep_rescored_reference_thresholds_seed_and_offset():
    model = GaussianWithUnknownMean()
    n = 10 ** 6
    post = model.posterior_results(n, IS, observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=5)
    assert post.length == n and post.num_paths == 1
    mu, lw = _host(post._values), _host(post._log_weights)
    s = math.sqrt(2)
    ref = _lp_normal(8.0, mu, s) + _lp_normal(9.0, mu, s)      # prior IS: the weight is the likelihood
    np.testing.assert_allclose(lw, ref, rtol=1e-5, atol=1e-5)
    # reference tests/test_inference.py:118-145: posterior Normal(7.25, sqrt(1/1.2)), deltas 0.75 / 0.75
    assert abs(float(post.mean) - 7.25) < 0.75
    assert abs(float(post.stddev) - math.sqrt(1 / 1.2)) < 0.75
    m, sd, ess = _weighted(post)
    assert abs(m - 7.25) < 0.05 and abs(sd - math.sqrt(1 / 1.2)) < 0.05 and ess > 0.005 * n
    again = model.posterior_results(n, IS, observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=5)
    assert torch.equal(again._values, post._values) and torch.equal(again._log_weights, post._log_weights)
    a = model.posterior_results(n // 2, IS, observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=5)
    b = model.posterior_results(n // 2, IS, observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=5, offset=n // 2)
    assert torch.equal(torch.cat([a._values, b._values]), post._values)
    assert torch.equal(torch.cat([a._log_weights, b._log_weights]), post._log_weights)


def test_marsaglia_lockstep_diverges_and_agrees_with_per_trace():
    model = GaussianWithUnknownMeanMarsagliaLockStep()
    post = model.posterior_results(200000, IS, observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=3)
    assert post.num_paths >= 2
    mu, lw = _host(post._values), _host(post._log_weights)
    s = math.sqrt(2)
    np.testing.assert_allclose(lw, _lp_normal(8.0, mu, s) + _lp_normal(9.0, mu, s), rtol=1e-5, atol=1e-4)
    m, sd, _ = _weighted(post)
    assert abs(m - 7.25) < 0.1 and abs(sd - math.sqrt(1 / 1.2)) < 0.1
    torch.manual_seed(0)
    ref = model.posterior_results(3000, IS, observe={'obs0': 8, 'obs1': 9})
    assert abs(float(ref.mean) - m) < 0.3 and abs(float(ref.stddev) - sd) < 0.3


class GammaPoisson(Model):
    def forward(self):
        rate = pyprob_amd.sample(D.Gamma(3.0, 1.5))
        for i in range(4):
            pyprob_amd.observe(D.Poisson(rate), name='k%d' % i)
        return rate


class BetaBinomial(Model):
    def forward(self):
        p = pyprob_amd.sample(D.Beta(2.0, 3.0))
        pyprob_amd.observe(D.Binomial(total_count=40, probs=p), name='k')
        return p


class GammaExponential(Model):
    def forward(self):
        lam = pyprob_amd.sample(D.Gamma(2.0, 1.0))
        for i in range(3):
            pyprob_amd.observe(D.Exponential(lam), name='y%d' % i)
        return lam


class NormalLogNormal(Model):
    def forward(self):
        m = pyprob_amd.sample(D.Normal(0.0, 1.0))
        pyprob_amd.observe(D.LogNormal(m, 0.5), name='y0')
        pyprob_amd.observe(D.LogNormal(m, 0.5), name='y1')
        return m


def test_conjugate_posteriors():
    n = 10 ** 6
    post = GammaPoisson().posterior_results(n, IS, observe={'k0': 2, 'k1': 4, 'k2': 3, 'k3': 5}, lock_step=True, seed=1)
    assert _weighted(post)[0] == pytest.approx(17 / 5.5, abs=0.02)               # Gamma(3 + 14, 1.5 + 4)
    post = BetaBinomial().posterior_results(n, IS, observe={'k': 28}, lock_step=True, seed=2)
    assert _weighted(post)[0] == pytest.approx(30 / 45, abs=0.005)               # Beta(2 + 28, 3 + 12)
    p = _host(post._values)
    lw = _host(post._log_weights)
    logit = np.log(np.clip(p, 1.2e-7, 1 - 1.2e-7)) - np.log1p(-np.clip(p, 1.2e-7, 1 - 1.2e-7))
    ref = (math.lgamma(41) - math.lgamma(29) - math.lgamma(13) + 28 * logit - 40 * np.logaddexp(0, logit))
    ok = np.isfinite(lw)
    np.testing.assert_allclose(lw[ok], ref[ok], rtol=1e-4, atol=1e-3)
    post = GammaExponential().posterior_results(n, IS, observe={'y0': 0.5, 'y1': 1.2, 'y2': 0.3}, lock_step=True, seed=3)
    assert _weighted(post)[0] == pytest.approx(5 / 3.0, abs=0.01)                # Gamma(2 + 3, 1 + 2)
    ys = (1.5, 2.5)
    post = NormalLogNormal().posterior_results(n, IS, observe={'y0': ys[0], 'y1': ys[1]}, lock_step=True, seed=4)
    prec = 1 + 2 / 0.25
    assert _weighted(post)[0] == pytest.approx(sum(math.log(y) for y in ys) / 0.25 / prec, abs=0.01)


class WeibullVonMisesTN(Model):
    def forward(self):
        k = pyprob_amd.sample(D.Weibull(1.5, 2.0))
        mu = pyprob_amd.sample(D.VonMises(0.5, 2.0))
        t = pyprob_amd.sample(D.TruncatedNormal(0.0, 1.0, -1.0, 2.0))
        pyprob_amd.observe(D.Weibull(k, 1.5), name='w')
        pyprob_amd.observe(D.VonMises(mu, 4.0), name='v')
        pyprob_amd.observe(D.TruncatedNormal(t, 0.5, -2.0, 3.0), name='t')
        return k * 100 + mu * 10 + t       # (unused: the values come from the statement log)


def test_weibull_vonmises_truncnormal_rescored():
    n = 10 ** 6
    post = WeibullVonMisesTN().posterior_results(n, IS, observe={'w': 1.1, 'v': 0.2, 't': 0.7}, lock_step=True, seed=8)
    log = post.statement_log
    k, mu, t = (_host(next(iter(log[j].values()))[0]) for j in range(3))
    assert (k > 0).all() and (np.abs(mu) <= math.pi).all() and (t >= -1).all() and (t <= 2).all()
    x = 1.1
    ref = np.log(1.5) - np.log(k) + 0.5 * np.log(x / k) - (x / k) ** 1.5
    ref += 4.0 * np.cos(0.2 - mu) - math.log(2 * math.pi) - math.log(np.i0(4.0))
    Z = 0.5 * (np.vectorize(math.erf)((3.0 - t) / 0.5 / math.sqrt(2)) - np.vectorize(math.erf)((-2.0 - t) / 0.5 / math.sqrt(2)))
    ref += _lp_normal(0.7, t, 0.5) - np.log(Z)
    np.testing.assert_allclose(_host(post._all_log_weights), ref, rtol=1e-4, atol=2e-4)


class FactorModel(Model):
    """reference tests/test_state.py:33-45"""
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(1.0, math.sqrt(5)))
        likelihood = D.Normal(mu, math.sqrt(2))
        pyprob_amd.factor(log_prob_func=lambda x: likelihood.log_prob(x), name='obs0')
        pyprob_amd.factor(log_prob_func=lambda x: likelihood.log_prob(x), name='obs1')
        return mu


class FactorModel2(Model):
    """reference tests/test_state.py:47-59"""
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(1.0, math.sqrt(5)))
        likelihood = D.Normal(mu, math.sqrt(2))
        pyprob_amd.factor(log_prob=likelihood.log_prob(8))
        pyprob_amd.factor(log_prob=likelihood.log_prob(9))
        return mu


@pytest.mark.parametrize('model_cls', [FactorModel, FactorModel2])
def test_factor_models(model_cls):
    n = 10 ** 6
    post = model_cls().posterior_results(n, IS, observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=11)
    # reference tests/test_state.py:65-80: posterior Normal(7.25, sqrt(1/1.2)), deltas 0.75
    assert abs(float(post.mean) - 7.25) < 0.75
    assert abs(float(post.stddev) - math.sqrt(1 / 1.2)) < 0.75
    mu, lw = _host(post._values), _host(post._log_weights)
    np.testing.assert_allclose(lw, _lp_normal(8.0, mu, math.sqrt(2)) + _lp_normal(9.0, mu, math.sqrt(2)), rtol=1e-5, atol=1e-5)
    m, sd, _ = _weighted(post)
    assert abs(m - 7.25) < 0.05 and abs(sd - math.sqrt(1 / 1.2)) < 0.05


def test_default_engine_still_runs_per_trace():
    torch.manual_seed(0)
    post = GaussianWithUnknownMean().posterior_results(50, IS, observe={'obs0': 8, 'obs1': 9})
    assert not hasattr(post, 'num_paths') and post.length == 50


# ---- an uncontrolled sample inside an IC lock-step run (reference state.py:218-221) ----------------------------------------
class ICUncontrolledGamma(Model):
    """One controlled Normal (proposed by the network), one UNCONTROLLED Gamma whose rate depends on it (a prior draw, no
    weight term), a per-particle branch on the uncontrolled value (two control-flow paths: the second replays mu and g from
    the first's prefix) and Gamma likelihoods whose rate depends on the controlled value through exp."""
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(1.0, math.sqrt(5)))
        g = pyprob_amd.sample(D.Gamma(2.0, torch.exp(0.1 * mu)), control=False)
        rate = torch.exp(0.2 * mu)
        if g >= 1.5:
            scale = rate * 1.0
        else:
            scale = rate + 0.0
        pyprob_amd.observe(D.Gamma(3.0, scale), name='obs0')
        pyprob_amd.observe(D.Gamma(3.0, scale), name='obs1')
        return mu


def _ic_uncontrolled_model():
    """The golden GUM network (H = 64, trained by the reference) with its address renamed to this program's `mu` statement."""
    from conftest import load_golden
    from helpers import spec_from_golden
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.state import TraceMode
    meta, params, batch, loss, isr = load_golden('gum')
    assert meta['lstm_dim'] == 64
    model = ICUncontrolledGamma()
    tr = next(model._trace_generator(trace_mode=TraceMode.PRIOR))
    new, old = tr.variables[0].address, meta['addresses'][0]
    params = {k.replace(old, new): v for k, v in params.items()}
    meta = dict(meta, addresses=[new])
    spec = spec_from_golden(meta, params)
    net = InferenceNetworkLSTM(observe_embeddings={n: {'dim': meta['observe_embedding_dims'][n]} for n in meta['obs_names']},
                               lstm_dim=64, device='cuda:0')
    net._obs_names = list(meta['obs_names'])
    net._engine = ICEngine(spec, device='cuda:0', seed=0)
    net._engine.load_state_dict(params)
    net._is = ISRunner(net._engine)
    net._layers_initialized = True
    model._inference_network = net
    return model, meta, params


def test_ic_lockstep_with_an_uncontrolled_gamma_sample():
    from oracle import ic_oracle as O
    IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
    model, meta, params = _ic_uncontrolled_model()
    obs = {'obs0': 8.0, 'obs1': 9.0}
    assert model._lock_step_safe(obs)             # the probe sends the program to lock step (it used to raise there)
    n = 20000
    post = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=7)
    assert post.num_paths == 2 and post.length == n
    mu = _host(post._all_values)
    lw = _host(post._all_log_weights)
    log = post.statement_log
    (a_mu, (v_mu, id_mu)), = log[0].items()
    (a_g, (v_g, id_g)), = log[1].items()
    assert id_mu == 0 and id_g is None            # the uncontrolled statement is no network statement
    assert np.array_equal(_host(v_mu), mu)        # the program returns the controlled value
    g = _host(v_g)
    assert np.isfinite(g).all() and (g > 0).all()
    # drawn after the deferred first statement was flushed: g * exp(0.1 mu) ~ Gamma(2, 1) needs the particles' own mu
    z = g * np.exp(0.1 * mu)
    assert abs(z.mean() - 2.0) < 6 * math.sqrt(2.0 / n) and abs(z.var() - 2.0) < 0.1
    # every particle re-scored in float64: log p(mu) - log q(mu) by the oracle's network restatement (one LSTM step: the
    # uncontrolled statement is not a previous variable) + the two Gamma likelihoods; nothing of g enters the weight
    onet = O.Net(params, meta['obs_names'], K=meta['mixture_components'])
    prior = np.tile(np.array([[1.0, math.sqrt(5), 0.0]]), (n, 1))
    _, _, _, ref = O.is_rescore(onet, np.array([8.0, 9.0]), np.ones(n, np.int64), np.zeros(n, np.int64), mu, prior,
                                meta['addresses'], ['Normal'])
    rate = np.exp(0.2 * mu.astype(np.float32).astype(np.float64))
    for y in (8.0, 9.0):
        ref = ref + 3.0 * np.log(rate) + 2.0 * math.log(y) - rate * y - math.lgamma(3.0)
    np.testing.assert_allclose(lw, ref, rtol=1e-4, atol=2e-4)
