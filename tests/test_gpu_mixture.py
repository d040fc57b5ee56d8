"""The Mixture family on the device: pp_mix_logweight / pp_mix_draw (csrc/dist_kernels.hip) through torch.ops.pyprob_hip.mix_*,
against the reference's recorded values (tests/golden/mixture_lp.npz), float64 restatements and pp_dist_draw, and the engines that
use them: lock-step prior IS, IC lock-step, lock-step prior traces and online training of a program with a mixture likelihood."""
import math

import numpy as np
import pytest
import torch

import mixture_cases as MC
import pyprob_amd
from helpers import chi2_p
from pyprob_amd import distributions as D
from pyprob_amd.model import Model
from pyprob_amd.state import InferenceEngine

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
IS = InferenceEngine.IMPORTANCE_SAMPLING
N_DRAWS = 1 << 20


@pytest.fixture(scope='module')
def ops():
    from pyprob_amd import build as B
    B.build()
    torch.cuda.set_device(0)
    from pyprob_amd.ops import ops as O
    return O


def _dev(v):
    return torch.as_tensor(v, dtype=torch.float32).reshape(-1).to(DEV).contiguous()


def mix_lp(ops, names, params, probs, x, scale=1.0, lw=None, rows=None, want_lp=True):
    x = _dev(x)
    n = x.numel() if lw is None else lw.numel()
    kinds, ps, ss = MC.op_args(names, params, DEV)
    lp = torch.full((n,), 7.0, dtype=torch.float32, device=DEV) if want_lp else None
    ops.mix_logweight(lw, kinds, ps, ss, _dev(probs), x, float(scale), rows, lp, n)
    return lp


def mix_draw(ops, names, params, probs, n=N_DRAWS, seed=1234, offset=0, stream=7, rows=None):
    kinds, ps, ss = MC.op_args(names, params, DEV)
    out = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    ops.mix_draw(kinds, ps, ss, _dev(probs), rows, out, seed, offset, stream)
    return out


def dist_draw(ops, name, p, n, seed=1234, offset=0, stream=7):
    kinds, ps, ss = MC.op_args([name], [p], DEV)
    out = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    ops.dist_draw(kinds[0], ps, ss, None, out, seed, offset, stream)
    return out


# ---- log-density -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MC.cases())
def test_log_density_matches_reference_and_float64(ops, case):
    g = MC.golden()
    names = [str(s) for s in g[case + '_names']]
    params, probs, xs, ref = g[case + '_params'], g[case + '_probs'], g[case + '_x'], g[case + '_lp']
    tol = 1e-4 if set(names) & {'Binomial', 'VonMises'} else 1e-5        # (per family, as test_gpu_dist_kernels.py has it)
    if probs.ndim == 1:      # V values, shared parameters: one launch of n = V
        got = mix_lp(ops, names, [[float(params[k, q, 0]) for q in range(4)] for k in range(len(names))], probs, xs).cpu().numpy()
        f64 = MC.mix_lp64(names, [[float(params[k, q, 0]) for q in range(4)] for k in range(len(names))], probs, xs)
    else:                    # one launch of n = B per value row: per-particle parameters and weights
        B = probs.shape[0]
        per = [[np.broadcast_to(params[k, q], (B,)).copy() for q in range(4)] for k in range(len(names))]
        got = np.stack([mix_lp(ops, names, per, probs, x).cpu().numpy() for x in xs])
        f64 = np.stack([MC.mix_lp64(names, per, probs, x) for x in xs])
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, err_msg=case)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and not np.isnan(got).any()
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], f64[fin], rtol=2e-4, atol=2e-4, err_msg=case + ' (float64)')
    assert np.array_equal(np.isneginf(f64), np.isneginf(ref))


def test_every_component_out_of_support_is_exactly_minus_inf(ops):
    lp = mix_lp(ops, ['Uniform', 'Exponential', 'Gamma', 'LogNormal'], [[0.0, 1.0], [1.0], [2.0, 1.0], [0.0, 1.0]], [1.0, 0.0, 2.0, 5.0],
                [-1.0, -1e-30, -40.0]).cpu()
    assert bool((lp == -math.inf).all()), lp
    nan = mix_lp(ops, ['Normal', 'Normal'], [[float('nan'), 1.0], [0.0, 1.0]], [0.5, 0.5], [0.3]).cpu()
    assert bool(torch.isnan(nan).all())          # a NaN parameter propagates


def _random_problem(n, K, seed):
    """K components of mixed families with per-particle parameters, per-particle weights [n, K] (some zero) and values."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: torch.rand(n, generator=gen) * (hi - lo) + lo  # noqa: E731
    fams = ['Normal', 'Gamma', 'Exponential', 'Uniform', 'LogNormal', 'Weibull', 'TruncatedNormal', 'Beta']
    names, params = [], []
    for k in range(K):
        nm = fams[(k + (K == 1)) % len(fams)]      # (K = 1: a Gamma, so that the support matters)
        names.append(nm)
        params.append({'Normal': [r(-2, 2), r(0.3, 2)], 'Gamma': [r(0.5, 4), 1.5], 'Exponential': [r(0.2, 3)], 'Uniform': [-1.0, r(0.5, 3)],
                       'LogNormal': [r(-1, 1), 0.7], 'Weibull': [r(0.5, 2), r(0.8, 3)], 'TruncatedNormal': [r(-1, 1), r(0.5, 2), -2.0, 3.0],
                       'Beta': [r(0.6, 3), 2.0, -1.0, r(2, 4)]}[nm])
    probs = torch.rand(n, K, generator=gen) * (torch.rand(n, K, generator=gen) > 0.2)
    probs[:, 0] += 0.05
    x = r(-2.5, 3.5)
    return names, params, probs, x


@pytest.mark.parametrize('n,K', [(1, 3), (255, 1), (257, 16), (2048 * 256 + 257, 3)])
def test_per_particle_parameters_and_weights_against_float64(ops, n, K):
    names, params, probs, x = _random_problem(n, K, seed=n + K)
    got = mix_lp(ops, names, params, probs, x).cpu().numpy()
    p64 = [[v.numpy() if torch.is_tensor(v) else v for v in p] for p in params]
    ref = MC.mix_lp64(names, p64, probs.numpy(), x.numpy())
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and not np.isnan(got).any()
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-4, atol=2e-4)


def test_row_lists_scale_and_lp_out(ops):
    n = 5000
    names, params, probs, x = _random_problem(n, 5, seed=11)
    full = mix_lp(ops, names, params, probs, x)
    torch.manual_seed(0)
    base = torch.randn(n, device=DEV)
    lw = base.clone()
    lp2 = mix_lp(ops, names, params, probs, x, scale=0.25, lw=lw)
    assert torch.equal(lp2, full)                                    # lp_out is unscaled
    fin = torch.isfinite(full)
    assert torch.equal(lw[fin], (base + 0.25 * full)[fin]) and bool((lw[~fin] == -math.inf).all())
    rows = torch.nonzero(torch.rand(n, device=DEV) < 0.3).reshape(-1)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[rows] = True
    lwr = base.clone()
    lpr = mix_lp(ops, names, params, probs, x, scale=0.25, lw=lwr, rows=rows)
    assert torch.equal(lpr[mask], full[mask]) and bool((lpr[~mask] == 7.0).all())
    assert torch.equal(lwr[mask], lw[mask])                          # listed rows: the full launch, bitwise
    assert torch.equal(lwr[~mask], base[~mask])                      # unlisted rows bit-unchanged
    lwo = base.clone()
    assert mix_lp(ops, names, params, probs, x, scale=2.0, lw=lwo, want_lp=False) is None
    assert torch.equal(lwo[fin], (base + 2.0 * full)[fin])


def test_operator_argument_checks(ops):
    out = torch.zeros(8, device=DEV)
    kinds, ps, ss = MC.op_args(['Normal', 'Normal'], [[0.0, 1.0], [1.0, 1.0]], DEV)
    with pytest.raises(RuntimeError):
        ops.mix_draw(kinds, ps, ss, _dev([0.5, 0.5, 0.5]), None, out, 1, 0, 7)               # probs of neither K nor n K elements
    with pytest.raises(RuntimeError):
        ops.mix_draw(kinds, ps, ss, _dev([0.5, 0.5]), None, out, 1, 0, 0x80000001)           # the selection stream's bit
    with pytest.raises(RuntimeError):
        ops.mix_draw([0, 5], ps, ss, _dev([0.5, 0.5]), None, out, 1, 0, 7)                   # a Categorical component
    with pytest.raises(RuntimeError):
        ops.mix_logweight(None, kinds, ps, ss, _dev([0.5, 0.5]), out, 1.0, None, None, 8)     # neither lw nor lp_out


# ---- draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,p', [('Normal', (1.0, 2.0)), ('Gamma', (0.7, 2.0)), ('TruncatedNormal', (0.0, 1.0, 0.5, 3.0))])
def test_one_component_or_identical_components_are_dist_draw_bitwise(ops, name, p):
    n = 200001
    ref = dist_draw(ops, name, p, n, seed=5, offset=1000, stream=9)
    assert torch.equal(mix_draw(ops, [name], [p], [1.0], n=n, seed=5, offset=1000, stream=9), ref)
    assert torch.equal(mix_draw(ops, [name] * 3, [p] * 3, [0.2, 0.5, 0.3], n=n, seed=5, offset=1000, stream=9), ref)
    gen = torch.Generator().manual_seed(1)
    per = [torch.rand(n, generator=gen) + 0.5 if q == 1 else v for q, v in enumerate(p)]       # a per-particle second parameter
    assert torch.equal(mix_draw(ops, [name], [per], [3.0], n=n, seed=5, stream=9), dist_draw(ops, name, per, n, seed=5, stream=9))


def test_a_zero_weight_component_of_another_kind_changes_nothing(ops):
    a, b, c = (-1.0, 0.5), (2.0, 0.25), (10.0, 11.0)
    two = mix_draw(ops, ['Normal', 'Normal'], [a, b], [0.3, 0.7], n=300000)
    three = mix_draw(ops, ['Normal', 'Normal', 'Uniform'], [a, b, c], [0.3, 0.7, 0.0], n=300000)       # two launches
    assert torch.equal(two, three) and bool((two != -7.0).all())


def test_normal_mixture_ks(ops):
    names, params, probs = ['Normal'] * 3, [(0.0, 0.1), (2.0, 0.1), (3.0, 0.5)], [0.7, 0.2, 0.1]
    v = mix_draw(ops, names, params, probs).cpu().numpy()
    assert np.isfinite(v).all()
    Dk = MC.ks_distance(v, lambda x: MC.mix_cdf64(names, params, probs, x))
    assert Dk < 2.5 / math.sqrt(v.size), Dk


def test_heterogeneous_mixture_ks_frequencies_and_every_launch_ran(ops):
    names, params, probs = ['Normal', 'Exponential', 'Uniform'], [(-50.0, 0.1), (1.0,), (100.0, 101.0)], [0.25, 0.5, 0.25]
    v = mix_draw(ops, names, params, probs).cpu().numpy()
    assert np.isfinite(v).all() and not (v == -7.0).any()            # no sentinel survives: every kind's launch wrote its lanes
    Dk = MC.ks_distance(v, lambda x: MC.mix_cdf64(names, params, probs, x))
    assert Dk < 2.5 / math.sqrt(v.size), Dk
    counts = np.array([(v < -40).sum(), ((v >= 0) & (v < 90)).sum(), (v >= 100).sum()], np.float64)
    assert counts.sum() == v.size
    assert chi2_p(counts, np.asarray(probs)) > 1e-5, counts


def test_per_particle_weights_select_by_row(ops):
    n, K = 4099, 4
    centres = [-30.0, -10.0, 10.0, 30.0]
    probs = torch.zeros(n, K)
    probs[torch.arange(n), torch.arange(n) % K] = 1.0
    v = mix_draw(ops, ['Normal'] * K, [(c, 0.5) for c in centres], probs, n=n).cpu().numpy()
    want = np.asarray(centres)[np.arange(n) % K]
    assert (np.abs(v - want) < 5.0).all()          # 10 standard deviations: a wrong row stride lands 20 or more away


def test_counters_rows_and_offsets(ops):
    names, params, probs = ['Gamma', 'TruncatedNormal', 'Normal'], [(0.7, 2.0), (0.0, 1.0, 0.5, 3.0), (-4.0, 0.3)], [0.3, 0.3, 0.4]
    n = 100000
    a = mix_draw(ops, names, params, probs, n=n, seed=99, stream=3)
    assert torch.equal(a, mix_draw(ops, names, params, probs, n=n, seed=99, stream=3))
    assert not torch.equal(a, mix_draw(ops, names, params, probs, n=n, seed=99, stream=4))
    assert not torch.equal(a, mix_draw(ops, names, params, probs, n=n, seed=98, stream=3))
    rows = torch.nonzero(torch.rand(n, device=DEV) < 0.4).reshape(-1)
    r = mix_draw(ops, names, params, probs, n=n, seed=99, stream=3, rows=rows)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[rows] = True
    assert torch.equal(r[mask], a[mask]) and bool((r[~mask] == -7.0).all())
    h = mix_draw(ops, names, params, probs, n=n // 2, seed=99, stream=3, offset=n // 2)
    assert torch.equal(h, a[n // 2:])              # counter = offset + particle, for the selection and for the draw


def test_bad_component_parameters_give_nan_not_a_hang(ops):
    v = mix_draw(ops, ['Gamma', 'TruncatedNormal', 'VonMises'], [(-1.0, 1.0), (0.0, 1.0, 1.0, -1.0), (0.0, -1.0)], [1.0, 1.0, 1.0], n=4096)
    torch.cuda.synchronize()
    assert torch.isnan(v).all()


# ---- engines ---------------------------------------------------------------------------------------------------------------
S_OBS = 0.5
PROBS = [0.3, 0.7]


def _host(t):
    return t.detach().double().cpu().numpy()


class MirroredGMM(Model):
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(0.0, 2.0))
        pyprob_amd.observe(D.Mixture([D.Normal(mu, S_OBS), D.Normal(-mu, S_OBS)], probs=PROBS), name='y')
        return torch.abs(mu)


def _gmm_lp64(mu, y):
    return MC.mix_lp64(['Normal', 'Normal'], [[mu, S_OBS], [-mu, S_OBS]], PROBS, np.full_like(mu, y))


def test_lock_step_prior_is_of_a_mixture_likelihood():
    n, y = 20000, 1.5
    post = MirroredGMM().posterior_results(n, IS, observe={'y': y}, lock_step=True, seed=5)
    assert post.num_paths == 1 and post.length == n
    mu = _host(next(iter(post.statement_log[0].values()))[0])
    lw, v = _host(post._all_log_weights), _host(post._all_values)
    assert np.array_equal(v, np.abs(mu))
    np.testing.assert_allclose(lw, _gmm_lp64(mu, y), rtol=0, atol=1e-4)          # every particle re-scored in float64
    grid = np.linspace(-20.0, 20.0, 400001)
    lp = MC.comp_lp64('Normal', [0.0, 2.0], grid) + _gmm_lp64(grid, y)
    wq = np.exp(lp - lp.max())
    exact = float((wq * np.abs(grid)).sum() / wq.sum())
    w = np.exp(lw - lw.max())
    w /= w.sum()
    est = float((w * v).sum())
    se = math.sqrt(float((w * w * (v - est) ** 2).sum()))                        # from the weighted sample itself
    assert abs(est - exact) < 5 * se, (est, exact, se)
    assert float(post.mean) == pytest.approx(est, abs=1e-5)


class MixturePrior(Model):
    def forward(self):
        z = pyprob_amd.sample(D.Mixture([D.Normal(-3.0, 0.5), D.Exponential(2.0), D.Uniform(4.0, 5.0)], probs=[1.0, 2.0, 1.0]))
        pyprob_amd.observe(D.Normal(z, 1.5), name='y')
        return z


def test_mixture_as_a_prior_is_drawn_on_the_device_and_adds_no_weight():
    n = 1 << 17
    post = MixturePrior().posterior_results(n, IS, observe={'y': 0.5}, lock_step=True, seed=2)
    z = _host(post._all_values)
    names, params, probs = ['Normal', 'Exponential', 'Uniform'], [(-3.0, 0.5), (2.0,), (4.0, 5.0)], [1.0, 2.0, 1.0]
    Dk = MC.ks_distance(z.astype(np.float32), lambda x: MC.mix_cdf64(names, params, probs, x))
    assert Dk < 2.5 / math.sqrt(n), Dk
    np.testing.assert_allclose(_host(post._all_log_weights), MC.comp_lp64('Normal', [z, 1.5], np.full(n, 0.5)), rtol=0, atol=1e-4)
    again = MixturePrior().posterior_results(n, IS, observe={'y': 0.5}, lock_step=True, seed=2)
    assert torch.equal(again._all_values, post._all_values)


class BranchThenMixture(Model):
    """Marsaglia's rejection loop (a per-particle branch: several control-flow paths), then a mixture likelihood on each path's rows."""
    def forward(self):
        u = D.Uniform(-1.0, 1.0)
        s = 1
        while s >= 1:
            a = pyprob_amd.sample(u)
            b = pyprob_amd.sample(u)
            s = a * a + b * b
        mu = 1.0 + 2.0 * (a * torch.sqrt(-2 * torch.log(s) / s))
        pyprob_amd.observe(D.Mixture([D.Normal(mu, S_OBS), D.Normal(-mu, S_OBS)], probs=PROBS), name='y')
        return mu


def test_mixture_likelihood_after_a_branch_uses_the_row_lists():
    n = 4096
    post = BranchThenMixture().posterior_results(n, IS, observe={'y': 1.5}, lock_step=True, seed=3)
    assert post.num_paths >= 2
    mu = _host(post._all_values)
    np.testing.assert_allclose(_host(post._all_log_weights), _gmm_lp64(mu, 1.5), rtol=0, atol=1e-4)


class ICMixtureOrFactor(Model):
    """A controlled Normal (proposed by the network), two Normal observations, and a third term that is either
    observe(Mixture) or a factor computing the same density with torch on the sampled values."""
    as_factor = False

    def forward(self):
        mu = pyprob_amd.sample(D.Normal(1.0, math.sqrt(5)))
        lik = D.Normal(mu, math.sqrt(2))
        pyprob_amd.observe(lik, name='obs0')
        pyprob_amd.observe(lik, name='obs1')
        rate = torch.exp(0.2 * mu)
        if self.as_factor:
            def density(x):
                x = torch.as_tensor(x, dtype=torch.float32)
                la = math.log(PROBS[0]) - (x - mu) ** 2 / (2 * S_OBS ** 2) - math.log(S_OBS) - 0.5 * math.log(2 * math.pi)
                lb = math.log(PROBS[1]) + 3.0 * torch.log(rate) + 2.0 * torch.log(x) - rate * x - math.lgamma(3.0)
                m = torch.maximum(la, lb)
                return m + torch.log(torch.exp(la - m) + torch.exp(lb - m))
            pyprob_amd.factor(log_prob_func=density, name='y')
        else:
            pyprob_amd.observe(D.Mixture([D.Normal(mu, S_OBS), D.Gamma(3.0, rate)], probs=PROBS), name='y')
        return mu


def test_ic_lock_step_mixture_observe_equals_the_factor_of_the_same_density():
    """The golden GUM network (trained by the reference, H = 64) with its address renamed to this program's statement, as
    test_gpu_prior_is_lockstep._ic_uncontrolled_model does."""
    from conftest import load_golden
    from helpers import spec_from_golden
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.state import TraceMode
    IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
    meta, params, batch, loss, isr = load_golden('gum')
    model = ICMixtureOrFactor()
    tr = next(model._trace_generator(trace_mode=TraceMode.PRIOR))
    new, old = tr.variables[0].address, meta['addresses'][0]
    params = {k.replace(old, new): v for k, v in params.items()}
    meta = dict(meta, addresses=[new])
    net = InferenceNetworkLSTM(observe_embeddings={n: {'dim': meta['observe_embedding_dims'][n]} for n in meta['obs_names']},
                               lstm_dim=64, device=DEV)
    net._obs_names = list(meta['obs_names'])
    net._engine = ICEngine(spec_from_golden(meta, params), device=DEV, seed=0)
    net._engine.load_state_dict(params)
    net._is = ISRunner(net._engine)
    net._layers_initialized = True
    model._inference_network = net
    obs = {'obs0': 8.0, 'obs1': 9.0, 'y': 6.5}
    assert model._lock_step_safe(obs)                    # the probe accepts a program with a mixture likelihood
    n = 20000
    a = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=7)
    model.as_factor = True
    b = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=7)
    assert torch.equal(a._all_values, b._all_values)
    assert bool(torch.isfinite(a._all_log_weights).all())
    np.testing.assert_allclose(_host(a._all_log_weights), _host(b._all_log_weights), rtol=0, atol=1e-4)
    mu = _host(a._all_values)
    extra = MC.mix_lp64(['Normal', 'Gamma'], [[mu, S_OBS], [3.0, np.exp(np.float32(0.2) * mu.astype(np.float32)).astype(np.float64)]],
                        PROBS, np.full(n, 6.5))
    assert float(np.abs(extra).max()) > 1.0              # the term is no rounding matter


def test_controlled_mixture_sample_is_refused_under_the_network():
    class Controlled(Model):
        def forward(self):
            z = pyprob_amd.sample(D.Mixture([D.Normal(0.0, 1.0), D.Normal(3.0, 1.0)]))
            pyprob_amd.observe(D.Normal(z, 1.0), name='y')
            return z
    with pytest.raises(RuntimeError, match='Distribution currently unsupported: Mixture'):
        Controlled().prior_traces_packed(8, ['y'], device=DEV)


def test_prior_traces_packed_draws_the_mixture_observation_on_the_device():
    n = 100000
    torch.manual_seed(4)
    lens, table, ids, vals, prior, obs = MirroredGMM().prior_traces_packed(n, ['y'], device=DEV)
    assert lens.tolist() == [1] * n and obs.shape == (n, 1) and np.isfinite(obs).all()
    mu, y = vals.astype(np.float64), obs[:, 0].astype(np.float64)
    # y | mu ~ 0.3 Normal(mu, s) + 0.7 Normal(-mu, s): its own CDF at y is uniform on (0, 1)
    u = MC.mix_cdf64(['Normal', 'Normal'], [(mu, S_OBS), (-mu, S_OBS)], PROBS, y)
    u = np.sort(u)
    i = np.arange(1, n + 1, dtype=np.float64)
    Dk = max(float((i / n - u).max()), float((u - (i - 1) / n).max()))
    assert Dk < 2.5 / math.sqrt(n), Dk
    far = np.abs(mu) > 3 * S_OBS
    first = np.abs(y[far] - mu[far]) < np.abs(y[far] + mu[far])
    assert abs(first.mean() - 0.3) < 5 * math.sqrt(0.21 / far.sum())


def test_online_training_of_a_program_with_a_mixture_likelihood():
    from pyprob_amd.state import InferenceNetwork
    torch.manual_seed(6)
    model = MirroredGMM()
    model.learn_inference_network(num_traces=2048, inference_network=InferenceNetwork.LSTM, observe_embeddings={'y': {'dim': 8}},
                                  batch_size=64, lstm_dim=32, seed=6, vectorised_prior=True, device=DEV)
    net = model._inference_network
    assert net._total_train_traces == 2048 and net._total_train_iterations == 32        # the reference's counters
    losses = np.asarray([float(v) for v in net._history_train_loss], np.float64)
    assert losses.size > 0 and np.isfinite(losses).all()
