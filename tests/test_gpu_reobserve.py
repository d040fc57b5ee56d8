"""Empirical.reobserve / pyprob_amd.reobserve_batch on the device, through Model: the particles of one lock-step posterior call
re-scored under new observations (state.ReobserveState replays the program over the statement log; one pp_is_reobserve_groups call).
 1. the prior-proposal engine, whose latents depend on (seed, offset) only: the re-observed posterior has the VALUES of the direct
    call bit for bit and its log-weights within a rounding bound;
 2. the inference-network engine on the small GUM golden network (H = 64): new minus old log-weights against float64 from the
    logged latents, after a first call and after a launch-plan replay, one of two names, a [1, 8, 8] vector observe;
 3. likelihood_funcs, likelihood_importance, the statement log under the new weights, dropped particles;
 4. reobserve_batch: members bit-equal to the single calls, the *_batch statistics on their one-execution route;
 5. the errors.
PP_REOBSERVE_ERRORS=<file> makes test 1 append its largest observed error ratio to that file: profiles/reobserve_errors.jsonl."""
import json
import math
import os
import warnings

import numpy as np
import pytest

from is_helpers import lockstep_network, network_from_golden
from models import GaussianWithUnknownMean
from pyprob_amd.state import InferenceEngine

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
IS = InferenceEngine.IMPORTANCE_SAMPLING
S2 = math.sqrt(2.0)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def nlp(x, mu, sd):
    return -((x - mu) ** 2) / (2.0 * sd * sd) - np.log(sd) - HALF_LOG_2PI


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def quiet(f, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return f(*args, **kwargs)


@pytest.fixture(scope='module')
def gum():
    """The GUM program on the golden network, one first call and one launch-plan replay of 1000 particles."""
    net, meta, params, isr = network_from_golden('gum', 'cuda:0')
    model = GaussianWithUnknownMean()
    model._inference_network = net
    first = quiet(model.posterior_results, 1000, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=3)
    replay = quiet(model.posterior_results, 1000, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=4)
    return model, first, replay


# ---- 1. the prior-proposal engine: fails without the feature ---------------------------------------------------------------------
def test_prior_proposal_particles_serve_another_observation():
    """FAILS WITHOUT THE FEATURE (AttributeError: reobserve). The direct call computes lw1 = (0 + t0') + t1' with t' = scale * lp'
    rounded; the re-observed one lw0 + (s' - old) with s' the same chain over the new values and old the chain over the old ones.
    Roundings, each relative to at most the magnitude it touches: a Normal log-density in fp32 takes 8 (difference, quotient,
    square, logarithm with 2 ulp, three sums), its product with the scale 1, its place in a chain 1 - 10 per term and
    evaluation. The new terms are evaluated twice (the direct call and this one): 20 on sum |scale lp_new|; the old terms enter
    lw0 and old: 20 on sum |scale lp_old|; the difference s' - old and the sum with lw0 are 2 more on |lw0| + |old| + |s'|. In
    all at most 24 * 2^-24 * (|lw0| + sum |scale lp_old| + sum |scale lp_new|) per particle. Measured on the MI355X
    (profiles/reobserve_errors.jsonl): 0.0 - for these observations s' and lw0 = old lie within a factor of two of each other for
    every particle, so the difference and the sum are exact, and the kernels share one formula per family."""
    model = GaussianWithUnknownMean()
    N, y0, y1 = 4096, {'obs0': 8.0, 'obs1': 9.0}, {'obs0': 6.5, 'obs1': 10.25}
    post0 = model.posterior_results(N, IS, observe=y0, lock_step=True, seed=21)
    post1 = model.posterior_results(N, IS, observe=y1, lock_step=True, seed=21)
    new = post0.reobserve(observe=y1)
    assert torch.equal(new._values, post1._values) and new.length == post1.length == N
    mu = host(post0._values)
    old_terms = np.abs(nlp(8.0, mu, S2)) + np.abs(nlp(9.0, mu, S2))
    new_terms = np.abs(nlp(6.5, mu, S2)) + np.abs(nlp(10.25, mu, S2))
    assert np.all(np.isfinite(old_terms + new_terms))
    unit = 2.0 ** -24 * (np.abs(host(post0._log_weights)) + old_terms + new_terms)
    ratio = float(np.max(np.abs(host(new._log_weights) - host(post1._log_weights)) / unit))
    print('reobserve against the direct call: largest error %.3f units of 2^-24 (|lw| + sum |old| + sum |new|)' % ratio)
    if os.environ.get('PP_REOBSERVE_ERRORS'):
        with open(os.environ['PP_REOBSERVE_ERRORS'], 'a') as f:
            f.write(json.dumps(dict(test='prior_proposal_gum', n=N, observe_old=y0, observe_new=y1, bound_units=24,
                                    largest_ratio=ratio)) + '\n')
    assert ratio <= 24.0
    assert abs(new.mean - post1.mean) < 1e-4 and new.metadata['op'] == 'reobserve'
    assert sorted(new.metadata['observables']) == ['obs0', 'obs1']


# ---- 2. the inference-network engine -----------------------------------------------------------------------------------------------
def test_ic_first_call_and_plan_replay_against_float64(gum):
    model, first, replay = gum
    assert getattr(replay, 'replayed_plan', False) and not getattr(first, 'replayed_plan', False)
    assert not torch.equal(first._values, replay._values)
    for post, (a, b) in ((first, (8.0, 9.0)), (replay, (8.0, 9.0))):
        mu = host(post.statement_log[0][post.addresses[0]][0])
        new = post.reobserve(observe={'obs0': 6.25, 'obs1': 10.5})
        want = nlp(6.25, mu, S2) + nlp(10.5, mu, S2) - nlp(a, mu, S2) - nlp(b, mu, S2)
        got = host(new._all_log_weights) - host(post._all_log_weights)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(want).max()))
        assert new._values is post._values
        # one of the two names: the other term stays
        one = post.reobserve(observe={'obs1': 5.0})
        np.testing.assert_allclose(host(one._all_log_weights) - host(post._all_log_weights), nlp(5.0, mu, S2) - nlp(b, mu, S2),
                                   rtol=1e-4, atol=1e-4)
        # the original observation again: the call's log-weights bit for bit
        assert torch.equal(post.reobserve(observe={'obs0': a, 'obs1': b})._all_log_weights, post._all_log_weights)


def test_vector_observe_of_shape_1_8_8(gum):
    import pyprob_amd as pyprob
    from pyprob_amd.distributions import Normal
    base, _, _ = gum
    template = torch.linspace(-1.0, 1.0, 64, device='cuda:0').reshape(1, 8, 8)

    class WithImage(GaussianWithUnknownMean):
        def forward(self):
            mu = pyprob.sample(Normal(self.prior_mean, self.prior_stddev))
            pyprob.observe(Normal(mu, self.likelihood_stddev), name='obs0')
            pyprob.observe(Normal(mu, self.likelihood_stddev), name='obs1')
            pyprob.observe(Normal(mu.reshape(-1, 1, 1, 1) * template, 0.8), name='img')
            return mu
    model = WithImage()
    model._inference_network = base._inference_network
    img0 = torch.full((1, 8, 8), 0.5)
    img1 = torch.linspace(2.0, -1.0, 64).reshape(1, 8, 8)
    post = quiet(model.posterior_results, 777, IC, observe={'obs0': 8.0, 'obs1': 9.0, 'img': img0}, lock_step=True, seed=6)
    new = post.reobserve(observe={'img': img1})
    mu = host(post.statement_log[0][post.addresses[0]][0])
    mean = mu[:, None] * host(template).reshape(1, 64)
    want = nlp(host(img1).reshape(1, 64), mean, 0.8).sum(1) - nlp(host(img0).reshape(1, 64), mean, 0.8).sum(1)
    got = host(new._all_log_weights) - host(post._all_log_weights)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(want).max()))
    assert torch.equal(post.reobserve(observe={'img': img0})._all_log_weights, post._all_log_weights)
    both = pyprob.reobserve_batch(post, [{'img': img0}, {'img': img1}])
    assert torch.equal(both[1]._all_log_weights, new._all_log_weights)


# ---- 3. likelihoods, scales, the statement log, dropped particles -----------------------------------------------------------------
def test_likelihood_funcs_and_likelihood_importance_against_float64(gum):
    from pyprob_amd.distributions import Normal
    model, first, _ = gum
    mu, lw = host(first.statement_log[0][first.addresses[0]][0]), host(first._all_log_weights)
    calls = []

    def doubled(v, trace):
        calls.append((v.name, float(v.value), trace))
        return Normal(v.distribution.mean, 2.0 * v.distribution.stddev)
    new = first.reobserve(likelihood_funcs={'obs0': doubled})
    assert calls == [('obs0', 8.0, None)]
    np.testing.assert_allclose(host(new._all_log_weights) - lw, nlp(8.0, mu, 2.0 * S2) - nlp(8.0, mu, S2), rtol=1e-4, atol=1e-4)
    half = first.reobserve(observe={'obs0': 7.0, 'obs1': 7.0}, likelihood_importance=0.5)
    want = 0.5 * (nlp(7.0, mu, S2) + nlp(7.0, mu, S2)) - (nlp(8.0, mu, S2) + nlp(9.0, mu, S2))
    np.testing.assert_allclose(host(half._all_log_weights) - lw, want, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(want).max()))


def test_statement_log_answers_under_the_new_weights(gum):
    model, first, _ = gum
    new = first.reobserve(observe={'obs0': 6.0, 'obs1': 6.5})
    a = new.addresses[0]
    mu, lw = host(new.statement_log[0][a][0]), host(new._all_log_weights)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    mean = float((w * mu).sum())
    assert abs(new.marginal(a).mean - mean) <= 1e-5 * max(1.0, abs(mean))
    j = new.joint()
    assert abs(float(j.mean[0]) - mean) <= 1e-5 * max(1.0, abs(mean))
    assert abs(float(j.cov[0, 0]) - float((w * (mu - mean) ** 2).sum())) <= 1e-4
    assert abs(new.mean - mean) <= 1e-5 * max(1.0, abs(mean)) and abs(new.mean - first.mean) > 0.1
    assert math.isfinite(new.pareto_k()) and new.psis().length == new.length


def test_particles_outside_the_new_support_are_dropped():
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal, Uniform

    class Window(Model):
        def forward(self):
            c = pyprob.sample(Normal(0.0, 1.0), name='c')
            pyprob.observe(Uniform(c - 2.0, c + 2.0), name='y')
            return c
    N = 2000
    post = quiet(Window().posterior_results, N, IS, observe={'y': 0.0}, lock_step=True, seed=9)
    assert post.length < N          # |c| >= 2 has no mass at y = 0
    new = quiet(post.reobserve, observe={'y': 1.5})
    c = host(post._all_values)
    inside = (1.5 >= c - 2.0) & (1.5 < c + 2.0) & np.isfinite(host(post._all_log_weights))
    assert new.length == int(inside.sum()) < post.length
    assert new._all_log_weights.numel() == N and new._all_values is post._all_values
    assert np.array_equal(np.isfinite(host(new._all_log_weights)), inside)
    assert np.array_equal(host(new._values), c[inside])


# ---- 4. reobserve_batch -----------------------------------------------------------------------------------------------------------
def test_reobserve_batch_members_and_their_batch_statistics(gum):
    import pyprob_amd
    from pyprob_amd import empirical_batch as EB
    model, first, _ = gum
    rng = np.random.default_rng(5)
    observes = [{'obs0': float(np.float32(rng.uniform(6, 10))), 'obs1': float(np.float32(rng.uniform(6, 10)))} for _ in range(5)]
    members = pyprob_amd.reobserve_batch(first, observes)
    singles = [first.reobserve(observe=o) for o in observes]
    for g, (m, one) in enumerate(zip(members, singles)):
        assert torch.equal(m._all_log_weights, one._all_log_weights) and torch.equal(m._values, one._values), g
        assert m.mean == one.mean and m.effective_sample_size == one.effective_sample_size, g
    assert EB._one_execution(members) is not None and EB._batch_column(members, None) is not None
    assert np.array_equal(pyprob_amd.pareto_k_batch(members), np.array([m.pareto_k() for m in members]))
    qs = [0.05, 0.5, 0.95]
    assert np.array_equal(pyprob_amd.quantile_batch(members, qs), np.stack([m.quantile(qs) for m in members]))
    # the loops: an address, and the joint moments, from every member's shared [N] columns
    a = first.addresses[0]
    assert np.array_equal(pyprob_amd.quantile_batch(members, qs, address=a), np.stack([m.marginal(a).quantile(qs) for m in members]))
    assert np.array_equal(pyprob_amd.joint_batch(members)[2].mean, members[2].joint().mean)
    drawn = pyprob_amd.resample_batch(members, 64, seed=3)
    assert len(drawn) == 5 and drawn[4].length == 64
    # a member of a posterior_results_batch result can be re-observed on its own
    posts = quiet(model.posterior_results_batch, 500, observes[:3], seed=8)
    mu = host(posts[1].statement_log[0][posts[1].addresses[0]][0])
    new = posts[1].reobserve(observe={'obs0': 7.0})
    np.testing.assert_allclose(host(new._all_log_weights) - host(posts[1]._all_log_weights),
                               nlp(7.0, mu, S2) - nlp(observes[1]['obs0'], mu, S2), rtol=1e-4, atol=1e-4)


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(gum, monkeypatch):
    from pyprob_amd.distributions import Categorical, Empirical
    model, first, _ = gum
    branching, _, _, _ = lockstep_network('cuda:0')
    post = quiet(branching.posterior_results, 300, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=3)
    assert post.num_paths > 1
    with pytest.raises(NotImplementedError):
        post.reobserve(observe={'obs0': 7.0})
    with pytest.raises(ValueError, match='obs0'):
        first.reobserve(observe={'height': 1.0})
    with pytest.raises(NotImplementedError, match='Categorical'):
        first.reobserve(likelihood_funcs={'obs0': lambda v, trace: Categorical([0.5, 0.5])})
    with pytest.raises(AttributeError):
        Empirical(values=[1.0, 2.0], log_weights=[0.0, 0.0]).reobserve(observe={'obs0': 1.0})
    import pyprob_amd as pyprob
    from pyprob_amd.distributions import Normal

    def other(self):
        z = pyprob.sample(Normal(0.0, 1.0), address='z')
        pyprob.observe(Normal(z, 1.0), name='obs0')
        return z
    with monkeypatch.context() as m:
        m.setattr(GaussianWithUnknownMean, 'forward', other)
        with pytest.raises(RuntimeError, match='statement log'):
            first.reobserve(observe={'obs0': 1.0})
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    with pytest.raises(ValueError, match='PP_EMPIRICAL_DEVICE'):
        first.reobserve(observe={'obs0': 1.0})
