"""The fused posterior pass (pp_is_step_net + pp_is_fused: draw, - log q, + log p, the observe terms that follow and the
importance statistics in ONE pass over the particles, state.LockStepState.flush) against the one-kernel-per-term path
(PP_IS_FUSED=0) through the drop-in API Model.posterior_results: same Philox stream -> bit-identical values, equal
log-weights and statistics; host-side Empirical reductions equal the device statistics."""
import math

import numpy as np
import pytest

from models import GaussianWithUnknownMean, GaussianWithUnknownMeanMarsagliaLockStep
from oracle import ic_oracle as O
from pyprob_amd.state import InferenceEngine, InferenceNetwork

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
OBS = {'obs0': 8, 'obs1': 9}
EMB = {'obs0': {'dim': 32}, 'obs1': {'dim': 32}}


@pytest.fixture(scope='module')
def gum():
    torch.manual_seed(3)
    model = GaussianWithUnknownMean()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=20000, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, seed=1)
    return model


@pytest.fixture(scope='module')
def gumm():
    torch.manual_seed(4)
    model = GaussianWithUnknownMeanMarsagliaLockStep()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=20000, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, seed=2)
    return model


@pytest.fixture(scope='module', params=[1, 16], ids=['k1', 'k16'])
def gum_k(request):
    """A fresh GUM network with one or sixteen mixture components: pp_is_fused draws through is_fused_kernel with a run-time
    K (only K = 10 has its own instantiation)."""
    torch.manual_seed(6)
    model = GaussianWithUnknownMean()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=4096, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, proposal_mixture_components=request.param, seed=7)
    assert model._inference_network._engine.spec.K == request.param
    return model


def _both(model, n, monkeypatch, observe, seed):
    monkeypatch.setenv('PP_IS_FUSED', '1')
    fused = model.posterior_results(n, IC, observe=observe, lock_step=True, seed=seed)
    monkeypatch.setenv('PP_IS_FUSED', '0')
    eager = model.posterior_results(n, IC, observe=observe, lock_step=True, seed=seed)
    return fused, eager


def _fused_equals_the_per_term_kernels(model, monkeypatch, n):
    fused, eager = _both(model, n, monkeypatch, OBS, seed=11)
    vf, ve = fused._all_values.cpu().numpy(), eager._all_values.cpu().numpy()
    assert np.array_equal(vf, ve)                              # the same Philox stream, the same draw arithmetic
    lf, le = fused._all_log_weights.cpu().numpy(), eager._all_log_weights.cpu().numpy()
    np.testing.assert_allclose(lf, le, rtol=1e-5, atol=1e-5)
    for k in ('mean', 'var', 'ess', 'max_lw', 'count'):
        assert abs(fused.device_stats[k] - eager.device_stats[k]) <= 1e-6 * max(1.0, abs(eager.device_stats[k])), k
    assert fused.length == n and int(fused.device_stats['count']) == n
    # the device statistics are what the reference's Empirical computes on the host in float64
    mean_dev, ess_dev, std_dev = fused.mean, fused.effective_sample_size, fused.stddev
    w = fused.weights_numpy()                                  # materialises the host-side weights
    v = fused.values_numpy()
    assert abs(float(np.sum(w * v)) - mean_dev) < 1e-6 * max(1.0, abs(mean_dev))
    assert abs(1.0 / float(np.sum(w * w)) - ess_dev) < 1e-6 * ess_dev
    assert abs(fused.mean - mean_dev) < 1e-6 and abs(fused.stddev - std_dev) < 1e-6
    return fused


@pytest.mark.parametrize('n', [1000, 65537, 1000000])
def test_fused_pass_equals_the_per_term_kernels(gum, monkeypatch, n):
    fused = _fused_equals_the_per_term_kernels(gum, monkeypatch, n)
    assert abs(fused.mean - 7.25) < 0.75


@pytest.mark.parametrize('n', [1000, 65537])
def test_fused_pass_at_other_mixture_sizes(gum_k, monkeypatch, n):
    """K = 1 and K = 16: the fused pass equals the per-term kernels, and every particle's log-weight equals the float64
    oracle's re-scoring at that K (log p - log q of the drawn mu + both Normal observe terms)."""
    fused = _fused_equals_the_per_term_kernels(gum_k, monkeypatch, n)
    eng = gum_k._inference_network._engine
    params = {k: v.numpy() for k, v in eng.state_dict().items()}
    net = O.Net(params, ['obs0', 'obs1'], K=eng.spec.K)
    v = fused._all_values.cpu().numpy().astype(np.float64)
    lw = fused._all_log_weights.cpu().numpy().astype(np.float64)
    steps = [dict(address=eng.spec.addresses[0].address, dist_name='Normal', values=v, prior=np.array([[1.0, math.sqrt(5)]]))]
    _, lw_ref = O.is_rescore_lockstep(net, [float(OBS['obs0']), float(OBS['obs1'])], steps, n, chunk=1 << 18)
    lw_ref = lw_ref + sum(np.asarray(O.normal_log_prob(float(y), v, math.sqrt(2)), np.float32).astype(np.float64)
                          for y in OBS.values())
    assert np.isfinite(lw_ref).all()
    err = np.abs(lw - lw_ref) / np.maximum(1.0, np.abs(lw_ref))
    assert err.max() < 1e-4, (err.max(), int(err.argmax()))


def test_fused_pass_in_a_program_with_control_flow(gumm, monkeypatch):
    """First statement deferred (Uniform prior -> TruncatedNormal mixture), flushed by the second statement; the diverging
    paths take the per-term kernels; the observe terms of every path are queued and flushed once per path."""
    obs = {'obs0': 4, 'obs1': 5}
    fused, eager = _both(gumm, 20000, monkeypatch, obs, seed=5)
    assert np.array_equal(fused._all_values.cpu().numpy(), eager._all_values.cpu().numpy())
    np.testing.assert_allclose(fused._all_log_weights.cpu().numpy(), eager._all_log_weights.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert fused.num_paths == eager.num_paths > 1
    assert abs(fused.device_stats['ess'] - eager.device_stats['ess']) <= 1e-5 * eager.device_stats['ess']


class GumShifted(GaussianWithUnknownMean):
    """The same program, but it LOOKS at the sampled value (arithmetic on it) before the observes."""

    def forward(self):
        import pyprob_amd as pyprob
        from pyprob_amd.distributions import Normal
        mu = pyprob.sample(Normal(self.prior_mean, self.prior_stddev))
        centre = mu * 1.0 + 0.0                                # reads the value: a deferred draw has to run here
        likelihood = Normal(centre, self.likelihood_stddev)
        pyprob.observe(likelihood, name='obs0')
        pyprob.observe(likelihood, name='obs1')
        return mu


def test_reading_a_deferred_value_materialises_it(monkeypatch):
    torch.manual_seed(5)
    model = GumShifted()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=8000, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, seed=3)
    fused, eager = _both(model, 30000, monkeypatch, OBS, seed=9)
    assert np.array_equal(fused._all_values.cpu().numpy(), eager._all_values.cpu().numpy())
    np.testing.assert_allclose(fused._all_log_weights.cpu().numpy(), eager._all_log_weights.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert np.all(np.isfinite(fused._all_log_weights.cpu().numpy()))


class BranchOnFirstDraw(GaussianWithUnknownMean):
    """`if k:` on the FIRST statement's value - ParticleTensor.__bool__ straight on a deferred draw: the draw has to
    be flushed before the branch reads it, otherwise the particles split on uninitialised memory."""

    def forward(self):
        import pyprob_amd as pyprob
        from pyprob_amd.distributions import Normal, Poisson
        k = pyprob.sample(Poisson(1.2))
        if k:
            mu = pyprob.sample(Normal(2.0, 1.0))
        else:
            mu = pyprob.sample(Normal(-2.0, 1.0))
        likelihood = Normal(mu, self.likelihood_stddev)
        pyprob.observe(likelihood, name='obs0')
        pyprob.observe(likelihood, name='obs1')
        return mu


def test_branching_on_a_deferred_first_draw(monkeypatch):
    """The Poisson head proposes continuous positive values (a TruncatedNormal mixture on [0, 40]), so `if k:` is True for every
    particle - provided the branch reads the DRAWN values. The deferred draw's storage comes from torch.empty: the caching
    allocator is primed with zeros of that size, so an unflushed read sees k = 0 everywhere and takes the other branch."""
    torch.manual_seed(6)
    model = BranchOnFirstDraw()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=8000, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, seed=4)
    obs = {'obs0': 1.0, 'obs1': 1.5}
    n = 20000
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv('PP_IS_FUSED', flag)
        for _ in range(4):
            z = [torch.zeros(n, device='cuda:0') for _ in range(8)]      # freed blocks of exactly the size torch.empty(n) asks for
            del z
        outs.append(model.posterior_results(n, IC, observe=obs, lock_step=True, seed=13))
    fused, eager = outs
    assert fused.num_paths == eager.num_paths == 1
    (af, (vf, _)), = fused.statement_log[0].items()
    (ae, (ve, _)), = eager.statement_log[0].items()
    assert af == ae and torch.equal(vf, ve) and bool((vf > 0).all())
    assert len(fused.statement_log[1]) == 1 and list(fused.statement_log[1]) == list(eager.statement_log[1])    # the `if` branch
    assert np.array_equal(fused._all_values.cpu().numpy(), eager._all_values.cpu().numpy())
    np.testing.assert_allclose(fused._all_log_weights.cpu().numpy(), eager._all_log_weights.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert fused._all_values.mean() > 0          # proposals of Normal(2, 1), not of Normal(-2, 1)


# ---- launch plan of a static program (Model._traces_lockstep) --------------------------------------------------------------
def _same(a, b):
    return (torch.equal(a._all_values, b._all_values) and torch.equal(a._all_log_weights, b._all_log_weights) and
            a.mean == b.mean and a.effective_sample_size == b.effective_sample_size)


def test_launch_plan_replay_equals_running_the_program(gum, monkeypatch):
    """A call that was one deferred draw + one fused pass is replayed without running forward(): bit-identical values,
    log-weights and statistics; replayed for OTHER observation values only after a second recording showed that the
    program's constants do not depend on them; a changed model attribute asks for a new recording."""
    monkeypatch.setenv('PP_IS_FUSED', '1')
    monkeypatch.setenv('PP_IS_PLAN', '1')
    gum.__dict__.pop('_lockstep_plans', None)
    n = 50000
    a = gum.posterior_results(n, IC, observe=OBS, lock_step=True, seed=3)
    assert not getattr(a, 'replayed_plan', False)
    b = gum.posterior_results(n, IC, observe=OBS, lock_step=True, seed=3)               # same observation: replayed
    assert getattr(b, 'replayed_plan', False) and _same(a, b)
    other = {'obs0': 6.5, 'obs1': 7.25}
    c = gum.posterior_results(n, IC, observe=other, lock_step=True, seed=4)             # unverified plan: the program runs
    assert not getattr(c, 'replayed_plan', False)
    third = {'obs0': 5.0, 'obs1': 5.5}
    d = gum.posterior_results(n, IC, observe=third, lock_step=True, seed=9)             # verified now: replayed with new values
    assert getattr(d, 'replayed_plan', False)
    monkeypatch.setenv('PP_IS_PLAN', '0')
    e = gum.posterior_results(n, IC, observe=third, lock_step=True, seed=9)
    assert not getattr(e, 'replayed_plan', False) and _same(d, e)
    assert abs(d.mean - 4.7) < 0.6                                                       # posterior of (5.0, 5.5): 4.72
    monkeypatch.setenv('PP_IS_PLAN', '1')
    old = gum.likelihood_stddev
    try:
        gum.likelihood_stddev = 1.0                                                      # the recorded constants are stale
        f = gum.posterior_results(n, IC, observe=third, lock_step=True, seed=9)
        assert not getattr(f, 'replayed_plan', False) and not torch.equal(f._all_log_weights, d._all_log_weights)
    finally:
        gum.likelihood_stddev = old


def test_first_statement_in_two_launches_equals_the_separate_calls(gum, monkeypatch):
    """pp_is_first_statement (observe embedding inside the one-row LSTM launch, observation read from pinned host memory,
    statistics polled in pinned host memory) against pp_is_init + pp_is_step_net behind a staged copy (PP_IS_FIRST=0): the
    same embedding, state and proposal bit for bit -> identical particles, log-weights and statistics; three observations."""
    monkeypatch.setenv('PP_IS_FUSED', '1')
    monkeypatch.setenv('PP_IS_PLAN', '1')
    n = 100000
    obs3 = ({'obs0': 8.0, 'obs1': 9.0}, {'obs0': 6.5, 'obs1': 7.25}, {'obs0': -1.0, 'obs1': 0.5})
    outs = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('PP_IS_FIRST', flag)
        gum.__dict__.pop('_lockstep_plans', None)
        res = []
        for rep in range(2):                      # first round records and verifies the plan, second round replays it
            for k, o in enumerate(obs3):
                res.append(gum.posterior_results(n, IC, observe=o, lock_step=True, seed=50 + k))
        assert all(getattr(r, 'replayed_plan', False) for r in res[3:])
        outs[flag] = res
    for a, b in zip(outs['1'], outs['0']):
        assert _same(a, b)
    for r, o in zip(outs['1'][3:], obs3):          # and a replay equals the recorded run of the same observation and seed
        assert abs(r.mean - (1.0 / 5 + (o['obs0'] + o['obs1']) / 2) / (1.0 / 5 + 1.0)) < 1.0      # posterior mean of the conjugate model


@pytest.mark.parametrize('program', ['gum', 'gumm'])
def test_embedding_inside_the_first_statement_without_a_plan(gum, gumm, monkeypatch, program):
    """forward() in every call (PP_IS_PLAN=0 - what runs with pyprob as the host): `ISRunner.init` only stages the observation and
    the first statement issues pp_is_first_statement (embedding + LSTM row + proposal layer in one launch) - against the
    separate pp_is_init launch (PP_IS_LAZY_INIT=0): identical particles, log-weights and statistics, also for a program with
    control flow (whose later statements read the embedding the fused launch left on the device)."""
    monkeypatch.setenv('PP_IS_FUSED', '1')
    monkeypatch.setenv('PP_IS_PLAN', '0')
    model = gum if program == 'gum' else gumm
    obs3 = ({'obs0': 8.0, 'obs1': 9.0}, {'obs0': 6.5, 'obs1': 7.25}, {'obs0': 4.0, 'obs1': 5.0})
    outs = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('PP_IS_LAZY_INIT', flag)
        outs[flag] = [model.posterior_results(30000, IC, observe=o, lock_step=True, seed=70 + k) for k, o in enumerate(obs3)]
        assert not any(getattr(r, 'replayed_plan', False) for r in outs[flag])
    for a, b in zip(outs['1'], outs['0']):
        assert _same(a, b)


class PrivateScale(GaussianWithUnknownMean):
    """The likelihood's scale lives in a PRIVATE attribute (`self._sigma`) and a constant in a module global reached through
    a helper method: state a launch-plan key that only fingerprinted public attributes never saw."""

    def __init__(self):
        super().__init__()
        self._sigma = 1.2

    def likelihood(self, mu):
        from pyprob_amd.distributions import Normal
        return Normal(mu, self._sigma * PLAN_GLOBAL_FACTOR)

    def forward(self):
        import pyprob_amd as pyprob
        from pyprob_amd.distributions import Normal
        mu = pyprob.sample(Normal(self.prior_mean, self.prior_stddev))
        lik = self.likelihood(mu)
        pyprob.observe(lik, name='obs0')
        pyprob.observe(lik, name='obs1')
        return mu


PLAN_GLOBAL_FACTOR = 1.0


def test_launch_plan_sees_private_attributes_globals_and_callees(monkeypatch):
    import sys
    monkeypatch.setenv('PP_IS_FUSED', '1')
    torch.manual_seed(9)
    model = PrivateScale()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=4000, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, seed=7)
    n = 20000
    obs3 = ({'obs0': 8.0, 'obs1': 9.0}, {'obs0': 6.5, 'obs1': 7.25}, {'obs0': 5.0, 'obs1': 5.5})

    def both(obs, seed):
        monkeypatch.setenv('PP_IS_PLAN', '1')
        a = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=seed)
        monkeypatch.setenv('PP_IS_PLAN', '0')
        b = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=seed)
        assert _same(a, b)
        return bool(getattr(a, 'replayed_plan', False))
    assert [both(o, 30 + k) for k, o in enumerate(obs3)] == [False, False, True]       # recorded, verified, replayed
    model._sigma = 2.5                    # a private attribute forward()'s callee reads: the plan's constants are stale
    assert both(obs3[2], 41) is False     # ... so the program runs (and equals PP_IS_PLAN=0 with the NEW scale)
    assert both(obs3[0], 42) is False and both(obs3[1], 43) is True
    mod = sys.modules[__name__]
    monkeypatch.setattr(mod, 'PLAN_GLOBAL_FACTOR', 0.5)                                  # a module global the callee reads
    assert both(obs3[1], 44) is False
    monkeypatch.setattr(PrivateScale, 'likelihood', lambda self, mu: __import__('pyprob_amd').distributions.Normal(mu, 3.0))
    assert both(obs3[1], 45) is False                                                    # a re-bound callee is a new program


class ScaleFromObservation(GaussianWithUnknownMean):
    """The likelihood's scale is computed IN PYTHON from an observed value: a launch plan recorded for one observation holds
    a constant that is wrong for another one."""

    def forward(self):
        import pyprob_amd as pyprob
        from pyprob_amd.distributions import Normal
        mu = pyprob.sample(Normal(self.prior_mean, self.prior_stddev))
        y0 = pyprob.observe(Normal(mu, self.likelihood_stddev), name='obs0')
        pyprob.observe(Normal(mu, 1.0 + 0.1 * abs(float(y0))), name='obs1')
        return mu


def test_launch_plan_is_not_replayed_when_constants_follow_the_observation(monkeypatch):
    monkeypatch.setenv('PP_IS_FUSED', '1')
    torch.manual_seed(8)
    model = ScaleFromObservation()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=4000, observe_embeddings=EMB, batch_size=128,
                                  lstm_dim=64, seed=6)
    n = 20000
    runs = []
    for k, obs in enumerate(({'obs0': 8.0, 'obs1': 9.0}, {'obs0': 2.0, 'obs1': 3.0}, {'obs0': -4.0, 'obs1': -3.0}, {'obs0': 8.0, 'obs1': 9.0})):
        monkeypatch.setenv('PP_IS_PLAN', '1')
        with_plan = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=20 + k)
        monkeypatch.setenv('PP_IS_PLAN', '0')
        without = model.posterior_results(n, IC, observe=obs, lock_step=True, seed=20 + k)
        assert _same(with_plan, without), k
        runs.append(bool(getattr(with_plan, 'replayed_plan', False)))
    assert runs == [False, False, False, False]        # never verified: every new observation runs the program
    again = model.posterior_results(n, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=99)
    monkeypatch.setenv('PP_IS_PLAN', '1')
    again = model.posterior_results(n, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=99)
    assert getattr(again, 'replayed_plan', False)      # the SAME observation as the last recording: its constants are right


class MarsagliaInPlace(GaussianWithUnknownMeanMarsagliaLockStep):
    """The rejection loop with IN-PLACE arithmetic on intermediate results (`s += y * y`): a reused (memoised) result that the
    program then modifies must not be handed out again as the product it once was."""

    def marsaglia(self, mean, stddev):
        import pyprob_amd as pyprob
        from pyprob_amd.distributions import Uniform
        uniform = Uniform(-1, 1)
        s = 1
        while s >= 1:
            x = pyprob.sample(uniform)
            y = pyprob.sample(uniform)
            s = x * x
            s += y * y
        return mean + stddev * (x * torch.sqrt(-2 * torch.log(s) / s))


@pytest.mark.parametrize('program', ['plain', 'inplace'])
def test_reusing_pure_results_across_control_flow_paths_changes_nothing(gumm, monkeypatch, program):
    """ParticleTensor memoisation (state.py): every path re-runs forward(); the arithmetic of its replayed iterations is served
    from the results of earlier paths. Values, log-weights, paths and statistics equal a run that recomputes everything."""
    model = gumm
    if program == 'inplace':
        torch.manual_seed(4)
        model = MarsagliaInPlace()
        model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=20000, observe_embeddings=EMB, batch_size=128,
                                      lstm_dim=64, seed=2)
    obs = {'obs0': 4, 'obs1': 5}
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv('PP_IS_MEMO', flag)
        outs.append(model.posterior_results(30000, IC, observe=obs, lock_step=True, seed=21))
    a, b = outs
    assert a.num_paths == b.num_paths > 3
    assert torch.equal(a._all_values, b._all_values) and torch.equal(a._all_log_weights, b._all_log_weights)
    assert a.mean == b.mean and a.effective_sample_size == b.effective_sample_size
