"""Empirical.reobserve / reweight on the host: the numpy restatement of pp_is_reobserve_groups against hand-computed cases, the
replay executor end to end on the oracle-backed CPU stand-ins (tests/oracle_ops.py) with the CPU double of the new operator,
reweight against the reference's definition (and the live reference where it is installed next to the repository), and the
header <-> PROTOTYPES <-> export agreement of the new entry point. The device side is tests/test_gpu_reobserve*.py."""
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
import reobserve_ref as RR
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def normal_lp(x, mu, sd):
    return -((x - mu) ** 2) / (2.0 * sd * sd) - np.log(sd) - HALF_LOG_2PI


# ---- the entry point -----------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_prototyped_and_exported():
    """FAILS WITHOUT THE FEATURE: the parent has no such symbol."""
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    name = 'pp_is_reobserve_groups'
    assert name in declared and name in L.PROTOTYPES and hasattr(lib, name)
    decl = hdr[hdr.index('%s(' % name):]
    decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
    assert decl.count(',') + 1 == len(L.PROTOTYPES[name][1]) == 8
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15          # an addition only
    assert int(re.search(r'#define PP_REOBS_MAX_TERMS (\d+)', hdr).group(1)) == L.PP_REOBS_MAX_TERMS == 8
    import ctypes as C
    assert C.sizeof(L.pp_reobs_term) == 16 + 5 * C.sizeof(L.pp_obs_operand) == 136
    assert 'empirical.py:469-544' in hdr


def test_refusals_need_no_device():
    lib = L.load()
    arr = (L.pp_reobs_term * 1)()
    assert lib.pp_is_reobserve_groups(arr, 0, None, None, None, 1, 1, None) != 0
    assert b'pp_is_reobserve_groups' in lib.pp_last_error()
    assert lib.pp_is_reobserve_groups(arr, 1, None, None, None, 1, 1, None) != 0


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_composition_by_hand():
    f = np.float32
    lw = np.array([1.5, -np.inf, np.nan, 0.25], f)
    old = np.array([-2.0, -1.0, -1.0, 0.5], f)
    lp0 = np.array([[-1.0, -2.0, -3.0, -4.0], [0.0, 0.0, 0.0, -np.inf]], f)
    lp1 = np.array([[-0.5, -0.5, -0.5, -0.5], [1.0, 1.0, 1.0, 1.0]], f)
    out = RR.compose32(lw, old, [lp0, lp1], [0.5, 2.0])
    # s = 0.5 lp0 + 2 lp1; out = lw + (s - old); a dropped particle keeps its lw for every group
    assert out[0, 0] == f(1.5) + ((f(-0.5) + f(-1.0)) - f(-2.0)) == f(2.0)
    assert out[0, 3] == f(0.25) + ((f(-2.0) + f(-1.0)) - f(0.5)) == f(-3.25)
    assert out[1, 0] == f(1.5) + (f(2.0) - f(-2.0)) == f(5.5)
    assert np.isneginf(out[:, 1]).all() and np.isnan(out[:, 2]).all() and np.isneginf(out[1, 3])
    # the roundings: product first, then the sum (never one fused operation)
    a, s = f(1.0) + f(2.0 ** -23), f(1.0) - f(2.0 ** -24)
    got = RR.compose32(np.zeros(1, f), None, [np.array([[a]], f)], [s])[0, 0]
    assert got == f(a * s) and float(got) != float(a) * float(s)


def test_float64_restatement_and_the_cpu_double_by_hand():
    lw = torch.tensor([0.5, -1.0, 2.0])
    mu = torch.tensor([0.0, 1.0, -1.0])
    sd = torch.tensor([2.0])
    x = torch.tensor([[0.5], [3.0]])
    old = torch.from_numpy(normal_lp(1.0, mu.numpy().astype(np.float64), 2.0).astype(np.float32))
    ref = RR.reobserve64(lw.numpy(), old.numpy(), [(0, 1, 1.0, [mu.reshape(3, 1), sd, None, None], x)], 2)
    want = lw.numpy().astype(np.float64)[None, :] + normal_lp(x.numpy().astype(np.float64), mu.numpy()[None, :], 2.0) - \
        old.numpy().astype(np.float64)[None, :]
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-12)
    got = RR.reobserve_groups_cpu(lw, old, [0], [1], [1.0], [mu.reshape(3, 1), sd, None, None], [x], 2)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=1e-6)
    # a vector term: k = 3 values per observe, one row of means per particle
    means = torch.tensor([[0.0, 1.0, 2.0], [1.0, 1.0, 1.0], [-1.0, 0.0, 1.0]])
    xs = torch.tensor([[0.0, 1.0, 2.0]])
    got = RR.reobserve_groups_cpu(lw, None, [0], [3], [0.5], [means, sd, None, None], [xs], 1)
    want = lw.numpy() + 0.5 * normal_lp(xs.numpy().astype(np.float64), means.numpy(), 2.0).sum(1)
    np.testing.assert_allclose(got.numpy()[0], want, rtol=1e-6, atol=1e-6)


# ---- the replay executor, end to end ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def two_statements():
    """The two-statement program of tests/test_joint_moments_host.py on the oracle-backed CPU stand-ins: a = sample, observe obs0
    under Normal(a, sqrt 2), b = sample, observe obs1 under Normal(b, sqrt 2); one lock-step IC posterior of 300 particles."""
    from test_joint_moments_host import _two_statement_model
    RR.register_cpu()
    model = _two_statement_model()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(300, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
    return model, post


def columns(post):
    a = post.statement_log[0]['a__Normal__1'][0].numpy().astype(np.float64)
    b = post.statement_log[1]['b__Normal__1'][0].numpy().astype(np.float64)
    return a, b, post._all_log_weights.numpy().astype(np.float64)


def test_reobserve_of_one_name_against_float64(two_statements):
    """FAILS WITHOUT THE FEATURE (AttributeError: reobserve)."""
    model, post = two_statements
    a, b, lw = columns(post)
    new = post.reobserve(observe={'obs1': 3.25})
    assert new._values is post._values and new.length == post.length and new.statement_log is post.statement_log
    want = lw + normal_lp(3.25, b, math.sqrt(2.0)) - normal_lp(1.5, b, math.sqrt(2.0))
    np.testing.assert_allclose(new._all_log_weights.numpy(), want, rtol=0, atol=2e-5)
    assert new.metadata['op'] == 'reobserve' and new.metadata['observables'] == ['obs1']
    assert new._origin[3] == {'obs0': 2.0, 'obs1': 3.25} and new._origin[0] is model
    # the statement log answers under the new weights
    w = np.exp(want - want.max())
    assert abs(new.marginal('mu').mean - float((w * a).sum() / w.sum())) < 1e-4
    assert abs(new.mean - float((w * b).sum() / w.sum())) < 1e-4
    # re-observing the original values at the original scale returns the call's log-weights bit for bit
    same = post.reobserve(observe={'obs0': 2.0, 'obs1': 1.5})
    assert np.array_equal(same._all_log_weights.numpy(), post._all_log_weights.numpy())
    # and the result can be re-observed again: back to the first observation
    back = new.reobserve(observe={'obs1': 1.5})
    np.testing.assert_allclose(back._all_log_weights.numpy(), lw, rtol=0, atol=4e-5)


def test_likelihood_funcs_and_importance_against_float64(two_statements):
    from pyprob_amd.distributions import Normal
    model, post = two_statements
    a, b, lw = columns(post)
    seen = []

    def wider(v, trace):
        seen.append((v.name, v.address, float(v.value), v.observed, trace))
        return Normal(v.distribution.mean, 2.0 * v.distribution.stddev)
    new = post.reobserve(likelihood_funcs={'obs0': wider})
    assert len(seen) == 1 and seen[0][0] == 'obs0' and seen[0][2:] == (2.0, True, None) and 'Normal' in seen[0][1]
    want = lw + normal_lp(2.0, a, 2.0 * math.sqrt(2.0)) - normal_lp(2.0, a, math.sqrt(2.0))
    np.testing.assert_allclose(new._all_log_weights.numpy(), want, rtol=0, atol=2e-5)
    half = post.reobserve(observe={'obs0': 1.0, 'obs1': 1.0}, likelihood_importance=0.5)
    want = lw + 0.5 * (normal_lp(1.0, a, math.sqrt(2.0)) + normal_lp(1.0, b, math.sqrt(2.0))) - \
        (normal_lp(2.0, a, math.sqrt(2.0)) + normal_lp(1.5, b, math.sqrt(2.0)))
    np.testing.assert_allclose(half._all_log_weights.numpy(), want, rtol=0, atol=4e-5)
    assert half._origin[4] == 0.5
    # one name at another scale: terms at two scales, the result cannot be re-observed again
    mixed = post.reobserve(observe={'obs0': 1.0}, likelihood_importance=0.5)
    with pytest.raises(ValueError, match='likelihood_importance'):
        mixed.reobserve(observe={'obs0': 2.0})


def test_reobserve_batch_members_equal_the_single_calls(two_statements):
    import pyprob_amd
    model, post = two_statements
    observes = [{'obs0': 2.0, 'obs1': 1.5}, {'obs0': 0.5, 'obs1': 2.5}, {'obs0': 3.0, 'obs1': -1.0}]
    members = pyprob_amd.reobserve_batch(post, observes)
    assert len(members) == 3
    for g, m in enumerate(members):
        one = post.reobserve(observe=observes[g])
        assert np.array_equal(m._all_log_weights.numpy(), one._all_log_weights.numpy()), g
        assert m._values is post._values and m.mean == one.mean and m.effective_sample_size == one.effective_sample_size
        assert m._batch[3] == g and m._batch[0].numel() == 3 * 300 and m._origin[3] == observes[g]
    as_dict = pyprob_amd.reobserve_batch(post, {'obs1': torch.tensor([1.5, 2.5, -1.0])})
    assert np.array_equal(as_dict[0]._all_log_weights.numpy(), post._all_log_weights.numpy())
    # joint_batch takes its loop: every member's joint from the shared [N] columns
    from test_joint_moments_host import _register_cpu_double
    _register_cpu_double()
    joints = pyprob_amd.joint_batch(members)
    assert np.array_equal(joints[1].mean, members[1].joint().mean)


def test_errors(two_statements, monkeypatch):
    from pyprob_amd.distributions import Categorical, Empirical
    model, post = two_statements
    with pytest.raises(ValueError, match='obs0'):
        post.reobserve(observe={'nothing': 1.0})
    with pytest.raises(ValueError):
        post.reobserve()
    with pytest.raises(NotImplementedError, match='Categorical'):
        post.reobserve(likelihood_funcs={'obs0': lambda v, trace: Categorical([0.5, 0.5])})
    with pytest.raises(AttributeError):
        Empirical(values=[1.0, 2.0], log_weights=[0.0, 0.0]).reobserve(observe={'obs0': 1.0})
    # a program that no longer matches the log
    forward = type(model).forward

    def other(self):
        import pyprob_amd as pyprob
        from pyprob_amd.distributions import Normal
        c = pyprob.sample(Normal(0.0, 1.0), address='c')
        pyprob.observe(Normal(c, 1.0), name='obs0')
        return c
    monkeypatch.setattr(type(model), 'forward', other)
    with pytest.raises(RuntimeError, match='statement log'):
        post.reobserve(observe={'obs0': 1.0})
    monkeypatch.setattr(type(model), 'forward', forward)
    branched = post.reobserve(observe={'obs0': 2.0})
    branched.num_paths = 3
    with pytest.raises(NotImplementedError, match='straight-line'):
        branched.reobserve(observe={'obs0': 1.0})
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    with pytest.raises(ValueError, match='PP_EMPIRICAL_DEVICE'):
        post.reobserve(observe={'obs0': 1.0})


# ---- the statement runtime next to the replay branch --------------------------------------------------------------------------------
def test_observed_name_sample_under_coroutines_keeps_its_likelihood():
    """`sample(..., name=<an observed name>)` in a coroutine run (posterior_results(lock_step=False)) is an observe: its
    likelihood joins the device accumulator that becomes every trace's log-weight. The program's addresses are unknown to the
    golden network, so the prior is the proposal and a particle's log-weight is its likelihood alone."""
    pytest.importorskip('greenlet')
    import pyprob_amd as pyprob
    from is_helpers import network_from_golden
    from models import GaussianWithUnknownMean
    from pyprob_amd.distributions import Normal
    net, meta, params, isr = network_from_golden('gum')

    class ObservedSample(GaussianWithUnknownMean):
        def forward(self):
            z = pyprob.sample(Normal(0., 1.))
            mu = pyprob.sample(Normal(self.prior_mean, self.prior_stddev))
            pyprob.observe(Normal(mu + 0 * z, self.likelihood_stddev), name='obs0')
            pyprob.sample(Normal(mu, self.likelihood_stddev), name='obs1')
            return mu
    model = ObservedSample()
    model._inference_network = net
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model._traces_coroutines(6, {'obs0': 8.0, 'obs1': 9.0}, map_func=lambda t: t)
    assert post.length == 6
    for tr in post.get_values():
        mu = float(tr.result)
        ref = float(normal_lp(8.0, mu, math.sqrt(2.0)) + normal_lp(9.0, mu, math.sqrt(2.0)))
        assert abs(tr.log_importance_weight - ref) < 1e-5


# ---- reweight ----------------------------------------------------------------------------------------------------------------------
def test_reweight_is_the_references_definition():
    from pyprob_amd.distributions import Empirical
    emp = Empirical(values=[0.5, 1.5, 2.5, 3.5], log_weights=[0.0, -1.0, -2.0, -3.0])
    calls = []

    def func(v):
        calls.append(v)
        return -0.5 * v * v
    new = emp.reweight(func)
    assert calls == [0.5, 1.5, 2.5, 3.5] and new.length == 4 and new.metadata['op'] == 'reweight'
    lw = np.array([-0.5 * v * v for v in calls])
    w = np.exp(lw - lw.max())
    assert abs(new.mean - float((w * np.array(calls)).sum() / w.sum())) < 1e-12
    part = emp.reweight(func, min_index=1, max_index=3)
    assert part.length == 2 and list(part.get_values()) == [1.5, 2.5]
    assert Empirical().reweight(func).length == 0


@pytest.mark.skipif(not os.path.isdir('/root/reference/pyprob'), reason='the live reference is not installed next to the repository')
def test_reweight_against_the_live_reference():
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(0, '/root/reference')
    try:
        import pyprob.distributions as ref      # (the directory is there: an import that fails is an error, not a skip)
    finally:
        sys.path.remove('/root/reference')
        sys.path.remove(os.path.join(REPO, 'oracle', 'refstubs'))
    from pyprob_amd.distributions import Empirical
    values, lws = [0.5, 1.5, 2.5, 3.5], [0.0, -1.0, -2.0, -3.0]
    func = lambda v: -0.5 * float(v) * float(v) + 0.25 * float(v)  # noqa: E731
    theirs = ref.Empirical(values=[torch.tensor(v) for v in values], log_weights=lws).reweight(func)
    ours = Empirical(values=values, log_weights=lws).reweight(func)
    assert abs(float(theirs.mean) - ours.mean) < 1e-6 and abs(float(theirs.effective_sample_size) - ours.effective_sample_size) < 1e-6
