"""Batched posteriors on the device (csrc/is_batch.hip; ISRunner.init_batch / first_batch / fused_groups;
Model.posterior_results_batch):
 1. pp_is_fused_groups indexes particles, groups, operands and Philox counters exactly: group g of an M-group call is bit-equal
    (values, log-weights, statistics row) to the one-group call on row g at offset + g N, and two identical calls are bit-equal;
 2. its log-weights against a float64 restatement of log q + the term (1e-4, the project's bar) and its statistics rows against
    float64 numpy over the returned particles (1e-10: N 2^-53 with N <= 10^4 plus a one-ulp fp64 exp);
 3. its draws as a distribution (Kolmogorov distance to the oracle's mixture CDF, the 1.95 / sqrt(n) bar of
    tests/test_gpu_is_step_fused.py);
 4. end to end on the golden networks: every particle of every group re-scored by the oracle with ITS group's observation;
 5. a program outside the fast path returns, bit for bit, what the loop of single calls returns.
Batched and single-call particles are not compared value by value: the M-row head outputs may differ from the one-row
kernel's in the last bits, and a uniform next to a component boundary then selects another component."""
import math
import warnings

import numpy as np
import pytest

import mixture_cases as MC
from helpers import is_engine
from is_helpers import lockstep_network, network_from_golden
from oracle import ic_oracle as O
from pyprob_amd.state import InferenceEngine, InferenceNetwork

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK

H = 64
SIGMA = 1.3
HEADS = {'a_normal': ('Normal', (1.0, math.sqrt(5.0))), 'a_uniform': ('Uniform', (5.0, 9.0))}
HEAD_CASES = [('a_normal', 1), ('a_normal', 10), ('a_normal', 16), ('a_uniform', 10)]
SHAPES = [(1, 1), (3, 1), (5, 63), (5, 64), (5, 65), (7, 1000), (257, 5), (2, 4097)]
_ENGINES = {}


def _eng(K):
    if K not in _ENGINES:
        _ENGINES[K] = is_engine(H, seed=3, K=K)
    return _ENGINES[K]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _inputs(address, K, M, rng):
    """Random head outputs y [M, ldy] (means | scales | logits, the padding columns poisoned) and one observation per group."""
    ldy = (3 * K + 3) & ~3
    y = np.full((M, ldy), np.nan, np.float32)
    y[:, :K] = rng.uniform(-1.0, 1.0, (M, K))
    y[:, K:2 * K] = rng.uniform(-2.0, 0.0, (M, K)) if address == 'a_normal' else rng.uniform(-6.0, -3.0, (M, K))
    y[:, 2 * K:3 * K] = rng.uniform(-1.5, 1.5, (M, K))
    lo, hi = (-4.0, 6.0) if address == 'a_normal' else (5.0, 9.0)
    return y, rng.uniform(lo, hi, M).astype(np.float32)


def _call(run, eng, address, y, x, n_per, seed, offset, stats=True):
    """One pp_is_fused_groups call: draw at `address`, one Normal(value, SIGMA) likelihood of the group's observation."""
    M = y.shape[0]
    dev = run.dev
    prior = torch.tensor(HEADS[address][1], dtype=torch.float32, device=dev)
    ty, tx = torch.from_numpy(y).to(dev), torch.from_numpy(x).to(dev)
    sigma = torch.tensor([SIGMA], dtype=torch.float32, device=dev)
    value = torch.full((M * n_per,), float('nan'), device=dev)
    lw = torch.full((M * n_per,), float('nan'), device=dev)
    terms = [((0, None, 0, sigma, 0), tx, 2, 1.0, 1)]       # p0 = the particle's value, x = per group
    st = run.fused_groups(eng.spec.address_id[address], n_per, prior, terms, value, lw, True, seed=seed, offset=offset, stats=stats, y=ty)
    return value, lw, st


# ---- 1. indexing, exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', SHAPES)
@pytest.mark.parametrize('address,K', HEAD_CASES, ids=['%s-K%d' % c for c in HEAD_CASES])
def test_group_of_a_batched_call_is_the_one_group_call(address, K, M, N):
    eng, run, sd = _eng(K)
    rng = np.random.default_rng(1000 * K + 10 * M + N)
    y, x = _inputs(address, K, M, rng)
    seed, offset = 31 + K, 5 * 4096 + 3
    value, lw, st = _call(run, eng, address, y, x, N, seed, offset)
    value2, lw2, st2 = _call(run, eng, address, y, x, N, seed, offset)
    singles = [_call(run, eng, address, y[g:g + 1], x[g:g + 1], N, seed, offset + g * N) for g in range(M)]
    v1 = torch.cat([s[0] for s in singles]).cpu().numpy()
    l1 = torch.cat([s[1] for s in singles]).cpu().numpy()
    s1 = torch.cat([s[2] for s in singles]).cpu().numpy()
    v, l, s = value.cpu().numpy(), lw.cpu().numpy(), st.cpu().numpy()
    assert s.shape == (M, 6) and np.isfinite(v).all() and np.isfinite(l).all()
    assert np.array_equal(_bits(v), _bits(value2.cpu().numpy())) and np.array_equal(_bits(l), _bits(lw2.cpu().numpy()))
    assert np.array_equal(_bits(s), _bits(st2.cpu().numpy()))
    assert np.array_equal(_bits(v), _bits(v1)), int(np.argmax(_bits(v) != _bits(v1)))
    assert np.array_equal(_bits(l), _bits(l1)), int(np.argmax(_bits(l) != _bits(l1)))
    assert np.array_equal(_bits(s), _bits(s1))
    assert (s[:, 5] == N).all()


# ---- 2. values --------------------------------------------------------------------------------------------------------------------
def _log_q64(address, K, y, values, n_per):
    """float64 log q of every particle under ITS group's head outputs."""
    dist, prior = HEADS[address]
    yy = np.repeat(y[:, :3 * K].astype(np.float64), n_per, axis=0)
    pr = np.tile(np.array([prior], np.float64), (len(values), 1))
    fn = O.head_normal_mixture if dist == 'Normal' else O.head_truncated_normal_mixture
    lq, _, params = fn(yy, pr, values.astype(np.float64), K)
    return lq, params


def _stats64(lw, x):
    lw, x = lw.astype(np.float64), x.astype(np.float64)
    ok = np.isfinite(lw)
    m = lw[ok].max()
    w = np.exp(lw[ok] - m)
    return m, w.sum(), (w * w).sum(), (w * x[ok]).sum(), (w * x[ok] * x[ok]).sum(), float(ok.sum()), (w * np.abs(x[ok])).sum()


@pytest.mark.parametrize('M,N', [(5, 65), (7, 1000), (2, 4097), (3, 10000)])
@pytest.mark.parametrize('address,K', HEAD_CASES, ids=['%s-K%d' % c for c in HEAD_CASES])
def test_log_weights_and_statistics_against_float64(address, K, M, N):
    eng, run, sd = _eng(K)
    rng = np.random.default_rng(77 * K + M + N)
    y, x = _inputs(address, K, M, rng)
    value, lw, st = _call(run, eng, address, y, x, N, 9, 12345)
    v, l, s = value.cpu().numpy(), lw.cpu().numpy(), st.cpu().numpy()
    lq, _ = _log_q64(address, K, y, v, N)
    vv = v.astype(np.float64)
    ref = -lq + O.normal_log_prob(np.repeat(x.astype(np.float64), N), vv, float(np.float32(SIGMA)))
    assert np.isfinite(ref).all()
    err = np.abs(l.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    print('lw: max relative error %.3g' % err.max())
    assert err.max() < 1e-4, (float(err.max()), int(err.argmax()))
    for g in range(M):
        m, sw, sw2, swx, swx2, cnt, swax = _stats64(l[g * N:(g + 1) * N], v[g * N:(g + 1) * N])
        assert s[g, 0] == m and s[g, 5] == cnt == N
        assert abs(s[g, 1] - sw) <= 1e-10 * sw and abs(s[g, 2] - sw2) <= 1e-10 * sw2, (g, s[g], sw, sw2)
        assert abs(s[g, 3] - swx) <= 1e-10 * swax and abs(s[g, 4] - swx2) <= 1e-10 * swx2, (g, s[g], swx, swx2)


def test_statistics_of_many_slices_and_non_finite_weights():
    """A group larger than one statistics slice (the partial records and their combine), and weights that are not finite: values
    given (no draw), the log-weights chosen through an identity term."""
    eng, run, sd = _eng(10)
    M, N = 2, 3 * 65536 + 17
    rng = np.random.default_rng(5)
    lw_in = (3.0 * rng.standard_normal(M * N) - 40.0).astype(np.float32)
    lw_in[::1000] = -np.inf
    lw_in[[3, N + 5]] = np.nan
    lw_in[N:N + 65536] = -np.inf           # a whole slice of group 1 without a finite weight
    x = rng.uniform(5.0, 9.0, M * N).astype(np.float32)
    tv, tl = torch.from_numpy(x).to(run.dev), torch.from_numpy(lw_in).to(run.dev)
    lw = torch.zeros(M * N, device=run.dev)
    st = run.fused_groups(None, N, None, [((2, None, 0, None, 0), tl, 1, 1.0, 0)], tv, lw, True, stats=True)
    st2 = run.fused_groups(None, N, None, [((2, None, 0, None, 0), tl, 1, 1.0, 0)], tv, lw, True, stats=True)
    assert np.array_equal(lw.cpu().numpy(), lw_in, equal_nan=True)
    s = st.cpu().numpy()
    assert np.array_equal(_bits(s), _bits(st2.cpu().numpy()))
    for g in range(M):
        m, sw, sw2, swx, swx2, cnt, swax = _stats64(lw_in[g * N:(g + 1) * N], x[g * N:(g + 1) * N])
        assert s[g, 0] == m and s[g, 5] == cnt
        # (N = 2e5: the derived bound N 2^-53 is 2.2e-11)
        assert abs(s[g, 1] - sw) <= 1e-10 * sw and abs(s[g, 2] - sw2) <= 1e-10 * sw2
        assert abs(s[g, 3] - swx) <= 1e-10 * swax and abs(s[g, 4] - swx2) <= 1e-10 * swx2
    # no finite weight at all: max = -inf, zero sums, zero count
    none = torch.full((8,), float('-inf'), device=run.dev)
    st = run.fused_groups(None, 4, None, [((2, None, 0, None, 0), none, 1, 1.0, 0)], tv[:8].contiguous(), torch.zeros(8, device=run.dev),
                          True, stats=True).cpu().numpy()
    assert (st[:, 0] == -np.inf).all() and (st[:, 1:] == 0).all()


def test_operand_codes_and_argument_checks():
    """Shared / per-particle / per-group operands of every slot against float64, and the rejected calls."""
    eng, run, sd = _eng(10)
    M, N = 4, 37
    n = M * N
    rng = np.random.default_rng(8)
    dev = run.dev
    value = rng.uniform(5.0, 9.0, n).astype(np.float32)
    mean_g, sd_p, x_g = rng.uniform(5, 9, M).astype(np.float32), rng.uniform(1, 3, n).astype(np.float32), rng.uniform(5, 9, M).astype(np.float32)
    rate_g = rng.uniform(3, 9, M).astype(np.float32)
    probs_g = rng.uniform(0.1, 1.0, (M, 12)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    tv = t(value)
    terms = [((0, t(mean_g), 2, t(sd_p), 1), t(x_g), 2, 1.0, 0),                       # Normal(mean_g, sd_i) at x_g
             ((3, t(rate_g), 2, None, 0), None, 0, 0.5, 4),                            # Poisson(rate_g) at the value
             ((5, t(probs_g), 2, None, 12), None, 0, 1.0, 4),                          # Categorical(row g) at the value
             ((1, t(np.array([2.0], np.float32)), 0, None, 0), t(x_g), 2, -1.0, 2)]    # Uniform(2, value) at x_g
    lw = torch.zeros(n, device=dev)
    run.fused_groups(None, N, None, terms, tv, lw, True)
    g = np.repeat(np.arange(M), N)
    v64 = value.astype(np.float64)
    ref = O.normal_log_prob(x_g[g].astype(np.float64), mean_g[g].astype(np.float64), sd_p.astype(np.float64))
    ref = ref + 0.5 * (v64 * np.log(rate_g[g].astype(np.float64)) - rate_g[g] - np.vectorize(math.lgamma)(v64 + 1.0))
    pg = probs_g[g].astype(np.float64)
    ref = ref + np.log(pg[np.arange(n), value.astype(np.int64)] / pg.sum(1))
    inside = (x_g[g] >= 2.0) & (x_g[g] < value)
    with np.errstate(divide='ignore'):
        ref = ref - np.where(inside, -np.log(v64 - 2.0), -np.inf)
    got = lw.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and np.isfinite(ref).any() and not np.isfinite(ref).all()
    ok = np.isfinite(ref)
    assert (np.abs(got[ok] - ref[ok]) <= 1e-4 * np.maximum(1.0, np.abs(ref[ok]))).all()
    # rejected before any launch
    before = lw.clone()
    one = t(np.array([1.0], np.float32))
    bad = {'operand code 3': [((0, one, 3, one, 0), one, 0, 1.0, 0)],
           'nine terms': [((2, None, 0, None, 0), one, 0, 1.0, 0)] * 9,
           'kind 6': [((6, one, 0, one, 0), one, 0, 1.0, 0)],
           'flag 1 on Poisson': [((3, one, 0, None, 0), one, 0, 1.0, 1)],
           'no x and no flag 4': [((0, one, 0, one, 0), None, 0, 1.0, 0)],
           'per-group operand shorter than M': [((0, t(mean_g[:2]), 2, one, 0), one, 0, 1.0, 0)]}
    for name, terms in bad.items():
        with pytest.raises(RuntimeError):
            run.fused_groups(None, N, None, terms, tv, lw, False)
    with pytest.raises(RuntimeError):       # a draw at a Categorical address
        run.fused_groups(eng.spec.address_id['a_cat'], N, one.expand(2).contiguous(), [], tv, lw, False, y=torch.zeros(M, 8, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(lw, before)


# ---- 3. the draws as a distribution ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('address,K', [('a_normal', 10), ('a_uniform', 10)])
def test_draws_follow_the_group_proposal(address, K):
    eng, run, sd = _eng(K)
    n = 40000
    rng = np.random.default_rng(3)
    y, x = _inputs(address, K, 3, rng)
    value, lw, _ = _call(run, eng, address, y, x, n, 4, 0, stats=False)
    v = value.cpu().numpy()
    dist, prior = HEADS[address]
    for g in (0, 2):
        _, (mu, sd_, p) = _log_q64(address, K, y[g:g + 1], v[:1], 1)
        mu, sd_, p = mu[0], sd_[0], p[0]
        if dist == 'Normal':
            cdf = lambda z: MC.mix_cdf64(['Normal'] * K, [[mu[k], sd_[k]] for k in range(K)], p, z)      # noqa: E731
        else:
            lo, hi = prior
            a, b = O.std_normal_cdf((lo - mu) / sd_), O.std_normal_cdf((hi - mu) / sd_)

            def cdf(z):
                zz = np.clip(np.asarray(z, np.float64), lo, hi)[:, None]
                return (p * (O.std_normal_cdf((zz - mu) / sd_) - a) / (b - a)).sum(1)
        d = MC.ks_distance(v[g * n:(g + 1) * n], cdf)
        print('KS distance, group %d: %.4f (bar %.4f)' % (g, d, 1.95 / math.sqrt(n)))
        assert d < 1.95 / math.sqrt(n), (address, g, d)


# ---- 4. end to end on the golden networks -----------------------------------------------------------------------------------------
def _observations(M, rng):
    return [{'obs0': float(np.float32(rng.uniform(5.0, 11.0))), 'obs1': float(np.float32(rng.uniform(5.0, 11.0)))} for _ in range(M)]


def _gum_model(net):
    from models import GaussianWithUnknownMean
    model = GaussianWithUnknownMean()
    model._inference_network = net
    return model


def _ff_model(net):
    """A one-statement program at the FeedForward golden network's first address (its own program is Marsaglia's loop)."""
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal, Uniform

    class UniformUnknownMean(Model):
        def forward(self):
            x = pyprob.sample(Uniform(-1, 1), address='32__forward__marsaglia__x')
            likelihood = Normal(x * 3.0 + 8.0, math.sqrt(2))
            pyprob.observe(likelihood, name='obs0')
            pyprob.observe(likelihood, name='obs1')
            return x
    model = UniformUnknownMean()
    model._inference_network = net
    return model


def _rescore_group(onet, meta, address, dist, prior, obs, v, mean_of, sigma):
    """Oracle log-weights of one group's particles under ITS observation (+ the two Normal observes around mean_of(v))."""
    y = [float(obs[k]) for k in meta['obs_names']]
    v64 = v.astype(np.float64)
    if meta.get('network', 'lstm') == 'feedforward':
        n = len(v)
        _, _, _, lw = O.is_rescore_feedforward(onet, y, np.ones(n, np.int64), np.zeros(n, np.int64), v64,
                                               np.tile(np.array([list(prior) + [0.0]]), (n, 1)), [address], [dist])
    else:
        _, lw = O.is_rescore_lockstep(onet, y, [dict(address=address, dist_name=dist, values=v64, prior=np.array([list(prior)]))], len(v))
    mean = mean_of(v64)
    return lw + sum(np.asarray(O.normal_log_prob(yy, mean, sigma), np.float32).astype(np.float64) for yy in y)


def _check_posteriors(model, posts, observes, N, onet, meta, address, dist, prior, mean_of):
    assert model._batch_ok is True and len(posts) == len(observes)
    for g, (post, obs) in enumerate(zip(posts, observes)):
        v = post._all_values.cpu().numpy()
        lw = post._all_log_weights.cpu().numpy().astype(np.float64)
        assert v.shape == (N,) and post.length == N and np.isfinite(v).all()
        ref = _rescore_group(onet, meta, address, dist, prior, obs, v, mean_of, math.sqrt(2))
        assert np.isfinite(ref).all()
        err = np.abs(lw - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() < 1e-4, (g, float(err.max()), int(err.argmax()))
        w = np.exp(lw - lw.max())
        w /= w.sum()
        assert abs(post.mean - float((w * v).sum())) <= 1e-9 * max(1.0, abs(post.mean)), g
        assert abs(post.effective_sample_size - 1.0 / float((w * w).sum())) <= 1e-9 * post.effective_sample_size, g


@pytest.mark.parametrize('case', ['gum', 'ff'])
def test_golden_networks_seven_observations(case):
    net, meta, params, isr = network_from_golden(case, 'cuda:0')
    onet = O.Net(params, meta['obs_names'], K=meta['mixture_components'])
    M, N = 7, 1000
    observes = _observations(M, np.random.default_rng(11))
    if case == 'gum':
        model, address, dist, prior, mean_of = _gum_model(net), meta['addresses'][0], 'Normal', (1.0, math.sqrt(5.0)), (lambda v: v)
    else:
        model, address, dist, prior, mean_of = _ff_model(net), meta['addresses'][0], 'Uniform', (-1.0, 1.0), (lambda v: 3.0 * v + 8.0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
        # the tensor form of `observes`, and the same call again: the same particles
        again = model.posterior_results_batch(N, {k: torch.tensor([o[k] for o in observes]) for k in ('obs0', 'obs1')}, seed=13, offset=64)
    _check_posteriors(model, posts, observes, N, onet, meta, address, dist, prior, mean_of)
    for a, b in zip(posts, again):
        assert torch.equal(a._all_values, b._all_values) and torch.equal(a._all_log_weights, b._all_log_weights)
        assert a.mean == b.mean and a.effective_sample_size == b.effective_sample_size
    if case == 'gum':       # M = 1: one row through pp_is_batch_first
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            one = model.posterior_results_batch(N, observes[3:4], seed=5)
        _check_posteriors(model, one, observes[3:4], N, onet, meta, address, dist, prior, mean_of)
        # the groups see different observations: their posteriors differ
        assert len(set(round(p.mean, 3) for p in posts)) == M


def test_h512_benchmark_network_sixty_four_observations():
    """The large-network route of pp_is_batch_first (the MFMA tile kernels of gemm_f32 at M = 64 rows, H = 512)."""
    from models import GaussianWithUnknownMean
    model = GaussianWithUnknownMean()
    torch.manual_seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=256, batch_size=256, lstm_dim=512, seed=1,
                                      observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}})
    eng = model._inference_network._engine
    params = {k: v.numpy() for k, v in eng.state_dict().items()}
    onet = O.Net(params, ['obs0', 'obs1'], K=eng.spec.K)
    meta = dict(obs_names=['obs0', 'obs1'])
    M, N = 64, 1024
    observes = _observations(M, np.random.default_rng(12))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=21)
    _check_posteriors(model, posts, observes, N, onet, meta, eng.spec.addresses[0].address, 'Normal', (1.0, math.sqrt(5.0)), lambda v: v)


# ---- 5. the fallback ------------------------------------------------------------------------------------------------------------
def test_two_statement_program_equals_the_loop_bit_for_bit():
    model, net, meta, params = lockstep_network('cuda:0')
    observes = [{'obs0': 8.0, 'obs1': 9.0}, {'obs0': 7.0, 'obs1': 7.5}, {'obs0': 9.5, 'obs1': 8.5}]
    N, seed, offset = 500, 3, 77
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=seed, offset=offset)
        assert model._batch_ok is False and len(posts) == 3
        for g, post in enumerate(posts):
            ref = model.posterior_results(N, IC, observe=observes[g], seed=seed, offset=offset + g * N)
            assert post.num_paths > 1
            assert torch.equal(post._all_values, ref._all_values) and torch.equal(post._all_log_weights, ref._all_log_weights)
            assert post.mean == ref.mean and post.effective_sample_size == ref.effective_sample_size


def test_program_that_computes_with_an_observed_value_equals_the_loop():
    """`y = observe(...)` handed back to the program is one value per group in a batched call: arithmetic that mixes it with a
    per-particle tensor is outside the fast path (not a shape error), and the call is the loop of single calls."""
    import pyprob_amd as pyprob
    from models import GaussianWithUnknownMean
    from pyprob_amd.distributions import Normal
    net, meta, params, isr = network_from_golden('gum', 'cuda:0')

    class ReadsObservation(GaussianWithUnknownMean):
        def forward(self):
            mu = pyprob.sample(Normal(self.prior_mean, self.prior_stddev))
            y = pyprob.observe(Normal(mu, self.likelihood_stddev), name='obs0')
            pyprob.observe(Normal(mu, self.likelihood_stddev), name='obs1')
            return mu + 0.0 * y
    model = ReadsObservation()
    model._inference_network = net
    observes = _observations(3, np.random.default_rng(2))
    N = 300
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=4, offset=9, lock_step=True)
        assert model._batch_ok is False and len(posts) == 3
        for g, post in enumerate(posts):
            ref = model.posterior_results(N, IC, observe=observes[g], seed=4, offset=9 + g * N, lock_step=True)
            assert torch.equal(post._all_values, ref._all_values) and torch.equal(post._all_log_weights, ref._all_log_weights)
