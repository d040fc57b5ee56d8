"""pp_is_gmm_groups (csrc/is_gmm.hip) and Empirical.density_estimate on the device.

1. PARITY with the float64 numpy restatement (gmm_ref.py) at fixed iteration counts (tol = 0), over the sizes at which the kernels
   take another path (one tile, exactly one tile, one particle more, several tiles, 35 tiles) and every compiled K of the list, with
   log-weights of spread ~1, every 97th particle skipped (-inf) and NaN under the skipped particles only; a narrow case far from 0.
   BOUND: the largest relative deviation of pi, mu, v and the lower bound measured on the MI355X is written per case to
   profiles/gmm_em_errors.jsonl (PP_GMM_ERRORS=<file> makes this test append its figures); the bound is 100 times the largest
   measured - the device and numpy differ in the order of the sums and in exp / log to an ulp or two - and never looser than 1e-8.
2. CONVERGENCE at tol = 1e-3 on cases whose reference change sequence stays 1 % away from tol: n_iter and the flag are equal.
3. EXACT EQUALITIES: repeated calls, groups against one-group calls, PP_GMM_CHECK, with and without statistics.
4. DEGENERATE input. 5. END TO END on a lock-step posterior, its marginal and a batched call."""
import json
import os
import warnings

import numpy as np
import pytest

import gmm_ref as G
from pyprob_amd import lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
DEV = 'cuda:0'
REG = 1e-6
# Measured on the MI355X (profiles/gmm_em_errors.jsonl): the largest relative deviation over all parity and convergence cases is
# MEASURED_MAX (K = 16, n_per = 70001, seven iterations; 1e-16 .. 1.3e-15 everywhere else); the bound is 100 times that.
MEASURED_MAX = 1.7e-15
BOUND = 100 * MEASURED_MAX
assert BOUND <= 1e-8

# (K, n_per, max_iter): every K at a one-tile size and at a many-tile size
PARITY = [(1, 1, 1), (1, 63, 2), (1, 4097, 7), (2, 2047, 7), (2, 70001, 2), (3, 2048, 2), (3, 2049, 7), (5, 63, 7), (5, 4097, 1),
          (16, 2047, 2), (16, 2049, 1), (16, 70001, 7)]


def _data(M, n, seed, narrow=False, modes=4):
    """lw, x [M, n] float32: `modes` Gaussian modes (narrow: three modes 0.2 apart at 1000, sd 0.05), log-weights of spread ~1,
    every 97th particle without weight and with a NaN value."""
    rng = np.random.default_rng(seed)
    comp = rng.integers(0, 3 if narrow else modes, (M, n))
    if narrow:
        x = 1000.0 + 0.2 * comp + rng.normal(0.0, 0.05, (M, n))
    else:
        x = 3.0 + 2.5 * comp + rng.normal(0.0, 0.5, (M, n)) * (1.0 + 0.3 * comp)
    lw = rng.normal(0.0, 1.0, (M, n))
    skip = (np.arange(n) % 97) == 13
    lw[:, skip], x[:, skip] = -np.inf, np.nan
    return lw.astype(np.float32), x.astype(np.float32)


def _init(lw, x, K):
    return np.stack([G.init_ref(lw[g], x[g], K, REG) for g in range(lw.shape[0])])


def _call(lw, x, K, init, max_iter, tol, stats=None, reg=REG):
    from pyprob_amd import ops as P
    M, n = lw.shape
    out = P.ops.is_gmm_groups(torch.from_numpy(lw.reshape(-1)).to(DEV), torch.from_numpy(x.reshape(-1)).to(DEV), K, n,
                              None if stats is None else torch.from_numpy(stats).to(DEV),
                              torch.from_numpy(np.ascontiguousarray(init, np.float64)).to(DEV), max_iter, tol, reg)
    assert out.dtype == torch.float64 and out.shape == (M, L.PP_IS_GMM_WIDTH(K)) and out.is_cuda
    return out.cpu().numpy()


def _record(label, K, n, max_iter, dev):
    print('gmm parity %-28s K %2d n_per %6d iterations %2d  max relative deviation %.3g' % (label, K, n, max_iter, dev))
    path = os.environ.get('PP_GMM_ERRORS')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps({'case': label, 'K': K, 'n_per': n, 'n_iter': max_iter, 'max_rel_dev': dev, 'bound': BOUND}) + '\n')


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,n,max_iter', PARITY)
def test_parity_with_the_numpy_restatement(K, n, max_iter):
    lw, x = _data(2, n, 100 + K + n)
    init = _init(lw, x, K)
    got = _call(lw, x, K, init, max_iter, 0.0)
    want = G.gmm_groups_ref(lw, x, init, max_iter, 0.0, REG)
    dev, same = G.deviation(got, want, K)
    _record('modes', K, n, max_iter, dev)
    assert same and (got[:, 3 * K + 1] == max_iter).all() and (got[:, 3 * K + 2] == 0).all()
    assert np.array_equal(got[:, 3 * K + 5], want[:, 3 * K + 5]) and np.abs(got[:, 3 * K + 3] / want[:, 3 * K + 3] - 1).max() <= BOUND
    assert np.isfinite(got).all() and dev <= BOUND


def test_parity_on_a_narrow_posterior_far_from_zero():
    """Three modes 0.2 apart at 1000, sd 0.05: sums about the current mean keep the variances."""
    K, n, max_iter = 3, 4097, 7
    lw, x = _data(2, n, 7, narrow=True)
    init = _init(lw, x, K)
    got = _call(lw, x, K, init, max_iter, 0.0)
    want = G.gmm_groups_ref(lw, x, init, max_iter, 0.0, REG)
    dev, same = G.deviation(got, want, K)
    _record('narrow at 1000', K, n, max_iter, dev)
    assert same and dev <= BOUND
    sd = np.sqrt(got[:, 2 * K:3 * K])
    assert (sd > 0.03).all() and (sd < 0.12).all() and (np.abs(np.sort(got[:, K:2 * K], 1) - [1000.0, 1000.2, 1000.4]) < 0.05).all()


# ---- 2. convergence --------------------------------------------------------------------------------------------------------
CONVERGENCE = [(1, 63, 1), (2, 2049, 2), (3, 4097, 3), (3, 2048, 4), (5, 70001, 5), (2, 70001, 6)]      # (K, n_per, seed)


@pytest.mark.parametrize('K,n,seed', CONVERGENCE)
def test_convergence_at_the_default_tolerance(K, n, seed):
    tol = 1e-3
    lw, x = _data(1, n, seed, modes=K)
    init = _init(lw, x, K)
    row, bounds = G.em_ref(lw[0], x[0], init[0], 100, tol, REG)
    changes = np.abs(np.diff(bounds))
    print('gmm convergence K %d n_per %d: reference changes %s' % (K, n, changes))
    # the case itself: no change of the reference within 1 % of tol, so an ulp cannot move the stop
    assert row[3 * K + 2] == 1.0 and (np.abs(changes - tol) > 0.01 * tol).all() and 2 <= row[3 * K + 1] <= 30
    got = _call(lw, x, K, init, 100, tol)
    dev, same = G.deviation(got, row[None], K)
    _record('converged', K, n, int(row[3 * K + 1]), dev)
    assert same and got[0, 3 * K + 1] == row[3 * K + 1] and got[0, 3 * K + 2] == 1.0 and dev <= BOUND


def test_a_fit_that_hits_max_iter_is_not_converged():
    K, n = 3, 2049
    lw, x = _data(1, n, 31)
    init = np.array([[1 / 3, 1 / 3, 1 / 3, 4.0, 6.0, 8.0, 4.0, 4.0, 4.0]])      # a wide start: the bound still climbs by > 2e-3 a step
    row, bounds = G.em_ref(lw[0], x[0], init[0], 5, 1e-3, REG)
    assert row[3 * K + 2] == 0.0 and (np.abs(np.diff(bounds)) > 2e-3).all()
    got = _call(lw, x, K, init, 5, 1e-3)
    dev, same = G.deviation(got, row[None], K)
    _record('max_iter reached', K, n, 5, dev)
    assert same and got[0, 3 * K + 1] == 5 and got[0, 3 * K + 2] == 0.0 and dev <= BOUND


# ---- 3. exact equalities ---------------------------------------------------------------------------------------------------
def _separated(M, n, seed):
    """Groups whose modes lie further apart from group to group: they converge at different iterations."""
    rng = np.random.default_rng(seed)
    comp = rng.integers(0, 3, (M, n))
    gap = 0.8 + 0.6 * (np.arange(M) % 5)[:, None]
    x = 2.0 + gap * comp + rng.normal(0.0, 0.5, (M, n))
    lw = rng.normal(0.0, 1.0, (M, n))
    lw[:, 13::97] = -np.inf
    return lw.astype(np.float32), x.astype(np.float32)


@pytest.mark.parametrize('n', [2049, 100])
def test_groups_equal_the_one_group_call_and_a_call_repeated(n):
    K = 3
    lw, x = _separated(257, n, 41)
    init = _init(lw, x, K)
    big = _call(lw, x, K, init, 40, 1e-3)
    assert np.array_equal(_bits(big), _bits(_call(lw, x, K, init, 40, 1e-3)))                    # a call repeated
    three = _call(lw[:3], x[:3], K, init[:3], 40, 1e-3)
    assert np.array_equal(_bits(three), _bits(big[:3]))
    for g in (0, 2, 129, 256):
        one = _call(lw[g:g + 1], x[g:g + 1], K, init[g:g + 1], 40, 1e-3)
        assert np.array_equal(_bits(one), _bits(big[g:g + 1])), g
    # groups that converge at different iterations keep their own n_iter (the reference's, for those it pins)
    iters = big[:, 3 * K + 1]
    print('n_per %d: n_iter of the 257 groups from %d to %d' % (n, iters.min(), iters.max()))
    assert len(np.unique(iters)) > 1 and (big[:, 3 * K + 2] == 1.0).all()
    for g in (0, 1, 2, 3, 4):
        row, bounds = G.em_ref(lw[g], x[g], init[g], 40, 1e-3, REG)
        if (np.abs(np.abs(np.diff(bounds)) - 1e-3) > 1e-5).all():
            assert big[g, 3 * K + 1] == row[3 * K + 1], g


def test_check_every_and_statistics_do_not_change_the_bits(monkeypatch):
    K, n = 2, 2049
    lw, x = _separated(5, n, 43)
    init = _init(lw, x, K)
    monkeypatch.setenv('PP_GMM_CHECK', '8')
    base = _call(lw, x, K, init, 60, 1e-4)
    assert len(np.unique(base[:, 3 * K + 1])) > 1 and base[:, 3 * K + 1].max() > 8
    for every in ('1', '100'):
        monkeypatch.setenv('PP_GMM_CHECK', every)
        assert np.array_equal(_bits(_call(lw, x, K, init, 60, 1e-4)), _bits(base)), every
    stats = np.zeros((5, 6))
    stats[:, 0] = np.where(np.isfinite(lw), lw, -np.inf).max(1).astype(np.float64)
    assert np.array_equal(_bits(_call(lw, x, K, init, 60, 1e-4, stats=stats)), _bits(base))
    sl, sx = lw[:2, :100].copy(), x[:2, :100].copy()                                # (one tile: the other route to the maximum)
    st = np.zeros((2, 6))
    st[:, 0] = np.where(np.isfinite(sl), sl, -np.inf).max(1).astype(np.float64)
    assert np.array_equal(_bits(_call(sl, sx, K, init[:2], 5, 0.0, stats=st)), _bits(_call(sl, sx, K, init[:2], 5, 0.0)))


# ---- 4. degenerate input -----------------------------------------------------------------------------------------------------
def test_degenerate_groups_terminate():
    K, n = 2, 300
    lw, x = _data(4, n, 51)
    lw[0] = -np.inf                                                               # no particle with a finite log-weight
    lw[1] = -np.inf
    lw[1, 77] = 0.5                                                               # one surviving particle
    x[2] = 4.25                                                                   # all values equal
    x[3] = np.where(np.isnan(x[3]), 0.0, x[3])
    lw[3, 13] = 0.0                                                               # a NaN value under a finite weight
    x[3, 13] = np.nan
    init = np.stack([np.array([0.5, 0.5, 3.0, 6.0, 1.0, 1.0])] * 4)
    init[2] = [0.5, 0.5, 4.25, 4.25, REG, REG]
    got = _call(lw, x, K, init, 9, 1e-3)
    empty, single, flat, nan = got
    assert np.isnan(empty[:3 * K + 1]).all() and empty[3 * K + 1:].tolist() == [0.0, 1.0, 0.0, 0.0, -np.inf]
    assert np.isfinite(single).all() and single[3 * K + 4] == 1 and single[3 * K + 3] == 1.0 and single[3 * K + 2] == 1.0
    assert np.abs(single[K:2 * K] - x[1, 77]).min() < 1e-3
    assert np.isfinite(flat).all() and (flat[2 * K:3 * K] == REG).all() and (flat[K:2 * K] == 4.25).all() and flat[3 * K + 2] == 1.0
    assert np.isnan(nan[:3 * K + 1]).all() and nan[3 * K + 1] == 9 and nan[3 * K + 2] == 0.0 and nan[3 * K + 4] > 0
    want = G.gmm_groups_ref(lw, x, init, 9, 1e-3, REG)
    # n_iter, flag and count are the reference's. The parameters of these groups are no parity case: the variance of ONE particle is
    # the rounding residue of Q / N - d^2 - two numbers of size (x - mu)^2 ~ 10 that differ in the 15th digit - on top of
    # reg_covar: an ulp of (x - mu)^2 is 2e-15, 2e-9 of reg_covar, and through -1/2 log v half of that reaches the weights
    # (measured on the MI355X: 1.2e-16 absolute on v, 6.2e-11 relative on pi_0). What holds is that bound.
    assert G.deviation(got[:3], want[:3], K)[1]
    assert (single[2 * K:3 * K] >= REG).all() and (single[2 * K:3 * K] <= REG * (1 + 2e-9)).all()
    np.testing.assert_allclose(single[:2 * K], want[1, :2 * K], rtol=1e-9)
    np.testing.assert_allclose(flat[:3 * K + 1], want[2, :3 * K + 1], rtol=1e-12)
    # five distinct values, sixteen components: components coincide, the output is finite
    rng = np.random.default_rng(52)
    x5 = rng.integers(0, 5, (1, 2500)).astype(np.float32)
    lw5 = rng.normal(0, 1, (1, 2500)).astype(np.float32)
    out = _call(lw5, x5, 16, _init(lw5, x5, 16), 25, 1e-3)
    assert np.isfinite(out).all() and abs(out[0, :16].sum() - 1.0) < 1e-12 and (out[0, 32:48] >= REG).all()
    assert (out[0, 16:32] >= 0).all() and (out[0, 16:32] <= 4).all()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
def test_posterior_and_marginal_end_to_end():
    from test_gpu_joint_moments import _log_columns, _posterior, _straight_line_model
    _straight_line_model()
    N = 100000
    post = _posterior(N)
    assert post._device_backed() and post.length == N
    mix = post.density_estimate(3)
    f = mix.fit
    assert f.converged and f.count == N and f.metadata['op'] == 'density_estimate' and abs(f.weights.sum() - 1.0) < 1e-12
    assert np.isfinite(f.lower_bound) and (f.stddevs > 0).all() and not post._host_weights_ready()
    lw, x = post._log_weights.cpu().numpy(), post._values.cpu().numpy()
    mean = float((f.weights * f.means).sum())
    assert abs(mean - post.mean) < 1e-6 * max(1.0, abs(post.mean)) + 1e-3 * post.stddev      # EM keeps the weighted mean
    # one further E-step from the fitted parameters: its lower bound is the weighted mean log-density of the fitted mixture
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        again = post.density_estimate(3, tol=0.0, max_iter=1, weights_init=f.weights, means_init=f.means, stddevs_init=f.stddevs)
    w = G.weights_ref(lw)[0]
    want = float((w * G.mixture_logpdf(x, f.weights, f.means, f.stddevs)).sum() / w.sum())
    print('lower bound of one further E-step %.17g, weighted mean log-density %.17g' % (again.fit.lower_bound, want))
    assert abs(again.fit.lower_bound - want) <= BOUND * abs(want)
    # the Mixture itself holds float32 parameters and scores in float32: 2^-24 on parameters of order 1 .. 10 and sd ~ 0.5 moves a
    # log-density of order 1 by ~1e-5; the weighted mean is taken in float64
    lp = mix.log_prob(post._values.cpu()).double().numpy()
    assert abs(float((w * lp).sum() / w.sum()) - want) <= 1e-4
    a = _log_columns(post)[0][1].cpu().numpy()
    lat = post.marginal('mu').density_estimate(2)
    all_lw = post._all_log_weights.cpu().numpy()
    ref = G.em_ref(all_lw, a, G.init_ref(all_lw, a, 2))[0]
    assert lat.fit.converged and lat.fit.n_iter == ref[7] and lat.fit.count == N
    np.testing.assert_allclose(np.concatenate([lat.fit.weights, lat.fit.means, lat.fit.stddevs ** 2]), ref[:6], rtol=1e-5)


def test_density_estimate_batch_is_one_operator_call_and_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from test_gpu_joint_moments import _straight_line_model
    model, full = _straight_line_model()
    M, N, K = 16, 3000, 3
    rng = np.random.default_rng(3)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
    assert model._batch_ok is True and len(posts) == M
    count = [0]
    real = P.ops.is_gmm_groups

    def counted(*a):
        count[0] += 1
        return real(*a)
    monkeypatch.setattr(P.ops, 'is_gmm_groups', counted, raising=False)

    def row(m):
        f = m.fit
        return np.concatenate([f.weights, f.means, f.stddevs, [f.lower_bound, f.n_iter, f.converged, f.count]])
    loop = [p.density_estimate(K) for p in posts]
    assert count[0] == M
    fast = pyprob_amd.density_estimate_batch(posts, K)
    assert count[0] == M + 1 and len(fast) == M                                   # ONE operator call for the M groups
    assert all(np.array_equal(_bits(row(a)), _bits(row(b))) for a, b in zip(fast, loop))
    assert all(m.fit.converged and m.fit.count == N for m in fast)
    lat = pyprob_amd.density_estimate_batch(posts, 2, address='mu')
    assert count[0] == M + 2
    assert all(np.array_equal(_bits(row(a)), _bits(row(p.marginal('mu').density_estimate(2)))) for a, p in zip(lat, posts))
