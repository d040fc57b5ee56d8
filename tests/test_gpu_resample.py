"""Resampling device-backed posteriors on the device (csrc/is_resample.hip pp_is_cdf_groups / pp_is_resample_groups; the
is_cdf_groups / is_resample_groups operators; Empirical.resample / sample / median; pyprob_amd.resample_batch):
 1. the cdf indexes particles, groups and tiles exactly: poison around the live block survives, the cdf never decreases and is flat
    exactly across particles of weight 0, every entry agrees with the float64 cumsum within (N + 4) 2^-52 of the group's total,
    group g of an M-group call is bit-equal to the one-group call on row g, two calls and both sources of the maximum are bit-equal;
 2. the drawn indices equal numpy.searchsorted on the device's own cdf at targets rebuilt on the host from the Philox block, element
    for element; values are gathered from the drawn index; an M-group call is the M one-group calls at offset + g n_out;
 3. the draws as a distribution (DKW bar), no particle of weight 0, and the uniform carries more than 24 bits;
 4. end to end on a GUM posterior of 10^5 particles - the test that fails without the feature (the parent's resample takes no seed
    and returns a Python list);
 5. resample_batch: one cdf launch and one draw launch for the M groups of a batched call, bit-equal to the loop.
If pyprob_amd/libpyprob_amd.so is missing or stale here nothing below can run: L.load() raises instead of skipping."""
import math
import warnings

import numpy as np
import pytest

import resample_ref as R
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK

T = L.PP_IS_CDF_TILE
SHAPES = [(1, 1), (3, 1), (257, 1), (5, 63), (5, 64), (5, 65), (5, 255), (5, 256), (5, 257), (5, T - 1), (5, T), (5, T + 1),
          (3, 2 * T + 1), (2, 70001), (66000, 2)]      # (66000 groups: two launch chunks of at most 65535)
# The draws of a shape: the float64 restatement runs Philox in numpy, a few seconds per 10^7 draws, so 66000 groups take 1 and 7
# draws each and not 1000 (the draw kernel strides over the outputs of a call: it has no launch chunk to cross).
DRAWS = [(M, N, n_out) for M, N in SHAPES for n_out in (1, 7, 1000) if M * n_out <= 2 ** 20]
PAD = 3            # poisoned rows in front of and behind the live block
DEV = 'cuda:0'
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _groups_to_check(M):
    return range(M) if M <= 7 else [0, 1, 127, 255, 256] + [g for g in (65534, 65535, 65536, M - 2) if g < M]


def _stats_rows(M):
    return range(M) if M <= 1000 else _groups_to_check(M)


def _inputs(M, N):
    """lw ~ normal(0, 3) with about 2 % of the entries -inf / NaN / +inf, the last group of M >= 2 entirely non-finite; values."""
    rng = np.random.default_rng(1000 * M + N)
    lw = rng.normal(0.0, 3.0, (M, N)).astype(np.float32)
    bad = rng.random((M, N)) < 0.02
    lw[bad] = rng.choice(np.array([-np.inf, np.nan, np.inf], np.float32), int(bad.sum()))
    if M >= 2:
        lw[M - 1] = rng.choice(np.array([-np.inf, np.nan, np.inf], np.float32), N)
    return lw, rng.normal(0.0, 2.0, (M, N)).astype(np.float32)


def _cdf_call(lw, stats=None):
    """One pp_is_cdf_groups call on host lw [M, N]; the device buffers carry PAD poisoned (NaN) rows in front of and behind the live
    block. Returns the host copy of the WHOLE cdf buffer [PAD + M + PAD, N] and the device buffer."""
    lib = L.load()
    M, N = lw.shape
    tl = torch.full((PAD + M + PAD, N), float('nan'), dtype=torch.float32, device=DEV)
    tl[PAD:PAD + M] = torch.from_numpy(lw).to(DEV)
    tc = torch.full((PAD + M + PAD, N), float('nan'), dtype=torch.float64, device=DEV)
    need = lib.pp_is_cdf_workspace_bytes(M, N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_cdf_groups(tl[PAD:].data_ptr(), M, N, L.ptr(stats), tc[PAD:].data_ptr(), ws.data_ptr(), need, L.stream_ptr()),
            'pp_is_cdf_groups')
    torch.cuda.synchronize()
    return tc.cpu().numpy(), tc


def _stats(lw, x):
    """pp_is_stats per group: device double [M, 6]. One launch per group: beyond 1000 groups only the rows of _stats_rows come from
    pp_is_stats; the others hold the maximum of the group's finite log-weights (exact in any arithmetic, and asserted below to be
    what pp_is_stats gives) and NaN in the five entries pp_is_cdf_groups does not read."""
    from pyprob_amd import ops as P
    M = lw.shape[0]
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    host = np.full((M, 6), np.nan)
    host[:, 0] = np.where(np.isfinite(lw), lw, -np.inf).max(axis=1)
    st = torch.from_numpy(host).to(DEV)
    for g in _stats_rows(M):
        st[g] = P.ops.is_stats(torch.from_numpy(lw[g]).to(DEV), torch.from_numpy(x[g]).to(DEV), scratch)[:6]
    some = np.isfinite(host[:, 0])      # (a group without a finite log-weight has no maximum to compare)
    assert np.array_equal(_bits(st[:, 0].cpu().numpy()[some]), _bits(host[some, 0]))
    return st.contiguous()


def _case(M, N):
    """The inputs of a shape and its device cdf, computed once and shared by the tests (never modified)."""
    if (M, N) not in _CASES:
        lw, x = _inputs(M, N)
        whole, dev = _cdf_call(lw)
        _CASES[(M, N)] = (lw, x, whole, dev)
    return _CASES[(M, N)]


# ---- 1. the cdf, exact indexing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', SHAPES)
def test_cdf_of_every_group(M, N):
    lw, x, whole, _ = _case(M, N)
    assert np.isnan(whole[:PAD]).all() and np.isnan(whole[PAD + M:]).all()          # the poison survives
    c = whole[PAD:PAD + M]
    assert np.isfinite(c).all()
    w = R.weights_ref(lw)
    ref = np.cumsum(w, axis=1)
    total = ref[:, -1:]
    d = np.diff(np.concatenate([np.zeros((M, 1)), c], axis=1), axis=1)
    assert (d >= 0).all()                                                           # never decreases
    assert (d[w == 0] == 0).all()                                                   # flat across a particle of weight 0 ...
    # ... and only there: an addend above 4 ulp of the sum it joins always moves it (sum <= total; every positive weight of these
    # inputs is far above that: lw spans < 60 around its maximum, e^-60 N > 2^-50 only for N > 10^10)
    big = w > 4 * 2.0 ** -52 * total
    assert (w[w > 0] > 0).all() and big[w > 0].all() and (d[big] > 0).all()
    # N roundings of a positive sum in any order, plus 2 ulp for each of the two exp implementations
    err = np.abs(c - ref)
    bound = (N + 4) * 2.0 ** -52 * total
    print('cdf: max error / bound = %.3g' % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    if M >= 2:
        assert (c[M - 1] == 0).all()                                                # the non-finite group
    # the maximum pp_is_stats reduced instead of the one found by the first launch: the same bits; sum_w to the same bound
    st = _stats(lw, x)
    with_stats, _ = _cdf_call(lw, st)
    assert np.array_equal(_bits(with_stats[PAD:PAD + M]), _bits(c))
    assert np.isnan(with_stats[:PAD]).all() and np.isnan(with_stats[PAD + M:]).all()
    rows = list(_stats_rows(M))
    sum_w = st.cpu().numpy()[rows, 1]
    assert (np.abs(c[rows, -1] - sum_w) <= bound[rows, 0]).all()
    # two identical calls
    again, _ = _cdf_call(lw)
    assert np.array_equal(_bits(again[PAD:PAD + M]), _bits(c))
    # group g against the one-group call on row g
    for g in _groups_to_check(M):
        one, _ = _cdf_call(lw[g:g + 1])
        assert np.array_equal(_bits(one[PAD]), _bits(c[g])), (g, int(np.argmax(_bits(one[PAD]) != _bits(c[g]))))


# ---- 2. the indices, exact ------------------------------------------------------------------------------------------------------------
def _draw_call(cdf_dev_rows, values, M, N, lo, hi, n_out, seed, offset):
    """One pp_is_resample_groups call; cdf_dev_rows: device double [M, N] (a view of the padded buffer). Index and value buffers
    carry PAD * n_out poisoned elements behind M n_out. Returns host copies of the whole buffers."""
    lib = L.load()
    ti = torch.full(((M + PAD) * n_out,), -7777, dtype=torch.int64, device=DEV)
    tv = torch.full(((M + PAD) * n_out,), float('nan'), dtype=torch.float32, device=DEV)
    L.check(lib.pp_is_resample_groups(cdf_dev_rows.data_ptr(), L.ptr(values), M, N, lo, hi, n_out, seed, offset, ti.data_ptr(),
                                      tv.data_ptr() if values is not None else None, L.stream_ptr()), 'pp_is_resample_groups')
    torch.cuda.synchronize()
    return ti.cpu().numpy(), tv.cpu().numpy()


@pytest.mark.parametrize('M,N,n_out', DRAWS)
def test_indices_are_searchsorted_on_the_device_cdf(M, N, n_out):
    lw, x, whole, dev = _case(M, N)
    c = whole[PAD:PAD + M]
    tx = torch.from_numpy(x).to(DEV).contiguous()
    seed, offset = 1234567 + N, 5 * 2 ** 32 + 17
    for lo, hi in {(0, N), (N // 3, N - N // 4)}:
        if not lo < hi:
            continue
        idx, val = _draw_call(dev[PAD:], tx, M, N, lo, hi, n_out, seed, offset)
        assert (idx[M * n_out:] == -7777).all() and np.isnan(val[M * n_out:]).all()      # the poison behind M n_out survives
        idx, val = idx[:M * n_out].reshape(M, n_out), val[:M * n_out].reshape(M, n_out)
        ref_idx, ref_val = R.resample_ref(c, x, lo, hi, n_out, seed, offset)
        assert np.array_equal(idx, ref_idx), (lo, hi, int((idx != ref_idx).sum()))
        assert np.array_equal(val.view(np.uint32), ref_val.view(np.uint32))              # value_out == values[g N + index]
        live = c[:, hi - 1] - (c[:, lo - 1] if lo > 0 else 0.0) > 0
        assert ((idx[live] >= lo) & (idx[live] < hi)).all()
        assert (idx[~live] == -1).all() and np.isnan(val[~live]).all()
        if M >= 2:
            assert not live[M - 1]                                                       # the all-non-finite group: -1 and NaN
        w = R.weights_ref(lw)
        assert (np.take_along_axis(w, np.maximum(idx, 0), 1)[live] > 0).all()            # no particle of weight 0
        # index only / an M-group call is the M one-group calls at offset + g n_out
        only, _ = _draw_call(dev[PAD:], None, M, N, lo, hi, n_out, seed, offset)
        assert np.array_equal(only[:M * n_out].reshape(M, n_out), idx)
        for g in _groups_to_check(M):
            one_i, one_v = _draw_call(dev[PAD + g:], tx[g:], 1, N, lo, hi, n_out, seed, offset + g * n_out)
            assert np.array_equal(one_i[:n_out], idx[g]) and np.array_equal(one_v[:n_out].view(np.uint32), val[g].view(np.uint32)), g


# ---- 3. the draws as a distribution ---------------------------------------------------------------------------------------------------
def test_draws_follow_the_weights():
    from pyprob_amd import ops as P
    rng = np.random.default_rng(7)
    N, n_out = 1000, 200000
    lw = rng.uniform(-13.8, 0.0, N).astype(np.float32)           # weights over six decades
    lw[rng.permutation(N)[:N // 10]] = -np.inf                      # a tenth of them at zero
    cdf = P.ops.is_cdf_groups(torch.from_numpy(lw).to(DEV), N, None)
    idx, none = P.ops.is_resample_groups(cdf, None, N, 0, N, n_out, 99, 0, True)
    assert none.numel() == 0
    idx = idx.cpu().numpy()
    c = cdf.cpu().numpy()
    counts = np.bincount(idx, minlength=N)
    assert counts[np.isinf(lw)].sum() == 0                          # no zero-weight index is drawn
    D = np.abs(np.cumsum(counts) / n_out - c / c[-1]).max()
    print('sup |F_n - F| = %.5f (bar %.5f)' % (D, 1.95 / math.sqrt(n_out)))
    assert D < 1.95 / math.sqrt(n_out)                              # DKW at 10^-3


def test_uniform_carries_more_than_24_bits():
    from pyprob_amd import ops as P
    N, n_out, seed, offset = 2 ** 18, 2 ** 20, 4242, 3
    cdf = P.ops.is_cdf_groups(torch.zeros(N, dtype=torch.float32, device=DEV), N, None)
    c = cdf.cpu().numpy()
    assert np.array_equal(c, np.arange(1, N + 1, dtype=np.float64))     # equal weights: exact
    idx = P.ops.is_resample_groups(cdf, None, N, 0, N, n_out, seed, offset, True)[0].cpu().numpy()
    distinct = len(np.unique(idx)) / n_out
    expect = (N / n_out) * (1.0 - math.exp(-n_out / N))
    print('distinct fraction %.5f (multinomial expectation %.5f)' % (distinct, expect))
    assert abs(distinct - expect) <= 0.01 * expect
    # a 24-bit uniform reaches 64 points per cell and still passes the above. The target rebuilt on the host is what the device
    # searched with (every index matches); total = 2^18 scales u exactly, so u's own bits are the target's
    u = R.uniform53(seed, offset + np.arange(n_out, dtype=np.uint64))
    target, total = R.targets_ref(c, 0, N, u)
    assert total == N and np.array_equal(idx, np.minimum(np.searchsorted(c, target, side='right'), N - 1))
    # (u 2^53 = bits + 0.5: the truncation is `bits`; u01's (x + 0.5) 2^-24 would give x 2^29 + 2^28, ONE value of the low 29 bits)
    low = (target / N * 2.0 ** 53).astype(np.uint64) & np.uint64(2 ** 29 - 1)
    assert len(np.unique(low)) > n_out // 2


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------
_GUM = {}


def _gum_posterior():
    if 'post' not in _GUM:
        import pyprob_amd as pyprob
        from pyprob_amd import Model
        from pyprob_amd.distributions import Normal
        from test_gpu_is_batch_multi import _attach_network

        class Gum(Model):
            def forward(self):
                mu = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='mu')
                pyprob.observe(Normal(mu, math.sqrt(2.0)), name='obs0')
                pyprob.observe(Normal(mu, math.sqrt(2.0)), name='obs1')
                return mu
        model = Gum()
        _attach_network(model, 'lstm', 64)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            _GUM['post'] = model.posterior_results(100000, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=11)
    return _GUM['post']


def test_posterior_is_resampled_on_the_device(monkeypatch):
    """FAILS WITHOUT THE FEATURE: the parent's resample has no seed and returns a list-backed Empirical."""
    from pyprob_amd.distributions import Empirical
    post = _gum_posterior()
    assert post._values.is_cuda and post.length == 100000
    ess = post.effective_sample_size
    bar = 5.0 * post.stddev / math.sqrt(min(20000, ess))
    get_values = Empirical.get_values

    def no_list(self):
        raise AssertionError('the device route built the list of particles')
    monkeypatch.setattr(Empirical, 'get_values', no_list)
    r = post.resample(20000, seed=5)
    again = post.resample(20000, seed=5)
    other = post.resample(20000, seed=6)
    torch.manual_seed(3)
    a = post.resample(100)
    torch.manual_seed(3)
    b = post.resample(100)
    s = post.sample()
    doubled = post.resample(20000, map_func=lambda v: v * 2, seed=5)
    monkeypatch.setattr(Empirical, 'get_values', get_values)
    assert torch.is_tensor(r._values) and r._values.is_cuda and r._log_weights.is_cuda
    assert r.length == 20000 and r._values.shape == (20000,)
    print('posterior mean %.5f stddev %.5f ESS %.1f; resampled mean %.5f (bar %.5f)' % (post.mean, post.stddev, ess, r.mean, bar))
    assert abs(r.mean - post.mean) <= bar
    assert r.effective_sample_size == 20000
    assert r.metadata['op'] == 'resample' and r.metadata['length'] == 100000 and r.metadata['num_samples'] == 20000
    assert r.metadata['ess_before'] == ess
    rv = r._values.cpu().numpy()
    assert abs(r.mean - rv.astype(np.float64).mean()) <= 1e-10 * max(1.0, abs(r.mean))
    assert np.array_equal(rv.view(np.uint32), again._values.cpu().numpy().view(np.uint32))
    assert not np.array_equal(rv, other._values.cpu().numpy())
    assert np.array_equal(a._values.cpu().numpy().view(np.uint32), b._values.cpu().numpy().view(np.uint32))
    pv = post.values_numpy()
    assert np.isin(rv.astype(np.float64), pv).all()                    # every drawn value is a particle
    assert torch.is_tensor(s) and s.dim() == 0 and post.min <= float(s) <= post.max
    # map_func: only the drawn values travel; a host-backed result
    assert isinstance(doubled._values, list) and doubled.length == 20000
    assert abs(doubled.mean - 2.0 * r.mean) <= bar
    # the weighted median (resample(1000).median) between the 0.45 and 0.55 weighted quantiles in float64
    lw = post._log_weights.cpu().numpy().astype(np.float64)
    w = np.exp(lw - lw.max())
    order = np.argsort(pv)
    cum = np.cumsum(w[order]) / w.sum()
    q45, q55 = pv[order][np.searchsorted(cum, 0.45)], pv[order][np.searchsorted(cum, 0.55)]
    torch.manual_seed(21)
    med = post.median
    print('median %.5f in [%.5f, %.5f]' % (med, q45, q55))
    assert q45 <= med <= q55
    # the A/B switch: the host route, list-backed as before
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    h = post.resample(50)
    assert isinstance(h._values, list) and h.length == 50
    monkeypatch.delenv('PP_EMPIRICAL_DEVICE')
    assert post.resample(50, seed=1)._values.is_cuda
    # an index range
    part = post.resample(500, min_index=1000, max_index=3000, seed=2)
    assert np.isin(part._values.cpu().numpy().astype(np.float64), pv[1000:3000]).all()
    with pytest.raises(ValueError):
        post.resample(5, min_index=10, max_index=10)


# ---- 5. batched --------------------------------------------------------------------------------------------------------------------------
def test_resample_batch_is_one_launch_pair_and_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from test_gpu_is_batch_multi import _model, _observations
    model, sd, addresses = _model(2, 'lstm', 64)
    M, N, K = 5, 300, 64
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, _observations(M, np.random.default_rng(3)), seed=13, offset=64)
        others = model.posterior_results_batch(N, _observations(M, np.random.default_rng(4)), seed=14, offset=0)
    assert model._batch_ok is True and len(posts) == M
    count = {'cdf': 0, 'draw': 0}
    cdf_op, draw_op = P.ops.is_cdf_groups, P.ops.is_resample_groups

    def cdf_counted(*a):
        count['cdf'] += 1
        return cdf_op(*a)

    def draw_counted(*a):
        count['draw'] += 1
        return draw_op(*a)
    monkeypatch.setattr(P.ops, 'is_cdf_groups', cdf_counted, raising=False)
    monkeypatch.setattr(P.ops, 'is_resample_groups', draw_counted, raising=False)
    loop = [p.resample(K, seed=9, offset=g * K) for g, p in enumerate(posts)]          # (every group scans its own cdf)
    assert count == {'cdf': M, 'draw': M}
    fast = pyprob_amd.resample_batch(posts, K, seed=9)
    assert count == {'cdf': M + 1, 'draw': M + 1} and len(fast) == M      # ONE execution of the fast path: a launch pair
    assert len(pyprob_amd.resample_batch(posts, K, seed=10)) == M
    assert count == {'cdf': M + 1, 'draw': M + 2}                         # the call's cdf is kept
    for g, (f, l) in enumerate(zip(fast, loop)):
        fv = f._values.cpu().numpy()
        assert f.length == K and np.array_equal(fv.view(np.uint32), l._values.cpu().numpy().view(np.uint32)), g
        m64 = fv.astype(np.float64).mean()
        assert abs(f.mean - m64) <= 1e-10 * max(1.0, abs(m64)) and abs(f.effective_sample_size - K) <= 1e-10 * K
        assert abs(l.mean - m64) <= 1e-10 * max(1.0, abs(m64)) and l.effective_sample_size == K
        assert f.metadata['op'] == 'resample' and f.metadata['ess_before'] == posts[g].effective_sample_size
        assert np.isin(fv, posts[g]._values.cpu().numpy()).all()
    assert len(set(round(f.mean, 3) for f in fast)) == M                   # the groups differ
    # a shuffled list and a list mixed from two calls take the loop and still match it
    for mixed in ([posts[i] for i in (2, 0, 4, 1, 3)], [posts[0], others[1], posts[2]], posts[:3]):
        before = dict(count)
        got = pyprob_amd.resample_batch(mixed, K, seed=9, offset=1000)
        assert count['draw'] - before['draw'] == len(mixed)
        for g, (p, r) in enumerate(zip(mixed, got)):
            want = p.resample(K, seed=9, offset=1000 + g * K)
            assert np.array_equal(r._values.cpu().numpy().view(np.uint32), want._values.cpu().numpy().view(np.uint32))
