"""Posterior marginals and joint moments of all latents on the device (csrc/is_moments.hip pp_is_moments_groups; the
is_moments_groups operator; Empirical.addresses / marginal / joint / resample_joint; pyprob_amd.joint_batch):
 1. every entry of the kernel's rows against the float64 restatement (tests/moments_ref.py) to 1e-10 of the sum of the absolute
    values of its terms - one particle, a part of a wave, a tile +- 1, the 4-column block edge and 16 columns; particles with
    lw = -inf / +inf / NaN carry NaN column values (a kernel that multiplies by a zero weight instead of skipping fails), one group
    has no finite weight; poison around the output survives;
 2. bit identity: two calls, group g of an M-group call against the one-group call on its slice, with and without `stats`;
 3. rejected calls launch nothing;
 4. a narrow posterior far from zero: the covariance to 1e-8 of sqrt(var_j var_k);
 5. end to end on a three-statement straight-line program; 6. on Marsaglia's branching program; 7. joint_batch is one operator call
    and equals the loop bit for bit; 8. resample_joint draws one index per sample, the index stream of resample();
 9. an address that sits at two statement indices (an `if` without `else` before a shared statement) is one latent over all the
    particles that executed it.
All of 1-8 FAIL WITHOUT THE FEATURE: the parent has neither the symbols nor the methods.
If pyprob_amd/libpyprob_amd.so is missing or stale here nothing below can run: L.load() raises instead of skipping."""
import ctypes as C
import math
import re
import warnings

import numpy as np
import pytest

import moments_ref as MR
from helpers import IS_EMB as EMB
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK

SHAPES = [(1, 1, 1), (1, 63, 2), (3, 257, 5), (7, 300, 3), (2, 2049, 16), (1, 4097, 4), (66000, 2, 1)]      # (66000: two launch chunks)
PAD = 2            # poisoned rows in front of and behind the live rows of the output
DEV = 'cuda:0'
BAR = 1e-10        # the project's bar for its fp64 statistics: 1e-10 of the scale of the sum
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _inputs(M, N, J):
    """lw ~ normal(0, 3); columns ~ normal(j, 1 + j / 4). Where the group is long enough, particles with lw = -inf, +inf and NaN
    whose column values are NaN - in group 1 (M >= 3) the group's FIRST particle among them, so its pivots are 0; the last group of
    M >= 2 has no finite weight at all."""
    rng = np.random.default_rng(10000 * M + 10 * N + J)
    lw = rng.normal(0.0, 3.0, (M, N)).astype(np.float32)
    x = (rng.normal(0.0, 1.0, (J, M, N)) * (1 + np.arange(J)[:, None, None] / 4) + np.arange(J)[:, None, None]).astype(np.float32)
    if N >= 63:
        for g in range(M):
            at = rng.choice(np.arange(1, N), 6, replace=False)
            if M >= 3 and g == 1:
                at[0] = 0
            lw[g, at] = np.array([-np.inf, np.inf, np.nan, -np.inf, np.inf, np.nan], np.float32)
            x[:, g, at] = np.nan
    if M >= 2:
        lw[M - 1] = rng.choice(np.array([-np.inf, np.nan, np.inf], np.float32), N)
        x[:, M - 1, ::2] = np.nan
    return lw, x


def _call(lw, x, stats=None):
    """One pp_is_moments_groups call on host lw [M, N], x [J, M, N]; the output buffer carries PAD poisoned (NaN) rows in front of
    and behind the live rows. Returns the host copy of the whole output [PAD + M + PAD, width]."""
    lib = L.load()
    J, M, N = x.shape
    tl = torch.from_numpy(np.ascontiguousarray(lw).reshape(-1)).to(DEV)
    cols = [torch.from_numpy(np.ascontiguousarray(c).reshape(-1)).to(DEV) for c in x]
    out = torch.full((PAD + M + PAD, L.PP_IS_MOMENTS_WIDTH(J)), float('nan'), dtype=torch.float64, device=DEV)
    need = lib.pp_is_moments_workspace_bytes(M, N, J)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptrs = (C.c_void_p * J)(*[c.data_ptr() for c in cols])
    L.check(lib.pp_is_moments_groups(tl.data_ptr(), C.cast(ptrs, C.c_void_p), J, M, N, L.ptr(stats), out[PAD:].data_ptr(),
                                     ws.data_ptr(), need, L.stream_ptr()), 'pp_is_moments_groups')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _groups_to_check(M):
    """The groups that get calls of their own: all of them, or (one launch each) the first ones and both sides of the launch chunk."""
    return range(M) if M <= 7 else sorted({g for g in (0, 1, 2, 65534, 65535, 65536, M - 2, M - 1) if g < M})


def _stats(lw, x0):
    """pp_is_stats per group: device double [M, 6]. Beyond 7 groups only the rows of _groups_to_check come from pp_is_stats; the
    others hold the maximum of the group's finite log-weights (exact in any arithmetic, and asserted here to be what pp_is_stats
    gives) and NaN in the five entries pp_is_moments_groups does not read."""
    from pyprob_amd import ops as P
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    host = np.full((lw.shape[0], 6), np.nan)
    host[:, 0] = np.where(np.isfinite(lw), lw, -np.inf).max(axis=1)
    st = torch.from_numpy(host).to(DEV)
    for g in _groups_to_check(lw.shape[0]):
        st[g] = P.ops.is_stats(torch.from_numpy(lw[g]).to(DEV), torch.from_numpy(x0[g]).to(DEV), scratch)[:6]
    some = np.isfinite(host[:, 0])      # (a group without a finite log-weight has no maximum to compare)
    assert np.array_equal(_bits(st[:, 0].cpu().numpy()[some]), _bits(host[some, 0]))
    return st.contiguous()


def _case(M, N, J):
    """The inputs of a shape, the device rows and the float64 reference, computed once and shared by the tests (never modified)."""
    key = (M, N, J)
    if key not in _CASES:
        lw, x = _inputs(M, N, J)
        ref, scale = MR.moments_ref(lw, x)
        _CASES[key] = (lw, x, _call(lw, x), ref, scale)
    return _CASES[key]


def _check_rows(got, ref, scale, J, label=''):
    """max lw, count and the pivots exactly; W and sum w^2 to BAR (sums of positive terms: their scale is their value); S and Q to
    BAR of the sum of the absolute values of their terms."""
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 3], ref[:, 3]), label
    assert np.array_equal(got[:, 4:4 + J], ref[:, 4:4 + J]), label
    assert (np.abs(got[:, 1:3] - ref[:, 1:3]) <= BAR * ref[:, 1:3]).all(), label
    err = np.abs(got[:, 4 + J:] - ref[:, 4 + J:])
    bound = BAR * scale[:, 4 + J:]
    print('%s moments: max error / bound = %.3g' % (label, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (label, np.argwhere(~(err <= bound))[:5].tolist())


# ---- 1. the kernel against float64 numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,J', SHAPES)
def test_rows_against_the_float64_restatement(M, N, J):
    lw, x, whole, ref, scale = _case(M, N, J)
    assert whole.shape == (PAD + M + PAD, MR.width(J))
    assert np.isnan(whole[:PAD]).all() and np.isnan(whole[PAD + M:]).all()          # the poison survives
    got = whole[PAD:PAD + M]
    assert np.isfinite(got[:, 1:]).all()            # no NaN of a skipped particle reached a sum (entry 0 is -inf without a weight)
    _check_rows(got, ref, scale, J, str((M, N, J)))
    if M >= 2:            # the group without a finite weight: count 0, sums 0
        assert got[M - 1, 0] == -np.inf and (got[M - 1, 1:4] == 0).all() and (got[M - 1, 4 + J:] == 0).all()
    if M >= 3 and N >= 63:
        assert (got[1, 4:4 + J] == 0).all()         # (its first particle carries NaN: pivot 0)
    # the rows as moments: means and covariances of every group with a weight against a two-pass computation
    from pyprob_amd.distributions import joint_from_moments
    for g in [g for g in _groups_to_check(M) if g < M - 1 or M == 1]:
        j = joint_from_moments(list(range(J)), got[g])
        mean, cov = MR.mean_cov_ref(lw[g], x[:, g])
        sd = np.sqrt(np.diag(cov))
        if int(got[g, 3]) > 1:
            assert (np.abs(j.mean - mean) <= 1e-9 * (np.abs(mean) + sd)).all() and (np.abs(j.cov - cov) <= 1e-8 * np.outer(sd, sd)).all()
        else:
            assert np.array_equal(j.mean, mean) and (j.cov == 0).all()
        assert j.count == int(np.isfinite(lw[g]).sum())


def test_a_non_finite_value_under_a_finite_weight_propagates():
    rng = np.random.default_rng(5)
    lw = rng.normal(0, 1, (1, 500)).astype(np.float32)
    x = rng.normal(0, 1, (2, 1, 500)).astype(np.float32)
    x[1, 0, 77] = np.inf
    got = _call(lw, x)[PAD]
    J = 2
    s, q = got[4 + J:4 + 2 * J], got[4 + 2 * J:]
    assert np.isfinite(got[:4]).all() and np.isfinite(s[0]) and np.isfinite(q[0])      # column 0 and the weights are untouched
    assert not np.isfinite(s[1]) and not np.isfinite(q[1]) and not np.isfinite(q[2])


# ---- 2. bit identity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,J', SHAPES)
def test_bit_identity_of_calls_groups_and_maxima(M, N, J):
    lw, x, whole, _, _ = _case(M, N, J)
    got = whole[PAD:PAD + M]
    assert np.array_equal(_bits(_call(lw, x)[PAD:PAD + M]), _bits(got))              # two identical calls
    st = _stats(lw, x[0])
    with_stats = _call(lw, x, st)
    assert np.isnan(with_stats[:PAD]).all() and np.isnan(with_stats[PAD + M:]).all()
    assert np.array_equal(_bits(with_stats[PAD:PAD + M]), _bits(got))                # the maximum pp_is_stats reduced: the same bits
    for g in _groups_to_check(M):
        one = _call(lw[g:g + 1], x[:, g:g + 1])[PAD]
        assert np.array_equal(_bits(one), _bits(got[g])), (g, np.nonzero(_bits(one) != _bits(got[g]))[0][:5].tolist())
        one = _call(lw[g:g + 1], x[:, g:g + 1], st[g:g + 1].contiguous())[PAD]
        assert np.array_equal(_bits(one), _bits(got[g])), g


# ---- 3. error returns ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_launch_nothing():
    lib = L.load()
    M, N, J = 3, 300, 5
    lw = torch.zeros(M * N, device=DEV)
    cols = [torch.ones(M * N, device=DEV) for _ in range(J)]
    out = torch.full((M, L.PP_IS_MOMENTS_WIDTH(J)), float('nan'), dtype=torch.float64, device=DEV)
    need = lib.pp_is_moments_workspace_bytes(M, N, J)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptrs = (C.c_void_p * 17)(*([c.data_ptr() for c in cols] * 4)[:17])
    holed = (C.c_void_p * J)(*[c.data_ptr() for c in cols])
    holed[4] = None

    def call(lw_p=lw.data_ptr(), cp=C.cast(ptrs, C.c_void_p), j=J, m=M, n_per=N, o=out.data_ptr(), w=ws.data_ptr(), wb=need):
        return lib.pp_is_moments_groups(lw_p, cp, j, m, n_per, None, o, w, wb, L.stream_ptr())
    EINVAL, ENOSPACE = -1, -2
    assert call(lw_p=None) == EINVAL and call(cp=None) == EINVAL and call(o=None) == EINVAL and call(w=None) == EINVAL
    assert call(cp=C.cast(holed, C.c_void_p)) == EINVAL
    assert call(j=0) == EINVAL and call(j=17, wb=2 ** 40) == EINVAL and call(n_per=0) == EINVAL and call(m=-1) == EINVAL
    assert call(m=2 ** 20, n_per=2 ** 11, wb=2 ** 40) == EINVAL
    assert call(wb=need - 1) == ENOSPACE and call(wb=0) == ENOSPACE
    assert call(m=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0                                  # and the accepted call writes every entry
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ---- 4. a narrow posterior far from zero --------------------------------------------------------------------------------------------------
def test_narrow_posterior_far_from_zero():
    """x = float32(1000 + 1e-3 z), two correlated columns, 10^5 particles: var ~ 1e-6 next to x^2 ~ 1e6. Sums about the pivot
    (the group's first value) carry deviations of ~1e-3 and land ~1e-10 of sqrt(var_j var_k) from a float64 two-pass covariance;
    raw second moments E[x_j x_k] - E[x_j] E[x_k] cancel twelve digits and land ~1e-4 .. 1e-3 away even in float64 (1.3e-3 on these
    inputs; printed below, computed in numpy) - four orders and more outside the 1e-8 bar this test sets."""
    from pyprob_amd.distributions import joint_from_moments
    rng = np.random.default_rng(8)
    n = 10 ** 5
    z = rng.normal(size=(2, n))
    z[1] = 0.6 * z[0] + 0.8 * z[1]
    x = (1000.0 + 1e-3 * z).astype(np.float32)[:, None, :]
    lw = rng.normal(0.0, 1.5, (1, n)).astype(np.float32)
    j = joint_from_moments(['x', 'y'], _call(lw, x)[PAD])
    mean, cov = MR.mean_cov_ref(lw[0], x[:, 0])
    sd = np.sqrt(np.diag(cov))
    err = np.abs(j.cov - cov) / np.outer(sd, sd)
    w = np.exp(lw[0].astype(np.float64) - lw[0].max())
    w /= w.sum()
    x64 = x[:, 0].astype(np.float64)
    raw = (w * x64) @ x64.T - np.outer((w * x64).sum(1), (w * x64).sum(1))
    print('narrow posterior: pivot error %.3g, raw-second-moment error %.3g (of sqrt(var_j var_k))'
          % (float(err.max()), float((np.abs(raw - cov) / np.outer(sd, sd)).max())))
    assert (err <= 1e-8).all(), err
    assert (np.abs(j.mean - mean) <= 1e-12 * np.abs(mean)).all()
    assert abs(j.corr[0, 1] - cov[0, 1] / (sd[0] * sd[1])) <= 1e-8 and 0.3 < j.corr[0, 1] < 0.9


# ---- 5 - 8. end to end ----------------------------------------------------------------------------------------------------------------------
SIGMA = math.sqrt(2.0)
_MODEL = []
_POSTS = {}


def _straight_line_model():
    """a ~ Normal(1, sqrt 5) (name='mu'); observe obs0 ~ Normal(a, .); b ~ Normal(a, 0.7); c ~ Uniform(b - 1, b + 1); observe obs1 ~
    Normal(c, .); returns c - the three-statement program of tests/test_gpu_is_batch_multi.py - with an LSTM network (H = 64) whose
    weights are constructed, not trained."""
    if _MODEL:
        return _MODEL[0]
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal, Uniform
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec
    from pyprob_amd.state import TraceMode

    class StraightLine(Model):
        def forward(self):
            a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a', name='mu')
            pyprob.observe(Normal(a, SIGMA), name='obs0')
            b = pyprob.sample(Normal(a, 0.7), address='b')
            c = pyprob.sample(Uniform(b - 1.0, b + 1.0), address='c')
            pyprob.observe(Normal(c, SIGMA), name='obs1')
            return c
    model = StraightLine()
    tr = next(model._trace_generator(trace_mode=TraceMode.PRIOR))
    addrs = [(v.address, v.distribution.name, None) for v in tr.variables_controlled]
    eng = ICEngine(NetSpec(EMB, lstm_dim=64, lstm_depth=1, proposal_mixture_components=10, network='lstm'), device=DEV, seed=2)
    eng.add_addresses(addrs)
    rng = np.random.default_rng(9)
    sd = {k: (v.numpy() * (3.0 if ('lstm' in k or 'proposal' in k) else 1.0)).astype(np.float32) for k, v in eng.state_dict().items()}
    for k in sd:
        if k.endswith('bias') or 'bias_' in k:
            sd[k] = (sd[k] + 0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
    eng.load_state_dict(sd)
    net = InferenceNetworkLSTM(observe_embeddings=EMB, lstm_dim=64, lstm_depth=1, device=DEV)
    net._obs_names = list(EMB)
    net._engine = eng
    net._is = ISRunner(eng)
    net._layers_initialized = True
    model._inference_network = net
    _MODEL.append((model, [a for a, _, _ in addrs]))
    return _MODEL[0]


def _posterior(N):
    if N not in _POSTS:
        model, _ = _straight_line_model()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            _POSTS[N] = model.posterior_results(N, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=13, offset=64)
    return _POSTS[N]


def _log_columns(post):
    return [(a, rec[0]) for entry in post.statement_log for a, rec in entry.items()]


def _joint_against_numpy(j, lw, cols):
    """A JointMoments against the float64 restatement's row for the same particles, entry for entry to the bar of (1) - the mean
    and the covariance are formed from the reference row by the arithmetic the host uses."""
    J = len(cols)
    ref, scale = MR.moments_ref(lw[None], np.stack(cols)[:, None])
    W = ref[0, 1]
    s_ref, s_bar = ref[0, 4 + J:4 + 2 * J] / W, BAR * scale[0, 4 + J:4 + 2 * J] / W
    assert (np.abs(j.mean - (ref[0, 4:4 + J] + s_ref)) <= s_bar + 1e-15 * np.abs(j.mean)).all()
    q_ref, q_bar = np.zeros((J, J)), np.zeros((J, J))
    q_ref[np.triu_indices(J)], q_bar[np.triu_indices(J)] = ref[0, 4 + 2 * J:] / W, BAR * scale[0, 4 + 2 * J:] / W
    q_ref, q_bar = q_ref + np.triu(q_ref, 1).T, q_bar + np.triu(q_bar, 1).T
    s_abs = scale[0, 4 + J:4 + 2 * J] / W
    cov_ref = q_ref - np.outer(s_ref, s_ref)
    # (Q / W to its bar; the product of the two first moments each to its own)
    bound = q_bar + BAR * 2 * np.outer(s_abs, s_abs) + 1e-15 * np.abs(cov_ref)
    assert (np.abs(j.cov - cov_ref) <= bound).all(), (np.abs(j.cov - cov_ref) / bound).max()
    assert j.count == int(np.isfinite(lw).sum()) and abs(j.ess - W * W / ref[0, 2]) <= 1e-10 * j.ess


@pytest.mark.parametrize('N', [300, 4097])
def test_straight_line_program_end_to_end(N):
    """`addresses` are the statement log's keys - the program's full addresses ('a__Normal__1' for address='a'); the address= a
    statement was given and its name= reach the same columns."""
    model, full = _straight_line_model()
    post = _posterior(N)
    assert post.addresses == full and [a.split('__')[0] for a in post.addresses] == ['a', 'b', 'c']
    assert [post._latent(k)[0] for k in ('a', 'b', 'c')] == post.addresses and post._latent('mu')[0] == full[0]
    assert post.statement_names == {'mu': full[0]} and all(r == {a: None} for r, a in zip(post.statement_rows, full))
    mc = post.marginal('c')      # the latent forward() returns: the posterior's own column and statistics
    assert mc._values is post._values and mc._log_weights is post._log_weights
    assert abs(mc.mean - post.mean) <= 1e-10 * abs(post.mean) and abs(mc.variance - post.variance) <= 1e-10 * post.variance
    assert abs(mc.effective_sample_size - post.effective_sample_size) <= 1e-10 * post.effective_sample_size
    ma = post.marginal('a')
    log = _log_columns(post)
    assert ma._values is log[0][1] and ma._log_weights is post._log_weights and ma.length == N and ma._device_backed()
    assert torch.equal(post.marginal('mu')._values, log[0][1])
    with pytest.raises(KeyError, match='b__Normal__1'):
        post.marginal('d')
    lw = post._all_log_weights.cpu().numpy()
    cols = [v.cpu().numpy() for _, v in log]
    j = post.joint()
    assert j.addresses == full and j.mean.shape == (3,) and j.cov.shape == j.corr.shape == (3, 3) and j.stddev.shape == (3,)
    _joint_against_numpy(j, lw, cols)
    # (the call's fused pass takes every weight from an fp32 exponent - relative error ~1e-7 each, csrc/is_kernels.hip - so its mean
    # and variance of the result column sit ~1e-9 from the fp64-exponent moments: 1e-6 of the column's scale is their common ground)
    assert abs(j.mean[2] - post.mean) <= 1e-6 * (abs(post.mean) + post.stddev) and abs(j.cov[2, 2] - post.variance) <= 1e-6 * post.variance
    assert abs(j.mean[0] - ma.mean) <= 1e-10 * (abs(ma.mean) + ma.stddev) and abs(j.cov[0, 0] - ma.variance) <= 1e-8 * ma.variance
    assert (np.abs(j.corr) <= 1 + 1e-9).all() and (np.abs(np.diag(j.corr) - 1) <= 1e-12).all()
    assert (np.abs(j.stddev - np.sqrt(np.diag(j.cov))) == 0).all()
    sub = post.joint(['c', 'mu'])
    assert sub.addresses == [full[2], full[0]]
    _joint_against_numpy(sub, lw, [cols[2], cols[0]])
    # the marginal resamples on the device like the result column does
    r = ma.resample(500, seed=3)
    assert r._device_backed() and r.length == 500 and bool(torch.isin(r._values, ma._values).all())


def test_marsaglia_end_to_end():
    from is_helpers import lockstep_network
    model, net, meta, params = lockstep_network(DEV)
    n = 400
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=3, offset=0)
    log, rows, addrs = post.statement_log, post.statement_rows, post.addresses
    assert len(rows) == len(log) >= 4 and len(addrs) == len(log) and all(set(r) == set(e) for r, e in zip(rows, log))
    assert rows[0][addrs[0]] is None and rows[1][addrs[1]] is None
    x0, y0 = (log[k][addrs[k]][0].cpu().numpy() for k in (0, 1))
    rejected = np.nonzero(x0 * x0 + y0 * y0 >= 1)[0]
    assert 0 < len(rejected) < n
    for k in (2, 3):
        assert np.array_equal(rows[k][addrs[k]].cpu().numpy(), rejected)
    lw = post._all_log_weights.cpu().numpy()
    j = post.joint()
    assert j.addresses == addrs[:2]                  # the addresses every particle executed
    _joint_against_numpy(j, lw, [x0, y0])
    with pytest.raises(ValueError, match=re.escape(addrs[2])):
        post.joint([addrs[0], addrs[2]])
    m = post.marginal(addrs[2])
    x1 = log[2][addrs[2]][0].cpu().numpy()[rejected]
    assert m.length == len(rejected) and np.array_equal(m._values.cpu().numpy(), x1)
    assert np.array_equal(m._log_weights.cpu().numpy(), lw[rejected])
    mean, cov = MR.mean_cov_ref(lw[rejected], x1[None])
    assert abs(m.mean - mean[0]) <= 1e-10 * (abs(mean[0]) + math.sqrt(cov[0, 0])) and abs(m.variance - cov[0, 0]) <= 1e-8 * cov[0, 0]


def test_joint_batch_is_one_operator_call_and_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    model, full = _straight_line_model()
    M, N = 7, 300
    rng = np.random.default_rng(3)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
    assert model._batch_ok is True and len(posts) == M
    count = {'moments': 0}
    op = P.ops.is_moments_groups

    def counted(*a):
        count['moments'] += 1
        return op(*a)
    monkeypatch.setattr(P.ops, 'is_moments_groups', counted, raising=False)
    loop = [p.joint() for p in posts]
    assert count['moments'] == M
    fast = pyprob_amd.joint_batch(posts)
    assert count['moments'] == M + 1 and len(fast) == M                   # ONE operator call for the M groups
    for g, (f, l, p) in enumerate(zip(fast, loop, posts)):
        assert f.addresses == l.addresses == full and f.count == l.count == N
        for name in ('mean', 'cov', 'corr', 'stddev'):
            assert np.array_equal(_bits(getattr(f, name)), _bits(getattr(l, name))), (g, name)
        assert f.ess == l.ess and abs(f.ess - p.effective_sample_size) <= 1e-6 * f.ess       # (fp32-exponent weights: see above)
        assert abs(f.mean[2] - p.mean) <= 1e-6 * (abs(p.mean) + p.stddev)
        cols = [v.cpu().numpy() for _, v in _log_columns(p)]
        _joint_against_numpy(f, p._all_log_weights.cpu().numpy(), cols)
    assert len(set(round(float(f.mean[0]), 3) for f in fast)) == M          # the groups see different observations
    # a subset of the addresses, by name; a shuffled list takes the loop and still matches it
    part = pyprob_amd.joint_batch(posts, ['c', 'mu'])
    assert count['moments'] == M + 2 and all(np.array_equal(q.mean, f.mean[[2, 0]]) for q, f in zip(part, fast))
    before = count['moments']
    mixed = pyprob_amd.joint_batch([posts[i] for i in (2, 0, 1)])
    assert count['moments'] - before == 3
    assert all(np.array_equal(_bits(m.cov), _bits(loop[i].cov)) for m, i in zip(mixed, (2, 0, 1)))


def test_resample_joint_draws_one_index_per_sample():
    post = _posterior(4097)
    _, full = _straight_line_model()
    K = 1000
    draws = post.resample_joint(K, seed=9, offset=17)
    assert set(draws) == set(full) | {'index'}
    idx = draws['index']
    assert idx.dtype == torch.int64 and idx.shape == (K,) and idx.is_cuda and int(idx.min()) >= 0 and int(idx.max()) < 4097
    for a, col in _log_columns(post):
        assert draws[a].shape == (K,) and draws[a].is_cuda and torch.equal(draws[a], col[idx])
    same = post.resample(K, seed=9, offset=17)._values
    assert np.array_equal(draws[full[2]].cpu().numpy().view(np.uint32), same.cpu().numpy().view(np.uint32))
    assert len(torch.unique(idx)) > 1
    only = post.resample_joint(K, ['mu'], seed=9, offset=17)
    assert set(only) == {full[0], 'index'} and torch.equal(only['index'], idx)


def test_an_address_at_two_statement_indices_is_one_latent_over_all_its_particles():
    """`if a > 0: b = sample(...)` before a shared `c = sample(...)`: the statement log, keyed by statement index first, holds 'c' at
    index 2 for the particles that took the branch and at index 1 for the others. marginal('c'), joint() and resample_joint answer
    for ALL of them, checked against numpy over every particle; 2100 particles are more than one tile of the kernel."""
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec

    class SkippingBranch(Model):
        def forward(self):
            a = pyprob.sample(Normal(0.0, 1.0), address='a')
            pyprob.observe(Normal(a, SIGMA), name='obs0')
            if a > 0:
                pyprob.sample(Normal(a, 0.7), address='b')
            c = pyprob.sample(Normal(a, 1.0), address='c')
            pyprob.observe(Normal(c, SIGMA), name='obs1')
            return c
    model = SkippingBranch()
    A, B, Cc = ('{}__Normal__1'.format(a) for a in 'abc')
    eng = ICEngine(NetSpec(EMB, lstm_dim=64, lstm_depth=1, proposal_mixture_components=10, network='lstm'), device=DEV, seed=2)
    eng.add_addresses([(a, 'Normal', None) for a in (A, B, Cc)])
    net = InferenceNetworkLSTM(observe_embeddings=EMB, lstm_dim=64, lstm_depth=1, device=DEV)
    net._obs_names = list(EMB)
    net._engine = eng
    net._is = ISRunner(eng)
    net._layers_initialized = True
    model._inference_network = net
    n = 2100
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 0.5, 'obs1': 0.25}, lock_step=True, seed=11, offset=0)
    log, rows = post.statement_log, post.statement_rows
    assert [sorted(e) for e in log] == [[A], [B, Cc], [Cc]]
    a = log[0][A][0].cpu().numpy()
    took, skipped = np.nonzero(a > 0)[0], np.nonzero(~(a > 0))[0]
    assert 0 < len(took) < n
    assert np.array_equal(rows[1][B].cpu().numpy(), took) and np.array_equal(rows[2][Cc].cpu().numpy(), took)
    assert np.array_equal(rows[1][Cc].cpu().numpy(), skipped)
    c = np.empty(n, np.float32)
    c[skipped], c[took] = log[1][Cc][0].cpu().numpy()[skipped], log[2][Cc][0].cpu().numpy()[took]
    lw = post._all_log_weights.cpu().numpy()
    assert np.isfinite(lw).all() and sorted(post.addresses) == [A, B, Cc]
    mc = post.marginal('c')
    assert mc.length == n and mc._device_backed() and np.array_equal(mc._values.cpu().numpy(), c)
    assert np.array_equal(post._all_values.cpu().numpy(), c)       # 'c' is what forward() returns
    mean, cov = MR.mean_cov_ref(lw, np.stack([a, c]))
    assert abs(mc.mean - mean[1]) <= 1e-10 * (abs(mean[1]) + math.sqrt(cov[1, 1])) and abs(mc.variance - cov[1, 1]) <= 1e-8 * cov[1, 1]
    assert abs(mc.mean - post.mean) <= 1e-6 * (abs(post.mean) + post.stddev)      # (fp32-exponent weights of the call: see above)
    j = post.joint()
    assert j.addresses == [A, Cc]                # every particle executed 'c'; 'b' belongs to the branch
    _joint_against_numpy(j, lw, [a, c])
    _joint_against_numpy(post.joint(['c']), lw, [c])
    with pytest.raises(ValueError, match=re.escape(B)):
        post.joint(['a', 'b'])
    mb = post.marginal('b')
    b = log[1][B][0].cpu().numpy()[took]
    mean_b, cov_b = MR.mean_cov_ref(lw[took], b[None])
    assert mb.length == len(took) and np.array_equal(mb._values.cpu().numpy(), b)
    assert abs(mb.mean - mean_b[0]) <= 1e-10 * (abs(mean_b[0]) + math.sqrt(cov_b[0, 0]))
    draws = post.resample_joint(500, seed=2)
    idx = draws['index'].cpu().numpy()
    assert set(draws) == {A, Cc, 'index'}
    assert np.array_equal(draws[Cc].cpu().numpy(), c[idx]) and np.array_equal(draws[A].cpu().numpy(), a[idx])
    # the merge wrote to none of the log's own tensors
    assert np.array_equal(log[1][Cc][0].cpu().numpy()[skipped], c[skipped]) and np.array_equal(log[2][Cc][0].cpu().numpy()[took], c[took])
