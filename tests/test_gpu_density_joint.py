"""pp_is_gmm_joint_groups (csrc/is_gmm_joint.hip), Empirical.density_estimate_joint and density_estimate_joint_batch on the device.
The operator at the C ABI against a numpy.longdouble restatement of the header's definition (_ref). BOUND per case and per block of
the row (weights, means, covariances, lower bound): 16 times the error of the float64 host route against the same long-double numbers,
never below 64 ulp of fp64 at the block's largest magnitude - the rule of test_gpu_psis.py. PP_GMM_JOINT_ERRORS=<file> appends every
case's device error, host error and bound (profiles/gmm_joint_errors.jsonl). Then bit equality, limits, a degenerate group and the
public route."""
import ctypes as C
import json
import math
import os
import warnings

import numpy as np
import pytest

from helpers import IS_EMB as EMB
from pyprob_amd import lib as L
from pyprob_amd.empirical_host import _host_gmm_joint

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
DEV = 'cuda:0'
REG = 1e-6
LD = np.longdouble
BLOCKS = ('weights', 'means', 'covariances', 'lower_bound')


def _sizes(J, K):
    tri = J * (J + 1) // 2
    return tri, K * (1 + J + tri)


def _data(M, n, J, seed, narrow=False):
    """lw [M, n], x [J, M, n] float32: three planted modes (narrow: at 1000, sd 0.01); 1 % of lw -inf, three NaN, four NaN coordinates."""
    rng = np.random.default_rng(seed)
    comp = rng.integers(0, 3, (M, n))
    mix = rng.normal(0.0, 1.0, (J, J)) * 0.4 + np.eye(J)
    z = np.einsum('jk,kmn->jmn', mix, rng.normal(0.0, 1.0, (J, M, n)))
    x = 1000.0 + 0.03 * comp + 0.01 * z if narrow else 2.5 * comp * (1.0 - 0.2 * np.arange(J))[:, None, None] + 0.6 * z
    lw = rng.normal(0.0, 1.0, (M, n))
    lw[rng.random((M, n)) < 0.01] = -np.inf
    for g in range(M):
        at = rng.choice(n, 7, replace=False)
        lw[g, at[:3]] = np.nan
        x[rng.integers(0, J, 4), g, at[3:]] = np.nan
    return lw.astype(np.float32), x.astype(np.float32)


def _init(lw, x, K, reg=REG):
    """[M, K P]: weights 1 / K, means K counted particles evenly spaced by index, covariances cov / K^(2 / J) + reg I."""
    J, M, n = x.shape
    iu = np.triu_indices(J)
    rows = []
    for g in range(M):
        keep = np.nonzero(np.isfinite(lw[g]) & np.isfinite(x[:, g]).all(0))[0]
        xs = x[:, g, keep].astype(np.float64)
        cov = np.atleast_2d(np.cov(xs)) / K ** (2.0 / J) + reg * np.eye(J)
        mu = xs[:, (np.arange(K) * len(keep)) // K + len(keep) // (2 * K)].T
        rows.append(np.concatenate([np.full(K, 1.0 / K), mu.ravel(), np.tile(cov[iu], K)]))
    return np.stack(rows)


def _call(lw, x, K, init, max_iter, tol, reg=REG, check_every=8):
    """One pp_is_gmm_joint_groups call on host lw [M, n], x [J, M, n]: the rows [M, width] in numpy."""
    lib = L.load()
    J, M, n = x.shape
    tl = torch.from_numpy(np.ascontiguousarray(lw).reshape(-1)).to(DEV)
    cols = [torch.from_numpy(np.ascontiguousarray(c).reshape(-1)).to(DEV) for c in x]
    ti = torch.from_numpy(np.ascontiguousarray(init, np.float64)).to(DEV)
    out = torch.full((M, L.PP_IS_GMM_JOINT_WIDTH(J, K)), float('nan'), dtype=torch.float64, device=DEV)
    need = lib.pp_is_gmm_joint_workspace_bytes(M, n, J, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptrs = (C.c_void_p * J)(*[c.data_ptr() for c in cols])
    L.check(lib.pp_is_gmm_joint_groups(tl.data_ptr(), C.cast(ptrs, C.c_void_p), J, K, M, n, None, ti.data_ptr(), max_iter, tol,
                                       reg, check_every, out.data_ptr(), ws.data_ptr(), need, L.stream_ptr()), 'pp_is_gmm_joint_groups')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ref(lw, x, init, K, max_iter, tol, reg):
    """The header's definition for one particle set in numpy.longdouble (forward substitution with the factor, not a product with
    its inverse): (the parameters of the row, lower bound, n_iter)."""
    J = x.shape[0]
    tri, off = _sizes(J, K)
    fin = np.isfinite(lw)
    keep = fin & np.isfinite(x).all(0)
    w, xs = np.exp(lw[keep].astype(LD) - LD(lw[fin].max())), x[:, keep].astype(LD)
    init = np.asarray(init, np.float64).astype(LD)
    pi, mu = init[:K].copy(), init[K:K + K * J].reshape(K, J).copy()
    cov = np.zeros((K, J, J), LD)
    iu = np.triu_indices(J)
    cov[:, iu[0], iu[1]] = init[K + K * J:].reshape(K, tri)
    log_2pi = np.log(LD(8) * np.arctan(LD(1)))
    W, before, lb, n_iter = w.sum(), -np.inf, None, 0
    for t in range(1, max_iter + 1):
        ell = np.empty((K, len(w)), LD)
        for k in range(K):
            Lk = np.zeros((J, J), LD)
            for j in range(J):
                for m in range(j + 1):
                    s = cov[k, m, j] - (Lk[j, :m] * Lk[m, :m]).sum()
                    Lk[j, m] = s / Lk[m, m] if m < j else np.sqrt(s)
            z = np.empty_like(xs)
            for j in range(J):
                z[j] = (xs[j] - mu[k, j] - (Lk[j, :j, None] * z[:j]).sum(0)) / Lk[j, j]
            ell[k] = np.log(pi[k]) - LD(J) / 2 * log_2pi - np.log(np.diag(Lk)).sum() - (z * z).sum(0) / 2
        peak = ell.max(0)
        Li = peak + np.log(np.exp(ell - peak).sum(0))
        lb = (w * Li).sum() / W
        N = np.empty(K, LD)
        new_mu, new_cov = np.empty_like(mu), np.zeros_like(cov)
        for k in range(K):
            r = w * np.exp(ell[k] - Li)
            N[k] = r.sum() + LD(10.0 * np.finfo(np.float64).eps)
            d = xs - mu[k][:, None]
            s = (r * d).sum(1) / N[k]
            new_mu[k] = mu[k] + s
            new_cov[k] = (r * d) @ d.T / N[k] - np.outer(s, s) + LD(reg) * np.eye(J)
        pi, mu, cov, n_iter = N / N.sum(), new_mu, new_cov, t
        if abs(lb - before) < tol:
            break
        before = lb
    return np.concatenate([pi, mu.ravel(), cov[:, iu[0], iu[1]].ravel()]), lb, n_iter


def _errors(label, got, host, lw, x, init, K, max_iter, tol=0.0, reg=REG):
    """Per group: the device row `got` and the host row against _ref, block by block; asserts the bound and records the figures."""
    J, M, n = x.shape
    tri, off = _sizes(J, K)
    cuts = {'weights': slice(0, K), 'means': slice(K, K + K * J), 'covariances': slice(K + K * J, off), 'lower_bound': slice(off, off + 1)}
    rec = dict(case=label, J=J, K=K, M=M, n_per=n, max_iter=max_iter, tol=tol)
    bounds = []
    for g in range(M):
        par, lb, n_iter = _ref(lw[g], x[:, g], init[g], K, max_iter, tol, reg)
        want = np.concatenate([par, [lb]])
        assert got[g, off + 1] == host[g, off + 1] == n_iter and got[g, off + 3] == 0 and got[g, off + 5] == host[g, off + 5]
        for name in BLOCKS:
            c = cuts[name]
            err, e64 = np.abs(got[g, c].astype(LD) - want[c]).max(), np.abs(host[g, c].astype(LD) - want[c]).max()
            bound = max(16 * e64, 64 * LD(np.spacing(np.float64(np.abs(want[c]).max()))))
            ulp = float(np.spacing(np.float64(np.abs(want[c]).max())))
            for key, v in (('err', err), ('host_err', e64), ('bound', bound)):
                rec['%s_%s_ulp' % (name, key)] = max(rec.get('%s_%s_ulp' % (name, key), 0.0), float(v) / ulp)
            bounds.append((g, name, float(err), float(bound)))
    print('gmm joint', json.dumps(rec))
    path = os.environ.get('PP_GMM_JOINT_ERRORS')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')
    assert all(err <= bound for _, _, err, bound in bounds), [b for b in bounds if b[2] > b[3]]
    return bounds


def _host(lw, x, init, K, max_iter, tol, reg=REG):
    return np.stack([_host_gmm_joint(lw[g], x[:, g], init[g], K, max_iter, tol, reg) for g in range(lw.shape[0])])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize('M,n', [(1, 300), (3, 2049)])
@pytest.mark.parametrize('K', [1, 3, 16])
@pytest.mark.parametrize('J', [1, 2, 5, 8])
def test_operator_against_the_long_double_restatement(J, K, M, n):
    lw, x = _data(M, n, J, 1000 * J + 10 * K + M)
    init = _init(lw, x, K)
    got, host = _call(lw, x, K, init, 4, 0.0), _host(lw, x, init, K, 4, 0.0)
    bounds = _errors('modes', got, host, lw, x, init, K, 4)
    off = _sizes(J, K)[1]
    assert np.isfinite(got).all() and (got[:, off + 2] == 0).all() and np.array_equal(got[:, off + 6], host[:, off + 6])
    assert np.abs(got[:, off + 4] / host[:, off + 4] - 1).max() <= 1e-13
    if J == 1:      # pp_is_gmm_groups on the same particles (its only way to skip a NaN value is a log-weight of -inf)
        from pyprob_amd import ops as P
        masked = np.where(np.isfinite(x[0]), lw, -np.inf).astype(np.float32)
        one = P.ops.is_gmm_groups(torch.from_numpy(masked.reshape(-1)).to(DEV), torch.from_numpy(x[0].reshape(-1)).to(DEV), K, n, None,
                                  torch.from_numpy(init).to(DEV), 4, 0.0, REG).cpu().numpy()
        for (g, name, _, bound), c in zip(bounds, [slice(0, K), slice(K, 2 * K), slice(2 * K, 3 * K), slice(3 * K, 3 * K + 1)] * M):
            assert np.abs(one[g, c] - got[g, c]).max() <= bound, (g, name)


def test_operator_on_a_narrow_posterior_far_from_zero():
    J, K, M, n = 2, 3, 1, 2049
    lw, x = _data(M, n, J, 7, narrow=True)
    init = _init(lw, x, K, 1e-9)
    got, host = _call(lw, x, K, init, 4, 0.0, 1e-9), _host(lw, x, init, K, 4, 0.0, 1e-9)
    _errors('narrow at 1000', got, host, lw, x, init, K, 4, reg=1e-9)
    assert (np.abs(got[0, K:K + K * J] - 1000.0) < 0.2).all()


def test_calls_groups_and_check_every_give_the_same_bits():
    J, K, M, n = 2, 3, 3, 2049
    lw, x = _data(M, n, J, 41)
    x[:, 1] = (x[:, 1] * 2.0).astype(np.float32)                   # (well separated modes: this group converges first)
    init = _init(lw, x, K)
    big = _call(lw, x, K, init, 60, 1e-3, check_every=8)
    off = _sizes(J, K)[1]
    assert np.array_equal(_bits(big), _bits(_call(lw, x, K, init, 60, 1e-3, check_every=8)))
    assert np.array_equal(_bits(big), _bits(_call(lw, x, K, init, 60, 1e-3, check_every=1)))
    for g in range(M):      # a group that converged early keeps its row while the others go on
        assert np.array_equal(_bits(big[g]), _bits(_call(lw[g:g + 1], x[:, g:g + 1], K, init[g:g + 1], 60, 1e-3)[0])), g
    iters = big[:, off + 1]
    print('n_iter of the groups', iters)
    assert (big[:, off + 2] == 1).all() and len(np.unique(iters)) > 1 and iters.max() - iters.min() >= 2


def test_limits_are_rejected_without_a_launch():
    lib = L.load()
    n = 300
    lw = torch.zeros(n, device=DEV)
    cols = [torch.ones(n, device=DEV) for _ in range(9)]
    ptrs = (C.c_void_p * 9)(*[c.data_ptr() for c in cols])
    init = torch.ones(17 * 55, dtype=torch.float64, device=DEV)
    out = torch.full((17 * 55 + 7,), float('nan'), dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)

    def call(j, k):
        return lib.pp_is_gmm_joint_groups(lw.data_ptr(), C.cast(ptrs, C.c_void_p), j, k, 1, n, None, init.data_ptr(), 4, 0.0, REG, 8,
                                          out.data_ptr(), ws.data_ptr(), 1 << 22, L.stream_ptr())
    assert call(9, 3) == -1 and call(2, 17) == -1 and call(0, 3) == -1 and call(2, 0) == -1      # PP_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_a_degenerate_group_freezes_and_leaves_the_others_alone():
    J, K, M, n = 2, 2, 3, 300
    lw, x = _data(M, n, J, 51)
    x[:, 1] = 4.25                                                   # identical particles: with reg_covar = 0 the covariance is 0
    init = _init(lw, x, K, reg=1e-3)
    iu = np.triu_indices(J)
    init[1] = np.concatenate([[0.5, 0.5], np.full(K * J, 4.25), np.tile(np.eye(J)[iu], K)])
    got = _call(lw, x, K, init, 9, 1e-3, reg=0.0)
    off = _sizes(J, K)[1]
    assert np.array_equal(got[1, :off], init[1]) and got[1, off + 1:off + 4].tolist() == [1.0, 0.0, 1.0] and np.isfinite(got[1]).all()
    for g in (0, 2):
        assert np.isfinite(got[g]).all() and got[g, off + 3] == 0 and got[g, off + 1] > 1
        assert np.array_equal(_bits(got[g]), _bits(_call(lw[g:g + 1], x[:, g:g + 1], K, init[g:g + 1], 9, 1e-3, reg=0.0)[0]))


_MODEL = []


def _two_statement_model():
    """a ~ Normal(1, sqrt 5); observe obs0 ~ Normal(a, .); b ~ Normal(a, 0.7) - its prior depends on the first draw -; observe
    obs1 ~ Normal(b, .); an LSTM network (H = 64) whose weights are constructed, not trained."""
    if _MODEL:
        return _MODEL[0]
    import pyprob_amd as pyprob
    from pyprob_amd.distributions import Normal
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec

    class TwoStatements(pyprob.Model):
        def forward(self):
            a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a')
            pyprob.observe(Normal(a, math.sqrt(2.0)), name='obs0')
            b = pyprob.sample(Normal(a, 0.7), address='b')
            pyprob.observe(Normal(b, math.sqrt(2.0)), name='obs1')
            return b
    model = TwoStatements()
    tr = next(model._trace_generator(trace_mode=pyprob.TraceMode.PRIOR))
    eng = ICEngine(NetSpec(EMB, lstm_dim=64, lstm_depth=1, proposal_mixture_components=10, network='lstm'), device=DEV, seed=2)
    eng.add_addresses([(v.address, v.distribution.name, None) for v in tr.variables_controlled])
    eng.load_state_dict({k: (v.numpy() * (3.0 if ('lstm' in k or 'proposal' in k) else 1.0)).astype(np.float32)
                         for k, v in eng.state_dict().items()})
    net = InferenceNetworkLSTM(observe_embeddings=EMB, lstm_dim=64, lstm_depth=1, device=DEV)
    net._obs_names, net._engine, net._is, net._layers_initialized = list(EMB), eng, ISRunner(eng), True
    model._inference_network = net
    _MODEL.append(model)
    return model


def _fit_row(f):
    return np.concatenate([f.weights, f.means.ravel(), f.covariances.ravel(), [f.lower_bound, f.n_iter, f.converged, f.degenerate, f.count]])


def test_density_estimate_joint_on_a_lock_step_posterior():
    from pyprob_amd.distributions import Mixture
    from pyprob_amd.state import InferenceEngine
    model, N, K, J = _two_statement_model(), 4097, 3, 2
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(N, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe={'obs0': 2.0, 'obs1': 1.5},
                                       lock_step=True, seed=13, offset=64)
        fit = post.density_estimate_joint(K)
        assert np.array_equal(_bits(_fit_row(fit)), _bits(_fit_row(post.density_estimate_joint(K))))      # deterministic
    lw = post._all_lw().cpu().numpy()[None]
    x = np.stack([rec[0].cpu().numpy() for entry in post.statement_log for rec in entry.values()])[:, None]
    assert x.shape == (J, 1, N) and fit.count == N and len(fit.addresses) == J and not fit.degenerate
    # the start, restated: the particles at the weighted quantiles (k + 1/2) / K of the first address, joint().cov / K^(2 / J) + reg I
    w = np.exp(lw[0].astype(np.float64) - lw[0].max())
    order = np.argsort(x[0, 0], kind='stable')
    cum = np.cumsum(w[order])
    at = order[np.searchsorted(cum, (np.arange(K) + 0.5) / K * cum[-1])]
    cov0 = post.joint().cov / K ** (2.0 / J) + REG * np.eye(J)
    init = np.concatenate([np.full(K, 1.0 / K), x[:, 0, at].T.ravel().astype(np.float64), np.tile(cov0[np.triu_indices(J)], K)])[None]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        given = post.density_estimate_joint(K, means_init=x[:, 0, at].T, covariances_init=[cov0] * K)
    assert np.array_equal(_bits(_fit_row(given)), _bits(_fit_row(fit)))                                      # the default start IS this one
    off = _sizes(J, K)[1]
    host = _host(lw, x, init, K, 100, 1e-3)
    got = np.concatenate([fit.weights, fit.means.ravel(), fit.covariances[:, np.triu_indices(J)[0], np.triu_indices(J)[1]].ravel(),
                          [fit.lower_bound, fit.n_iter, fit.converged, fit.degenerate, host[0, off + 4], fit.count, host[0, off + 6]]])[None]
    _errors('public route', got, host, lw, x, init, K, 100, tol=1e-3)
    m = fit.marginal('a')
    assert isinstance(m, Mixture) and isinstance(fit.marginal(fit.addresses[1]), Mixture)
    assert np.isfinite(fit.log_prob(fit.sample(5, seed=1))).all()


def test_density_estimate_joint_batch_is_one_operator_call_and_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    model, M, N, K = _two_statement_model(), 3, 300, 2
    rng = np.random.default_rng(3)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    count, real = [0], P.ops.is_gmm_joint_groups

    def counted(*a):
        count[0] += 1
        return real(*a)
    monkeypatch.setattr(P.ops, 'is_gmm_joint_groups', counted, raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
        assert model._batch_ok is True and len(posts) == M
        loop = [p.density_estimate_joint(K) for p in posts]
        assert count[0] == M
        fast = pyprob_amd.density_estimate_joint_batch(posts, K)
    assert count[0] == M + 1 and len(fast) == M
    assert all(np.array_equal(_bits(_fit_row(a)), _bits(_fit_row(b))) and a.count == N for a, b in zip(fast, loop))
    assert len({round(float(f.means[0, 0]), 3) for f in fast}) == M          # the groups see different observations
