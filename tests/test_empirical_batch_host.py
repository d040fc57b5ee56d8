"""The *_batch functions of pyprob_amd/empirical_batch.py on the CPU, through the CPU doubles of the operators: the M groups of one
batched execution in order take the fast path - ONE call of each operator, not M - and give the loop's result bit for bit, for the
value forward() returned and for address= a second logged column; every list that is not that (reversed, a strict sub-list, one group
twice, a member without _batch, a member after add(), everything under PP_EMPIRICAL_DEVICE=0) takes the loop and gives the loop's
result or raises what the loop raises. resample_batch's fast path needs a runner (tests/test_gpu_resample.py): here its loop.
M = 3 groups of N = 70 particles, one -inf log-weight in group 1, two logged columns."""
import os
import warnings

import numpy as np
import pytest

import gmm_ref as G
import histogram_ref as H
import interval_ref as I
import moments_ref as MR
import order_stats_ref as R
import psis_ref as PR
import resample_ref as RR
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from is_helpers import _batch_of
from test_joint_moments_host import _register_cpu_double

torch = pytest.importorskip('torch')

M, N = 3, 70
Y = 'y__Normal__2'
COUNTERS = (G.calls, H.calls, I.calls, MR.calls, R.calls, PR.calls, RR.calls)
_rng = np.random.default_rng(63)
PTS = _rng.normal(0, 2, (M, 4))


@pytest.fixture
def device_style(monkeypatch):
    """Empirical._device_backed without its is_cuda clauses: a from_device Empirical over CPU tensors takes the device route, whose
    operators are the CPU doubles."""
    from pyprob_amd.distributions import Empirical
    for ref in (G, H, I, R, PR, RR):
        ref.register_cpu_doubles()
    _register_cpu_double()

    def backed(self):
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.dtype == torch.float32 and
                lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and v.numel() == lw.numel() and v.numel() > 0 and
                v.is_contiguous() and lw.is_contiguous() and os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')
    monkeypatch.setattr(Empirical, '_device_backed', backed)


def _posts():
    """A fresh batch (add() changes its member): (posteriors, the group index of each)."""
    rng = np.random.default_rng(7)
    x = rng.normal(0, 2, M * N).astype(np.float32)
    y = (0.5 * x + rng.integers(-2, 3, M * N)).astype(np.float32)             # (ties among the values)
    lw = (-0.5 * np.log(1.0 - rng.random(M * N))).astype(np.float32)          # (weights U^-1/2: a Pareto tail psis can fit)
    lw[N + 3] = -np.inf
    return _batch_of(torch.from_numpy(x), torch.from_numpy(lw), M, N, second=torch.from_numpy(y)), list(range(M))


def _t(p, a):
    return p if a is None else p.marginal(a)


def _arrays(*parts):
    return [np.ascontiguousarray(np.asarray(a, np.float64)) for a in parts]


def _hist_key(hs):
    return [a for h in hs for a in _arrays(h.edges, h.mass, h.count, h.density, [h.below, h.above, h.nan, h.particles])]


def _joint_key(js):
    return [a for j in js for a in _arrays(j.mean, j.cov, j.corr, j.stddev, [j.ess, j.count])] + [list(j.addresses) for j in js]


def _psis_key(ps):
    return [a for p in ps for a in (p._log_weights.numpy() if torch.is_tensor(p._log_weights) else np.asarray(p._log_weights),
                                    *_arrays([p.fit.khat, p.fit.sigma, p.fit.tail, p.fit.grid, p.fit.log_cutoff, p.fit.count,
                                              p.fit.ess_before, p.fit.ess_after, p.length]))] + [p.metadata['op'] for p in ps]


def _mix_key(ms):
    return [a for m in ms for a in _arrays(m.fit.weights, m.fit.means, m.fit.stddevs,
                                           [m.fit.lower_bound, m.fit.n_iter, m.fit.converged, m.fit.count])]


def _values_key(ps):
    return [p._values.numpy() if torch.is_tensor(p._values) else np.asarray([float(v) for v in p._values]) for p in ps]


def _array_key(a):
    return [np.ascontiguousarray(a)]


def _cases():
    """name: (the batch call, the loop over the members, the operator every member's call runs once, the key of a result). Both
    calls take (posteriors, address, the group index of each member)."""
    import pyprob_amd.distributions as D
    qs, levels = [0.05, 0.5, 0.95], [0.5, 0.9]
    return {
        'histogram_batch': (lambda ps, a, i: D.histogram_batch(ps, 16, None, a),
                            lambda ps, a, i: [_t(p, a).histogram(16, None) for p in ps], (H.calls, 'is_hist_groups'), _hist_key),
        'joint_batch': (lambda ps, a, i: D.joint_batch(ps), lambda ps, a, i: [p.joint() for p in ps],
                        (MR.calls, 'is_moments_groups'), _joint_key),
        'quantile_batch': (lambda ps, a, i: D.quantile_batch(ps, qs, a),
                           lambda ps, a, i: np.stack([_t(p, a).quantile(qs) for p in ps]), (R.calls, 'is_quantile_groups'),
                           _array_key),
        'hpd_batch': (lambda ps, a, i: D.hpd_batch(ps, levels, a),
                      lambda ps, a, i: np.stack([_t(p, a).hpd_interval(levels) for p in ps]), (I.calls, 'is_hpd_groups'),
                      _array_key),
        'cdf_batch': (lambda ps, a, i: D.cdf_batch(ps, PTS[i], a),
                      lambda ps, a, i: np.stack([_t(p, a).cdf(PTS[g]) for g, p in zip(i, ps)]), (I.calls, 'is_ecdf_groups'),
                      _array_key),
        'pareto_k_batch': (lambda ps, a, i: D.pareto_k_batch(ps), lambda ps, a, i: np.array([p.pareto_k() for p in ps], np.float64),
                           (PR.calls, 'is_psis_groups'), _array_key),
        'psis_batch': (lambda ps, a, i: D.psis_batch(ps), lambda ps, a, i: [p.psis() for p in ps], (PR.calls, 'is_psis_groups'),
                       _psis_key),
        'density_estimate_batch': (lambda ps, a, i: D.density_estimate_batch(ps, 2, a),
                                   lambda ps, a, i: [_t(p, a).density_estimate(2) for p in ps], (G.calls, 'is_gmm_groups'),
                                   _mix_key),
        'resample_batch': (lambda ps, a, i: D.resample_batch(ps, 9, seed=5, offset=3),
                           lambda ps, a, i: [p.resample(9, seed=5, offset=3 + 9 * g) for g, p in enumerate(ps)],
                           (RR.calls, 'is_resample_groups'), _values_key),
    }


FAST = ('histogram_batch', 'joint_batch', 'quantile_batch', 'hpd_batch', 'cdf_batch', 'pareto_k_batch', 'psis_batch',
        'density_estimate_batch')
ALL = FAST + ('resample_batch',)
TAKES_ADDRESS = ('histogram_batch', 'quantile_batch', 'hpd_batch', 'cdf_batch', 'density_estimate_batch')


def _with_addresses(names):
    return [(n, None) for n in names] + [(n, Y) for n in names if n in TAKES_ADDRESS]


# what each fast path calls ONCE for the whole list (counters that are not named stay 0)
FAST_CALLS = {
    'histogram_batch': {'is_extent_groups': 1, 'is_hist_groups': 1},
    'joint_batch': {'is_moments_groups': 1},
    'quantile_batch': {'is_sort_groups': 1, 'is_cdf_groups': 1, 'is_quantile_groups': 1},
    'hpd_batch': {'is_sort_groups': 1, 'is_cdf_groups': 1, 'is_hpd_groups': 1},
    'cdf_batch': {'is_sort_groups': 1, 'is_cdf_groups': 1, 'is_ecdf_groups': 1},
    'pareto_k_batch': {'is_sort_groups': 1, 'is_psis_groups': 1},
    'psis_batch': {'is_sort_groups': 1, 'is_psis_groups': 1},
    'density_estimate_batch': {'is_sort_groups': 1, 'is_cdf_groups': 1, 'is_quantile_groups': 1, 'is_gmm_groups': 1},
}


def _reset():
    for c in COUNTERS:
        for k in c:
            c[k] = 0


def _called():
    return {k: v for c in COUNTERS for k, v in c.items() if v}


def _outcome(call, key, *args):
    """('ok', the key of the result) or ('raises', the exception's type): a list the loop cannot serve fails alike in the batch call."""
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            return 'ok', key(call(*args))
        except (AttributeError, ValueError, RuntimeError) as e:
            return 'raises', type(e)


def _same(a, b):
    if a[0] != b[0] or a[0] == 'raises':
        return a == b
    return len(a[1]) == len(b[1]) and all(
        (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y
        for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize('name,address', _with_addresses(FAST))
def test_the_groups_in_order_take_one_operator_call_and_equal_the_loop(device_style, name, address):
    batch, loop, _, key = _cases()[name]
    posts, idx = _posts()
    want = _outcome(loop, key, posts, address, idx)
    _reset()
    got = _outcome(batch, key, posts, address, idx)
    assert _called() == FAST_CALLS[name]
    assert want[0] == 'ok' and _same(got, want)


def _reversed(posts, idx):
    return posts[::-1], idx[::-1]


def _sub_list(posts, idx):
    return posts[:2], idx[:2]


def _one_group_twice(posts, idx):
    return [posts[0], posts[1], posts[1]], [idx[0], idx[1], idx[1]]


def _member_without_batch(posts, idx):
    from pyprob_amd.distributions import Empirical
    p = posts[1]
    q = Empirical.from_device(p._values, p._log_weights, None)
    q.statement_log, q._statement_rows_raw, q.statement_names = p.statement_log, p._statement_rows_raw, p.statement_names
    return [posts[0], q, posts[2]], idx


def _member_after_add(posts, idx):
    posts[0].add(0.25, -1.0)
    posts[0].finalize()
    return posts, idx


def _in_order(posts, idx):
    return posts, idx


# (the list, how many members' calls still reach the device operator)
OTHER_LISTS = {'reversed': (_reversed, 3), 'sub_list': (_sub_list, 2), 'one_group_twice': (_one_group_twice, 3),
               'member_without_batch': (_member_without_batch, 3), 'member_after_add': (_member_after_add, 2),
               'host_route': (_in_order, 0)}


@pytest.mark.parametrize('other', sorted(OTHER_LISTS))
@pytest.mark.parametrize('name,address', _with_addresses(ALL))
def test_every_other_list_takes_the_loop_and_gives_its_result(device_style, monkeypatch, name, other, address):
    batch, loop, (counter, op), key = _cases()[name]
    build, members_on_device = OTHER_LISTS[other]
    posts, idx = build(*_posts())
    if other == 'host_route':
        monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    want = _outcome(loop, key, posts, address, idx)
    _reset()
    got = _outcome(batch, key, posts, address, idx)
    assert _same(got, want)
    # (what raises does so at the first member the loop asks - no operator ran, where the fast path would have run one)
    assert counter[op] == (members_on_device if got[0] == 'ok' else 0)


def test_resample_batch_without_a_runner_is_the_loop(device_style):
    """The groups in order, but no _batch_runner: the loop, one draw call per member, under the key and offsets of its docstring."""
    batch, loop, (counter, op), key = _cases()['resample_batch']
    posts, idx = _posts()
    want = _outcome(loop, key, posts, None, idx)
    _reset()
    got = _outcome(batch, key, posts, None, idx)
    assert want[0] == 'ok' and _same(got, want) and counter[op] == M
