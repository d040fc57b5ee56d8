"""pp_is_twosample_groups (csrc/is_twosample.hip) against a plain restatement of its two walks, on the READ-BACK output of the device
sort and cumulative weights (pinned by tests/test_gpu_order_stats.py). ks, ks_location and the position of the maximum equal the float64
restatement bit for bit, the counts are exact. wasserstein1, wasserstein2 and energy go against the restatement in numpy.longdouble:
per case 16 times the error the float64 restatement itself shows (it adds the same terms in merged order), never below 64 ulp of fp64;
PP_TWOSAMPLE_ERRORS=<file> appends the worst figures per case (profiles/twosample_errors.jsonl). End to end on the straight-line
program at H = 64 of tests/test_gpu_joint_moments.py."""
import json
import os
import warnings

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_CASES = {}


def _lw(rng, n):
    return (-1.5 * rng.random(n)).astype(np.float32)


def _normals(rng, na, nb):
    return [_lw(rng, na), rng.normal(0.0, 1.0, na), _lw(rng, nb), rng.normal(0.3, 1.2, nb)]


def _interleaved(rng):                   # a = 0, 2, 4 ..., b = 1, 3, 5 ...: alternating across the tile boundary at 2048
    k = np.arange(1500.0)
    return _lw(rng, 1500), rng.permutation(2.0 * k), _lw(rng, 1500), rng.permutation(2.0 * k + 1.0)


def _not_counted(rng):                   # -inf log-weights and NaN values: ca < n_per on both sides
    lw_a, x_a, lw_b, x_b = _normals(rng, 1700, 900)
    lw_a[rng.random(1700) < 0.3], x_a[rng.random(1700) < 0.1], lw_b[::7], x_b[5::11] = -np.inf, np.nan, -np.inf, np.nan
    return lw_a, x_a, lw_b, x_b


def _underflow(rng):                     # weights that are exactly 0 in fp64 between the others
    lw_a, x_a, lw_b, x_b = _normals(rng, 1300, 1100)
    lw_a[rng.random(1300) < 0.5] = -3000.0
    lw_b[1::2] -= 2500.0
    return lw_a, x_a, lw_b, x_b


def _infinite(rng):                      # +-inf values under finite weights, matched and unmatched
    lw_a, x_a, lw_b, x_b = _normals(rng, 40, 50)
    x_a[[3, 17]], x_a[[5, 6]], x_b[[1, 2, 30]] = -np.inf, np.inf, np.inf
    return lw_a, x_a, lw_b, x_b


def _three_groups(rng):                  # M = 3 with counts of their own; group 1 has nothing counted on side a
    lw_a, x_a, lw_b, x_b = (t.reshape(3, -1) for t in _normals(rng, 3 * 600, 3 * 2500))
    lw_a[0, 100:], lw_a[1], lw_b[1, ::3], x_b[2, :40] = -np.inf, -np.inf, -np.inf, np.nan
    return lw_a, x_a, lw_b, x_b


CASES = {'1+1': lambda rng: (np.zeros(1), [0.5], np.zeros(1), [1.5]), '1+5': lambda rng: _normals(rng, 1, 5),
         'merged 2048': lambda rng: _normals(rng, 1000, 1048), 'merged 2049': lambda rng: _normals(rng, 1000, 1049),
         # every a below every b: tiles that hold one side only
         'disjoint 2048+2048': lambda rng: (_lw(rng, 2048), rng.random(2048), _lw(rng, 2048), 2.0 + rng.random(2048)),
         'interleaved': _interleaved,
         'five values': lambda rng: (_lw(rng, 3000), rng.integers(0, 5, 3000), _lw(rng, 2500), rng.integers(0, 5, 2500)),
         # one run of ties across four tile boundaries
         'identical 5000+5000': lambda rng: (_lw(rng, 5000), np.full(5000, 1.25), _lw(rng, 5000), np.full(5000, 1.25)),
         'not counted': _not_counted, 'underflow': _underflow, 'infinite values': _infinite, 'three groups': _three_groups}


def _merge(ka, kb):
    """The stable merge of two ascending lists, A before B on ties: per merged element (from A?, i, j), the numbers consumed from
    each side BEFORE it."""
    i = j = 0
    out = []
    while i < len(ka) or j < len(kb):
        from_a = i < len(ka) and (j >= len(kb) or ka[i] <= kb[j])
        out.append((from_a, i, j))
        i, j = i + from_a, j + (not from_a)
    m = np.array(out, np.int64)
    return m[:, 0].astype(bool), m[:, 1], m[:, 2]


def _total(terms, real):
    return np.cumsum(terms.astype(real))[-1] if terms.size else real(0)


def _walks(a, wa, b, wb, real):
    """The two walks of include/pyprob_amd.h on the counted sorted values a, b (float32) and their cumulative weights wa, wb (float64):
    (ks, ks_location, position - float64 by definition; wasserstein1, wasserstein2, energy - products and sums in `real`)."""
    ca, cb = len(a), len(b)
    if ca == 0 or cb == 0 or not (0 < wa[-1] < np.inf and 0 < wb[-1] < np.inf):
        return (np.nan,) * 6
    ua, ub = wa / wa[-1], wb / wb[-1]
    with np.errstate(invalid='ignore', over='ignore'):
        from_a, i, j = _merge(a.tolist(), b.tolist())
        z = np.where(from_a, a[np.minimum(i, ca - 1)], b[np.minimum(j, cb - 1)])
        i, j = i + from_a, j + ~from_a
        D = np.where(i > 0, ua[np.maximum(i, 1) - 1], 0.0) - np.where(j > 0, ub[np.maximum(j, 1) - 1], 0.0)
        step = np.append(z[1:] > z[:-1], False)
        end = step.copy()
        end[-1] = True
        k = int(np.argmax(np.where(end, np.abs(D), -1.0)))
        t = step & (D != 0)
        gap = np.append(z[1:], z[-1])[t].astype(real) - z[t].astype(real)
        w1 = _total(np.abs(D[t]).astype(real) * gap, real)
        energy = 2 * _total(D[t].astype(real) ** 2 * gap, real)
        from_a, i, j = _merge(ua.tolist(), ub.tolist())
        u = np.where(from_a, ua[np.minimum(i, ca - 1)], ub[np.minimum(j, cb - 1)])
        prev = np.concatenate([[0.0], u[:-1]])
        x, y = a[np.minimum(i, ca - 1)].astype(real), b[np.minimum(j, cb - 1)].astype(real)
        d = np.where(x == y, real(0), x - y)
        wide = u > prev
        w2 = np.sqrt(_total((u.astype(real) - prev.astype(real))[wide] * d[wide] ** 2, real))
    return abs(D[k]), np.float64(z[k]), float(k), w1, w2, energy


def _sorted_side(lw, x):
    """(the device sort of M groups as the operator takes it, its read-back: per group the counted values and cumulative weights)."""
    from pyprob_amd import ops as P
    M, n = lw.shape
    d_lw, d_x = (torch.from_numpy(np.ascontiguousarray(t, np.float32).reshape(-1)).to(DEV) for t in (lw, x))
    value, ls, _, counted = P.ops.is_sort_groups(d_lw, d_x, n, None)
    cdf, c = P.ops.is_cdf_groups(ls, n, None), counted.cpu().numpy()[:, 0]
    v, w = value.cpu().numpy().reshape(M, n), cdf.cpu().numpy().reshape(M, n)
    return (value, cdf, counted, n), [(v[g, :c[g]], w[g, :c[g]]) for g in range(M)]


def _op(sa, sb):
    from pyprob_amd import ops as P
    return P.ops.is_twosample_groups(sa[0], sa[1], sa[2], sa[3], sb[0], sb[1], sb[2], sb[3]).cpu().numpy()


def _case(name):
    """The inputs, the device sort and its read-back, the device call and the two restatements of a case: computed once, never
    modified."""
    if name not in _CASES:
        rng = np.random.default_rng(sorted(CASES).index(name))
        lw_a, x_a, lw_b, x_b = (np.atleast_2d(np.asarray(t, np.float32)) for t in CASES[name](rng))
        (sa, ha), (sb, hb) = _sorted_side(lw_a, x_a), _sorted_side(lw_b, x_b)
        _CASES[name] = dict(sa=sa, sb=sb, ha=ha, hb=hb, got=_op(sa, sb),
                            ref64=[_walks(*p, *q, np.float64) for p, q in zip(ha, hb)],
                            refL=[_walks(*p, *q, np.longdouble) for p, q in zip(ha, hb)])
    return _CASES[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ulps(err, ref):
    return float(err / np.spacing(np.float64(max(abs(float(ref)), 2.0 ** -1000))))


@pytest.mark.parametrize('name', sorted(CASES))
def test_distances_against_the_restatement(name):
    c = _case(name)
    rec = {'case': name}
    ok = True
    for g, (row, r64, rL) in enumerate(zip(c['got'], c['ref64'], c['refL'])):
        assert (row[5], row[6]) == (len(c['ha'][g][0]), len(c['hb'][g][0])), (g, row)
        # ks, where and at which merged position: the float64 restatement's bits (NaN where a side has nothing)
        assert np.array_equal(_bits(row[[0, 1, 7]]), _bits(r64[:3])) or (np.isnan(r64[0]) and np.isnan(row[[0, 1, 2, 3, 4, 7]]).all()), \
            (g, row, r64)
        if np.isnan(r64[0]):
            continue
        for k, what in ((2, 'wasserstein1'), (3, 'wasserstein2'), (4, 'energy')):
            got, f64, ref = np.longdouble(row[k]), np.longdouble(r64[k + 1]), rL[k + 1]
            if not np.isfinite(ref):
                assert row[k] == float(ref), (g, what, row, rL)
                continue
            err, e64 = abs(got - ref), abs(f64 - ref)
            bound = max(16 * e64, 64 * np.longdouble(np.spacing(np.float64(abs(float(ref))))))
            if _ulps(err, ref) >= rec.get(what + '_err_ulp', -1.0):
                rec.update({what + '_err_ulp': _ulps(err, ref), what + '_f64_restatement_err_ulp': _ulps(e64, ref),
                            what + '_bound_ulp': _ulps(bound, ref)})
            ok = ok and bool(err <= bound)
    print('twosample %s' % json.dumps(rec))
    if os.environ.get('PP_TWOSAMPLE_ERRORS'):
        with open(os.environ['PP_TWOSAMPLE_ERRORS'], 'a') as f:
            f.write(json.dumps(rec) + '\n')
    assert ok, rec
    if name == 'identical 5000+5000':
        assert (c['got'][0, [0, 2, 3, 4]] == 0).all() and c['got'][0, 1] == 1.25
    if name == 'three groups':
        assert np.isnan(c['got'][1, :5]).all() and not np.isnan(c['got'][[0, 2]]).any()


@pytest.mark.parametrize('name', sorted(CASES))
def test_same_bits_again_and_per_group_and_zero_against_itself(name):
    c = _case(name)
    assert np.array_equal(_bits(_op(c['sa'], c['sb'])), _bits(c['got']))
    for g in range(len(c['got']) if len(c['got']) > 1 else 0):
        one = [(v[g * n:(g + 1) * n], w[g * n:(g + 1) * n], cnt[g:g + 1], n) for v, w, cnt, n in (c['sa'], c['sb'])]
        assert np.array_equal(_bits(_op(*one)[0]), _bits(c['got'][g])), g
    for side in (c['sa'], c['sb']):
        rows = _op(side, side)
        live = ~np.isnan(rows[:, 0])
        assert live.sum() >= len(rows) - 1 and (rows[live][:, [0, 2, 3, 4]] == 0).all(), rows


def test_compare_end_to_end_and_compare_batch_is_one_operator_call_that_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import Empirical, TwoSample
    from test_gpu_joint_moments import _posterior, _straight_line_model
    model, _ = _straight_line_model()
    a, b = _posterior(300), _posterior(4097)
    r = a.compare(b)
    assert isinstance(r, TwoSample) and r.count == (300, 4097) and r.ess == (a.effective_sample_size, b.effective_sample_size)
    assert 0 < r.ks <= 1 and 0 <= r.ks_pvalue <= 1 and 0 < r.wasserstein1 <= r.wasserstein2 * (1 + 1e-12) and r.energy > 0
    assert '_dev_sorted' in a.__dict__ and '_dev_sorted' in b.__dict__
    same = a.compare(a)
    assert (same.ks, same.wasserstein1, same.wasserstein2, same.energy, same.ks_pvalue) == (0, 0, 0, 0, 1)
    host = [Empirical(values=list(p._values.cpu().numpy().astype(np.float64)), log_weights=list(p._log_weights.cpu().numpy().astype(np.float64)))
            for p in (a, b)]
    h = a.compare(host[1])
    assert h.ks_location == r.ks_location and h.count == r.count
    for k in ('ks', 'wasserstein1', 'wasserstein2', 'energy'):
        assert abs(getattr(h, k) - getattr(r, k)) <= 1e-12 * getattr(r, k), k
    assert a.compare(b, address='mu').wasserstein1 == a.marginal('mu').compare(b.marginal('mu')).wasserstein1
    # the groups of two batched calls with different num_traces, pairwise
    M = 3
    rng = np.random.default_rng(5)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pa = model.posterior_results_batch(300, observes, seed=13, offset=64)
        pb = model.posterior_results_batch(2300, observes, seed=14, offset=64)
    loop = [x.compare(y) for x, y in zip(pa, pb)]
    loop_mu = [x.compare(y, address='mu') for x, y in zip(pa, pb)]
    calls = []
    for k in ('sort', 'twosample'):
        monkeypatch.setattr(P.ops, 'is_%s_groups' % k, lambda *args, k=k, real=getattr(P.ops, 'is_%s_groups' % k): calls.append(k) or real(*args),
                            raising=False)
    fields = ('ks', 'ks_location', 'ks_pvalue', 'wasserstein1', 'wasserstein2', 'energy', 'count', 'ess')
    for address, want in ((None, loop), ('mu', loop_mu), (None, loop)):
        before = calls.count('twosample')
        fast = pyprob_amd.compare_batch(pa, pb, address=address)
        assert calls.count('twosample') == before + 1 and len(fast) == M
        for f, l in zip(fast, want):
            assert all(np.array_equal(_bits(getattr(f, k)), _bits(getattr(l, k))) for k in fields), (address, vars(f), vars(l))
    assert calls.count('sort') == 4            # two sides, two columns; the third call found both sorts kept
    assert pyprob_amd.compare_batch(pa[::-1], pb)[0].ks == pa[2].compare(pb[0]).ks          # (not one execution in order: the loop)
