"""The distribution families at the extremes of their parameters (tests/dist_edge_cases.py) on the device: the one per-element
log-density of csrc/dist_math.hpp, scalar_log_prob_at, through the three kernels that score with it, and the samplers'
regime branches with per-lane parameters.

Expectation: the float64 restatement dist_edge_cases.lp64 at the float32 inputs, rounded to the fp32 range. Metric:
|got - ref64| / max(1, |ref64|) over finite expectations, the +-inf pattern exactly, no NaN for a value that is not NaN, and
-inf or NaN for x = NaN. Bar per case: max(2e-4, 4 x the error of the reference's own fp32 value of that case)
(tests/golden/dist_edges.npz; at most 1e-2, tests/test_dist_edges_host.py); 2e-4 is the float64 bar of
tests/test_gpu_dist_kernels.py, the 4 is for the device's logf / lgammaf / erff and evaluation order, a few ulp each from
torch's (the rule of tests/test_gpu_head_edges.py). On REFERENCE_BROKEN elements - the TruncatedNormal tails above all - the
reference is no yardstick and the bar is the floor 2e-4. No bar comes from a kernel's output.

With PP_DIST_EDGES_ERRORS=<file> every check appends {case, route, kernel_err, reference_fp32_err, bar}
(profiles/dist_edges_errors.jsonl); the REFERENCE_BROKEN elements of a case get a line of their own, route '<route>/broken',
reference_fp32_err null.

Routes: `dist` pp_dist_logweight with lp_out (every case); `mix` pp_mix_logweight with one component of weight 1; `obs_k1`
pp_obs_logweight with k = 1; `obs_k6` pp_obs_logweight with k = 6, six elements of one family per row (a packed group of four
and a remainder of two; its kernel_err is the worst row's error over that row's bar).
"""
import json
import os

import numpy as np
import pytest
import torch

import dist_edge_cases as E

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dist_edges.npz')
CASES = E.dist_edge_cases()
SCALAR_FAMILIES = [f for f in E.KIND if f != 'Categorical']
N_LANES = 64 * 7 + 5


@pytest.fixture(scope='module')
def ops():
    from pyprob_amd import build as B
    B.build()
    from pyprob_amd.ops import ops as O
    return O


@pytest.fixture(scope='module')
def record():
    """name -> (expectation [V], bars [V], the reference's fp32 error): computed once, read-only."""
    G = np.load(GOLDEN)
    out = {}
    for name, case in CASES.items():
        for key in ('params', 'x'):
            assert np.array_equal(G[name + '/' + key].view(np.int32), case[key].view(np.int32)), \
                'dist_edges.npz is stale: rerun make_dist_edges_golden.py'
        bars, ref_err = E.bars(name, case, G[name + '/lp'])
        assert ref_err <= E.REFERENCE_CAP
        exp = E.expected(case)
        for a in (exp, bars):
            a.setflags(write=False)
        out[name] = (exp, bars, ref_err)
    return out


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32).reshape(-1)).to(DEV)       # (a copy: the table's arrays are read-only)


def _scalar_args(case):
    """(params, strides) of a case for pp_dist: every parameter shared (stride 0); Categorical: one row of C weights."""
    if case['family'] == 'Categorical':
        return [_dev(case['params']), None, None, None], [0, len(case['params']), 0, 0]
    np_ = E.NPAR[case['kind']]
    return [_dev(case['params'][q:q + 1]) for q in range(np_)] + [None] * (4 - np_), [0, 0, 0, 0]


def run_dist(ops, case):
    x = _dev(case['x'])
    n = x.numel()
    ps, ss = _scalar_args(case)
    lp = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    ops.dist_logweight(None, [case['kind']], ps, ss, [x], [1.0], None, lp, n)
    return lp.cpu().numpy()


@pytest.fixture(scope='module')
def direct(ops):
    """name -> the lp_out of pp_dist_logweight on the case, parameters shared: what every other route is compared with bit for bit."""
    out = {name: run_dist(ops, case) for name, case in CASES.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def check(name, route, got, rec):
    """The rules of the module docstring on one case's values; writes the record lines, then asserts."""
    case = CASES[name]
    exp, bars, ref_err = rec
    live = case['tags'] != 'nan'
    assert not np.isnan(got[live]).any(), (name, route, 'NaN for a value that is not NaN', got)
    assert E.nan_rule_holds(got, case['tags']), (name, route, 'x = NaN scored', got[~live])
    assert np.array_equal(np.isneginf(got[live]), np.isneginf(exp[live])), (name, route, '-inf pattern', got, exp)
    assert np.array_equal(np.isposinf(got[live]), np.isposinf(exp[live])), (name, route, '+inf pattern', got, exp)
    errs = E.element_errors(got, exp)
    good, broken = E.reference_split(name, case)
    lines = [dict(case=name, route=route, kernel_err=float(errs[good].max()), reference_fp32_err=float(ref_err), bar=float(bars[good].max()))]
    if broken.any():
        lines.append(dict(case=name, route=route + '/broken', kernel_err=float(errs[broken].max()), reference_fp32_err=None,
                          bar=float(bars[broken].max())))
    path = os.environ.get('PP_DIST_EDGES_ERRORS')
    if path:
        with open(path, 'a') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')
    for ln in lines:
        print(json.dumps(ln))
    assert np.all(errs[live] <= bars[live]), (name, route, case['x'][live][errs[live] > bars[live]], got, exp, bars)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---- 1. pp_dist_logweight, lp_out ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_dist_logweight(record, direct, name):
    check(name, 'dist', direct[name], record[name])


# ---- 2. the other two kernels --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def log_weight_one(ops):
    """What pp_mix_logweight adds for a component of weight 1: log of the weight clamped to 1 - eps (util.clamp_probs), read
    from the kernel itself through a component whose log-density is exactly 0 - Uniform(0, 1) at 0.5."""
    lp = torch.empty(1, dtype=torch.float32, device=DEV)
    ops.mix_logweight(None, [1], [_dev([0.0]), _dev([1.0]), None, None], [0, 0, 0, 0], _dev([1.0]), _dev([0.5]), 1.0, None, lp, 1)
    v = np.float32(lp.item())
    assert abs(float(v) + E.EPS) < 1e-13, v          # log(1 - eps) = -eps - eps^2 / 2
    return v


@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c['family'] != 'Categorical'))
def test_routes_mixture_and_obs_k1(ops, record, direct, log_weight_one, name):
    """pp_mix_logweight with one component of weight 1 and pp_obs_logweight with k = 1 give pp_dist_logweight's bits: the
    mixture after its one fp32 addition of log(1 - eps), the clamped weight's log, to the component's log-density."""
    case = CASES[name]
    x = _dev(case['x'])
    n = x.numel()
    ps, ss = _scalar_args(case)
    lp = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    ops.obs_logweight(None, case['kind'], ps, x.reshape(n, 1), 1, 1.0, None, lp, n)
    obs = lp.cpu().numpy()
    nan = np.isnan(direct[name])
    assert np.array_equal(np.isnan(obs), nan) and np.array_equal(bits(obs)[~nan], bits(direct[name])[~nan]), (name, obs, direct[name])
    check(name, 'obs_k1', obs, record[name])
    lp = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    ops.mix_logweight(None, [case['kind']], ps, ss, _dev([1.0]), x, 1.0, None, lp, n)
    mix = lp.cpu().numpy()
    with np.errstate(all='ignore'):
        want = (log_weight_one + direct[name]).astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(mix), nan) and np.array_equal(bits(mix)[~nan], bits(want)[~nan]), (name, mix, want)
    check(name, 'mix', mix, record[name])


def family_elements(family, finite_only=False, record=None):
    """[(case name, column)] of a family in table order (finite_only: the elements with a finite expectation)."""
    out = []
    for name, case in CASES.items():
        if case['family'] != family:
            continue
        for i, tag in enumerate(case['tags']):
            if finite_only and (tag != 'in' or not np.isfinite(record[name][0][i])):
                continue
            out.append((name, i))
    return out


@pytest.mark.parametrize('family', SCALAR_FAMILIES)
def test_route_obs_k6(ops, record, family):
    """pp_obs_logweight with k = 6: every row holds six different elements of one family (parameters and values [n, 6]), a
    packed group of four and a remainder of two, against the float64 sum. The bar of a row is the sum of its elements' bars,
    each in its element's own scale: sum_i bar_i max(1, |ref64_i|). The last row swaps one element for one outside the support
    where the table has one for the family: -inf."""
    elems = family_elements(family, True, record)
    k = 6
    n = (len(elems) + k - 1) // k + 1
    idx = [[elems[(r * k + e) % len(elems)] for e in range(k)] for r in range(n)]
    out_elem = next(((nm, i) for nm, c in CASES.items() if c['family'] == family for i, t in enumerate(c['tags']) if t == 'out'), None)
    if out_elem is not None:
        idx[-1][4] = out_elem
    np_ = E.NPAR[E.KIND[family]]
    P = np.array([[CASES[nm]['params'] for nm, _ in row] for row in idx], np.float32)           # [n, 6, 4]
    X = np.array([[CASES[nm]['x'][i] for nm, i in row] for row in idx], np.float32)
    ps = [torch.from_numpy(np.ascontiguousarray(P[:, :, q])).to(DEV) for q in range(np_)] + [None] * (4 - np_)
    lp = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    ops.obs_logweight(None, E.KIND[family], ps, torch.from_numpy(X).to(DEV), k, 1.0, None, lp, n)
    got = lp.cpu().numpy().astype(np.float64)
    worst = 0.0
    for r, row in enumerate(idx):
        exp = np.array([record[nm][0][i] for nm, i in row])
        bar = float(sum(record[nm][1][i] * max(1.0, abs(record[nm][0][i])) for nm, i in row if np.isfinite(record[nm][0][i])))
        if np.isneginf(exp).any():
            assert np.isneginf(got[r]), (family, r, got[r])
            continue
        err = abs(got[r] - exp.sum())
        worst = max(worst, err / bar)
        assert np.isfinite(got[r]) and err <= bar, (family, r, row, got[r], exp.sum(), err, bar)
    line = dict(case=family, route='obs_k6', kernel_err=worst, reference_fp32_err=None, bar=1.0)      # (err / the row's bar)
    path = os.environ.get('PP_DIST_EDGES_ERRORS')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(line) + '\n')
    print(json.dumps(line))
    if out_elem is not None:
        assert np.isneginf(got[-1])


# ---- 3. per-lane parameters, log-density ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', SCALAR_FAMILIES + ['Categorical_C1', 'Categorical_C2', 'Categorical_C64'])
def test_per_lane_parameters_log_density(ops, direct, family):
    """One pp_dist_logweight call of 64 * 7 + 5 lanes, every parameter with stride 1, consecutive lanes cycling through the
    family's elements - neighbouring lanes of a wave in different cases and on both sides of every per-lane branch: each lane
    carries the bits of the scalar-parameter call of its case."""
    if family.startswith('Categorical'):
        C = int(family.split('_C')[1])
        elems = [(nm, i) for nm, i in family_elements('Categorical') if len(CASES[nm]['params']) == C]
        kind = 5
    else:
        elems = family_elements(family)
        kind = E.KIND[family]
    lanes = [elems[r % len(elems)] for r in range(N_LANES)]
    X = np.array([CASES[nm]['x'][i] for nm, i in lanes], np.float32)
    P = np.array([CASES[nm]['params'] for nm, _ in lanes], np.float32)
    if kind == 5:
        ps, ss = [_dev(P), None, None, None], [P.shape[1], P.shape[1], 0, 0]
    else:
        np_ = E.NPAR[kind]
        ps, ss = [_dev(P[:, q]) for q in range(np_)] + [None] * (4 - np_), [1] * np_ + [0] * (4 - np_)
    lp = torch.full((N_LANES,), 7.0, dtype=torch.float32, device=DEV)
    ops.dist_logweight(None, [kind], ps, ss, [_dev(X)], [1.0], None, lp, N_LANES)
    got = lp.cpu().numpy()
    want = np.array([direct[nm][i] for nm, i in lanes], np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (family, np.nonzero(np.isnan(got) != nan)[0])
    bad = np.nonzero(bits(got)[~nan] != bits(want)[~nan])[0]
    assert bad.size == 0, (family, [(lanes[j], got[~nan][j], want[~nan][j]) for j in bad[:5]])


# ---- 4. per-lane parameters, draws --------------------------------------------------------------------------------------------
def _logit(p):
    return float(np.log(p) - np.log1p(-p))


DRAW_REGIMES = {
    'Poisson': [(0.0,), (0.3,), (9.999,), (10.0,), (3000.0,)],
    'Binomial': [(0.0, _logit(0.5)), (10.0, _logit(0.3)), (40.0, _logit(0.25)), (39.0, _logit(0.25)), (200.0, _logit(0.4)),
                 (5000.0, _logit(0.97)), (200.0, 40.0), (200.0, -40.0)],
    'Gamma': [(0.05, 1.0), (0.999, 2.0), (1.0, 1.0), (4.5, 0.5), (500.0, 3.0)],
    'Beta': [(0.05, 500.0, 0.0, 1.0), (0.999, 0.05, 0.0, 1.0), (1.0, 0.999, -2.0, 3.0), (4.5, 1.0, 0.0, 1.0), (500.0, 4.5, 1.0, 4.0)],
    'VonMises': [(0.0, 1e-6), (1.0, 9e-6), (0.0, 1.1e-5), (-2.5, 8.0), (0.0, 300.0)],
    'TruncatedNormal': [(0.0, 1.0, -1.0, 2.0), (0.0, 1.0, -3.0, -0.5), (0.0, 1.0, 0.5, 3.0), (0.0, 1.0, 3.99, 5.0), (0.0, 1.0, 4.0, 5.0),
                        (0.0, 1.0, 6.0, 6.1), (0.0, 1.0, -31.0, -30.0)],
}


def _draw(ops, kind, ps, ss, n, seed, offset, stream, rows=None):
    out = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    ops.dist_draw(kind, ps, ss, rows, out, seed, offset, stream)
    return out.cpu().numpy()


@pytest.mark.parametrize('family', sorted(DRAW_REGIMES))
def test_per_lane_parameters_draws(ops, family):
    """One pp_dist_draw of 64 * 7 + 5 lanes with stride-1 parameters cycling through the sampler's regimes, so that every wave
    diverges across its branches (each consumes another number of Philox blocks per lane): lane r carries the bits of lane r of
    the scalar-parameter call with the same seed, offset and stream. Again with a row list and an offset."""
    kind = E.KIND[family]
    sets = DRAW_REGIMES[family]
    np_ = E.NPAR[kind]
    n = N_LANES
    P = np.array([sets[r % len(sets)] for r in range(n)], np.float32)
    lane_ps = [_dev(P[:, q]) for q in range(np_)] + [None] * (4 - np_)
    lane_ss = [1] * np_ + [0] * (4 - np_)
    rows = torch.from_numpy(np.nonzero(np.random.default_rng(3).random(n) < 0.6)[0].astype(np.int64)).to(DEV)
    for seed, offset, stream, rw in ((41, 0, 3, None), (41, 10 ** 6 + 7, 5, rows)):
        got = _draw(ops, kind, lane_ps, lane_ss, n, seed, offset, stream, rw)
        listed = np.ones(n, bool) if rw is None else np.isin(np.arange(n), rw.cpu().numpy())
        assert np.all(got[~listed] == -7.0)
        assert not np.isnan(got[listed]).any(), (family, np.nonzero(np.isnan(got))[0][:5])
        for s, p in enumerate(sets):
            sc_ps = [_dev([p[q]]) for q in range(np_)] + [None] * (4 - np_)
            ref = _draw(ops, kind, sc_ps, [0, 0, 0, 0], n, seed, offset, stream, rw)
            mine = listed & (np.arange(n) % len(sets) == s)
            assert np.array_equal(bits(got[mine]), bits(ref[mine])), (family, p, offset, got[mine][:6], ref[mine][:6])


# ---- 5. the degenerate regimes, exactly -------------------------------------------------------------------------------------------
def test_degenerate_discrete_draws_are_exact(ops):
    n = 1 << 16
    for name, p, want in (('Poisson', (0.0,), 0.0), ('Binomial', (0.0, 0.3), 0.0), ('Binomial', (0.0, -2.0), 0.0),
                          ('Binomial', (200.0, 40.0), 200.0), ('Binomial', (200.0, -40.0), 0.0),
                          ('Binomial', (5000.0, 40.0), 5000.0), ('Binomial', (5000.0, -40.0), 0.0)):
        kind = E.KIND[name]
        ps = [_dev([v]) for v in p] + [None] * (4 - len(p))
        v = _draw(ops, kind, ps, [0, 0, 0, 0], n, 9, 0, 2)
        assert np.all(v == want), (name, p, np.unique(v)[:5])


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------
def test_lockstep_observe_in_the_far_tail():
    """t = sample(Normal(0, 1)); observe(TruncatedNormal(t, 1, 6, 7), 6.5), 300 particles in lock step: the interval lies 3 to 9
    standard deviations above each particle's mean. Every log-weight is finite and is the float64 log-density of its own t
    under the floor bar."""
    import pyprob_amd
    from pyprob_amd import distributions as D
    from pyprob_amd.model import Model
    from pyprob_amd.state import InferenceEngine

    class NormalThenTail(Model):
        def forward(self):
            t = pyprob_amd.sample(D.Normal(0.0, 1.0))
            pyprob_amd.observe(D.TruncatedNormal(t, 1.0, 6.0, 7.0), name='y')
            return t

    n = 300
    post = NormalThenTail().posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, observe={'y': 6.5}, lock_step=True, seed=7)
    t = post._values.detach().cpu().numpy()
    lw = post._log_weights.detach().cpu().numpy()
    assert t.shape == (n,) and lw.shape == (n,), '%d of %d particles left: the others had a non-finite log-weight' % (len(lw), n)
    assert np.isfinite(lw).all(), lw[~np.isfinite(lw)]
    ref = np.array([float(E.lp64('TruncatedNormal', (float(v), 1.0, 6.0, 7.0), [6.5])[0]) for v in t])
    err = np.abs(lw - ref) / np.maximum(1.0, np.abs(ref))
    print('lockstep tail: worst', err.max(), 'at t', t[err.argmax()], 'alpha from', (6.0 - t).min(), 'to', (6.0 - t).max())
    assert err.max() <= E.FLOOR_BAR, (err.max(), t[err.argmax()])
