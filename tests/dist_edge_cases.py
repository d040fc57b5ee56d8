"""The distribution families at the extremes of their parameters: the case table behind tests/golden/dist_edges.npz
(make_dist_edges_golden.py), tests/test_dist_edges_host.py and tests/test_gpu_dist_edges.py, and the float64 restatement of
every family's log-density (lp64). Host only: numpy and torch on the CPU.

dist_edge_cases() returns name -> dict(family, kind, params, x, tags). A case is one parameter row of one family: `params` is
the row in pp_dist order p0..p3 ([4] float32, unused slots 0; Categorical: the C unnormalised weights), `x` the [V] float32 values
scored under it, `tags` [V] strings. Everything lies on the single-precision grid: parameters and values are rounded to float32
first and the float64 expectation is taken AT those float32 numbers, so the kernels and the expectation see the same inputs.

Tags: 'in' - inside the support; 'out' - outside (the device scores -inf there); 'nan' - x = NaN, for which the only rule is
"-inf or NaN, never finite" (nan_rule_holds).

expected(case) is the float64 value rounded to the fp32 range: below -3.4e38 it is -inf, above +3.4e38 +inf.

Metric (lp_error): |v - ref64| / max(1, |ref64|) over the finite expectations, the +-inf pattern compared exactly (a mismatch is
an infinite error).

What "the family's log-density" means where the reference clamps: Bernoulli scores the probability clamped to [eps, 1 - eps] and
Categorical the normalised weight clamped likewise (torch's probs_to_logits, eps = 2^-23); the restatement clamps too - p = 0
scores log eps at x = 1, not -inf.

REFERENCE_BROKEN names the elements (case, tag-less column index) where the reference's own fp32 value is no yardstick: it is
off the float64 value by more than the cap 1e-2 or is not finite where float64 is (or the reverse). tests/test_dist_edges_host.py
asserts both directions: every listed element exceeds the cap or is not finite in the record, every other stays at or below the
cap. The list was measured with pyprob's wrapper classes (the golden's).
  TruncatedNormal with alpha >= 5 or beta <= -5   Z = Phi(beta) - Phi(alpha) from 0.5 (1 + erf) in fp32: 1e-2 to 6e-2 off at 5 sigma,
                                                   Z = 0 (log-density +inf) from 5.5 sigma on
  Weibull(1, 50) at x = 1e-38, 1e-6, 100, 1e30    torch's transform chain: z^k underflows to 0 and the Jacobian's log gives -inf
                                                   where float64 has -4283.5 and -673.0; NaN (inf - inf) where z^k overflows
  Weibull(1e-3, 2) at x = 1e-38, 1e30             the same chain: -inf for -73.0, NaN for -inf
  Exponential(1e30) at x = 1e30                   -inf, as float64 rounded to the fp32 range: not finite, so no yardstick

Dropped from the table, because pyprob's Beta wrapper takes y = (x - low) / (high - low) in fp32 and on [-2, 3] that rounding alone
moves log(1 - y) at y = 1 - 6e-8 by 0.47 (the float64 expectation takes y from the same float32 x in float64): two elements of
about 560, with the reference's measured error in this module's metric -
  Beta(1e-3, 1e-3, -2, 3) at y = 1 - 6e-8         2.6e-2
  Beta(500, 300, -2, 3) at y = 1 - 6e-8           1.55e-2
The same rows keep every other y, the rows on [0, 1] keep y = 1 - 6e-8, and Beta(0.05, 1) / Beta(1, 1) / Beta(1e4, 1) keep it on
[-2, 3] as well.
"""
import math

import numpy as np
import torch

KIND = {'Normal': 0, 'Uniform': 1, 'Poisson': 3, 'Bernoulli': 4, 'Categorical': 5, 'Exponential': 6, 'Gamma': 7, 'Beta': 8,
        'LogNormal': 9, 'Weibull': 10, 'Binomial': 11, 'VonMises': 12, 'TruncatedNormal': 13}
NPAR = {0: 2, 1: 2, 3: 1, 4: 1, 6: 1, 7: 2, 8: 4, 9: 2, 10: 2, 11: 2, 12: 2, 13: 4}
FP32_MAX = 3.4e38
EPS = float(np.finfo(np.float32).eps)
REFERENCE_CAP = 1e-2          # the reference's own fp32 error per case (the cap of head_edges)
FLOOR_BAR = 2e-4              # the float64 bar of tests/test_gpu_dist_kernels.py


# ---- float64 restatements ----------------------------------------------------------------------------------------------
def _lgamma(x):
    return np.vectorize(math.lgamma, otypes=[np.float64])(np.asarray(x, np.float64))


def truncnormal_log_z(alpha, beta):
    """log(Phi(beta) - Phi(alpha)) in float64. A one-sided interval is taken in its tail's own coordinates,
    log Q(a) + log1p(-Q(b) / Q(a)): finite to 35 sigma."""
    if alpha >= 0 or beta <= 0:
        a, b = (alpha, beta) if alpha >= 0 else (-beta, -alpha)
        qa, qb = 0.5 * math.erfc(a / math.sqrt(2)), 0.5 * math.erfc(b / math.sqrt(2))
        return math.log(qa) + math.log1p(-qb / qa)
    return math.log(0.5 * (math.erf(beta / math.sqrt(2)) - math.erf(alpha / math.sqrt(2))))


def lp64(name, p, x):
    """log p(x) of family `name` with parameters p (pp_dist order; Categorical: the weights) in float64, -inf outside the support."""
    x = np.asarray(x, np.float64)
    p = [float(v) for v in p]
    with np.errstate(all='ignore'):
        if name == 'Normal':
            out = -(x - p[0]) ** 2 / (2 * p[1] ** 2) - math.log(p[1]) - 0.5 * math.log(2 * math.pi)
            ok = np.ones(x.shape, bool)
        elif name == 'Uniform':
            out = np.full(x.shape, -math.log(p[1] - p[0]))
            ok = (x >= p[0]) & (x < p[1])
        elif name == 'Poisson':
            ok = (x >= 0) & (x == np.floor(x))
            xs = np.where(ok, x, 0.0)
            out = np.where(xs == 0, 0.0, xs * math.log(p[0])) - p[0] - _lgamma(xs + 1)
        elif name == 'Bernoulli':
            q = min(max(p[0], EPS), 1 - EPS)
            out = x * math.log(q) + (1 - x) * math.log1p(-q)
            ok = (x == 0) | (x == 1)
        elif name == 'Categorical':
            w = np.asarray(p, np.float64)
            lq = np.log(np.clip(w / w.sum(), EPS, 1 - EPS))
            ok = (x >= 0) & (x < len(w)) & (x == np.floor(x))
            out = lq[np.where(ok, x, 0).astype(np.int64)]
        elif name == 'Exponential':
            out = np.log(p[0]) - p[0] * x
            ok = x >= 0
        elif name == 'Gamma':
            a, b = p[0], p[1]
            out = a * np.log(b) + np.where((a - 1) == 0, 0.0, (a - 1) * np.log(x)) - b * x - math.lgamma(a)
            ok = x >= 0
        elif name == 'Beta':
            y = (x - p[2]) / (p[3] - p[2])
            out = (np.where(p[0] == 1, 0, (p[0] - 1) * np.log(y)) + np.where(p[1] == 1, 0, (p[1] - 1) * np.log1p(-y)) +
                   math.lgamma(p[0] + p[1]) - math.lgamma(p[0]) - math.lgamma(p[1]))
            ok = (y >= 0) & (y <= 1)
        elif name == 'LogNormal':
            ly = np.log(x)
            out = -(ly - p[0]) ** 2 / (2 * p[1] ** 2) - math.log(p[1]) - 0.5 * math.log(2 * math.pi) - ly
            ok = x > 0
        elif name == 'Weibull':
            z = x / p[0]
            out = math.log(p[1]) - math.log(p[0]) + (p[1] - 1) * np.log(z) - z ** p[1]
            ok = x > 0
        elif name == 'Binomial':
            n, t = p[0], p[1]
            lq = -np.logaddexp(0, -t)       # log p
            l1q = -np.logaddexp(0, t)       # log (1 - p)
            ok = (x >= 0) & (x <= n) & (x == np.floor(x))
            xs = np.where(ok, x, 0.0)
            out = _lgamma(n + 1) - _lgamma(xs + 1) - _lgamma(n - xs + 1) + xs * lq + (n - xs) * l1q
        elif name == 'VonMises':
            k = torch.tensor(p[1], dtype=torch.float64)
            log_i0 = p[1] + float(torch.log(torch.special.i0e(k)))
            out = p[1] * np.cos(x - p[0]) - math.log(2 * math.pi) - log_i0
            ok = np.isfinite(x)
        elif name == 'TruncatedNormal':
            mu, sd, lo, hi = p
            z = (x - mu) / sd
            alpha, beta = (lo - mu) / sd, (hi - mu) / sd
            if alpha >= 0 or beta <= 0:       # phi(z) / Z with the exponents joined: neither part underflows
                a = alpha if alpha >= 0 else -beta
                zt = z if alpha >= 0 else -z
                out = (-0.5 * (zt - a) * (zt + a) - 0.5 * math.log(2 * math.pi) - math.log(sd) -
                       (truncnormal_log_z(alpha, beta) + 0.5 * a * a))
            else:
                out = -0.5 * z * z - 0.5 * math.log(2 * math.pi) - math.log(sd) - truncnormal_log_z(alpha, beta)
            ok = (x >= lo) & (x <= hi)
        else:
            raise KeyError(name)
    return np.where(ok, out, -np.inf)


def to_fp32_range(v):
    """A float64 result as the fp32 range holds it: -inf below -3.4e38, +inf above 3.4e38."""
    v = np.asarray(v, np.float64)
    return np.where(v < -FP32_MAX, -np.inf, np.where(v > FP32_MAX, np.inf, v))


def expected(case):
    """The float64 expectation of a case ([V]; NaN at the 'nan' columns, which have a rule of their own)."""
    x = case['x'].astype(np.float64)
    nan = case['tags'] == 'nan'
    out = to_fp32_range(lp64(case['family'], case['params'].astype(np.float64), np.where(nan, 1.0, x)))
    return np.where(nan, np.nan, out)


def lp_error(v, ref64):
    """|v - ref64| / max(1, |ref64|) over the finite expectations; inf where the +-inf pattern (or a NaN) differs. NaN
    expectations (the 'nan' columns) are left out."""
    v, ref64 = np.asarray(v, np.float64), np.asarray(ref64, np.float64)
    keep = ~np.isnan(ref64)
    v, ref64 = v[keep], ref64[keep]
    if v.size == 0:
        return 0.0
    fin = np.isfinite(ref64)
    if np.isnan(v).any() or not np.array_equal(v[~fin], ref64[~fin]) or not np.isfinite(v[fin]).all():
        return float('inf')
    if not fin.any():
        return 0.0
    return float((np.abs(v[fin] - ref64[fin]) / np.maximum(1.0, np.abs(ref64[fin]))).max())


def nan_rule_holds(v, tags):
    """x = NaN scores -inf or NaN, never a finite value (and never +inf)."""
    v = np.asarray(v)[np.asarray(tags) == 'nan']
    return bool(np.all(np.isnan(v) | np.isneginf(v)))


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _f32(v):
    return np.asarray(v, np.float32)


def _down(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def _up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def _fmt(v):
    s = str(np.float32(v)).replace('+', '')       # (the shortest text that names the float32)
    return s[:-2] if s.endswith('.0') else s


def _support(family, p, x):
    """in / out per element (float32 arithmetic where the device's own test is float32: Beta's y)"""
    x = _f32(x)
    with np.errstate(all='ignore'):
        if family in ('Normal',):
            ok = np.ones(x.shape, bool)
        elif family == 'VonMises':
            ok = np.isfinite(x)
        elif family == 'Uniform':
            ok = (x >= p[0]) & (x < p[1])
        elif family in ('Exponential', 'Gamma'):
            ok = x >= 0
        elif family in ('LogNormal', 'Weibull'):
            ok = x > 0
        elif family == 'Poisson':
            ok = (x >= 0) & (x == np.floor(x))
        elif family == 'Bernoulli':
            ok = (x == 0) | (x == 1)
        elif family == 'Categorical':
            ok = (x >= 0) & (x < len(p)) & (x == np.floor(x))
        elif family == 'Beta':
            y = (x - p[2]) / (p[3] - p[2])
            ok = (y >= 0) & (y <= 1)
        elif family == 'Binomial':
            ok = (x >= 0) & (x <= p[0]) & (x == np.floor(x))
        else:
            ok = (x >= p[2]) & (x <= p[3])
    return ok


def _case(out, family, p, xs):
    p = _f32(p)
    x = np.concatenate([_f32(xs), _f32([np.nan])])
    tags = np.where(_support(family, p, x), 'in', 'out')
    tags[-1] = 'nan'
    params = p if family == 'Categorical' else np.concatenate([p, np.zeros(4 - len(p), np.float32)])
    name = '%s(%s)' % (family, ', '.join(_fmt(v) for v in p)) if family != 'Categorical' else 'Categorical_C%d_%d' % (
        len(p), sum(1 for n in out if n.startswith('Categorical_C%d_' % len(p))))
    assert name not in out, name
    out[name] = dict(family=family, kind=KIND[family], params=params, x=x, tags=tags)


# dropped (module docstring): y = 1 - 6e-8 of these rows
DROPPED_BETA_NEAR_ONE = [(1e-3, 1e-3, -2, 3), (500, 300, -2, 3)]
TRUNCNORMAL_ROWS = [(0, 1, -1, 2), (0, 1, 3, 4), (0, 1, 3.99, 5), (0, 1, 4, 5), (0, 1, 5, 6), (0, 1, 5.5, 6.5), (0, 1, 6, 6.1),
                    (2, 0.5, 4.5, 4.6), (1, 2, 10, 40), (0, 1, 30, 31)]


def dist_edge_cases():
    out = {}
    f = np.float32
    for a, b in [(0.05, 1), (1e-3, 1), (1, 1e-6), (2, 1e6), (500, 3), (1e4, 100)]:
        _case(out, 'Gamma', (a, b), [0, 1e-30, 1e-6, f(a) / f(b), f(10) * f(a) / f(b), 1e30])
    for c1, c0 in [(0.05, 1), (1e-3, 1e-3), (1, 1), (500, 300), (1e4, 1)]:
        for lo, hi in [(0, 1), (-2, 3)]:
            ys = [0, 1e-30, 1e-7, 0.5, f(c1) / (f(c1) + f(c0)), 1 - 6e-8, 1]
            if (c1, c0, lo, hi) in DROPPED_BETA_NEAR_ONE:
                ys.remove(1 - 6e-8)
            _case(out, 'Beta', (c1, c0, lo, hi), f(lo) + _f32(ys) * (f(hi) - f(lo)))
    for loc, scale in [(0, 1), (0, 1e-3), (50, 0.1), (-50, 5)]:
        _case(out, 'LogNormal', (loc, scale), [1e-45, 1e-38, 1e-10, 1, math.exp(min(loc, 80)), 1e30, 3e38])
    for l, k in [(1, 1), (2, 0.05), (1e3, 0.7), (1, 50), (1e-3, 2)]:
        _case(out, 'Weibull', (l, k), [1e-38, f(1e-6) * f(l), f(0.999) * f(l), l, 3 * f(l), 100 * f(l), 1e30])
    for rate in [1e-30, 40, 1e30]:
        _case(out, 'Exponential', (rate,), [0, 1e-30, f(1) / f(rate), 1e30])
    for loc, scale in [(0, 1e-15), (1e6, 1), (0, 1e15)]:
        _case(out, 'Normal', (loc, scale), [loc, f(loc) + f(scale), f(loc) + f(30) * f(scale)])
    for lo, hi in [(0, 1e-30), (1, 2), (0, 1e30)]:
        _case(out, 'Uniform', (lo, hi), [lo, _down(lo), _down(hi), hi])
    for rate in [1e-45, 1e-30, 0.3, 3000]:
        _case(out, 'Poisson', (rate,), [0, 1, round(rate), round(rate + 3 * math.sqrt(rate)), 1e4, 2.5, -1])
    for p in [0, 1e-10, 0.5, 1 - 6e-8, 1]:
        _case(out, 'Bernoulli', (p,), [0, 1, 0.5, -1, 2])
    rng = np.random.default_rng(5)
    for C in (1, 2, 64):
        rows = {1: [[1.0], [7.5]], 2: [[0.0, 1.0], [3.0, 1.0], [1e-10, 0.5]],
                64: [np.where(np.arange(64) % 5 == 0, 0.0, rng.uniform(0.1, 4.0, 64)), np.concatenate([[1e3], np.full(63, 1e-6)])]}[C]
        for row in rows:       # unnormalised rows; rows with zero weights (C = 64: on the first and the last index)
            row = _f32(row)
            if C == 64:
                row[-1] = 0.0
            _case(out, 'Categorical', row, [0, C - 1, C, -1, 1.5] + ([1] if C == 64 else []))
    for n, t in [(0, 0), (1, 0), (10, 0), (200, 40), (200, -90), (5000, 3.5), (5000, -8), (1e5, 0)]:
        _case(out, 'Binomial', (n, t), [0, 1, n // 2, n - 1, n, n + 1, 2.5])
    for loc, k in [(0, 1e-6), (0, 3.7499), (0, 3.75), (0, 300), (0, 1e4), (3, 1e5), (100, 2)]:
        _case(out, 'VonMises', (loc, k), [loc, f(loc) + f(1e-3), f(loc) + f(math.pi), -3, 1e4, np.inf])
    rows = list(TRUNCNORMAL_ROWS)
    # the mirror image of every one-sided row in the lower tail, and (0, 1, -8, -7)
    rows += [(-mu, sd, -hi, -lo) for mu, sd, lo, hi in TRUNCNORMAL_ROWS if (lo - mu) / sd >= 0] + [(0, 1, -8, -7)]
    for mu, sd, lo, hi in rows:
        w = f(hi) - f(lo)
        _case(out, 'TruncatedNormal', (mu, sd, lo, hi), [_down(lo), lo, f(lo) + f(1e-3) * w, f(0.5) * (f(lo) + f(hi)), hi, _up(hi)])
    for c in out.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def _tn_broken():
    names = []
    for mu, sd, lo, hi in TRUNCNORMAL_ROWS:
        if (lo - mu) / sd >= 5:
            names += ['TruncatedNormal(%s)' % ', '.join(_fmt(np.float32(v)) for v in r) for r in ((mu, sd, lo, hi), (-mu, sd, -hi, -lo))]
    return names + ['TruncatedNormal(0, 1, -8, -7)']


# (case, columns of x): the elements where the reference's fp32 value exceeds REFERENCE_CAP or is not finite (docstring)
REFERENCE_BROKEN = dict({name: (1, 2, 3, 4) for name in _tn_broken()},       # every value inside [low, high]
                        **{'Weibull(1, 50)': (0, 1, 5, 6), 'Weibull(0.001, 2)': (0, 6), 'Exponential(1e30)': (3,)})


def reference_split(case_name, case):
    """(columns the reference is a yardstick for, columns listed in REFERENCE_BROKEN); the 'nan' column is in neither."""
    broken = np.zeros(len(case['x']), bool)
    broken[list(REFERENCE_BROKEN.get(case_name, ()))] = True
    live = case['tags'] != 'nan'
    return live & ~broken, live & broken


def reference_errors(case_name, case, ref32):
    """(the reference's fp32 error over the columns it is a yardstick for, its per-element error on the broken ones)"""
    exp = expected(case)
    good, broken = reference_split(case_name, case)
    return lp_error(np.asarray(ref32)[good], exp[good]), [lp_error(np.asarray(ref32)[i:i + 1], exp[i:i + 1]) for i in np.nonzero(broken)[0]]


def bars(case_name, case, ref32):
    """Per element of the case: max(2e-4, 4 x the reference's fp32 error of the case); the floor on REFERENCE_BROKEN elements.
    Returns ([V] bars, the reference's error)."""
    err, _ = reference_errors(case_name, case, ref32)
    good, broken = reference_split(case_name, case)
    return np.where(broken, FLOOR_BAR, max(FLOOR_BAR, 4.0 * err)), err


def element_errors(v, exp):
    """Per-element |v - exp| / max(1, |exp|) ([V]; inf on a +-inf / NaN mismatch, 0 where both are the same infinity, NaN on
    the 'nan' columns)."""
    return np.array([np.nan if np.isnan(e) else lp_error(np.asarray(v)[i:i + 1], np.asarray(exp)[i:i + 1]) for i, e in enumerate(exp)])
