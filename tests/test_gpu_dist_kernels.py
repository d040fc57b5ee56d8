"""pp_dist_logweight / pp_dist_draw (csrc/dist_kernels.hip, ABI 15) on the device: the log-densities of every pyprob family
against the reference's own fp32 values (tests/golden/dist_lp.npz) and a float64 restatement, row lists and eight-term launches,
the samplers against float64 CDFs / pmfs (Kolmogorov-Smirnov, chi-square, moments), and the Philox counter scheme."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dist_edge_cases import lp64
from helpers import chi2_p

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KIND = {'Normal': 0, 'Uniform': 1, 'Poisson': 3, 'Bernoulli': 4, 'Exponential': 6, 'Gamma': 7, 'Beta': 8, 'LogNormal': 9,
        'Weibull': 10, 'Binomial': 11, 'VonMises': 12, 'TruncatedNormal': 13}
NPAR = {0: 2, 1: 2, 3: 1, 4: 1, 6: 1, 7: 2, 8: 4, 9: 2, 10: 2, 11: 2, 12: 2, 13: 4}
N_DRAWS = 1 << 20


@pytest.fixture(scope='module')
def ops():
    from pyprob_amd import build as B
    B.build()
    from pyprob_amd.ops import ops as O
    return O


def _vec(v, n=None):
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1).to(DEV).contiguous()
    return t if n is None or t.numel() == n else t.expand(n).contiguous()


def _params(kind, p):
    ps = [_vec(p[q]) for q in range(NPAR[kind])] + [None] * (4 - NPAR[kind])
    ss = [0 if t is None or t.numel() == 1 else 1 for t in ps]
    return ps, ss


def log_prob(ops, kind, p, x):
    x = _vec(x)
    n = x.numel()
    ps, ss = _params(kind, p)
    lp = torch.empty(n, dtype=torch.float32, device=DEV)
    ops.dist_logweight(None, [kind], ps, ss, [x], [1.0], None, lp, n)
    return lp


def draw(ops, kind, p, n=N_DRAWS, seed=1234, offset=0, stream=7, rows=None, out=None):
    ps, ss = _params(kind, p)
    out = torch.full((n,), -7.0, dtype=torch.float32, device=DEV) if out is None else out
    ops.dist_draw(kind, ps, ss, rows, out, seed, offset, stream)
    return out


# ---- float64 restatements: dist_edge_cases.lp64 (shared with tests/test_gpu_dist_edges.py) ----------------------------------
def _lgamma(x):
    return np.vectorize(math.lgamma)(np.asarray(x, np.float64))


FAMILIES = ['Exponential', 'Gamma', 'Beta', 'LogNormal', 'Weibull', 'Binomial', 'VonMises', 'TruncatedNormal']


@pytest.mark.parametrize('name', FAMILIES)
def test_log_density_matches_reference_and_float64(ops, name):
    g = dict(np.load(os.path.join(GOLDEN, 'dist_lp.npz')))
    kind = KIND[name]
    # Binomial (lgamma of counts up to 200, differences of terms of ~1e3) and VonMises (the I0 polynomial: torch's fp32
    # evaluation order vs ours) lose a few more fp32 digits than the others
    tol = 1e-4 if name in ('Binomial', 'VonMises') else 1e-5
    for i, p in enumerate(g[name + '_params']):
        x = g[name + '_x'][i]
        got = log_prob(ops, kind, p, x).cpu().numpy()
        ref = g[name + '_lp'][i]
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, err_msg='%s %s' % (name, p))
        assert np.array_equal(np.isneginf(got), np.isneginf(ref))
        fin = np.isfinite(ref)
        # the polynomial log I0 of torch is itself ~1e-7 relative off the true Bessel function; fp32 lgamma sums ~1e-6
        np.testing.assert_allclose(got[fin], lp64(name, p, x)[fin], rtol=2e-4, atol=2e-4, err_msg='%s %s (float64)' % (name, p))


def test_out_of_support_is_exactly_minus_inf(ops):
    cases = [('Exponential', (1.0,), -0.5), ('Gamma', (2.0, 1.0), -1e-3), ('Beta', (2.0, 2.0, 1.0, 3.0), 3.5),
             ('LogNormal', (0.0, 1.0), 0.0), ('Weibull', (1.0, 2.0), -1.0), ('Binomial', (10.0, 0.0), 11.0),
             ('Binomial', (10.0, 0.0), 2.5), ('TruncatedNormal', (0.0, 1.0, -1.0, 1.0), 1.0001),
             ('VonMises', (0.0, 1.0), float('inf'))]
    for name, p, x in cases:
        v = float(log_prob(ops, KIND[name], p, [x]).item())
        assert v == float('-inf'), (name, p, x, v)


def test_row_lists_and_eight_terms(ops):
    n = 5000
    torch.manual_seed(0)
    gen = [('Gamma', (torch.rand(n) * 3 + 0.2, 1.5), torch.rand(n) * 4),
           ('Beta', (0.7, torch.rand(n) + 0.5, 0.0, 2.0), torch.rand(n) * 2),
           ('LogNormal', (torch.randn(n), 0.8), torch.rand(n) * 5 + 0.01),
           ('Weibull', (2.0, torch.rand(n) + 0.5), torch.rand(n) * 3 + 0.01),
           ('Binomial', (30.0, torch.randn(n)), torch.randint(0, 31, (n,)).float()),
           ('VonMises', (torch.randn(n), 4.0), torch.rand(n) * 6 - 3),
           ('TruncatedNormal', (torch.randn(n), 1.3, -2.0, 2.0), torch.rand(n) * 4 - 2),
           ('Exponential', (torch.rand(n) + 0.1,), torch.rand(n) * 3)]
    scales = [1.0, 0.5, -1.0, 2.0, 1.0, 0.25, 1.0, 3.0]
    ps_all, ss_all, xs, kinds = [], [], [], []
    for name, p, x in gen:
        ps, ss = _params(KIND[name], p)
        ps_all += ps
        ss_all += ss
        xs.append(_vec(x))
        kinds.append(KIND[name])
    base = torch.randn(n, device=DEV)
    lw8 = base.clone()
    ops.dist_logweight(lw8, kinds, ps_all, ss_all, xs, scales, None, None, n)
    lw1 = base.clone()
    for q in range(8):
        ops.dist_logweight(lw1, [kinds[q]], ps_all[4 * q:4 * q + 4], ss_all[4 * q:4 * q + 4], [xs[q]], [scales[q]], None, None, n)
    torch.testing.assert_close(lw8, lw1, rtol=1e-5, atol=1e-4)
    rows = torch.nonzero(torch.rand(n, device=DEV) < 0.3).reshape(-1)
    lwr = base.clone()
    ops.dist_logweight(lwr, kinds, ps_all, ss_all, xs, scales, rows, None, n)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[rows] = True
    assert torch.equal(lwr[mask], lw8[mask])
    assert torch.equal(lwr[~mask], base[~mask])          # unlisted rows bit-unchanged


# ---- samplers ---------------------------------------------------------------------------------------------------------
def _phi(z):
    return 0.5 * (1 + torch.special.erf(z / math.sqrt(2)))


def _numeric_cdf(pdf, lo, hi, x):
    grid = torch.linspace(lo, hi, 400001, dtype=torch.float64)
    f = pdf(grid)
    c = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(0.5 * (f[1:] + f[:-1]) * (grid[1:] - grid[:-1]), 0)])
    c = c / c[-1]
    return torch.from_numpy(np.interp(x.numpy(), grid.numpy(), c.numpy()))


def cdf64(name, p, x):
    x = x.double()
    if name == 'Normal':
        return _phi((x - p[0]) / p[1])
    if name == 'Uniform':
        return ((x - p[0]) / (p[1] - p[0])).clamp(0, 1)
    if name == 'Exponential':
        return 1 - torch.exp(-p[0] * x.clamp(min=0))
    if name == 'Gamma':
        return torch.special.gammainc(torch.tensor(float(p[0]), dtype=torch.float64), p[1] * x.clamp(min=0))
    if name == 'LogNormal':
        return _phi((torch.log(x) - p[0]) / p[1])
    if name == 'Weibull':
        return 1 - torch.exp(-(x.clamp(min=0) / p[0]) ** p[1])
    if name == 'Beta':
        a, b, lo, hi = p
        y = ((x - lo) / (hi - lo)).clamp(0, 1)
        if b == 1.0:
            return y ** a
        if a == 1.0:
            return 1 - (1 - y) ** b
        return _numeric_cdf(lambda t: t ** (a - 1) * (1 - t) ** (b - 1), 0.0, 1.0, y)
    if name == 'VonMises':
        mu, k = p
        return _numeric_cdf(lambda t: torch.exp(k * (torch.cos(t - mu) - 1)), -math.pi, math.pi, x)
    mu, sd, lo, hi = p
    a, b = _phi(torch.tensor((lo - mu) / sd, dtype=torch.float64)), _phi(torch.tensor((hi - mu) / sd, dtype=torch.float64))
    return ((_phi((x - mu) / sd) - a) / (b - a)).clamp(0, 1)


def moments64(name, p):
    if name == 'Normal':
        return p[0], p[1] ** 2
    if name == 'Uniform':
        return 0.5 * (p[0] + p[1]), (p[1] - p[0]) ** 2 / 12
    if name == 'Exponential':
        return 1 / p[0], 1 / p[0] ** 2
    if name == 'Gamma':
        return p[0] / p[1], p[0] / p[1] ** 2
    if name == 'LogNormal':
        return math.exp(p[0] + p[1] ** 2 / 2), (math.exp(p[1] ** 2) - 1) * math.exp(2 * p[0] + p[1] ** 2)
    if name == 'Weibull':
        g1, g2 = math.gamma(1 + 1 / p[1]), math.gamma(1 + 2 / p[1])
        return p[0] * g1, p[0] ** 2 * (g2 - g1 * g1)
    if name == 'Beta':
        a, b, lo, hi = p
        r = hi - lo
        return lo + r * a / (a + b), r * r * a * b / ((a + b) ** 2 * (a + b + 1))
    if name == 'VonMises':
        return None
    mu, sd, lo, hi = p
    al, be = (lo - mu) / sd, (hi - mu) / sd
    pa, pb = math.exp(-al * al / 2) / math.sqrt(2 * math.pi), math.exp(-be * be / 2) / math.sqrt(2 * math.pi)
    Z = 0.5 * (math.erf(be / math.sqrt(2)) - math.erf(al / math.sqrt(2)))
    m = mu + sd * (pa - pb) / Z
    return m, sd * sd * (1 + (al * pa - be * pb) / Z - ((pa - pb) / Z) ** 2)


CONTINUOUS = [('Normal', (1.0, 2.0)), ('Uniform', (-1.0, 3.0)), ('Exponential', (0.5,)), ('Exponential', (40.0,)),
              ('Gamma', (0.05, 1.0)), ('Gamma', (0.5, 2.0)), ('Gamma', (1.0, 1.0)), ('Gamma', (4.5, 0.5)), ('Gamma', (500.0, 3.0)),
              ('Beta', (2.0, 3.0, 0.0, 1.0)), ('Beta', (0.5, 1.0, 1.0, 4.0)), ('Beta', (1.0, 0.2, 0.0, 1.0)),
              ('Beta', (0.05, 1.0, 0.0, 1.0)), ('LogNormal', (0.5, 0.7)), ('Weibull', (2.0, 0.7)), ('Weibull', (1.0, 5.0)),
              ('VonMises', (1.0, 1e-6)), ('VonMises', (0.5, 0.3)), ('VonMises', (-2.5, 8.0)), ('VonMises', (0.0, 300.0)),
              ('TruncatedNormal', (0.0, 1.0, -1.0, 2.0)), ('TruncatedNormal', (3.0, 0.5, -1.0, 1.0)),
              ('TruncatedNormal', (0.0, 1.0, 3.99, 5.0))]      # (the last interval below the switch to Robert's tail sampler)


@pytest.mark.parametrize('name,p', CONTINUOUS, ids=['%s%s' % c for c in CONTINUOUS])
def test_continuous_sampler_ks_and_moments(ops, name, p):
    v = draw(ops, KIND[name], p).cpu()
    assert not torch.isnan(v).any() and torch.isfinite(v).all()
    xs, _ = torch.sort(v)
    # the draws are fp32 roundings of the true variates: X rounds to x when it falls between the midpoints to x's fp32
    # neighbours, so P(X_fp32 <= x) = F(upper midpoint) and P(X_fp32 < x) = F(lower midpoint) - this keeps the point masses
    # of rounding (Beta(1, 0.2) at 1.0, Gamma(0.05) below the smallest denormal at 0) out of the distance
    x32 = xs.numpy()
    up = 0.5 * (x32.astype(np.float64) + np.nextafter(x32, np.float32(np.inf)).astype(np.float64))
    lo = 0.5 * (x32.astype(np.float64) + np.nextafter(x32, np.float32(-np.inf)).astype(np.float64))
    F_up = cdf64(name, p, torch.from_numpy(up))
    F_lo = cdf64(name, p, torch.from_numpy(lo))
    n = xs.numel()
    i = torch.arange(1, n + 1, dtype=torch.float64)
    D = max(float((i / n - F_up).max()), float((F_lo - (i - 1) / n).max()))
    assert D < 2.5 / math.sqrt(n), (name, p, D)
    mom = moments64(name, p)
    if mom is not None:
        m, var = mom
        se = math.sqrt(var / n)
        assert abs(float(v.double().mean()) - m) < 6 * se + 1e-6 * abs(m), (name, p, float(v.double().mean()), m)
        if name != 'LogNormal':      # (heavy tail: the variance estimate itself is too noisy for a tight bound)
            assert float(v.double().var()) == pytest.approx(var, rel=0.02, abs=1e-12), (name, p)


DISCRETE = [('Poisson', (0.3,)), ('Poisson', (4.0,)), ('Poisson', (25.0,)), ('Poisson', (3000.0,)),
            ('Poisson', (9.999,)), ('Poisson', (10.0,)), ('Binomial', (40.0, 0.25)),      # (either side of the regime switches)
            ('Binomial', (10.0, 0.3)), ('Binomial', (1000.0, 0.005)), ('Binomial', (200.0, 0.4)), ('Binomial', (5000.0, 0.97)),
            ('Bernoulli', (0.3,))]


@pytest.mark.parametrize('name,p', DISCRETE, ids=['%s%s' % c for c in DISCRETE])
def test_discrete_sampler_chi_square_and_moments(ops, name, p):
    if name == 'Binomial':
        n_, pr = p
        par = (n_, math.log(pr) - math.log1p(-pr))
    else:
        par = p
    v = draw(ops, KIND[name], par).cpu().double()
    assert not torch.isnan(v).any()
    assert torch.equal(v, torch.floor(v)) and float(v.min()) >= 0
    k = np.arange(0, int(v.max()) + 1, dtype=np.float64)
    if name == 'Poisson':
        lam = p[0]
        pmf = np.exp(k * math.log(lam) - lam - _lgamma(k + 1))
        m, var = lam, lam
    elif name == 'Binomial':
        n_, pr = p
        assert float(v.max()) <= n_
        pmf = np.exp(_lgamma(n_ + 1) - _lgamma(k + 1) - _lgamma(n_ - k + 1) + k * math.log(pr) + (n_ - k) * math.log1p(-pr))
        m, var = n_ * pr, n_ * pr * (1 - pr)
    else:
        pmf = np.array([1 - p[0], p[0]])[:len(k)]
        m, var = p[0], p[0] * (1 - p[0])
    counts = np.bincount(v.long().numpy(), minlength=len(k)).astype(np.float64)
    full = pmf / pmf.sum() if name == 'Bernoulli' else pmf
    assert chi2_p(counts, full) > 1e-5, (name, p)
    n = v.numel()
    assert abs(float(v.mean()) - m) < 6 * math.sqrt(var / n), (name, p)
    assert float(v.var()) == pytest.approx(var, rel=0.02), (name, p)


def test_categorical_draws(ops):
    probs = _vec([0.2, 0.5, 0.1, 0.2])
    out = torch.empty(N_DRAWS, dtype=torch.float32, device=DEV)
    ops.dist_draw(5, [probs, None, None, None], [0, 4, 0, 0], None, out, 3, 0, 9)
    counts = np.bincount(out.long().cpu().numpy(), minlength=4).astype(np.float64)
    assert len(counts) == 4
    assert chi2_p(counts, np.array([0.2, 0.5, 0.1, 0.2])) > 1e-5


# ---- counters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,p', [('Gamma', (0.7, 2.0)), ('Binomial', (300.0, 0.2)), ('VonMises', (0.0, 2.0)),
                                    ('TruncatedNormal', (0.0, 1.0, 0.5, 3.0)), ('Poisson', (50.0,)), ('Beta', (0.3, 0.4, 0.0, 1.0))])
def test_counters_rows_and_offsets(ops, name, p):
    kind = KIND[name]
    n = 100000
    a = draw(ops, kind, p, n=n, seed=99, stream=3)
    b = draw(ops, kind, p, n=n, seed=99, stream=3)
    assert torch.equal(a, b)
    assert not torch.equal(a, draw(ops, kind, p, n=n, seed=99, stream=4))
    rows = torch.nonzero(torch.rand(n, device=DEV) < 0.4).reshape(-1)
    r = draw(ops, kind, p, n=n, seed=99, stream=3, rows=rows)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[rows] = True
    assert torch.equal(r[mask], a[mask])
    assert bool((r[~mask] == -7.0).all())          # unlisted rows untouched
    # counter = offset + particle: the second half of a call is a call of its own with offset n / 2
    h = draw(ops, kind, p, n=n // 2, seed=99, stream=3, offset=n // 2)
    assert torch.equal(h, a[n // 2:])


def test_normal_uniform_bit_identical_to_prior_draw(ops):
    n = 300000
    for kind, p in ((0, (torch.randn(n), torch.rand(n) + 0.1)), (1, (-2.0, 5.0)), (0, (1.0, 2.0))):
        p0, p1 = _vec(p[0]), _vec(p[1])
        ref = ops.prior_draw(kind, p0, p1, n, 77, 1000, 5)
        got = draw(ops, kind, (p0, p1), n=n, seed=77, offset=1000, stream=5)
        assert torch.equal(ref, got)


def test_bad_parameters_give_nan_not_a_hang(ops):
    for name, p in (('Gamma', (-1.0, 1.0)), ('Binomial', (2.5, 0.0)), ('VonMises', (0.0, -1.0)),
                    ('TruncatedNormal', (0.0, 1.0, 1.0, -1.0)), ('TruncatedNormal', (0.0, -1.0, 0.0, 1.0))):
        v = draw(ops, KIND[name], p, n=4096)
        torch.cuda.synchronize()
        assert torch.isnan(v).all(), (name, p)


@pytest.mark.parametrize('p', [(0.0, 1.0, 30.0, 31.0), (0.0, 1.0, -31.0, -30.0), (2.0, 0.5, 4.5, 4.6), (1.0, 2.0, 10.0, 40.0),
                               (-1.0, 1.0, -9.0, -5.0),
                               (0.0, 1.0, 6.0, 6.1), (0.0, 1.0, -6.1, -6.0)])      # (narrower than 1 / lambda: the uniform proposal)
def test_truncated_normal_far_tails(ops, p):
    """Intervals entirely beyond 4 standard deviations (Robert's tail sampler): finite draws inside [low, high] that follow
    the float64 CDF (written with erfc: the tail masses are ~1e-197 at 30 sigma)."""
    mu, sd, lo, hi = p
    v = draw(ops, 13, p).cpu()
    assert torch.isfinite(v).all() and float(v.min()) >= lo and float(v.max()) <= hi
    x32 = torch.sort(v)[0].numpy()
    up = 0.5 * (x32.astype(np.float64) + np.nextafter(x32, np.float32(np.inf)).astype(np.float64))
    lo_m = 0.5 * (x32.astype(np.float64) + np.nextafter(x32, np.float32(-np.inf)).astype(np.float64))
    a, b = (lo - mu) / sd, (hi - mu) / sd
    sign = 1.0 if a > 0 else -1.0          # work in the tail's own coordinates: Q(t) = erfc(t / sqrt 2) / 2 of |t|

    def F(x):
        t = torch.from_numpy((x - mu) / sd)
        q = lambda z: 0.5 * torch.special.erfc(sign * torch.as_tensor(z, dtype=torch.float64) / math.sqrt(2))  # noqa: E731
        if sign > 0:
            return ((q(a) - q(t)) / (q(a) - q(b))).clamp(0, 1)
        return ((q(t) - q(a)) / (q(b) - q(a))).clamp(0, 1)
    n = x32.size
    i = torch.arange(1, n + 1, dtype=torch.float64)
    D = max(float((i / n - F(up)).max()), float((F(lo_m) - (i - 1) / n).max()))
    assert D < 2.5 / math.sqrt(n), (p, D)
