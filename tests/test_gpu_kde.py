"""pp_is_kde_groups / pp_is_kde2d_groups (csrc/is_kde.hip), Empirical.kde / kde2d and pyprob_amd.kde_batch on the device, against a
float64 numpy broadcast. The bound is the one derived at the head of csrc/is_kde.hip (u = 2^-24; a = the exponent of a term):
    sum_i wbar_i k_i expm1((9 |a_i| + c2) u + sum_axes sqrt(2 |a|) (|p| / h) 2^-48) / norm
        + (4 n + 16) 2^-53 density + (4 + 4 n) 2^-126 / norm,      c2 = 259 (1-D: fp32 sub-tile of 256), 4103 (2-D: MFMA over a tile)
computed per point from the reference itself. PP_KDE_ERRORS=<file> appends every case's largest error / bound ratio
(profiles/kde_errors.jsonl). All of it fails without the feature: the parent has neither the symbols nor the methods."""
import json
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

DEV = 'cuda:0'
U = 2.0 ** -24
_trapz = getattr(np, 'trapezoid', None) or np.trapz


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _data(M, n, seed, kind='plain'):
    """lw [M, n], x and y [M, n] in float32: two modes, one particle in seven without a weight, one in eleven with a NaN value."""
    rng = np.random.default_rng(seed)
    lw = (2.0 * rng.standard_normal((M, n))).astype(np.float32)
    x = np.where(rng.random((M, n)) < 0.3, -2.0, 1.0) + 0.5 * rng.standard_normal((M, n))
    y = 0.5 * x + 0.3 * rng.standard_normal((M, n))
    if kind == 'narrow':
        x = 1000.0 + 1e-2 * rng.standard_normal((M, n))
    x, y = x.astype(np.float32), y.astype(np.float32)
    i = np.arange(n)
    if n > 2:
        lw[:, i % 7 == 3] = -np.inf
        x[:, i % 11 == 5] = np.nan
        y[:, i % 13 == 6] = np.nan
    if kind == 'one':       # all weight on one particle: the others underflow in float64 or have none
        lw[:] = np.where(i % 2 == 0, -2000.0, -np.inf)
        lw[:, n // 2] = 0.0
        x[:, n // 2], y[:, n // 2] = 0.25, -0.5
    return lw, x, y


def _ref(lw, cols, pts, hs, c2):
    """(density, bound) of one group in float64: cols / pts / hs hold one entry per axis; the result has one dimension per axis."""
    keep = np.isfinite(lw) & ~np.any([np.isnan(c) for c in cols], axis=0)
    w = np.exp(lw[keep].astype(np.float64) - lw[np.isfinite(lw)].max())
    n, J = len(lw), len(cols)
    shape = lambda j, a: a.reshape([-1 if k == j else 1 for k in range(J)] + [1])      # noqa: E731
    a = [-0.5 * ((shape(j, pts[j]) - cols[j][keep].astype(np.float64)) / hs[j]) ** 2 for j in range(J)]
    A = sum(a)
    term = np.exp(A) * (w / w.sum())
    with np.errstate(over='ignore'):          # (a term that is 0 in float64 has an exponent beyond expm1's range: it carries no error)
        rel = np.expm1((9.0 * np.abs(A) + c2) * U +
                       sum(np.sqrt(2.0 * np.abs(a[j])) * np.abs(shape(j, pts[j])) / hs[j] for j in range(J)) * 2.0 ** -48)
    norm = np.prod([h * np.sqrt(2.0 * np.pi) for h in hs])
    dens = term.sum(-1) / norm
    return dens, np.where(term > 0, term * np.where(term > 0, rel, 0.0), 0.0).sum(-1) / norm + (4 * n + 16) * 2.0 ** -53 * dens + (4 + 4 * n) * 2.0 ** -126 / norm


def _check(label, got, lw, cols, pts, hs, c2):
    """got [2, ...] (density | log density) of one group against the reference and its bound."""
    dens, bound = _ref(lw, cols, pts, hs, c2)
    err = np.abs(got[0] - dens)
    rec = dict(case=label, n=len(lw), points=list(dens.shape), max_err=float(err.max()), max_density=float(dens.max()),
               worst_ratio=float((err / bound).max()))
    print('kde', json.dumps(rec))
    if os.environ.get('PP_KDE_ERRORS'):
        with open(os.environ['PP_KDE_ERRORS'], 'a') as f:
            f.write(json.dumps(rec) + '\n')
    assert not np.isnan(got).any() and (err <= bound).all(), rec
    with np.errstate(divide='ignore'):
        assert np.allclose(got[1], np.log(got[0]), rtol=1e-15, atol=0) and (got[1][got[0] == 0] == -np.inf).all()


CASES_1D = [(n, Q, 'plain') for n in (1, 2, 63, 2048, 2049, 5000) for Q in (1, 7, 64, 257)] + \
           [(2049, 513, 'plain'), (2049, 1025, 'plain'), (63, 4096, 'plain'),       # the edges of P = 2 and P = 4, the largest Q
            (300, 64, 'one'), (5000, 64, 'one'), (2049, 257, 'narrow'), (300, 7, 'far')]


@pytest.mark.parametrize('n,Q,kind', CASES_1D)
def test_kde_operator_against_float64(n, Q, kind):
    from pyprob_amd import ops as P
    M = 2
    lw, x, _ = _data(M, n, 1000 * n + Q, kind)
    h = np.array([2e-3, 3e-3]) if kind == 'narrow' else np.array([0.21, 0.4])
    lo, hi = (999.95, 1000.05) if kind == 'narrow' else (-4.5, 3.5)
    pts = np.stack([np.linspace(lo, hi + 0.1 * g, Q) for g in range(M)]) if Q > 1 else np.array([[0.3], [-1.9]])
    if kind == 'far':
        pts = np.array([[-1e6, 1e6, 3e38, -3e38, 1e4, -1e4, 2e5]] * M)
    got = P.ops.is_kde_groups(_dev(lw.reshape(-1)), _dev(x.reshape(-1)), n, _dev(pts), _dev(h), None).cpu().numpy()
    for g in range(M):
        _check('1d %s' % kind, got[:, g], lw[g], [x[g]], [pts[g]], [h[g]], 259.0)
    if kind == 'far':
        assert (got[0] == 0).all() and (got[1] == -np.inf).all()
    if kind == 'narrow':
        assert got[0].max() > 10.0          # (the density of a posterior of width 1e-2 survives at 1000)


@pytest.mark.parametrize('grid', [(32, 32), (33, 17), (64, 64), (1, 5)])
@pytest.mark.parametrize('n', [1, 63, 2048, 2049, 5000])
def test_kde2d_operator_against_float64(grid, n):
    from pyprob_amd import ops as P
    M = 2
    lw, x, y = _data(M, n, 77 * n + grid[0])
    hx, hy = np.array([0.3, 0.45]), np.array([0.2])
    px = np.stack([np.linspace(-4.0, 3.0 + g, grid[0]) for g in range(M)])
    py = np.linspace(-2.5, 2.0, grid[1])
    got = P.ops.is_kde2d_groups(_dev(lw.reshape(-1)), _dev(x.reshape(-1)), _dev(y.reshape(-1)), n, _dev(px), _dev(py), _dev(hx), _dev(hy),
                                None).cpu().numpy()
    for g in range(M):
        _check('2d', got[:, g], lw[g], [x[g], y[g]], [px[g], py], [hx[g], hy[0]], 4103.0)


@pytest.mark.parametrize('n', [300, 5000])
def test_groups_and_repeated_calls_give_the_same_bits(n):
    from pyprob_amd import ops as P
    M, Q = 3, 70
    lw, x, y = _data(M, n, 5)
    pts, h = np.stack([np.linspace(-4.0, 3.0 + g, Q) for g in range(M)]), np.array([0.2, 0.3, 0.25])
    L, X, Y = (_dev(a.reshape(-1)) for a in (lw, x, y))
    stats = torch.zeros((M, 6), dtype=torch.float64, device=DEV)
    stats[:, 0] = _dev(np.where(np.isfinite(lw), lw, -np.inf).max(1).astype(np.float64))      # (the maximum a caller hands over)
    one = P.ops.is_kde_groups(L, X, n, _dev(pts), _dev(h), None).cpu().numpy()
    two = P.ops.is_kde2d_groups(L, X, Y, n, _dev(pts), _dev(pts[0, :33]), _dev(h), _dev(h[:1]), None).cpu().numpy()
    assert np.array_equal(one.view(np.int64), P.ops.is_kde_groups(L, X, n, _dev(pts), _dev(h), stats).cpu().numpy().view(np.int64))
    assert np.array_equal(two.view(np.int64), P.ops.is_kde2d_groups(L, X, Y, n, _dev(pts), _dev(pts[0, :33]), _dev(h), _dev(h[:1]),
                                                                   stats).cpu().numpy().view(np.int64))
    for g in range(M):
        s = slice(g * n, (g + 1) * n)
        a = P.ops.is_kde_groups(L[s], X[s], n, _dev(pts[g]), _dev(h[g:g + 1]), None).cpu().numpy()
        b = P.ops.is_kde2d_groups(L[s], X[s], Y[s], n, _dev(pts[g]), _dev(pts[0, :33]), _dev(h[g:g + 1]), _dev(h[:1]), None).cpu().numpy()
        assert np.array_equal(a[:, 0].view(np.int64), one[:, g].view(np.int64))
        assert np.array_equal(b[:, 0].view(np.int64), two[:, g].view(np.int64))


def _same(a, b):
    return all(np.array_equal(getattr(a, f).view(np.int64), getattr(b, f).view(np.int64)) for f in ('x', 'density', 'log_density')) and \
        (a.bandwidth, a.count, a.ess, a.mode) == (b.bandwidth, b.count, b.ess, b.mode)


def test_kde_batch_is_one_operator_call_and_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from test_gpu_density_joint import _two_statement_model
    model, M, N = _two_statement_model(), 3, 300
    rng = np.random.default_rng(3)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    count, real = [0], P.ops.is_kde_groups

    def counted(*a):
        count[0] += 1
        return real(*a)
    monkeypatch.setattr(P.ops, 'is_kde_groups', counted, raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
    assert model._batch_ok is True and len(posts) == M
    shared, own = np.linspace(-3.0, 5.0, 40), np.stack([np.linspace(-3.0, 5.0 + g, 40) for g in range(M)])
    for kw, each in ((dict(x=shared, bandwidth=0.3), lambda g: dict(x=shared, bandwidth=0.3)),
                     (dict(x=own, bandwidth=[0.2, 0.3, 0.4]), lambda g: dict(x=own[g], bandwidth=[0.2, 0.3, 0.4][g])),
                     (dict(grid=65), lambda g: dict(grid=65)), (dict(grid=33, address='a'), None)):
        before = count[0]
        fast = pyprob_amd.kde_batch(posts, **kw)
        assert count[0] == before + 1 and len(fast) == M
        loop = [p.kde(**each(g)) if each else p.marginal('a').kde(grid=33) for g, p in enumerate(posts)]
        assert all(_same(a, b) and a.count == N for a, b in zip(fast, loop))
    assert len({f.bandwidth for f in fast}) == M          # the groups see different observations


def test_kde_on_a_lock_step_posterior_against_the_host_route():
    from pyprob_amd.empirical_host import _host_kde, _host_kde2d
    from pyprob_amd.state import InferenceEngine
    from test_gpu_density_joint import _two_statement_model
    model, N = _two_statement_model(), 4097
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(N, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe={'obs0': 2.0, 'obs1': 1.5},
                                       lock_step=True, seed=13, offset=64)
        smoothed = post.psis()
    for name, e in (('post', post), ('marginal', post.marginal('a')), ('psis', smoothed)):
        h = e.kde().bandwidth
        lw, x = e._log_weights.cpu().numpy(), e._values.cpu().numpy()
        assert h == pytest.approx(0.9 * min(e.stddev, np.subtract(*e.quantile([0.75, 0.25])) / 1.34) * e.effective_sample_size ** -0.2)
        # a grid 8 h beyond the particles at a step of h / 4: the trapezoid rule of a Gaussian mixture of width h at that step is exact
        # to exp(-2 pi^2 (h / step)^2) = e^-315, the mass outside 2 Phi(-8) = 1.3e-15; what is left is the kernel's own bound
        grid = np.arange(x.min() - 8 * h, x.max() + 8 * h, h / 4)[:4096]
        k = e.kde(grid, bandwidth=h)
        assert k.count == N and len(grid) < 4096 and k.x[0] == grid[0]
        _check('public ' + name, np.stack([k.density, k.log_density]), lw, [x], [grid], [h], 259.0)
        bound = _ref(lw, [x], [grid], [h], 259.0)[1]
        assert abs(_trapz(k.density, grid) - 1.0) <= _trapz(bound, grid) + 1e-14
        assert (np.abs(k.density - _host_kde(lw.astype(np.float64), x.astype(np.float64), grid, h)[0]) <= 2 * bound).all()
    two = post.kde2d('a', 'b')
    cols = [rec[0].cpu().numpy() for entry in post.statement_log for rec in entry.values()]
    lw = post._all_lw().cpu().numpy()
    moments = post.joint(['a', 'b'])
    assert two.bandwidth == pytest.approx(tuple(moments.stddev * moments.ess ** (-1.0 / 6.0))) and two.density.shape == (64, 64)
    assert two.x[0] == pytest.approx(cols[0].min() - 3 * two.bandwidth[0]) and two.count == N
    _check('public 2d', np.stack([two.density, two.log_density]), lw, cols, [two.x, two.y], two.bandwidth, 4103.0)
    host = _host_kde2d(lw.astype(np.float64), cols[0].astype(np.float64), cols[1].astype(np.float64), two.x, two.y, *two.bandwidth)
    assert (np.abs(two.density - host[0]) <= 2 * _ref(lw, cols, [two.x, two.y], two.bandwidth, 4103.0)[1]).all()
    # the grid ends 3 h beyond the particles: at most 2 Phi(-3) of the mass of the end particles lies outside, per axis
    wide = post.kde2d('a', 'b', grid=256, range=((cols[0].min() - 8 * two.bandwidth[0], cols[0].max() + 8 * two.bandwidth[0]),
                                                 (cols[1].min() - 8 * two.bandwidth[1], cols[1].max() + 8 * two.bandwidth[1])))
    step = (wide.x[1] - wide.x[0]) / wide.bandwidth[0], (wide.y[1] - wide.y[0]) / wide.bandwidth[1]
    assert max(step) < 1.0          # (the trapezoid error exp(-2 pi^2 / step^2) < 3e-9 per axis)
    # the bound integrates to (9 E|a| + 4103) u with E|a| = 1/2 per axis; 1 % for the second order of expm1
    assert abs(_trapz(_trapz(wide.density, wide.y), wide.x) - 1.0) <= 2 * 3e-9 + 1.01 * (9.0 + 4103.0) * U
