"""Empirical.kde / kde_batch on the float64 numpy route (empirical_host._host_kde / _host_kde2d: the definitions of pp_is_kde_groups and
pp_is_kde2d_groups), the bandwidth rules, the refusals, and the two entry points in the library, the bindings and the header."""
import math
import os

import numpy as np
import pytest

import pyprob_amd
from pyprob_amd.distributions import Empirical
from pyprob_amd.empirical_host import _host_kde, _host_kde2d

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _particles(n=50, seed=4):
    rng = np.random.default_rng(seed)
    lw, x, y = rng.standard_normal(n), 2.0 * rng.standard_normal(n) + 1.0, rng.standard_normal(n)
    lw[3], x[7] = -np.inf, np.nan           # both skipped
    return lw, x, y


def test_host_route_against_a_double_loop():
    lw, x, y = _particles()
    pts, h, hy = np.linspace(-6.0, 8.0, 9), 0.7, 0.4
    one, two, total = np.zeros(9), np.zeros((9, 3)), 0.0
    for i in range(len(lw)):
        if not math.isfinite(lw[i]) or math.isnan(x[i]):
            continue
        w = math.exp(lw[i] - np.max(lw))
        total += w
        for q in range(9):
            kx = math.exp(-0.5 * ((pts[q] - x[i]) / h) ** 2) / (h * math.sqrt(2.0 * math.pi))
            one[q] += w * kx
            for b in range(3):
                two[q, b] += w * kx * math.exp(-0.5 * ((pts[b] - y[i]) / hy) ** 2) / (hy * math.sqrt(2.0 * math.pi))
    k = Empirical(values=list(x), log_weights=lw).kde(pts, bandwidth=h)
    assert np.allclose(k.density, one / total, rtol=1e-13, atol=0) and np.allclose(k.log_density, np.log(one / total), rtol=1e-13)
    assert k.count == 48 and k.bandwidth == h and k.mode == pts[np.argmax(one)] and np.array_equal(k.x, pts)
    assert np.allclose(_host_kde2d(lw, x, y, pts, pts[:3], h, hy)[0], two / total, rtol=1e-13, atol=0)
    far = _host_kde(lw, x, np.array([1e6]), h)
    assert far[0, 0] == 0.0 and far[1, 0] == -np.inf
    assert Empirical(values=list(x), log_weights=lw).kde(0.5, bandwidth=h).density.shape == (1,)
    both = pyprob_amd.kde_batch([Empirical(values=list(x), log_weights=lw)] * 2, x=np.stack([pts, pts + 1.0]), bandwidth=[h, 2 * h])
    assert np.array_equal(both[0].density, k.density) and both[1].bandwidth == 2 * h and both[1].x[0] == pts[0] + 1.0


def test_bandwidth_rules_and_the_default_grid():
    from pyprob_amd.empirical import _scott, _silverman
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])           # uniform weights: ess 8, stddev sqrt(5.25), quartiles 1 and 5
    e = Empirical(values=list(x), log_weights=np.zeros(8))
    k = e.kde()
    assert k.bandwidth == pytest.approx(0.9 * min(math.sqrt(5.25), 4.0 / 1.34) * 8.0 ** -0.2, rel=1e-14) and k.ess == pytest.approx(8.0)
    assert len(k.x) == 512 and k.x[0] == 0.0 - 3 * k.bandwidth and k.x[-1] == pytest.approx(7.0 + 3 * k.bandwidth, rel=1e-15)
    assert e.kde(grid=5).x.shape == (5,)
    assert _silverman(2.0, (1.0, 1.0), 32.0, 9) == pytest.approx(0.9 * 2.0 * 0.5)          # an IQR of 0 leaves the stddev
    assert _silverman(2.0, (0.0, 1.34), 32.0, 9) == pytest.approx(0.9 * 1.0 * 0.5)
    assert _scott(3.0, 64.0, 9) == pytest.approx(1.5)


def test_density_integrates_to_one():
    lw, x, _ = _particles()
    e = Empirical(values=list(np.where(np.isnan(x), 0.0, x)), log_weights=lw)
    h = e.kde().bandwidth
    # 8 h beyond the particles at a step of h / 4: the trapezoid rule of a mixture of Gaussians of width h is exact to
    # 2 exp(-2 pi^2 (h / step)^2) = 2 e^-315 (Poisson summation), the mass outside is 2 Phi(-8) = 1.3e-15; the rest is float64 rounding
    grid = np.arange(np.nanmin(x) - 8 * h, np.nanmax(x) + 8 * h, h / 4)
    k = e.kde(grid, bandwidth=h)
    step = np.diff(grid)
    assert abs(np.sum(0.5 * (k.density[1:] + k.density[:-1]) * step) - 1.0) <= 1.3e-15 + len(grid) * 2.0 ** -52


@pytest.mark.parametrize('kw', [dict(bandwidth=0.0), dict(bandwidth=-1.0), dict(bandwidth=float('nan')), dict(bandwidth=float('inf')),
                                dict(x=[]), dict(x=np.zeros(4097)), dict(x=[0.0, float('inf')]), dict(x=np.zeros((2, 2))),
                                dict(grid=0), dict(grid=4097), dict(grid=2.5)])
def test_refusals(kw):
    e = Empirical(values=[0.0, 1.0, 3.0], log_weights=np.zeros(3))
    with pytest.raises(ValueError):
        e.kde(**{'bandwidth': 0.5, **kw})


def test_no_spread_names_bandwidth_and_kde2d_needs_the_statement_log():
    for values, lw in (([2.0, 2.0, 2.0], np.zeros(3)), ([1.0, 2.0], np.array([0.0, -np.inf]))):
        with pytest.raises(ValueError, match='bandwidth='):
            Empirical(values=values, log_weights=lw).kde()
        assert Empirical(values=values, log_weights=lw).kde(values[0], bandwidth=0.5).density[0] == pytest.approx(1.0 / (0.5 * math.sqrt(2 * math.pi)))
    with pytest.raises(AttributeError, match='statement log'):
        Empirical(values=[0.0, 1.0], log_weights=np.zeros(2)).kde2d('a', 'b')
    with pytest.raises(ValueError):
        pyprob_amd.kde_batch([Empirical(values=[0.0, 1.0], log_weights=np.zeros(2))] * 2, x=np.zeros((3, 4)), bandwidth=1.0)


def test_entry_points_are_exported_prototyped_and_in_the_header():
    from pyprob_amd import lib as L
    lib = L.load()
    header = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    for name in ('pp_is_kde_groups', 'pp_is_kde2d_groups', 'pp_is_kde_workspace_bytes', 'pp_is_kde2d_workspace_bytes'):
        assert hasattr(lib, name) and name in L.PROTOTYPES and header.count(name + '(') == 1
    assert L.PP_ABI_VERSION == 15 == lib.pp_abi_version() and '#define PP_ABI_VERSION 15' in header
    assert '#define PP_IS_KDE_MAX_POINTS %d' % L.PP_IS_KDE_MAX_POINTS in header
    assert '#define PP_IS_KDE2D_MAX_SIDE %d' % L.PP_IS_KDE2D_MAX_SIDE in header
    assert lib.pp_is_kde_workspace_bytes(3, 2049, 4096) > 3 * 2 * 4096 * 8 and lib.pp_is_kde_workspace_bytes(3, 2049, 4097) == 0
    assert lib.pp_is_kde2d_workspace_bytes(3, 2049, 256, 256) > 0 == lib.pp_is_kde2d_workspace_bytes(3, 2049, 257, 4)
    assert open(os.path.join(REPO, 'INTEGRATION.md')).read().count('pp_abi_version() == 15') == 1
    assert all(hasattr(pyprob_amd, n) for n in ('kde_batch', 'KernelDensity', 'KernelDensity2D'))
