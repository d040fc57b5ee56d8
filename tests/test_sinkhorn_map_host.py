"""The float64 numpy route of Empirical.sinkhorn(transport=True) (empirical_host._host_sinkhorn_map) - the comparator of
tests/test_gpu_sinkhorn_map.py - against a dense, unchunked restatement of the definition in include/pyprob_amd.h in numpy.longdouble, the
operator's symbols, and the method through the host route. No GPU. The tolerance is the project's rule (tests/test_gpu_twosample.py): 16
times the distance of the SAME dense restatement in float64 from the long-double one, never below 64 ulp of fp64. All of it fails
without the feature: the parent has neither the symbol, the function nor the keyword."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g, real):
    """(map_ab, map_ba, log_mass_a, log_mass_b, plan) on the counted particles, every matrix dense, in `real`; plan = P_ij."""
    keep = [np.isfinite(lw) & np.isfinite((x - center) / scale).all(1) for lw, x in ((lw_a, x_a), (lw_b, x_b))]
    z = [((x[k].astype(real) - center.astype(real)) / scale.astype(real)) for x, k in ((x_a, keep[0]), (x_b, keep[1]))]
    w = [np.exp(lw[k].astype(real) - lw[k].max()) / np.exp(lw[k].astype(real) - lw[k].max()).sum() for lw, k in ((lw_a, keep[0]), (lw_b, keep[1]))]
    pot = [f[keep[0]].astype(real), g[keep[1]].astype(real)]
    C = ((z[0][:, None, :] - z[1][None, :, :]) ** 2).sum(-1) / 2
    out = []
    for q, s, cost in ((0, 1, C), (1, 0, C.T)):
        k = w[s][None, :] * np.exp((pot[s][None, :] - cost) / real(eps))
        out.append((center + scale * ((k @ z[s]) / k.sum(1)[:, None]), pot[q] / real(eps) + np.log(k.sum(1))))
    plan = w[0][:, None] * w[1][None, :] * np.exp((pot[0][:, None] + pot[1][None, :] - C) / real(eps))
    return out[0][0], out[1][0], out[0][1], out[1][1], plan, keep


def _tolerance(d64, dL):
    return max(16 * float(np.abs(d64.astype(np.longdouble) - dL).max()), 64 * float(np.spacing(np.float64(np.abs(dL).max()))))


def test_the_operator_is_declared_prototyped_built_and_exported():
    from pyprob_amd import build as B, lib as L
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    for name in ('pp_is_sinkhorn_map_groups', 'pp_is_sinkhorn_map_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in L.PROTOTYPES and hasattr(L.load(), name)
    assert 'is_sinkhorn_map.hip' in B.SOURCES and L.load().pp_abi_version() == 15 == L.PP_ABI_VERSION
    assert L.load().pp_is_sinkhorn_map_workspace_bytes(2, 600, 129, 8) > 0 == L.load().pp_is_sinkhorn_map_workspace_bytes(2, 600, 129, 9)


@pytest.mark.parametrize('na,nb,J', [(1, 1, 1), (37, 300, 2), (300, 37, 8)])
def test_host_map_is_the_dense_definition(na, nb, J):
    from pyprob_amd.empirical_host import _host_sinkhorn_map
    rng = np.random.default_rng(na + J)
    center, scale, eps = rng.uniform(-1, 1, J), rng.uniform(0.5, 2.0, J), 0.1 * J
    x_a, x_b = center + scale * rng.standard_normal((na, J)), center + scale * (0.5 + rng.standard_normal((nb, J)))
    lw_a, lw_b, f, g = -3.0 * rng.random(na), -3.0 * rng.random(nb), eps * rng.uniform(-5, 5, na), eps * rng.uniform(-5, 5, nb)
    if na > 1:
        lw_a[2], x_a[5, 0], f[2], lw_b[7], x_b[3, J - 1], g[3] = -np.inf, np.nan, np.nan, -np.inf, np.nan, np.nan
    got = _host_sinkhorn_map(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g)
    d64, dL = (_dense(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g, real) for real in (np.float64, np.longdouble))
    for k, (out, keep) in enumerate(zip(got, (dL[5][0], dL[5][1]) * 2)):
        assert np.isnan(out[~keep]).all() and keep.sum() == (len(keep) - 2 if na > 1 else 1)
        assert np.abs(out[keep] - dL[k]).max() <= _tolerance(d64[k], dL[k]), k
    # an empty side: every row is NaN
    empty = _host_sinkhorn_map(np.full(na, -np.inf), x_a, lw_b, x_b, center, scale, eps, f, g)
    assert all(np.isnan(t).all() for t in empty) and empty[1].shape == (nb, J)


def _vector_posterior(x, lw):
    from pyprob_amd.distributions import Empirical
    return Empirical(values=[torch.tensor(v) for v in x], log_weights=[float(a) for a in lw])


def test_the_method_carries_the_maps_and_a_shifted_cloud_moves_by_its_shift(monkeypatch):
    """Cloud b is cloud a moved by d, equal weights: with the row marginals exact (the last update is f's) the weighted mean of map_ab - x_a
    is d + sum_j (column mass_j - b_j) (x'_j - c) for any c. The tolerance is that sum's bound at the returned potentials, taken in long
    double, plus the rounding rule above: the analytic value has none of its own."""
    from pyprob_amd import ops as P
    monkeypatch.setattr(P, 'ops', None)          # (the host route must not reach for an operator)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    rng = np.random.default_rng(5)
    n, d = 120, np.array([1.0, -0.5])
    x = rng.standard_normal((n, 2))
    a, b = _vector_posterior(x, np.zeros(n)), _vector_posterior(x + d, np.zeros(n))
    plain = a.sinkhorn(b, epsilon=0.1, tol=1e-9, max_iter=20000)
    assert plain.map_ab is plain.map_ba is plain.log_mass_a is plain.log_mass_b is None and all(plain.converged)
    with pytest.raises(ValueError, match='transport=True'):
        plain.displacement()
    r = a.sinkhorn(b, epsilon=0.1, tol=1e-9, max_iter=20000, transport=True)
    assert (r.ot_ab, r.n_iter) == (plain.ot_ab, plain.n_iter) and np.array_equal(r.f, plain.f)
    assert r.map_ab.shape == (n, 2) == r.map_ba.shape and r.log_mass_a.shape == (n,) == r.log_mass_b.shape
    disp = r.displacement()
    assert np.array_equal(disp[0], r.map_ab - x) and np.array_equal(disp[1], r.map_ba - (x + d))
    d64, dL = (_dense(np.zeros(n), x, np.zeros(n), x + d, r.center, r.scale, r.epsilon, r.f, r.g, real) for real in (np.float64, np.longdouble))
    tol = _tolerance(d64[0], dL[0])
    assert np.abs(r.map_ab - dL[0]).max() <= tol and np.abs(r.log_mass_a).max() <= _tolerance(d64[2], dL[2]) + np.abs(dL[2]).max()
    slack = float((np.abs(dL[4].sum(0) - np.longdouble(1) / n)[:, None] * np.abs(x + d - r.center)).sum(0).max())
    assert slack < 1e-6 and np.abs(disp[0].mean(0) - d).max() <= slack + tol + float(np.abs(dL[4].sum(1) * n - 1).max()) * np.abs(dL[0]).max()
