"""pp_is_sinkhorn_map_groups (csrc/is_sinkhorn_map.hip) and Empirical.sinkhorn(transport=True) on the device against the float64 numpy
definition (empirical_host._host_sinkhorn_map) evaluated at the SAME potentials. The bound is the one derived at the head of
csrc/is_sinkhorn_map.hip, per direction (u = 2^-24, K = J + 2 rounded up to even, alpha^2 = log2(e) / eps, R_s, R_q the largest |z| of the
summed and the query side, L_max the largest log2(e) |lw - max| and F_max the largest log2(e) |pot| / eps of the summed side):
    S = alpha^2 (R_s^2 + R_q^2 + R_s R_q) + L_max + F_max,   e = expm1(ln 2 (2 K + 12) S u) + 650 u + (n + 64) 2^-52 + n 2^-124
    |map_j - exact| <= scale_j 2 e R_s / (1 - e) + 2^-50 (|center_j| + scale_j R_s)
    |log_mass - exact| <= -log1p(-e) + 2^-50 (log2(e) |pot_q| / eps + S)
PP_SINKHORN_MAP_ERRORS=<file> appends every case's worst error / bound ratio (profiles/sinkhorn_map_errors.jsonl). All of it fails
without the feature: the parent has neither the symbol nor the keyword."""
import json
import os
import warnings

import numpy as np
import pytest

from test_gpu_sinkhorn import _dev, _side

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

U, LOG2E = 2.0 ** -24, 1.4426950408889634


def _op(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g):
    """One pp_is_sinkhorn_map_groups call on host arrays lw [M, n], x [M, n, J] (float32), center / scale [M, J], eps [M], f, g [M, n]."""
    from pyprob_amd import ops as P
    side = lambda lw, x: (_dev(lw.reshape(-1)), [_dev(x[:, :, j].reshape(-1)) for j in range(x.shape[2])], lw.shape[1], None)  # noqa: E731
    out = P.ops.is_sinkhorn_map_groups(*side(lw_a, x_a), *side(lw_b, x_b), _dev(center), _dev(1.0 / scale), _dev(eps), _dev(f), _dev(g),
                                       True, True)
    return [t.cpu().numpy() for t in out]


def _bounds(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g):
    """(bound on map_ab [J], on map_ba [J], on log_mass_a [n_a], on log_mass_b [n_b], the larger e) of one group."""
    K, n, side = (x_a.shape[1] + 3) & ~1, max(len(lw_a), len(lw_b)), []
    for lw, x, pot in ((lw_a, x_a, f), (lw_b, x_b, g)):
        z = (x.astype(np.float64) - center) / scale
        keep = np.isfinite(lw) & np.isfinite(z).all(1)
        side.append((np.sqrt((z[keep] ** 2).sum(1)).max(), LOG2E * np.abs(lw[keep].astype(np.float64) - lw[np.isfinite(lw)].max()).max(),
                     LOG2E * np.abs(np.where(keep, pot, 0.0)) / eps))
    maps, masses, es = [], [], []
    for (Rq, _, Fq), (Rs, Ls, Fs) in ((side[0], side[1]), (side[1], side[0])):
        S = LOG2E / eps * (Rs * Rs + Rq * Rq + Rs * Rq) + Ls + Fs.max()
        e = np.expm1(np.log(2.0) * (2 * K + 12) * S * U) + 650 * U + (n + 64) * 2.0 ** -52 + n * 2.0 ** -124
        maps.append(scale * 2 * e * Rs / (1 - e) + 2.0 ** -50 * (np.abs(center) + scale * Rs))
        masses.append(-np.log1p(-e) + 2.0 ** -50 * (Fq + S))
        es.append(e)
    return maps[0], maps[1], masses[0], masses[1], max(es)


def _ratios(got, want, bounds):
    """The worst error / bound ratio of each of the four outputs of one group; NaN rows exactly where the definition has them."""
    assert all(np.array_equal(np.isnan(a), np.isnan(b)) for a, b in zip(got, want))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # (an all-NaN output has no worst element)
        return [float(np.nan_to_num(np.nanmax(np.abs(a - b) / bound))) for a, b, bound in zip(got, want, bounds)]


def _record(rec):
    print('sinkhorn_map', json.dumps(rec))
    if os.environ.get('PP_SINKHORN_MAP_ERRORS'):
        with open(os.environ['PP_SINKHORN_MAP_ERRORS'], 'a') as f:
            f.write(json.dumps(rec) + '\n')


def _same_bits(a, b):
    return all(np.array_equal(u.view(np.int64), v.view(np.int64)) for u, v in zip(a, b))


@pytest.mark.parametrize('J', [1, 2, 8])
@pytest.mark.parametrize('na,nb', [(1, 1), (33, 257), (129, 600), (600, 129)])
def test_maps_and_masses_stay_within_the_derived_bound(na, nb, J):
    from pyprob_amd.empirical_host import _host_sinkhorn_map
    rng = np.random.default_rng(1000 * na + 10 * J)
    center, scale, eps = rng.uniform(-2.0, 2.0, (2, J)), rng.uniform(0.5, 2.0, (2, J)), np.array([0.05 * J, 0.08 * J])
    (lw_a, x_a), (lw_b, x_b) = ([np.stack(t) for t in zip(*[_side(rng, n, J, center[k], scale[k], s) for k in range(2)])]
                                for n, s in ((na, 0.0), (nb, 0.5 / np.sqrt(J))))
    # generated potentials, up to 150 eps, NaN where a particle does not count (from five particles on: _side drops two)
    f, g = (eps[:, None] * rng.uniform(-150.0, 150.0, (2, n)) for n in (na, nb))
    for pot, n in ((f, na), (g, nb)):
        if n >= 5:
            pot[:, [1, n - 2]] = np.nan
    got = _op(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g)
    worst = []
    for k in range(2):
        args = (lw_a[k], x_a[k], lw_b[k], x_b[k], center[k], scale[k], eps[k], f[k], g[k])
        want, bounds = _host_sinkhorn_map(*args), _bounds(*args)
        assert [int(np.isnan(w.reshape(len(w), -1)).any(1).sum()) for w in want] == [2 * (na >= 5), 2 * (nb >= 5)] * 2
        assert bounds[4] < 1e-2, bounds[4]      # (a looser derivation is not a test)
        worst.append(_ratios([t[k] for t in got], want, bounds[:4]))
        s = slice(k, k + 1)      # group k of the two-group call carries the bits of its own call
        assert _same_bits([t[k] for t in got], [t[0] for t in _op(lw_a[s], x_a[s], lw_b[s], x_b[s], center[s], scale[s], eps[s], f[s], g[s])])
    _record(dict(case='%d x %d, J = %d' % (na, nb, J), worst_ratio=dict(zip(('map_ab', 'map_ba', 'log_mass_a', 'log_mass_b'), np.max(worst, 0).tolist()))))
    assert np.max(worst) <= 1.0, worst
    assert _same_bits(got, _op(lw_a, x_a, lw_b, x_b, center, scale, eps, f, g))      # the same bits again


def test_a_query_forty_units_away_lands_on_the_nearest_particle():
    from pyprob_amd.empirical_host import _host_sinkhorn_map
    rng = np.random.default_rng(40)
    na, nb, J, eps, center, scale = 40, 300, 2, 0.1, np.zeros(2), np.ones(2)
    (lw_a, x_a), (lw_b, x_b) = _side(rng, na, J, center, scale, 0.0), _side(rng, nb, J, center, scale, 0.3)
    x_a[0], x_b[0], lw_b[0] = (40.0, 0.0), (4.5, 0.0), -1.0      # every other b has |z| <= 3.9: half a unit further, 180 / eps in the exponent
    f, g = np.zeros((1, na)), np.zeros((1, nb))
    args = (lw_a, x_a, lw_b, x_b, center, scale, eps, f[0], g[0])
    got = _op(lw_a[None], x_a[None], lw_b[None], x_b[None], center[None], scale[None], np.array([eps]), f, g)
    want, bounds = _host_sinkhorn_map(*args), _bounds(*args)
    ratios = _ratios([t[0] for t in got], want, bounds[:4])
    _record(dict(case='far query 40 x 300, J = 2', worst_ratio=ratios, e=bounds[4], map=got[0][0, 0].tolist(), log_mass=got[2][0, 0]))
    assert np.isfinite(got[0][0, 0]).all() and np.isfinite(got[2][0, 0]) and np.abs(want[0][0] - x_b[0]).max() < 1e-12
    assert (np.abs(got[0][0, 0] - x_b[0]) <= bounds[0]).all() and max(ratios) <= 1.0, ratios


def test_transport_through_the_method_is_the_operator_on_its_own_potentials():
    from pyprob_amd import ops as P
    from test_gpu_density_joint import _two_statement_model
    model = _two_statement_model()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = model.posterior_results_batch(300, [{'obs0': 1.0, 'obs1': 0.5}], seed=13, offset=64)[0]
        b = model.posterior_results_batch(400, [{'obs0': 1.5, 'obs1': 0.0}], seed=14, offset=64)[0]
        r, plain = a.sinkhorn(b, max_iter=50, transport=True), a.sinkhorn(b, max_iter=50)
    assert plain.map_ab is plain.log_mass_a is None and plain.ot_ab == r.ot_ab and torch.equal(plain.f, r.f) and torch.equal(plain.g, r.g)
    (_, lw_a, cols_a, stats_a), (_, lw_b, cols_b, stats_b) = a._pair_columns(None), b._pair_columns(None)
    again = P.ops.is_sinkhorn_map_groups(lw_a, list(cols_a), 300, stats_a, lw_b, list(cols_b), 400, stats_b, _dev(r.center[None]),
                                         _dev(1.0 / r.scale[None]), _dev(np.array([r.epsilon])), r.f[None], r.g[None], True, True)
    assert r.map_ab.shape == (300, 2) and r.map_ba.shape == (400, 2) and r.map_ab.is_cuda and r.log_mass_b.shape == (400,)
    assert all(torch.equal(t[0], u) for t, u in zip(again, (r.map_ab, r.map_ba, r.log_mass_a, r.log_mass_b)))
    x_a = torch.stack(list(cols_a), 1).double()
    assert torch.equal(r.displacement()[0], r.map_ab - x_a) and r.displacement()[1].shape == (400, 2)
    # f is the last update: the row masses are 1 up to the roundings of the half-step that made f and of this pass, each within the bound
    host = lambda lw, cols: (lw.cpu().numpy(), np.stack([c.cpu().numpy() for c in cols], 1))      # noqa: E731
    bounds = _bounds(*host(lw_a, cols_a), *host(lw_b, cols_b), r.center, r.scale, r.epsilon, r.f.cpu().numpy(), r.g.cpu().numpy())
    mass = r.log_mass_a.cpu().numpy()
    _record(dict(case='public 300 x 400, J = 2', worst_ratio=float(np.abs(mass / (2 * bounds[2])).max()), e=bounds[4]))
    assert (np.abs(mass) <= 2 * bounds[2]).all() and bounds[4] < 1e-2
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        drawn = b.sinkhorn(a, num_samples=500, seed=3, max_iter=50, transport=True)
    assert drawn.map_ab.shape == (500, 2) and torch.isfinite(drawn.displacement()[1]).all()
