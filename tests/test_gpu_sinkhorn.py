"""pp_is_sinkhorn_groups (csrc/is_sinkhorn.hip) and Empirical.sinkhorn on the device against the float64 numpy route
(empirical_host._host_sinkhorn). The bound is the one derived at the head of csrc/is_sinkhorn.hip (u = 2^-24, K = J + 2 rounded up to even,
alpha^2 = log2(e) / eps, R_a, R_b the largest |z| of the sides, L_max the largest log2(e) |lw - max|, F_max = log2(e) / eps times the
largest |potential| any iteration of the problem saw), per half-step:
    e = expm1(ln 2 (2 K + 12) (alpha^2 (R_s^2 + R_q^2 + R_s R_q) + L_max + F_max) u) + 650 u + (n + 64) 2^-52 + n 2^-124,  d = -log1p(-e)
    after T iterations |f - exact| <= 2 T eps d, |g - exact| <= (2 T - 1) eps d, |p - exact| <= T eps d / 2
    |ot_ab - exact| <= err(f) + err(g) + c (max |f| + max |g|),  |ot_aa - exact| <= 2 err(p) + 2 c max |p|,  c = (n + 64) 2^-52
PP_SINKHORN_ERRORS=<file> appends every case's worst error / bound ratio (profiles/sinkhorn_errors.jsonl). All of it fails without the
feature: the parent has neither the symbol nor the method."""
import json
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

DEV = 'cuda:0'
U, LOG2E, ITERS = 2.0 ** -24, 1.4426950408889634, 8


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _op(lw_a, x_a, lw_b, x_b, center, scale, eps, tol=0.0, max_iter=ITERS, check_every=8):
    """One pp_is_sinkhorn_groups call on host arrays lw [M, n], x [M, n, J] (float32), center / scale [M, J], eps [M]: out, f, g, p_a, p_b."""
    from pyprob_amd import ops as P
    side = lambda lw, x: (_dev(lw.reshape(-1)), [_dev(x[:, :, j].reshape(-1)) for j in range(x.shape[2])], lw.shape[1], None)  # noqa: E731
    out = P.ops.is_sinkhorn_groups(*side(lw_a, x_a), *side(lw_b, x_b), _dev(center), _dev(1.0 / scale), _dev(eps), tol, max_iter, check_every)
    return [t.cpu().numpy() for t in out]


def _bounds(lw_a, x_a, lw_b, x_b, center, scale, eps, peak, iters):
    """(bounds on f, g, p_a, p_b, bounds on the three costs [3], the largest e) of one group after `iters` iterations."""
    from pyprob_amd.empirical_host import _kdej_counted
    K, n = (x_a.shape[1] + 3) & ~1, max(len(lw_a), len(lw_b))
    R, L = [], []
    for lw, x in ((lw_a, x_a), (lw_b, x_b)):
        z = _kdej_counted(lw, x, center, scale)[0]
        keep = np.isfinite(lw) & np.isfinite((x.astype(np.float64) - center) / scale).all(1)
        R.append(np.sqrt((z * z).sum(1)).max())
        L.append(LOG2E * np.abs(lw[keep].astype(np.float64) - lw[np.isfinite(lw)].max()).max())
    e = np.array([np.expm1(np.log(2.0) * (2 * K + 12) * (LOG2E / eps * (R[s] ** 2 + R[q] ** 2 + R[s] * R[q]) + L[s] + LOG2E / eps * pk) * U)
                  for s, q, pk in ((0, 1, peak[0]), (1, 0, peak[0]), (0, 0, peak[1]), (1, 1, peak[2]))])
    e = e + 650 * U + (n + 64) * 2.0 ** -52 + n * 2.0 ** -124
    d = -np.log1p(-e)
    d_ab, c = max(d[0], d[1]), (n + 64) * 2.0 ** -52
    pot = np.array([2 * iters * eps * d_ab, (2 * iters - 1) * eps * d_ab, iters * eps * d[2] / 2, iters * eps * d[3] / 2])
    cost = np.array([pot[0] + pot[1] + 2 * c * peak[0], 2 * pot[2] + 2 * c * peak[1], 2 * pot[3] + 2 * c * peak[2]])
    return pot, cost, e.max()


def _side(rng, n, J, center, scale, shift):
    """lw [n] within 20 of its maximum and x [n, J] with |z| <= 3.9, float32; from five particles on, two of them dropped: lw = -inf and
    a NaN coordinate under a finite weight."""
    z = rng.standard_normal((n, J)) + shift
    z *= np.minimum(1.0, 3.9 / np.sqrt((z * z).sum(1)))[:, None]
    x, lw = (center + scale * z).astype(np.float32), (-20.0 * rng.random(n)).astype(np.float32)
    if n >= 5:
        lw[1], x[n - 2, J - 1] = -np.inf, np.nan
    return lw, x


def _record(rec):
    print('sinkhorn', json.dumps(rec))
    if os.environ.get('PP_SINKHORN_ERRORS'):
        with open(os.environ['PP_SINKHORN_ERRORS'], 'a') as f:
            f.write(json.dumps(rec) + '\n')


def _worst(got, want, pot_bound, cost_bound):
    """The worst error / bound ratios of (out, f, g, p_a, p_b) against _host_sinkhorn's, NaN rows where the host's are."""
    assert all(np.array_equal(np.isnan(g[0]), np.isnan(w)) for g, w in zip(got[1:5], want[1:5]))
    pots = [np.nanmax(np.abs(g[0] - w)) / b for g, w, b in zip(got[1:5], want[1:5], pot_bound)]
    return dict(zip(('f', 'g', 'p_a', 'p_b'), pots)), (np.abs(got[0][0, :3] - want[0][:3]) / cost_bound).tolist()


def _cases():
    from pyprob_amd import lib as L
    block, tile, chunk = L.PP_IS_SINKHORN_PARTICLE_BLOCK, L.PP_IS_SINKHORN_QUERY_TILE, L.PP_IS_SINKHORN_CHUNK
    two = L.PP_IS_SINKHORN_MAX_STRIPS * chunk + 1      # (the first size at which a strip holds two chunks: few queries, or itself)
    sizes = [1, block - 1, block + 1, tile + 1, chunk - 1, chunk + 1, two]
    other = [block + 1, 1, tile + 1, block - 1, chunk + 1, chunk - 1, block + 1]
    cases = [(na, nb, (1, 3, 8)[i % 3], 'plain') for i, (na, nb) in enumerate(zip(sizes, other))]
    return cases + [(chunk + 1, tile + 1, 3, 'narrow')]


@pytest.mark.parametrize('na,nb,J,kind', _cases())
def test_potentials_and_costs_stay_within_the_derived_bound(na, nb, J, kind):
    from pyprob_amd import lib as L
    from pyprob_amd.empirical_host import _host_sinkhorn
    rng = np.random.default_rng(1000 * na + 10 * J + len(kind))
    center = np.full(J, 1000.0) if kind == 'narrow' else rng.uniform(-2.0, 2.0, J)
    scale = np.full(J, 1e-2) if kind == 'narrow' else rng.uniform(0.5, 2.0, J)
    (lw_a, x_a), (lw_b, x_b), eps = _side(rng, na, J, center, scale, 0.0), _side(rng, nb, J, center, scale, 0.5 / np.sqrt(J)), 0.05 * J
    args = (lw_a[None], x_a[None], lw_b[None], x_b[None], center[None], scale[None], np.array([eps]))
    got = _op(*args)
    want = _host_sinkhorn(lw_a, x_a, lw_b, x_b, center, scale, eps, 0.0, ITERS)
    pot_bound, cost_bound, e = _bounds(lw_a, x_a, lw_b, x_b, center, scale, eps, want[5], ITERS)
    pots, costs = _worst(got, want, pot_bound, cost_bound)
    _record(dict(case='%d x %d, J = %d, %s' % (na, nb, J, kind), worst_ratio=dict(pots, costs=costs), e=e,
                 strips=L.load().pp_is_sinkhorn_strips(na, nb)))
    assert e < 1e-2, e      # (a looser derivation is not a test)
    assert max(pots.values()) <= 1.0 and max(costs) <= 1.0, (pots, costs)
    assert np.array_equal(got[0][0, 3:6], want[0][3:6]) and got[0][0, 9:].tolist() == [na - 2 if na >= 5 else na, nb - 2 if nb >= 5 else nb, 7]
    again = _op(*args)
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(again, got))      # the same bits


def test_group_g_of_two_groups_carries_the_bits_of_its_own_call():
    from pyprob_amd import lib as L
    rng = np.random.default_rng(7)
    na, nb, J = 2 * L.PP_IS_SINKHORN_CHUNK + 5, L.PP_IS_SINKHORN_QUERY_TILE + 1, 3
    center, scale, eps = rng.uniform(-2.0, 2.0, (2, J)), rng.uniform(0.5, 2.0, (2, J)), np.array([0.15, 0.4])
    (lw_a, x_a), (lw_b, x_b) = ([np.stack(t) for t in zip(*[_side(rng, n, J, center[g], scale[g], s) for g in range(2)])]
                                for n, s in ((na, 0.0), (nb, 0.3)))
    both = _op(lw_a, x_a, lw_b, x_b, center, scale, eps)
    for g in range(2):
        s = slice(g, g + 1)
        one = _op(lw_a[s], x_a[s], lw_b[s], x_b[s], center[s], scale[s], eps[s])
        assert all(np.array_equal(b[g].view(np.int64), o[0].view(np.int64)) for b, o in zip(both, one))
    assert not np.array_equal(both[0][0], both[0][1])


def test_convergence_does_not_depend_on_check_every_and_the_plan_has_the_marginals():
    from pyprob_amd.empirical_host import _host_sinkhorn, _kdej_counted
    rng = np.random.default_rng(11)
    na, nb, J, tol = 300, 260, 3, 1e-3
    center, scale, eps = rng.uniform(-2.0, 2.0, J), rng.uniform(0.5, 2.0, J), 0.05 * J
    (lw_a, x_a), (lw_b, x_b) = _side(rng, na, J, center, scale, 0.0), _side(rng, nb, J, center, scale, 0.5 / np.sqrt(J))
    args = (lw_a[None], x_a[None], lw_b[None], x_b[None], center[None], scale[None], np.array([eps]))
    got, other = _op(*args, tol=tol, max_iter=1000, check_every=1), _op(*args, tol=tol, max_iter=1000, check_every=8)
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(got, other))
    out = got[0][0]
    assert out[11] == 0 and (out[6:9] < tol).all() and (out[3:6] >= 1).all() and (out[3:6] < 1000).all()
    # sum_i P_ij / b_j = exp((g_j - T(f)_j) / eps) with T in float64: T(f) is within tol eps of the g that f was computed from (the
    # residual, 1-Lipschitz) plus one half-step's eps d
    host = _host_sinkhorn(lw_a, x_a, lw_b, x_b, center, scale, eps, tol, 1000)
    _, _, e = _bounds(lw_a, x_a, lw_b, x_b, center, scale, eps, host[5], int(out[3]))
    (za, la), (zb, lb) = _kdej_counted(lw_a, x_a, center, scale), _kdej_counted(lw_b, x_b, center, scale)
    f, g = got[1][0][~np.isnan(got[1][0])], got[2][0][~np.isnan(got[2][0])]
    cost = ((za[:, None, :] - zb[None, :, :]) ** 2).sum(-1) / 2
    col = np.exp(la[:, None] + lb[None, :] + (f[:, None] + g[None, :] - cost) / eps).sum(0)
    _record(dict(case='marginals 300 x 260, J = 3', n_iter=out[3:6].tolist(), host_n_iter=host[0][3:6].tolist(),
                 worst=float(np.abs(col / np.exp(lb) - 1).max()), allowed=float(np.expm1(tol - np.log1p(-e)))))
    assert np.abs(col / np.exp(lb) - 1).max() <= np.expm1(tol - np.log1p(-e)) and e < 1e-2


def test_sinkhorn_on_lock_step_posteriors(monkeypatch):
    from pyprob_amd.distributions import TwoSampleTransport
    from pyprob_amd.empirical_host import _host_sinkhorn
    from test_gpu_density_joint import _two_statement_model
    model = _two_statement_model()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = model.posterior_results_batch(300, [{'obs0': 1.0, 'obs1': 0.5}], seed=13, offset=64)[0]
        b = model.posterior_results_batch(400, [{'obs0': 1.5, 'obs1': 0.0}], seed=14, offset=64)[0]
    with pytest.warns(UserWarning, match='max_iter=2'):
        assert not any(a.sinkhorn(b, max_iter=2).converged)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        r = a.sinkhorn(b, tol=0.0, max_iter=ITERS)
        monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
        host = a.sinkhorn(b, tol=0.0, max_iter=ITERS)
        monkeypatch.delenv('PP_EMPIRICAL_DEVICE')
    assert isinstance(r, TwoSampleTransport) and r.count == host.count == (300, 400) and r.n_iter == host.n_iter == (ITERS,) * 3
    assert np.allclose(host.center, r.center, rtol=1e-9) and np.allclose(host.scale, r.scale, rtol=1e-9) and r.epsilon == 0.1
    particles = lambda p: (p._pair_columns(None)[1].cpu().numpy(), np.stack([c.cpu().numpy() for c in p._pair_columns(None)[2]], 1))  # noqa: E731
    (lw_a, x_a), (lw_b, x_b) = particles(a), particles(b)
    peak = _host_sinkhorn(lw_a, x_a, lw_b, x_b, r.center, r.scale, r.epsilon, 0.0, ITERS)[5]
    pot_bound, cost_bound, e = _bounds(lw_a, x_a, lw_b, x_b, r.center, r.scale, r.epsilon, peak, ITERS)
    got, want = np.array([r.ot_ab, r.ot_aa, r.ot_bb]), np.array([host.ot_ab, host.ot_aa, host.ot_bb])
    _record(dict(case='public 300 x 400, J = 2', worst_ratio=dict(costs=(np.abs(got - want) / cost_bound).tolist(),
                                                                  f=float(np.abs(r.f.cpu().numpy() - host.f).max() / pot_bound[0])), e=e))
    assert (np.abs(got - want) <= cost_bound).all() and np.abs(r.f.cpu().numpy() - host.f).max() <= pot_bound[0] and e < 1e-2
    assert abs(r.divergence - host.divergence) <= cost_bound[0] + (cost_bound[1] + cost_bound[2]) / 2 and r.wasserstein2 > 0
    # a posterior against itself: f = g = p at the fixed point, where the divergence is 0; the last move of a potential is residual eps
    # (problem (a, b) of a self-pair may still be moving at max_iter under the default epsilon: plain iterations, no annealing)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        same = a.sinkhorn(a)
    assert abs(same.divergence) <= same.epsilon * (2 * same.residual[0] + same.residual[1] + same.residual[2]) + 2 * cost_bound[0]
    assert same.converged[1:] == (True, True) and same.ot_aa == same.ot_bb
    drawn = b.sinkhorn(a, num_samples=500, seed=3)
    assert drawn.count == (500, 500) and drawn.ess == pytest.approx((500.0, 500.0)) and drawn.divergence > 0
