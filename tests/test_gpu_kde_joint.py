"""pp_is_kde_joint_groups and pp_is_meanshift_groups (csrc/is_kde_joint.hip), Empirical.kde_joint and Empirical.modes on the device against
the float64 numpy route (empirical_host). The bound is the one derived at the head of csrc/is_kde_joint.hip (u = 2^-24, K = J + 2 rounded
up to even, alpha^2 = log2(e) / h^2, R the largest |z_i|, L_max the largest log2(e) |lw_i - max|), per query:
    eps = expm1(ln 2 (2 K + 12) (alpha^2 (R^2 + |z_q|^2 + R |z_q|) + L_max) u) + 650 u + (n + 64) 2^-52 + n 2^-124
    |log_density - exact| <= -log1p(-eps),   |mean_j - exact| <= 2 eps R / (1 - eps)
PP_KDE_JOINT_ERRORS=<file> appends every case's worst error / bound ratio (profiles/kde_joint_errors.jsonl). All of it fails without the
feature: the parent has neither the symbols nor the methods."""
import json
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

DEV = 'cuda:0'
U, LOG2E = 2.0 ** -24, 1.4426950408889634


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _cols(lw, x):
    return _dev(lw.reshape(-1)), [_dev(x[:, :, j].reshape(-1)) for j in range(x.shape[2])], lw.shape[1], None


def _op(lw, x, center, scale, h, points, want_mean=True):
    """One pp_is_kde_joint_groups call on host arrays lw [M, n], x [M, n, J] (float32), center / scale [M, J], h [M], points [M, Q, J]."""
    from pyprob_amd import ops as P
    out = P.ops.is_kde_joint_groups(*_cols(lw, x), _dev(center), _dev(1.0 / scale), _dev(h), _dev(points), want_mean)
    return [t.cpu().numpy() for t in out]


def _bounds(lw, x, center, scale, h, points):
    """(bound on log_density [Q], bound on a mean coordinate [Q], eps [Q]) of one group."""
    from pyprob_amd.empirical_host import _kdej_counted
    J = x.shape[1]
    K = (J + 3) & ~1
    z, logw = _kdej_counted(lw, x, center, scale)
    top = lw[np.isfinite(lw)].max()
    keep = np.isfinite(lw) & np.isfinite((x.astype(np.float64) - center) / scale).all(1)
    R, L = np.sqrt((z * z).sum(1)).max(), LOG2E * np.abs(lw[keep].astype(np.float64) - top).max()
    rq = np.sqrt((((points - center) / scale) ** 2).sum(1))
    S = LOG2E / (h * h) * (R * R + rq * rq + R * rq) + L
    eps = np.expm1(np.log(2.0) * (2 * K + 12) * S * U) + 650 * U + (len(lw) + 64) * 2.0 ** -52 + len(lw) * 2.0 ** -124
    return -np.log1p(-eps), 2 * eps * R / (1 - eps), eps


def _particles(rng, n, J, center, scale):
    """lw [n] within 20 of its maximum and x [n, J] with |z_j| <= 3.9, float32; from five particles on, two of them dropped: lw = -inf
    and a NaN coordinate under a finite weight."""
    x = (center + scale * np.clip(rng.standard_normal((n, J)), -3.9, 3.9)).astype(np.float32)
    lw = (-20.0 * rng.random(n)).astype(np.float32)
    if n >= 5:
        lw[1], x[n - 2, J - 1] = -np.inf, np.nan
    return lw, x


def _scott(lw, J):
    w = np.exp(lw[np.isfinite(lw)].astype(np.float64))
    return float((w.sum() ** 2 / (w * w).sum()) ** (-1.0 / (J + 4)))


def _record(rec):
    print('kde_joint', json.dumps(rec))
    if os.environ.get('PP_KDE_JOINT_ERRORS'):
        with open(os.environ['PP_KDE_JOINT_ERRORS'], 'a') as f:
            f.write(json.dumps(rec) + '\n')


def _cases():
    from pyprob_amd import lib as L
    block, chunk, strip = L.PP_IS_KDEJ_PARTICLE_BLOCK, L.PP_IS_KDEJ_CHUNK, L.PP_IS_KDEJ_MAX_STRIPS * L.PP_IS_KDEJ_CHUNK
    queries = (1, L.PP_IS_KDEJ_QUERY_BLOCK + 1, L.PP_IS_KDEJ_QUERY_TILE + 1)
    sizes = [1] + [b + d for b in (block, chunk, strip) for d in (-1, 0, 1)]      # (above `strip` a strip holds two chunks)
    cases = [(n, queries[(i + k) % 3], J, 'plain') for i, n in enumerate(sizes) for k, J in enumerate((1, 3, 8))]
    return cases + [(chunk + 1, queries[1], J, kind) for J in (3, 8) for kind in ('narrow', 'fifth')]


@pytest.mark.parametrize('n,Q,J,kind', _cases())
def test_density_and_mean_stay_within_the_derived_bound(n, Q, J, kind):
    from pyprob_amd.empirical_host import _host_kde_joint
    rng = np.random.default_rng(1000 * n + 10 * J + len(kind))
    center = np.full(J, 1000.0) if kind == 'narrow' else rng.uniform(-2.0, 2.0, J)
    scale = np.full(J, 1e-2) if kind == 'narrow' else rng.uniform(0.5, 2.0, J)
    lw, x = _particles(rng, n, J, center, scale)
    h = _scott(lw, J) * (0.2 if kind == 'fifth' else 1.0)
    points = center + scale * rng.standard_normal((Q, J))
    if Q > 1:       # the last query: 40 h beyond the farthest particle; exp of its exponents underflows fp32 without the running maximum
        points[-1] = center + scale * (3.9 * np.sqrt(J) + 40.0 * h) * np.eye(J)[0]
    args = (lw[None], x[None], center[None], scale[None], np.array([h]), points[None])
    logd, mean, count = _op(*args)
    want_d, want_m, want_c = _host_kde_joint(lw, x, center, scale, h, points, want_mean=True)
    bound_d, bound_m, eps = _bounds(lw, x, center, scale, h, points)
    ratio_d, ratio_m = np.abs(logd[0] - want_d) / bound_d, np.abs(mean[0] - want_m).max(1) / bound_m
    _record(dict(case='%d x %d, J = %d, %s' % (n, Q, J, kind), worst_ratio=dict(log_density=ratio_d.max(), mean=ratio_m.max()),
                 eps=dict(near=eps[:max(Q - 1, 1)].max(), far=eps[-1])))
    assert eps[:max(Q - 1, 1)].max() < (0.1 if kind == 'fifth' else 5e-3), eps      # (a looser derivation is not a test)
    assert np.isfinite(logd).all() and np.isfinite(mean).all()
    assert (ratio_d <= 1.0).all() and (ratio_m <= 1.0).all(), (ratio_d.max(), ratio_m.max())
    assert count[0] == want_c == (n - 2 if n >= 5 else n)
    again = _op(*args)
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(again, (logd, mean, count)))      # the same bits
    only = _op(*args, want_mean=False)
    assert np.array_equal(only[0].view(np.int64), logd.view(np.int64)) and only[1].size == 0
    if (n, J) == (31, 3):       # no counted particle: NaN rows, count 0
        dead = _op(np.full_like(args[0], -np.inf), *args[1:])
        assert np.isnan(dead[0]).all() and np.isnan(dead[1]).all() and dead[2][0] == 0


def test_group_g_of_two_groups_carries_the_bits_of_its_own_call():
    from pyprob_amd import lib as L
    rng = np.random.default_rng(7)
    n, Q, J = 2 * L.PP_IS_KDEJ_CHUNK + 5, L.PP_IS_KDEJ_QUERY_TILE + 1, 3
    center, scale = rng.uniform(-2.0, 2.0, (2, J)), rng.uniform(0.5, 2.0, (2, J))
    lw, x = (np.stack(t) for t in zip(*[_particles(rng, n, J, center[g], scale[g]) for g in range(2)]))
    h = np.array([0.3, 0.7])
    points = center[:, None, :] + scale[:, None, :] * rng.standard_normal((2, Q, J))
    both = _op(lw, x, center, scale, h, points)
    for g in range(2):
        one = _op(lw[g:g + 1], x[g:g + 1], center[g:g + 1], scale[g:g + 1], h[g:g + 1], points[g:g + 1])
        assert all(np.array_equal(b[g].view(np.int64), o[0].view(np.int64)) for b, o in zip(both, one))
    assert not np.array_equal(both[0][0], both[0][1])


def mixture_particles(components, J, n=3000, seed=0):
    """Weighted samples of a mixture of `components` unit Gaussians whose means differ by 10 in at least half of the J coordinates, drawn
    component by component in equal numbers and re-weighted to the masses 0.5, 0.3(, 0.2): (lw [n], x [n, J] float32, the means)."""
    rng = np.random.default_rng(seed + 10 * J + components)
    signs = np.array([[1.0] * J, [-1.0] * J, [(-1.0) ** j for j in range(J)] if J > 1 else [0.0]])[:components]
    means, mass = 5.0 * signs, np.array([0.5, 0.3, 0.2])[:components] if components == 3 else np.array([0.6, 0.4])
    k = np.arange(n) % components
    x = (means[k] + rng.standard_normal((n, J))).astype(np.float32)
    lw = (np.log(mass[k]) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return lw, x, means


@pytest.mark.parametrize('components,J', [(2, 2), (3, 2), (2, 8), (3, 8)])
def test_mean_shift_finds_the_modes_the_float64_route_finds(components, J):
    from pyprob_amd import ops as P
    from pyprob_amd.empirical_host import _host_joint_moments, _host_kde_joint, _host_meanshift, _merge_modes
    lw, x, means = mixture_particles(components, J)
    center, scale, ess, _ = _host_joint_moments(lw, x)
    h, tol, S = ess ** (-1.0 / (J + 4)), 1e-3, 96
    seeds = ((x[np.arange(S) * (len(lw) // S)].astype(np.float64) - center) / scale)
    want = _host_meanshift(lw, x, center, scale, h, seeds, tol, 200)
    reps, label = _merge_modes(want[0], want[1], h)
    # the inputs are such that the float64 route alone is unambiguous: every seed converges to within h / 8 of its mode, and the modes
    # lie more than h apart - no perturbation of the size of the bound moves a seed from one basin's end point to another's
    assert want[3].all() and (label >= 0).all() and len(reps) == components
    assert (np.sqrt(((want[0] - want[0][reps][label]) ** 2).sum(1)) < h / 8).all()
    assert all(np.sqrt(((want[0][a] - want[0][b]) ** 2).sum()) > h for a in reps for b in reps if a != b)
    got = [t.cpu().numpy()[0] for t in P.ops.is_meanshift_groups(*_cols(lw[None], x[None]), _dev(center[None]), _dev(1.0 / scale[None]),
                                                               _dev(np.array([h])), _dev(seeds[None]), tol, 200, 8)]
    other = [t.cpu().numpy()[0] for t in P.ops.is_meanshift_groups(*_cols(lw[None], x[None]), _dev(center[None]), _dev(1.0 / scale[None]),
                                                                 _dev(np.array([h])), _dev(seeds[None]), tol, 200, 3)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, other))      # (the check interval changes nothing)
    assert got[3].all() and got[4] == len(lw)
    got_reps, got_label = _merge_modes(got[0], got[1], h)
    assert len(got_reps) == components
    share = lambda lab, k: np.bincount(lab, minlength=k) / float(S)      # noqa: E731
    assert np.array_equal(share(got_label, components), share(label, components))
    # the float64 mean-shift map moves a returned mode by less than (tol + the derived bound on the mean) h
    modes = center + got[0][got_reps] * scale
    bound_d, bound_m, _ = _bounds(lw, x, center, scale, h, modes)
    logd, moved, _ = _host_kde_joint(lw, x, center, scale, h, modes, want_mean=True)
    step = np.sqrt(((moved - got[0][got_reps]) ** 2).sum(1))
    _record(dict(case='modes %d components, J = %d' % (components, J), step_over_h=(step / h).tolist(),
                 allowed=(tol + np.sqrt(J) * bound_m / h).tolist(), n_iter=int(got[2].max())))
    assert (step < (tol + np.sqrt(J) * bound_m / h) * h).all()
    assert (np.abs(got[1][got_reps] - logd) <= bound_d).all()
    assert np.sqrt((((means[0] - center) / scale - got[0][got_reps[0]]) ** 2).sum()) < h      # the heaviest component's mean


def test_kde_joint_and_modes_on_a_lock_step_posterior(monkeypatch):
    from pyprob_amd.distributions import JointModes, KernelDensityJoint
    from test_gpu_density_joint import _two_statement_model
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = _two_statement_model().posterior_results_batch(2300, [{'obs0': 1.0, 'obs1': 0.5}], seed=13, offset=64)[0]
    j = post.joint()
    pts = j.mean + j.stddev * np.random.default_rng(3).standard_normal((40, len(j.mean)))
    dens, found = post.kde_joint(pts), post.modes(num_seeds=64, seed=5)
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    host, host_found = post.kde_joint(pts), post.modes(num_seeds=64, seed=5)
    assert isinstance(dens, KernelDensityJoint) and isinstance(found, JointModes) and found.metadata['op'] == 'modes'
    assert dens.count == host.count == j.count and dens.bandwidth == pytest.approx(j.ess ** (-1.0 / (len(j.mean) + 4)))
    assert np.allclose(dens.log_density, host.log_density, rtol=0, atol=1e-3) and np.allclose(dens.density, np.exp(dens.log_density))
    assert len(found.modes) >= 1 and found.share.sum() == pytest.approx(1.0) and (np.diff(found.log_density) <= 0).all()
    assert np.sqrt((((found.modes[0] - host_found.modes[0]) / found.scale) ** 2).sum()) < found.bandwidth
