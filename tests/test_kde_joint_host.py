"""The float64 numpy route of Empirical.kde_joint and Empirical.modes (empirical_host._host_kde_joint, _host_meanshift) - the comparator of
tests/test_gpu_kde_joint.py - against a direct double loop, and the argument errors of the two methods. No GPU. All of it fails without the
feature: the parent has neither the functions nor the methods."""
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')


def _vector_posterior(x, lw):
    from pyprob_amd.distributions import Empirical
    return Empirical(values=[torch.tensor(v) for v in x], log_weights=[float(a) for a in lw])


@pytest.mark.parametrize('J', [1, 3, 8])
def test_host_kde_joint_is_the_double_loop(J):
    from pyprob_amd.empirical_host import _host_kde_joint
    rng = np.random.default_rng(J)
    n, center, scale, h = 23, rng.uniform(-1, 1, J), rng.uniform(0.5, 2.0, J), 0.4
    x, lw = center + scale * rng.standard_normal((n, J)), -3.0 * rng.random(n)
    lw[2], x[5, J - 1] = -np.inf, np.nan
    points = center + scale * rng.standard_normal((4, J))
    points[3] = center + scale * 60.0 * h        # exp of its exponents underflows float64's neighbour float32, not the maximum route
    logd, mean, count = _host_kde_joint(lw, x, center, scale, h, points, want_mean=True)
    keep = [i for i in range(n) if i not in (2, 5)]
    W = sum(math.exp(lw[i]) for i in keep)
    for q in range(4):
        zq = (points[q] - center) / scale
        e = [lw[i] - sum((zq[j] - (x[i, j] - center[j]) / scale[j]) ** 2 for j in range(J)) / (2 * h * h) for i in keep]
        top = max(e)
        k = [math.exp(v - top) for v in e]
        assert logd[q] == pytest.approx(top + math.log(sum(k)) - math.log(W) - J * math.log(h * math.sqrt(2 * math.pi)), rel=1e-12)
        for j in range(J):
            assert mean[q, j] == pytest.approx(sum(k[a] * (x[i, j] - center[j]) / scale[j] for a, i in enumerate(keep)) / sum(k), rel=1e-9)
    assert count == n - 2 and np.isfinite(logd).all()


def test_host_meanshift_stops_at_a_fixed_point():
    from pyprob_amd.empirical_host import _host_kde_joint, _host_meanshift, _merge_modes
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal((200, 2)) * 0.2 + 3.0, rng.standard_normal((100, 2)) * 0.2 - 3.0])
    lw, center, scale, h = np.zeros(300), np.zeros(2), np.ones(2), 0.5
    pts, logd, n_iter, conv, count = _host_meanshift(lw, x, center, scale, h, x[::30], 1e-6, 500)
    assert conv.all() and count == 300 and (n_iter >= 1).all()
    moved = _host_kde_joint(lw, x, center, scale, h, pts, want_mean=True)[1]
    assert np.sqrt(((moved - pts) ** 2).sum(1)).max() < 1e-6 * h          # x = mean(x) at the end points
    reps, label = _merge_modes(pts, logd, h)
    assert len(reps) == 2 and np.abs(pts[reps[0]] - 3.0).max() < 0.1 and np.abs(pts[reps[1]] + 3.0).max() < 0.1
    assert np.bincount(label).tolist() == [7, 3]


def test_kde_joint_and_modes_take_the_host_route_and_check_their_arguments(monkeypatch):
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import JointModes, KernelDensityJoint
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    monkeypatch.setattr(P, 'ops', None)          # (the host route must not reach for an operator)
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal((150, 2)) + 4.0, rng.standard_normal((150, 2)) - 4.0])
    post = _vector_posterior(x, np.zeros(300))
    dens = post.kde_joint(x[:5])
    assert isinstance(dens, KernelDensityJoint) and dens.x.shape == (5, 2) and dens.count == 300 and dens.ess == pytest.approx(300.0)
    assert dens.bandwidth == pytest.approx(300.0 ** (-1.0 / 6.0)) and np.allclose(dens.density, np.exp(dens.log_density))
    found = post.modes(num_seeds=32, seed=0)
    assert isinstance(found, JointModes) and found.metadata['op'] == 'modes' and len(found.modes) == 2
    assert found.share.tolist() == [0.5, 0.5] and np.abs(np.abs(found.modes) - 4.0).max() < 0.5 and found.converged.all()
    with pytest.raises(ValueError, match='num_seeds'):
        post.modes(num_seeds=4097)
    with pytest.raises(ValueError, match='scale='):
        _vector_posterior(np.stack([x[:, 0], np.ones(300)], 1), np.zeros(300)).kde_joint(x[:2])
    with pytest.raises(ValueError, match='1 .. 8 addresses'):
        _vector_posterior(rng.standard_normal((20, 9)), np.zeros(20)).kde_joint(np.zeros((1, 9)))


def test_an_address_of_a_branch_raises_as_joint_does():
    from pyprob_amd.empirical import Empirical
    calls = []

    class Branching(Empirical):
        def _joint_columns(self, addresses, host_ok=False):
            calls.append(addresses)
            raise ValueError('address executed by some of the particles only (a branch)')
    post = Branching(values=[torch.tensor(0.0)], log_weights=[0.0])
    post.__dict__['statement_log'] = object()
    for call in (lambda: post.kde_joint(np.zeros((1, 1)), ['a']), lambda: post.modes(['a'])):
        with pytest.raises(ValueError, match='branch'):
            call()
    assert calls == [['a'], ['a']]
