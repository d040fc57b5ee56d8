"""The float64 numpy route of the joint Gaussian-mixture fit (empirical_host._host_gmm_joint: pp_is_gmm_joint_groups' definition,
include/pyprob_amd.h) against closed forms, and the operator's place in the library - no GPU."""
import numpy as np
import pytest

import gmm_ref as G
from pyprob_amd.empirical_host import _host_gmm_joint

REG = 1e-6


def _init(K, mu, cov):
    """weights 1 / K | means [K, J] | upper triangles of cov [K, J, J]."""
    iu = np.triu_indices(np.shape(mu)[1])
    return np.concatenate([np.full(K, 1.0 / K), np.ravel(mu), np.asarray(cov)[:, iu[0], iu[1]].ravel()])


def _unpack(row, J, K):
    iu = np.triu_indices(J)
    cov = np.zeros((K, J, J))
    cov[:, iu[0], iu[1]] = row[K + K * J:-7].reshape(K, -1)
    cov[:, iu[1], iu[0]] = cov[:, iu[0], iu[1]]
    return row[:K], row[K:K + K * J].reshape(K, J), cov, row[-7:]


def _planted(n, seed):
    """Two correlated 2-D components (correlation +0.8 and -0.8) whose marginals overlap: x [2, n], the planted means."""
    rng = np.random.default_rng(seed)
    means = np.array([[0.0, 0.0], [1.5, 0.5]])
    covs = np.array([[[1.0, 0.8], [0.8, 1.0]], [[1.0, -0.8], [-0.8, 1.0]]]) * 0.5
    comp = rng.random(n) < 0.4
    z = rng.standard_normal((n, 2))
    x = np.where(comp[:, None], means[1] + z @ np.linalg.cholesky(covs[1]).T, means[0] + z @ np.linalg.cholesky(covs[0]).T)
    return x.T.copy(), means


def test_one_component_one_iteration_is_the_weighted_mean_and_covariance():
    rng = np.random.default_rng(1)
    x = rng.normal(3.0, 2.0, (3, 500))
    lw = rng.normal(0.0, 1.0, 500)
    lw[::50] = -np.inf
    row = _host_gmm_joint(lw, x, _init(1, [[1.0, 2.0, 3.0]], [np.eye(3) * 4.0]), 1, 1, 0.0, REG)
    w = np.where(np.isfinite(lw), np.exp(lw - lw[np.isfinite(lw)].max()), 0.0)
    mean = (w * x).sum(1) / w.sum()
    cov = (w * (x - mean[:, None])) @ (x - mean[:, None]).T / w.sum() + REG * np.eye(3)
    pi, mu, got, tail = _unpack(row, 3, 1)
    np.testing.assert_allclose(mu[0], mean, rtol=1e-13)
    np.testing.assert_allclose(got[0], cov, rtol=1e-12, atol=1e-14)
    assert pi[0] == 1.0 and tail[1:4].tolist() == [1.0, 0.0, 0.0] and tail[5] == 490 and tail[4] == pytest.approx(w.sum(), rel=1e-14)


def test_integer_weights_equal_repeated_rows():
    x, _ = _planted(400, 2)
    reps = np.random.default_rng(3).integers(1, 5, 400)
    init = _init(2, [[-0.5, 0.0], [1.0, 1.0]], [np.eye(2)] * 2)
    a = _host_gmm_joint(np.log(reps.astype(np.float64)), x, init, 2, 6, 0.0, REG)
    b = _host_gmm_joint(np.zeros(reps.sum()), np.repeat(x, reps, axis=1), init, 2, 6, 0.0, REG)
    np.testing.assert_allclose(a[:-7], b[:-7], rtol=1e-10)                 # (the parameters; W is scaled by the largest weight)
    assert a[-7] == pytest.approx(b[-7], rel=1e-12) and a[-6] == b[-6] == 6


@pytest.mark.parametrize('K', [1, 3])
def test_one_dimension_reproduces_the_diagonal_fit(K):
    rng = np.random.default_rng(4)
    x = (3.0 + 2.5 * rng.integers(0, 3, 3000) + rng.normal(0.0, 0.5, 3000)).astype(np.float32)
    lw = rng.normal(0.0, 1.0, 3000).astype(np.float32)
    init = G.init_ref(lw, x, K, REG)
    want, _ = G.em_ref(lw, x, init, 30, 1e-3, REG)
    row = _host_gmm_joint(lw, x[None], init, K, 30, 1e-3, REG)
    got = np.concatenate([row[:3 * K + 3], row[3 * K + 4:]])             # (without the degenerate flag: the 1-D row)
    dev, same = G.deviation(got, want, K)
    assert same and dev <= 1e-9 and row[3 * K + 3] == 0.0


def test_a_planted_correlated_mixture_is_recovered():
    n = 20000
    x, means = _planted(n, 5)
    init = _init(2, [[-1.0, 0.0], [2.0, 0.0]], [np.cov(x) / 2.0] * 2)
    pi, mu, cov, tail = _unpack(_host_gmm_joint(np.zeros(n), x, init, 2, 200, 1e-6, REG), 2, 2)
    assert tail[2] == 1.0 and tail[3] == 0.0
    se = np.sqrt(cov[:, [0, 1], [0, 1]] / (pi[:, None] * n))
    assert (np.abs(mu - means) <= 3.0 * se).all(), (mu, se)
    assert cov[0, 0, 1] > 0.3 and cov[1, 0, 1] < -0.3                     # the two ridges, hidden in either marginal


def test_the_operator_is_exported_and_the_abi_version_stays():
    from pyprob_amd import build as B, lib as L
    lib = L.load()
    assert hasattr(lib, 'pp_is_gmm_joint_groups') and hasattr(lib, 'pp_is_gmm_joint_workspace_bytes')
    assert 'is_gmm_joint.hip' in B.SOURCES and lib.pp_abi_version() == 15 == L.PP_ABI_VERSION
    assert L.PP_IS_GMM_JOINT_WIDTH(8, 16) == 16 * 45 + 7 and lib.pp_is_gmm_joint_workspace_bytes(3, 2049, 8, 16) > 0
    assert lib.pp_is_gmm_joint_workspace_bytes(3, 2049, 9, 16) == 0 == lib.pp_is_gmm_joint_workspace_bytes(3, 2049, 8, 17)
