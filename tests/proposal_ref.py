"""Plain numpy restatement of pp_is_proposal_groups' density (include/pyprob_amd.h) in any float type - float64, and numpy.longdouble
for the error bounds -, the packed rows the operator reads, and the analytic moments of a Gaussian mixture."""
import numpy as np


def cholesky(a, dtype):
    J = a.shape[0]
    L = np.zeros((J, J), dtype)
    for j in range(J):
        for m in range(j + 1):
            s = a[j, m] - (L[j, :m] * L[m, :m]).sum()
            L[j, m] = np.sqrt(s) if m == j else s / L[m, m]
    return L


def neg_log_q(x, weights, means, covs, dtype=np.float64):
    """-log sum_k pi_k N(x; mu_k, Sigma_k) of x [n, J] by forward substitution with the Cholesky factor, all in `dtype`."""
    x, w, means, covs = (np.asarray(t, dtype) for t in (x, weights, means, covs))
    w = w / w.sum()
    n, J = x.shape
    log_2pi = np.log(dtype(8) * np.arctan(dtype(1)))
    ell = np.empty((n, len(w)), dtype)
    for k in range(len(w)):
        L = cholesky(covs[k], dtype)
        d = x - means[k]
        y = np.empty_like(d)
        for j in range(J):
            y[:, j] = (d[:, j] - (y[:, :j] * L[j, :j]).sum(1)) / L[j, j]
        ell[:, k] = np.log(w[k]) - dtype(J) / 2 * log_2pi - np.log(np.diag(L)).sum() - (y * y).sum(1) / 2
    top = ell.max(1)
    return -(top + np.log(np.exp(ell - top[:, None]).sum(1)))


def normal_lp(x, loc, scale):
    return -0.5 * ((x - loc) / scale) ** 2 - np.log(scale) - 0.5 * np.log(2 * np.pi)


def fit_row(weights, means, covs):
    """weights [K] | means [K, J] | upper triangles row by row, float64: the leading part of a pp_is_gmm_joint_groups row."""
    iu, ku = np.triu_indices(np.shape(means)[1])
    return np.concatenate([np.ravel(weights), np.ravel(means), np.ravel(np.asarray(covs)[:, iu, ku])]).astype(np.float64)


def random_fit(rng, J, K, center=0.0, width=1.0):
    """A well-conditioned mixture: weights that do not sum to 1, means around `center`, covariances width^2 (A A^T / J + I / 2)."""
    a = rng.normal(size=(K, J, J))
    covs = width ** 2 * (a @ a.transpose(0, 2, 1) / J + 0.5 * np.eye(J))
    return rng.uniform(0.5, 2.0, K), center + 3.0 * width * rng.normal(size=(K, J)), covs


def moments(weights, means, covs):
    """(E x [J], E x x^T [J, J], Var x [J], Var(x_j x_m) [J, J]) of the mixture; the fourth moments by Isserlis' theorem."""
    w = np.asarray(weights, np.float64) / np.sum(weights)
    m1 = np.einsum('k,kj->j', w, means)
    second = covs + np.einsum('kj,km->kjm', means, means)
    m2 = np.einsum('k,kjm->jm', w, second)
    d = np.einsum('kjj->kj', covs) + means ** 2
    fourth = np.einsum('kj,km->kjm', d, d) + 2 * covs ** 2 + 4 * np.einsum('kj,km->kjm', means, means) * covs
    return m1, m2, np.diag(m2) - m1 ** 2, np.einsum('k,kjm->jm', w, fourth) - m2 ** 2
