"""Float64 numpy restatement of pp_is_gmm_groups (include/pyprob_amd.h) and of Empirical.density_estimate's default start for the
tests: the weights and the skip rule, the deterministic initial parameters (1 / K, the exact weighted quantiles (k + 1/2) / K, the
weighted variance / K^2 + reg_covar), the EM itself - E-step, M-step from sums about the current mean, the stop rule - and the
output row; a CPU double of the operator with a call counter. scikit-learn's GaussianMixture(covariance_type='diag') on values
repeated by integer weights is what the definition restates: tests/golden/gmm_sklearn.npz pins this file against it."""
import numpy as np
import torch

EPS10 = 10.0 * np.finfo(np.float64).eps
calls = {'is_gmm_groups': 0}      # how often the CPU double ran


def width(K):
    return 3 * K + 6


def weights_ref(lw):
    """(w [n] float64 with 0 for the skipped particles, the largest finite log-weight or -inf)."""
    lw = np.asarray(lw, np.float64)
    fin = np.isfinite(lw)
    if not fin.any():
        return np.zeros(len(lw)), -np.inf
    top = lw[fin].max()
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(fin, np.exp(np.where(fin, lw, top) - top), 0.0), top


def quantiles_ref(lw, x, q):
    """The inverted-cdf quantiles Empirical.quantile defines: counted particles in stable value order, the first whose cumulative
    weight reaches q T."""
    w, _ = weights_ref(lw)
    x = np.asarray(x, np.float64)
    keep = np.nonzero(np.isfinite(np.asarray(lw, np.float64)) & ~np.isnan(x))[0]
    order = keep[np.argsort(x[keep], kind='stable')]
    cum = np.cumsum(w[order])
    t = np.asarray(q, np.float64) * cum[-1]
    k = np.where(t > 0, np.searchsorted(cum, t, side='left'), np.count_nonzero(cum <= 0))
    return x[order][np.minimum(k, len(order) - 1)]


def init_ref(lw, x, K, reg_covar=1e-6):
    """The default start [3 K] of one particle set: weights | means | variances."""
    w, _ = weights_ref(lw)
    x = np.asarray(x, np.float64)
    keep = w > 0
    mean = (w[keep] * x[keep]).sum() / w[keep].sum()
    var = (w[keep] * (x[keep] - mean) ** 2).sum() / w[keep].sum()
    return np.concatenate([np.full(K, 1.0 / K), quantiles_ref(lw, x, (np.arange(K) + 0.5) / K), np.full(K, var / K ** 2 + reg_covar)])


def em_ref(lw, x, init, max_iter=100, tol=1e-3, reg_covar=1e-6):
    """(row [3 K + 6], [lb_1, lb_2, ...]) of one particle set by the header's definition, component by component."""
    init = np.asarray(init, np.float64)
    K = len(init) // 3
    pi, mu, v = init[:K].copy(), init[K:2 * K].copy(), init[2 * K:].copy()
    w_all, top = weights_ref(lw)
    fin = np.isfinite(np.asarray(lw, np.float64))
    count = int(fin.sum())
    if count == 0:
        return np.concatenate([np.full(3 * K, np.nan), [np.nan, 0.0, 1.0, 0.0, 0.0, -np.inf]]), []
    w, xs = w_all[fin], np.asarray(x, np.float64)[fin]
    W = w.sum()
    before, n_iter, converged, bounds = -np.inf, 0, 0.0, []
    with np.errstate(all='ignore'):
        for t in range(1, int(max_iter) + 1):
            ell = np.stack([np.log(pi[k]) - 0.5 * np.log(2.0 * np.pi * v[k]) - (xs - mu[k]) ** 2 / (2.0 * v[k]) for k in range(K)])
            peak = ell.max(0)
            L = peak + np.log(np.exp(ell - peak).sum(0))
            lb = (w * L).sum() / W
            new = np.empty((3, K))
            N = np.empty(K)
            for k in range(K):
                r = w * np.exp(ell[k] - L)
                N[k] = r.sum() + EPS10
                d = (r * (xs - mu[k])).sum() / N[k]
                new[1, k] = mu[k] + d
                new[2, k] = np.maximum((r * (xs - mu[k]) ** 2).sum() / N[k] - d * d, 0.0) + reg_covar
            new[0] = N / N.sum()
            pi, mu, v = new
            bounds.append(float(lb))
            n_iter = t
            if abs(lb - before) < tol:
                converged = 1.0
                break
            before = lb
    return np.concatenate([pi, mu, v, [bounds[-1], float(n_iter), converged, W, float(count), top]]), bounds


def gmm_groups_ref(lw, x, init, max_iter=100, tol=1e-3, reg_covar=1e-6):
    """lw, x [M, N] float32, init [M, 3 K] -> rows [M, 3 K + 6]."""
    lw, x, init = np.asarray(lw, np.float32), np.asarray(x, np.float32), np.asarray(init, np.float64)
    return np.stack([em_ref(lw[g], x[g], init[g], max_iter, tol, reg_covar)[0] for g in range(lw.shape[0])])


def mixture_logpdf(x, pi, mu, sd):
    """log sum_k pi_k Normal(x; mu_k, sd_k) in float64."""
    x = np.asarray(x, np.float64)[:, None]
    ell = np.log(pi) - 0.5 * np.log(2.0 * np.pi * sd * sd) - (x - mu) ** 2 / (2.0 * sd * sd)
    peak = ell.max(1)
    return peak + np.log(np.exp(ell - peak[:, None]).sum(1))


def deviation(got, want, K):
    """The largest relative deviation of weights, means, variances and the lower bound of rows [.., 3 K + 6] (NaN where both are
    NaN counts as equal), and whether the integer slots (n_iter, converged, count) are equal."""
    got, want = np.asarray(got, np.float64).reshape(-1, width(K)), np.asarray(want, np.float64).reshape(-1, width(K))
    a, b = got[:, :3 * K + 1], want[:, :3 * K + 1]
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(both_nan, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    rel = np.where(np.isnan(rel), np.inf, rel)
    same = np.array_equal(got[:, [3 * K + 1, 3 * K + 2, 3 * K + 4]], want[:, [3 * K + 1, 3 * K + 2, 3 * K + 4]])
    return float(rel.max()) if rel.size else 0.0, bool(same)


def is_gmm_groups_cpu(lw, x, n_components, n_per, stats, params_init, max_iter, tol, reg_covar):
    calls['is_gmm_groups'] += 1
    n, K = int(n_per), int(n_components)
    return torch.from_numpy(gmm_groups_ref(lw.numpy().reshape(-1, n), x.numpy().reshape(-1, n), params_init.numpy().reshape(-1, 3 * K),
                                           int(max_iter), float(tol), float(reg_covar)))


_registered = False


def register_cpu_doubles():
    """The product has no CPU implementation of the operator: the tests register the numpy restatement as its CPU kernel."""
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_gmm_groups', is_gmm_groups_cpu, 'CPU')
        _registered = True
