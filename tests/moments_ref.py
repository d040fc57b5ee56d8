"""Float64 restatement of pp_is_moments_groups (include/pyprob_amd.h) for the tests: the weights about the maximum of the finite
log-weights, the pivot rule, the skipped particles - and the scales |got - ref| is measured against; a two-pass weighted mean and
covariance; a CPU double of the operator."""
import numpy as np
import torch


def width(J):
    return 4 + 2 * J + J * (J + 1) // 2


def moments_ref(lw, cols):
    """lw [M, N], cols [J, M, N] -> (rows [M, width(J)], scale [M, width(J)]): the output rows and, per entry, the sum of the
    absolute values of its terms (0 for the entries that are not sums). A particle whose lw is not finite is left out BEFORE any
    arithmetic touches its column values."""
    lw = np.asarray(lw, np.float32)
    cols = np.asarray(cols, np.float32)
    J, M, N = cols.shape
    rows, scale = np.zeros((M, width(J))), np.zeros((M, width(J)))
    fin = np.isfinite(lw)                                                     # [M, N]
    m = np.where(fin, lw, -np.inf).astype(np.float64).max(axis=1)             # (-inf: no finite log-weight in the group)
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.where(fin, np.exp(np.where(fin, lw, 0.0).astype(np.float64) - np.where(np.isfinite(m), m, 0.0)[:, None]), 0.0)
    first = cols[:, :, 0].astype(np.float64)                                  # [J, M]
    c = np.where(np.isfinite(first), first, 0.0)
    d = np.where(fin, cols, 0.0).astype(np.float64) - c[:, :, None]           # (a skipped particle's values are replaced, not used:
    d = np.where(fin, d, 0.0)                                                 # every term of it is an exact zero)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = m, w.sum(1), (w * w).sum(1), fin.sum(1)
    rows[:, 4:4 + J] = c.T
    rows[:, 4 + J:4 + 2 * J] = (w * d).sum(2).T
    scale[:, 4 + J:4 + 2 * J] = (w * np.abs(d)).sum(2).T
    e = 4 + 2 * J
    for j in range(J):
        for k in range(j, J):
            rows[:, e] = (w * d[j] * d[k]).sum(1)
            scale[:, e] = (w * np.abs(d[j]) * np.abs(d[k])).sum(1)
            e += 1
    return rows, scale


def mean_cov_ref(lw, cols):
    """Two passes in float64 over lw [N], cols [J, N]: the normalised weights, the means, the covariance about the means."""
    lw = np.asarray(lw, np.float64)
    x = np.asarray(cols, np.float64)
    fin = np.isfinite(lw)
    w = np.exp(lw[fin] - lw[fin].max())
    w = w / w.sum()
    x = x[:, fin]
    mean = (w * x).sum(1)
    d = x - mean[:, None]
    return mean, (w * d) @ d.T


calls = {'is_moments_groups': 0}      # how often the CPU double ran


def is_moments_groups_cpu(lw, cols, n_per, stats):
    calls['is_moments_groups'] += 1
    n_per = int(n_per)
    rows, _ = moments_ref(lw.numpy().reshape(-1, n_per), np.stack([c.numpy().reshape(-1, n_per) for c in cols]))
    return torch.from_numpy(rows)
