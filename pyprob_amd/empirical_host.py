"""The float64 numpy routes of Empirical's statistics (pyprob_amd/empirical.py): what a host-backed Empirical, and every
Empirical under PP_EMPIRICAL_DEVICE=0, computes by the definitions of the device kernels. numpy only: nothing here imports torch."""
import math

import numpy as np


def _host_order(lw, x):
    """The indices of the particles with a finite log-weight and a value that is not NaN, in stable ascending order of value
    (numpy compares -0.0 == +0.0: ties keep particle order) - pp_is_sort_groups' order in float64."""
    keep = np.nonzero(np.isfinite(lw) & ~np.isnan(x))[0]
    return keep[np.argsort(x[keep], kind='stable')].astype(np.int64)


def _host_sorted_cdf(lw, x):
    """(values in sorted order, their cumulative weights) of the counted particles in float64 numpy; (None, None) where nothing
    is counted or the total is not positive and finite."""
    order = _host_order(lw, x)
    if len(order) == 0:
        return None, None
    cdf = np.cumsum(np.exp(lw[order] - np.max(lw[np.isfinite(lw)])))
    if not (cdf[-1] > 0 and np.isfinite(cdf[-1])):
        return None, None
    return x[order].astype(np.float64), cdf


def _host_quantiles(lw, x, qs):
    """pp_is_quantile_groups' definition in float64 numpy for one particle set."""
    v, cdf = _host_sorted_cdf(lw, x)
    if v is None:
        return np.full(len(qs), np.nan)
    t = qs * cdf[-1]
    k = np.where(t > 0, np.searchsorted(cdf, t, side='left'), np.count_nonzero(cdf <= 0))
    return v[np.minimum(k, len(v) - 1)]


def _hpd_search(v, cdf, levels):
    """pp_is_hpd_groups' definition on sorted values v and their cumulative weights cdf (float64 [c]): ([L, 2] values, [L, 2]
    positions)."""
    out, pos = np.full((len(levels), 2), np.nan), np.full((len(levels), 2), -1, np.int64)
    c = len(cdf)
    if c == 0 or not (cdf[-1] > 0 and np.isfinite(cdf[-1])):
        return out, pos
    T = cdf[-1]
    prev = np.concatenate([[0.0], cdf[:-1]])
    for l, L in enumerate(levels):
        if not (L > 0 and L <= 1):
            continue
        t = prev + L * T
        starts = np.nonzero((cdf > prev) & (t <= T))[0]
        ends = np.maximum(starts, np.searchsorted(cdf, t[starts], side='left'))
        with np.errstate(invalid='ignore'):
            width = v[ends].astype(np.float64) - v[starts].astype(np.float64)
        width = np.where(np.isnan(width), np.inf, width)
        k = int(np.argmin(width))                 # (the first minimum: ties go to the smallest start)
        pos[l] = starts[k], ends[k]
        out[l] = v[starts[k]], v[ends[k]]
    return out, pos


def _host_hpd(lw, x, levels):
    """pp_is_hpd_groups' definition in float64 numpy for one particle set: [L, 2]."""
    v, cdf = _host_sorted_cdf(lw, x)
    if v is None:
        return np.full((len(levels), 2), np.nan)
    return _hpd_search(v, cdf, levels)[0]


def _host_ecdf(lw, x, xs, strict):
    """pp_is_ecdf_groups' definition in float64 numpy for one particle set."""
    v, cdf = _host_sorted_cdf(lw, x)
    if v is None:
        return np.full(len(xs), np.nan)
    k = np.searchsorted(v, np.where(np.isnan(xs), 0.0, xs), side='left' if strict else 'right')
    out = np.where(k == 0, 0.0, cdf[np.maximum(k, 1) - 1] / cdf[-1])
    return np.where(np.isnan(xs), np.nan, out)


def _host_extent(lw, x):
    """pp_is_extent_groups' row in numpy: min, max over the values with a finite log-weight that are not NaN, the two counts."""
    fin = np.isfinite(lw)
    nan = np.isnan(x)
    v = x[fin & ~nan]
    return np.array([v.min() if v.size else np.inf, v.max() if v.size else -np.inf, v.size, int((fin & nan).sum())])


def _host_hist_row(lw, x, e):
    """The row [2, bins + 3] of the host route: float64 weight sums and counts per slot by pp_is_hist_groups' bin rule."""
    bins = len(e) - 1
    fin = np.isfinite(lw)
    l, v = lw[fin], x[fin]
    w = np.exp(l - l.max()) if l.size else np.zeros(0)
    with np.errstate(invalid='ignore'):
        b = np.searchsorted(e, v, side='right') - 1
        slot = np.where(np.isnan(v), bins + 2, np.where(v < e[0], bins, np.where(v > e[-1], bins + 1, np.minimum(b, bins - 1))))
    return np.stack([np.bincount(slot, weights=w, minlength=bins + 3), np.bincount(slot, minlength=bins + 3).astype(np.float64)])


def _host_psis(lw, tail, want_weights=True):
    """pp_is_psis_groups' definition in float64 numpy for one particle set: (smoothed log-weights float64 [n] or None, the row of
    PP_IS_PSIS_WIDTH doubles). The smoothed tail log-weights are rounded to float32 as the device stores them."""
    lw = np.asarray(lw, np.float64)
    fin = np.nonzero(np.isfinite(lw))[0]
    order = fin[np.argsort(lw[fin], kind='stable')]
    s = lw[order]
    c = len(s)
    row = np.array([np.inf, np.nan, 0.0, 0.0, 0.0, np.nan, float(c), np.nan])
    new = lw.copy() if want_weights else None
    if c == 0:
        return new, row
    Mg = row[7] = s[c - 1]
    b = c - (tail if tail > 0 else int(math.ceil(min(c / 5.0, 3.0 * math.sqrt(float(c)))))) - 1
    if b < 0:
        return new, row
    f = int(np.count_nonzero(s <= s[b]))
    n = c - f
    u = np.exp(s[b] - Mg)
    row[2], row[4], row[5] = n, f, s[b]
    if n <= 4:
        return new, row
    y = np.exp(s[f:] - Mg) - u
    if not y[0] > 0:
        return new, row
    m = 30 + int(math.floor(math.sqrt(float(n))))
    q = y[int(n / 4.0 + 0.5) - 1]
    with np.errstate(all='ignore'):
        theta = 1.0 / y[n - 1] + (1.0 - np.sqrt(m / (np.arange(1, m + 1) - 0.5))) / (3.0 * q)
        kap = np.array([np.sum(np.log1p(-t * y)) / n for t in theta])
        L = n * (np.log(-theta / kap) - kap - 1.0)
        omega = np.array([1.0 / np.sum(np.exp(L - Lj)) for Lj in L])
        that = np.sum(omega * theta)
        kappa = np.sum(np.log1p(-that * y)) / n
        sigma = -kappa / that
        khat = (n * kappa + 5.0) / (n + 10.0)
        row[0], row[1], row[3] = khat, sigma, m
        if want_weights and np.isfinite(khat):
            lp = np.log1p(-(np.arange(n) + 0.5) / n)
            w = u - sigma * lp if khat == 0 else u + sigma * np.expm1(-khat * lp) / khat
            new[order[f:]] = (np.minimum(np.log(w), 0.0) + Mg).astype(np.float32).astype(np.float64)
    return new, row


def _host_gmm(lw, x, init, max_iter, tol, reg_covar):
    """pp_is_gmm_groups' definition (include/pyprob_amd.h) in float64 numpy for one particle set: its output row [3 K + 6]."""
    K = len(init) // 3
    pi, mu, v = (np.array(init[j * K:(j + 1) * K], np.float64) for j in range(3))
    fin = np.isfinite(lw)
    if not fin.any():
        return np.concatenate([np.full(3 * K + 1, np.nan), [0.0, 1.0, 0.0, 0.0, -np.inf]])
    top = lw[fin].max()
    w, xs = np.exp(lw[fin] - top), np.asarray(x, np.float64)[fin]
    W = w.sum()
    before, lb, n_iter, converged = -np.inf, np.nan, 0, False
    with np.errstate(all='ignore'):
        for t in range(1, max_iter + 1):
            d = xs[:, None] - mu[None, :]
            l = np.log(pi) - 0.5 * np.log(2.0 * np.pi * v) - d * d / (2.0 * v)
            m = l.max(1)
            L = m + np.log(np.exp(l - m[:, None]).sum(1))
            r = w[:, None] * np.exp(l - L[:, None])
            lb = float((w * L).sum() / W)
            N = r.sum(0) + 10.0 * np.finfo(np.float64).eps
            dk = (r * d).sum(0) / N
            mu = mu + dk
            v = np.maximum((r * d * d).sum(0) / N - dk * dk, 0.0) + reg_covar
            pi = N / N.sum()
            n_iter = t
            if abs(lb - before) < tol:
                converged = True
                break
            before = lb
    return np.concatenate([pi, mu, v, [lb, float(n_iter), float(converged), W, float(fin.sum()), top]])
