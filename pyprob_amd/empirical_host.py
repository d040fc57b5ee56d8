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


def _host_twosample(lw_a, x_a, lw_b, x_b):
    """pp_is_twosample_groups' definition (include/pyprob_amd.h) in float64 numpy for one pair of particle sets: its row of 8 - ks,
    ks_location, wasserstein1, wasserstein2, energy, the two counts, the merged position of the ks maximum."""
    ca, cb = len(_host_order(lw_a, x_a)), len(_host_order(lw_b, x_b))
    a, wa = _host_sorted_cdf(lw_a, x_a)
    b, wb = _host_sorted_cdf(lw_b, x_b)
    row = np.array([np.nan, np.nan, np.nan, np.nan, np.nan, float(ca), float(cb), np.nan])
    if a is None or b is None:
        return row
    ua, ub = wa / wa[-1], wb / wb[-1]
    from_a = np.arange(ca + cb) < ca                    # (of the concatenation: a stable sort takes A before B on ties)

    def merged(keys_a, keys_b):
        """(the keys in merged order, how many of each side are consumed AFTER every merged element, whether it came from A)."""
        keys = np.concatenate([keys_a, keys_b])
        order = np.argsort(keys, kind='stable')
        i = np.cumsum(from_a[order])
        return keys[order], i, np.arange(1, ca + cb + 1) - i, from_a[order]
    with np.errstate(invalid='ignore', over='ignore'):
        # the value walk: F - G after every merged element, steps where the next value is larger
        z, i, j, _ = merged(a, b)
        D = np.where(i > 0, ua[np.maximum(i, 1) - 1], 0.0) - np.where(j > 0, ub[np.maximum(j, 1) - 1], 0.0)
        step = np.append(z[1:] > z[:-1], False)
        end = step.copy()
        end[-1] = True
        k = int(np.argmax(np.where(end, np.abs(D), -1.0)))          # (the first maximum)
        term = step & (D != 0)
        gap = np.append(z[1:], z[-1])[term] - z[term]
        # the quantile walk: both quantile functions between two merged u, the heads BEFORE every element
        u, i, j, was_a = merged(ua, ub)
        prev = np.concatenate([[0.0], u[:-1]])
        x, y = a[np.minimum(i - was_a, ca - 1)], b[np.minimum(j - ~was_a, cb - 1)]
        d = np.where(x == y, 0.0, x - y)
        wide = u > prev
        row[:5] = (abs(D[k]), z[k], np.sum(np.abs(D[term]) * gap), math.sqrt(np.sum((u - prev)[wide] * d[wide] ** 2)),
                   2.0 * np.sum(D[term] ** 2 * gap))
    row[7] = k
    return row


def _pairs_standardise(mean_a, var_a, mean_b, var_b, scale):
    """(center, scale) [.., J] of compare_joint from the means and variances of the two sides: the mean and the standard deviation of
    their equal mixture, or the caller's J positive numbers in place of the latter."""
    mean_a, mean_b = np.asarray(mean_a, np.float64), np.asarray(mean_b, np.float64)
    center = 0.5 * (mean_a + mean_b)
    if scale is None:
        s = np.sqrt(0.5 * (np.asarray(var_a, np.float64) + np.asarray(var_b, np.float64)) + 0.25 * (mean_a - mean_b) ** 2)
    else:
        s = np.asarray(scale, np.float64).reshape(-1)
        if s.shape[0] != center.shape[-1] or not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError('scale= takes %d finite positive numbers, one per address' % center.shape[-1])
        s = np.array(np.broadcast_to(s, center.shape))
    if not np.isfinite(center).all() or not np.isfinite(s).all():
        raise ValueError('the joint moments of a side are not finite (no particle with a weight, or a NaN or infinite coordinate '
                         'under a finite weight): nothing to standardise by')
    if (s == 0).any():
        raise ValueError('an address has no spread on either side: pass scale= (J positive numbers)')
    return center, s


def _pairs_bandwidth(bandwidth, J):
    h = math.sqrt(J) if bandwidth is None else float(bandwidth)
    if not (math.isfinite(h) and h > 0):
        raise ValueError('bandwidth must be a finite positive number (standardised units)')
    return h


def _host_twosample_joint(lw_a, x_a, lw_b, x_b, bandwidth=None, scale=None, chunk=1024):
    """pp_is_pairs_groups' row of 10 (include/pyprob_amd.h) for one pair of particle sets in chunked float64 numpy, with the
    standardisation of compare_joint in front: (row, center, scale, bandwidth). x_*: [n, J]; a particle counts where its log-weight is
    finite and its J coordinates are. The moments are joint()'s: over the particles with a finite log-weight."""
    sides = []
    for lw, x in ((lw_a, x_a), (lw_b, x_b)):
        lw, x = np.asarray(lw, np.float64).reshape(-1), np.asarray(x, np.float64)
        x = x.reshape(len(lw), -1)
        fin = np.isfinite(lw)
        w = np.where(fin, np.exp(lw - (lw[fin].max() if fin.any() else 0.0)), 0.0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = (w[fin, None] * x[fin]).sum(0) / w.sum()
            var = np.maximum((w[fin, None] * (x[fin] - mean) ** 2).sum(0) / w.sum(), 0.0)
        sides.append((w, x, mean, var))
    J = sides[0][1].shape[1]
    if sides[1][1].shape[1] != J or not 1 <= J <= 8:
        raise ValueError('compare_joint takes 1 .. 8 addresses, the same on both sides')
    h = _pairs_bandwidth(bandwidth, J)
    center, s = _pairs_standardise(sides[0][2], sides[0][3], sides[1][2], sides[1][3], scale)
    parts = []
    for (w, x, _, _), lw in zip(sides, (lw_a, lw_b)):
        with np.errstate(invalid='ignore'):
            z = (x - center) * (1.0 / s)
        keep = np.isfinite(z).all(1) & np.isfinite(np.asarray(lw, np.float64).reshape(-1))
        parts.append((z[keep], w[keep]))
    row = np.full(10, np.nan)
    row[8], row[9] = len(parts[0][1]), len(parts[1][1])

    def sums(p, q):
        (zp, wp), (zq, wq) = p, q
        k = d = 0.0
        for i in range(0, len(wp), chunk):
            diff = zp[i:i + chunk, None, :] - zq[None, :, :]
            r2 = (diff * diff).sum(-1)
            ww = wp[i:i + chunk, None] * wq[None, :]
            k += (ww * np.exp(r2 * (-0.5 / (h * h)))).sum()
            d += (ww * np.sqrt(r2)).sum()
        with np.errstate(invalid='ignore', divide='ignore'):
            norm = wp.sum() * wq.sum()
            return np.float64(k) / norm, np.float64(d) / norm
    (row[0], row[3]), (row[1], row[4]), (row[2], row[5]) = sums(parts[0], parts[0]), sums(parts[1], parts[1]), sums(parts[0], parts[1])
    with np.errstate(invalid='ignore', divide='ignore'):
        row[6], row[7] = [np.float64((w * w).sum()) / np.float64(w.sum()) ** 2 for _, w in parts]
    return row, center, s, h


def _sinkhorn_epsilon(epsilon, J):
    eps = 0.05 * J if epsilon is None else float(epsilon)
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError('epsilon must be a finite positive number (standardised units squared)')
    return eps


def _sinkhorn_softmin(z_s, logw_s, pot_s, z_q, eps, chunk=256):
    """-eps log sum_i w_i exp((pot_i - |z_i - zq|^2 / 2) / eps) per query [Q] in chunked float64 numpy, the maximum of the exponents
    taken out before the exponential."""
    out = np.empty(len(z_q))
    for a in range(0, len(z_q), chunk):
        r2 = np.zeros((len(z_q[a:a + chunk]), len(z_s)))
        for j in range(z_s.shape[1]):
            r2 += (z_q[a:a + chunk, j, None] - z_s[None, :, j]) ** 2
        e = logw_s[None, :] + (pot_s[None, :] - 0.5 * r2) / eps
        m = e.max(1)
        out[a:a + chunk] = -eps * (m + np.log(np.exp(e - m[:, None]).sum(1)))
    return out


def _host_sinkhorn(lw_a, x_a, lw_b, x_b, center, scale, epsilon, tol=1e-3, max_iter=1000):
    """pp_is_sinkhorn_groups' definition (include/pyprob_amd.h) for one pair of particle sets in chunked float64 numpy: (row of 12, f
    [n_a], g [n_b], p_a [n_a], p_b [n_b], peak [3]), the potentials NaN where a particle does not count and peak the largest |potential|
    any iteration of problem ab, aa, bb saw (what the device's error bound takes). x_*: [n, J]."""
    eps, tol, max_iter = float(epsilon), float(tol), int(max_iter)
    sides, full = [], []
    for lw, x in ((lw_a, x_a), (lw_b, x_b)):
        lw, x = np.asarray(lw, np.float64).reshape(-1), np.asarray(x, np.float64)
        with np.errstate(invalid='ignore'):
            z = (x.reshape(len(lw), -1) - center) * (1.0 / scale)
        keep = np.isfinite(lw) & np.isfinite(z).all(1)
        sides.append(_kdej_counted(lw, x, center, scale))
        full.append(keep)
    (za, la), (zb, lb) = sides
    row = np.full(12, np.nan)
    row[3:6], row[9], row[10] = 0.0, len(la), len(lb)

    def spread(pot, keep):
        out = np.full(len(keep), np.nan)
        out[keep] = pot
        return out
    if len(la) == 0 or len(lb) == 0:
        row[11] = 8.0
        return (row,) + tuple(np.full(len(k), np.nan) for k in (full[0], full[1], full[0], full[1])) + (np.full(3, np.nan),)
    status, peak = 0, np.zeros(3)
    f, g = np.zeros(len(la)), np.zeros(len(lb))
    for it in range(1, max_iter + 1):
        g_new = _sinkhorn_softmin(za, la, f, zb, eps)
        f_new = _sinkhorn_softmin(zb, lb, g_new, za, eps)
        row[6] = max(np.abs(f_new - f).max(), np.abs(g_new - g).max()) / eps
        f, g, row[3] = f_new, g_new, it
        peak[0] = max(peak[0], np.abs(f).max(), np.abs(g).max())
        if row[6] < tol:
            break
    else:
        status |= 1
    row[0] = (np.exp(la) * f).sum() + (np.exp(lb) * g).sum()
    pots = []
    for k, (z, l) in enumerate(sides):
        p = np.zeros(len(l))
        for it in range(1, max_iter + 1):
            p_new = 0.5 * (p + _sinkhorn_softmin(z, l, p, z, eps))
            row[7 + k] = np.abs(p_new - p).max() / eps
            p, row[4 + k] = p_new, it
            peak[1 + k] = max(peak[1 + k], np.abs(p).max())
            if row[7 + k] < tol:
                break
        else:
            status |= 2 << k
        row[1 + k] = 2.0 * (np.exp(l) * p).sum()
        pots.append(p)
    row[11] = status
    return row, spread(f, full[0]), spread(g, full[1]), spread(pots[0], full[0]), spread(pots[1], full[1]), peak


def _host_sinkhorn_map(lw_a, x_a, lw_b, x_b, center, scale, epsilon, f, g, chunk=256):
    """pp_is_sinkhorn_map_groups' definition (include/pyprob_amd.h) for one pair of particle sets in chunked float64 numpy: (map_ab [n_a,
    J], map_ba [n_b, J], log_mass_a [n_a], log_mass_b [n_b]) from the potentials f [n_a], g [n_b] (NaN allowed where a particle does
    not count), NaN rows where a particle does not count or a side has no counted particle. x_*: [n, J]."""
    eps, center, scale = float(epsilon), np.asarray(center, np.float64), np.asarray(scale, np.float64)
    sides = []
    for lw, x, pot in ((lw_a, x_a, f), (lw_b, x_b, g)):
        lw, x = np.asarray(lw, np.float64).reshape(-1), np.asarray(x, np.float64)
        with np.errstate(invalid='ignore'):
            keep = np.isfinite(lw) & np.isfinite((x.reshape(len(lw), -1) - center) * (1.0 / scale)).all(1)
        sides.append(_kdej_counted(lw, x, center, scale) + (np.asarray(pot, np.float64).reshape(-1)[keep], keep))
    out = []
    for (zq, _, pq, keep_q), (zs, ls, ps, _) in ((sides[0], sides[1]), (sides[1], sides[0])):
        T, mass = np.full((len(keep_q), zq.shape[1]), np.nan), np.full(len(keep_q), np.nan)
        if len(ls) and len(pq):
            mean, lm = np.empty_like(zq), np.empty(len(zq))
            for a in range(0, len(zq), chunk):
                r2 = np.zeros((len(zq[a:a + chunk]), len(zs)))
                for j in range(zs.shape[1]):
                    r2 += (zq[a:a + chunk, j, None] - zs[None, :, j]) ** 2
                e = ls[None, :] + (ps[None, :] - 0.5 * r2) / eps
                m = e.max(1)
                p = np.exp(e - m[:, None])
                mean[a:a + chunk] = (p @ zs) / p.sum(1)[:, None]
                lm[a:a + chunk] = pq[a:a + chunk] / eps + (m + np.log(p.sum(1)))
            T[keep_q], mass[keep_q] = center + scale * mean, lm
        out.append((T, mass))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _kdej_standardise(mean, stddev, scale):
    """(center, scale) [J] of kde_joint / modes: the object's own joint() mean and per-address standard deviation, or the caller's J
    positive numbers in place of the latter."""
    center = np.asarray(mean, np.float64).reshape(-1)
    if scale is None:
        s = np.asarray(stddev, np.float64).reshape(-1)
    else:
        s = np.asarray(scale, np.float64).reshape(-1)
        if s.shape != center.shape or not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError('scale= takes %d finite positive numbers, one per address' % center.shape[0])
    if not np.isfinite(center).all() or not np.isfinite(s).all():
        raise ValueError('the joint moments are not finite (no particle with a weight, or a NaN or infinite coordinate under a '
                         'finite weight): nothing to standardise by')
    if (s == 0).any():
        raise ValueError('an address has no spread: pass scale= (J positive numbers)')
    return center, s


def _host_joint_moments(lw, x):
    """(mean [J], stddev [J], ess, count) of joint(): over the particles with a finite log-weight, in float64 numpy."""
    lw, x = np.asarray(lw, np.float64).reshape(-1), np.asarray(x, np.float64)
    fin = np.isfinite(lw)
    w = np.where(fin, np.exp(lw - (lw[fin].max() if fin.any() else 0.0)), 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = (w[fin, None] * x[fin]).sum(0) / w.sum()
        std = np.sqrt(np.maximum((w[fin, None] * (x[fin] - mean) ** 2).sum(0) / w.sum(), 0.0))
        ess = float(w.sum() ** 2 / (w * w).sum())
    return mean, std, ess, int(fin.sum())


def _kdej_counted(lw, x, center, scale):
    """(z [c, J], log of the normalised weights [c]) of the particles pp_is_kde_joint_groups counts: a finite log-weight and J finite
    standardised coordinates."""
    lw, x = np.asarray(lw, np.float64).reshape(-1), np.asarray(x, np.float64)
    with np.errstate(invalid='ignore'):
        z = (x.reshape(len(lw), -1) - center) * (1.0 / scale)
    keep = np.isfinite(lw) & np.isfinite(z).all(1)
    z, lw = z[keep], lw[keep]
    if len(lw):
        lw = lw - lw.max()
        lw = lw - math.log(np.exp(lw).sum())
    return z, lw


def _kdej_at(z, logw, zq, h, want_mean, chunk=64):
    """log sum_i w_i N_J(zq; z_i, h^2 I) [Q] and the mean-shift mean [Q, J] (or None) in chunked float64 numpy, the maximum of the
    exponents taken out before the exponential as the device does."""
    Q, J = zq.shape
    logd, mean = np.full(Q, np.nan), (np.full((Q, J), np.nan) if want_mean else None)
    if len(logw) == 0:
        return logd, mean
    norm = J * (math.log(h) + 0.5 * math.log(2.0 * math.pi))
    for a in range(0, Q, chunk):
        with np.errstate(invalid='ignore', over='ignore'):
            diff = zq[a:a + chunk, None, :] - z[None, :, :]
            e = logw[None, :] - (diff * diff).sum(-1) * (0.5 / (h * h))
            m = np.nanmax(np.where(np.isnan(e), -np.inf, e), axis=1)
            p = np.exp(e - m[:, None])
            S = p.sum(1)
            logd[a:a + chunk] = m + np.log(S) - norm
            if want_mean:
                mean[a:a + chunk] = (p @ z) / S[:, None]
    return logd, mean


def _host_kde_joint(lw, x, center, scale, h, points, want_mean=False):
    """pp_is_kde_joint_groups' definition (include/pyprob_amd.h) for one particle set: x [n, J], points [Q, J] in the ORIGINAL
    coordinates. (log_density [Q] of the standardised coordinates, mean [Q, J] standardised or None, count)."""
    z, logw = _kdej_counted(lw, x, center, scale)
    with np.errstate(invalid='ignore'):
        zq = (np.asarray(points, np.float64).reshape(-1, len(center)) - center) * (1.0 / scale)
    logd, mean = _kdej_at(z, logw, zq, float(h), want_mean)
    return logd, mean, len(logw)


def _host_meanshift(lw, x, center, scale, h, seeds, tol, max_iter):
    """pp_is_meanshift_groups' definition for one particle set, seeds [S, J] STANDARDISED: (points [S, J], log_density [S], n_iter
    [S], converged [S], count)."""
    z, logw = _kdej_counted(lw, x, center, scale)
    pts = np.array(seeds, np.float64).reshape(-1, len(center))
    S = len(pts)
    state, n_iter = np.zeros(S, np.int64), np.zeros(S, np.int32)
    for it in range(1, int(max_iter) + 1):
        live = np.flatnonzero(state == 0)
        if len(live) == 0:
            break
        mean = _kdej_at(z, logw, pts[live], float(h), True)[1]
        step2 = ((mean - pts[live]) ** 2).sum(1)
        pts[live], n_iter[live] = mean, it
        state[live] = np.where(np.isnan(step2), 2, np.where(step2 < (tol * h) ** 2, 1, 0))
    return pts, _kdej_at(z, logw, pts, float(h), False)[0], n_iter, state == 1, len(logw)


def _merge_modes(points, log_density, h):
    """The end points of mean shift merged in float64: in descending order of density, a point within h / 2 of a mode's
    representative joins it, else it opens a mode. (the representatives' indices, the mode of every point or -1 for a NaN point)."""
    order = [int(i) for i in np.argsort(-np.where(np.isnan(log_density), -np.inf, log_density), kind='stable')]
    reps, label = [], np.full(len(points), -1, np.int64)
    for i in order:
        if not (np.isfinite(points[i]).all() and np.isfinite(log_density[i])):
            continue
        if reps:
            d2 = ((points[reps] - points[i]) ** 2).sum(1)
            k = int(np.argmin(d2))
            if d2[k] < 0.25 * h * h:
                label[i] = k
                continue
        label[i] = len(reps)
        reps.append(i)
    return np.asarray(reps, np.int64), label


def _kolmogorov_sf(lam):
    """P(K > lam) of the Kolmogorov distribution: the series 2 sum_k (-1)^(k-1) exp(-2 k^2 lam^2), below lam = 1.18 its theta-function
    form 1 - sqrt(2 pi) / lam sum_k exp(-(2 k - 1)^2 pi^2 / (8 lam^2)), which converges where the first does not."""
    lam = float(lam)
    if math.isnan(lam):
        return float('nan')
    if lam <= 0:
        return 1.0
    if lam < 1.18:
        y = math.exp(-math.pi ** 2 / (8.0 * lam * lam))
        p = 1.0 - math.sqrt(2.0 * math.pi) / lam * (y + y ** 9 + y ** 25 + y ** 49)
    else:
        x = math.exp(-2.0 * lam * lam)
        p = 2.0 * (x - x ** 4 + x ** 9)
    return min(max(p, 0.0), 1.0)


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


def _host_kde(lw, x, pts, h):
    """pp_is_kde_groups' definition in float64 numpy for one particle set: [2, Q] (density | log density) at the points pts under the
    bandwidth h, over the particles with a finite log-weight and a value that is not NaN. Nothing counted: NaN."""
    keep = np.isfinite(lw) & ~np.isnan(x)
    if not keep.any():
        return np.full((2, len(pts)), np.nan)
    v, w = x[keep], np.exp(lw[keep] - np.max(lw[np.isfinite(lw)]))
    dens = np.empty(len(pts))
    step = max(1, (1 << 22) // len(v))
    for q in range(0, len(pts), step):
        z = (pts[q:q + step, None] - v[None, :]) / h
        dens[q:q + step] = np.exp(-0.5 * z * z) @ w
    dens /= h * math.sqrt(2.0 * math.pi) * w.sum()
    with np.errstate(divide='ignore'):
        return np.stack([dens, np.log(dens)])


def _host_kde2d(lw, x, y, px, py, hx, hy):
    """pp_is_kde2d_groups' definition in float64 numpy for one particle set: [2, Qx, Qy] on the grid px x py (product kernel), over the
    particles with a finite log-weight and neither coordinate NaN."""
    keep = np.isfinite(lw) & ~np.isnan(x) & ~np.isnan(y)
    if not keep.any():
        return np.full((2, len(px), len(py)), np.nan)
    u, v, w = x[keep], y[keep], np.exp(lw[keep] - np.max(lw[np.isfinite(lw)]))
    dens = np.zeros((len(px), len(py)))
    step = max(1, (1 << 22) // max(len(px), len(py)))
    for i in range(0, len(u), step):
        zx = (px[:, None] - u[None, i:i + step]) / hx
        zy = (py[:, None] - v[None, i:i + step]) / hy
        dens += (np.exp(-0.5 * zx * zx) * w[i:i + step]) @ np.exp(-0.5 * zy * zy).T
    dens /= 2.0 * math.pi * hx * hy * w.sum()
    with np.errstate(divide='ignore'):
        return np.stack([dens, np.log(dens)])


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


def _cholesky_lower(cov):
    """(the lower Cholesky factors [K, J, J] of the K matrices whose UPPER triangles are read from cov [K, J, J], whether every
    pivot was positive) - all K matrices at once, column by column as pp_is_gmm_joint_groups factorises them."""
    K, J, _ = cov.shape
    L = np.zeros_like(cov)
    for j in range(J):
        for m in range(j + 1):
            s = cov[:, m, j] - (L[:, j, :m] * L[:, m, :m]).sum(1)
            if m < j:
                L[:, j, m] = s / L[:, m, m]
            elif not (s > 0).all():
                return L, False
            else:
                L[:, j, j] = np.sqrt(s)
    return L, True


def _host_gmm_joint(lw, cols, init, K, max_iter, tol, reg_covar):
    """pp_is_gmm_joint_groups' definition (include/pyprob_amd.h) in float64 numpy for one particle set: cols [J, n], init
    [K (1 + J + J (J + 1) / 2)] = weights | means | covariances (upper triangles); its output row."""
    lw, cols = np.asarray(lw, np.float64), np.asarray(cols, np.float64)
    J = cols.shape[0]
    iu, ku = np.triu_indices(J)
    init = np.asarray(init, np.float64)
    pi, mu = init[:K].copy(), init[K:K + K * J].reshape(K, J).copy()
    cov = np.zeros((K, J, J))
    cov[:, iu, ku] = init[K + K * J:].reshape(K, len(iu))
    cov[:, ku, iu] = cov[:, iu, ku]

    def row(pi, mu, cov, *tail):
        return np.concatenate([pi, mu.reshape(-1), cov[:, iu, ku].reshape(-1), tail])
    fin = np.isfinite(lw)
    keep = fin & np.isfinite(cols).all(0)
    top = lw[fin].max() if fin.any() else -np.inf
    L, ok = _cholesky_lower(cov)
    if not ok:
        return row(pi, mu, cov, -np.inf, 0.0, 0.0, 1.0, 0.0, 0.0, -np.inf)
    if not keep.any():
        return row(pi * np.nan, mu * np.nan, cov * np.nan, np.nan, 0.0, 1.0, 0.0, 0.0, 0.0, top)
    w, x = np.exp(lw[keep] - top), cols[:, keep].T
    W, eye = w.sum(), np.eye(J)
    before, lb, n_iter, converged = -np.inf, np.nan, 0, False
    with np.errstate(all='ignore'):
        for t in range(1, max_iter + 1):
            l = np.empty((len(w), K))
            for k in range(K):
                z = np.linalg.solve(L[k], (x - mu[k]).T)
                l[:, k] = np.log(pi[k]) - 0.5 * J * np.log(2.0 * np.pi) - np.log(np.diag(L[k])).sum() - 0.5 * (z * z).sum(0)
            m = l.max(1)
            Li = m + np.log(np.exp(l - m[:, None]).sum(1))
            r = w[:, None] * np.exp(l - Li[:, None])
            lb = float((w * Li).sum() / W)
            N = r.sum(0) + 10.0 * np.finfo(np.float64).eps
            new_mu, new_cov = np.empty_like(mu), np.empty_like(cov)
            for k in range(K):
                d = x - mu[k]
                rd = r[:, k, None] * d
                s = rd.sum(0) / N[k]
                new_mu[k] = mu[k] + s
                new_cov[k] = rd.T @ d / N[k] - np.outer(s, s) + reg_covar * eye
            new_L, ok = _cholesky_lower(new_cov)
            n_iter = t
            if not ok:       # (degenerate: the parameters from before this M-step)
                return row(pi, mu, cov, lb, float(t), 0.0, 1.0, W, float(keep.sum()), top)
            pi, mu, cov, L = N / N.sum(), new_mu, new_cov, new_L
            if abs(lb - before) < tol:
                converged = True
                break
            before = lb
    return row(pi, mu, cov, lb, float(n_iter), float(converged), 0.0, W, float(keep.sum()), top)
