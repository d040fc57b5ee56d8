"""Float64 restatement of pp_obs_logweight (include/pyprob_amd.h) for the tests: the per-element log-densities of the 12 scalar
families (kinds 0, 1, 3, 4, 6-13) with the support guards of csrc/dist_math.hpp, their sum over a row, and a CPU double of the
`obs_logweight` operator."""
import numpy as np
import torch

KINDS = (0, 1, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13)
N_PARAMS = {0: 2, 1: 2, 3: 1, 4: 1, 6: 1, 7: 2, 8: 4, 9: 2, 10: 2, 11: 2, 12: 2, 13: 4}
NAMES = {0: 'Normal', 1: 'Uniform', 3: 'Poisson', 4: 'Bernoulli', 6: 'Exponential', 7: 'Gamma', 8: 'Beta', 9: 'LogNormal',
         10: 'Weibull', 11: 'Binomial', 12: 'VonMises', 13: 'TruncatedNormal'}
_HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
_EPS = float(np.finfo(np.float32).eps)


def _lgamma(a):
    return torch.lgamma(torch.from_numpy(np.ascontiguousarray(a, np.float64))).numpy()


def _ndtr(a):
    return torch.special.ndtr(torch.from_numpy(np.ascontiguousarray(a, np.float64))).numpy()


def _log_i0(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float64))
    return (torch.log(torch.special.i0e(t)) + t.abs()).numpy()


def _xlogy(a, x):
    with np.errstate(all='ignore'):
        return np.where((a == 0) & ~np.isnan(x), 0.0, a * np.log(x))


def elem_lp(kind, p, x):
    """log p_kind(x | p[0..3]) elementwise in float64 (p: float64 arrays broadcastable with x); -inf outside the support."""
    a = p[0]
    b = p[1] if len(p) > 1 else None
    with np.errstate(all='ignore'):
        if kind == 0:
            return -((x - a) ** 2) / (2.0 * b * b) - np.log(b) - _HALF_LOG_2PI
        if kind == 1:
            return np.where((x >= a) & (x < b), -np.log(b - a), -np.inf)
        if kind == 3:
            return np.where((x >= 0) & (x == np.floor(x)), _xlogy(x, a) - a - _lgamma(np.maximum(x, 0) + 1.0), -np.inf)
        if kind == 4:
            q = np.clip(a, _EPS, 1.0 - _EPS)
            return np.where((x == 0) | (x == 1), x * np.log(q) + (1.0 - x) * np.log1p(-q), -np.inf)
        if kind == 6:
            return np.where(x >= 0, np.log(a) - a * x, -np.inf)
        if kind == 7:
            return np.where(x >= 0, _xlogy(a, b) + _xlogy(a - 1.0, x) - b * x - _lgamma(a), -np.inf)
        if kind == 8:
            y = (x - p[2]) / (p[3] - p[2])
            lp = _xlogy(a - 1.0, y) + _xlogy(b - 1.0, 1.0 - y) + _lgamma(a + b) - _lgamma(a) - _lgamma(b)
            return np.where((y >= 0) & (y <= 1), lp, -np.inf)
        if kind == 9:
            y = np.log(x)
            return np.where(x > 0, -((y - a) ** 2) / (2.0 * b * b) - np.log(b) - _HALF_LOG_2PI - y, -np.inf)
        if kind == 10:
            z = x / a
            return np.where(x > 0, np.log(b) - np.log(a) + (b - 1.0) * np.log(z) - z ** b, -np.inf)
        if kind == 11:
            norm = a * np.maximum(b, 0.0) + a * np.log1p(np.exp(-np.abs(b))) - _lgamma(a + 1.0)
            lp = x * b - _lgamma(np.maximum(x, 0) + 1.0) - _lgamma(np.maximum(a - x, 0) + 1.0) - norm
            return np.where((x >= 0) & (x <= a) & (x == np.floor(x)), lp, -np.inf)
        if kind == 12:
            return np.where(np.isfinite(x), b * np.cos(x - a) - 2.0 * _HALF_LOG_2PI - _log_i0(b), -np.inf)
        lo, hi = p[2], p[3]
        z = (x - a) / b
        Z = _ndtr((hi - a) / b) - _ndtr((lo - a) / b)
        return np.where((x >= lo) & (x <= hi), -(z * z) / 2.0 - _HALF_LOG_2PI - np.log(b * Z), -np.inf)


def operand(t, n, k):
    """A scalar, [k], [1, k], [n], [n, 1], [n, k] or [n, *event] operand as a float64 [n, k] array (pyprob_amd.ops.obs_draw_strides'
    readings: a 1-D tensor of k elements is the shared row also when n == k)."""
    a = np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, np.float64)
    if a.size == 1:
        return np.broadcast_to(a.reshape(1, 1), (n, k))
    if a.shape in ((k,), (1, k)):
        return np.broadcast_to(a.reshape(1, k), (n, k))
    if a.shape in ((n,), (n, 1)):
        return np.broadcast_to(a.reshape(n, 1), (n, k))
    assert a.shape[0] == n and a.size == n * k, (a.shape, n, k)
    return a.reshape(n, k)


def row_lp(kind, params, x, n, k):
    """lp[r] = sum_e log p_kind(x[r, e] | params[.][r, e]) in float64, and the sum of |terms| (the tests' summation bound)."""
    ps = [operand(q, n, k) for q in params[:N_PARAMS[kind]]]
    e = elem_lp(kind, ps, operand(x, n, k))
    with np.errstate(all='ignore'):
        return e.sum(1), np.abs(e).sum(1)


calls = [0]      # how often the CPU double ran


def obs_logweight_cpu(lw, kind, params, x, k, scale, rows, lp_out, n):
    """The operator's CPU double (the product registers the device implementation only); counts its calls."""
    calls[0] += 1
    with np.errstate(all='ignore'):      # (stale parameters of particles off the path may be anything)
        lp = torch.from_numpy(row_lp(int(kind), list(params), x, int(n), int(k))[0].astype(np.float32))
    idx = slice(None) if rows is None else rows
    if lp_out is not None:
        lp_out[idx] = lp[idx]
    if lw is not None:
        lw[idx] += np.float32(scale) * lp[idx]


_registered = False


def register_cpu_double():
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('obs_logweight', obs_logweight_cpu, 'CPU')
        _registered = True
