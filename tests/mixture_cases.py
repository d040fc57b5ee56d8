"""Shared by the Mixture tests (test_mixture.py, test_gpu_mixture.py): the golden cases of tests/golden/mixture_lp.npz
(make_mixture_golden.py) as mirror objects and as operator arguments, and float64 restatements of the mixture log-density and
CDF."""
import math
import os

import numpy as np
import torch

from conftest import GOLDEN

from pyprob_amd import distributions as D

KIND = {'Normal': 0, 'Uniform': 1, 'Poisson': 3, 'Bernoulli': 4, 'Exponential': 6, 'Gamma': 7, 'Beta': 8, 'LogNormal': 9,
        'Weibull': 10, 'Binomial': 11, 'VonMises': 12, 'TruncatedNormal': 13}
NPAR = {'Normal': 2, 'Uniform': 2, 'Poisson': 1, 'Bernoulli': 1, 'Exponential': 1, 'Gamma': 2, 'Beta': 4, 'LogNormal': 2,
        'Weibull': 2, 'Binomial': 2, 'VonMises': 2, 'TruncatedNormal': 4}
_GOLDEN = []


def golden():
    if not _GOLDEN:
        _GOLDEN.append(dict(np.load(os.path.join(GOLDEN, 'mixture_lp.npz'))))
    return _GOLDEN[0]


def cases():
    return [str(c) for c in golden()['cases']]


def component(name, p):
    """The mirror object of one component; p = its parameters in pp_dist order (floats or tensors)."""
    p = list(p)[:NPAR[name]]
    if name == 'Beta':
        return D.Beta(p[0], p[1], low=p[2], high=p[3])
    if name == 'Binomial':
        return D.Binomial(total_count=p[0], logits=p[1])
    return getattr(D, name)(*p)


def mirror(case):
    g = golden()
    names, params = [str(s) for s in g[case + '_names']], g[case + '_params']

    def par(v):       # [B] -> a float (B = 1) or a tensor
        return float(v[0]) if v.shape[0] == 1 else torch.from_numpy(v.copy())
    return D.Mixture([component(nm, [par(params[k, q]) for q in range(4)]) for k, nm in enumerate(names)],
                     probs=torch.from_numpy(g[case + '_probs'].copy()))


def _lgamma(x):
    return np.vectorize(math.lgamma)(np.asarray(x, np.float64))


def _phi(z):
    return 0.5 * (1 + np.vectorize(math.erf)(np.asarray(z, np.float64) / math.sqrt(2)))


def comp_lp64(name, p, x):
    """float64 log-density of one component; p = [p0..p3], each a float or an array like x. -inf outside the support."""
    x = np.asarray(x, np.float64)
    p = [np.asarray(v, np.float64) for v in p]
    with np.errstate(all='ignore'):
        if name == 'Normal':
            out, ok = -(x - p[0]) ** 2 / (2 * p[1] ** 2) - np.log(p[1]) - 0.5 * math.log(2 * math.pi), np.ones_like(x, bool)
        elif name == 'Uniform':
            out, ok = -np.log(p[1] - p[0]) + 0 * x, (x >= p[0]) & (x < p[1])
        elif name == 'Exponential':
            out, ok = np.log(p[0]) - p[0] * x, x >= 0
        elif name == 'Gamma':
            out = p[0] * np.log(p[1]) + np.where(p[0] == 1, 0.0, (p[0] - 1) * np.log(x)) - p[1] * x - _lgamma(p[0])
            ok = x >= 0
        elif name == 'LogNormal':
            ly = np.log(x)
            out, ok = -(ly - p[0]) ** 2 / (2 * p[1] ** 2) - np.log(p[1]) - 0.5 * math.log(2 * math.pi) - ly, x > 0
        elif name == 'Weibull':
            z = x / p[0]
            out, ok = np.log(p[1]) - np.log(p[0]) + (p[1] - 1) * np.log(z) - z ** p[1], x > 0
        elif name == 'Beta':
            y = (x - p[2]) / (p[3] - p[2])
            out = (np.where(p[0] == 1, 0, (p[0] - 1) * np.log(y)) + np.where(p[1] == 1, 0, (p[1] - 1) * np.log1p(-y)) +
                   _lgamma(p[0] + p[1]) - _lgamma(p[0]) - _lgamma(p[1]))
            ok = (y >= 0) & (y <= 1)
        elif name == 'TruncatedNormal':
            mu, sd, lo, hi = p
            z = (x - mu) / sd
            out = -0.5 * z * z - 0.5 * math.log(2 * math.pi) - np.log(sd * (_phi((hi - mu) / sd) - _phi((lo - mu) / sd)))
            ok = (x >= lo) & (x <= hi)
        else:
            raise NotImplementedError(name)
    return np.where(ok, out, -np.inf)


def mix_lp64(names, params, probs, x):
    """float64 Mixture.log_prob: params[k] = [p0..p3] (floats or [n] arrays), probs [K] or [n, K] unnormalised, x [n]."""
    x = np.asarray(x, np.float64)
    probs = np.asarray(probs, np.float64)
    q = probs / probs.sum(-1, keepdims=True)
    eps = 2.0 ** -23
    lq = np.log(np.clip(q, eps, 1 - eps))
    t = np.stack([comp_lp64(nm, params[k], x) for k, nm in enumerate(names)], -1) + lq
    with np.errstate(all='ignore'):
        m = t.max(-1)
        out = m + np.log(np.exp(t - np.where(np.isfinite(m), m, 0.0)[..., None]).sum(-1))
    return np.where(np.isneginf(m), -np.inf, out)


def comp_cdf64(name, p, x):
    x = np.asarray(x, np.float64)
    if name == 'Normal':
        return _phi((x - p[0]) / p[1])
    if name == 'Uniform':
        return np.clip((x - p[0]) / (p[1] - p[0]), 0.0, 1.0)
    if name == 'Exponential':
        return np.where(x > 0, -np.expm1(-p[0] * np.maximum(x, 0.0)), 0.0)
    raise NotImplementedError(name)


def mix_cdf64(names, params, probs, x):
    probs = np.asarray(probs, np.float64)
    q = probs / probs.sum()
    return sum(q[k] * comp_cdf64(nm, params[k], x) for k, nm in enumerate(names))


def ks_distance(values, cdf):
    """Kolmogorov distance of fp32 draws from a float64 CDF, evaluated at the midpoints to each value's fp32 neighbours (the draws
    are roundings of the true variates: test_gpu_dist_kernels.test_continuous_sampler_ks_and_moments)."""
    x32 = np.sort(np.asarray(values, np.float32))
    up = 0.5 * (x32.astype(np.float64) + np.nextafter(x32, np.float32(np.inf)).astype(np.float64))
    lo = 0.5 * (x32.astype(np.float64) + np.nextafter(x32, np.float32(-np.inf)).astype(np.float64))
    n = x32.size
    i = np.arange(1, n + 1, dtype=np.float64)
    return max(float((i / n - cdf(up)).max()), float((cdf(lo) - (i - 1) / n).max()))


# ---- operator arguments ---------------------------------------------------------------------------------------------------
def op_args(names, params, device):
    """(kinds [K], parameters [4 K], strides [4 K]) of pyprob_hip::mix_*: params[k] = the component's parameters (floats or
    [n] tensors)."""
    kinds, ps, ss = [], [], []
    for nm, p in zip(names, params):
        kinds.append(KIND[nm])
        for q in range(4):
            if q < NPAR[nm]:
                t = torch.as_tensor(p[q], dtype=torch.float32).reshape(-1).to(device).contiguous()
                ps.append(t)
                ss.append(0 if t.numel() == 1 else 1)
            else:
                ps.append(None)
                ss.append(0)
    return kinds, ps, ss


def register_mix_cpu_doubles(registered=[]):
    """TEST DOUBLES: "CPU" kernels for pyprob_hip::mix_logweight / mix_draw (the product registers the device kernels only),
    restated with the mirror Mixture's log_prob and sample_n - enough to run the host logic of a lock-step call without a
    device (the pattern of test_dist_families._register_dist_cpu_doubles)."""
    if registered:
        return
    from pyprob_amd import ops as P
    names = {v: k for k, v in KIND.items()}

    def mixture(kinds, params, probs, n, idx):
        comps = []
        for k, kind in enumerate(kinds):
            p = [None if t is None else t.reshape(-1).expand(n)[idx] for t in params[4 * k:4 * k + 4]]
            comps.append(component(names[int(kind)], p))
        K = len(kinds)
        return D.Mixture(comps, probs=probs.reshape(-1, K).expand(n, K)[idx])

    def logweight_cpu(lw, kinds, params, strides, probs, x, scale, rows, lp_out, n):
        idx = torch.arange(n) if rows is None else rows
        lp = mixture(kinds, params, probs, n, idx).log_prob(x.reshape(-1).expand(n)[idx]).reshape(-1).float()
        if lp_out is not None:
            lp_out[idx] = lp
        if lw is not None:
            lw[idx] += float(scale) * lp

    def draw_cpu(kinds, params, strides, probs, rows, out, seed, offset, stream_id):
        n = out.numel()
        idx = torch.arange(n) if rows is None else rows
        out[idx] = mixture(kinds, params, probs, n, idx).sample_n(idx.numel())

    P._lib.impl('mix_logweight', logweight_cpu, 'CPU')
    P._lib.impl('mix_draw', draw_cpu, 'CPU')
    registered.append(True)
