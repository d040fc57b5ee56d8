"""Record tests/golden/dist_lp.npz: the reference's own distribution classes (pyprob/distributions/{exponential,gamma,beta,
log_normal,weibull,binomial,von_mises,truncated_normal}.py) evaluated in fp32 on a parameter x value grid, plus their
mean / stddev. Runs only where the reference tree exists (default /root/reference; --reference PATH); the tests read the
.npz alone.

Per family F the file holds F_params [P, 4] (the constructor's parameters in pp_dist order p0..p3), F_x [P, V], F_lp [P, V]
(log_prob of the reference class; -inf where x lies outside the family's support - the convention of the device kernels,
where torch would raise or return NaN), F_mean [P], F_stddev [P]. Binomial records total_count and the logits torch derives
from probs (the device reads the logits, like torch's Binomial.log_prob). TruncatedNormal rows with p4 = 1 were built with
clamp_mean_between_low_high=True; F_params then holds the clamped mean (what the device receives from the host).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

GRID = {
    'Exponential': [(0.5,), (1.0,), (3.0,)],
    'Gamma': [(1.0, 1.0), (2.5, 0.5), (0.3, 2.0), (0.05, 1.0), (30.0, 4.0)],
    'Beta': [(2.0, 3.0, 0.0, 1.0), (0.5, 0.5, 0.0, 1.0), (1.0, 1.0, -2.0, 3.0), (0.5, 1.0, 1.0, 4.0), (5.0, 2.0, -1.0, 1.0)],
    'LogNormal': [(0.0, 1.0), (1.5, 0.3), (-1.0, 2.0)],
    'Weibull': [(1.0, 1.0), (2.0, 0.5), (0.5, 3.0)],
    'Binomial': [(10.0, 0.3), (1.0, 0.5), (50.0, 0.9), (200.0, 0.02)],
    'VonMises': [(0.0, 0.5), (1.0, 2.0), (-2.0, 3.75), (0.5, 50.0), (0.0, 500.0)],
    'TruncatedNormal': [(0.0, 1.0, -1.0, 2.0), (2.0, 0.5, 0.0, 1.0), (-1.0, 3.0, -5.0, 5.0), (5.0, 1.0, 0.0, 2.0)],
}


def values(name, p):
    if name in ('Exponential', 'Gamma'):
        return [-1.0, 0.0, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 20.0]
    if name == 'Beta':
        lo, hi = p[2], p[3]
        return [lo - 0.5, lo] + [lo + f * (hi - lo) for f in (1e-3, 0.1, 0.3, 0.5, 0.77, 0.999)] + [hi, hi + 0.5]
    if name in ('LogNormal', 'Weibull'):
        return [-1.0, 0.0, 1e-3, 0.1, 0.5, 1.0, 2.5, 7.0, 30.0]
    if name == 'Binomial':
        n = p[0]
        return [-1.0, 0.0, 1.0, 2.5, float(int(n // 3)), float(int(n // 2)), float(n - 1), float(n), float(n + 1)]
    if name == 'VonMises':
        return [-3.1, -2.0, -0.5, 0.0, 0.3, 1.0, 2.5, 3.14, 7.0]
    lo, hi = p[2], p[3]
    return [lo - 1.0, lo, lo + 1e-3, 0.5 * (lo + hi), hi - 1e-3, hi, hi + 0.5, lo + 0.2 * (hi - lo), lo + 0.9 * (hi - lo)]


def in_support(name, p, x):
    if name in ('Exponential', 'Gamma'):
        return x >= 0
    if name in ('LogNormal', 'Weibull'):
        return x > 0
    if name == 'Beta':
        y = (np.float32(x) - np.float32(p[2])) / (np.float32(p[3]) - np.float32(p[2]))
        return 0 <= y <= 1
    if name == 'Binomial':
        return 0 <= x <= p[0] and x == int(x)
    if name == 'TruncatedNormal':
        return p[2] <= x <= p[3]
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, args.reference)
    import pyprob.distributions as R
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    out = {}
    for name, grid in GRID.items():
        rows = list(grid)
        if name == 'TruncatedNormal':
            rows = [r + (0.0,) for r in rows] + [(5.0, 1.0, 0.0, 2.0, 1.0), (-3.0, 0.5, -1.0, 1.0, 1.0)]
        P, X, LP, M, S = [], [], [], [], []
        for p in rows:
            if name == 'Exponential':
                d = R.Exponential(f32(p[0]))
                pp = (p[0], 0, 0, 0)
            elif name == 'Gamma':
                d = R.Gamma(f32(p[0]), f32(p[1]))
                pp = p + (0, 0)
            elif name == 'Beta':
                d = R.Beta(f32(p[0]), f32(p[1]), low=f32(p[2]), high=f32(p[3]))
                pp = p
            elif name == 'LogNormal':
                d = R.LogNormal(f32(p[0]), f32(p[1]))
                pp = p + (0, 0)
            elif name == 'Weibull':
                d = R.Weibull(f32(p[0]), f32(p[1]))
                pp = p + (0, 0)
            elif name == 'Binomial':
                d = R.Binomial(total_count=p[0], probs=f32(p[1]))
                pp = (p[0], float(d.logits), 0, 0)
            elif name == 'VonMises':
                d = R.VonMises(f32(p[0]), f32(p[1]))
                pp = p + (0, 0)
            else:
                d = R.TruncatedNormal(f32(p[0]), f32(p[1]), f32(p[2]), f32(p[3]), clamp_mean_between_low_high=bool(p[4]))
                pp = (float(d.mean_non_truncated), p[1], p[2], p[3])
            xs = values(name, pp)
            lp = []
            for x in xs:
                if not in_support(name, pp, x):
                    lp.append(-np.inf)
                    continue
                torch.distributions.Distribution.set_default_validate_args(False)
                lp.append(float(d.log_prob(f32(x))))
            P.append(pp)
            X.append(xs)
            LP.append(lp)
            M.append(float(d.mean))
            S.append(float(d.stddev) if hasattr(d, 'stddev') else float(d.variance) ** 0.5)
        out[name + '_params'] = np.asarray(P, np.float32)
        out[name + '_x'] = np.asarray(X, np.float32)
        out[name + '_lp'] = np.asarray(LP, np.float32)
        out[name + '_mean'] = np.asarray(M, np.float32)
        out[name + '_stddev'] = np.asarray(S, np.float32)
    path = os.path.join(HERE, 'dist_lp.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
