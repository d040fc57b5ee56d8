"""Record tests/golden/dist_edges.npz: the reference's own distribution classes (pyprob/distributions/*.py) evaluated in fp32
on the case table of tests/dist_edge_cases.py - every family at the extremes of its parameters. Follows make_dist_golden.py: the
reference's classes, fp32, -inf outside the family's support (the convention of the device kernels, where torch would raise or
return something finite), validate_args off. Runs only where the reference tree exists (default /root/reference; --reference
PATH); the tests read the .npz alone.

Per case name N (dist_edge_cases.dist_edge_cases()) the file holds N/params, N/x (the inputs, fp32: the staleness check of the
tests) and N/lp (the reference's fp32 log_prob per value; NaN at x = NaN, whatever the class returns elsewhere inside the
support - NaN and +inf included: tests/test_dist_edges_host.py measures them).
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import dist_edge_cases as E  # noqa: E402


def reference_dist(R, family, p):
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)  # noqa: E731
    if family == 'Normal':
        return R.Normal(f32(p[0]), f32(p[1]))
    if family == 'Uniform':
        return R.Uniform(f32(p[0]), f32(p[1]))
    if family == 'Poisson':
        return R.Poisson(f32(p[0]))
    if family == 'Bernoulli':
        return R.Bernoulli(probs=f32(p[0]))
    if family == 'Categorical':
        return R.Categorical(probs=torch.from_numpy(np.array(p, np.float32)))
    if family == 'Exponential':
        return R.Exponential(f32(p[0]))
    if family == 'Gamma':
        return R.Gamma(f32(p[0]), f32(p[1]))
    if family == 'Beta':
        return R.Beta(f32(p[0]), f32(p[1]), low=f32(p[2]), high=f32(p[3]))
    if family == 'LogNormal':
        return R.LogNormal(f32(p[0]), f32(p[1]))
    if family == 'Weibull':
        return R.Weibull(f32(p[0]), f32(p[1]))
    if family == 'Binomial':
        return R.Binomial(total_count=f32(p[0]), logits=f32(p[1]))
    if family == 'VonMises':
        return R.VonMises(f32(p[0]), f32(p[1]))
    return R.TruncatedNormal(f32(p[0]), f32(p[1]), f32(p[2]), f32(p[3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, args.reference)
    import pyprob.distributions as R
    torch.distributions.Distribution.set_default_validate_args(False)
    out = {}
    for name, case in E.dist_edge_cases().items():
        d = reference_dist(R, case['family'], case['params'])
        lp = np.empty(len(case['x']), np.float32)
        for i, (x, tag) in enumerate(zip(case['x'], case['tags'])):
            if tag == 'out':
                lp[i] = -np.inf
            elif tag == 'nan':
                lp[i] = np.nan
            else:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    v = d.log_prob(torch.tensor(float(x), dtype=torch.float32))
                assert v.dtype == torch.float32 and v.numel() == 1, (name, v)
                lp[i] = float(v)
        out[name + '/params'] = case['params']
        out[name + '/x'] = case['x']
        out[name + '/lp'] = lp
    path = os.path.join(HERE, 'dist_edges.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out) // 3, 'cases')


if __name__ == '__main__':
    main()
