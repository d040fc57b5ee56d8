"""Record tests/golden/mixture_lp.npz: the reference's Mixture (pyprob/distributions/mixture.py) evaluated in fp32 - log_prob on
a grid of values, mean and stddev - for the cases the Mixture tests read. Runs only where the reference tree exists (default
/root/reference; --reference PATH); the tests read the .npz alone.

`cases` lists the case names. Per case C the file holds
    C_names  [K]        the components' family names          C_suffix  the address suffix of the reference object
    C_params [K, 4, B]  constructor parameters in pp_dist order p0..p3 (B = 1: scalar components)
    C_probs  [K] or [B, K], as given to the constructor (not normalised)
    C_x      [V] (1-D probs: V values scored one at a time, as the reference's log_prob takes them) or [V, B]
    C_lp     like C_x    C_mean, C_stddev  [] or [B]
A component's log_prob is -inf where x lies outside its support - the convention of the device kernels and of
make_dist_golden.py, where torch (argument validation off) returns NaN or a finite number: the reference's components are
wrapped to say so before its own Mixture.log_prob combines them.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

# name -> (components [(family, p0..)], probs, values). A parameter is a float or a list (one per batch element).
CASES = {
    # the reference's own two test mixtures (tests/test_distributions.py:2096-2139)
    'ref1d': ([('Normal', 0, 0.1), ('Normal', 2, 0.1), ('Normal', 3, 0.1)], [0.7, 0.2, 0.1], [0.7, 0.0, 1.9, 3.2, -4.0, 40.0]),
    'ref2d': ([('Normal', [0, 1], [0.1, 1]), ('Normal', [2, 5], [0.1, 1]), ('Normal', [3, 10], [0.1, 1])],
              [[0.7, 0.2, 0.1], [0.1, 0.2, 0.7]], [[0.7, 8.1], [0.0, 1.0], [2.1, 5.5], [3.0, 12.0], [-30.0, 60.0]]),
    # families differ; x inside and outside each support (Uniform [1, 3), Gamma / Exponential x >= 0)
    'hetero': ([('Normal', -1.0, 0.5), ('Uniform', 1.0, 3.0), ('Gamma', 2.5, 0.5), ('Exponential', 2.0)], [0.1, 0.4, 0.3, 0.2],
               [-2.0, -1.0, -1e-3, 0.0, 0.5, 1.0, 2.0, 2.999, 3.0, 7.5, 40.0]),
    # every component's support missed: Uniform [0, 1) and Exponential
    'nosupport': ([('Uniform', 0.0, 1.0), ('Exponential', 1.0)], [0.5, 0.5], [-1.0, -0.5, 0.25, 2.0]),
    'k1': ([('Gamma', 2.0, 3.0)], [1.0], [-1.0, 0.0, 0.4, 2.0]),
    'k16': ([('Normal', float(k) - 8.0, 0.25 + 0.05 * k) for k in range(16)], [1.0 + (k % 4) for k in range(16)],
            [-9.0, -7.9, -3.3, 0.0, 0.5, 4.2, 7.0, 12.0]),
    'unnormalised': ([('Normal', 0.0, 1.0), ('LogNormal', 0.5, 0.8), ('Weibull', 2.0, 1.5)], [3.0, 5.0, 12.0], [-1.0, 0.0, 0.3, 1.0, 4.0]),
    # a zero weight is clamped to eps = 2^-23: the Normal still answers where the Exponential is out of its support
    'zero': ([('Normal', 0.0, 1.0), ('Exponential', 1.0), ('Normal', 4.0, 0.5)], [0.0, 0.6, 0.4], [-3.0, -1.0, 0.0, 1.0, 4.0]),
    'hetero2d': ([('Normal', [0.0, 1.0, -2.0], 0.5), ('TruncatedNormal', 1.0, [1.0, 2.0, 0.5], -1.0, 3.0), ('Beta', 2.0, 3.0, 0.0, [1.0, 2.0, 4.0])],
                 [[0.2, 0.3, 0.5], [1.0, 1.0, 2.0], [0.0, 0.5, 0.5]], [[0.5, 0.5, 0.5], [-2.0, 1.5, 3.5], [2.0, -0.5, 0.0]]),
}


def in_support(name, p, x):
    if name in ('Gamma', 'Exponential'):
        return x >= 0
    if name in ('LogNormal', 'Weibull'):
        return x > 0
    if name == 'TruncatedNormal':
        return (x >= p[2]) & (x <= p[3])
    if name == 'Beta':
        y = (x - p[2]) / (p[3] - p[2])
        return (y >= 0) & (y <= 1)
    return torch.ones_like(x, dtype=torch.bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, args.reference)
    import pyprob.distributions as R
    torch.distributions.Distribution.set_default_validate_args(False)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731

    def guarded(d, name, p):
        orig = d.log_prob

        def log_prob(value, sum=False):
            value = torch.as_tensor(value, dtype=torch.float32)
            ok = in_support(name, p, value)
            lp = orig(value)
            return torch.where(ok, lp, torch.full_like(lp, float('-inf')))
        d.log_prob = log_prob
        return d

    out = {'cases': np.asarray(list(CASES))}
    for case, (comps, probs, xs) in CASES.items():
        B = max([len(v) for c in comps for v in c[1:] if isinstance(v, list)] + [1])
        dists, params = [], np.zeros((len(comps), 4, B), np.float32)
        for k, c in enumerate(comps):
            name, p = c[0], [f32(v) for v in c[1:]]
            for q, v in enumerate(p):
                params[k, q, :] = v.numpy()
            if name == 'Beta':
                d = R.Beta(p[0], p[1], low=p[2], high=p[3])
            else:
                d = getattr(R, name)(*p)
            dists.append(guarded(d, name, p))
        mix = R.Mixture(dists, probs=f32(probs))
        x = f32(xs)
        lp = torch.stack([mix.log_prob(v) for v in x])
        assert lp.shape == x.shape, (case, lp.shape, x.shape)
        out[case + '_names'] = np.asarray([c[0] for c in comps])
        out[case + '_suffix'] = np.asarray(mix._address_suffix)
        out[case + '_params'] = params
        out[case + '_probs'] = np.asarray(probs, np.float32)
        out[case + '_x'] = x.numpy()
        out[case + '_lp'] = lp.numpy().astype(np.float32)
        out[case + '_mean'] = mix.mean.numpy().astype(np.float32)
        out[case + '_stddev'] = mix.stddev.numpy().astype(np.float32)
        print(case, out[case + '_lp'].tolist())
    path = os.path.join(HERE, 'mixture_lp.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
