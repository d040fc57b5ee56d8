"""Record tests/golden/vec_lp.npz: for each of the 12 scalar families of pp_obs_logweight (kinds 0, 1, 3, 4, 6-13) n = 5 rows of
k = 67 parameter values and observed values, all inside the family's support, and the float32 sum over a row of the
reference's own log_prob (pyprob/distributions/<family>.py) - what trace.py:123-125 adds to a trace's log-weight for a
vector-valued observe. Runs only where the reference tree exists (default /root/reference; --reference PATH); the tests read
the .npz alone.

Per kind K the file holds kK_p [4, n, k] (the parameters in pp_dist order p0..p3, unused slots zero; Binomial: p1 = the
logits torch derives from the probs), kK_x [n, k] and kK_lp [n].
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
N, K = 5, 67
KINDS = (0, 1, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13)


def inputs(kind, rng):
    """(constructor parameters in pp_dist order, x), float32 [N, K] each."""
    u = lambda a, b: rng.uniform(a, b, (N, K)).astype(np.float32)  # noqa: E731
    if kind == 0:
        m, s = u(-2, 2), u(0.3, 2)
        return [m, s], (m + s * rng.standard_normal((N, K))).astype(np.float32)
    if kind == 1:
        lo = u(-2, 0)
        hi = lo + u(0.5, 3)
        return [lo, hi], lo + (hi - lo) * u(0.05, 0.95)
    if kind == 3:
        r = u(0.5, 6)
        return [r], rng.poisson(r).astype(np.float32)
    if kind == 4:
        return [u(0.1, 0.9)], (rng.uniform(size=(N, K)) < 0.5).astype(np.float32)
    if kind == 6:
        return [u(0.5, 3)], u(0.05, 3)
    if kind == 7:
        return [u(0.5, 4), u(0.5, 3)], u(0.05, 4)
    if kind == 8:
        lo = u(-2, 0)
        hi = lo + u(1, 3)
        return [u(0.5, 4), u(0.5, 4), lo, hi], lo + (hi - lo) * u(0.05, 0.95)
    if kind == 9:
        return [u(-1, 1), u(0.3, 1.5)], u(0.1, 4)
    if kind == 10:
        return [u(0.5, 2), u(0.5, 3)], u(0.1, 3)
    if kind == 11:
        n = rng.randint(1, 21, (N, K)).astype(np.float32)
        return [n, u(0.1, 0.9)], np.floor(rng.uniform(size=(N, K)) * (n + 1)).clip(0, n).astype(np.float32)
    if kind == 12:
        return [u(-3, 3), u(0.2, 8)], u(-3.1, 3.1)
    lo, hi = -2 + u(0, 0.5), 2 + u(0, 0.5)
    return [u(-1, 1), u(0.5, 2), lo, hi], lo + (hi - lo) * u(0.02, 0.98)


def reference_object(R, kind, p):
    t = [torch.from_numpy(np.ascontiguousarray(q)) for q in p]
    if kind == 0:
        return R.Normal(t[0], t[1])
    if kind == 1:
        return R.Uniform(t[0], t[1])
    if kind == 3:
        return R.Poisson(t[0])
    if kind == 4:
        return R.Bernoulli(t[0])
    if kind == 6:
        return R.Exponential(t[0])
    if kind == 7:
        return R.Gamma(t[0], t[1])
    if kind == 8:
        return R.Beta(t[0], t[1], low=t[2], high=t[3])
    if kind == 9:
        return R.LogNormal(t[0], t[1])
    if kind == 10:
        return R.Weibull(t[0], t[1])
    if kind == 11:
        return R.Binomial(total_count=t[0], probs=t[1])
    if kind == 12:
        return R.VonMises(t[0], t[1])
    return R.TruncatedNormal(t[0], t[1], t[2], t[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, args.reference)
    import pyprob.distributions as R
    torch.distributions.Distribution.set_default_validate_args(False)
    rng = np.random.RandomState(20)
    out = {}
    for kind in KINDS:
        p, x = inputs(kind, rng)
        d = reference_object(R, kind, p)
        lp = d.log_prob(torch.from_numpy(x))
        assert lp.shape == (N, K) and lp.dtype == torch.float32 and bool(torch.isfinite(lp).all()), (kind, lp.shape)
        if kind == 11:
            p = [p[0], d.logits.numpy().astype(np.float32)]
        full = np.zeros((4, N, K), np.float32)
        for q, v in enumerate(p):
            full[q] = v
        out['k%d_p' % kind], out['k%d_x' % kind], out['k%d_lp' % kind] = full, x.astype(np.float32), lp.sum(-1).numpy()
    path = os.path.join(HERE, 'vec_lp.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
