"""Wall time per call of the prior-proposal engine in lock step (posterior_results(IMPORTANCE_SAMPLING, lock_step=True)) and of
the per-trace loop for contrast, plus device time per sampler launch (pp_dist_draw, 10^6 draws, hipEvent-timed). Writes one JSON
line to profiles/<tag>_prior_is_bench.json.

    python tools/prior_is_bench.py [--tag r07] [--reps 20]
For kernel names and times of the same launches run it once more under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import distributions as D  # noqa: E402
from pyprob_amd.model import Model  # noqa: E402
from pyprob_amd.state import InferenceEngine  # noqa: E402
from models import GaussianWithUnknownMean, GaussianWithUnknownMeanMarsagliaLockStep  # noqa: E402

IS = InferenceEngine.IMPORTANCE_SAMPLING


class GammaPoisson(Model):
    def forward(self):
        rate = pyprob_amd.sample(D.Gamma(3.0, 1.5))
        for i in range(4):
            pyprob_amd.observe(D.Poisson(rate), name='k%d' % i)
        return rate


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def kernel_ms(kind, params, reps):
    from pyprob_amd.ops import ops
    n = 10 ** 6
    ps = [torch.tensor([float(v)], device='cuda') for v in params] + [None] * (4 - len(params))
    ss = [0, 0, 0, 0]
    if kind == 5:
        ps = [torch.full((8,), 0.125, device='cuda'), None, None, None]
        ss = [0, 8, 0, 0]
    out = torch.empty(n, device='cuda')
    ops.dist_draw(kind, ps, ss, None, out, 1, 0, 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for r in range(reps):
        e0.record()
        ops.dist_draw(kind, ps, ss, None, out, r, 0, 1)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


SAMPLERS = {'Normal': (0, (0.0, 1.0)), 'Uniform': (1, (0.0, 1.0)), 'Poisson_4': (3, (4.0,)), 'Poisson_300': (3, (300.0,)),
            'Bernoulli': (4, (0.3,)), 'Categorical_8': (5, ()), 'Exponential': (6, (1.0,)), 'Gamma_0.3': (7, (0.3, 1.0)),
            'Gamma_5': (7, (5.0, 1.0)), 'Beta_0.5_1': (8, (0.5, 1.0, 0.0, 1.0)), 'LogNormal': (9, (0.0, 1.0)),
            'Weibull': (10, (1.0, 1.5)), 'Binomial_20_0.3': (11, (20.0, math.log(0.3 / 0.7))),
            'Binomial_1000_0.4': (11, (1000.0, math.log(0.4 / 0.6))), 'VonMises_2': (12, (0.0, 2.0)),
            'TruncatedNormal': (13, (0.0, 1.0, -1.0, 2.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tag', default='r07')
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gum, mars, gp = GaussianWithUnknownMean(), GaussianWithUnknownMeanMarsagliaLockStep(), GammaPoisson()
    obs = {'obs0': 8, 'obs1': 9}
    rec = {'device': torch.cuda.get_device_name(0)}
    rec['gum_1e6_ms'] = wall(lambda: gum.posterior_results(10 ** 6, IS, observe=obs, lock_step=True, seed=1), a.reps)
    rec['marsaglia_2e5_ms'] = wall(lambda: mars.posterior_results(200000, IS, observe=obs, lock_step=True, seed=1), a.reps)
    rec['gamma_poisson_1e6_ms'] = wall(lambda: gp.posterior_results(10 ** 6, IS, observe={'k0': 2, 'k1': 4, 'k2': 3, 'k3': 5},
                                                                    lock_step=True, seed=1), a.reps)
    t0 = time.perf_counter()
    gum.posterior_results(10 ** 4, IS, observe=obs)
    rec['gum_per_trace_1e4_ms'] = (time.perf_counter() - t0) * 1e3
    rec['gum_lockstep_particles_per_sec'] = 1e6 / (rec['gum_1e6_ms'] * 1e-3)
    rec['gum_per_trace_particles_per_sec'] = 1e4 / (rec['gum_per_trace_1e4_ms'] * 1e-3)
    rec['sampler_ms_1e6'] = {k: round(kernel_ms(kind, p, a.reps), 4) for k, (kind, p) in SAMPLERS.items()}
    for k, v in rec.items():
        if isinstance(v, float):
            rec[k] = round(v, 4)
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
    with open(os.path.join(REPO, 'profiles', '%s_prior_is_bench.json' % a.tag), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
