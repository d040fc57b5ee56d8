"""Device time of the Mixture kernels (pp_mix_logweight, pp_mix_draw; 10^6 rows, hipEvent-timed like the sampler table of
tools/prior_is_bench.py), of the only other device route to the same log-density - K pp_dist_logweight launches with lp_out, then
torch.logsumexp - and the wall time of a lock-step prior-IS call of a Gaussian mixture model at 10^6 particles. Writes one JSON
line to profiles/mixture_bench.json (--out PATH for another place).

    python tools/mixture_bench.py [--reps 20]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import distributions as D  # noqa: E402
from pyprob_amd.model import Model  # noqa: E402
from pyprob_amd.state import InferenceEngine  # noqa: E402

N = 10 ** 6
DEV = 'cuda:0'


class MirroredGMM(Model):
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(0.0, 2.0))
        pyprob_amd.observe(D.Mixture([D.Normal(mu, 0.5), D.Normal(-mu, 0.5)], probs=[0.3, 0.7]), name='y')
        return mu


def event_ms(fn, reps):
    fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for r in range(reps):
        e0.record()
        fn(r + 1)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 4)


def case(kinds, params, probs):
    """Operator arguments of a mixture with shared parameters: params[k] = the component's parameters."""
    ps, ss = [], []
    for p in params:
        ps += [torch.tensor([float(v)], device=DEV) for v in p] + [None] * (4 - len(p))
        ss += [0, 0, 0, 0]
    return list(kinds), ps, ss, torch.tensor(probs, dtype=torch.float32, device=DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mixture_bench.json'))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from pyprob_amd.ops import ops
    rec = {'device': torch.cuda.get_device_name(0), 'rows': N}
    cases = {'normal_k3': case([0, 0, 0], [(0.0, 0.1), (2.0, 0.1), (3.0, 0.5)], [0.7, 0.2, 0.1]),
             'hetero_k3': case([0, 6, 1], [(-50.0, 0.1), (1.0,), (100.0, 101.0)], [0.25, 0.5, 0.25])}
    x = torch.rand(N, device=DEV) * 4
    lw = torch.zeros(N, device=DEV)
    out = torch.empty(N, device=DEV)
    lps = torch.empty(3, N, device=DEV)
    for name, (kinds, ps, ss, probs) in cases.items():
        rec['mix_logweight_ms_' + name] = event_ms(
            lambda r: ops.mix_logweight(lw, kinds, ps, ss, probs, x, 1.0, None, None, N), a.reps)
        rec['mix_draw_ms_' + name] = event_ms(lambda r: ops.mix_draw(kinds, ps, ss, probs, None, out, r, 0, 1), a.reps)
        logq = torch.log(probs / probs.sum()).reshape(3, 1)

        def k_launches(r):      # the route without the mixture kernel: one log-density launch per component, then torch
            for k in range(3):
                ops.dist_logweight(None, [kinds[k]], ps[4 * k:4 * k + 4], ss[4 * k:4 * k + 4], [x], [1.0], None, lps[k], N)
            lw.add_(torch.logsumexp(lps + logq, 0))
        rec['k_dist_logweight_plus_logsumexp_ms_' + name] = event_ms(k_launches, a.reps)
    model = MirroredGMM()
    model.posterior_results(N, InferenceEngine.IMPORTANCE_SAMPLING, observe={'y': 1.5}, lock_step=True, seed=0)
    torch.cuda.synchronize()
    ts = []
    for r in range(a.reps):
        t0 = time.perf_counter()
        model.posterior_results(N, InferenceEngine.IMPORTANCE_SAMPLING, observe={'y': 1.5}, lock_step=True, seed=r + 1)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    rec['gmm_prior_is_1e6_ms'] = round(statistics.median(ts) * 1e3, 4)
    rec['gmm_prior_is_particles_per_sec'] = round(N / (statistics.median(ts)), 1)
    assert all(math.isfinite(v) for v in rec.values() if isinstance(v, float))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
