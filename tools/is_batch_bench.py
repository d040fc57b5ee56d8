"""Wall time of Model.posterior_results_batch against the loop it replaces: M observations x N particles of the GaussianUnknownMean
program on the H = 512 benchmark network (BASELINE.json configs[3]), the batched call (one lock-step execution of forward() for
all M N particles: pp_is_batch_first + pp_is_fused_groups) next to M plan-cached Model.posterior_results calls on the same
observations (pp_is_first_statement + pp_is_fused each - code this feature does not touch). Both are timed with a host clock
between device synchronisations, alternating inside every repetition; medians of --reps repetitions after warm-up. Writes one
JSON document to profiles/is_batch_bench.json (--out PATH for another place).

    python tools/is_batch_bench.py [--reps 20] [--M 1 16 256 4096] [--N 256 1000 10000]"""
import argparse
import contextlib
import io
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd.distributions import Normal  # noqa: E402
from pyprob_amd.model import Model  # noqa: E402
from pyprob_amd.state import InferenceEngine, InferenceNetwork  # noqa: E402

IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK


class GaussianWithUnknownMean(Model):
    def __init__(self):
        self.prior_mean, self.prior_stddev, self.likelihood_stddev = 1, math.sqrt(5), math.sqrt(2)
        super().__init__('Gaussian with unknown mean')

    def forward(self):
        mu = pyprob_amd.sample(Normal(self.prior_mean, self.prior_stddev))
        likelihood = Normal(mu, self.likelihood_stddev)
        pyprob_amd.observe(likelihood, name='obs0')
        pyprob_amd.observe(likelihood, name='obs1')
        return mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--M', type=int, nargs='+', default=[1, 16, 256, 4096])
    ap.add_argument('--N', type=int, nargs='+', default=[256, 1000, 10000])
    ap.add_argument('--train-traces', type=int, default=16 * 1024)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'is_batch_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('is_batch_bench: needs a ROCm device (nothing is measured without one)')
    model = GaussianWithUnknownMean()
    torch.manual_seed(123)
    with contextlib.redirect_stdout(io.StringIO()):
        model.learn_inference_network(num_traces=args.train_traces, inference_network=InferenceNetwork.LSTM,
                                      observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, batch_size=1024, lstm_dim=512, seed=1)
    rng = np.random.default_rng(7)
    records = []
    for M in args.M:
        obs = rng.uniform(5.0, 11.0, (M, 2)).astype(np.float32)
        as_list = [{'obs0': float(a), 'obs1': float(b)} for a, b in obs]
        as_dict = {'obs0': torch.from_numpy(obs[:, 0].copy()), 'obs1': torch.from_numpy(obs[:, 1].copy())}
        for N in args.N:
            def batched(seed):
                posts = model.posterior_results_batch(N, as_dict, seed=seed)
                return posts[-1].effective_sample_size

            def loop(seed):
                ess = 0.0
                for g in range(M):
                    post = model.posterior_results(N, IC, observe=as_list[g], lock_step=True, seed=seed, offset=g * N)
                    ess = post.effective_sample_size          # (the caller looks at every result, as bench.py's loop does)
                return ess

            def timed(fn, seed):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(seed)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for w in range(args.warmup):
                batched(w), loop(w)
            assert model._batch_ok is True
            last = model.posterior_results(N, IC, observe=as_list[-1], lock_step=True, seed=0, offset=(M - 1) * N)
            assert getattr(last, 'replayed_plan', False), 'the loop is meant to run on the launch plan'
            tb, tl = [], []
            for r in range(args.reps):
                tb.append(timed(batched, 100 + r))
                tl.append(timed(loop, 100 + r))
            b, l = statistics.median(tb), statistics.median(tl)
            rec = dict(M=M, N=N, batched_ms=round(b, 4), loop_ms=round(l, 4), loop_over_batched=round(l / b, 3),
                       batched_min_ms=round(min(tb), 4), batched_max_ms=round(max(tb), 4), loop_min_ms=round(min(tl), 4),
                       loop_max_ms=round(max(tl), 4), batched_faster_in_every_pair=all(x < y for x, y in zip(tb, tl)),
                       batched_posteriors_per_s=round(M / b * 1e3, 1), loop_posteriors_per_s=round(M / l * 1e3, 1),
                       batched_particles_per_s=round(M * N / b * 1e3, 1), loop_particles_per_s=round(M * N / l * 1e3, 1))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), lstm_dim=512, program='GaussianWithUnknownMean', reps=args.reps, warmup=args.warmup,
               timing='host clock between device synchronisations, batched and loop alternating in every repetition, medians',
               batched='Model.posterior_results_batch(N, {name: tensor [M]}): forward() runs in every call',
               loop='M x Model.posterior_results(N, ..., lock_step=True, offset=g N) on the launch plan (forward() is not run)',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
