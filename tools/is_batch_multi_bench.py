"""Wall time of Model.posterior_results_batch on a MULTI-STATEMENT straight-line program against the loop it replaces: M
observations x N particles of
    a ~ Normal(1, sqrt 5); observe obs0 ~ Normal(a, sqrt 2); b ~ Normal(a, 0.7); observe obs1 ~ Normal(b, sqrt 2)
on an H = 512 network trained for a few steps. The batched call is one lock-step execution of forward() for all M N particles
(pp_is_batch_first + pp_is_fused_groups for `a`, pp_is_batch_bias + pp_is_statement_groups for `b`); the loop is M
Model.posterior_results calls on the same observations - what the batched call was for this program before later statements
were served. Both are timed with a host clock between device synchronisations, alternating inside every repetition; medians of
--reps repetitions after warm-up. Writes one JSON document to profiles/is_batch_multi_bench.json (--out PATH for another place).

    python tools/is_batch_multi_bench.py [--reps 20] [--M 1 16 256] [--N 1000 10000]"""
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


class TwoStatements(Model):
    def __init__(self):
        super().__init__('two-statement straight line')

    def forward(self):
        a = pyprob_amd.sample(Normal(1.0, math.sqrt(5.0)))
        pyprob_amd.observe(Normal(a, math.sqrt(2.0)), name='obs0')
        b = pyprob_amd.sample(Normal(a, 0.7))
        pyprob_amd.observe(Normal(b, math.sqrt(2.0)), name='obs1')
        return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--M', type=int, nargs='+', default=[1, 16, 256])
    ap.add_argument('--N', type=int, nargs='+', default=[1000, 10000])
    ap.add_argument('--train-traces', type=int, default=4 * 1024)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'is_batch_multi_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('is_batch_multi_bench: needs a ROCm device (nothing is measured without one)')
    model = TwoStatements()
    torch.manual_seed(123)
    with contextlib.redirect_stdout(io.StringIO()):
        model.learn_inference_network(num_traces=args.train_traces, inference_network=InferenceNetwork.LSTM,
                                      observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, batch_size=1024, lstm_dim=512, seed=1)
    rng = np.random.default_rng(7)
    records = []
    for M in args.M:
        obs = rng.uniform(-2.0, 4.0, (M, 2)).astype(np.float32)
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
    doc = dict(device=torch.cuda.get_device_name(0), lstm_dim=512, program='a ~ Normal; obs0 ~ Normal(a, .); b ~ Normal(a, 0.7); obs1 ~ Normal(b, .)', reps=args.reps, warmup=args.warmup,
               timing='host clock between device synchronisations, batched and loop alternating in every repetition, medians',
               batched='Model.posterior_results_batch(N, {name: tensor [M]}): forward() runs in every call',
               loop='M x Model.posterior_results(N, ..., lock_step=True, offset=g N): one lock-step execution of forward() per observation',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
