"""Wall time of Model.posterior_results_batch on an IMAGE program: M observed 28 x 28 images x N particles of the two-statement
renderer
    x ~ Uniform(6, 22); a ~ Normal(1, 0.1); observe img ~ Normal(a exp(-((xx - x)^2 + (yy - 14)^2) / 8), 0.1)
on an H = 512 LSTM network with a CNN2D5C observe embedding, trained for a few steps. The call is timed with a host clock between
device synchronisations; medians (and min - max) of --reps calls after warm-up. The comparator is THE SAME CALL on the parent
commit, where an image observe sends the call to the loop of M posterior_results calls: run this script there with --series-only
and hand its output to the run on this tree with --parent. `route` says what the call did ('one execution' or 'loop').
Also timed alone, with device events: the grouped likelihood launch (pp_obs_logweight_groups, x [M, 784] per group, mean
[M N, 784] per particle) with its achieved bytes/s from the M N k 4 bytes it has to read.
Writes one JSON document to profiles/is_batch_image_bench.json (--out PATH for another place).

    python tools/is_batch_image_bench.py --series-only --out parent_series.json        # in a checkout of the parent
    python tools/is_batch_image_bench.py --parent parent_series.json [--reps 20] [--M 1 16 256] [--N 1000 10000]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import ObserveEmbedding  # noqa: E402
from pyprob_amd.distributions import Normal, Uniform  # noqa: E402
from pyprob_amd.model import Model  # noqa: E402
from pyprob_amd.state import InferenceNetwork  # noqa: E402

SIDE = 28
K = SIDE * SIDE


class Renderer(Model):
    runs = 0

    def __init__(self):
        super().__init__('renderer 28 x 28')
        self.yy, self.xx = torch.meshgrid(torch.arange(float(SIDE)), torch.arange(float(SIDE)), indexing='ij')
        self.grids = {}

    def forward(self):
        type(self).runs += 1
        x = pyprob_amd.sample(Uniform(6, 22))
        a = pyprob_amd.sample(Normal(1, 0.1))
        if x.device not in self.grids:
            self.grids[x.device] = (self.xx.to(x.device), self.yy.to(x.device))
        gx, gy = self.grids[x.device]
        mean = a.reshape(-1, 1, 1) * torch.exp(-((gx - x.reshape(-1, 1, 1)) ** 2 + (gy - 14.0) ** 2) / 8.0)
        pyprob_amd.observe(Normal(mean, 0.1), name='img')
        return x


def series(model, args):
    rng = np.random.default_rng(7)
    yy, xx = np.meshgrid(np.arange(float(SIDE)), np.arange(float(SIDE)), indexing='ij')
    records = []
    for M in args.M:
        xs, gains = rng.uniform(8.0, 20.0, M), rng.normal(1.0, 0.1, M)
        images = np.stack([g * np.exp(-((xx - x) ** 2 + (yy - 14.0) ** 2) / 8.0) for x, g in zip(xs, gains)])
        images = torch.from_numpy((images + 0.1 * rng.standard_normal(images.shape)).astype(np.float32))
        for N in args.N:
            def call(seed):
                posts = model.posterior_results_batch(N, {'img': images}, seed=seed)
                return posts[-1].effective_sample_size          # (the caller looks at the result)

            def timed(seed):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(seed)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for w in range(args.warmup):
                call(w)
            before = Renderer.runs
            ts = [timed(100 + r) for r in range(args.reps)]
            per_call = (Renderer.runs - before) / args.reps
            rec = dict(M=M, N=N, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                       forward_runs_per_call=per_call, batch_ok=getattr(model, '_batch_ok', None),
                       route='one execution' if getattr(model, '_batch_ok', None) is True else 'loop')
            records.append(rec)
            print(json.dumps(rec), flush=True)
    return records


def likelihood_alone(args):
    """The grouped likelihood launch alone, event-timed: None where the tree has no such operator."""
    from pyprob_amd.ops import ops
    if not hasattr(ops, 'obs_logweight_groups'):
        return None
    out = []
    sd = torch.tensor([0.1], device='cuda')
    for M in args.M:
        for N in args.N:
            n = M * N
            mean = torch.rand(n, K, device='cuda')
            x = torch.rand(M, K, device='cuda')
            lw = torch.zeros(n, device='cuda')
            for _ in range(3):
                ops.obs_logweight_groups(lw, 0, [mean, sd, None, None], x, 16, K, 1.0, None, M, N)
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.obs_logweight_groups(lw, 0, [mean, sd, None, None], x, 16, K, 1.0, None, M, N)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            us = statistics.median(ts)
            rec = dict(M=M, N=N, k=K, median_us=round(us, 2), min_us=round(min(ts), 2), max_us=round(max(ts), 2),
                       bytes=n * K * 4, achieved_GB_per_s=round(n * K * 4 / us * 1e-3, 1))
            out.append(rec)
            print(json.dumps(rec), flush=True)
            del mean, x, lw
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--M', type=int, nargs='+', default=[1, 16, 256])
    ap.add_argument('--N', type=int, nargs='+', default=[1000, 10000])
    ap.add_argument('--train-traces', type=int, default=1024)
    ap.add_argument('--series-only', action='store_true', help='time the call and write the series alone (the run on the parent commit)')
    ap.add_argument('--parent', default=None, help='the series a --series-only run on the parent commit wrote')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'is_batch_image_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('is_batch_image_bench: needs a ROCm device (nothing is measured without one)')
    model = Renderer()
    torch.manual_seed(123)
    with contextlib.redirect_stdout(io.StringIO()):
        model.learn_inference_network(num_traces=args.train_traces, inference_network=InferenceNetwork.LSTM, batch_size=256, lstm_dim=512,
                                      observe_embeddings={'img': {'dim': 32, 'reshape': [1, SIDE, SIDE], 'embedding': ObserveEmbedding.CNN2D5C}},
                                      seed=1)
    records = series(model, args)
    doc = dict(device=torch.cuda.get_device_name(0), lstm_dim=512, image=[1, SIDE, SIDE], reps=args.reps, warmup=args.warmup,
               program='x ~ Uniform(6, 22); a ~ Normal(1, 0.1); img ~ Normal(a blob(x), 0.1) on 28 x 28',
               timing='host clock between device synchronisations around Model.posterior_results_batch(N, {img: tensor [M, 28, 28]}); '
                      'median, min and max of `reps` calls after `warmup` calls',
               records=records)
    if not args.series_only:
        doc['likelihood_launch_alone'] = likelihood_alone(args)
        doc['likelihood_timing'] = 'device events around one pp_obs_logweight_groups launch; achieved bytes/s = M N k 4 / median'
        if args.parent:
            parent = json.load(open(args.parent))
            doc['parent_records'] = parent['records']
            doc['comparison'] = []
            by = {(r['M'], r['N']): r for r in parent['records']}
            for r in records:
                p = by.get((r['M'], r['N']))
                if p is None:
                    continue
                doc['comparison'].append(dict(M=r['M'], N=r['N'], new_median_ms=r['median_ms'], parent_median_ms=p['median_ms'],
                                              parent_min_ms=p['min_ms'], parent_over_new=round(p['median_ms'] / r['median_ms'], 3),
                                              new_median_below_parent_fastest=r['median_ms'] < p['min_ms']))
            doc['acceptance'] = ('at M = 16 and M = 256 the new median lies below the fastest of the parent\'s timings: %s'
                                 % all(c['new_median_below_parent_fastest'] for c in doc['comparison'] if c['M'] in (16, 256)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
