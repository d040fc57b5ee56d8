"""Time of Empirical.reobserve / pyprob_amd.reobserve_batch against what they replace: M new observations for the N particles of
one posterior, for two programs on H = 512 networks - GaussianUnknownMean (BASELINE.json configs[3]: two scalar Normal observes)
and the two-statement 28 x 28 renderer of tools/is_batch_image_bench.py (one image observe, k = 784).

    reobserve        post.reobserve(observe=...) (M = 1) / reobserve_batch(post, observes): one replay of forward() over the
                     statement log, the accumulate route for `old`, ONE pp_is_reobserve_groups call, the statistics
    posterior        Model.posterior_results (M = 1) / Model.posterior_results_batch on the same observations: the network runs
                     for all M N rows. Timed on THIS tree and, with --parent, on a checkout of the parent commit
    torch_broadcast  the same log-density as torch broadcasts on the device (the image program: one broadcast per group)
    operator         pp_is_reobserve_groups alone, with the bytes it must move and its log-density evaluations, computed from
                     the shapes; for the scalar program also with PP_REOBS_PLAIN=1 (the general kernel instead of the k = 1 one)

Device events around each call, medians of --reps after --warmup, written to profiles/reobserve_bench.json (--out PATH).

    python tools/reobserve_bench.py --tree PARENT_CHECKOUT --posterior-only --out parent.json      # the parent's posterior calls
    python tools/reobserve_bench.py --parent parent.json --bench-ab PARENT_CHECKOUT                # everything, into --out

--tree PATH imports pyprob_amd from another checkout (its library built there); --posterior-only times the `posterior` column
alone, which is all a tree without the feature can run. --bench-ab PATH runs `bench.py --workload is` in PATH and in this tree,
--ab-rounds rounds of one fresh process each, the first side alternating, and writes both series and their spread into the same document (`bench_is_ab`)."""
import argparse
import contextlib
import io
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = REPO
if '--tree' in sys.argv:
    TREE = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, TREE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import ObserveEmbedding  # noqa: E402
from pyprob_amd.distributions import Normal, Uniform  # noqa: E402
from pyprob_amd.model import Model  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402
from pyprob_amd.state import InferenceEngine, InferenceNetwork  # noqa: E402

IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
S2 = math.sqrt(2.0)
SIDE = 28
K = SIDE * SIDE


class GaussianWithUnknownMean(Model):
    def __init__(self):
        self.prior_mean, self.prior_stddev, self.likelihood_stddev = 1, math.sqrt(5), S2
        super().__init__('Gaussian with unknown mean')

    def forward(self):
        mu = pyprob_amd.sample(Normal(self.prior_mean, self.prior_stddev))
        likelihood = Normal(mu, self.likelihood_stddev)
        pyprob_amd.observe(likelihood, name='obs0')
        pyprob_amd.observe(likelihood, name='obs1')
        return mu


class Renderer(Model):
    """tools/is_batch_image_bench.py's program: x ~ Uniform(6, 22); a ~ Normal(1, 0.1); img ~ Normal(a blob(x), 0.1) on 28 x 28."""

    def __init__(self):
        super().__init__('renderer 28 x 28')
        self.yy, self.xx = torch.meshgrid(torch.arange(float(SIDE)), torch.arange(float(SIDE)), indexing='ij')
        self.grids = {}

    def mean(self, x, a):
        if x.device not in self.grids:
            self.grids[x.device] = (self.xx.to(x.device), self.yy.to(x.device))
        gx, gy = self.grids[x.device]
        return a.reshape(-1, 1, 1) * torch.exp(-((gx - x.reshape(-1, 1, 1)) ** 2 + (gy - 14.0) ** 2) / 8.0)

    def forward(self):
        x = pyprob_amd.sample(Uniform(6, 22))
        a = pyprob_amd.sample(Normal(1, 0.1))
        pyprob_amd.observe(Normal(self.mean(x, a), 0.1), name='img')
        return x


def timed(fn, reps, warmup):
    """Median, minimum and maximum milliseconds of fn() between two device events."""
    ts = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def gum_case(args):
    model = GaussianWithUnknownMean()
    torch.manual_seed(123)
    with contextlib.redirect_stdout(io.StringIO()):
        model.learn_inference_network(num_traces=16 * 1024, inference_network=InferenceNetwork.LSTM,
                                      observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, batch_size=1024, lstm_dim=512, seed=1)

    def observes(M, rng):
        obs = rng.uniform(5.0, 11.0, (M, 2)).astype(np.float32)
        return {'obs0': torch.from_numpy(obs[:, 0].copy()), 'obs1': torch.from_numpy(obs[:, 1].copy())}

    def first(N):
        for w in range(3):      # (the launch plan is recorded and verified)
            post = model.posterior_results(N, IC, observe={'obs0': 8.0 + 0.1 * w, 'obs1': 9.0}, lock_step=True, seed=w)
        return post

    def device_forms(post, obs, M, N):
        lw, mu = post._all_log_weights, post.statement_log[0][post.addresses[0]][0]
        sd = torch.tensor([S2], device=lw.device)
        x0, x1 = (obs[k].reshape(M, 1).to(lw.device) for k in ('obs0', 'obs1'))
        old = torch.zeros_like(lw)
        params = [mu.reshape(N, 1), sd, None, None] * 2

        def operator():
            return ops.reobserve_groups(lw, old, [0, 0], [1, 1], [1.0, 1.0], params, [x0, x1], M)

        def broadcast():
            m = mu[None, :]
            return lw[None, :] + ((Normal(m, S2).log_prob(x0) + Normal(m, S2).log_prob(x1)) - old[None, :])
        return operator, broadcast, 4 * (3 * N + M * N + 2 * M), 2 * M * N
    return dict(name='GaussianWithUnknownMean', model=model, observes=observes, first=first, device_forms=device_forms, plain=True,
                evals_per_row=2)


def image_case(args):
    model = Renderer()
    torch.manual_seed(123)
    with contextlib.redirect_stdout(io.StringIO()):
        model.learn_inference_network(num_traces=1024, inference_network=InferenceNetwork.LSTM, batch_size=256, lstm_dim=512,
                                      observe_embeddings={'img': {'dim': 32, 'reshape': [1, SIDE, SIDE], 'embedding': ObserveEmbedding.CNN2D5C}},
                                      seed=1)
    yy, xx = np.meshgrid(np.arange(float(SIDE)), np.arange(float(SIDE)), indexing='ij')

    def observes(M, rng):
        xs, gains = rng.uniform(8.0, 20.0, M), rng.normal(1.0, 0.1, M)
        images = np.stack([g * np.exp(-((xx - x) ** 2 + (yy - 14.0) ** 2) / 8.0) for x, g in zip(xs, gains)])
        return {'img': torch.from_numpy((images + 0.1 * rng.standard_normal(images.shape)).astype(np.float32))}

    def first(N):
        return model.posterior_results(N, IC, observe={'img': observes(1, np.random.default_rng(3))['img'][0]}, lock_step=True, seed=1)

    def device_forms(post, obs, M, N):
        lw = post._all_log_weights
        x, a = (post.statement_log[j][post.addresses[j]][0] for j in (0, 1))
        mean = model.mean(x, a).reshape(N, K).contiguous()
        sd = torch.tensor([0.1], device=lw.device)
        img = obs['img'].reshape(M, K).to(lw.device)
        old = torch.zeros_like(lw)

        def operator():
            return ops.reobserve_groups(lw, old, [0], [K], [1.0], [mean, sd, None, None], [img], M)

        def broadcast():
            return torch.stack([lw + (Normal(mean, 0.1).log_prob(img[g][None, :]).sum(1) - old) for g in range(M)])
        return operator, broadcast, 4 * (2 * N + N * K + M * K + M * N), M * N * K
    return dict(name='renderer 28 x 28 (two statements, one image observe)', model=model, observes=observes, first=first,
                device_forms=device_forms, plain=False, evals_per_row=K)


def run_case(case, args, records):
    model = case['model']
    rng = np.random.default_rng(7)
    for N in args.N:
        post = case['first'](N)
        for M in args.M:
            obs = case['observes'](M, rng)
            one = {k: v[0] for k, v in obs.items()}
            rec = dict(program=case['name'], N=N, M=M)
            if M * N * case['evals_per_row'] > args.max_evaluations:
                rec['skipped'] = 'more than %.0e log-density evaluations per call' % args.max_evaluations
                records.append(rec)
                print(json.dumps(rec), flush=True)
                continue

            def network():
                if M == 1:
                    return model.posterior_results(N, IC, observe=one, lock_step=True, seed=5).effective_sample_size
                return model.posterior_results_batch(N, obs, seed=5)[-1].effective_sample_size
            if M * N <= args.max_network_rows and M * N * case['evals_per_row'] <= args.max_network_elements:
                rec['posterior'] = timed(network, args.reps, args.warmup)
            if not args.posterior_only:
                def api():
                    if M == 1:
                        return post.reobserve(observe=one).effective_sample_size
                    return pyprob_amd.reobserve_batch(post, obs)[-1].effective_sample_size
                operator, broadcast, nbytes, evals = case['device_forms'](post, obs, M, N)
                rec.update(operator_bytes=nbytes, operator_log_densities=evals, reobserve=timed(api, args.reps, args.warmup),
                           operator=timed(operator, args.reps, args.warmup), torch_broadcast=timed(broadcast, args.reps, args.warmup))
                if case['plain']:
                    os.environ['PP_REOBS_PLAIN'] = '1'
                    rec['operator_general_kernel'] = timed(operator, args.reps, args.warmup)
                    del os.environ['PP_REOBS_PLAIN']
                    rec['general_over_k1'] = round(rec['operator_general_kernel']['median_ms'] / rec['operator']['median_ms'], 3)
                if 'posterior' in rec:
                    rec['posterior_over_reobserve'] = round(rec['posterior']['median_ms'] / rec['reobserve']['median_ms'], 3)
                rec['broadcast_over_operator'] = round(rec['torch_broadcast']['median_ms'] / rec['operator']['median_ms'], 3)
                rec['operator_gb_per_s'] = round(nbytes / rec['operator']['median_ms'] / 1e6, 1)
                rec['operator_g_evaluations_per_s'] = round(evals / rec['operator']['median_ms'] / 1e6, 1)
            records.append(rec)
            print(json.dumps(rec), flush=True)
        del post


def bench_ab(parent, rounds):
    """`bench.py --workload is` in the parent checkout and in this tree, alternating, each in a fresh process."""
    cmd = [sys.executable, 'bench.py', '--workload', 'is', '--gpus', '1', '--steps', '20', '--warmup', '3']
    series = {'parent': [], 'this': []}
    for r in range(rounds):      # (the side that goes first changes every round)
        for side, cwd in ((('parent', parent), ('this', REPO)) if r % 2 == 0 else (('this', REPO), ('parent', parent))):
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, check=True, timeout=300).stdout
            series[side].append(json.loads([line for line in out.splitlines() if line.startswith('{')][-1]))
    ms = {side: [r['ms_per_step'] for r in rs] for side, rs in series.items()}
    return dict(command=' '.join(cmd[1:]), order='%d rounds of one fresh process per side, the side that goes first alternating (parent first in round 1)' % rounds,
                parent_ms_per_call=ms['parent'], this_ms_per_call=ms['this'], parent_median_ms=statistics.median(ms['parent']),
                this_median_ms=statistics.median(ms['this']),
                spread_ms=round(max(max(v) - min(v) for v in ms.values()), 4),
                parent_particles_per_s=[r['value'] for r in series['parent']], this_particles_per_s=[r['value'] for r in series['this']])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--M', type=int, nargs='+', default=[1, 16, 256])
    ap.add_argument('--N', type=int, nargs='+', default=[10000, 1000000])
    ap.add_argument('--programs', nargs='+', default=['gum', 'image'], choices=['gum', 'image'])
    ap.add_argument('--max-network-rows', type=int, default=64 * 10 ** 6, help='the posterior calls are not timed above this many M N rows')
    ap.add_argument('--max-network-elements', type=float, default=4e9,
                    help='nor above this many M N k likelihood elements (the program materialises them: 4 bytes each, several times)')
    ap.add_argument('--max-evaluations', type=float, default=2e10, help='a cell with more log-density evaluations per call is skipped')
    ap.add_argument('--tree', default=None, help='import pyprob_amd from this checkout instead of the one the script lies in')
    ap.add_argument('--posterior-only', action='store_true', help='time the posterior calls alone (a tree without the feature)')
    ap.add_argument('--parent', default=None, help='the document a --posterior-only run on the parent commit wrote')
    ap.add_argument('--bench-ab', default=None, help='a checkout of the parent commit: alternate bench.py --workload is with this tree')
    ap.add_argument('--ab-rounds', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'reobserve_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('reobserve_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    for name in args.programs:
        run_case({'gum': gum_case, 'image': image_case}[name](args), args, records)
        torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), lstm_dim=512, reps=args.reps, warmup=args.warmup, tree=os.path.basename(TREE),
               timing='device events around each call, medians', records=records)
    if args.parent:
        parent = json.load(open(args.parent))
        by = {(r['program'], r['N'], r['M']): r for r in parent['records']}
        for r in records:
            p = by.get((r['program'], r['N'], r['M']))
            if p is not None and 'posterior' in p:
                r['posterior_parent'] = p['posterior']
                if 'reobserve' in r:
                    r['parent_posterior_over_reobserve'] = round(p['posterior']['median_ms'] / r['reobserve']['median_ms'], 3)
    if args.bench_ab:
        doc['bench_is_ab'] = bench_ab(os.path.abspath(args.bench_ab), args.ab_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
