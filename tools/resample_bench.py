"""Wall time of Empirical.resample / sample and pyprob_amd.resample_batch on device-backed posteriors: the device route
(csrc/is_resample.hip) next to the host route the same objects take under PP_EMPIRICAL_DEVICE=0 (the code path of the commit before
the device route existed). GaussianUnknownMean on the H = 512 benchmark network; a posterior of N = 10^6 particles for resample(1000),
resample(N) and sample(); M = 256 posteriors of 10^4 particles for resample_batch(., 1000). Host clock between device
synchronisations, one block of --warmup + --reps calls per route (device first), medians. pp_is_cdf_groups
alone is timed with device events (20 launches per event pair) and reported with its bytes per second. Writes one JSON document to
profiles/resample_bench.json (--out PATH for another place).

    python tools/resample_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]
    python tools/resample_bench.py --package-root TREE --child       # resample(1000) of ANOTHER checkout's package (the parent commit),
                                                                     # one JSON line; the main run starts this when --parent-tree is given"""
import argparse
import contextlib
import gc
import io
import json
import math
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--train-traces', type=int, default=16 * 1024)
    ap.add_argument('--package-root', default=REPO, help='the checkout whose pyprob_amd package is measured')
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit (with its library built): resample(1000) is '
                    'measured there too, in a child process')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'resample_bench.json'))
    return ap.parse_args()


args = _args()
sys.path.insert(0, os.path.abspath(args.package_root))

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


def trained_model():
    model = GaussianWithUnknownMean()
    torch.manual_seed(123)
    with contextlib.redirect_stdout(io.StringIO()):
        model.learn_inference_network(num_traces=args.train_traces, inference_network=InferenceNetwork.LSTM,
                                      observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, batch_size=1024, lstm_dim=512, seed=1)
    return model


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


@contextlib.contextmanager
def host_route():
    os.environ['PP_EMPIRICAL_DEVICE'] = '0'
    try:
        yield
    finally:
        del os.environ['PP_EMPIRICAL_DEVICE']


def child():
    """resample(1000) on the posterior of N particles with whatever package --package-root holds."""
    model = trained_model()
    post = model.posterior_results(args.N, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=1)
    for _ in range(args.warmup):
        post.resample(1000)
    ts = [timed(lambda: post.resample(1000)) for _ in range(args.reps)]
    print(json.dumps(dict(case='resample(1000)', N=args.N, package_root=os.path.abspath(args.package_root),
                          has_device_route=hasattr(pyprob_amd.distributions.Empirical, '_device_backed'), **summary(ts))), flush=True)


def ab(name, fn, records, **extra):
    """fn on the device route, then on the host route: one block of warm-up + repetitions each, not interleaved - a host-route
    call leaves up to 10^6 Python objects behind whose collection would be billed to the device-route call after it (interleaved,
    resample(N) on the device measured 21 ms at the median against 0.8 ms at best)."""
    gc.collect()
    for _ in range(args.warmup):
        fn()
    td = [timed(fn) for _ in range(args.reps)]
    with host_route():
        for _ in range(args.warmup):
            fn()
        th = [timed(fn) for _ in range(args.reps)]
    gc.collect()
    d, h = summary(td), summary(th)
    rec = dict(case=name, device=d, host=h, host_over_device=round(h['median_ms'] / d['median_ms'], 2),
               slowest_device_below_fastest_host=max(td) < min(th), **extra)
    records.append(rec)
    print(json.dumps(rec), flush=True)


def cdf_alone(M, N, with_stats):
    """pp_is_cdf_groups through its operator, device events around 20 launches, median of --reps such windows."""
    from pyprob_amd import lib as L
    from pyprob_amd.ops import ops
    g = torch.Generator(device='cuda').manual_seed(5)
    lw = torch.randn(M * N, device='cuda', generator=g) * 3.0
    stats = None
    if with_stats:
        scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device='cuda')
        stats = torch.stack([ops.is_stats(lw[q * N:(q + 1) * N], None, scratch)[:6] for q in range(M)]).contiguous()
    for _ in range(args.warmup):
        ops.is_cdf_groups(lw, N, stats)
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            ops.is_cdf_groups(lw, N, stats)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 20)
    tiles = -(-N // L.PP_IS_CDF_TILE)
    # bytes the launches move per particle: the scan reads 4 and writes 8; groups of more than one tile read and write the 8 again
    # when the offsets are added, and read the 4 once more for the tile maxima when no statistics are given
    per = 12 + (16 if tiles > 1 else 0) + (4 if (tiles > 1 and not with_stats) else 0)
    ms = statistics.median(ts)
    return dict(case='is_cdf_groups', M=M, N=N, stats_given=with_stats, launches=(1 if tiles == 1 else (3 if with_stats else 4)),
                bytes_per_particle=per, **summary(ts), achieved_GB_per_s=round(M * N * per / (ms * 1e-3) / 1e9, 1),
                timing='device events around 20 calls of the operator (each allocates its output and workspace)')


def main():
    if not torch.cuda.is_available():
        raise SystemExit('resample_bench: needs a ROCm device (nothing is measured without one)')
    if args.child:
        return child()
    from pyprob_amd.distributions import Empirical
    model = trained_model()
    records = []
    N = args.N
    post = model.posterior_results(N, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=1)
    assert post._device_backed() and post.length == N
    extra = dict(N=N, ess=round(post.effective_sample_size, 1))
    ab('resample(1000)', lambda: post.resample(1000), records, **extra)
    ab('resample(N)', lambda: post.resample(N), records, **extra)
    ab('sample()', lambda: post.sample(), records, **extra)
    # the FIRST call on an object: the device route scans its cdf, the host route reads the log-weights back and normalises them
    def fresh():
        return Empirical.from_device(post._values, post._log_weights, post.device_stats)
    ab('resample(1000), first call on an object', lambda: fresh().resample(1000), records, **extra)
    ab('sample(), first call on an object', lambda: fresh().sample(), records, **extra)
    # a small posterior: where the host route is still competitive
    for n_small in (100, 1000, 10000):
        small = model.posterior_results(n_small, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=2)
        ab('sample()', lambda: small.sample(), records, N=n_small)
    M, Nb = args.batch
    rng = np.random.default_rng(7)
    obs = rng.uniform(5.0, 11.0, (M, 2)).astype(np.float32)
    posts = model.posterior_results_batch(Nb, {'obs0': torch.from_numpy(obs[:, 0].copy()), 'obs1': torch.from_numpy(obs[:, 1].copy())}, seed=3)
    assert model._batch_ok is True and posts[0].__dict__.get('_batch') is not None
    ab('resample_batch(posts, 1000)', lambda: pyprob_amd.resample_batch(posts, 1000), records, M=M, N=Nb)
    for (m, n) in ((1, N), (M, Nb)):
        for with_stats in (True, False):
            rec = cdf_alone(m, n, with_stats)
            records.append(rec)
            print(json.dumps(rec), flush=True)
    parent = None
    if args.parent_tree:
        # a fresh process: the parent commit's package cannot share this one's modules
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--package-root', args.parent_tree, '--N', str(N), '--reps', str(args.reps),
               '--warmup', str(args.warmup), '--train-traces', str(args.train_traces)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit('resample_bench: the parent tree failed:\n' + out.stderr[-2000:])
        parent = json.loads(out.stdout.strip().splitlines()[-1])
        parent['package_root'] = 'parent commit'
        assert parent['has_device_route'] is False
        print(json.dumps(parent), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), lstm_dim=512, program='GaussianWithUnknownMean', reps=args.reps, warmup=args.warmup,
               timing='host clock between device synchronisations; per case a block of warm-up + repetitions on the device route, then one on the host route; medians',
               device_route='Empirical.resample / sample / resample_batch on device tensors (pp_is_cdf_groups cached per object, '
                            'pp_is_resample_groups, pp_is_stats / grouped statistics)',
               host_route='the same calls under PP_EMPIRICAL_DEVICE=0: get_values() list, host exp and cumsum, one Python iteration per draw',
               parent_commit=parent, records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
