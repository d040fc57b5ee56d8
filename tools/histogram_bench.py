"""Time of Empirical.histogram / histogram2d and pyprob_amd.histogram_batch (csrc/is_hist.hip) next to the host route to the same
numbers on the same commit: cpu() of the log-weights and the values, exp in float64, numpy.histogram / numpy.histogram2d.
The posteriors are built from synthetic columns the way a lock-step call leaves them (Empirical.from_device + statement_log; for the
batch the call's whole tensors and its [M, 6] statistics). Cases: histogram(50) and histogram(2048) at N = 10^6 particles for a BROAD
posterior (x ~ normal, range found by pp_is_extent_groups) and a NARROW one whose particles all fall into the two bins around 0 of
range=(-4, 4) - every lane of a wave adds to one of two LDS addresses, the contention case; histogram2d at 32 x 32; histogram_batch
at M = 256 posteriors of 10^4 particles against the loop of histogram() calls. Every figure is the median of --reps device-event
timings of ONE call after --warmup calls (the event pair spans the launches, the copies and the host arithmetic of the call); the
kernel sequence alone (the operator, 20 calls per event pair, edges already on the device) is reported with its effective bytes per
second against (4 + 4) bytes per particle (12 for 2-D). Writes one JSON document to profiles/histogram_bench.json (--out PATH).

    python tools/histogram_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import lib as L  # noqa: E402
from pyprob_amd.distributions import Empirical  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'histogram_bench.json'))
    return ap.parse_args()


args = _args()
DEV = 'cuda'


def event_timed(fn, per=1):
    """Median, minimum and maximum over --reps event pairs around `per` calls of fn, in ms per call, after --warmup calls."""
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / per)
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def columns(M, N, seed, narrow=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    x = torch.randn(M * N, device=DEV, generator=g) * (1e-4 if narrow else 1.0)
    y = torch.randn(M * N, device=DEV, generator=g) * 1.5 + 0.5 * x
    return lw, x, y


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, x, y, stats_row):
    from pyprob_amd.is_engine import DistRunner
    emp = Empirical.from_device(x, lw, DistRunner._stats_dict(stats_row))
    emp._all_values, emp._all_log_weights = x, lw
    emp.statement_log = [{'y': (y, 0)}, {'x': (x, 1)}]
    emp._statement_rows_raw, emp.statement_names = [{'y': None}, {'x': None}], {}
    return emp


def host_weights(lw, M, N):
    l = lw.cpu().numpy().reshape(M, N).astype(np.float64)
    w = np.exp(l - l.max(1, keepdims=True))
    return w / w.sum(1, keepdims=True)


def host_route(lw, x, M, N, bins, rng):
    w = host_weights(lw, M, N)
    v = x.cpu().numpy().reshape(M, N).astype(np.float64)
    return [np.histogram(v[g], bins, range=rng, weights=w[g]) for g in range(M)]


def host_route_2d(lw, x, y, N, bins):
    w = host_weights(lw, 1, N)[0]
    return np.histogram2d(x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64), bins, weights=w)


def record(case, M, N, ours, host, kernel_fn, per_particle, extra=None):
    kernel = event_timed(kernel_fn, per=20)
    rec = dict(case=case, M=M, N=N, ours=event_timed(ours), host_numpy=event_timed(host),
               kernel_alone=dict(kernel, bytes_per_particle=per_particle,
                                 effective_GB_per_s=round(M * N * per_particle / (kernel['median_ms'] * 1e-3) / 1e9, 1),
                                 timing='device events around 20 calls of the operator (each allocates its output and workspace)'))
    rec['host_over_ours'] = round(rec['host_numpy']['median_ms'] / rec['ours']['median_ms'], 2)
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit('histogram_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    for narrow in (False, True):
        lw, x, y = columns(1, N, 21 + narrow, narrow)
        post = posterior(lw, x, y, group_stats(lw, x, 1, N)[0].cpu().numpy())
        rng = (-4.0, 4.0) if narrow else None
        for bins in (50, 2048):
            h = post.histogram(bins, range=rng)
            ref = host_route(lw, x, 1, N, bins, rng)[0]
            assert np.array_equal(h.count, np.histogram(x.cpu().numpy().astype(np.float64), bins, range=rng)[0])
            assert np.abs(h.mass - ref[0]).max() <= 1e-9
            if narrow:
                assert (h.count > 0).sum() == 2, 'the narrow posterior must sit in two bins'
            edges = torch.from_numpy(h.edges).to(DEV)
            records.append(record('histogram(%d), %s' % (bins, 'narrow: all particles in two bins, range given' if narrow
                                                         else 'broad, range from the extent kernel'), 1, N,
                                  lambda: post.histogram(bins, range=rng), lambda: host_route(lw, x, 1, N, bins, rng),
                                  lambda: ops.is_hist_groups(lw, x, None, N, edges, None, None), 8))
        if not narrow:
            h2 = post.histogram2d('x', 'y', bins=(32, 32))
            ref2 = host_route_2d(lw, x, y, N, (32, 32))
            assert np.abs(h2.mass - ref2[0]).max() <= 1e-9
            ex, ey = torch.from_numpy(h2.x_edges).to(DEV), torch.from_numpy(h2.y_edges).to(DEV)
            records.append(record('histogram2d(32 x 32), broad, ranges from the extent kernel', 1, N,
                                  lambda: post.histogram2d('x', 'y', bins=(32, 32)), lambda: host_route_2d(lw, x, y, N, (32, 32)),
                                  lambda: ops.is_hist_groups(lw, x, y, N, ex, ey, None), 12))
            extent = event_timed(lambda: ops.is_extent_groups(lw, x, N), per=20)
            records.append(dict(case='pp_is_extent_groups alone', M=1, N=N, kernel_alone=dict(
                extent, bytes_per_particle=8, effective_GB_per_s=round(N * 8 / (extent['median_ms'] * 1e-3) / 1e9, 1))))
            print(json.dumps(records[-1]), flush=True)
    M, Nb = args.batch
    lw, x, y = columns(M, Nb, 7)
    stats = group_stats(lw, x, M, Nb)
    host_stats = stats.cpu().numpy()
    whole_log = [{'y': (y, 0)}, {'x': (x, 1)}]
    posts = []
    for g in range(M):
        sl = slice(g * Nb, (g + 1) * Nb)
        p = posterior(lw[sl], x[sl], y[sl], host_stats[g])
        p._batch, p._batch_log = (x, lw, stats, g, Nb), whole_log
        posts.append(p)
    fast = pyprob_amd.histogram_batch(posts, 50)
    loop = [p.histogram(50) for p in posts]
    assert all(np.array_equal(f.mass, l.mass) and np.array_equal(f.edges, l.edges) and np.array_equal(f.count, l.count)
               for f, l in zip(fast, loop))
    edges = torch.from_numpy(np.stack([f.edges for f in fast])).to(DEV)
    loop_time = event_timed(lambda: [p.histogram(50) for p in posts])
    records.append(record('histogram_batch(posts, 50), every group its own extent', M, Nb, lambda: pyprob_amd.histogram_batch(posts, 50),
                          lambda: host_route(lw, x, M, Nb, 50, None), lambda: ops.is_hist_groups(lw, x, None, Nb, edges, None, stats), 8,
                          extra=dict(loop_of_histogram=loop_time)))
    records[-1]['loop_over_ours'] = round(loop_time['median_ms'] / records[-1]['ours']['median_ms'], 2)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup',
               inputs='synthetic values and log-weights (normal), attached to Empiricals as a lock-step call attaches them',
               ours='Empirical.histogram / histogram2d / pyprob_amd.histogram_batch: pp_is_extent_groups where the range is needed, '
                    'pp_is_hist_groups (fp64 weights, 64-bit fixed-point LDS histogram per tile), one copy of the rows',
               host_numpy='cpu() of the log-weights and the values, exp in float64, numpy.histogram / histogram2d with weights',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
