"""Time of Empirical.quantile / credible_interval / combine_duplicates and pyprob_amd.quantile_batch (csrc/is_sort.hip) next to two
other routes to the same numbers on the same machine, neither of which is the code under test:
    torch   torch.sort (stable) of the values on the device, the weights exp(lw - max) in float64, torch.cumsum and
            torch.searchsorted (quantiles); torch.unique_consecutive and index_add_ of the float64 weights (combine_duplicates);
    numpy   cpu() of the log-weights and the values, numpy's stable argsort, cumsum and searchsorted; numpy.unique and bincount.
The posteriors are built from synthetic columns the way a lock-step call leaves them (Empirical.from_device; for the batch the call's
whole tensors and its [M, 6] statistics). Cases at ONE group of --N particles: quantile(0.5) on a fresh object (sort, cumulative
weights and search) and on one that is already sorted; credible_interval on a sorted object; combine_duplicates on a latent of five
values and on an all-distinct one (fresh objects); quantile_batch at --batch M N against the loop. Every figure is the median of
--reps device-event timings of ONE call after --warmup calls (the event pair spans the launches, the copies and the host arithmetic
of the call); the sort operator alone (10 calls per event pair) is reported in microseconds and as effective TB/s against the
20 bytes per particle it must move (lw and x in; value, lw and index out). Writes one JSON document to
profiles/order_stats_bench.json (--out PATH).

    python tools/order_stats_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'order_stats_bench.json'))
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


def columns(M, N, seed, five=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    x = torch.randn(M * N, device=DEV, generator=g)
    if five:
        x = torch.clamp(torch.round(x), -2.0, 2.0) + 0.0      # (+ 0.0: no -0.0, so that every route sees five bit patterns)
    return lw, x


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, x, stats_row):
    from pyprob_amd.is_engine import DistRunner
    return Empirical.from_device(x, lw, DistRunner._stats_dict(stats_row))


# ---- the two other routes ---------------------------------------------------------------------------------------------------
def torch_quantiles(lw, x, M, N, qs):
    v, idx = torch.sort(x.view(M, N), dim=1, stable=True)
    l = torch.gather(lw.view(M, N), 1, idx).double()
    cdf = torch.cumsum(torch.exp(l - l.max(1, keepdim=True)[0]), 1)
    t = torch.as_tensor(qs, dtype=torch.float64, device=x.device)[None, :] * cdf[:, -1:]
    k = torch.searchsorted(cdf, t.contiguous()).clamp(max=N - 1)
    return torch.gather(v, 1, k).cpu().numpy()


def numpy_quantiles(lw, x, M, N, qs):
    l, v = lw.cpu().numpy().reshape(M, N).astype(np.float64), x.cpu().numpy().reshape(M, N)
    out = np.empty((M, len(qs)))
    for g in range(M):
        order = np.argsort(v[g], kind='stable')
        cdf = np.cumsum(np.exp(l[g][order] - l[g].max()))
        out[g] = v[g][order][np.minimum(np.searchsorted(cdf, np.asarray(qs) * cdf[-1]), N - 1)]
    return out


def torch_combine(lw, x):
    v, idx = torch.sort(x, stable=True)
    l = lw[idx].double()
    u, inv = torch.unique_consecutive(v, return_inverse=True)
    mass = torch.zeros(u.numel(), dtype=torch.float64, device=x.device).index_add_(0, inv, torch.exp(l - l.max()))
    return u, (torch.log(mass) + l.max()).float()


def numpy_combine(lw, x):
    l, v = lw.cpu().numpy().astype(np.float64), x.cpu().numpy()
    u, inv = np.unique(v, return_inverse=True)
    return u, np.log(np.bincount(inv, weights=np.exp(l - l.max()))) + l.max()


def record(case, M, N, ours, torch_route, numpy_route, extra=None):
    rec = dict(case=case, M=M, N=N, ours=event_timed(ours), torch_sort_route=event_timed(torch_route),
               cpu_numpy_route=event_timed(numpy_route))
    rec['torch_over_ours'] = round(rec['torch_sort_route']['median_ms'] / rec['ours']['median_ms'], 2)
    rec['numpy_over_ours'] = round(rec['cpu_numpy_route']['median_ms'] / rec['ours']['median_ms'], 2)
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit('order_stats_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    lw, x = columns(1, N, 31)
    row = group_stats(lw, x, 1, N)[0].cpu().numpy()
    post = posterior(lw, x, row)
    qs = [0.05, 0.5, 0.95]
    want = numpy_quantiles(lw, x, 1, N, qs)[0]
    # (the three routes round their cumulative weights differently: where q T falls within that rounding of a particle's
    # cumulative weight they may name neighbouring particles - 1e-3 apart at most at this density)
    assert np.abs(post.quantile(qs) - want).max() <= 1e-3 and np.abs(torch_quantiles(lw, x, 1, N, qs)[0] - want).max() <= 1e-3
    records.append(record('quantile(0.5), first call on an object: sort, cumulative weights, search', 1, N,
                          lambda: posterior(lw, x, row).quantile(0.5), lambda: torch_quantiles(lw, x, 1, N, [0.5]),
                          lambda: numpy_quantiles(lw, x, 1, N, [0.5])))
    records.append(record('quantile(0.5), the object already sorted (the other routes sort again: they keep nothing)', 1, N,
                          lambda: post.quantile(0.5), lambda: torch_quantiles(lw, x, 1, N, [0.5]),
                          lambda: numpy_quantiles(lw, x, 1, N, [0.5])))
    records.append(record('credible_interval(0.9), the object already sorted', 1, N, lambda: post.credible_interval(0.9),
                          lambda: torch_quantiles(lw, x, 1, N, [0.05, 0.95]), lambda: numpy_quantiles(lw, x, 1, N, [0.05, 0.95])))
    for five in (True, False):
        lw2, x2 = columns(1, N, 41 + five, five)
        row2 = group_stats(lw2, x2, 1, N)[0].cpu().numpy()
        d = posterior(lw2, x2, row2).combine_duplicates()
        u, nl = numpy_combine(lw2, x2)
        assert np.array_equal(d._values.cpu().numpy(), u)
        assert np.abs(np.exp(d.log_weights_numpy() - nl.max()) - np.exp(nl - nl.max())).max() <= 1e-9
        records.append(record('combine_duplicates(), fresh object, %s' % ('a latent of five values' if five else 'all values distinct'),
                              1, N, lambda: posterior(lw2, x2, row2).combine_duplicates(), lambda: torch_combine(lw2, x2),
                              lambda: numpy_combine(lw2, x2), extra=dict(distinct=int(d.length))))
    sort = event_timed(lambda: ops.is_sort_groups(lw, x, N, None), per=10)
    records.append(dict(case='is_sort_groups alone', M=1, N=N, kernel_alone=dict(
        sort, microseconds=round(sort['median_ms'] * 1e3, 1), bytes_per_particle=20,
        effective_TB_per_s=round(N * 20 / (sort['median_ms'] * 1e-3) / 1e12, 4),
        timing='device events around 10 calls of the operator (each allocates its outputs and workspace)'),
        torch_sort_alone=event_timed(lambda: torch.sort(x, stable=True), per=10)))
    print(json.dumps(records[-1]), flush=True)
    M, Nb = args.batch
    lw, x = columns(M, Nb, 7)
    stats = group_stats(lw, x, M, Nb)
    host_stats = stats.cpu().numpy()
    posts, whole_log = [], []
    for g in range(M):
        sl = slice(g * Nb, (g + 1) * Nb)
        p = posterior(lw[sl], x[sl], host_stats[g])
        p._batch, p._batch_log = (x, lw, stats, g, Nb), whole_log
        posts.append(p)
    from pyprob_amd.empirical_batch import _batch_column
    assert _batch_column(posts, None) is not None, 'the posteriors must be recognised as one batched execution'
    fast = pyprob_amd.quantile_batch(posts, qs)
    assert np.array_equal(fast, np.stack([p.quantile(qs) for p in posts])) and np.abs(fast - numpy_quantiles(lw, x, M, Nb, qs)).max() <= 0.05

    def fresh_loop():
        for p in posts:
            p.__dict__.pop('_dev_sorted', None)
        return [p.quantile(qs) for p in posts]
    loop_time = event_timed(fresh_loop)
    records.append(record('quantile_batch(posts, [0.05, 0.5, 0.95])', M, Nb, lambda: pyprob_amd.quantile_batch(posts, qs),
                          lambda: torch_quantiles(lw, x, M, Nb, qs), lambda: numpy_quantiles(lw, x, M, Nb, qs),
                          extra=dict(loop_of_first_quantile_calls=loop_time)))
    records[-1]['loop_over_ours'] = round(loop_time['median_ms'] / records[-1]['ours']['median_ms'], 2)
    sort = event_timed(lambda: ops.is_sort_groups(lw, x, Nb, stats), per=10)
    records.append(dict(case='is_sort_groups alone', M=M, N=Nb, kernel_alone=dict(
        sort, microseconds=round(sort['median_ms'] * 1e3, 1), bytes_per_particle=20,
        effective_TB_per_s=round(M * Nb * 20 / (sort['median_ms'] * 1e-3) / 1e12, 4)),
        torch_sort_alone=event_timed(lambda: torch.sort(x.view(M, Nb), dim=1, stable=True), per=10)))
    print(json.dumps(records[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup',
               inputs='synthetic values and log-weights (normal), attached to Empiricals as a lock-step call attaches them',
               ours='Empirical.quantile / credible_interval / combine_duplicates / pyprob_amd.quantile_batch: pp_is_sort_groups (stable '
                    'LSD radix sort, 8-bit digits), pp_is_cdf_groups over the sorted log-weights, pp_is_quantile_groups / '
                    'pp_is_unique_groups, one copy of the answers',
               torch_sort_route='torch.sort(stable) + float64 exp / cumsum + searchsorted (unique_consecutive + index_add_) on the device',
               cpu_numpy_route='cpu() of the columns, numpy stable argsort + cumsum + searchsorted (unique + bincount)',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
