"""Time of Empirical.hpd_interval / cdf / resample(scheme=) and pyprob_amd.hpd_batch / cdf_batch (csrc/is_hpd.hip,
pp_is_resample_scheme_groups of csrc/is_resample.hip) next to two other routes to the same numbers on the same machine, neither of
which is the code under test:
    torch   the same definition in float64 on the device: torch.sort (stable), exp(lw - max), torch.cumsum, torch.searchsorted of
            every start's target and torch.argmin of the widths (HPD); searchsorted of the points in the sorted values (cdf);
            searchsorted of the (j + u) / n positions in the cumulative weights (resample);
    numpy   cpu() of the log-weights and the values, then the same definition in numpy.
The posteriors are built from synthetic columns the way a lock-step call leaves them (Empirical.from_device; for the batch the call's
whole tensors and its [M, 6] statistics). Cases at ONE group of --N particles: hpd_interval(0.9), cdf at 1 point and at 1000 points and
resample(N, scheme) on a fresh object (sort or cumulative weights included) and on one that already holds them; hpd_batch and cdf_batch
at --batch M N against the loop. Every figure is the median of --reps device-event timings of ONE call after --warmup calls (the
event pair spans the launches, the copies and the host arithmetic of the call); the operators alone (10 calls per event pair) are
reported in microseconds. Writes one JSON document to profiles/intervals_bench.json (--out PATH).

    python tools/intervals_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'intervals_bench.json'))
    return ap.parse_args()


args = _args()
DEV = 'cuda'
SCHEMES = {'multinomial': 0, 'stratified': 1, 'systematic': 2}


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


def columns(M, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    x = -torch.log(torch.rand(M * N, device=DEV, generator=g).clamp_min(1e-30))      # a one-sided (Exponential) latent
    return lw, x


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, x, stats_row):
    from pyprob_amd.is_engine import DistRunner
    return Empirical.from_device(x, lw, DistRunner._stats_dict(stats_row))


# ---- the two other routes ---------------------------------------------------------------------------------------------------
def torch_sorted(lw, x, M, N):
    v, idx = torch.sort(x.view(M, N), dim=1, stable=True)
    l = torch.gather(lw.view(M, N), 1, idx).double()
    return v, torch.cumsum(torch.exp(l - l.max(1, keepdim=True)[0]), 1)


def torch_hpd(lw, x, M, N, level):
    v, cdf = torch_sorted(lw, x, M, N)
    T = cdf[:, -1:]
    prev = torch.cat([torch.zeros_like(T), cdf[:, :-1]], 1)
    t = prev + level * T
    ends = torch.maximum(torch.searchsorted(cdf, t.contiguous()).clamp(max=N - 1), torch.arange(N, device=x.device)[None, :])
    width = torch.gather(v, 1, ends).double() - v.double()
    width = torch.where((cdf > prev) & (t <= T), width, torch.full_like(width, float('inf')))
    i = torch.argmin(width, 1, keepdim=True)
    return torch.cat([torch.gather(v, 1, i), torch.gather(v, 1, torch.gather(ends, 1, i))], 1).cpu().numpy()


def numpy_hpd(lw, x, M, N, level):
    l, v = lw.cpu().numpy().reshape(M, N).astype(np.float64), x.cpu().numpy().reshape(M, N)
    out = np.empty((M, 2))
    for g in range(M):
        order = np.argsort(v[g], kind='stable')
        sv = v[g][order]
        cdf = np.cumsum(np.exp(l[g][order] - l[g].max()))
        prev = np.concatenate([[0.0], cdf[:-1]])
        t = prev + level * cdf[-1]
        starts = np.nonzero((cdf > prev) & (t <= cdf[-1]))[0]
        ends = np.maximum(starts, np.searchsorted(cdf, t[starts]))
        k = np.argmin(sv[ends].astype(np.float64) - sv[starts])
        out[g] = sv[starts[k]], sv[ends[k]]
    return out


def torch_cdf(lw, x, M, N, pts):
    v, cdf = torch_sorted(lw, x, M, N)
    k = torch.searchsorted(v, pts.float().contiguous(), right=True)
    out = torch.gather(cdf, 1, (k - 1).clamp(min=0)) / cdf[:, -1:]
    return torch.where(k == 0, torch.zeros_like(out), out).cpu().numpy()


def numpy_cdf(lw, x, M, N, pts):
    l, v, p = lw.cpu().numpy().reshape(M, N).astype(np.float64), x.cpu().numpy().reshape(M, N), pts.cpu().numpy()
    out = np.empty(p.shape)
    for g in range(M):
        order = np.argsort(v[g], kind='stable')
        cdf = np.cumsum(np.exp(l[g][order] - l[g].max()))
        k = np.searchsorted(v[g][order], p[g], side='right')
        out[g] = np.where(k == 0, 0.0, cdf[np.maximum(k, 1) - 1] / cdf[-1])
    return out


def torch_resample(lw, x, n, scheme):
    l = lw.double()
    cdf = torch.cumsum(torch.exp(l - l.max()), 0)
    u = torch.rand(1 if scheme == 'systematic' else n, dtype=torch.float64, device=x.device)
    p = u if scheme == 'multinomial' else (torch.arange(n, dtype=torch.float64, device=x.device) + u) / n
    return x[torch.searchsorted(cdf, p * cdf[-1], right=True).clamp(max=x.numel() - 1)]


def numpy_resample(lw, x, n, scheme):
    l, v = lw.cpu().numpy().astype(np.float64), x.cpu().numpy()
    cdf = np.cumsum(np.exp(l - l.max()))
    u = np.random.random(1 if scheme == 'systematic' else n)
    p = u if scheme == 'multinomial' else (np.arange(n) + u) / n
    return v[np.minimum(np.searchsorted(cdf, p * cdf[-1], side='right'), len(v) - 1)]


def record(case, M, N, ours, torch_route, numpy_route, extra=None):
    rec = dict(case=case, M=M, N=N, ours=event_timed(ours), torch_route=event_timed(torch_route),
               cpu_numpy_route=event_timed(numpy_route))
    rec['torch_over_ours'] = round(rec['torch_route']['median_ms'] / rec['ours']['median_ms'], 2)
    rec['numpy_over_ours'] = round(rec['cpu_numpy_route']['median_ms'] / rec['ours']['median_ms'], 2)
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def alone(case, M, N, fn):
    t = event_timed(fn, per=10)
    rec = dict(case=case, M=M, N=N, kernel_alone=dict(t, microseconds=round(t['median_ms'] * 1e3, 1),
               timing='device events around 10 calls of the operator (each allocates its outputs and workspace)'))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit('intervals_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    lw, x = columns(1, N, 31)
    row = group_stats(lw, x, 1, N)[0].cpu().numpy()
    post = posterior(lw, x, row)
    # the three routes round their cumulative weights differently: where a target falls within that rounding of a particle's
    # cumulative weight they may name neighbouring particles, so the ends agree to the spacing of the particles, not to the bit
    want = numpy_hpd(lw, x, 1, N, 0.9)[0]
    got = np.array(post.hpd_interval(0.9))
    # - what they agree on is the minimum they found, the width
    other = torch_hpd(lw, x, 1, N, 0.9)[0]
    assert abs((got[1] - got[0]) - (want[1] - want[0])) <= 1e-3 and abs((other[1] - other[0]) - (want[1] - want[0])) <= 1e-3, (got, want)
    one = torch.tensor([[1.0]], dtype=torch.float64, device=DEV)
    many = torch.linspace(0.0, 8.0, 1000, dtype=torch.float64, device=DEV)[None].contiguous()
    assert np.abs(post.cdf(many[0].cpu().numpy()) - numpy_cdf(lw, x, 1, N, many)[0]).max() <= 1e-9
    assert np.abs(torch_cdf(lw, x, 1, N, many)[0] - numpy_cdf(lw, x, 1, N, many)[0]).max() <= 1e-2      # (float32 points)
    records.append(record('hpd_interval(0.9), first call on an object: sort, cumulative weights, search', 1, N,
                          lambda: posterior(lw, x, row).hpd_interval(0.9), lambda: torch_hpd(lw, x, 1, N, 0.9),
                          lambda: numpy_hpd(lw, x, 1, N, 0.9), extra=dict(interval=[float(got[0]), float(got[1])],
                          equal_tailed=list(post.credible_interval(0.9)))))
    records.append(record('hpd_interval(0.9), the object already sorted (the other routes sort again: they keep nothing)', 1, N,
                          lambda: post.hpd_interval(0.9), lambda: torch_hpd(lw, x, 1, N, 0.9), lambda: numpy_hpd(lw, x, 1, N, 0.9)))
    for name, pts in (('1 point', one), ('1000 points', many)):
        host_pts = pts[0].cpu().numpy()
        records.append(record('cdf at %s, first call on an object' % name, 1, N, lambda: posterior(lw, x, row).cdf(host_pts),
                              lambda: torch_cdf(lw, x, 1, N, pts), lambda: numpy_cdf(lw, x, 1, N, pts)))
        records.append(record('cdf at %s, the object already sorted' % name, 1, N, lambda: post.cdf(host_pts),
                              lambda: torch_cdf(lw, x, 1, N, pts), lambda: numpy_cdf(lw, x, 1, N, pts)))
    for scheme in SCHEMES:
        kw = {} if scheme == 'multinomial' else dict(scheme=scheme)
        records.append(record('resample(N, %s), first call on an object: cumulative weights, draws, statistics' % scheme, 1, N,
                              lambda: posterior(lw, x, row).resample(N, seed=3, **kw), lambda: torch_resample(lw, x, N, scheme),
                              lambda: numpy_resample(lw, x, N, scheme)))
        post._device_cdf()
        records.append(record('resample(N, %s), the cumulative weights kept' % scheme, 1, N,
                              lambda: post.resample(N, seed=3, **kw), lambda: torch_resample(lw, x, N, scheme),
                              lambda: numpy_resample(lw, x, N, scheme)))
    value, _, _, counted, cdf = post._device_sorted()
    level = torch.tensor([0.9], dtype=torch.float64, device=DEV)
    records.append(alone('is_hpd_groups alone, 1 level', 1, N, lambda: ops.is_hpd_groups(value, cdf, counted, N, level)))
    records.append(alone('is_ecdf_groups alone, 1 point', 1, N, lambda: ops.is_ecdf_groups(value, cdf, counted, N, one, False)))
    records.append(alone('is_ecdf_groups alone, 1000 points', 1, N, lambda: ops.is_ecdf_groups(value, cdf, counted, N, many, False)))
    plain = post._device_cdf()
    records.append(alone('is_resample_groups alone, N draws', 1, N, lambda: ops.is_resample_groups(plain, x, N, 0, N, N, 3, 0, False)))
    for scheme in ('stratified', 'systematic'):
        records.append(alone('is_resample_scheme_groups alone, N draws, %s' % scheme, 1, N,
                             lambda: ops.is_resample_scheme_groups(plain, x, N, 0, N, N, SCHEMES[scheme], 3, 0, False)))
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
    truths = torch.rand(M, 1, dtype=torch.float64, device=DEV) * 3.0
    host_truths = truths.cpu().numpy()[:, 0]
    fast = pyprob_amd.hpd_batch(posts, 0.9)
    slow = numpy_hpd(lw, x, M, Nb, 0.9)
    assert np.array_equal(fast, np.stack([p.hpd_interval(0.9) for p in posts]))
    assert np.abs((fast[:, 1] - fast[:, 0]) - (slow[:, 1] - slow[:, 0])).max() <= 1e-3
    fast = pyprob_amd.cdf_batch(posts, host_truths)
    assert np.array_equal(fast, np.array([p.cdf(t) for p, t in zip(posts, host_truths)]))
    assert np.abs(fast - numpy_cdf(lw, x, M, Nb, truths)[:, 0]).max() <= 1e-9

    def fresh(call):
        def run():
            for p in posts:
                p.__dict__.pop('_dev_sorted', None)
            return [call(g, p) for g, p in enumerate(posts)]
        return run
    loop = event_timed(fresh(lambda g, p: p.hpd_interval(0.9)))
    records.append(record('hpd_batch(posts, 0.9)', M, Nb, lambda: pyprob_amd.hpd_batch(posts, 0.9), lambda: torch_hpd(lw, x, M, Nb, 0.9),
                          lambda: numpy_hpd(lw, x, M, Nb, 0.9), extra=dict(loop_of_first_hpd_interval_calls=loop)))
    records[-1]['loop_over_ours'] = round(loop['median_ms'] / records[-1]['ours']['median_ms'], 2)
    loop = event_timed(fresh(lambda g, p: p.cdf(host_truths[g])))
    records.append(record('cdf_batch(posts, truths [M])', M, Nb, lambda: pyprob_amd.cdf_batch(posts, host_truths),
                          lambda: torch_cdf(lw, x, M, Nb, truths), lambda: numpy_cdf(lw, x, M, Nb, truths),
                          extra=dict(loop_of_first_cdf_calls=loop)))
    records[-1]['loop_over_ours'] = round(loop['median_ms'] / records[-1]['ours']['median_ms'], 2)
    value, lws, _, counted = ops.is_sort_groups(lw, x, Nb, stats)
    cdf = ops.is_cdf_groups(lws, Nb, stats)
    records.append(alone('is_hpd_groups alone, 1 level', M, Nb, lambda: ops.is_hpd_groups(value, cdf, counted, Nb, level)))
    records.append(alone('is_ecdf_groups alone, 1 point per group', M, Nb, lambda: ops.is_ecdf_groups(value, cdf, counted, Nb, truths, False)))
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup',
               inputs='synthetic log-weights (normal, sd 2) and values (Exponential), attached to Empiricals as a lock-step call attaches them',
               ours='Empirical.hpd_interval / cdf / resample(scheme=) / pyprob_amd.hpd_batch / cdf_batch: pp_is_sort_groups, '
                    'pp_is_cdf_groups over the sorted log-weights, pp_is_hpd_groups / pp_is_ecdf_groups / '
                    'pp_is_resample_scheme_groups, one copy of the answers',
               torch_route='torch.sort(stable) + float64 exp / cumsum + searchsorted (+ argmin) on the device',
               cpu_numpy_route='cpu() of the columns, numpy stable argsort + cumsum + searchsorted (+ argmin)',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
