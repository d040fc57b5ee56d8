"""Time of Empirical.compare and pyprob_amd.compare_batch (csrc/is_twosample.hip) next to two other routes to the same numbers on the
same commit: the definitions in torch float64 on the device (sort + cumsum + searchsorted, batched over the groups) and cpu() of the
particles followed by the float64 numpy route (empirical_host._host_twosample). The posteriors are built from synthetic columns the
way a lock-step call leaves them. Cases: compare at N = 10^6 against 10^6 particles on FRESH objects (both sorts are part of the
call) and on already-SORTED ones (the sorts are kept with the objects); compare_batch at M = 256 pairs of 10^4 particles, fresh,
sorted and as the loop of compare calls. Every figure is the median of --reps device-event timings of ONE call after --warmup calls.
The operator alone is reported with the bytes it reads per second: 24 per merged element (a float value and a double cumulative
weight in each of the two walks). Writes one JSON document to profiles/twosample_bench.json (--out PATH).

    python tools/twosample_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
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
from pyprob_amd.empirical_host import _host_twosample  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

DEV = 'cuda'
FIELDS = ('ks', 'wasserstein1', 'wasserstein2', 'energy')


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'twosample_bench.json'))
    return ap.parse_args()


args = _args()


def event_timed(fn, reps=None, warmup=None):
    """Median, minimum and maximum over event pairs around one call of fn, in ms, after --warmup calls."""
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    ts = []
    for _ in range(reps or args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def posteriors(M, N, seed, shift):
    """The M groups of one batched call over synthetic columns: every member holds the call's tensors (`_batch`)."""
    from pyprob_amd.is_engine import DistRunner
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    x = torch.randn(M * N, device=DEV, generator=g) + shift
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    stats = torch.stack([ops.is_stats(lw[k * N:(k + 1) * N], x[k * N:(k + 1) * N], scratch)[:6] for k in range(M)]).contiguous()
    rows, log, posts = stats.cpu().numpy(), [{'x': (x, 0)}], []
    for k in range(M):
        p = Empirical.from_device(x[k * N:(k + 1) * N], lw[k * N:(k + 1) * N], DistRunner._stats_dict(rows[k]))
        p._batch, p._batch_log = (x, lw, stats, k, N), log
        posts.append(p)
    return lw, x, posts


def torch_twosample(lw_a, x_a, lw_b, x_b, M):
    """[M, 4] (ks, wasserstein1, wasserstein2, energy) by the definitions in torch float64 on the device, all groups at once."""
    def side(lw, x):
        v, order = torch.sort(x.view(M, -1).double(), dim=1)
        lw = lw.view(M, -1).double()
        c = torch.cumsum(torch.exp(torch.gather(lw, 1, order) - lw.max(dim=1, keepdim=True)[0]), dim=1)
        return v.contiguous(), (c / c[:, -1:]).contiguous()

    def at(u, k):       # the cumulative weight of the first k particles
        return torch.where(k > 0, torch.gather(u, 1, (k - 1).clamp(min=0)), torch.zeros((), dtype=u.dtype, device=u.device))
    (a, ua), (b, ub) = side(lw_a, x_a), side(lw_b, x_b)
    z = torch.sort(torch.cat([a, b], dim=1), dim=1)[0]
    D = at(ua, torch.searchsorted(a, z, right=True)) - at(ub, torch.searchsorted(b, z, right=True))
    gap = z[:, 1:] - z[:, :-1]
    u = torch.sort(torch.cat([ua, ub], dim=1), dim=1)[0]
    width = u - torch.cat([torch.zeros_like(u[:, :1]), u[:, :-1]], dim=1)
    d = torch.gather(a, 1, torch.searchsorted(ua, u).clamp(max=a.shape[1] - 1)) - \
        torch.gather(b, 1, torch.searchsorted(ub, u).clamp(max=b.shape[1] - 1))
    return torch.stack([D.abs().max(dim=1)[0], (D[:, :-1].abs() * gap).sum(1), (width * d * d).sum(1).sqrt(),
                        2.0 * (D[:, :-1] ** 2 * gap).sum(1)], dim=1).cpu().numpy()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def fresh(posts):
    for p in posts:
        for k in ('_dev_sorted', '_batch_sorted'):
            p.__dict__.pop(k, None)


def operator_alone(pa, pb, M, n_a, n_b):
    (va, _, _, ca, wa), (vb, _, _, cb, wb) = pa, pb
    op = event_timed(lambda: ops.is_twosample_groups(va, wa, ca, n_a, vb, wb, cb, n_b))
    return dict(op, bytes_read=24 * M * (n_a + n_b), bytes_per_s=float('%.4g' % (24 * M * (n_a + n_b) / (op['median_ms'] * 1e-3))))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('twosample_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    (lw_a, x_a, (a,)), (lw_b, x_b, (b,)) = posteriors(1, N, 21, 0.0), posteriors(1, N, 22, 0.1)
    r, ref = a.compare(b), torch_twosample(lw_a, x_a, lw_b, x_b, 1)[0]
    assert all(abs(getattr(r, k) - ref[i]) <= 1e-9 * ref[i] for i, k in enumerate(FIELDS)), (vars(r), ref)

    def compare_fresh():
        fresh([a, b])
        return a.compare(b)
    records.append(dict(case='compare, 10^6 against 10^6', M=1, N=[N, N], ours_fresh=event_timed(compare_fresh),
                        ours_sorted=event_timed(lambda: a.compare(b)),
                        torch_float64=event_timed(lambda: torch_twosample(lw_a, x_a, lw_b, x_b, 1), reps=5),
                        cpu_numpy=event_timed(lambda: _host_twosample(host(lw_a), host(x_a), host(lw_b), host(x_b)), reps=3, warmup=1),
                        operator_alone=operator_alone(a._device_sorted(), b._device_sorted(), 1, N, N)))
    print(json.dumps(records[-1]), flush=True)
    M, Nb = args.batch
    (lw_a, x_a, pa), (lw_b, x_b, pb) = posteriors(M, Nb, 7, 0.0), posteriors(M, Nb, 8, 0.1)
    fast, loop, ref = pyprob_amd.compare_batch(pa, pb), [p.compare(q) for p, q in zip(pa, pb)], torch_twosample(lw_a, x_a, lw_b, x_b, M)
    assert all(vars(f) == vars(l) for f, l in zip(fast, loop))
    assert all(abs(getattr(f, k) - ref[g, i]) <= 1e-9 * ref[g, i] for g, f in enumerate(fast) for i, k in enumerate(FIELDS))

    def batch_fresh():
        fresh(pa + pb)
        return pyprob_amd.compare_batch(pa, pb)
    ha, hb = [host(t).reshape(M, Nb) for t in (lw_a, x_a)], [host(t).reshape(M, Nb) for t in (lw_b, x_b)]
    records.append(dict(case='compare_batch', M=M, N=[Nb, Nb], ours_fresh=event_timed(batch_fresh),
                        ours_sorted=event_timed(lambda: pyprob_amd.compare_batch(pa, pb)),
                        loop_of_compare_sorted=event_timed(lambda: [p.compare(q) for p, q in zip(pa, pb)], reps=5),
                        torch_float64=event_timed(lambda: torch_twosample(lw_a, x_a, lw_b, x_b, M), reps=5),
                        cpu_numpy=event_timed(lambda: [_host_twosample(ha[0][g], ha[1][g], hb[0][g], hb[1][g]) for g in range(M)],
                                              reps=3, warmup=1),
                        operator_alone=operator_alone(pa[0].__dict__['_batch_sorted'][None], pb[0].__dict__['_batch_sorted'][None], M, Nb, Nb)))
    print(json.dumps(records[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup (torch '
                      'route 5 repetitions, numpy route 3 after 1; cpu_numpy of the batch excludes the copy of the particles)',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
