"""Time of Empirical.kde / kde2d and pyprob_amd.kde_batch (csrc/is_kde.hip) next to two other routes to the same numbers on the same
commit: the definition as a torch float64 broadcast on the device (chunked over the points so that a chunk stays below 2^27 elements)
and cpu() of the particles followed by the float64 numpy route (empirical_host). The posteriors are built from synthetic columns the
way a lock-step call leaves them. Cases: kde at N = 10^6 with Q = 512 and 2048; kde_batch at M = 256 posteriors of 10^4 particles
(Q = 512) against the loop of kde() calls; kde2d at 64 x 64 and 256 x 256. Every figure is the median of --reps device-event timings
of ONE call after --warmup calls. The operator alone (bandwidth and points on the device) is reported as pair evaluations per second
and as a share of a peak: 1-D, one v_exp_f32 per pair against 16 per clock and CU (quarter rate) x 256 CUs x 2.4 GHz = 9.83e12 / s;
2-D, the executed MFMA FLOPs (2 per pair of the padded 32 x 32 blocks) against the 157.3 TFLOP/s fp32 matrix peak of the data sheet.
Writes one JSON document to profiles/kde_bench.json (--out PATH).

    python tools/kde_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
import argparse
import json
import math
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
from pyprob_amd.empirical_host import _host_kde, _host_kde2d  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

EXP_PEAK = 16 * 256 * 2.4e9
MFMA_PEAK = 157.3e12
DEV = 'cuda'


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'kde_bench.json'))
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


def columns(M, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    x = torch.randn(M * N, device=DEV, generator=g)
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


def torch_kernel(pts, v, h):
    """exp(-z^2 / 2) [Q, n] in float64 on the device."""
    z = (pts[:, None] - v[None, :].double()) / h
    return torch.exp(-0.5 * z * z)


def torch_kde(lw, x, pts, h):
    w = torch.exp(lw.double() - lw.max().double())
    step = max(1, (1 << 27) // x.numel())
    dens = torch.cat([torch_kernel(pts[q:q + step], x, h) @ w for q in range(0, pts.numel(), step)])
    return (dens / (h * math.sqrt(2.0 * math.pi) * w.sum())).cpu().numpy()


def torch_kde2d(lw, x, y, px, py, hx, hy):
    w = torch.exp(lw.double() - lw.max().double())
    dens = torch.zeros((px.numel(), py.numel()), dtype=torch.float64, device=DEV)
    step = max(1, (1 << 27) // max(px.numel(), py.numel()))
    for i in range(0, x.numel(), step):
        dens += (torch_kernel(px, x[i:i + step], hx) * w[i:i + step]) @ torch_kernel(py, y[i:i + step], hy).T
    return (dens / (2.0 * math.pi * hx * hy * w.sum())).cpu().numpy()


def host(a):
    return a.cpu().numpy().astype(np.float64)


def emit(records, rec):
    print(json.dumps(rec), flush=True)
    records.append(rec)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('kde_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    lw, x, y = columns(1, N, 21)
    post = posterior(lw, x, y, group_stats(lw, x, 1, N)[0].cpu().numpy())
    as_dev = lambda a: torch.from_numpy(np.atleast_1d(np.asarray(a, np.float64))).to(DEV)      # noqa: E731
    for Q in (512, 2048):
        k = post.kde(grid=Q)
        pts, h = as_dev(k.x), as_dev(k.bandwidth)
        ref = torch_kde(lw, x, pts, k.bandwidth)
        assert np.abs(k.density - ref).max() <= 3e-5 * ref.max()
        op = event_timed(lambda: ops.is_kde_groups(lw, x, N, pts, h, None))
        rate = N * Q / (op['median_ms'] * 1e-3)
        emit(records, dict(case='kde(grid=%d)' % Q, M=1, N=N, Q=Q, ours=event_timed(lambda: post.kde(grid=Q)),
                           torch_float64_broadcast=event_timed(lambda: torch_kde(lw, x, pts, k.bandwidth), reps=5),
                           cpu_numpy=event_timed(lambda: _host_kde(host(lw), host(x), k.x, k.bandwidth), reps=1, warmup=0),
                           operator_alone=dict(op, pair_evaluations_per_s=float('%.4g' % rate), share_of_v_exp_f32_peak=round(rate / EXP_PEAK, 3))))
    for side in (64, 256):
        k2 = post.kde2d('x', 'y', grid=side)
        px, py, hx, hy = as_dev(k2.x), as_dev(k2.y), as_dev(k2.bandwidth[0]), as_dev(k2.bandwidth[1])
        ref = torch_kde2d(lw, x, y, px, py, *k2.bandwidth)
        assert np.abs(k2.density - ref).max() <= 3e-4 * ref.max()
        op = event_timed(lambda: ops.is_kde2d_groups(lw, x, y, N, px, py, hx, hy, None))
        padded = (32 * math.ceil(side / 32)) ** 2
        emit(records, dict(case='kde2d(grid=%d x %d)' % (side, side), M=1, N=N, ours=event_timed(lambda: post.kde2d('x', 'y', grid=side)),
                           torch_float64_broadcast=event_timed(lambda: torch_kde2d(lw, x, y, px, py, *k2.bandwidth), reps=5),
                           cpu_numpy=event_timed(lambda: _host_kde2d(host(lw), host(x), host(y), k2.x, k2.y, *k2.bandwidth), reps=1, warmup=0),
                           operator_alone=dict(op, pair_evaluations_per_s=float('%.4g' % (N * side * side / (op['median_ms'] * 1e-3))),
                                               share_of_fp32_mfma_peak_on_executed_flops=round(
                                                   2.0 * N * padded / (op['median_ms'] * 1e-3) / MFMA_PEAK, 3))))
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
    fast, loop = pyprob_amd.kde_batch(posts), [p.kde() for p in posts]
    assert all(np.array_equal(f.density, l.density) and np.array_equal(f.x, l.x) for f, l in zip(fast, loop))
    pts, h = as_dev(np.stack([f.x for f in fast])), as_dev([f.bandwidth for f in fast])
    op = event_timed(lambda: ops.is_kde_groups(lw, x, Nb, pts, h, stats))
    rate = M * Nb * 512 / (op['median_ms'] * 1e-3)
    hl, hx = host(lw).reshape(M, Nb), host(x).reshape(M, Nb)
    emit(records, dict(case='kde_batch(posts), every group its own grid and bandwidth', M=M, N=Nb, Q=512,
                       ours=event_timed(lambda: pyprob_amd.kde_batch(posts)), loop_of_kde=event_timed(lambda: [p.kde() for p in posts], reps=5),
                       torch_float64_broadcast=event_timed(lambda: [torch_kde(lw[g * Nb:(g + 1) * Nb], x[g * Nb:(g + 1) * Nb], pts[g],
                                                                              fast[g].bandwidth) for g in range(M)], reps=5),
                       cpu_numpy=event_timed(lambda: [_host_kde(hl[g], hx[g], fast[g].x, fast[g].bandwidth) for g in range(M)], reps=1, warmup=0),
                       operator_alone=dict(op, pair_evaluations_per_s=float('%.4g' % rate), share_of_v_exp_f32_peak=round(rate / EXP_PEAK, 3))))
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup '
                      '(torch route 5 repetitions; numpy route ONE call without a warm-up; cpu_numpy of the batch excludes the copy of the particles)',
               peaks=dict(v_exp_f32_per_s=EXP_PEAK, fp32_mfma_flops=MFMA_PEAK,
                          note='16 v_exp_f32 per clock and CU x 256 CUs x 2.4 GHz; the data sheet\'s fp32 matrix rate'),
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
