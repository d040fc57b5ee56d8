"""Time of Empirical.pareto_k / psis and pyprob_amd.pareto_k_batch / psis_batch (csrc/is_psis.hip) next to two other routes to the
same numbers on the same machine, neither of which is the code under test:
    torch   the same definition in float64 on the device: torch.sort (stable) of the log-weights, the exceedances, the m x n table
            of log1p as one broadcast, the m x m table of exp for the weights of the grid, the smoothed tail scattered back (one
            group at a time: the tail bounds of a group are data-dependent);
    numpy   cpu() of the log-weights, then the same definition in numpy (the host route of Empirical.psis).
The posteriors are built from synthetic columns the way a lock-step call leaves them (Empirical.from_device; for the batch the call's
whole tensors and its [M, 6] statistics). Cases at ONE group of --N particles: pareto_k() and psis() on a fresh object (the sort by
log-weight included) and on one that already holds it; pareto_k_batch and psis_batch at --batch M N against the loop. Every figure is
the median of --reps device-event timings of ONE call after --warmup calls (the event pair spans the launches, the copies and the host
arithmetic of the call); the operator alone (10 calls per event pair) is reported in microseconds. Writes one JSON document to
profiles/psis_bench.json (--out PATH).

    python tools/psis_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
import argparse
import json
import math
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import lib as L  # noqa: E402
from pyprob_amd.distributions import Empirical  # noqa: E402
from pyprob_amd.empirical_host import _host_psis  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'psis_bench.json'))
    return ap.parse_args()


args = _args()
DEV = 'cuda'
warnings.simplefilter('ignore')          # (psis() warns above k-hat 0.7: not what is timed)


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
    lw = -0.5 * torch.log(torch.rand(M * N, device=DEV, generator=g).clamp_min(1e-30))      # weights U^-0.5: a Pareto tail, k = 0.5
    x = torch.randn(M * N, device=DEV, generator=g)
    return lw.contiguous(), x


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, x, stats_row):
    from pyprob_amd.is_engine import DistRunner
    return Empirical.from_device(x, lw, DistRunner._stats_dict(stats_row))


# ---- the two other routes ---------------------------------------------------------------------------------------------------
def torch_psis(lw, want_weights):
    """(k-hat, smoothed log-weights or None) of one group of finite log-weights."""
    s, idx = torch.sort(lw.double(), stable=True)
    c = s.numel()
    b = c - int(math.ceil(min(c / 5.0, 3.0 * math.sqrt(float(c))))) - 1
    f = int(torch.searchsorted(s, s[b:b + 1], right=True))
    n = c - f
    Mg = s[-1]
    u = torch.exp(s[b] - Mg)
    y = torch.exp(s[f:] - Mg) - u
    m = 30 + int(math.floor(math.sqrt(float(n))))
    q = y[int(n / 4.0 + 0.5) - 1]
    j = torch.arange(1, m + 1, dtype=torch.float64, device=lw.device)
    theta = 1.0 / y[-1] + (1.0 - torch.sqrt(m / (j - 0.5))) / (3.0 * q)
    kap = torch.log1p(-theta[:, None] * y[None, :]).sum(1) / n
    prof = n * (torch.log(-theta / kap) - kap - 1.0)
    omega = 1.0 / torch.exp(prof[None, :] - prof[:, None]).sum(1)
    that = (omega * theta).sum()
    kappa = torch.log1p(-that * y).sum() / n
    sigma = -kappa / that
    khat = (n * kappa + 5.0) / (n + 10.0)
    out = None
    if want_weights:
        lp = torch.log1p(-(torch.arange(n, dtype=torch.float64, device=lw.device) + 0.5) / n)
        w = u + sigma * torch.expm1(-khat * lp) / khat
        out = lw.clone()
        out[idx[f:]] = (torch.clamp(torch.log(w), max=0.0) + Mg).float()
    return float(khat), out


def numpy_psis(lw, want_weights):
    new, row = _host_psis(lw.cpu().numpy().astype(np.float64), 0, want_weights)
    return float(row[0]), new


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
        raise SystemExit('psis_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    lw, x = columns(1, N, 31)
    row = group_stats(lw, x, 1, N)[0].cpu().numpy()
    post = posterior(lw, x, row)
    k = post.pareto_k()
    kt, wt = torch_psis(lw, True)
    kn, wn = numpy_psis(lw, True)
    sm = post.psis()
    assert abs(k - kn) <= 1e-9 and abs(kt - kn) <= 1e-9, (k, kt, kn)
    assert float((sm._log_weights - wt).abs().max()) <= 1e-5 and np.abs(sm._log_weights.cpu().numpy() - wn).max() <= 1e-5
    fit = dict(khat=k, tail=sm.fit.tail, grid=sm.fit.grid, ess_before=sm.fit.ess_before, ess_after=sm.fit.ess_after)
    records.append(record('pareto_k(), first call on an object: sort by log-weight, fit', 1, N, lambda: posterior(lw, x, row).pareto_k(),
                          lambda: torch_psis(lw, False), lambda: numpy_psis(lw, False), extra=dict(fit=fit)))
    records.append(record('pareto_k(), the object already sorted by log-weight (the other routes sort again: they keep nothing)', 1, N,
                          lambda: post.pareto_k(), lambda: torch_psis(lw, False), lambda: numpy_psis(lw, False)))
    records.append(record('psis(), first call on an object: sort by log-weight, fit, smoothing, statistics', 1, N,
                          lambda: posterior(lw, x, row).psis(), lambda: torch_psis(lw, True), lambda: numpy_psis(lw, True)))
    records.append(record('psis(), the object already sorted by log-weight', 1, N, lambda: post.psis(), lambda: torch_psis(lw, True),
                          lambda: numpy_psis(lw, True)))
    ls, index, counted = post._device_lw_sorted()
    records.append(alone('is_psis_groups alone, diagnostic only', 1, N, lambda: ops.is_psis_groups(ls, index, counted, N, None, 0, False)))
    records.append(alone('is_psis_groups alone, with the smoothed weights', 1, N,
                         lambda: ops.is_psis_groups(ls, index, counted, N, None, 0, True)))
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
    parts = lw.split(Nb)
    fast = pyprob_amd.pareto_k_batch(posts)
    assert np.array_equal(fast, np.array([p.pareto_k() for p in posts]))
    assert np.abs(fast - np.array([numpy_psis(part, False)[0] for part in parts])).max() <= 1e-9
    both = pyprob_amd.psis_batch(posts)
    assert all(torch.equal(a._log_weights, p.psis()._log_weights) for a, p in zip(both, posts))

    def fresh(call):
        def run():
            for p in posts:
                p.__dict__.pop('_dev_lw_sorted', None)
            return [call(p) for p in posts]
        return run
    loop = event_timed(fresh(lambda p: p.pareto_k()))
    records.append(record('pareto_k_batch(posts)', M, Nb, lambda: pyprob_amd.pareto_k_batch(posts),
                          lambda: [torch_psis(part, False) for part in parts], lambda: [numpy_psis(part, False) for part in parts],
                          extra=dict(loop_of_first_pareto_k_calls=loop, khat_min=float(fast.min()), khat_max=float(fast.max()))))
    records[-1]['loop_over_ours'] = round(loop['median_ms'] / records[-1]['ours']['median_ms'], 2)
    loop = event_timed(fresh(lambda p: p.psis()))
    records.append(record('psis_batch(posts)', M, Nb, lambda: pyprob_amd.psis_batch(posts),
                          lambda: [torch_psis(part, True) for part in parts], lambda: [numpy_psis(part, True) for part in parts],
                          extra=dict(loop_of_first_psis_calls=loop)))
    records[-1]['loop_over_ours'] = round(loop['median_ms'] / records[-1]['ours']['median_ms'], 2)
    _, ls, index, counted = ops.is_sort_groups(lw, lw, Nb, stats)
    records.append(alone('is_sort_groups alone, keyed on the log-weights', M, Nb, lambda: ops.is_sort_groups(lw, lw, Nb, stats)))
    records.append(alone('torch.sort of the [M, N] log-weights alone', M, Nb, lambda: torch.sort(lw.view(M, Nb), dim=1, stable=True)))
    records.append(alone('is_psis_groups alone, diagnostic only', M, Nb, lambda: ops.is_psis_groups(ls, index, counted, Nb, stats, 0, False)))
    records.append(alone('is_psis_groups alone, with the smoothed weights', M, Nb,
                         lambda: ops.is_psis_groups(ls, index, counted, Nb, stats, 0, True)))
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup',
               inputs='synthetic log-weights -0.5 log U (a Pareto tail of shape 0.5) and normal values, attached to Empiricals as a '
                      'lock-step call attaches them',
               ours='Empirical.pareto_k / psis / pyprob_amd.pareto_k_batch / psis_batch: pp_is_sort_groups keyed on the log-weights, '
                    'pp_is_psis_groups, one copy of the rows of out (psis: pp_is_stats of every smoothed group)',
               torch_route='torch.sort(stable) + the m x n float64 log1p table as one broadcast, one group at a time',
               cpu_numpy_route='cpu() of the log-weights, the host route of Empirical.psis in numpy, one group at a time',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
