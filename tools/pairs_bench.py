"""Time of Empirical.compare_joint and pyprob_amd.compare_joint_batch (csrc/is_pairs.hip) next to other routes to the same numbers on
the same commit: the definitions as chunked torch float64 on the device, cpu() + the chunked float64 numpy route
(empirical_host._host_twosample_joint) where that finishes in reasonable time, and the loop of compare_joint calls. The posteriors are
built from synthetic columns the way a lock-step call leaves them. Cases: compare_joint at N = 10^4 and 10^5 particles per side for
J = 2 and 8, ONCE at 10^6 (--big 0 leaves it out), num_samples = 10^4 out of the largest N, compare_joint_batch at M = 256 pairs of 10^4
particles. Every figure but the single ones is the median of --reps device-event timings of ONE call after --warmup calls. The operator
alone (operand passes, both pair kernels and the combine) is reported with the pairs it evaluates per second and that as a fraction of
the v_exp_f32 rate (16 per clock and CU: one per pair of the Gaussian sum) - a LOWER bound for the Gaussian kernel, which shares the time
with the distance kernel. Writes one JSON document to profiles/compare_joint_bench.json (--out PATH).

    python tools/pairs_bench.py [--reps 20] [--warmup 3] [--big 1000000] [--batch 256 10000]"""
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
from pyprob_amd.empirical_host import _host_twosample_joint  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

DEV = 'cuda'
NAMES = ('k_aa', 'k_bb', 'k_ab', 'd_aa', 'd_bb', 'd_ab')
CUS, CLOCK_HZ = 256, 2.4e9          # MI355X: the v_exp_f32 rate DESIGN.md 4.3 uses is 16 per clock and CU


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--big', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'compare_joint_bench.json'))
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
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), reps=len(ts))


def posteriors(M, N, J, seed, shift):
    """The M groups of one batched call over J synthetic columns: every member holds the call's tensors (`_batch`) and its own
    slices of the statement log."""
    from pyprob_amd.is_engine import DistRunner
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    cols = [torch.randn(M * N, device=DEV, generator=g) + shift * (j + 1) for j in range(J)]
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    stats = torch.stack([ops.is_stats(lw[k * N:(k + 1) * N], cols[0][k * N:(k + 1) * N], scratch)[:6] for k in range(M)]).contiguous()
    rows, log, posts = stats.cpu().numpy(), [{'x%d' % j: (c, 0)} for j, c in enumerate(cols)], []
    for k in range(M):
        p = Empirical.from_device(cols[0][k * N:(k + 1) * N], lw[k * N:(k + 1) * N], DistRunner._stats_dict(rows[k]))
        p.statement_log = [{'x%d' % j: (c[k * N:(k + 1) * N], 0)} for j, c in enumerate(cols)]
        p._statement_rows_raw = [{'x%d' % j: None} for j in range(J)]
        p._batch, p._batch_log = (cols[0], lw, stats, k, N), log
        posts.append(p)
    return lw, cols, posts


def torch_pairs(lw_a, cols_a, lw_b, cols_b, center, scale, h, chunk=2048):
    """The six sums of ONE pair of particle sets as chunked torch float64 on the device."""
    c, s = torch.from_numpy(center).to(DEV), torch.from_numpy(scale).to(DEV)
    side = lambda lw, cols: ((torch.stack(cols, 1).double() - c) / s, torch.softmax(lw.double(), 0))      # noqa: E731
    (za, wa), (zb, wb) = side(lw_a, cols_a), side(lw_b, cols_b)
    out = []
    for (zr, wr), (zc, wc) in (((za, wa), (za, wa)), ((zb, wb), (zb, wb)), ((za, wa), (zb, wb))):
        k = d = torch.zeros((), dtype=torch.float64, device=DEV)
        for i in range(0, len(wr), chunk):
            dist = torch.cdist(zr[i:i + chunk], zc)
            k = k + (wr[i:i + chunk] @ torch.exp(dist * dist * (-0.5 / (h * h)))) @ wc
            d = d + (wr[i:i + chunk] @ dist) @ wc
        out.append((k, d))
    return torch.stack([o[0] for o in out] + [o[1] for o in out]).cpu().numpy()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def operator_alone(a, b, r, N, J):
    sides = [(p._all_lw(), p._joint_columns(None)[1], N, p._group_stats_row()) for p in (a, b)]
    as_dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(DEV)      # noqa: E731
    c, i, h = as_dev(r.center[None]), as_dev(1.0 / r.scale[None]), as_dev([r.bandwidth])
    reps = 1 if N >= 10 ** 6 else None
    op = event_timed(lambda: ops.is_pairs_groups(*sides[0], *sides[1], c, i, h), reps=reps, warmup=0 if reps else None)
    pairs = 2.0 * N * N          # aa and bb over the upper triangle, ab in full
    rate = pairs / (op['median_ms'] * 1e-3)
    return dict(op, pairs=pairs, pairs_per_s=float('%.4g' % rate), fraction_of_v_exp_rate=round(rate / (16 * CUS * CLOCK_HZ), 4),
                fraction_of_fp32_mfma_peak=round(rate * 2 * 10 / 157.3e12, 4) if J == 8 else None)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('pairs_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    for N in [10 ** 4, 10 ** 5] + ([args.big] if args.big else []):
        for J in (2, 8):
            (lw_a, cols_a, (a,)), (lw_b, cols_b, (b,)) = posteriors(1, N, J, 21, 0.0), posteriors(1, N, J, 22, 0.1)
            big = N >= 10 ** 6
            r = a.compare_joint(b)
            rec = dict(case='compare_joint', N=[N, N], J=J, mmd2=r.mmd2, energy=r.energy,
                       ours=event_timed(lambda: a.compare_joint(b), reps=1 if big else None, warmup=0 if big else None),
                       operator_alone=operator_alone(a, b, r, N, J))
            if N <= 10 ** 5:
                ref = torch_pairs(lw_a, cols_a, lw_b, cols_b, r.center, r.scale, r.bandwidth)
                assert np.allclose([getattr(r, k) for k in NAMES], ref, rtol=1e-4), (vars(r), ref)
                rec['torch_float64'] = event_timed(lambda: torch_pairs(lw_a, cols_a, lw_b, cols_b, r.center, r.scale, r.bandwidth),
                                                   reps=3, warmup=1)
            if N <= 10 ** 4:
                rec['cpu_numpy'] = event_timed(lambda: _host_twosample_joint(host(lw_a), np.stack([host(c) for c in cols_a], 1), host(lw_b),
                                                                             np.stack([host(c) for c in cols_b], 1)), reps=1, warmup=0)
            if big and J == 2:
                rec['ours_num_samples_10000'] = event_timed(lambda: a.compare_joint(b, num_samples=10 ** 4, seed=1))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    M, Nb = args.batch
    (_, _, pa), (_, _, pb) = posteriors(M, Nb, 2, 7, 0.0), posteriors(M, Nb, 2, 8, 0.1)
    fast, loop = pyprob_amd.compare_joint_batch(pa, pb), [p.compare_joint(q) for p, q in zip(pa, pb)]
    assert all(f.mmd2 == l.mmd2 and f.energy == l.energy for f, l in zip(fast, loop))
    records.append(dict(case='compare_joint_batch', M=M, N=[Nb, Nb], J=2, ours=event_timed(lambda: pyprob_amd.compare_joint_batch(pa, pb), reps=5),
                        loop_of_compare_joint=event_timed(lambda: [p.compare_joint(q) for p, q in zip(pa, pb)], reps=3, warmup=1)))
    print(json.dumps(records[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, copies, host arithmetic), medians of `reps` after --warmup; the cases at '
                      '10^6 particles and the numpy route are timed once, the torch route 3 times after 1',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
