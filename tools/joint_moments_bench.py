"""Time of Empirical.joint and pyprob_amd.joint_batch (csrc/is_moments.hip) next to the two other routes to the same numbers on the
same commit: torch in float64 on the device (w = exp(lw.double() - max), X.double(), X^T (w X)) and the host (cpu() + numpy).
The posteriors are built from synthetic columns the way a lock-step call leaves them (Empirical.from_device + statement_log; for the
batch the call's whole tensors and its [M, 6] statistics): joint() at N = 10^6 particles with J = 2, 4, 16 latents, joint_batch at
M = 256 posteriors of 10^4 particles with J = 3. Every figure is the median of --reps device-event timings of ONE call after
--warmup calls (the event pair spans the launch, the device-to-host copy and the host arithmetic of the call); the kernel alone
(the operator, 20 calls per event pair) is reported with its effective bytes per second against (J + 1) 4 bytes per particle.
Writes one JSON document to profiles/joint_moments_bench.json (--out PATH for another place).

    python tools/joint_moments_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'joint_moments_bench.json'))
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


def columns(M, N, J, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lw = torch.randn(M * N, device=DEV, generator=g) * 2.0
    cols = [torch.randn(M * N, device=DEV, generator=g) * (1.0 + 0.25 * j) + j for j in range(J)]
    return lw, cols


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, cols, stats_row):
    from pyprob_amd.is_engine import DistRunner
    emp = Empirical.from_device(cols[-1], lw, DistRunner._stats_dict(stats_row))
    emp._all_values, emp._all_log_weights = cols[-1], lw
    emp.statement_log = [{'x%d' % j: (c, j)} for j, c in enumerate(cols)]
    emp._statement_rows_raw, emp.statement_names = [{'x%d' % j: None} for j in range(len(cols))], {}
    return emp


def torch_route(lw, cols, M, N):
    """The moments about zero in float64 on the device with torch operators, one device-to-host copy."""
    l = lw.view(M, N).double()
    w = torch.exp(l - l.max(1, keepdim=True)[0])
    X = torch.stack(cols, 1).view(M, N, len(cols)).double()
    wX = w.unsqueeze(2) * X
    out = torch.cat([w.sum(1, keepdim=True), (w * w).sum(1, keepdim=True), wX.sum(1), torch.bmm(X.transpose(1, 2), wX).flatten(1)], 1)
    return out.cpu().numpy()


def host_route(lw, cols, M, N):
    l = lw.cpu().numpy().reshape(M, N).astype(np.float64)
    X = np.stack([c.cpu().numpy() for c in cols], 1).reshape(M, N, len(cols)).astype(np.float64)
    w = np.exp(l - l.max(1, keepdims=True))
    wX = w[:, :, None] * X
    return w.sum(1), (w * w).sum(1), wX.sum(1), np.matmul(X.transpose(0, 2, 1), wX)


def record(case, M, N, J, ours, lw, cols, stats, extra=None):
    per = (J + 1) * 4
    kernel = event_timed(lambda: ops.is_moments_groups(lw, cols, N, stats), per=20)
    rec = dict(case=case, M=M, N=N, J=J, ours=event_timed(ours), torch_float64=event_timed(lambda: torch_route(lw, cols, M, N)),
               host_numpy=event_timed(lambda: host_route(lw, cols, M, N)),
               kernel_alone=dict(kernel, stats_given=stats is not None, bytes_per_particle=per,
                                 effective_GB_per_s=round(M * N * per / (kernel['median_ms'] * 1e-3) / 1e9, 1),
                                 timing='device events around 20 calls of the operator (each allocates its output and workspace)'))
    rec['torch_over_ours'] = round(rec['torch_float64']['median_ms'] / rec['ours']['median_ms'], 2)
    rec['host_over_ours'] = round(rec['host_numpy']['median_ms'] / rec['ours']['median_ms'], 2)
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit('joint_moments_bench: needs a ROCm device (nothing is measured without one)')
    records = []
    N = args.N
    for J in (2, 4, 16):
        lw, cols = columns(1, N, J, 10 + J)
        post = posterior(lw, cols, group_stats(lw, cols[-1], 1, N)[0].cpu().numpy())
        j = post.joint()
        ref = host_route(lw, cols, 1, N)
        mean = ref[2][0] / ref[0][0]
        assert np.allclose(j.mean, mean, rtol=1e-9, atol=1e-12) and np.allclose(j.cov, ref[3][0] / ref[0][0] - np.outer(mean, mean), rtol=1e-6)
        records.append(record('joint()', 1, N, J, post.joint, lw, cols, None))
    M, Nb = args.batch
    J = 3
    lw, cols = columns(M, Nb, J, 7)
    stats = group_stats(lw, cols[-1], M, Nb)
    host_stats = stats.cpu().numpy()
    posts = []
    whole_log = [{'x%d' % j: (c, j)} for j, c in enumerate(cols)]
    for g in range(M):
        p = posterior(lw[g * Nb:(g + 1) * Nb], [c[g * Nb:(g + 1) * Nb] for c in cols], host_stats[g])
        p._batch, p._batch_log = (cols[-1], lw, stats, g, Nb), whole_log
        posts.append(p)
    fast = pyprob_amd.joint_batch(posts)
    loop = [p.joint() for p in posts]
    assert all(np.array_equal(f.cov, l.cov) and np.array_equal(f.mean, l.mean) for f, l in zip(fast, loop))
    loop_time = event_timed(lambda: [p.joint() for p in posts])
    records.append(record('joint_batch(posts)', M, Nb, J, lambda: pyprob_amd.joint_batch(posts), lw, cols, stats,
                          extra=dict(loop_of_joint=loop_time)))
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               timing='device events around ONE call (launches, device-to-host copy, host arithmetic), medians of --reps after --warmup',
               inputs='synthetic columns and log-weights (normal), attached to Empiricals as a lock-step call attaches them',
               ours='Empirical.joint / pyprob_amd.joint_batch: pp_is_moments_groups (fp64 sums about a pivot) + one copy',
               torch_float64='torch on the device: exp(lw.double() - max), stack + double of the columns, bmm; raw moments about zero; one copy',
               host_numpy='cpu() of the log-weights and every column, numpy float64 matmul', records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
