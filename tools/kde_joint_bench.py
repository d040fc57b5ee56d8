"""Time of the joint kernel density and of mean shift (csrc/is_kde_joint.hip) at the operator, next to two other routes to the same
numbers on the same machine, neither of which is the code under test:
    torch   the same definition in chunked torch float64 on the device (a [chunk, N] block of exponents at a time);
    cpu     cpu() of the log-weights and columns and the float64 numpy route (empirical_host), on --cpu-queries points, scaled to Q.
Cases: pp_is_kde_joint_groups at --N particles and --Q points for J = 2, 4, 8, with and without the mean; pp_is_meanshift_groups from
256 seeds at --N and at 10^4 particles, J = 2 (the iterations taken and the time per iteration). For the operator the document states
the pairs per second, and the share of the v_exp_f32 rate and of the fp32 MFMA peak (--exp-rate and --mfma-peak, per second for
the whole device: state the figures of the part the run is on) that the pair count implies: 17 / 16 exponentials per pair, and 2 K
(density) or 2 K + 64 (with the mean) matrix flops per pair, the padding rows of the second product included. Every figure is the median of
--reps device-event timings of ONE call after --warmup calls. Writes one JSON document to profiles/kde_joint_bench.json (--out PATH).

    python tools/kde_joint_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--Q 4096]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyprob_amd.empirical_host import _host_kde_joint, _host_meanshift  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--N', type=int, default=10 ** 6)
ap.add_argument('--Q', type=int, default=4096)
ap.add_argument('--cpu-queries', type=int, default=8)
ap.add_argument('--exp-rate', type=float, default=256 * 4 * 16 * 2.4e9 / 4, help='v_exp_f32 per second of the device')
ap.add_argument('--mfma-peak', type=float, default=256 * 256 * 2.4e9, help='fp32 MFMA flops per second of the device')
ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'kde_joint_bench.json'))
args = ap.parse_args()
DEV = 'cuda'


def event_timed(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def particles(n, J, seed):
    """Two unit Gaussian modes 6 apart in every coordinate, log-weights within 3 of their maximum; standardised by their moments."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, J)) + 3.0 * np.where(np.arange(n) % 2, 1.0, -1.0)[:, None]).astype(np.float32)
    lw = (-3.0 * rng.random(n)).astype(np.float32)
    return lw, x, x.mean(0, dtype=np.float64), x.std(0, dtype=np.float64)


def torch_route(lw, cols, center, inv_scale, h, zq, want_mean, chunk=256):
    z = (torch.stack(cols, 1).double() - center) * inv_scale
    logw = torch.log_softmax(lw.double(), 0)
    out, means = [], []
    for a in range(0, zq.shape[0], chunk):
        e = logw[None, :] - torch.cdist(zq[a:a + chunk], z) ** 2 * (0.5 / (h * h))
        m = e.max(1).values
        p = torch.exp(e - m[:, None])
        S = p.sum(1)
        out.append(m + torch.log(S))
        if want_mean:
            means.append(p @ z / S[:, None])
    return torch.cat(out), (torch.cat(means) if want_mean else None)


def on_device(lw, x, center, scale):
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)      # noqa: E731
    return (torch.from_numpy(lw).to(DEV), [torch.from_numpy(np.ascontiguousarray(x[:, j])).to(DEV) for j in range(x.shape[1])],
            as_dev(center[None]), as_dev(1.0 / scale[None]))


doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, N=args.N, Q=args.Q, kde_joint=[], modes=[])
for J in (2, 4, 8):
    lw, x, center, scale = particles(args.N, J, J)
    h = float(args.N ** (-1.0 / (J + 4)))
    d_lw, d_cols, d_center, d_inv = on_device(lw, x, center, scale)
    pts = center + scale * np.random.default_rng(1).standard_normal((args.Q, J)) * 2.0
    d_pts, d_h = torch.from_numpy(pts[None]).to(DEV), torch.tensor([h], dtype=torch.float64, device=DEV)
    K, pairs = (J + 3) & ~1, float(args.N) * args.Q
    row = dict(J=J, bandwidth=h)
    for want_mean in (False, True):
        t = event_timed(lambda: ops.is_kde_joint_groups(d_lw, d_cols, args.N, None, d_center, d_inv, d_h, d_pts, want_mean))
        sec = t['median_ms'] * 1e-3
        t.update(pairs_per_s=pairs / sec, share_of_exp_rate=pairs * 17 / 16 / sec / args.exp_rate,
                 share_of_mfma_peak=pairs * (2 * K + (64 if want_mean else 0)) / sec / args.mfma_peak)
        row['operator_with_mean' if want_mean else 'operator'] = t
    zq = (d_pts[0] - d_center[0]) * d_inv[0]
    row['torch_float64'] = event_timed(lambda: torch_route(d_lw, d_cols, d_center[0], d_inv[0], h, zq, False))
    t0 = time.perf_counter()
    _host_kde_joint(d_lw.cpu().numpy(), torch.stack(d_cols, 1).cpu().numpy(), center, scale, h, pts[:args.cpu_queries])
    row['cpu_numpy_ms_scaled_to_Q'] = (time.perf_counter() - t0) * 1e3 * args.Q / args.cpu_queries
    doc['kde_joint'].append(row)
    print(json.dumps(row), flush=True)

for n in (args.N, 10 ** 4):
    J, S = 2, 256
    lw, x, center, scale = particles(n, J, 9)
    h = float(n ** (-1.0 / (J + 4)))
    d_lw, d_cols, d_center, d_inv = on_device(lw, x, center, scale)
    seeds = (x[:: n // S][:S].astype(np.float64) - center) / scale
    d_seeds, d_h = torch.from_numpy(seeds[None]).to(DEV), torch.tensor([h], dtype=torch.float64, device=DEV)
    call = lambda: ops.is_meanshift_groups(d_lw, d_cols, n, None, d_center, d_inv, d_h, d_seeds, 1e-3, 200, 8)      # noqa: E731
    iters = int(call()[2].max().item())
    row = dict(N=n, J=J, seeds=S, bandwidth=h, iterations=iters, operator=event_timed(call))
    row['ms_per_iteration'] = row['operator']['median_ms'] / (iters + 1)      # (+ the final density pass)

    def torch_shift():
        zq = d_seeds[0].clone()
        for _ in range(iters):
            zq = torch_route(d_lw, d_cols, d_center[0], d_inv[0], h, zq, True)[1]
        return zq
    row['torch_float64'] = event_timed(torch_shift)
    if n <= 10 ** 4:
        t0 = time.perf_counter()
        _host_meanshift(lw, x, center, scale, h, seeds, 1e-3, 200)
        row['cpu_numpy_ms'] = (time.perf_counter() - t0) * 1e3
    doc['modes'].append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as f:
    json.dump(doc, f, indent=1)
