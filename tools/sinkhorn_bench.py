"""Time of the Sinkhorn operator (csrc/is_sinkhorn.hip), next to two other routes to the same numbers on the same machine, neither of
which is the code under test:
    torch   a dense log-domain Sinkhorn in torch float64 on the device (the three n x n cost matrices stored), the same iteration count;
    cpu     cpu() of the log-weights and columns and the float64 numpy route (empirical_host._host_sinkhorn), ONE iteration.
Cases: pp_is_sinkhorn_groups at --N against --N particles for J = 2 and 8, --iters iterations at tol = 0 (the time per iteration) and
to tol = 1e-3 (the iterations taken); one run at --big against --big particles, timed ONCE, with the size of ONE dense float64 cost
matrix at that shape and whether the device could allocate it (the dense route needs three and its temporaries; it is not run
there). An iteration visits 4 N^2 pairs (two half-steps of problem (a, b), one each of (a, a) and (b, b)); the
document states the pairs per second and the share of the v_exp_f32 rate and of the fp32 MFMA peak (--exp-rate and --mfma-peak, per
second for the whole device: state the figures of the part the run is on) that the pair count implies: 17 / 16 exponentials and 2 K
matrix flops per pair. Every other figure is the median of --reps device-event timings of ONE call after --warmup calls. Writes one
JSON document to profiles/sinkhorn_bench.json (--out PATH).

    python tools/sinkhorn_bench.py [--reps 20] [--warmup 3] [--N 10000] [--big 100000]"""
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

from pyprob_amd.empirical_host import _host_sinkhorn  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--N', type=int, default=10 ** 4)
ap.add_argument('--big', type=int, default=10 ** 5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--exp-rate', type=float, default=256 * 4 * 16 * 2.4e9 / 4, help='v_exp_f32 per second of the device')
ap.add_argument('--mfma-peak', type=float, default=256 * 256 * 2.4e9, help='fp32 MFMA flops per second of the device')
ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sinkhorn_bench.json'))
args = ap.parse_args()
DEV = 'cuda'


def event_timed(fn, reps=None, warmup=None):
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    ts = []
    for _ in range(args.reps if reps is None else reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def sides(n, J, seed):
    """Two unit Gaussians half a standard deviation apart, log-weights within 3 of their maximum; centre 0, scale 1."""
    rng = np.random.default_rng(seed)
    out = []
    for shift in (0.0, 0.5 / np.sqrt(J)):
        x = (rng.standard_normal((n, J)) + shift).astype(np.float32)
        out.append(((-3.0 * rng.random(n)).astype(np.float32), x))
    return out


def on_device(lw, x):
    return torch.from_numpy(lw).to(DEV), [torch.from_numpy(np.ascontiguousarray(x[:, j])).to(DEV) for j in range(x.shape[1])]


def operator(a, b, J, eps, tol, iters):
    one = lambda v: torch.full((1, J), v, dtype=torch.float64, device=DEV)      # noqa: E731
    return ops.is_sinkhorn_groups(a[0], a[1], a[0].numel(), None, b[0], b[1], b[0].numel(), None, one(0.0), one(1.0),
                                  torch.tensor([eps], dtype=torch.float64, device=DEV), tol, iters, 8)


def torch_dense(a, b, eps, iters):
    za, zb = torch.stack(a[1], 1).double(), torch.stack(b[1], 1).double()
    la, lb = torch.log_softmax(a[0].double(), 0), torch.log_softmax(b[0].double(), 0)
    soft = lambda lw, pot, C: -eps * torch.logsumexp(lw[:, None] + (pot[:, None] - C) / eps, 0)      # noqa: E731
    C = torch.cdist(za, zb) ** 2 / 2
    f, g = torch.zeros_like(la), torch.zeros_like(lb)
    for _ in range(iters):
        g = soft(la, f, C)
        f = soft(lb, g, C.T)
    out = [(la.exp() * f).sum() + (lb.exp() * g).sum()]
    for l, z in ((la, za), (lb, zb)):
        C, p = torch.cdist(z, z) ** 2 / 2, torch.zeros_like(l)
        for _ in range(iters):
            p = (p + soft(l, p, C)) / 2
        out.append(2 * (l.exp() * p).sum())
    return out


doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, N=args.N, iters=args.iters, cases=[])
for J in (2, 8):
    (lw_a, x_a), (lw_b, x_b) = sides(args.N, J, J)
    a, b, eps, K = on_device(lw_a, x_a), on_device(lw_b, x_b), 0.05 * J, (J + 3) & ~1
    row = dict(J=J, epsilon=eps, operator=event_timed(lambda: operator(a, b, J, eps, 0.0, args.iters)))
    sec, pairs = row['operator']['median_ms'] * 1e-3 / args.iters, 4.0 * args.N * args.N
    row.update(ms_per_iteration=sec * 1e3, pairs_per_s=pairs / sec, share_of_exp_rate=pairs * 17 / 16 / sec / args.exp_rate,
               share_of_mfma_peak=pairs * 2 * K / sec / args.mfma_peak)
    done = operator(a, b, J, eps, 1e-3, 1000)[0][0].cpu().numpy()
    row['to_tol_1e-3'] = dict(n_iter=done[3:6].tolist(), status=done[11], divergence=done[0] - (done[1] + done[2]) / 2,
                              **event_timed(lambda: operator(a, b, J, eps, 1e-3, 1000), reps=5, warmup=1))
    got, want = operator(a, b, J, eps, 0.0, args.iters)[0][0, :3].cpu().numpy(), [float(v) for v in torch_dense(a, b, eps, args.iters)]
    row['costs'], row['torch_costs'] = got.tolist(), want
    row['torch_float64_dense'] = event_timed(lambda: torch_dense(a, b, eps, args.iters), reps=5, warmup=1)
    t0 = time.perf_counter()
    _host_sinkhorn(lw_a, x_a, lw_b, x_b, np.zeros(J), np.ones(J), eps, 0.0, 1)
    row['cpu_numpy_ms_one_iteration'] = (time.perf_counter() - t0) * 1e3
    doc['cases'].append(row)
    print(json.dumps(row), flush=True)

J, n, iters = 8, args.big, 5
(lw_a, x_a), (lw_b, x_b) = sides(n, J, 99)
a, b = on_device(lw_a, x_a), on_device(lw_b, x_b)
torch.cuda.synchronize()
big = dict(N=n, J=J, iterations=iters, timed='once', operator_ms=event_timed(lambda: operator(a, b, J, 0.05 * J, 0.0, iters), reps=1, warmup=0),
           dense_float64_matrix_bytes=8.0 * n * n)
try:
    torch.empty((n, n), dtype=torch.float64, device=DEV)
    big['dense_route'] = 'the matrix could be allocated on this device'
except RuntimeError as err:
    big['dense_route'] = 'cannot allocate its matrix: %s' % str(err).splitlines()[0][:120]
big['ms_per_iteration'] = big['operator_ms']['median_ms'] / iters
doc['big'] = big
print(json.dumps(big), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as f:
    json.dump(doc, f, indent=1)
