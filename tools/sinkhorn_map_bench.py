"""Time of the transport-map operator (csrc/is_sinkhorn_map.hip) ALONE, next to the dense formulation of the same numbers in torch float64
on the same device (the n x n plan stored; not the code under test). Cases: pp_is_sinkhorn_map_groups, both directions, at --N against
--N particles for J = 2 and 8, and ONE run at --big against --big particles (J = 8), timed once, where the dense route is not run (one
float64 matrix at that shape is 8 n^2 bytes). The potentials are random numbers of a few epsilon: the operator does not care whether
they are converged. A call visits 2 N^2 pairs (two directions); the document states the pairs per second and the share of the
v_exp_f32 rate (one exponential per pair) and of the fp32 MFMA peak (--exp-rate and --mfma-peak, per second for the whole device: state
the figures of the part the run is on) that the pair count implies: 2 K flops per pair in the first product and 64 in the second,
whose 32 result rows are issued whether used or not ("issued"), of which 2 (J + 1) are the map's and the normaliser's ("useful").
Every other figure is the median of --reps device-event timings of ONE call after --warmup calls. Writes one JSON document to
profiles/sinkhorn_map_bench.json (--out PATH).

    python tools/sinkhorn_map_bench.py [--reps 20] [--warmup 3] [--N 10000] [--big 100000]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyprob_amd import lib as L  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--N', type=int, default=10 ** 4)
ap.add_argument('--big', type=int, default=10 ** 5)
ap.add_argument('--exp-rate', type=float, default=256 * 4 * 16 * 2.4e9 / 4, help='v_exp_f32 per second of the device')
ap.add_argument('--mfma-peak', type=float, default=256 * 256 * 2.4e9, help='fp32 MFMA flops per second of the device')
ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sinkhorn_map_bench.json'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'the benchmark needs the device: nothing here is measured without it'
DEV = 'cuda'


def event_timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def sides(n, J, eps, seed):
    """Two unit Gaussians half a standard deviation apart, log-weights within 3 of their maximum, potentials within 3 epsilon; centre 0,
    scale 1. Per side (lw, columns, potential [1, n]) on the device."""
    rng = np.random.default_rng(seed)
    out = []
    for shift in (0.0, 0.5 / np.sqrt(J)):
        x = (rng.standard_normal((n, J)) + shift).astype(np.float32)
        out.append((torch.from_numpy((-3.0 * rng.random(n)).astype(np.float32)).to(DEV),
                    [torch.from_numpy(np.ascontiguousarray(x[:, j])).to(DEV) for j in range(J)],
                    torch.from_numpy(eps * rng.uniform(-3.0, 3.0, (1, n))).to(DEV)))
    return out


def operator(a, b, J, eps):
    one = lambda v: torch.full((1, J), v, dtype=torch.float64, device=DEV)      # noqa: E731
    return ops.is_sinkhorn_map_groups(a[0], a[1], a[0].numel(), None, b[0], b[1], b[0].numel(), None, one(0.0), one(1.0),
                                      torch.tensor([eps], dtype=torch.float64, device=DEV), a[2], b[2], True, True)


def torch_dense(a, b, eps):
    za, zb = torch.stack(a[1], 1).double(), torch.stack(b[1], 1).double()
    la, lb = torch.log_softmax(a[0].double(), 0), torch.log_softmax(b[0].double(), 0)
    C = torch.cdist(za, zb) ** 2 / 2
    out = []
    for E, z, pot in ((lb[None, :] + (b[2] - C) / eps, zb, a[2][0]), (la[None, :] + (a[2] - C.T) / eps, za, b[2][0])):
        out += [torch.softmax(E, 1) @ z, pot / eps + torch.logsumexp(E, 1)]
    return out[0], out[2], out[1], out[3]


def shares(n, J, ms):
    pairs, K, sec = 2.0 * n * n, (J + 3) & ~1, ms * 1e-3
    return dict(pairs_per_s=pairs / sec, share_of_exp_rate=pairs / sec / args.exp_rate,
                share_of_mfma_peak_issued=pairs * (2 * K + 64) / sec / args.mfma_peak,
                share_of_mfma_peak_useful=pairs * (2 * K + 2 * (J + 1)) / sec / args.mfma_peak)


doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, N=args.N, cases=[])
for J in (2, 8):
    eps = 0.05 * J
    a, b = sides(args.N, J, eps, J)
    row = dict(J=J, epsilon=eps, operator=event_timed(lambda: operator(a, b, J, eps), args.reps, args.warmup))
    row.update(shares(args.N, J, row['operator']['median_ms']))
    row['workspace_bytes'] = L.load().pp_is_sinkhorn_map_workspace_bytes(1, args.N, args.N, J)
    got, want = operator(a, b, J, eps), torch_dense(a, b, eps)
    row['max_abs_difference_from_torch_float64'] = [float((g[0] - w).abs().max()) for g, w in zip(got, want)]
    row['torch_float64_dense'] = event_timed(lambda: torch_dense(a, b, eps), 5, 1)
    doc['cases'].append(row)
    print(json.dumps(row), flush=True)

J, n = 8, args.big
a, b = sides(n, J, 0.05 * J, 99)
operator(a, b, J, 0.05 * J)      # (one untimed call: the first launch of a shape loads code and allocates the workspace)
torch.cuda.synchronize()
big = dict(N=n, J=J, timed='once, after one untimed call', operator=event_timed(lambda: operator(a, b, J, 0.05 * J), 1, 0),
           workspace_bytes=L.load().pp_is_sinkhorn_map_workspace_bytes(1, n, n, J), dense_float64_matrix_bytes=8.0 * n * n)
big.update(shares(n, J, big['operator']['median_ms']))
doc['big'] = big
print(json.dumps(big), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as f:
    json.dump(doc, f, indent=1)
