"""Device time of pp_obs_draw at n = 16384 rows of k = 784 values (a chunk of 28x28 images), Normal, for a full [n, k] mean and
for one shared image - hipEvent-timed medians with the launch included, like the sampler table of tools/prior_is_bench.py - next to
the only other device route to the same block: pp_prior_draw over the flattened n * k elements, with the [n, k] materialisation of
the parameter it needs counted in. Then traces/s of one VectorisedOnlineDataset chunk of a lock-step captcha program (28x28) against
OnlineDataset on the same program (one forward() per trace, 256 traces). Writes one JSON line to profiles/obs_draw_bench.json
(--out PATH for another place).

    python tools/obs_draw_bench.py [--reps 20]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import distributions as D  # noqa: E402
from pyprob_amd.model import Model  # noqa: E402

N, K = 16384, 784
DEV = 'cuda:0'

_yy, _xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing='ij')
PATTERNS = torch.stack([0.5 + 0.4 * torch.sin((_yy * (1 + k % 3) + _xx * (1 + k // 3)) * 0.35) for k in range(6)])


class Captcha(Model):
    """Lock-step safe: d ~ Categorical(6), gain ~ Normal(1, 0.1), the image is the d-th pattern times the gain plus pixel noise."""

    def forward(self):
        d = pyprob_amd.sample(D.Categorical([1 / 6.] * 6))
        gain = pyprob_amd.sample(D.Normal(1.0, 0.1))
        mean = PATTERNS.to(d.device)[d.long()] * gain.reshape(-1, 1, 1)
        pyprob_amd.observe(D.Normal(mean, 0.1), name='img')
        return d


def event_ms(fn, reps):
    fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for r in range(reps):
        e0.record()
        fn(r + 1)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'obs_draw_bench.json'))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from pyprob_amd.ops import ops
    rec = {'device': torch.cuda.get_device_name(0), 'rows': N, 'k': K, 'block_bytes': N * K * 4}
    block = torch.rand(N, K, device=DEV)
    image = torch.rand(1, K, device=DEV)
    sigma = torch.tensor([0.1], device=DEV)
    for name, mean in (('block_mean', block), ('shared_image', image)):
        ms = event_ms(lambda r: ops.obs_draw(0, mean, sigma, N, K, r, 0, 0x4000), a.reps)
        rec['obs_draw_ms_' + name] = ms
        rec['obs_draw_write_GBps_' + name] = round(N * K * 4 / (ms * 1e-3) / 1e9, 1)

        def flattened(r):       # the parent's device route: one value per "particle" over n * k, parameters as n * k vectors
            return ops.prior_draw(0, mean.expand(N, K).reshape(-1), sigma, N * K, r, 0, 0x4000).reshape(N, K)
        rec['prior_draw_flattened_ms_' + name] = event_ms(flattened, a.reps)
    # the same values where the two routes overlap: element 0 of every row is pp_prior_draw's value of the row
    assert torch.equal(ops.obs_draw(0, block[:, :1].contiguous(), sigma, N, K, 3, 0, 0x4000)[:, 0],
                       ops.prior_draw(0, block[:, 0].contiguous(), sigma, N, 3, 0, 0x4000))

    from pyprob_amd.dataset import VectorisedOnlineDataset
    from pyprob_amd.nn import OnlineDataset
    model = Captcha('captcha-like, lock step')
    ds = VectorisedOnlineDataset(model, ['img'], chunk_traces=N, device=DEV)      # (first chunk: warm-up)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ds.refresh()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    rec['vectorised_chunk_traces'] = N
    rec['vectorised_chunk_ms'] = round(statistics.median(ts) * 1e3, 3)
    rec['vectorised_traces_per_sec'] = round(N / statistics.median(ts), 1)
    online = OnlineDataset(model=model)
    online[0]
    t0 = time.perf_counter()
    for i in range(256):
        online[i]
    dt = time.perf_counter() - t0
    rec['per_trace_traces'] = 256
    rec['per_trace_traces_per_sec'] = round(256 / dt, 1)
    assert all(math.isfinite(v) for v in rec.values() if isinstance(v, float))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
