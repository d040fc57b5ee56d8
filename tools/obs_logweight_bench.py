"""Device time of pp_obs_logweight (the summed log-density of a vector-valued observe, one launch) against the route it replaces
in a lock-step importance-sampling call - distribution.log_prob through torch, a torch sum over the k elements and a Factor
term (PP_VEC_LIKELIHOOD=torch: the parent commit's route) - on the same device tensors, in alternating pairs, hipEvent-timed
with the launch included like tools/mixture_bench.py; and the wall time of one whole lock-step prior-IS call of a captcha-like
program under both routes. Writes one JSON line to profiles/obs_logweight_bench.json (--out PATH for another place).

    python tools/obs_logweight_bench.py [--reps 20]

Shapes: (1) Normal, n = 131072 particles of a 28x28 image, per-particle mean [n, k], scalar stddev; (2) the same with a shared
mean row and a per-particle gain that the program folds into the mean (the multiply is part of both routes); (3) k = 8,
n = 10^6. Achieved GB/s are algorithmic bytes (the parameter block read once, the k observed values, n floats read and
written) over the kernel's time, next to the 6.29 TB/s of a float4 copy on this device. For shapes (1) and (3) the record
also holds the time per launch of 50 launches issued back to back through the C ABI: the kernel without the operator dispatch
that the event-timed single call includes."""
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
from pyprob_amd.state import InferenceEngine  # noqa: E402

DEV = 'cuda:0'
COPY_GBPS = 6290.0
H = W = 28


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def pairs(kernel, route, reps):
    """Alternating (kernel, torch route) timings in ms after one warm-up of each."""
    kernel()
    route()
    torch.cuda.synchronize()
    return [(timed(kernel), timed(route)) for _ in range(reps)]


BURST = 50


def back_to_back_ms(lw, mean, sd, x, k, n):
    """Time per launch of BURST launches issued back to back straight through the C ABI (arguments built once): the kernel
    without the operator dispatch, and with the launch gaps the stream leaves between dependent kernels."""
    from pyprob_amd import lib as L
    lib = L.load()
    arr = (L.pp_obs_operand * 4)()
    arr[0].p, arr[0].row_stride, arr[0].elem_stride = mean.data_ptr(), k, 1
    arr[1].p, arr[1].row_stride, arr[1].elem_stride = sd.data_ptr(), 0, 0
    xo = L.pp_obs_operand()
    xo.p, xo.row_stride, xo.elem_stride = x.data_ptr(), 0, 1
    st = L.stream_ptr()

    def burst():
        for _ in range(BURST):
            L.check(lib.pp_obs_logweight(0, arr, xo, k, 1.0, lw.data_ptr(), None, None, n, n, st), 'pp_obs_logweight')
    burst()
    torch.cuda.synchronize()
    return statistics.median(timed(burst) for _ in range(5)) / BURST


def summary(rec, name, ts, nbytes, b2b_ms=None):
    k_ms, t_ms = statistics.median(t[0] for t in ts), statistics.median(t[1] for t in ts)
    rec[name + '_kernel_ms'] = round(k_ms, 4)
    rec[name + '_torch_route_ms'] = round(t_ms, 4)
    rec[name + '_ratio_of_medians'] = round(t_ms / k_ms, 2)
    rec[name + '_min_pair_ratio'] = round(min(t[1] / t[0] for t in ts), 2)
    rec[name + '_kernel_faster_in_every_pair'] = all(t[0] < t[1] for t in ts)
    rec[name + '_algorithmic_bytes'] = int(nbytes)
    rec[name + '_kernel_GBps'] = round(nbytes / (k_ms * 1e-3) / 1e9, 1)
    rec[name + '_fraction_of_copy_rate'] = round(nbytes / (k_ms * 1e-3) / 1e9 / COPY_GBPS, 3)
    if b2b_ms is not None:
        rec[name + '_kernel_back_to_back_ms'] = round(b2b_ms, 4)
        rec[name + '_kernel_back_to_back_GBps'] = round(nbytes / (b2b_ms * 1e-3) / 1e9, 1)
        rec[name + '_kernel_back_to_back_fraction_of_copy_rate'] = round(nbytes / (b2b_ms * 1e-3) / 1e9 / COPY_GBPS, 3)


def patterns():
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing='ij')
    return torch.stack([0.5 + 0.4 * torch.sin((yy * (1 + c % 3) + xx * (1 + c // 3)) * 0.35) for c in range(6)])


class Captcha(Model):
    def __init__(self):
        super().__init__('captcha-like')
        self.patterns = patterns().to(DEV)

    def forward(self):
        d = pyprob_amd.sample(D.Categorical([1 / 6.] * 6))
        gain = pyprob_amd.sample(D.Normal(1.0, 0.1))
        pyprob_amd.observe(D.Normal(self.patterns[d.long()] * gain.reshape(-1, 1, 1), 0.1), name='img')
        return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'obs_logweight_bench.json'))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from pyprob_amd.ops import ops
    rec = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'copy_rate_GBps': COPY_GBPS, 'back_to_back_burst': BURST}
    gen = torch.Generator(device=DEV).manual_seed(1)
    none4 = [None] * 4

    def torch_route(lw, mean, sd, x, n):      # state._lock_step_likelihood's torch branch
        lp = D.Normal(mean, sd).log_prob(x)
        s = lp.reshape(n, -1).sum(1).contiguous()
        ops.dist_logweight(lw, [2], none4, [0] * 4, [s], [1.0], None, None, n)

    sd = torch.tensor([0.1], device=DEV)
    # (1) per-particle mean [n, k]
    n, k = 131072, H * W
    img = torch.rand(H, W, device=DEV, generator=gen)
    mean = torch.rand(n, H, W, device=DEV, generator=gen)
    lw = torch.zeros(n, device=DEV)
    ts = pairs(lambda: ops.obs_logweight(lw, 0, [mean, sd, None, None], img.reshape(-1), k, 1.0, None, None, n),
               lambda: torch_route(lw, mean, 0.1, img, n), a.reps)
    summary(rec, 'mean_nk_784', ts, 4 * (n * k + k + 2 * n), back_to_back_ms(lw, mean, sd, img.reshape(-1), k, n))
    # (2) shared mean row, per-particle gain folded in by the program
    row, gain = img.reshape(1, H, W), 0.9 + 0.2 * torch.rand(n, 1, 1, device=DEV, generator=gen)
    ts = pairs(lambda: ops.obs_logweight(lw, 0, [row * gain, sd, None, None], img.reshape(-1), k, 1.0, None, None, n),
               lambda: torch_route(lw, row * gain, 0.1, img, n), a.reps)
    summary(rec, 'row_times_gain_784', ts, 4 * (2 * n * k + 2 * k + 3 * n))      # the product is written, then read
    del mean
    # (3) k = 8, n = 10^6
    n, k = 10 ** 6, 8
    x8 = torch.rand(k, device=DEV, generator=gen)
    mean = torch.rand(n, k, device=DEV, generator=gen)
    lw = torch.zeros(n, device=DEV)
    ts = pairs(lambda: ops.obs_logweight(lw, 0, [mean, sd, None, None], x8, k, 1.0, None, None, n),
               lambda: torch_route(lw, mean, 0.1, x8, n), a.reps)
    summary(rec, 'mean_nk_8', ts, 4 * (n * k + k + 2 * n), back_to_back_ms(lw, mean, sd, x8, k, n))
    del mean
    # one whole lock-step prior-IS call of the captcha-like program under both routes, alternating
    n = 131072
    model = Captcha()
    image = (model.patterns[2] * 1.05 + 0.1 * torch.randn(H, W, device=DEV, generator=gen)).cpu()
    wall = {'auto': [], 'torch': []}
    for r in range(a.reps + 1):
        for route in ('auto', 'torch'):
            os.environ['PP_VEC_LIKELIHOOD'] = route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, observe={'img': image}, lock_step=True, seed=r)
            torch.cuda.synchronize()
            if r:
                wall[route].append(time.perf_counter() - t0)
    os.environ.pop('PP_VEC_LIKELIHOOD', None)
    rec['captcha_prior_is_131072_kernel_ms'] = round(statistics.median(wall['auto']) * 1e3, 4)
    rec['captcha_prior_is_131072_torch_route_ms'] = round(statistics.median(wall['torch']) * 1e3, 4)
    rec['captcha_prior_is_131072_kernel_faster_in_every_pair'] = all(p < q for p, q in zip(wall['auto'], wall['torch']))
    assert all(math.isfinite(v) for v in rec.values() if isinstance(v, float))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
