"""Device time of the CNN2D5C observe embedding (csrc/cnn2d.hip): every launch of the convolution stack on its own
(in-stream hipEvent pairs, pp_prof_arm classes PP_PROF_CNN_FWD + k / PP_PROF_CNN_BWD + k), the whole forward and backward
of the stack, and the whole ICEngine.train_step of an LSTM network (H = 512) with a [1, 28, 28] image observable next to a
scalar one, at B = 64 and B = 1024. Baseline (`kind: port`): the same stack built from torch.nn modules in float32 on the
host's CPU threads. Writes one JSON document.

    python tools/cnn_embed_bench.py [--out profiles/cnn2d5c_bench.json] [--reps 20] [--batches 64,1024]
For kernel names and times of the same launches run it once more under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyprob_amd import ObserveEmbedding  # noqa: E402
from pyprob_amd import lib as L  # noqa: E402
from pyprob_amd.cnn import CNN2D5CStack  # noqa: E402
from pyprob_amd.engine import ICEngine  # noqa: E402
from pyprob_amd.packed import PackedBatch  # noqa: E402
from pyprob_amd.spec import NetSpec  # noqa: E402

PEAK_F32_MATRIX = 157.3e12      # the fp32-matrix peak the project's rooflines use
SHAPE = [1, 28, 28]
FWD = ['weight_images', 'conv1', 'conv2', 'pool1', 'conv3', 'conv4', 'conv5', 'pool2']
BWD = ['pool2_bwd', 'conv5_wgrad', 'conv5_dgrad', 'conv4_wgrad', 'conv4_dgrad', 'conv3_wgrad', 'conv3_dgrad', 'pool1_bwd',
       'conv2_wgrad', 'conv2_dgrad', 'conv1_wgrad']


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def class_times(lib, which, fn, reps):
    """Median milliseconds and the work of the launches of timing class `which` over `reps` calls of fn."""
    fn()
    torch.cuda.synchronize()
    lib.pp_prof_arm(which, reps)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, fl, cnt = np.zeros(reps, np.float32), np.zeros(reps, np.float64), C.c_int32(0)
    lib.pp_prof_collect(ms.ctypes.data, reps, C.byref(cnt), fl.ctypes.data)
    lib.pp_prof_arm(which, 0)
    assert cnt.value == reps, (which, cnt.value)
    return float(np.median(ms)), float(fl[0])


def synthetic_batch(B, spec, rng):
    """Traces of one (Categorical) and two (Categorical, Normal) statements, alternating; U[0, 1) images."""
    trace_len = np.where(np.arange(B) % 2 == 0, 1, 2).astype(np.int32)
    ids, values, prior = [], [], []
    for n in trace_len:
        ids.append(0); values.append(float(rng.integers(0, 10))); prior.append([0.1, 0.1])
        if n == 2:
            ids.append(1); values.append(float(rng.standard_normal())); prior.append([0.0, 1.0])
    obs = np.concatenate([rng.random((B, 784), dtype=np.float32), rng.standard_normal((B, 1)).astype(np.float32)], 1)
    return PackedBatch.from_ragged(trace_len, np.asarray(ids, np.int64), np.asarray(values, np.float32),
                                   np.asarray(prior, np.float32), obs, len(spec.addresses))


def cpu_port(B, reps):
    """The same stack from torch.nn modules, float32, forward + backward on the CPU threads of this host."""
    import torch.nn as nn
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(1, 64, 3), nn.ReLU(), nn.Conv2d(64, 64, 3), nn.ReLU(), nn.MaxPool2d(2),
                        nn.Conv2d(64, 128, 3), nn.ReLU(), nn.Conv2d(128, 128, 3), nn.ReLU(), nn.Conv2d(128, 128, 3), nn.ReLU(),
                        nn.MaxPool2d(2), nn.Flatten())
    x = torch.rand(B, *SHAPE)
    d = torch.randn(B, 1152) / B
    ts = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        net.zero_grad()
        net(x).backward(d)
        if i:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'cnn2d5c_bench.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batches', default='64,1024')
    ap.add_argument('--cpu-reps', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a ROCm device: a timing taken anywhere else says nothing about this code'
    lib = L.load()
    spec = NetSpec({'img': {'dim': 32, 'reshape': SHAPE, 'embedding': ObserveEmbedding.CNN2D5C}, 'y': {'dim': 8}}, lstm_dim=512)
    spec.add_address('d', 'Categorical', 10)
    spec.add_address('s', 'Normal')
    eng = ICEngine(spec, seed=0)
    stack = CNN2D5CStack(spec, 'img')
    rng = np.random.default_rng(1)
    doc = dict(device=torch.cuda.get_device_name(0), shape=SHAPE, lstm_dim=512, peak_f32_matrix_tflops=PEAK_F32_MATRIX / 1e12,
               cpu_threads=torch.get_num_threads(), runs=[])
    for B in [int(b) for b in args.batches.split(',')]:
        x = torch.from_numpy(rng.random((B, 784), dtype=np.float32)).cuda()
        d = torch.from_numpy((rng.standard_normal((B, 1152)) / B).astype(np.float32)).cuda()
        grads = torch.zeros_like(eng.params)

        def both():
            stack.forward(eng.params, x)
            stack.backward(eng.params, d, grads)

        kernels = {}
        for k, name in list(enumerate(FWD)) + [(16 + k, n) for k, n in enumerate(BWD)]:
            ms, flops = class_times(lib, L.PP_PROF_CNN_FWD + k, both, args.reps)
            kernels[name] = dict(us=1e3 * ms, flops=flops, fraction_of_peak=(flops / (ms * 1e-3) / PEAK_F32_MATRIX) if flops else None)
        fwd_ms = event_ms(lambda: stack.forward(eng.params, x), args.reps)
        both_ms = event_ms(both, args.reps)
        pb = synthetic_batch(B, spec, rng).to(eng.device)
        step_ms = event_ms(lambda: eng.train_step(pb, lr=1e-4), args.reps)
        loss_ms = event_ms(lambda: eng.loss(pb, backward=True), args.reps)
        total_flops = sum(v['flops'] for v in kernels.values())
        doc['runs'].append(dict(
            B=B, kernels=kernels, stack_forward_us=1e3 * fwd_ms, stack_forward_backward_us=1e3 * both_ms,
            stack_flops=total_flops, stack_fraction_of_peak=total_flops / (both_ms * 1e-3) / PEAK_F32_MATRIX,
            train_step_us=1e3 * step_ms, loss_backward_us=1e3 * loss_ms,
            stack_workspace_bytes=stack.workspace_bytes(B), ic_workspace_bytes=int(eng.ws_bytes),
            baseline=dict(kind='port', what='torch.nn float32 forward + backward of the stack on the CPU',
                          stack_forward_backward_us=1e3 * cpu_port(B, args.cpu_reps))))
        r = doc['runs'][-1]
        print('B = %d: stack fwd %.0f us, fwd + bwd %.0f us (%.1f %% of the fp32-matrix peak), train_step %.0f us, CPU port %.0f us'
              % (B, r['stack_forward_us'], r['stack_forward_backward_us'], 100 * r['stack_fraction_of_peak'], r['train_step_us'],
                 r['baseline']['stack_forward_backward_us']))
        for name, v in kernels.items():
            print('    %-14s %9.1f us  %s' % (name, v['us'], '%.1f %%' % (100 * v['fraction_of_peak']) if v['flops'] else ''))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
