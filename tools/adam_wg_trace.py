"""Per-workgroup timeline of ONE Adam launch of the single-statement training step that bench.py times (GPU box; the sibling of
tools/wg_trace_wgrad_single.py):
   python tools/adam_wg_trace.py                    # the launch the training paths use (PP_ADAM_LIVE as set; default: live chunks)
   PP_ADAM_LIVE=0 python tools/adam_wg_trace.py     # the full grid (adam_kernel): what the step ran before the live-chunk launch
Stamps (pp_debug_wgtrace mode 3, 10 ns ticks): workgroup start, tensor known, gradient arrived, p / m / v arrived, corrections
ready (after the second barrier), stores issued, workgroup end - reported for the workgroups of W_hh (zero gradient for ever in a
single-statement program) and for all others. An "arrived" stamp waits for the loads issued so far, so the traced launch is a
little slower than the untraced one: the stamps show where a workgroup's time goes, the launch's length comes from rocprofv3."""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'tests'))
import torch
import bench
from helpers import synthetic_gum_arrays
from pyprob_amd import lib as L
from pyprob_amd.packed import PackedBatch

lib = L.load()
dev = torch.device('cuda:0')
eng = bench.make_engine(512, dev, seed=123)
batches = []
for i in range(4):
    arr = synthetic_gum_arrays(1024, seed=100 + i)
    batches.append(PackedBatch.from_ragged(arr['trace_len'], arr['addr_idx'], arr['values'], arr['prior'], arr['obs'], 1).to(dev))
for i in range(40):
    eng.train_step(batches[i % 4], 1e-3)
torch.cuda.synchronize()
names = list(eng.spec.tensors.keys())
whh = names.index('_layers_lstm.weight_hh_l0')
n_chunks = eng.spec.n_params // 1024
print('PP_ADAM_LIVE=%s: %d tensors, %d chunks (%d of W_hh); untouched tensors: %s' % (
    os.environ.get('PP_ADAM_LIVE', '1'), len(names), n_chunks, int((eng.chunk_tensor == whh).sum()),
    [names[t] for t in np.nonzero(~eng.live_info()[1])[0]] if hasattr(eng, 'live_info') else 'n/a'))
cap = 4096
buf = torch.zeros(8 * cap, dtype=torch.int64, device=dev)
STAMPS = ('tensor known', 'gradient arrived', 'p/m/v arrived', 'corrections ready', 'stores issued', 'end')
for rep in range(3):
    buf.zero_()
    eng.loss(batches[rep], backward=True)            # (the launches before Adam run untraced)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(buf.data_ptr(), cap, 3)
    eng.optimizer_step(1e-3, zero_grads=True, skip=eng.status_buf, live=True)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(None, 0, 0)
    t = buf.cpu().numpy().reshape(cap, 8)
    started = t[:, 0] > 0
    t0 = t[started, 0].min()
    us = lambda x: (x - t0) / 100.0
    done = started & (t[:, 6] > 0)
    print('rep %d: %d workgroups started, %d ran the update path; launch span %.2f us (first start to last end)' % (
        rep, started.sum(), done.sum(), us(max(t[done, 6].max(), t[started, 0].max()))))
    print('  workgroup starts: median %.2f us, 90 %% by %.2f us, last %.2f us' % (
        np.median(us(t[started, 0])), np.quantile(us(t[started, 0]), 0.9), us(t[started, 0].max())))
    for label, m in (('W_hh workgroups', done & (t[:, 7] == whh)), ('all other workgroups', done & (t[:, 7] != whh))):
        if not m.any():
            print('  %-22s none in this launch' % label)
            continue
        s = t[m, 0]
        print('  %-22s %4d: start %5.2f .. %5.2f us; end median %5.2f, last %5.2f us; lifetime median %5.2f, max %5.2f us' % (
            label, m.sum(), us(s.min()), us(s.max()), np.median(us(t[m, 6])), us(t[m, 6].max()),
            np.median((t[m, 6] - s) / 100.0), ((t[m, 6] - s) / 100.0).max()))
        prev = s
        for k, name in enumerate(STAMPS, start=1):
            col = t[m, k]
            ok = col > 0          # (a stamp is taken by the thread named in the kernel; 0 = not taken on this path)
            if not ok.any():
                continue
            seg = (col[ok] - prev[ok]) / 100.0
            print('      -> %-18s +%5.2f us median (+%5.2f max); at %5.2f us median since the workgroup started' % (
                name, np.median(seg), seg.max(), np.median((col[ok] - s[ok]) / 100.0)))
            prev = np.where(ok, col, prev)
    span = int(us(t[done, 6].max())) + 1
    run = np.zeros(span + 1)
    for a, b in zip(us(t[done, 0]), us(t[done, 6])):
        run[int(a):int(b) + 1] += 1
    print('  resident workgroups every 1 us:', ' '.join('%d' % run[i] for i in range(0, span)))
