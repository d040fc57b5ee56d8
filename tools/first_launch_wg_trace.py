"""Per-workgroup timeline of the FIRST launch (obs_embed_fwd_kernel) of the single-statement training step that bench.py times
(GPU box; the sibling of tools/adam_wg_trace.py: the same engine, batches and warm-up):
   python tools/first_launch_wg_trace.py                     # the order the step runs (PP_FIRST_EARLY as set; default 1)
   PP_FIRST_EARLY=0 python tools/first_launch_wg_trace.py    # the parent's order
   PP_PANEL_EMBED=0 python tools/first_launch_wg_trace.py    # with the embedding workgroups (unset, the panel kernel embeds its
                                                             # rows and this launch has none: bias and image workgroups only)
Stamps (pp_debug_wgtrace mode 4, 10 ns ticks). Embedding workgroups: start, entry loads issued, weights arrived, LDS image
complete (behind the barrier), observation arrived and layer 0 done, last dense layer done, stores issued, end. Bias and
image workgroups: start, operands arrived, end, job kind. An "arrived" stamp waits for the loads issued so far, so the traced
launch is a little slower than the untraced one: the stamps show where a workgroup's time goes, the launch's length comes from
rocprofv3. Only the first launch of eng.loss(..., backward=True) is traced: the panel kernel and the rest run behind it
untraced."""
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
print('PP_FIRST_EARLY=%s' % os.environ.get('PP_FIRST_EARLY', '1'))
cap = 4096
buf = torch.zeros(8 * cap, dtype=torch.int64, device=dev)
STAMPS = ('entry loads issued', 'weights arrived', 'LDS image complete', 'layer 0 done', 'last layer done', 'stores issued', 'end')
KINDS = {1: 'bias workgroups', 2: 'image workgroups'}
for rep in range(3):
    buf.zero_()
    eng.optimizer_step(1e-3, zero_grads=True, skip=eng.status_buf, live=True)   # (Adam has just rewritten the weights, as in the loop)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(buf.data_ptr(), cap, 4)
    eng.loss(batches[rep], backward=True)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(None, 0, 0)
    t = buf.cpu().numpy().reshape(cap, 8)
    started = t[:, 0] > 0
    if not started.any():
        print('rep %d: no workgroup stamped (the step did not take the fused first launch)' % rep)
        continue
    t0 = t[started, 0].min()
    us = lambda x: (x - t0) / 100.0
    emb = started & (t[:, 7] > 2)          # word 7 of an embedding workgroup is its end stamp, of a job workgroup its kind
    last_end = max(t[emb, 7].max() if emb.any() else 0, t[started & ~emb, 2].max() if (started & ~emb).any() else 0)
    print('rep %d: %d workgroups started (%d embedding); launch span %.2f us (first start to last end)' % (
        rep, started.sum(), emb.sum(), us(last_end)))
    print('  workgroup starts: median %.2f us, 90 %% by %.2f us, last %.2f us' % (
        np.median(us(t[started, 0])), np.quantile(us(t[started, 0]), 0.9), us(t[started, 0].max())))
    if emb.any():
        s = t[emb, 0]
        e = t[emb, 7]
        print('  %-22s %4d: start %5.2f .. %5.2f us; end median %5.2f, last %5.2f us; lifetime median %5.2f, max %5.2f us' % (
            'embedding workgroups', emb.sum(), us(s.min()), us(s.max()), np.median(us(e)), us(e.max()),
            np.median((e - s) / 100.0), ((e - s) / 100.0).max()))
        prev = s
        for k, name in enumerate(STAMPS, start=1):
            col = t[emb, k]
            ok = col > 0          # (0 = not taken on this path)
            if not ok.any():
                continue
            seg = (col[ok] - prev[ok]) / 100.0
            print('      -> %-18s +%5.2f us median (+%5.2f max); at %5.2f us median since the workgroup started' % (
                name, np.median(seg), seg.max(), np.median((col[ok] - s[ok]) / 100.0)))
            prev = np.where(ok, col, prev)
    for kind, label in KINDS.items():
        m = started & (t[:, 7] == kind) & (t[:, 2] > 0)
        if not m.any():
            print('  %-22s none in this launch' % label)
            continue
        s = t[m, 0]
        e = t[m, 2]
        arrived = t[m, 1]
        ok = arrived > 0
        print('  %-22s %4d: start %5.2f .. %5.2f us; end median %5.2f, last %5.2f us; lifetime median %5.2f, max %5.2f us; '
              'operands arrived +%5.2f us median' % (
                  label, m.sum(), us(s.min()), us(s.max()), np.median(us(e)), us(e.max()), np.median((e - s) / 100.0),
                  ((e - s) / 100.0).max(), np.median((arrived[ok] - s[ok]) / 100.0) if ok.any() else float('nan')))
    ends = np.where(emb, t[:, 7], t[:, 2])
    done = started & (ends > 0)
    span = int(us(ends[done].max())) + 1
    run = np.zeros(span + 1)
    for a, b in zip(us(t[done, 0]), us(ends[done])):
        run[int(a):int(b) + 1] += 1
    print('  resident workgroups every 1 us:', ' '.join('%d' % run[i] for i in range(0, span)))
