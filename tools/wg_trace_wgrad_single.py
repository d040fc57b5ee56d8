"""Per-workgroup timeline of wgrad_t1_kernel (+ the reduction jobs behind it) for the single-statement training step that
bench.py times (GPU box; the sibling of tools/wg_trace_wgrad.py, which traces the ragged step):
   python tools/wg_trace_wgrad_single.py     # per problem of the launch: when its workgroups start, how long the K loop and the
                                             # epilogue take, when they end; the last tile / the last reduction workgroup; the
                                             # workgroups that start after t = 0; resident workgroups over time"""
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
cap = 8192
buf = torch.zeros(8 * cap, dtype=torch.int64, device=dev)
for rep in range(2):
    buf.zero_()
    lib.pp_debug_wgtrace(buf.data_ptr(), cap, 1)
    eng.train_step(batches[rep], 1e-3)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(None, 0, 0)
    t = buf.cpu().numpy().reshape(cap, 8)
    live = t[:, 1] > 0
    idx = np.nonzero(live)[0]
    t = t[live]
    t0 = t[:, 0].min()
    us = lambda x: (x - t0) / 100.0
    tile = t[:, 2] < 100
    print('rep %d: %d workgroups stamped (%d tiles, %d reduction jobs), launch span %.2f us' % (
        rep, len(t), tile.sum(), (~tile).sum(), us(t[:, 1].max())))
    print('  last tile workgroup ends %.2f us, last reduction workgroup ends %.2f us' % (
        us(t[tile, 1].max()), us(t[~tile, 1].max()) if (~tile).any() else 0.0))
    # "after t = 0": a workgroup that starts later than the first wave of dispatches (1 us) waited for a slot or for the dispatcher
    late = us(t[:, 0]) > 1.0
    print('  workgroups that start after 1 us: %d (%d tiles, %d reduction jobs), the latest at %.2f us' % (
        late.sum(), (late & tile).sum(), (late & ~tile).sum(), us(t[:, 0].max())))
    for q in sorted(set(t[:, 2].tolist())):
        m = t[:, 2] == q
        s, e = us(t[m, 0]), us(t[m, 1])
        line = 'problem %3d: %4d wgs (ids %4d..%4d) start %6.2f .. %6.2f  end %6.2f .. %6.2f  duration mean %6.2f max %6.2f' % (
            q, m.sum(), idx[m].min(), idx[m].max(), s.min(), s.max(), e.min(), e.max(), (e - s).mean(), (e - s).max())
        if q < 100:
            k = us(t[m, 4])
            line += '  K loop mean %6.2f  epilogue mean %5.2f' % ((k - s).mean(), (e - k).mean())
        print(line)
    # the workgroups that end last: launch index, problem (100 = reduction job), row split, K loop / epilogue
    for w in np.argsort(-t[:, 1])[:12]:
        line = '  ends %6.2f: workgroup %4d problem %3d split %d start %5.2f' % (us(t[w, 1]), idx[w], t[w, 2], t[w, 3], us(t[w, 0]))
        if t[w, 2] < 100:
            line += '  K loop %5.2f epilogue %5.2f' % (us(t[w, 4]) - us(t[w, 0]), us(t[w, 1]) - us(t[w, 4]))
        print(line)
    span = int(us(t[:, 1].max())) + 1
    run = np.zeros(span + 1)
    for a, b in zip(us(t[:, 0]), us(t[:, 1])):
        run[int(a):int(b) + 1] += 1
    print('resident workgroups every 1 us:', ' '.join('%d' % run[i] for i in range(0, span)))
