"""PP_PANEL_PUBLISH (csrc/panel16.hip): in its second cross-workgroup exchange the 16-row panel kernel publishes its partial
dX before it writes the observe-embedding weight image into LDS and leaves dX itself unwritten (the default, early), or does
what it did before (late: the image first, dX stored). The granules, their slots and the order of every sum are the same,
so every value behind the exchange must be bit for bit the same. (The 16-byte double granules this file is named after lost
to the 8-byte ones in tools/micro/handoff_probe.hip and were not built, and publishing only the rows a partner reads did
not pay: DESIGN.md section 8.) One process alternates the switch from step to step on the SAME workspace - old, new, old,
new; a slot of an earlier step carries an older epoch's tag and must never read as ready. Batches: one panel, a ragged last
panel, a second panel with one live row behind the longer batch's stale slots, and the wide network; then a short run of
training steps under each setting. Both settings are also held against the float64 oracle (the observe-embedding tensors
are the only outputs the second exchange reaches)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grad_check, synthetic_gum_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (lstm_dim, rows, seed) in the order they run, through one engine per lstm_dim
CASES = ((512, 16, 41), (512, 1003, 42), (512, 17, 43), (1024, 1003, 44), (1024, 17, 45))
ORDER = ('late', 'early', 'late', 'early')    # the switch of the four steps of every case
RUN_ROWS = (1024, 1003, 17)

SCRIPT = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
from helpers import synthetic_gum_arrays
from pyprob_amd.engine import ICEngine
from pyprob_amd.packed import PackedBatch
from pyprob_amd.spec import NetSpec
out = {}
def batch(B, seed):
    arr = synthetic_gum_arrays(B, seed=seed)
    return PackedBatch.from_ragged(arr['trace_len'], arr['addr_idx'], arr['values'], arr['prior'], arr['obs'], 1)
def make(H, seed):
    spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=H)
    spec.add_address('mu', 'Normal')
    return ICEngine(spec, device='cuda:0', seed=seed)

# ---- the step: loss + backward with per-row log_prob, the switch alternating on one workspace ----
engines = {}
for H, B, seed in %(cases)r:
    if H not in engines:
        engines[H] = make(H, 11)
        for name, t in engines[H].state_dict().items():
            out['param%%d/%%s' %% (H, name)] = t.numpy()
    eng = engines[H]
    pb = batch(B, seed).to(eng.device)
    for k, mode in enumerate(%(order)r):
        os.environ['PP_PANEL_PUBLISH'] = mode       # (read by the library at every call)
        l, lp = eng.loss(pb, backward=True, keep_lp=True)
        torch.cuda.synchronize()
        tag = 'h%%d_b%%d_s%%d' %% (H, B, k)
        out[tag + '_loss'] = l.cpu().numpy()
        out[tag + '_lp'] = lp.cpu().numpy()
        out[tag + '_status'] = eng.status_buf[:1].cpu().numpy()
        out[tag + '_grads'] = eng.grads.cpu().numpy()

# ---- three training steps from one initial state under each setting ----
for mode in ('late', 'early'):
    os.environ['PP_PANEL_PUBLISH'] = mode
    eng = make(512, 5)
    losses = []
    for k, B in enumerate(%(run_rows)r):
        losses.append(eng.train_step(batch(B, 500 + k).to(eng.device), 1e-3).clone())
    torch.cuda.synchronize()
    out['run_losses_' + mode] = torch.cat(losses).cpu().numpy()
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    f = str(tmp_path_factory.mktemp('handoff16') / 'runs.npz')
    e = dict(os.environ, PP_DETERMINISTIC='0')
    for k in ('PP_PANEL', 'PP_PANEL_HANDOFF', 'PP_PANEL_PUBLISH', 'PP_STORE_WT'):
        e.pop(k, None)
    script = SCRIPT % dict(repo=REPO, cases=CASES, order=ORDER, run_rows=RUN_ROWS)
    subprocess.run([sys.executable, '-c', script, f], check=True, env=e, timeout=600)
    return dict(np.load(f))


@pytest.fixture(scope='module')
def oracle_refs(runs):
    """Loss and gradients of the cases from the float64 oracle (the parameters do not change between the steps)."""
    from oracle import ic_oracle as O
    refs = {}
    for H, B, seed in CASES:
        pre = 'param%d/' % H
        P = {k[len(pre):]: v.astype(np.float64) for k, v in runs.items() if k.startswith(pre)}
        net = O.Net(P, ['obs0', 'obs1'], K=10)
        refs[(H, B)] = O.loss_and_grads(net, synthetic_gum_arrays(B, seed=seed), ['mu'], ['Normal'])
    return refs


@pytest.mark.parametrize('H,B', [(h, b) for h, b, _ in CASES])
def test_rows_are_bitwise_equal_under_both_orders(runs, H, B):
    """Per-row log_prob and the status word involve no atomics: the same bits in all four steps, whichever setting filled the
    slots one step earlier."""
    first = runs['h%d_b%d_s0_lp' % (H, B)]
    assert first.shape == (B,) and np.isfinite(first).all()
    for k in range(len(ORDER)):
        tag = 'h%d_b%d_s%d' % (H, B, k)
        assert int(runs[tag + '_status'][0]) == 0, tag
        assert np.array_equal(runs[tag + '_lp'].view(np.int32), first.view(np.int32)), (tag, ORDER[k])


@pytest.mark.parametrize('mode', ['late', 'early'])
@pytest.mark.parametrize('H,B', [(h, b) for h, b, _ in CASES])
def test_step_matches_the_oracle_under_both_orders(runs, oracle_refs, H, B, mode):
    """The comparison of tests/test_gpu_panel.py test_panel_kernel_against_the_oracle, same helpers and bounds, for both steps
    of the setting."""
    from pyprob_amd.spec import NetSpec
    spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=H)
    spec.add_address('mu', 'Normal')
    ref = oracle_refs[(H, B)]
    for k in (i for i, s in enumerate(ORDER) if s == mode):
        tag = 'h%d_b%d_s%d' % (H, B, k)
        loss = float(runs[tag + '_loss'][0])
        print(tag, 'publish', mode, 'loss', loss, 'oracle', ref['loss'])
        assert abs(loss - ref['loss']) <= 2e-5 * abs(ref['loss'])
        for n, (off, shape) in spec.tensors.items():
            if np.abs(ref['grads'][n]).max() > 1e-7:
                g = runs[tag + '_grads'][off:off + int(np.prod(shape))].reshape(shape)
                grad_check('handoff16_%s_%s/%s' % (mode, tag, n), g, ref['grads'][n], 5e-6)


def test_training_steps_agree_under_both_orders(runs):
    """Three Adam steps from the same initial state, B = 1024, 1003, 17 (the bound of the store-policy tests)."""
    a, b = runs['run_losses_late'], runs['run_losses_early']
    assert a.shape == (3,) and np.isfinite(a).all() and np.isfinite(b).all()
    print('run losses', a, b)
    np.testing.assert_allclose(b, a, rtol=2e-4, atol=2e-5)
