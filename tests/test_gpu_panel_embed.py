"""PP_PANEL_EMBED (csrc/panel16.hip EMBED): the 16-row panel kernel computes the observe embedding of its rows in its staging
phase - layer 0 on VALU, the per-observable output layers and the two 64 x 64 layers on MFMA - and writes E (also into the X
rows), cat, f1 and the observables' hidden rows itself; the step's first launch then has no embedding workgroups (1; the
default at lstm_dim 512), or the first launch embeds as before (0; the default at 1024, where 1 measured slower). The MFMA sums associate E differently from the scalar walk, so the two settings
need not agree bit for bit with each other; under ONE setting every per-row value is reproducible. One process alternates the
switch from step to step on the SAME workspace - 0, 1, 0, 1. Batches: one full panel, a second panel with one live row (the
row clamp and the unwritten pad rows), a ragged middle size, and the wide network. Both settings are held against the float64
oracle: the embedding's weight and bias gradients use E / X, cat, f1, the hidden rows and the observations as operands, so this
covers every buffer the panel kernel now stores.

Shapes: panel16_obs_ok wants <= 16 hidden units and a multiple of 16 outputs per observable, 64 outputs in all; NetSpec's hidden
width is (input_dim + dim) // 2, so the ONE shape it can build that the kernel accepts is two observables of dim 32 with scalar
inputs (a single observable of dim 64 has >= 32 hidden units). The rejected shape here is dims 16 + 48 (24 hidden units in the
second observable): it keeps the first launch's embedding workgroups whatever the switch says, and must match the oracle too.
Which path a step took is read off the first launch's workgroup trace (pp_debug_wgtrace mode 4: an embedding workgroup leaves
its end stamp in word 7, a job workgroup its kind, 1 or 2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grad_check, synthetic_gum_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OBS = {'two32': {'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, 'rejected': {'obs0': {'dim': 16}, 'obs1': {'dim': 48}}}
# (network, lstm_dim, rows, seed) in the order they run, through one engine per (network, lstm_dim)
CASES = (('two32', 512, 16, 61), ('two32', 512, 17, 62), ('two32', 512, 40, 63), ('two32', 1024, 17, 64), ('rejected', 512, 40, 65))
ORDER = ('0', '1', '0', '1')    # the switch of the four steps of every case
RUN_ROWS = (1024, 1003, 17)
NAN_ROWS, NAN_ROW = 40, 21      # the NaN observation: row 21 of 40 (the second panel, workgroup quarter 1)

SCRIPT = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
from helpers import synthetic_gum_arrays
from pyprob_amd import lib as L
from pyprob_amd.engine import ICEngine
from pyprob_amd.packed import PackedBatch
from pyprob_amd.spec import NetSpec
lib = L.load()
OBS = %(obs)r
out = {}
def packed(arr):
    return PackedBatch.from_ragged(arr['trace_len'], arr['addr_idx'], arr['values'], arr['prior'], arr['obs'], 1)
def batch(B, seed):
    return packed(synthetic_gum_arrays(B, seed=seed))
def make(net, H, seed):
    spec = NetSpec(OBS[net], lstm_dim=H)
    spec.add_address('mu', 'Normal')
    return ICEngine(spec, device='cuda:0', seed=seed)
CAP = 4096
trace = torch.zeros(8 * CAP, dtype=torch.int64, device='cuda:0')

# ---- the step: loss + backward with per-row log_prob, the switch alternating on one workspace ----
engines = {}
for net, H, B, seed in %(cases)r:
    if (net, H) not in engines:
        engines[(net, H)] = make(net, H, 11)
        for name, t in engines[(net, H)].state_dict().items():
            out['param_%%s%%d/%%s' %% (net, H, name)] = t.numpy()
    eng = engines[(net, H)]
    pb = batch(B, seed).to(eng.device)
    for k, mode in enumerate(%(order)r):
        os.environ['PP_PANEL_EMBED'] = mode       # (read by the library at every call)
        trace.zero_()
        torch.cuda.synchronize()
        lib.pp_debug_wgtrace(trace.data_ptr(), CAP, 4)
        l, lp = eng.loss(pb, backward=True, keep_lp=True)
        torch.cuda.synchronize()
        lib.pp_debug_wgtrace(None, 0, 0)
        t = trace.cpu().numpy().reshape(CAP, 8)
        tag = '%%s_h%%d_b%%d_s%%d' %% (net, H, B, k)
        out[tag + '_wgs'] = np.array([(t[:, 0] > 0).sum(), ((t[:, 0] > 0) & (t[:, 7] > 2)).sum()])   # started, embedding
        out[tag + '_loss'] = l.cpu().numpy()
        out[tag + '_lp'] = lp.cpu().numpy()
        out[tag + '_status'] = eng.status_buf[:1].cpu().numpy()
        out[tag + '_grads'] = eng.grads.cpu().numpy()

# ---- a NaN observation in one row ----
arr = synthetic_gum_arrays(%(nan_rows)d, seed=77)
arr['obs'][%(nan_row)d, 0] = np.nan
eng = engines[('two32', 512)]
pb = packed(arr).to(eng.device)
for mode in ('0', '1'):
    os.environ['PP_PANEL_EMBED'] = mode
    l, lp = eng.loss(pb, backward=True, keep_lp=True)
    torch.cuda.synchronize()
    out['nan_loss_' + mode] = l.cpu().numpy()
    out['nan_lp_' + mode] = lp.cpu().numpy()
    out['nan_status_' + mode] = eng.status_buf[:1].cpu().numpy()

# ---- three training steps from one initial state under each setting ----
for mode in ('0', '1'):
    os.environ['PP_PANEL_EMBED'] = mode
    eng = make('two32', 512, 5)
    losses = []
    for k, B in enumerate(%(run_rows)r):
        losses.append(eng.train_step(batch(B, 500 + k).to(eng.device), 1e-3).clone())
    torch.cuda.synchronize()
    out['run_losses_' + mode] = torch.cat(losses).cpu().numpy()
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    f = str(tmp_path_factory.mktemp('panel_embed') / 'runs.npz')
    e = dict(os.environ, PP_DETERMINISTIC='0')
    for k in ('PP_PANEL', 'PP_PANEL_HANDOFF', 'PP_PANEL_PUBLISH', 'PP_PANEL_EMBED', 'PP_STORE_WT', 'PP_FIRST_EARLY'):
        e.pop(k, None)
    script = SCRIPT % dict(repo=REPO, obs=OBS, cases=CASES, order=ORDER, run_rows=RUN_ROWS, nan_rows=NAN_ROWS, nan_row=NAN_ROW)
    subprocess.run([sys.executable, '-c', script, f], check=True, env=e, timeout=600)
    return dict(np.load(f))


def _spec(net, H):
    from pyprob_amd.spec import NetSpec
    spec = NetSpec(OBS[net], lstm_dim=H)
    spec.add_address('mu', 'Normal')
    return spec


@pytest.fixture(scope='module')
def oracle_refs(runs):
    """Loss and gradients of the cases from the float64 oracle (the parameters do not change between the steps)."""
    from oracle import ic_oracle as O
    refs = {}
    for net, H, B, seed in CASES:
        pre = 'param_%s%d/' % (net, H)
        P = {k[len(pre):]: v.astype(np.float64) for k, v in runs.items() if k.startswith(pre)}
        refs[(net, H, B)] = O.loss_and_grads(O.Net(P, ['obs0', 'obs1'], K=10), synthetic_gum_arrays(B, seed=seed), ['mu'], ['Normal'])
    return refs


CASE_IDS = [(n, h, b) for n, h, b, _ in CASES]


@pytest.mark.parametrize('net,H,B', CASE_IDS)
def test_the_switch_selects_the_launch_that_embeds(runs, net, H, B):
    """Setting 1 on the accepted shape: the first launch has job workgroups only. Setting 0, and the rejected shape under either
    setting: one embedding wave per trace, four per workgroup."""
    for k, mode in enumerate(ORDER):
        started, emb = (int(x) for x in runs['%s_h%d_b%d_s%d_wgs' % (net, H, B, k)])
        print(net, H, B, 'PP_PANEL_EMBED', mode, 'workgroups', started, 'embedding', emb)
        assert started > 0
        assert emb == (0 if (mode == '1' and net == 'two32') else (B + 3) // 4)


@pytest.mark.parametrize('net,H,B', CASE_IDS)
def test_rows_are_bitwise_equal_within_a_setting(runs, net, H, B):
    """Per-row log_prob and the status word involve no atomics: under one setting the same bits in both of its steps, whichever
    setting ran one step earlier on the workspace."""
    for k in range(len(ORDER)):
        tag = '%s_h%d_b%d_s%d' % (net, H, B, k)
        lp = runs[tag + '_lp']
        first = runs['%s_h%d_b%d_s%d_lp' % (net, H, B, ORDER.index(ORDER[k]))]
        assert lp.shape == (B,) and np.isfinite(lp).all(), tag
        assert int(runs[tag + '_status'][0]) == 0, tag
        assert np.array_equal(lp.view(np.int32), first.view(np.int32)), (tag, ORDER[k])


@pytest.mark.parametrize('mode', ['0', '1'])
@pytest.mark.parametrize('net,H,B', CASE_IDS)
def test_step_matches_the_oracle_under_both_settings(runs, oracle_refs, net, H, B, mode):
    """The comparison of tests/test_gpu_panel_handoff16.py, same helpers and bounds, for both steps of the setting."""
    spec = _spec(net, H)
    ref = oracle_refs[(net, H, B)]
    for k in (i for i, s in enumerate(ORDER) if s == mode):
        tag = '%s_h%d_b%d_s%d' % (net, H, B, k)
        loss = float(runs[tag + '_loss'][0])
        print(tag, 'embed', mode, 'loss', loss, 'oracle', ref['loss'])
        assert abs(loss - ref['loss']) <= 2e-5 * abs(ref['loss'])
        for n, (off, shape) in spec.tensors.items():
            if np.abs(ref['grads'][n]).max() > 1e-7:
                g = runs[tag + '_grads'][off:off + int(np.prod(shape))].reshape(shape)
                grad_check('panel_embed_%s_%s/%s' % (mode, tag, n), g, ref['grads'][n], 5e-6)


def test_training_steps_agree_under_both_settings(runs):
    """Three Adam steps from the same initial state, B = 1024, 1003, 17 (the bound of the store-policy tests)."""
    a, b = runs['run_losses_0'], runs['run_losses_1']
    assert a.shape == (3,) and np.isfinite(a).all() and np.isfinite(b).all()
    print('run losses', a, b)
    np.testing.assert_allclose(b, a, rtol=2e-4, atol=2e-5)


def test_a_nan_observation_reads_the_same_under_both_settings(runs):
    """One NaN observation: the same status word and the same non-finite loss; the row itself is non-finite and every other
    row of its panel stays finite (rows are independent in the MFMA layers) under both settings."""
    s0, s1 = int(runs['nan_status_0'][0]), int(runs['nan_status_1'][0])
    l0, l1 = float(runs['nan_loss_0'][0]), float(runs['nan_loss_1'][0])
    print('nan status', s0, s1, 'loss', l0, l1)
    assert s0 == s1 == 1
    assert not np.isfinite(l0) and not np.isfinite(l1)
    assert np.isnan(l0) == np.isnan(l1)
    others = np.arange(NAN_ROWS) != NAN_ROW
    for mode in ('0', '1'):
        lp = runs['nan_lp_' + mode]
        assert not np.isfinite(lp[NAN_ROW]), mode
        assert np.isfinite(lp[others]).all(), mode
