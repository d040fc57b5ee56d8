"""PP_STORE_WT (csrc/common.hpp store16_wt): the training step's results leave their kernels as 16-byte write-through
stores (default, 1) or as the plain stores they were (0). Only the cache policy differs, so every stored value must be
bit for bit the same: Adam at the C ABI (pp_adam_step: idle tensor, two steps, a skipped call), the step's per-row
log_prob and status at one panel, a second panel with one live row, a ragged last panel and the wide network, and a
short run of training steps. One subprocess per setting; both settings are also held against the float64 oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grad_check, rel_err, synthetic_gum_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ADAM_SIZES = (1, 1023, 1024, 1025, 3000)     # tensors of the flat buffer, each padded to 1024-float chunks
ADAM_IDLE = 2                                # the tensor whose gradient is all zero (and whose moments therefore are)
ADAM_LR = 1e-3
# (lstm_dim, rows, seed) in the order they run: every batch is followed by a different one through the same workspace
# (1003 then 17: rows 1..15 of the second panel hold the longer batch's values and must stay masked)
STEP_CASES = ((512, 16, 31), (512, 1003, 32), (512, 17, 33), (1024, 1003, 34), (1024, 17, 35))
ORACLE_CASES = ((512, 16, 31), (512, 17, 33), (512, 1003, 32), (1024, 17, 35))

SCRIPT = r'''
import ctypes as C, sys, numpy as np, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
from helpers import synthetic_gum_arrays
from pyprob_amd import lib as L
from pyprob_amd.engine import ICEngine
from pyprob_amd.packed import PackedBatch
from pyprob_amd.spec import NetSpec
out = {}
dev = torch.device('cuda:0')
lib = L.load()

# ---- pp_adam_step on a hand-made flat buffer ----
sizes = %(sizes)r
chunks = [(s + 1023) // 1024 for s in sizes]
offs = [1024 * sum(chunks[:t]) for t in range(len(sizes))]
n = 1024 * sum(chunks)
def flat(seed, scale, skip_tensor=None):
    rng = np.random.default_rng(seed)
    a = np.zeros(n, np.float32)
    for t, s in enumerate(sizes):
        v = (scale * rng.standard_normal(s)).astype(np.float32)
        if t != skip_tensor:
            a[offs[t]:offs[t] + s] = v
    return a
P = torch.from_numpy(flat(7, 1.0)).to(dev)
M = torch.zeros(n, device=dev); V = torch.zeros(n, device=dev); G = torch.zeros(n, device=dev)
ct = torch.from_numpy(np.repeat(np.arange(len(sizes)), chunks).astype(np.int32)).to(dev)
active = torch.ones(len(sizes), device=dev)
tstep = torch.zeros(len(sizes), dtype=torch.int32, device=dev)
scratch = torch.zeros(L.PP_ADAM_SCRATCH * len(sizes), dtype=torch.int32, device=dev)
skip = torch.zeros(1, dtype=torch.int32, device=dev)
out['adam_p0'] = P.cpu().numpy()
for call in range(3):        # two steps, then a call with the skip flag set
    g = flat(100 + call, 0.1, skip_tensor=%(idle)d)
    out['adam_g%%d' %% call] = g
    G.copy_(torch.from_numpy(g))
    skip.fill_(1 if call == 2 else 0)
    rc = lib.pp_adam_step(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, ct.data_ptr(), active.data_ptr(),
                          tstep.data_ptr(), scratch.data_ptr(), len(sizes), %(lr)r, 0.9, 0.999, 1e-8, 0.0, 1.0,
                          L.PP_ADAM_ZERO_GRADS, skip.data_ptr(), None)
    L.check(rc, 'pp_adam_step')
    torch.cuda.synchronize()
    for k, t in (('p', P), ('m', M), ('v', V), ('g', G), ('step', tstep)):
        out['adam_%%s_after%%d' %% (k, call)] = t.cpu().numpy()

# ---- the step: loss + backward with per-row log_prob ----
engines = {}
def batch(B, seed):
    arr = synthetic_gum_arrays(B, seed=seed)
    return PackedBatch.from_ragged(arr['trace_len'], arr['addr_idx'], arr['values'], arr['prior'], arr['obs'], 1)
for H, B, seed in %(cases)r:
    if H not in engines:
        spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=H)
        spec.add_address('mu', 'Normal')
        engines[H] = ICEngine(spec, device='cuda:0', seed=11)
        for name, t in engines[H].state_dict().items():
            out['param%%d/%%s' %% (H, name)] = t.numpy()
    eng = engines[H]
    l, lp = eng.loss(batch(B, seed).to(eng.device), backward=True, keep_lp=True)
    torch.cuda.synchronize()
    tag = 'h%%d_b%%d' %% (H, B)
    out[tag + '_loss'] = l.cpu().numpy()
    out[tag + '_lp'] = lp.cpu().numpy()
    out[tag + '_status'] = eng.status_buf[:1].cpu().numpy()
    out[tag + '_grads'] = eng.grads.cpu().numpy()

# ---- three training steps from the initial state ----
spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=512)
spec.add_address('mu', 'Normal')
eng = ICEngine(spec, device='cuda:0', seed=5)
losses = []
for k, B in enumerate((1024, 1003, 17)):
    losses.append(eng.train_step(batch(B, 500 + k).to(eng.device), 1e-3).clone())
torch.cuda.synchronize()
out['run_losses'] = torch.cat(losses).cpu().numpy()
np.savez(sys.argv[1], **out)
'''


def _run(tmp_path, wt):
    f = str(tmp_path / ('wt%s.npz' % wt))
    e = dict(os.environ, PP_DETERMINISTIC='0', PP_STORE_WT=wt)
    script = SCRIPT % dict(repo=REPO, sizes=ADAM_SIZES, idle=ADAM_IDLE, lr=ADAM_LR, cases=STEP_CASES)
    subprocess.run([sys.executable, '-c', script, f], check=True, env=e, timeout=600)
    return dict(np.load(f))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('store_policy')
    return {wt: _run(d, wt) for wt in ('0', '1')}


@pytest.fixture(scope='module')
def oracle_refs(runs):
    """Loss and gradients of the step cases from the float64 oracle (the parameters are the same in both runs)."""
    from oracle import ic_oracle as O
    refs = {}
    for H, B, seed in ORACLE_CASES:
        pre = 'param%d/' % H
        P = {k[len(pre):]: v.astype(np.float64) for k, v in runs['1'].items() if k.startswith(pre)}
        net = O.Net(P, ['obs0', 'obs1'], K=10)
        refs[(H, B)] = O.loss_and_grads(net, synthetic_gum_arrays(B, seed=seed), ['mu'], ['Normal'])
    return refs


def test_adam_stores_the_same_bits_under_both_policies(runs):
    a, b = runs['0'], runs['1']
    for call in range(3):
        for k in ('p', 'm', 'v', 'g', 'step'):
            key = 'adam_%s_after%d' % (k, call)
            assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key


@pytest.mark.parametrize('wt', ['0', '1'])
def test_adam_matches_the_oracle_under_both_policies(runs, wt):
    """Two steps against ic_oracle.adam_step (tolerance of tests/test_gpu_optim.py), then the skipped call: nothing moves,
    no step is counted, the gradients are cleared all the same."""
    from oracle import ic_oracle as O
    r = runs[wt]
    chunks = [(s + 1023) // 1024 for s in ADAM_SIZES]
    offs = [1024 * sum(chunks[:t]) for t in range(len(ADAM_SIZES))]
    P = r['adam_p0'].astype(np.float64)
    M, V = np.zeros_like(P), np.zeros_like(P)
    # the betas reach the device as C floats: the oracle gets those values (1 - 0.999 differs from 1 - float32(0.999) by 1.3e-5
    # of itself, and exp_avg_sq is that factor times g^2 after one step)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for call in range(2):
        g = r['adam_g%d' % call].astype(np.float64)
        for t, s in enumerate(ADAM_SIZES):
            sl = slice(offs[t], offs[t] + s)
            O.adam_step(P[sl], g[sl], M[sl], V[sl], call + 1, ADAM_LR, beta1=b1, beta2=b2)
        for t, s in enumerate(ADAM_SIZES):
            sl = slice(offs[t], offs[t] + s)
            worst = float(np.abs(r['adam_p_after%d' % call][sl] - P[sl]).max() / max(np.abs(P[sl]).max(), 1e-12))
            assert worst < 3e-6, (call, t, worst)
            if t != ADAM_IDLE:
                assert rel_err(r['adam_m_after%d' % call][sl], M[sl]) < 3e-6, (call, t)
                assert rel_err(r['adam_v_after%d' % call][sl], V[sl]) < 3e-6, (call, t)
        assert not r['adam_g_after%d' % call].any()                      # consumed gradients were cleared
        assert (r['adam_step_after%d' % call] == call + 1).all()
    idle = slice(offs[ADAM_IDLE], offs[ADAM_IDLE] + 1024 * chunks[ADAM_IDLE])
    for call in range(3):      # the tensor without a gradient: parameters untouched, moments still zero
        assert np.array_equal(r['adam_p_after%d' % call][idle], r['adam_p0'][idle])
        assert not r['adam_m_after%d' % call][idle].any() and not r['adam_v_after%d' % call][idle].any()
    for k in ('p', 'm', 'v', 'step'):                                    # the skipped call
        assert np.array_equal(r['adam_%s_after2' % k], r['adam_%s_after1' % k]), k
    assert r['adam_g2'].any() and not r['adam_g_after2'].any()


@pytest.mark.parametrize('H,B', [(h, b) for h, b, _ in STEP_CASES])
def test_step_rows_are_bitwise_equal_under_both_policies(runs, H, B):
    """Per-row log_prob and the status word involve no atomics: the same bits. (The loss and the gradients go through float
    atomics: they are held against the oracle below.)"""
    tag = 'h%d_b%d' % (H, B)
    a, b = runs['0'], runs['1']
    assert a[tag + '_lp'].shape == (B,)
    assert np.array_equal(a[tag + '_lp'].view(np.int32), b[tag + '_lp'].view(np.int32)), tag
    assert int(a[tag + '_status'][0]) == int(b[tag + '_status'][0]) == 0, tag


@pytest.mark.parametrize('wt', ['0', '1'])
@pytest.mark.parametrize('H,B', [(h, b) for h, b, _ in ORACLE_CASES])
def test_step_matches_the_oracle_under_both_policies(runs, oracle_refs, H, B, wt):
    """The comparison of tests/test_gpu_panel.py test_panel_kernel_against_the_oracle, same helpers and bounds."""
    from pyprob_amd.spec import NetSpec
    spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=H)
    spec.add_address('mu', 'Normal')
    r, ref = runs[wt], oracle_refs[(H, B)]
    tag = 'h%d_b%d' % (H, B)
    loss = float(r[tag + '_loss'][0])
    print(tag, 'wt', wt, 'loss', loss, 'oracle', ref['loss'])
    assert abs(loss - ref['loss']) <= 2e-5 * abs(ref['loss'])
    for n, (off, shape) in spec.tensors.items():
        if np.abs(ref['grads'][n]).max() > 1e-7:
            g = r[tag + '_grads'][off:off + int(np.prod(shape))].reshape(shape)
            grad_check('store_policy_wt%s_%s/%s' % (wt, tag, n), g, ref['grads'][n], 5e-6)


def test_training_steps_agree_under_both_policies(runs):
    """Three Adam steps from the same initial state (the loss trajectory, compared like run_losses of tests/test_gpu_panel.py)."""
    a, b = runs['0']['run_losses'], runs['1']['run_losses']
    assert a.shape == (3,) and np.isfinite(a).all() and np.isfinite(b).all()
    np.testing.assert_allclose(b, a, rtol=2e-4, atol=2e-5)
