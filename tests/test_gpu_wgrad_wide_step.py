"""The weight-gradient launch of a whole backward pass with its 16-byte loop (csrc/wgrad_t1.hip: float4 operand loads on
v_mfma_f32_16x16x4_f32, tile edges in units of 16, the b128 LDS epilogue; PP_WGRAD_WIDE=0 keeps the dword loop). Every named
gradient tensor of a backward pass against the float64 oracle (B = 37, B = 250) or against the switch-off run of the same tree
(B = 1003: three row ranges; B = 250 on the tile path, PP_PANEL=0, which queues other products; one ragged GUMM batch of 64
traces: the row gather of dW_hh and zero blocks that cover a prefix of the rows), at the bar tests/test_gpu_wgrad_jobs.py and
tests/test_gpu_panel.py use for these tensors (5e-6 of a tensor's largest element; measured there: 4.6e-7). Tensors that the
reference leaves at zero must be zero. A second, different minibatch through the same workspace must match its own reference.
One subprocess per environment; the switch is flipped inside it (it is read per launch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grad_check, synthetic_gum_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 5e-6

SCRIPT = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
from helpers import synthetic_gum_arrays, synthetic_gumm_arrays
from pyprob_amd.engine import ICEngine
from pyprob_amd.packed import PackedBatch
from pyprob_amd.spec import NetSpec
out = {}
for case in sys.argv[2].split(','):
    name, switches = case.split(':')
    for sw in switches:
        os.environ['PP_WGRAD_WIDE'] = sw
        spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=512)
        if name == 'gumm64':
            _, addresses = synthetic_gumm_arrays(8, seed=0, max_iter=6)
            for a in addresses:
                spec.add_address(a, 'Uniform')
            arrs = [synthetic_gumm_arrays(64, seed=s, max_iter=6)[0] for s in (4, 9)]
        else:
            B = int(name[1:])
            spec.add_address('mu', 'Normal')
            arrs = [synthetic_gum_arrays(B, seed=s) for s in (3 + B, 77 + B)]
        eng = ICEngine(spec, device='cuda:0', seed=5)
        for k, arr in enumerate(arrs):      # the second minibatch goes through the workspace the first one left behind
            pb = PackedBatch.from_ragged(arr['trace_len'], arr['addr_idx'], arr['values'], arr['prior'], arr['obs'],
                                         len(spec.addresses)).to(eng.device)
            l = eng.loss(pb, backward=True)
            torch.cuda.synchronize()
            assert int(eng.status_buf[0].item()) == 0
            out['%%s|%%s|%%d|loss' %% (name, sw, k)] = l.cpu().numpy()
            for n, g in eng.grad_dict().items():
                out['%%s|%%s|%%d|g|%%s' %% (name, sw, k, n)] = np.asarray(g)
        if sw == '1':
            for n, v in eng.state_dict().items():
                out['%%s|p|%%s' %% (name, n)] = v.numpy()
np.savez(sys.argv[1], **out)
'''


def _run(tmp_path, cases, **env):
    f = str(tmp_path / 'out.npz')
    e = dict(os.environ, PP_DETERMINISTIC='0', **env)
    e.pop('PP_WGRAD_WIDE', None)
    subprocess.run([sys.executable, '-c', SCRIPT % dict(repo=REPO), f, cases], check=True, env=e, timeout=600)
    return dict(np.load(f))


@pytest.fixture(scope='module')
def panel_run(tmp_path_factory):
    return _run(tmp_path_factory.mktemp('wgwide_panel'), 'g37:1,g250:1,g1003:10,gumm64:10')


@pytest.fixture(scope='module')
def tile_run(tmp_path_factory):
    return _run(tmp_path_factory.mktemp('wgwide_tiles'), 'g250:10', PP_PANEL='0')


def _grads(run, name, sw, k):
    pre = '%s|%s|%d|g|' % (name, sw, k)
    return {key[len(pre):]: v for key, v in run.items() if key.startswith(pre)}


def _check(label, got, ref):
    """Every named tensor: 5e-6 of its largest element; a tensor the reference leaves at zero must be zero."""
    assert got.keys() == ref.keys() and len(got) > 10
    for n in sorted(got):
        r = np.asarray(ref[n], np.float64)
        if not np.any(r):
            assert not np.any(got[n]), (label, n)
            continue
        err = grad_check('%s/%s' % (label, n), got[n], r, BAR)
        print('%s/%s: max |error| %.3e of max |gradient| %.3e' % (label, n, err, np.abs(r).max()))


def _same_loss(run, name, k):
    """The forward pass adds the rows' log_prob up with float atomics: two runs agree to rounding (the bar of
    tests/test_gpu_panel.py between two paths)."""
    a, b = float(run['%s|1|%d|loss' % (name, k)][0]), float(run['%s|0|%d|loss' % (name, k)][0])
    assert abs(a - b) <= 2e-6 * abs(b), (name, k, a, b)


def _biases_live(label, g):
    # b1 / b2 of the head, fin_b0 / fin_b1, obs_b0 / obs_b1 of both observables (a single statement has no previous sample:
    # the sample embedding's bias gets no gradient)
    names = [n for n in g if n.endswith('.bias') and ('_layers_proposal' in n or '_layers_observe_embedding' in n)]
    assert len(names) == 8, sorted(g)
    for n in names:
        assert np.any(g[n] != 0), (label, n)


@pytest.mark.parametrize('B', [37, 250])
def test_wide_loop_against_the_oracle(panel_run, B):
    from oracle import ic_oracle as O
    name = 'g%d' % B
    P = {k[len(name) + 3:]: v.astype(np.float64) for k, v in panel_run.items() if k.startswith(name + '|p|')}
    net = O.Net(P, ['obs0', 'obs1'], K=10)
    for k, seed in enumerate((3 + B, 77 + B)):
        ref = O.loss_and_grads(net, synthetic_gum_arrays(B, seed=seed), ['mu'], ['Normal'])
        loss = float(panel_run['%s|1|%d|loss' % (name, k)][0])
        assert abs(loss - ref['loss']) <= 2e-5 * abs(ref['loss'])
        g = _grads(panel_run, name, '1', k)
        _check('wgwide_%s_batch%d' % (name, k), g, {n: ref['grads'][n] for n in g})
        if B == 37:
            _biases_live(name, g)


@pytest.mark.parametrize('name', ['g1003', 'gumm64'])
def test_wide_loop_equals_the_dword_loop(panel_run, name):
    for k in range(2):
        _same_loss(panel_run, name, k)
        g = _grads(panel_run, name, '1', k)
        _check('wgwide_%s_batch%d' % (name, k), g, _grads(panel_run, name, '0', k))
        if name == 'g1003':
            _biases_live(name, g)


def test_wide_loop_on_the_tile_path(tile_run):
    for k in range(2):
        _same_loss(tile_run, 'g250', k)
        _check('wgwide_tiles_g250_batch%d' % k, _grads(tile_run, 'g250', '1', k), _grads(tile_run, 'g250', '0', k))
