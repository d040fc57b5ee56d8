"""PP_FIRST_EARLY (csrc/obs_embed.hip): the embedding workgroups of the step's first launch load the observation at entry, stage
the weight matrices through 16-byte loads and store a trace's results behind its last dense layer (default, 1) or run in the
order they had before (0). The arithmetic is the same in the same order, so every value the launch writes must be bit for bit the same: the
per-row log_prob on the default path (and with it every term of the loss, whose atomic sum does not repeat to the last bit
even within one setting: it is held against the float64 sum of the rows), the loss and every gradient tensor under
PP_DETERMINISTIC=1 (no atomics: this pins the
saved activations cat, f1, obs_h, E and the X rows, which have no accessor of their own), ragged rows, the kernel's template
and width edges, and the particles of a lock-step posterior. One subprocess per setting and mode; all run the same cases in
the same order through the same workspaces. The default setting is also held against the float64 oracle (the bars of
tests/test_gpu_store_policy.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grad_check, synthetic_gum_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# GUM, H = 512, rows in the order they run through ONE engine: one wave with work; a second workgroup with one trace; a full and
# a ragged panel; 1003 then 17 again (the stale rows of the longer batch must stay out); 1025: two traces per wave, the last
# wave partial (the observation of the next trace is loaded one iteration ahead); 2051: three traces per wave
GUM_ROWS = (1, 5, 16, 17, 1003, 17, 1025, 2051)
GUM_DET_ROWS = (17, 1025)
ORACLE_ROWS = (17, 1003)          # default mode, first occurrence
# template and width edges (B = 17, PP_DETERMINISTIC=1): one observable (NOBS = 1); three (NOBS = 4, one slot empty); an
# observable of input width 8 (the widest the fused kernel takes) next to one of width 3
EDGE_SPECS = (('one', (('o0', 32, 2),)), ('three', (('o0', 16, 1), ('o1', 16, 1), ('o2', 32, 1))),
              ('wide', (('o0', 32, 8), ('o1', 32, 3))))
RAGGED_H = 64                     # the smallest lstm_dim of the ragged cases in tests/test_gpu_compact.py

SCRIPT = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
from helpers import synthetic_gum_arrays, synthetic_gumm_arrays
from pyprob_amd.engine import ICEngine
from pyprob_amd.packed import PackedBatch
from pyprob_amd.spec import NetSpec
det = os.environ.get('PP_DETERMINISTIC') == '1'
out = {}

def gum_batch(B, seed, obs=None):
    arr = synthetic_gum_arrays(B, seed=seed)
    return PackedBatch.from_ragged(arr['trace_len'], arr['addr_idx'], arr['values'], arr['prior'], arr['obs'] if obs is None else obs, 1)

def record(tag, eng, pb, grads):
    l, lp = eng.loss(pb.to(eng.device), backward=True, keep_lp=True)
    torch.cuda.synchronize()
    out[tag + '_loss'] = l.cpu().numpy()
    out[tag + '_lp'] = lp.cpu().numpy()
    out[tag + '_status'] = eng.status_buf[:1].cpu().numpy()
    if grads:
        out[tag + '_grads'] = eng.grads.cpu().numpy()

# ---- GUM, H = 512 ----
spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=512)
spec.add_address('mu', 'Normal')
eng = ICEngine(spec, device='cuda:0', seed=11)
for name, t in eng.state_dict().items():
    out['param/' + name] = t.numpy()
for k, B in enumerate(%(det_rows)r if det else %(rows)r):
    record('gum%%d_b%%d' %% (k, B), eng, gum_batch(B, 40 + k), grads=True)
if not det:      # forward only: the launch does not clear dX
    l, lp = eng.loss(gum_batch(17, 60).to(eng.device), backward=False, keep_lp=True)
    torch.cuda.synchronize()
    out['gumfwd_b17_loss'] = l.cpu().numpy()
    out['gumfwd_b17_lp'] = lp.cpu().numpy()

# ---- ragged rows ----
arr, addresses = synthetic_gumm_arrays(37, seed=9, max_iter=6)
spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=%(ragged_h)d)
for a in addresses: spec.add_address(a, 'Uniform')
eng = ICEngine(spec, device='cuda:0', seed=8)
ids = np.array([spec.address_id[addresses[j]] for j in arr['addr_idx']])
pb = PackedBatch.from_ragged(arr['trace_len'], ids, arr['values'], arr['prior'], arr['obs'], len(spec.addresses))
record('ragged', eng, pb, grads=True)

if det:
    # ---- template and width edges ----
    for name, obs_spec in %(edges)r:
        spec = NetSpec({n: {'dim': d, 'input_dim': w} for n, d, w in obs_spec}, lstm_dim=512)
        spec.add_address('mu', 'Normal')
        eng = ICEngine(spec, device='cuda:0', seed=21)
        width = sum(w for _, _, w in obs_spec)
        obs = np.random.default_rng(77).standard_normal((17, width)).astype(np.float32) * 2.0 + 3.0
        record('edge_' + name, eng, gum_batch(17, 70, obs=obs), grads=True)
    # ---- the first statement of a lock-step posterior (training repeats bit for bit in this mode, so the networks are equal) ----
    from models import GaussianWithUnknownMean
    from pyprob_amd.state import InferenceEngine, InferenceNetwork
    torch.manual_seed(3)
    model = GaussianWithUnknownMean()
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=256, batch_size=128, lstm_dim=64, seed=1,
                                  observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}})
    post = model.posterior_results(300, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe={'obs0': 8, 'obs1': 9},
                                   lock_step=True, seed=11)
    out['is_values'] = post._all_values.cpu().numpy()
    out['is_lw'] = post._all_log_weights.cpu().numpy()
np.savez(sys.argv[1], **out)
'''


def _run(tmp_path, early, det):
    f = str(tmp_path / ('early%s_det%s.npz' % (early, det)))
    e = dict(os.environ, PP_DETERMINISTIC=det, PP_FIRST_EARLY=early)
    script = SCRIPT % dict(repo=REPO, rows=GUM_ROWS, det_rows=GUM_DET_ROWS, edges=EDGE_SPECS, ragged_h=RAGGED_H)
    subprocess.run([sys.executable, '-c', script, f], check=True, env=e, timeout=600)
    return dict(np.load(f))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('first_launch')
    return {(early, det): _run(d, early, det) for det in ('0', '1') for early in ('0', '1')}


def _same_bits(a, b, key):
    assert a[key].shape == b[key].shape, key
    assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key


def _loss_is_the_mean_of_the_rows(r, tag, n_traces):
    """Default mode: the step adds the rows' log_prob into the loss slots with float atomics, in an order that differs from run
    to run, so the loss of one and the same setting repeats only to the last bit (B = 1003: 2.2279842 / 2.227984 in two runs).
    Its terms are pinned bit for bit by `log_prob`; the sum is held against their float64 sum with the bar the oracle
    comparisons of this suite use for a loss (2e-5)."""
    ref = -float(r[tag + '_lp'].astype(np.float64).sum()) / n_traces
    loss = float(r[tag + '_loss'][0])
    print(tag, 'loss', loss, 'float64 sum of the rows', ref)
    assert abs(loss - ref) <= 2e-5 * abs(ref), (tag, loss, ref)


@pytest.mark.parametrize('k,B', list(enumerate(GUM_ROWS)))
def test_default_path_is_bitwise_equal_under_both_orders(runs, k, B):
    a, b = runs[('0', '0')], runs[('1', '0')]
    tag = 'gum%d_b%d' % (k, B)
    assert a[tag + '_lp'].shape == (B,)
    _same_bits(a, b, tag + '_lp')
    _loss_is_the_mean_of_the_rows(a, tag, B)
    _loss_is_the_mean_of_the_rows(b, tag, B)
    assert int(a[tag + '_status'][0]) == int(b[tag + '_status'][0]) == 0, tag


def test_forward_only_call_is_bitwise_equal_under_both_orders(runs):
    a, b = runs[('0', '0')], runs[('1', '0')]
    assert a['gumfwd_b17_lp'].shape == (17,)
    _same_bits(a, b, 'gumfwd_b17_lp')
    _loss_is_the_mean_of_the_rows(a, 'gumfwd_b17', 17)
    _loss_is_the_mean_of_the_rows(b, 'gumfwd_b17', 17)


@pytest.mark.parametrize('k,B', list(enumerate(GUM_DET_ROWS)))
def test_deterministic_mode_gradients_are_bitwise_equal_under_both_orders(runs, k, B):
    """Full-width rows (addr[b] and the table columns) and every gradient tensor: the saved activations are their operands."""
    a, b = runs[('0', '1')], runs[('1', '1')]
    tag = 'gum%d_b%d' % (k, B)
    assert np.abs(a[tag + '_grads']).max() > 0
    for key in ('_loss', '_lp', '_grads'):
        _same_bits(a, b, tag + key)


@pytest.mark.parametrize('det', ['0', '1'])
def test_ragged_rows_are_bitwise_equal_under_both_orders(runs, det):
    a, b = runs[('0', det)], runs[('1', det)]
    assert np.isfinite(a['ragged_loss']).all() and a['ragged_lp'].size >= 37
    _same_bits(a, b, 'ragged_lp')
    if det == '1':
        _same_bits(a, b, 'ragged_loss')
        _same_bits(a, b, 'ragged_grads')
    else:
        _loss_is_the_mean_of_the_rows(a, 'ragged', 37)
        _loss_is_the_mean_of_the_rows(b, 'ragged', 37)


@pytest.mark.parametrize('name', [n for n, _ in EDGE_SPECS])
def test_template_and_width_edges_are_bitwise_equal_under_both_orders(runs, name):
    a, b = runs[('0', '1')], runs[('1', '1')]
    tag = 'edge_' + name
    assert np.isfinite(a[tag + '_loss']).all() and np.abs(a[tag + '_grads']).max() > 0
    for key in ('_loss', '_lp', '_grads'):
        _same_bits(a, b, tag + key)


def test_posterior_particles_are_bitwise_equal_under_both_orders(runs):
    a, b = runs[('0', '1')], runs[('1', '1')]
    assert a['is_values'].shape[0] == 300 and np.isfinite(a['is_lw']).all()
    _same_bits(a, b, 'is_values')
    _same_bits(a, b, 'is_lw')


@pytest.fixture(scope='module')
def oracle_refs(runs):
    from oracle import ic_oracle as O
    r = runs[('1', '0')]
    P = {k[len('param/'):]: v.astype(np.float64) for k, v in r.items() if k.startswith('param/')}
    net = O.Net(P, ['obs0', 'obs1'], K=10)
    return {B: O.loss_and_grads(net, synthetic_gum_arrays(B, seed=40 + GUM_ROWS.index(B)), ['mu'], ['Normal']) for B in ORACLE_ROWS}


@pytest.mark.parametrize('B', ORACLE_ROWS)
def test_early_order_matches_the_oracle(runs, oracle_refs, B):
    """The comparison of tests/test_gpu_store_policy.py test_step_matches_the_oracle_under_both_policies, same helpers and bounds."""
    from pyprob_amd.spec import NetSpec
    spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=512)
    spec.add_address('mu', 'Normal')
    r, ref = runs[('1', '0')], oracle_refs[B]
    tag = 'gum%d_b%d' % (GUM_ROWS.index(B), B)
    loss = float(r[tag + '_loss'][0])
    print(tag, 'loss', loss, 'oracle', ref['loss'])
    assert abs(loss - ref['loss']) <= 2e-5 * abs(ref['loss'])
    for n, (off, shape) in spec.tensors.items():
        if np.abs(ref['grads'][n]).max() > 1e-7:
            g = r[tag + '_grads'][off:off + int(np.prod(shape))].reshape(shape)
            grad_check('first_launch_%s/%s' % (tag, n), g, ref['grads'][n], 5e-6)
