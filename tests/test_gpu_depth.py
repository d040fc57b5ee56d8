"""The training step (pp_ic_loss with backward, Adam) against the float64 oracle where the suite had not run it: three and four
stacked LSTM layers, single-statement batches under a stacked LSTM, and the generic observe embedding (observe_embedding_fwd
layer by layer, obs_backward_generic) at depths 1..4 and at depth 2 outside the fused envelope. Cases, weights and batches:
tests/depth_cases.py. Every case compares the status word, the loss (2e-5 relative), the per-row log_prob and every gradient
tensor (helpers.GRAD_BAR of its largest element + the project's absolute floors; a tensor that is identically zero in the oracle
must be identically zero on the device). The `gumm4d` golden holds the same depths against the reference's own records."""
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_cases as D
from conftest import REPO, load_golden
from helpers import check_golden_step, first_launch_workgroups, rel_err
from oracle import ic_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def test_golden_gumm4d_loss_logprob_and_gradients():
    """tests/test_gpu_path.py::test_golden_loss_logprob_and_gradients, same body and bars, on the reference's records of
    nn.LSTM(I, 32, 4) with observe embeddings of depth 4 and 2."""
    check_golden_step('gumm4d', *load_golden('gumm4d')[:4])


@pytest.mark.parametrize('name', list(D.RAGGED))
def test_stacked_lstm_ragged_against_oracle(name):
    """lstm_backward at depth 3 and 4: dH / dH2 ping-pong, the tail launches, the stored dHp partials and dC shared by the layers,
    per-layer bias gradients and weight-gradient products in the grouped launch."""
    H, depth, B = D.RAGGED[name]
    eng, arrays, addresses, dists = D.build('ragged', H, depth, B)
    assert eng.spec.lstm_depth == depth and '_layers_lstm.weight_hh_l%d' % (depth - 1) in eng.spec.tensors
    pb, _, _ = D.step_against_oracle('depth_ragged_' + name, eng, arrays, addresses, dists, D.abs_floor('ragged'))
    assert pb.t_max >= 4      # a recurrence: W_hh of every layer gets a gradient
    if name.endswith('_tail'):     # the precondition of tests/test_gpu_tail.py: the late time steps run in the tail launches
        assert os.environ.get('PP_LSTM_TAIL', '1') != '0'
        assert pb.t_max >= 4 and pb.n_active[-1] <= 8, (pb.t_max, list(pb.n_active))


@pytest.mark.parametrize('name', list(D.SINGLE))
def test_stacked_lstm_single_statement_against_oracle(name):
    """T = 1 with more than one LSTM layer: plan_step keeps the compact rows and dX as split partials, and turns off the lean
    cell, the fused cell backward and both panel kernels. W_hh of every layer has no gradient: exactly zero on the device."""
    H, depth, B = D.SINGLE[name]
    eng, arrays, addresses, dists = D.build('single', H, depth, B)
    assert int(arrays['trace_len'].max()) == 1 and eng.spec.lstm_depth == depth >= 2
    D.step_against_oracle('depth_single_' + name, eng, arrays, addresses, dists, D.abs_floor('single'))
    g = eng.grad_dict()
    for l in range(depth):
        assert not np.any(g['_layers_lstm.weight_hh_l%d' % l]), l
        assert np.any(g['_layers_lstm.weight_ih_l%d' % l]), l


def test_three_addresses_single_statement_depth3_against_oracle():
    """Three addresses of two families in one single-statement batch at depth 3 (H = 64, B = 100): without the fused cell backward
    the per-address group sums of dG come from the column-sum jobs of input_backward."""
    eng, arrays, addresses, dists = D.build('multi', 64, 3, 100)
    assert len(np.unique(arrays['addr_idx'])) == 3
    D.step_against_oracle('depth_multi_h64_d3_b100', eng, arrays, addresses, dists, D.abs_floor('multi'))


def test_one_workspace_large_small_large_depth4_against_oracle():
    """One engine, one workspace at (256, 4): ragged B = 300, single statements B = 17, ragged B = 40 - a stale dH / dH2 / dHp
    row of the larger batch read by a smaller one shows up against the oracle."""
    H, depth, batches = D.SEQUENCE
    eng = D.engine('ragged', H, depth)
    for k, (kind, B) in enumerate(batches):
        arrays, addresses, dists = D.batch(eng, kind, B, seed=10 * k)
        D.step_against_oracle('depth_sequence_h256_d4_%d_%s_b%d' % (k, kind, B), eng, arrays, addresses, dists, D.abs_floor(kind))
        if k == 0:
            shape = eng.ws_shape
    assert eng.ws_shape == shape      # the later batches ran in the first one's workspace


@pytest.mark.parametrize('kind', ['single', 'ragged'])
@pytest.mark.parametrize('name', list(D.EMBEDDINGS))
def test_generic_observe_embedding_against_oracle(name, kind):
    """The layer-by-layer observe embedding and its backward at H = 64, B = 130, on a single-statement and on a ragged batch."""
    emb = D.EMBEDDINGS[name]
    eng, arrays, addresses, dists = D.build(kind, 64, 1, 130, emb=emb)
    assert [eng.spec.obs_depth[o[0]] for o in eng.spec.obs] == [n for _, n in emb] and eng.spec.e_obs == sum(d for d, _ in emb)
    D.step_against_oracle('depth_embed_%s_%s' % (name, kind), eng, arrays, addresses, dists, D.abs_floor(kind))


def test_generic_embedding_takes_the_step_off_the_panel_path():
    """(512, depth 1, B = 40) single statements would run on the 16-row panel kernel behind the fused first launch; with
    embeddings of depth 4 and 2 the step must take the generic path instead. Observed, not assumed: the fused first launch
    stamps its workgroups in the trace (mode 4) - none with the deep embedding, some with the default one on the same batch."""
    eng, arrays, addresses, dists = D.build(*D.EMB_H512)
    pb, _, _ = D.step_against_oracle('depth_embed_d4_d2_h512_b40', eng, arrays, addresses, dists, D.abs_floor('single'))
    assert first_launch_workgroups(eng, pb) == 0
    control = D.engine('single', 512, 1)
    assert first_launch_workgroups(control, D.packed(arrays, control.spec).to(control.device)) > 0


def test_generic_embedding_feedforward_network_against_oracle():
    """network='feedforward' with embeddings of depth 3 and 1 on a ragged batch: the heads read Hs rows gathered from E
    (in_place is off), the embedding's gradient sums over each trace's time steps."""
    eng, arrays, addresses, dists = D.build(*D.EMB_FF)
    assert eng.spec.feedforward and eng.spec.lstm_dim == 0
    D.step_against_oracle('depth_embed_ff_d3_d1_ragged', eng, arrays, addresses, dists, D.abs_floor('ragged', 'feedforward'))


def test_generic_embedding_under_three_lstm_layers_against_oracle():
    """Depth-4 and depth-2 embeddings under three LSTM layers, ragged B = 130: both generic backward passes in one step."""
    eng, arrays, addresses, dists = D.build(*D.EMB_LSTM3)
    D.step_against_oracle('depth_embed_d4_d2_lstm3_ragged', eng, arrays, addresses, dists, D.abs_floor('ragged'))


# ---- PP_DETERMINISTIC=1 (read once per process: a child process, as tests/test_gpu_holes.py) --------------------------------------
DET_CASES = (('ragged', 64, 4, 130, None), ('single', 512, 2, 40, None), ('single', 64, 1, 130, D.EMBEDDINGS['d4_d2']))
DET_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
import depth_cases as D
out = {}
for k, (kind, H, depth, B, emb) in enumerate(%(cases)r):
    eng, arrays, addresses, dists = D.build(kind, H, depth, B, emb=emb)
    for rep in range(2):
        _, loss, grads = D.step_against_oracle('depth_det_%%d_%%d' %% (k, rep), eng, arrays, addresses, dists, D.abs_floor(kind))
        out['loss_%%d_%%d' %% (k, rep)] = np.array([loss], np.float32)
        out['grads_%%d_%%d' %% (k, rep)] = grads
np.savez(sys.argv[1], **out)
'''


def test_deterministic_mode_is_bitwise_repeatable_and_matches_the_oracle(tmp_path):
    """PP_DETERMINISTIC=1 at (64, 4) ragged, (512, 2) single statements and the depth-4 / depth-2 embedding: each case twice in one
    process - both runs within the bars of the oracle (the child asserts them), loss and gradients bit-equal. The bias gradients
    of every LSTM layer then come from the per-layer column-sum job on Gl[l]."""
    f = str(tmp_path / 'det.npz')
    r = subprocess.run([sys.executable, '-c', DET_SCRIPT % dict(repo=REPO, cases=DET_CASES), f],
                       env=dict(os.environ, PP_DETERMINISTIC='1'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = dict(np.load(f))
    for k in range(len(DET_CASES)):
        assert np.array_equal(d['loss_%d_0' % k].view(np.int32), d['loss_%d_1' % k].view(np.int32)), k
        assert np.array_equal(d['grads_%d_0' % k].view(np.int32), d['grads_%d_1' % k].view(np.int32)), k
        assert np.any(d['grads_%d_0' % k])


# ---- training steps: the live-chunk Adam plan over four LSTM layers and four embedding layers ------------------------------------
def _train_steps_track_the_oracle(eng, batches):
    """tests/test_gpu_path.py::test_train_steps_track_the_oracle, same comparison and bounds: the loss of every step within 1e-4
    of the oracle's on the oracle's own float64 trajectory, the parameters after the last step within 5e-3."""
    P = {k: v.numpy().astype(np.float64) for k, v in eng.state_dict().items()}
    M = {k: np.zeros_like(v) for k, v in P.items()}
    V = {k: np.zeros_like(v) for k, v in P.items()}
    names = list(eng.spec.tensors.keys())
    steps = dict.fromkeys(names, 0)
    for step, (arrays, addresses, dists) in enumerate(batches, 1):
        pb = D.packed(arrays, eng.spec).to(eng.device)
        act = eng.spec.active_mask(pb.cur_counts, pb.prev_counts)
        l = float(eng.train_step(pb, lr=1e-3).item())
        out = D.oracle_run(eng.spec, P, arrays, addresses, dists)
        print('step', step, 'loss', l, 'oracle', out['loss'])
        assert abs(l - out['loss']) < 1e-4 * abs(out['loss']), (step, l, out['loss'])
        for i, n in enumerate(names):
            if act[i]:
                steps[n] += 1
                O.adam_step(P[n], out['grads'][n], M[n], V[n], steps[n], 1e-3)
    assert int(eng.status_buf[0].item()) == 0
    sd = eng.state_dict()
    assert max(rel_err(sd[n].numpy(), P[n]) for n in names) < 5e-3
    assert [int(s) for s in eng.tensor_step.cpu().numpy()] == [steps[n] for n in names]


def test_train_steps_depth4_deep_embedding_track_the_oracle():
    """Three Adam steps at (64, 4) with embeddings of depth 4 and 2 on a ragged B = 130."""
    eng, arrays, addresses, dists = D.build(*D.TRAIN_D4)
    _train_steps_track_the_oracle(eng, [(arrays, addresses, dists)] * 3)


def test_train_steps_depth3_single_statements_track_the_oracle():
    """Three Adam steps at (512, 3) on single-statement batches of B = 130, 17 and 130."""
    H, depth, sizes = D.TRAIN_SINGLE
    eng = D.engine('single', H, depth)
    _train_steps_track_the_oracle(eng, [D.batch(eng, 'single', B, seed=k) for k, B in enumerate(sizes)])
