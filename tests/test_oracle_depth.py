"""Pins the CPU oracle (oracle/ic_oracle.py) to the reference at the largest depths the engine accepts: the `gumm4d` records
(tests/golden/make_golden.py: the Marsaglia program, nn.LSTM(I, 32, 4), observe embeddings of depth 4 and 2). The loops of the
oracle over net.depth and over the layers of net.ff(...) are otherwise held to the reference at LSTM depth <= 2 and embedding
depths 3 / 1 only. The assertions are those of tests/test_oracle.py, called on this case. Below them, the cases of
tests/test_gpu_depth.py are built with the oracle alone: each must find its traces away from the ReLU kinks. CPU only."""
import numpy as np
import pytest

import depth_cases as D
import test_oracle as T
from conftest import load_golden
from helpers import packed


@pytest.fixture(scope='module')
def gumm4d():
    return ('gumm4d',) + load_golden('gumm4d')


def test_the_case_is_the_deep_one(gumm4d):
    case, meta, params, batch, loss, isr = gumm4d
    assert meta['lstm_depth'] == 4 and meta['lstm_dim'] == 32
    assert meta['observe_embedding_depths'] == {'obs0': 4, 'obs1': 2} and meta['observe_embedding_dims'] == {'obs0': 32, 'obs1': 16}
    assert '_layers_lstm.weight_hh_l3' in params and '_layers_observe_embedding.obs0._layers.3.weight' in params
    assert max(batch['trace_len']) >= 4 and len(meta['sub_batches']) > 1      # ragged: several sub-batches, a recurrence


def test_param_counts(gumm4d):
    T.test_param_counts(gumm4d)


def test_sub_batching_matches_reference(gumm4d):
    T.test_sub_batching_matches_reference(gumm4d)


def test_loss_forward_matches_reference(gumm4d):
    T.test_loss_forward_matches_reference(gumm4d)


def test_loss_forward_fp32_mode(gumm4d):
    T.test_loss_forward_fp32_mode(gumm4d)


def test_gradients_match_reference(gumm4d):
    T.test_gradients_match_reference(gumm4d)


def test_gradients_of_every_lstm_and_embedding_layer_match_reference(gumm4d):
    """The tensors this case is there for - four LSTM layers, embedding layers 0..3 and the tables - at the 5e-4 of the other
    goldens (measured: 2.8e-4 on the top layer's biases, below 1.5e-4 elsewhere); only the TruncatedNormal heads, whose
    gradients of 1e-6..1e-5 carry the record's own fp32 round-off, use the 1e-3 of gumm2 above."""
    case, meta, params, batch, loss, isr = gumm4d
    out = T._run(gumm4d)
    names = [n for n in meta['param_names'] if not n.startswith('_layers_proposal.')]
    assert sum(n.startswith('_layers_lstm.') for n in names) == 16
    assert sum(n.startswith('_layers_observe_embedding.') for n in names) == 12
    for n in names:
        i = meta['param_names'].index(n)
        ref = loss['g%d' % i]
        err = np.abs(out['grads'][n] - ref).max() / max(np.abs(ref).max(), 1e-6)
        assert err < 5e-4, (n, err)
        assert meta['has_grad'][i] or not np.any(out['grads'][n]), n


def test_is_log_weights_match_reference(gumm4d):
    T.test_is_log_weights_match_reference(gumm4d)


# ---- the cases of tests/test_gpu_depth.py, with the oracle alone --------------------------------------------------------------------
def _reaches(kind, depth, emb, arrays, pb):
    """What the case is there for, as far as the batch and the network decide it."""
    assert int(arrays['trace_len'].max()) == pb.t_max and (pb.t_max == 1) == (kind != 'ragged')
    if kind == 'ragged':
        assert pb.t_max >= 4 and pb.n_active[-1] <= 8      # a recurrence; few traces in the late time steps
        assert np.isin(1.25, arrays['values'])             # rescued rows
    if emb is not None:      # outside the fused envelope (obs_embed.hpp obs_fused_supported)
        hid = [(1 + d) // 2 for d, _ in emb]
        assert any(n != 2 for _, n in emb) or max(hid) > 32 or sum(hid) > 64 or sum(d for d, _ in emb) > 64


@pytest.mark.parametrize('label', list(D.all_builds()))
def test_kink_filter_keeps_enough_traces(label):
    """Every case finds its B traces among B + 64 candidates (the filter asserts it), on the host copy of the engine's buffers:
    the initial weights are the same on either device."""
    kind, H, depth, B, emb, network = D.all_builds()[label]
    eng, arrays, addresses, dists = D.build(kind, H, depth, B, emb=emb, network=network, device='cpu')
    assert len(arrays['trace_len']) == B
    _reaches(kind, depth, emb, arrays, packed(arrays, eng.spec))


def test_kink_filter_keeps_enough_traces_in_the_sequences():
    H, depth, batches = D.SEQUENCE
    eng = D.engine('ragged', H, depth, device='cpu')
    for k, (kind, B) in enumerate(batches):
        assert len(D.batch(eng, kind, B, seed=10 * k)[0]['trace_len']) == B
    H, depth, sizes = D.TRAIN_SINGLE
    eng = D.engine('single', H, depth, device='cpu')
    for k, B in enumerate(sizes):
        assert len(D.batch(eng, 'single', B, seed=k)[0]['trace_len']) == B
