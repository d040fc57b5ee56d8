"""The cases of tests/test_gpu_depth.py: the training step at LSTM depth 3-4, single-statement batches under a stacked LSTM
and the generic (layer by layer) observe embedding, each held against the float64 oracle. Shared between the tests, the
PP_DETERMINISTIC=1 child process of the suite and the CPU check that the ReLU-kink filter leaves enough traces
(tests/test_oracle_depth.py), so that all three build the same network and the same batch.

Every case uses trained-looking weights (helpers.trained_looking) and B traces out of B + 64 candidates that lie away from the
ReLU kinks of the proposal layers (helpers.away_from_relu_kinks)."""
import numpy as np

from helpers import (GRAD_ABS_RAGGED, GRAD_ABS_RAGGED_TRAINED, GRAD_ABS_UNIFORM_TRAINED, away_from_relu_kinks, check_grads,
                     check_lp, fresh_engine, oracle_lp_rows, oracle_run, packed, single_statement_arrays, synthetic_gum_arrays,
                     synthetic_gumm_arrays, trained_looking, unpack_lp)

# (H, lstm_depth, B): ragged Marsaglia batches, max_iter = 5, every 53rd value outside the support
RAGGED = {
    'h64_d3_b130': (64, 3, 130),       # the first depth at which lstm_backward swaps dH / dH2 both ways
    'h64_d4_b130': (64, 4, 130),       # ... and swaps back: layer 0 reads w.dH again
    'h256_d4_b300_tail': (256, 4, 300),   # the LSTM tail launches (tests/test_gpu_tail.py's shape) of four layers
    'h512_d3_b130_dhp': (512, 3, 130),    # dh_{t-1} as stored split partials (w.dHp), shared by the three layers
    'h256_d3_b300': (256, 3, 300),
}
# (H, lstm_depth, B): single-statement batches of one Normal address. p.L > 1: no lean cell, no fused cell backward, no panel;
# dX still as stored split partials and compact input rows
SINGLE = {
    'h512_d2_b40': (512, 2, 40),
    'h512_d4_b130': (512, 4, 130),
    'h64_d3_b17': (64, 3, 17),
    'h1024_d2_b40': (1024, 2, 40),
}
# observe embeddings as ((dim, depth), ...) per observable: all outside obs_fused_supported, so observe_embedding_fwd runs
# layer by layer and obs_backward_generic follows the step's grouped launch
EMBEDDINGS = {
    'd4_d2': ((32, 4), (16, 2)),          # depth 4: both scratch buffers (w.dObsH / w.dObsH2) and obs_hl[o][2]
    'd1_d3': ((32, 1), (32, 3)),
    'd4_d4': ((16, 4), (16, 4)),
    'one_obs_hid64': ((128, 2),),         # depth 2, but 64 hidden units in one observable
    'e_obs128': ((64, 2), (64, 2)),       # depth 2, but e_obs = 128
}


EMB_H512 = ('single', 512, 1, 40, EMBEDDINGS['d4_d2'], 'lstm')            # would take the panel kernel with a fused embedding
EMB_FF = ('ragged', 64, 1, 130, ((32, 3), (16, 1)), 'feedforward')       # Hs rows gathered from E: in_place is off
EMB_LSTM3 = ('ragged', 64, 3, 130, EMBEDDINGS['d4_d2'], 'lstm')
SEQUENCE = (256, 4, (('ragged', 300), ('single_a0', 17), ('ragged', 40)))   # one engine, one workspace
TRAIN_D4 = ('ragged', 64, 4, 130, EMBEDDINGS['d4_d2'], 'lstm')
TRAIN_SINGLE = (512, 3, (130, 17, 130))


def all_builds():
    """{label: (kind, H, lstm_depth, B, embeddings or None, network)} of every case that build() serves."""
    cases = {'ragged_' + n: ('ragged', H, d, B, None, 'lstm') for n, (H, d, B) in RAGGED.items()}
    cases.update({'single_' + n: ('single', H, d, B, None, 'lstm') for n, (H, d, B) in SINGLE.items()})
    cases['multi_h64_d3_b100'] = ('multi', 64, 3, 100, None, 'lstm')
    for n, emb in EMBEDDINGS.items():
        for kind in ('single', 'ragged'):
            cases['embed_%s_%s' % (n, kind)] = (kind, 64, 1, 130, emb, 'lstm')
    cases.update(embed_h512=EMB_H512, embed_ff=EMB_FF, embed_lstm3=EMB_LSTM3, train_d4=TRAIN_D4)
    return cases


def obs_of(emb):
    return {'obs%d' % i: {'dim': d, 'depth': n} for i, (d, n) in enumerate(emb)}


def multi_arrays(n):
    """Single-statement traces of three addresses and two distribution types (the `multi` batch of tests/test_gpu_compact.py)."""
    arr = synthetic_gum_arrays(n, seed=7)
    rng = np.random.default_rng(11)
    arr['addr_idx'] = rng.integers(0, 3, n).astype(np.int32)
    uni = arr['addr_idx'] == 1
    arr['values'][uni] = rng.uniform(-1, 1, int(uni.sum())).astype(np.float32)
    arr['prior'][uni] = np.array([-1.0, 1.0], np.float32)
    return arr


MULTI_ADDRS = (('a0', 'Normal', None), ('a1', 'Uniform', None), ('a2', 'Normal', None))


def candidates(kind, B, n_obs=2, seed=0):
    """(arrays of B candidate traces, addresses, distribution names) of a batch kind: 'ragged', 'single' (one Normal address),
    'multi', or 'single_a0' (single statements at the first address of the ragged program)."""
    if kind == 'ragged':
        arrays, addresses = synthetic_gumm_arrays(B, seed=4 + seed, max_iter=5)
        arrays['values'][::53] = 1.25           # outside U(-1, 1): rescued rows
        dists = ['Uniform'] * len(addresses)
    elif kind == 'single':
        arrays, addresses, dists = single_statement_arrays(B, 'Normal', seed=B + seed), ['mu'], ['Normal']
    elif kind == 'multi':
        arrays, addresses, dists = multi_arrays(B), [a for a, _, _ in MULTI_ADDRS], [d for _, d, _ in MULTI_ADDRS]
    elif kind == 'single_a0':
        _, addresses = synthetic_gumm_arrays(1, seed=0, max_iter=5)
        arrays = synthetic_gum_arrays(B, seed=77 + seed)
        arrays['values'] = np.clip(arrays['values'], -0.99, 0.99)
        arrays['prior'] = np.tile(np.array([[-1.0, 1.0]], np.float32), (B, 1))
        dists = ['Uniform'] * len(addresses)
    else:
        raise ValueError(kind)
    arrays['obs'] = np.ascontiguousarray(arrays['obs'][:, :n_obs])
    return arrays, addresses, dists


def engine(kind, H, depth, emb=None, network='lstm', device='cuda:0'):
    if kind == 'multi':
        eng = fresh_engine(H, [], None, lstm_depth=depth, extra=MULTI_ADDRS, obs=obs_of(emb) if emb else None, device=device)
    else:
        addresses = candidates(kind, 1)[1]
        eng = fresh_engine(H, addresses, 'Normal' if kind == 'single' else 'Uniform', lstm_depth=depth, network=network,
                           obs=obs_of(emb) if emb else None, device=device)
    return trained_looking(eng, seed=H + depth)


def batch(eng, kind, B, seed=0):
    """B traces of B + 64 candidates, away from the ReLU kinks under the engine's current weights - those of the embedding layers
    included: the generic path sums an embedding layer in another order than the oracle, and with the oracle alone 4 of these
    24 cases had a trace among their first B with an embedding unit inside KINK_MARGIN, the nearest at 1.2e-7 of its terms (the
    fp32 round-off of such a sum). The filter drops 0..3 of the candidates for it."""
    arrays, addresses, dists = candidates(kind, B + 64, n_obs=len(eng.spec.obs), seed=seed)
    return away_from_relu_kinks(eng, arrays, addresses, dists, B, embedding=True), addresses, dists


def build(kind, H, depth, B, emb=None, network='lstm', device='cuda:0'):
    eng = engine(kind, H, depth, emb, network, device)
    return (eng,) + batch(eng, kind, B)


def abs_floor(kind, network='lstm'):
    """The project's absolute floors (helpers.GRAD_ABS_*): ragged batches of trained-looking weights, the ragged FeedForward
    cases, single statements."""
    if kind == 'ragged':
        return GRAD_ABS_RAGGED if network == 'feedforward' else GRAD_ABS_RAGGED_TRAINED
    return GRAD_ABS_UNIFORM_TRAINED


def step_against_oracle(label, eng, arrays, addresses, dists, floor):
    """One loss + backward on the device against the oracle: status word, loss (2e-5 relative), per-row log_prob, every gradient
    tensor. Returns (packed batch, loss, flat gradients)."""
    import torch
    pb = packed(arrays, eng.spec).to(eng.device)
    l, lp = eng.loss(pb, backward=True, keep_lp=True)
    torch.cuda.synchronize()
    status, loss = int(eng.status_buf[0].item()), float(l.item())
    params = {k: v.numpy() for k, v in eng.state_dict().items()}
    out = oracle_run(eng.spec, params, arrays, addresses, dists)
    assert np.isfinite(out['loss']) and status == 0, (label, status, out['loss'])
    print(label, 'loss', loss, 'oracle', out['loss'])
    assert abs(loss - out['loss']) <= 2e-5 * abs(out['loss']), (label, loss, out['loss'])
    check_lp(unpack_lp(pb, lp.cpu().numpy()), oracle_lp_rows(out, arrays), label + '/lp')
    check_grads(label, eng, out, floor)
    return pb, loss, eng.grads.cpu().numpy().copy()
