"""The training step (pp_ic_loss with backward, Adam) against the float64 oracle at network dimensions off the grid the rest of
the suite uses: hidden sizes that are no multiple of 64 / 32 / 16 / 4 / 2, sample / address / distribution-type embedding widths
other than 4 / 64 / 8, and the panel widths with a W_ih row length other than 212. Every fused route of the engine stands behind a
predicate on these dimensions (restated in dim_cases.routes); here the routes behind them - the scalar GEMM stagers with ld = H,
full-width LSTM input rows by default, the atomic dh path, the per-step recurrence at a large H, the panel kernels at another
ldw - run on the device. Cases, weights and batches: tests/dim_cases.py. Every training step compares the status word, the loss
(2e-5 relative), the per-row log_prob and every gradient tensor (helpers.GRAD_BAR of its largest element + the project's absolute
floors; a tensor that is identically zero in the oracle must be identically zero on the device) through
depth_cases.step_against_oracle. No call may fail: pp_last_error is never consulted. The IS statement at these dimensions:
tests/test_gpu_is_step_fused.py."""
import numpy as np
import pytest

import depth_cases as D
import dim_cases as DC
from helpers import packed
from oracle import ic_oracle as O
from test_gpu_embed_envelope import error_text_not_consulted  # noqa: F401  (autouse: applies to every test of this module)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _step(label, name, kind, B):
    eng, arrays, addresses, dists = DC.build(name, kind, B)
    pb, _, _ = D.step_against_oracle('dims_' + label, eng, arrays, addresses, dists, D.abs_floor(kind))
    assert pb.n_traces == B and ((pb.t_max == 1) if kind == 'single' else (pb.t_max >= 4))
    return eng, pb


def _first_launch_trace(eng, pb):
    """(embedding workgroups, panel-image job workgroups) of the first launch of one more step: pp_debug_wgtrace mode 4 - an
    embedding workgroup leaves its end stamp in word 7, an address-bias job 1, a job that builds the panel kernels' weight
    images 2 (obs_embed.hip). The image jobs run exactly when plan_step chose a panel kernel."""
    from pyprob_amd import lib as L
    lib, cap = L.load(), 4096
    trace = torch.zeros(8 * cap, dtype=torch.int64, device=eng.device)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(trace.data_ptr(), cap, 4)
    try:
        eng.loss(pb, backward=True)
        torch.cuda.synchronize()
    finally:
        lib.pp_debug_wgtrace(None, 0, 0)
    t = trace.cpu().numpy().reshape(cap, 8)
    started = t[:, 0] > 0
    return int((started & (t[:, 7] > 2)).sum()), int((started & (t[:, 7] == 2)).sum())


def _kinds(names, ragged_only=()):
    return [(n, k) for n in names for k in ('single', 'ragged') if k == 'ragged' or n not in ragged_only]


@pytest.mark.parametrize('name,kind', _kinds(DC.HIDDEN, DC.HIDDEN_RAGGED_ONLY))
def test_hidden_sizes_against_oracle(name, kind):
    """Default embedding dims, B = 130. h96 / h48: compact rows without the lean cell and the fast input launch. h100: full-width
    rows by default, no cell epilogue in the recurrent product. h50 / h33: dh_{t-1} by atomics, every operand with ld = H on the
    scalar stagers, head hidden widths 40 / 31. h384: the lean cell on single statements, and on the ragged batch the per-step
    recurrence at a width that is neither a tail width nor small. h100_d2 / h50_d3: the same under stacked layers."""
    eng, pb = _step('%s_%s' % (name, kind), name, kind, DC.B_STEP)
    g = eng.grad_dict()
    for l in range(eng.spec.lstm_depth):
        assert np.any(g['_layers_lstm.weight_hh_l%d' % l]) == (kind == 'ragged'), l


@pytest.mark.parametrize('name,kind', _kinds(DC.EMBED))
def test_embedding_dims_against_oracle(name, kind):
    """H = 64 (all_odd: 33, three layers), B = 130: sample embeddings of 1 / 8 / 9 columns, address + distribution-type widths at
    and beyond both edges of compact_rows (ne = 2, 18, 71, 136)."""
    eng, pb = _step('%s_%s' % (name, kind), name, kind, DC.B_STEP)
    g = eng.grad_dict()
    smp = [n for n in eng.spec.tensors if n.startswith('_layers_sample_embedding.') and n.endswith('weight')]
    assert smp and all(g[n].shape[0] == DC.ALL[name][2] for n in smp)
    assert any(np.any(g[n]) for n in smp) == (kind == 'ragged')      # (a single statement has no previous value)


@pytest.mark.parametrize('name,B', [(n, B) for n in DC.PANEL for B in DC.PANEL_B[n]])
def test_panel_widths_against_oracle(name, B):
    """Single statements of one address at H = 512 / 1024 with compact rows kept on: the shapes plan_step hands to the panel
    kernels, with W_ih rows of 216 / 104 / 140 floats instead of 212. h512_smp3 (c2 = 67) has full-width rows: no lean cell, so
    the panels must step aside. Which way a step went is observed: the jobs that build a panel kernel's weight images ride in the
    first launch and stamp its trace."""
    eng, pb = _step('%s_single_b%d' % (name, B), name, 'single', B)
    panel = DC.routes(DC.ALL[name])['panel_dims']
    assert panel == (name != 'h512_smp3')
    _, image_jobs = _first_launch_trace(eng, pb)
    assert int(eng.status_buf[0].item()) == 0
    assert (image_jobs > 0) == panel, (name, B, image_jobs)


def test_one_workspace_large_small_large_at_h50_against_oracle():
    """One engine, one workspace at H = 50: ragged B = 300, single statements B = 17, ragged B = 40. round4(H) != H: a stale row of
    the larger batch in a buffer with a padded leading dimension, read by a smaller one, shows up against the oracle."""
    name, batches = DC.SEQUENCE
    eng = DC.engine(name, 'ragged')
    assert eng.spec.lstm_dim % 4 != 0
    for k, (kind, B) in enumerate(batches):
        arrays, addresses, dists = D.batch(eng, kind, B, seed=10 * k)
        D.step_against_oracle('dims_sequence_%s_%d_%s_b%d' % (name, k, kind, B), eng, arrays, addresses, dists, D.abs_floor(kind))
        if k == 0:
            shape = eng.ws_shape
    assert eng.ws_shape == shape      # the later batches ran in the first one's workspace


@pytest.mark.parametrize('name,kind', DC.ADAM)
def test_adam_steps_leave_padding_and_untouched_tensors_alone(name, kind):
    """Three train_step calls (loss, backward, the live-chunk Adam launch) on networks whose tensors end inside a 1024-float chunk
    at odd places, against O.adam_step fed with the gradients the device's own backward pass left (read just before the optimizer
    consumes them), at the bar of tests/test_gpu_optim.py: 3e-6 of a tensor's largest element. The padding behind every tensor
    and every tensor without a gradient stay bit-identical; step counts follow the presence map."""
    eng, arrays, addresses, dists = DC.build(name, kind, DC.B_STEP)
    spec = eng.spec
    names = list(spec.tensors)
    pb = packed(arrays, spec).to(eng.device)
    act = spec.active_mask(pb.cur_counts, pb.prev_counts)
    assert 0 < act.sum() < len(names)
    before = eng.params.cpu().numpy().copy()
    P = {k: v.numpy().astype(np.float64) for k, v in eng.state_dict().items()}
    M = {k: np.zeros_like(v) for k, v in P.items()}
    V = {k: np.zeros_like(v) for k, v in P.items()}
    seen, real = [], eng.optimizer_step

    def optimizer_step(*args, **kwargs):
        seen.append(eng.grad_dict())
        return real(*args, **kwargs)
    eng.optimizer_step = optimizer_step
    for step in range(1, 4):
        eng.train_step(pb, DC.ADAM_LR)
        torch.cuda.synchronize()
        assert int(eng.status_buf[0].item()) == 0 and len(seen) == step
        for i, n in enumerate(names):
            if act[i]:
                O.adam_step(P[n], seen[-1][n].astype(np.float64), M[n], V[n], step, DC.ADAM_LR)
        sd = eng.state_dict()
        worst = max(float(np.abs(sd[n].numpy() - P[n]).max() / max(np.abs(P[n]).max(), 1e-12)) for n in names)
        print('dims_adam', name, kind, 'step', step, 'worst', worst)
        assert worst < 3e-6, (step, worst)
    after = eng.params.cpu().numpy()
    pad = np.ones(spec.n_params, bool)
    for i, (n, (off, shape)) in enumerate(spec.tensors.items()):
        size = int(np.prod(shape))
        pad[off:off + size] = False
        if act[i]:      # (W_hh of a single-statement batch: a gradient of zeros, no movement)
            assert np.array_equal(after[off:off + size], before[off:off + size]) == (not any(np.any(g[n]) for g in seen)), n
        else:      # no gradient: not touched (no decay, no moment)
            assert np.array_equal(after[off:off + size].view(np.uint32), before[off:off + size].view(np.uint32)), n
            assert not eng.tensor(n, eng.exp_avg).any() and not eng.tensor(n, eng.exp_avg_sq).any(), n
    assert pad.sum() > 0 and np.array_equal(after[pad].view(np.uint32), before[pad].view(np.uint32))
    assert not after[pad].any() and not eng.exp_avg.cpu().numpy()[pad].any() and not eng.exp_avg_sq.cpu().numpy()[pad].any()
    assert [int(s) for s in eng.tensor_step.cpu().numpy()] == [3 if a else 0 for a in act]
