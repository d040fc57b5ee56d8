"""The cases of tests/test_gpu_dims.py and the off-grid cases of tests/test_gpu_is_step_fused.py (tests/dim_cases.py), with the
oracle alone: every case lies in the route class its name says (dim_cases.routes, the engine's dimension predicates restated, flag
by flag), each build finds its B traces away from the ReLU kinks among B + 64 candidates and has the shape the case is there for,
the Adam cases stay finite over their three steps, and the inputs of the IS statement cases leave more than 99 % of the
particles a finite float64 log q. CPU only."""
import numpy as np
import pytest

import depth_cases as D
import dim_cases as DC
from helpers import IS_ADDRS, is_engine, oracle_run, packed
from oracle import ic_oracle as O

torch = pytest.importorskip('torch')


@pytest.mark.parametrize('name', list(DC.ALL))
def test_every_case_lies_in_its_route_class(name):
    got, want = DC.routes(DC.ALL[name]), DC.expected(name)
    assert list(got) == list(want)
    for flag in want:
        assert bool(got[flag]) == want[flag], (name, flag, got[flag])


def test_the_cases_are_the_ones_their_names_say():
    H = {n: c[0] for n, c in DC.ALL.items()}
    assert H['h96'] % 32 == 0 and H['h96'] % 64 != 0 and H['h48'] % 16 == 0 and H['h48'] % 32 != 0
    assert H['h100'] % 4 == 0 and H['h100'] % 16 != 0 and H['h50'] % 2 == 0 and H['h50'] % 4 != 0 and H['h33'] % 2 == 1
    assert H['h384'] % 64 == 0 and not DC.routes(DC.ALL['h384'])['tail'] and not DC.routes(DC.ALL['h384'])['panel_dims']
    assert [DC.lstm_in(DC.ALL[n]) for n in ('smp1', 'smp8', 'smp9', 'addr10', 'addr128', 'dtype7', 'ne2', 'all_odd')] == \
        [209, 216, 217, 104, 340, 210, 72, 32]
    assert [DC.lstm_in(DC.ALL[n]) for n in ('h512_smp8', 'h512_addr10', 'h512_addr32_dtype4', 'h1024_addr10')] == [216, 104, 140, 104]
    assert all(DC.lstm_in(DC.ALL[n]) == 212 for n in DC.HIDDEN)
    # the panel cases keep compact rows (the only way to the panel kernels); their control does not
    assert all(DC.routes(DC.PANEL[n])['panel_dims'] for n in DC.PANEL if n != 'h512_smp3')
    assert not DC.routes(DC.PANEL['h512_smp3'])['compact']


def test_the_cases_cover_as_many_route_classes_as_listed():
    classes = {tuple(DC.routes(c).values()) for c in DC.CASES.values()}
    assert len(classes) >= DC.N_CLASSES, sorted(classes)
    for flag in DC.expected('h96'):      # every flag is on in one case and off in another
        assert {DC.routes(c)[flag] for c in DC.CASES.values()} == {True, False}, flag


def _reaches(kind, B, arrays, pb):
    assert len(arrays['trace_len']) == B and int(arrays['trace_len'].max()) == pb.t_max
    if kind == 'ragged':
        assert pb.t_max >= 4 and pb.n_active[-1] <= 8      # a recurrence; few traces in the late time steps
        assert np.isin(1.25, arrays['values'])             # rescued rows
    else:
        assert pb.t_max == 1


@pytest.mark.parametrize('label', list(DC.all_builds()))
def test_kink_filter_keeps_enough_traces(label):
    """Every case finds its B traces among B + 64 candidates (the filter asserts it), on the host copy of the engine's buffers:
    the initial weights are the same on either device. The oracle evaluates the network: a finite loss."""
    name, kind, B = DC.all_builds()[label]
    eng, arrays, addresses, dists = DC.build(name, kind, B, device='cpu')
    c = DC.ALL[name]
    assert [(o[3], o[1]) for o in eng.spec.obs] == list(DC.obs_pairs(c)) and arrays['obs'].shape == (B, len(DC.obs_pairs(c)))
    head = eng.spec.head_dims(eng.spec.addresses[0])
    assert head[1] == (c[0] + 30) // 2 and head[0] == 30      # (h50: 40 hidden units, h33: 31)
    _reaches(kind, B, arrays, packed(arrays, eng.spec))
    params = {k: v.numpy() for k, v in eng.state_dict().items()}
    assert np.isfinite(oracle_run(eng.spec, params, arrays, addresses, dists, want_grads=False)['loss'])


def test_kink_filter_keeps_enough_traces_in_the_sequence():
    name, batches = DC.SEQUENCE
    eng = DC.engine(name, 'ragged', device='cpu')
    for k, (kind, B) in enumerate(batches):
        arrays = D.batch(eng, kind, B, seed=10 * k)[0]
        assert len(arrays['trace_len']) == B and (int(arrays['trace_len'].max()) == 1) == (kind == 'single_a0')


@pytest.mark.parametrize('name,kind', DC.ADAM)
def test_the_adam_cases_stay_finite(name, kind):
    """Three float64 Adam steps of the oracle at dim_cases.ADAM_LR on the case's batch: every loss finite, so that no device step
    is skipped for its status word."""
    eng, arrays, addresses, dists = DC.build(name, kind, DC.B_STEP, device='cpu')
    pb = packed(arrays, eng.spec)
    act = eng.spec.active_mask(pb.cur_counts, pb.prev_counts)
    P = {k: v.numpy().astype(np.float64) for k, v in eng.state_dict().items()}
    M = {k: np.zeros_like(v) for k, v in P.items()}
    V = {k: np.zeros_like(v) for k, v in P.items()}
    sizes = [int(np.prod(s)) for _, s in eng.spec.tensors.values()]
    assert any(n % 2 for n in sizes) and any(n % 1024 for n in sizes)      # padding behind tensors in the chunked layout
    for step in range(1, 4):
        out = oracle_run(eng.spec, P, arrays, addresses, dists)
        assert np.isfinite(out['loss']), (step, out['loss'])
        for i, n in enumerate(eng.spec.tensors):
            if act[i]:
                assert np.isfinite(out['grads'][n]).all(), (step, n)
                O.adam_step(P[n], out['grads'][n], M[n], V[n], step, DC.ADAM_LR)
    assert np.isfinite(oracle_run(eng.spec, P, arrays, addresses, dists, want_grads=False)['loss'])


# ---- the IS statement cases: the oracle-backed operators on the host copy of the engine ----------------------------------------------
@pytest.mark.parametrize('name,n,prev,cur', DC.IS_STATEMENTS, ids=['%s-%d-%d' % (c[0], c[1], i) for i, c in enumerate(DC.IS_STATEMENTS)])
def test_is_statement_inputs_leave_log_q_finite(name, n, prev, cur):
    """The statement's inputs through the oracle-backed is_step: more than 99 % of the particles with a finite log q at values
    drawn from the oracle's own proposal - the cap the GPU test keeps is met by the oracle alone."""
    from pyprob_amd.ops import ops
    eng, run, sd = is_engine(DC.ALL[name][0], device='cpu', **DC.is_kw(name))
    ids = eng.spec.address_id
    assert (eng.spec.smp_dim, eng.spec.addr_dim, eng.spec.dtype_dim) == DC.ALL[name][2:5]
    assert eng.spec.head_dims(eng.spec.addresses[ids[cur[0]]])[0] <= 32
    assert sd['_layers_address_embedding.a_normal'].shape == (DC.ALL[name][3],)
    assert sd['_layers_distribution_type_embedding.Normal'].shape == (DC.ALL[name][4],)
    assert sd['_layers_sample_embedding.a_cat._layers.0.weight'].shape == (DC.ALL[name][2], 7)
    from test_gpu_is_step_fused import statement_inputs
    h0, c0, pv, prior = statement_inputs(DC.ALL[name][0], DC.ALL[name][1], n, prev, cur)
    h, c = torch.from_numpy(h0.copy()), torch.from_numpy(c0.copy())
    run._ensure_ws(n)
    value, logq = ops.is_step(eng.params, run.ws, eng.net_handle, ids[cur[0]], ids[prev[0]], n, run.e_obs, torch.from_numpy(pv),
                              torch.from_numpy(prior), h, c, n, None, 1234, 0)
    assert np.isfinite(value.numpy()).all() and np.isfinite(logq.numpy()).mean() > 0.99
    assert np.isfinite(h.numpy()).all() and not np.array_equal(h.numpy(), h0)


@pytest.mark.parametrize('name', DC.IS_FIRST)
def test_first_statement_inputs_leave_log_q_finite(name):
    """A trace's first statement (no previous address, one shared state row) through the oracle-backed is_step."""
    eng, run, sd = is_engine(DC.ALL[name][0], device='cpu', **DC.is_kw(name))
    run.begin(DC.IS_FIRST_N)
    value, logq = run.step(eng.spec.address_id[DC.UNIFORM[0]], None, torch.tensor([DC.IS_FIRST_PRIOR]), seed=77)
    lo, hi = DC.IS_FIRST_PRIOR
    assert ((value.numpy() >= lo) & (value.numpy() < hi)).all() and np.isfinite(logq.numpy()).mean() > 0.99
    assert np.isfinite(run.h[:, 0].numpy()).all() and run.state_rows == 1


def test_the_is_cases_are_the_listed_ones():
    smp_with_cat = sorted({DC.ALL[n][2] for n, _, prev, _ in DC.IS_STATEMENTS if prev == DC.CAT})
    assert smp_with_cat == sorted({DC.ALL[n][2] for n, _, _, _ in DC.IS_STATEMENTS}) == [1, 4, 5, 8, 9]
    counts = [n for _, n, _, _ in DC.IS_STATEMENTS]
    assert set(counts) == {1, 257, 300} and counts.count(1) == 1
    assert [DC.routes(DC.ALL[n])['is_first'] for n in DC.IS_FIRST] == [False, False, False, True, True]
    assert [a for a, _, _ in IS_ADDRS][:3] == [DC.NORMAL[0], DC.UNIFORM[0], DC.CAT[0]]
    fused = {n: DC.routes(DC.ALL[n]) for n, _, _, _ in DC.IS_STATEMENTS}
    assert not any(fused[n]['is_fused'] for n in ('h50', 'h100', 'h33', 'smp9', 'h512_smp9', 'all_odd'))
    assert all(fused[n]['is_small'] for n in ('smp1', 'h64_smp5', 'smp8', 'h96_smp8_d2', 'addr128', 'dtype7'))
    assert all(fused[n]['is_fused'] and not fused[n]['is_small'] for n in ('h512_smp1', 'h512_smp8', 'h1024_smp8'))
