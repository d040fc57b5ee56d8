"""The fused observe embedding (csrc/obs_embed.hip: obs_embed_fwd_kernel<NOBS, EARLY>, obs_embed_dgrad_kernel<NOBS>, and the
weight-gradient products and column sums fed from their buffers) against the float64 oracle over the envelope that
obs_fused_supported accepts, and the embeddings next to its edges, which must take the generic path. Cases, weights and
batches: tests/embed_cases.py. Every training step compares the status word, the loss (2e-5 relative), the per-row log_prob and
every gradient tensor (helpers.GRAD_BAR of its largest element + the project's absolute floors) through
depth_cases.step_against_oracle. Which path ran is observed: the fused first launch stamps its workgroups under
pp_debug_wgtrace mode 4. No call may fail: pp_last_error is never consulted."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as D
import embed_cases as EC
from helpers import first_launch_workgroups, fresh_engine, trained_looking
from oracle import ic_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def error_text_not_consulted(monkeypatch):
    """Every caller of the C ABI reads pp_last_error only behind a non-zero return code."""
    from pyprob_amd import lib as L
    lib, asked = L.load(), []
    real = lib.pp_last_error

    def last_error():
        asked.append(real())
        return asked[-1]
    monkeypatch.setattr(lib, 'pp_last_error', last_error)
    yield
    assert not asked, asked


def _floor(kind, network='lstm'):
    # ('len2' is the Marsaglia program's batch - Uniform addresses, TruncatedNormal heads - and takes its floor)
    return D.abs_floor('ragged' if kind == 'len2' else kind, network)


def _step(label, name, kind, H, B, network='lstm'):
    eng, arrays, addresses, dists = EC.build(name, kind, H, B, network=network)
    emb = EC.CASES[name]
    assert eng.spec.e_obs == sum(d for d, _ in emb) and eng.spec.obs_width == EC.width_of(emb) == arrays['obs'].shape[1]
    assert all(eng.spec.obs_depth[o[0]] == 2 for o in eng.spec.obs)
    pb, _, _ = D.step_against_oracle(label, eng, arrays, addresses, dists, _floor(kind, network))
    assert pb.n_traces == B
    return eng, pb


def _fused_ran(name, eng, pb):
    """Fitting cases run the fused launch, the others must not."""
    stamps = first_launch_workgroups(eng, pb)
    assert int(eng.status_buf[0].item()) == 0
    assert (stamps > 0) == (name in EC.FIT), (name, stamps)


@pytest.mark.parametrize('kind', ['single', 'ragged'])
@pytest.mark.parametrize('name', list(EC.CASES))
def test_training_step_against_oracle(name, kind):
    """H = 64, B = 130. single: T = 1 - the fused row build, dX as split partials (n_split > 1 in the backward kernel's load).
    ragged: the Marsaglia program, max_iter = 5 - a separate gather, dE summed over a trace's time steps."""
    eng, pb = _step('embed_%s_%s' % (name, kind), name, kind, 64, EC.B_STEP)
    assert (pb.t_max == 1) if kind == 'single' else (pb.t_max > 2)
    _fused_ran(name, eng, pb)


@pytest.mark.parametrize('name', EC.LEN2)
def test_traces_of_length_two_against_oracle(name):
    """T = 2: the first launch builds the rows of both time steps itself (the t >= 1 branch of obs_build_rows)."""
    eng, pb = _step('embed_%s_len2' % name, name, 'len2', 64, EC.B_STEP)
    assert pb.t_max == 2 and pb.n_rows == 2 * EC.B_STEP
    _fused_ran(name, eng, pb)


@pytest.mark.parametrize('name', EC.TWO_PER_WAVE)
def test_two_traces_per_wave_against_oracle(name):
    """B = 1030 single statements: above 1 024 traces a wave walks two, the last wave one; both kernels fetch the next trace's
    observation / activations one iteration ahead."""
    assert EC.B_TWO_PER_WAVE > 1024 and EC.B_TWO_PER_WAVE % 8 != 0
    eng, pb = _step('embed_%s_b1030' % name, name, 'single', 64, EC.B_TWO_PER_WAVE)
    _fused_ran(name, eng, pb)


@pytest.mark.parametrize('name', EC.H512)
def test_h512_single_statements_against_oracle(name):
    """H = 512, B = 40, e_obs = 64: the shape at which plan_step consults the panel predicates. Three and eight observables must
    stay off the panel kernels' embedding code (at most two observables); whichever path runs is held against the oracle."""
    eng, pb = _step('embed_%s_h512' % name, name, 'single', 512, EC.B_H512)
    assert eng.spec.e_obs == 64
    _fused_ran(name, eng, pb)


@pytest.mark.parametrize('kind', ['single', 'ragged'])
@pytest.mark.parametrize('name', EC.FEEDFORWARD)
def test_feedforward_network_against_oracle(name, kind):
    """network='feedforward'. single: the heads read E in place, with a leading dimension round4(e_obs) > e_obs for e_obs = 30.
    ragged: the heads' rows are gathered from E (embedding_rows)."""
    eng, pb = _step('embed_%s_ff_%s' % (name, kind), name, kind, 64, EC.B_STEP, network='feedforward')
    assert eng.spec.feedforward and eng.spec.lstm_dim == 0


def test_one_workspace_large_small_large_against_oracle():
    """One engine, one workspace: ragged B = 300, single statements B = 17, ragged B = 40 - a stale obs_h / cat / f1 row of the
    larger batch read by a smaller one shows up against the oracle."""
    name, batches = EC.SEQUENCE
    eng = EC.engine(name, 'ragged', 64)
    for k, (kind, B) in enumerate(batches):
        arrays, addresses, dists = EC.batch(eng, kind, B, seed=10 * k)
        D.step_against_oracle('embed_sequence_%s_%d_%s_b%d' % (name, k, kind, B), eng, arrays, addresses, dists, D.abs_floor(kind))
        if k == 0:
            shape = eng.ws_shape
    assert eng.ws_shape == shape      # the later batches ran in the first one's workspace


# ---- importance sampling: the embedding of the one observation ---------------------------------------------------------------------
def _is_runner(name):
    from pyprob_amd.is_engine import ISRunner
    emb = EC.CASES[name]
    eng = trained_looking(fresh_engine(64, ['mu'], 'Normal', obs=EC.obs_of(emb)), seed=64 + len(emb))
    observe = EC.observations(np.array([[8.0, 9.0]], np.float32), EC.width_of(emb), seed=3)[0]
    net = O.Net({k: v.numpy() for k, v in eng.state_dict().items()}, [o[0] for o in eng.spec.obs], K=eng.spec.K)
    ref = O.embed_observe(net, observe.astype(np.float64).reshape(1, -1))[0][0]
    assert np.count_nonzero(ref) >= 1
    return eng, ISRunner(eng), observe, ref


def _embedding_from_init(run, observe, e):
    run.init(observe)
    got = run.e_obs[:e].cpu().numpy()       # (deferred: this launches pp_is_init)
    assert run._init_pending == 0
    return got


@pytest.mark.parametrize('name', list(EC.CASES))
def test_is_init_embedding_against_oracle(name, monkeypatch):
    """pp_is_init (PP_IS_FIRST=0: no fused first statement anywhere): the embedding row against the oracle, absolute 2e-6."""
    monkeypatch.setenv('PP_IS_FIRST', '0')
    eng, run, observe, ref = _is_runner(name)
    assert eng.lib.pp_is_first_statement_supported(C.byref(eng.net), 0) == 0
    got = _embedding_from_init(run, observe, eng.spec.e_obs)
    print(name, 'pp_is_init max |E - oracle|', float(np.abs(got - ref).max()), 'max |E|', float(np.abs(ref).max()))
    assert np.abs(got - ref).max() <= 2e-6, (name, float(np.abs(got - ref).max()))


@pytest.mark.parametrize('name', list(EC.CASES))
def test_first_statement_route_is_taken_exactly_by_the_fitting_cases(name, monkeypatch):
    """pp_is_first_statement_supported is 1 for the fitting cases and 0 for the others. Where it is 1, the embedding that
    pp_is_first_statement leaves in e_out is within 2e-6 of the oracle, and bit-equal to pp_is_init's: obs_forward_row
    (obs_embed.hpp) walks the layers in the order and with the sums of obs_embed_fwd_kernel, and include/pyprob_amd.h promises
    'bit-identical to the two calls it replaces'. With at most 8 observation values ISRunner.step_net takes that route itself
    (the default one); wider observations reach the kernel through the C ABI here."""
    from pyprob_amd import lib as L
    monkeypatch.delenv('PP_IS_FIRST', raising=False)
    eng, run, observe, ref = _is_runner(name)
    e, lib = eng.spec.e_obs, eng.lib
    supported = lib.pp_is_first_statement_supported(C.byref(eng.net), 0)
    assert supported == (1 if name in EC.FIT else 0), (name, supported)
    monkeypatch.setenv('PP_IS_FIRST', '0')
    separate = _embedding_from_init(run, observe, e)
    monkeypatch.delenv('PP_IS_FIRST')
    run.init(observe)
    run.begin(8)
    run.step_net(0, None)                # the default route of a trace's first statement
    torch.cuda.synchronize()
    default = run.e_obs[:e].cpu().numpy()
    assert np.abs(default - ref).max() <= 2e-6, (name, float(np.abs(default - ref).max()))
    assert np.array_equal(default.view(np.uint32), separate.view(np.uint32)), name
    if not supported:
        return
    run.init(observe)                    # stages the observation in pinned memory; the launch below reads it in place
    e_out = torch.zeros(run.e_obs_floats(), dtype=torch.float32, device=eng.device)
    L.check(lib.pp_is_first_statement(C.byref(eng.net), eng.params.data_ptr(), run._obs_pin.data_ptr(), 0, e_out.data_ptr(),
                                      run.h.data_ptr(), run.c.data_ptr(), run.ws.data_ptr(), run.ws_bytes, L.stream_ptr()),
            'pp_is_first_statement')
    torch.cuda.synchronize()
    run._init_pending = 0
    out = e_out.cpu().numpy()
    e4, k = (e + 3) & ~3, min(len(observe), 8)
    print(name, 'pp_is_first_statement max |E - oracle|', float(np.abs(out[:e] - ref).max()))
    assert np.abs(out[:e] - ref).max() <= 2e-6, (name, float(np.abs(out[:e] - ref).max()))
    assert np.array_equal(out[:e].view(np.uint32), separate.view(np.uint32)), name
    assert np.array_equal(out[e4:e4 + k], observe[:k])      # the device copies of the first 8 observation values
