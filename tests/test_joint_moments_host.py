"""Posterior marginals and joint moments of all latents, on the host side: the entry points of csrc/is_moments.hip
(pp_is_moments_workspace_bytes, pp_is_moments_groups) are declared, prototyped and exported and PP_IS_MOMENTS_WIDTH agrees between
header and binding; the workspace grows with the call; bad arguments are rejected before anything touches a device; the moments ->
mean / cov / corr arithmetic on a hand-made row; Empiricals without a statement log refuse with a sentence; and, through a CPU
double of the operator registered here (moments_ref.py, float64 numpy), joint() / joint_batch / marginal / resample_joint on the
CPU device: a two-statement straight-line program and Marsaglia's branching program. The kernel is the GPU's:
tests/test_gpu_joint_moments.py."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import moments_ref as MR
import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
import resample_ref as R
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_moments_workspace_bytes', 'pp_is_moments_groups')
_registered = False


def _register_cpu_double():
    """The product has no CPU implementation of the operator: this file registers the float64 restatement as its CPU kernel."""
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_moments_groups', MR.is_moments_groups_cpu, 'CPU')
        _registered = True


def test_entry_points_are_declared_prototyped_and_exported():
    """FAILS WITHOUT THE FEATURE: the parent has neither symbol."""
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.PROTOTYPES, name
        assert hasattr(lib, name), name
        decl = hdr[hdr.index('%s(' % name):]
        decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
        assert decl.count(',') + 1 == len(L.PROTOTYPES[name][1]), name
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15          # additions only
    block = hdr[hdr.index('Joint weighted moments of up to'):hdr.index('#define PP_IS_MOMENTS_MAX_COLS')]
    for ref in ('empirical.py:298-309', ':451-466', ':668-690'):
        assert ref in block, ref


def test_width_macro_agrees_between_header_and_binding():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    assert int(re.search(r'#define PP_IS_MOMENTS_MAX_COLS (\d+)', hdr).group(1)) == L.PP_IS_MOMENTS_MAX_COLS == 16
    body = re.search(r'#define PP_IS_MOMENTS_WIDTH\(J\) (.*)', hdr).group(1)
    for J in range(1, 17):
        assert eval(body.replace('/', '//'), {'J': J}) == L.PP_IS_MOMENTS_WIDTH(J) == 4 + 2 * J + J * (J + 1) // 2
    assert L.PP_IS_MOMENTS_WIDTH(16) == 172


def test_workspace_bytes_are_monotone():
    lib = L.load()
    per = (1, 63, 2047, 2048, 2049, 4097, 70001, 10 ** 6)
    for J in (1, 4, 5, 16):
        for M in (0, 1, 3, 257, 70000):
            sizes = [lib.pp_is_moments_workspace_bytes(M, n, J) for n in per if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (J, M, sizes)
        for n in per:
            sizes = [lib.pp_is_moments_workspace_bytes(M, n, J) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0, (J, n, sizes)
    assert lib.pp_is_moments_workspace_bytes(4, 10 ** 6, 3) > lib.pp_is_moments_workspace_bytes(1, 10 ** 6, 3) > \
        lib.pp_is_moments_workspace_bytes(1, 2048, 3)
    assert lib.pp_is_moments_workspace_bytes(1, 10 ** 6, 16) > lib.pp_is_moments_workspace_bytes(1, 10 ** 6, 4)
    for bad in ((-1, 5, 2), (1, 0, 2), (1, 5, 0), (1, 5, 17)):
        assert lib.pp_is_moments_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    import ctypes as C
    lib = L.load()
    M, N, J = 3, 5000, 5
    lw = torch.zeros(M * N)
    cols = [torch.zeros(M * N) for _ in range(J)]
    stats = torch.zeros(M, 6, dtype=torch.float64)
    out = torch.zeros(M, L.PP_IS_MOMENTS_WIDTH(J), dtype=torch.float64)
    ws_bytes = lib.pp_is_moments_workspace_bytes(M, N, J)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8)
    ptrs = (C.c_void_p * 17)(*([c.data_ptr() for c in cols] * 4)[:17])
    holed = (C.c_void_p * J)(*[c.data_ptr() for c in cols])
    holed[3] = None

    def call(lw_p=lw.data_ptr(), cp=C.cast(ptrs, C.c_void_p), j=J, m=M, n_per=N, o=out.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.pp_is_moments_groups(lw_p, cp, j, m, n_per, stats.data_ptr(), o, w, wb, None)
    EINVAL, ENOSPACE = -1, -2
    assert call(lw_p=None) == EINVAL and call(cp=None) == EINVAL and call(o=None) == EINVAL and call(w=None) == EINVAL
    assert call(cp=C.cast(holed, C.c_void_p)) == EINVAL                       # a NULL column pointer
    assert call(j=0) == EINVAL and call(j=17, wb=2 ** 40) == EINVAL and call(j=-1) == EINVAL
    assert call(n_per=0) == EINVAL and call(n_per=-2) == EINVAL and call(m=-1) == EINVAL
    assert call(m=2 ** 20, n_per=2 ** 11, wb=2 ** 40) == EINVAL                # M n_per = 2^31
    assert b'pp_is_moments_groups' in lib.pp_last_error()
    assert call(wb=ws_bytes - 1) == ENOSPACE and call(wb=0) == ENOSPACE
    assert b'workspace too small' in lib.pp_last_error()
    assert call(m=0) == 0                                                    # no group: nothing to launch
    for t in [lw, out] + cols:
        assert float(t.double().abs().sum()) == 0.0


def test_moments_to_mean_cov_corr_on_a_hand_made_row():
    from pyprob_amd.distributions import joint_from_moments
    # three particles, weights 1, 2, 1 (W = 4); x = (10, 11, 12), y = (5, 3, 4); pivots c = (10, 5)
    w = np.array([1.0, 2.0, 1.0])
    x, y = np.array([10.0, 11.0, 12.0]), np.array([5.0, 3.0, 4.0])
    dx, dy = x - 10.0, y - 5.0
    row = [0.25, w.sum(), (w * w).sum(), 3, 10.0, 5.0, (w * dx).sum(), (w * dy).sum(),
           (w * dx * dx).sum(), (w * dx * dy).sum(), (w * dy * dy).sum()]
    assert len(row) == L.PP_IS_MOMENTS_WIDTH(2)
    j = joint_from_moments(['x', 'y'], row)
    assert j.addresses == ['x', 'y'] and j.count == 3 and j.ess == pytest.approx(16.0 / 6.0, rel=1e-15)
    np.testing.assert_allclose(j.mean, [11.0, 3.75], rtol=1e-15)
    # by hand: var x = (1 + 0 + 1) / 4 = 0.5; var y = (1.5625 + 2 * 0.5625 + 0.0625) / 4 = 0.6875; cov = (-1.25 + 0 + 0.25) / 4
    np.testing.assert_allclose(j.cov, [[0.5, -0.25], [-0.25, 0.6875]], rtol=1e-14)
    np.testing.assert_allclose(j.stddev, np.sqrt([0.5, 0.6875]), rtol=1e-14)
    np.testing.assert_allclose(j.corr, [[1.0, -0.25 / math.sqrt(0.5 * 0.6875)], [-0.25 / math.sqrt(0.5 * 0.6875), 1.0]], rtol=1e-14)
    # no particle with a finite weight: NaN arrays
    empty = joint_from_moments(['x', 'y'], [-np.inf, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert empty.count == 0 and empty.ess == 0.0
    assert np.isnan(empty.mean).all() and np.isnan(empty.cov).all() and np.isnan(empty.corr).all() and np.isnan(empty.stddev).all()
    # a constant column: variance 0 (clamped, never negative), its correlations NaN
    flat = joint_from_moments(['x', 'y'], [0.0, 4.0, 6.0, 3, 10.0, 7.0, 4.0, 0.0, 6.0, 0.0, -1e-30])
    assert flat.cov[1, 1] == 0.0 and flat.stddev[1] == 0.0 and np.isnan(flat.corr[0, 1]) and flat.corr[0, 0] == 1.0


def test_empiricals_without_a_statement_log_refuse(monkeypatch):
    import pyprob_amd
    from pyprob_amd.distributions import Empirical
    rng = np.random.default_rng(0)
    host = Empirical(values=[float(v) for v in rng.normal(size=20)], log_weights=rng.normal(size=20))
    dev = Empirical.from_device(torch.zeros(20), torch.zeros(20), None)
    for emp in (host, dev):
        for call in (lambda: emp.addresses, lambda: emp.marginal('a'), lambda: emp.joint(), lambda: emp.resample_joint(5),
                     lambda: emp.statement_rows, lambda: pyprob_amd.joint_batch([emp])):
            with pytest.raises(AttributeError, match='no statement log'):
                call()
    assert pyprob_amd.joint_batch([]) == []
    # PP_EMPIRICAL_DEVICE=0 keeps the host route: the log is not served, and the message says so
    dev.statement_log = [{'a': (torch.zeros(20), 0)}]
    dev._statement_rows_raw = [{'a': None}]
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    for call in (lambda: dev.addresses, lambda: dev.marginal('a'), lambda: dev.joint(), lambda: dev.resample_joint(5)):
        with pytest.raises(ValueError, match='PP_EMPIRICAL_DEVICE=0'):
            call()


def test_operator_schema_and_column_blocks_through_the_cpu_double():
    """The operator's shape contract, and the host's assembly of more than 16 columns from calls over pairs of 8-column blocks."""
    from pyprob_amd import ops as P
    from pyprob_amd.empirical import _moment_rows, joint_from_moments
    _register_cpu_double()
    rng = np.random.default_rng(1)
    M, N = 3, 70
    lw = rng.normal(0, 2, (M, N)).astype(np.float32)
    lw[0, 3], lw[1, 5], lw[2, :] = -np.inf, np.nan, np.inf
    for J in (1, 5, 16):
        x = rng.normal(3, 1, (J, M, N)).astype(np.float32)
        x[:, 0, 3] = np.nan
        out = P.ops.is_moments_groups(torch.from_numpy(lw.reshape(-1)), [torch.from_numpy(c.reshape(-1)) for c in x], N, None)
        assert out.dtype == torch.float64 and out.shape == (M, L.PP_IS_MOMENTS_WIDTH(J))
        o = out.numpy()
        assert o[0, 3] == N - 1 and o[1, 3] == N - 1 and o[2, 3] == 0 and (o[2, 1:3] == 0).all() and np.isfinite(o[:2]).all()
    MR.calls['is_moments_groups'] = 0
    J = 21
    x = (rng.normal(0, 1, (J, N)) + np.arange(J)[:, None]).astype(np.float32)
    l1 = torch.from_numpy(lw[0].copy())
    rows = _moment_rows(l1, [torch.from_numpy(c.copy()) for c in x], N, None)
    assert rows.shape == (1, L.PP_IS_MOMENTS_WIDTH(J)) and MR.calls['is_moments_groups'] == 3      # blocks (0,1), (0,2), (1,2)
    j = joint_from_moments(list(range(J)), rows[0])
    mean, cov = MR.mean_cov_ref(lw[0], x)
    np.testing.assert_allclose(j.mean, mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(j.cov, cov, rtol=1e-10, atol=1e-12)


def _two_statement_model():
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec
    from pyprob_amd.state import TraceMode

    class TwoStatements(Model):
        def forward(self):
            a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a', name='mu')
            pyprob.observe(Normal(a, math.sqrt(2.0)), name='obs0')
            b = pyprob.sample(Normal(a, 0.7), address='b')
            pyprob.observe(Normal(b, math.sqrt(2.0)), name='obs1')
            return b
    model = TwoStatements()
    tr = next(model._trace_generator(trace_mode=TraceMode.PRIOR))
    emb = {'obs0': {'dim': 32}, 'obs1': {'dim': 32}}
    eng = oracle_ops.CpuBufferEngine(NetSpec(emb, lstm_dim=64, proposal_mixture_components=10), seed=1)
    eng.add_addresses([(v.address, v.distribution.name, None) for v in tr.variables_controlled])
    net = InferenceNetworkLSTM(observe_embeddings=emb, lstm_dim=64, device='cpu')
    net._obs_names = list(emb)
    net._engine = eng
    net._is = ISRunner(eng)
    net._layers_initialized = True
    model._inference_network = net
    return model


def test_joint_of_the_two_statement_program_on_the_cpu_device_matches_numpy():
    import pyprob_amd
    _register_cpu_double()
    R.register_cpu_doubles()
    model = _two_statement_model()
    n = 64
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
    A, B = 'a__Normal__1', 'b__Normal__1'
    assert post.addresses == [A, B] and post.statement_names == {'mu': A}
    assert post.statement_rows == [{A: None}, {B: None}]
    lw = post._all_log_weights.numpy()
    cols = np.stack([post.statement_log[0][A][0].numpy(), post.statement_log[1][B][0].numpy()])
    mean, cov = MR.mean_cov_ref(lw, cols)
    j = post.joint()
    assert j.addresses == [A, B] and j.count == n
    np.testing.assert_allclose(j.mean, mean, rtol=1e-12)
    np.testing.assert_allclose(j.cov, cov, rtol=1e-10)
    np.testing.assert_allclose(j.corr, cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov))), rtol=1e-10)
    assert j.ess == pytest.approx(post.effective_sample_size, rel=1e-12)
    assert j.mean[1] == pytest.approx(post.mean, rel=1e-10) and j.cov[1, 1] == pytest.approx(post.variance, rel=1e-8)
    # by the statement's address= and by its name=, reordered
    k = post.joint(['b', 'mu'])
    assert k.addresses == [B, A] and np.array_equal(k.mean, j.mean[::-1]) and k.cov[0, 1] == j.cov[0, 1]
    # the marginal shares the log's tensor and the log-weights; the return value's marginal is the posterior itself
    ma, mb = post.marginal('mu'), post.marginal('b')
    assert ma._values is post.statement_log[0][A][0] and ma._log_weights is post._log_weights
    assert ma.mean == pytest.approx(mean[0], rel=1e-10) and ma.variance == pytest.approx(cov[0, 0], rel=1e-8)
    assert mb.mean == pytest.approx(post.mean, rel=1e-12) and ma.metadata['op'] == 'marginal' and ma.metadata['address'] == A
    with pytest.raises(KeyError, match="'a__Normal__1', 'b__Normal__1'"):
        post.marginal('nope')
    # the loop of joint() calls is what joint_batch returns for anything that is not one batched execution
    both = pyprob_amd.joint_batch([post, post], ['a'])
    assert len(both) == 2 and all(np.array_equal(b.cov, post.joint(['a']).cov) for b in both)
    # one index per joint draw; the index stream is resample()'s
    draws = post.resample_joint(50, seed=5, offset=3)
    assert set(draws) == {A, B, 'index'} and draws['index'].dtype == torch.int64 and draws['index'].shape == (50,)
    for a, col in zip((A, B), cols):
        assert np.array_equal(draws[a].numpy(), col[draws['index'].numpy()])
    with pytest.raises(ValueError):
        post.resample_joint(0)


def test_marsaglia_on_the_cpu_device_records_who_executed_what():
    """A branching program: the first pair of draws is everybody's, later pairs belong to the particles that rejected - joint()
    serves the former, marginal() the latter over their own particles, and the row lists partition as the program says."""
    from is_helpers import lockstep_network
    _register_cpu_double()
    model, net, meta, params = lockstep_network()
    n = 200
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 8.0, 'obs1': 9.0}, lock_step=True, seed=3, offset=0)
    log, rows = post.statement_log, post.statement_rows
    assert len(rows) == len(log) >= 4 and all(set(r) == set(e) for r, e in zip(rows, log))
    addrs = post.addresses
    assert len(addrs) == len(log) and rows[0][addrs[0]] is None and rows[1][addrs[1]] is None
    x0, y0 = (log[k][addrs[k]][0].numpy() for k in (0, 1))
    rejected = np.nonzero(x0 * x0 + y0 * y0 >= 1)[0]
    for k in (2, 3):
        assert np.array_equal(rows[k][addrs[k]].numpy(), rejected)
    j = post.joint()
    assert j.addresses == addrs[:2] and j.count == n
    lw = post._all_log_weights.numpy()
    mean, cov = MR.mean_cov_ref(lw, np.stack([x0, y0]))
    np.testing.assert_allclose(j.mean, mean, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(j.cov, cov, rtol=1e-10)
    with pytest.raises(ValueError, match=re.escape(addrs[2])):
        post.joint([addrs[0], addrs[2]])
    m = post.marginal(addrs[2])
    assert m.length == len(rejected) and np.array_equal(m._values.numpy(), log[2][addrs[2]][0].numpy()[rejected])
    sub_mean, sub_cov = MR.mean_cov_ref(lw[rejected], log[2][addrs[2]][0].numpy()[rejected][None])
    assert m.mean == pytest.approx(sub_mean[0], rel=1e-10) and m.variance == pytest.approx(sub_cov[0, 0], rel=1e-8)


def _skipping_branch_model():
    """a ~ Normal(0, 1); `if a > 0:` b ~ Normal(a, 0.7); c ~ Normal(a, 1); observe obs0 ~ Normal(c, .); returns c - an `if` without
    `else` before a shared statement: 'c' is statement 2 of the particles that took the branch and statement 1 of the others."""
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec

    class SkippingBranch(Model):
        def forward(self):
            a = pyprob.sample(Normal(0.0, 1.0), address='a')
            if a > 0:
                pyprob.sample(Normal(a, 0.7), address='b')
            c = pyprob.sample(Normal(a, 1.0), address='c')
            pyprob.observe(Normal(c, math.sqrt(2.0)), name='obs0')
            return c
    model = SkippingBranch()
    emb = {'obs0': {'dim': 32}}
    eng = oracle_ops.CpuBufferEngine(NetSpec(emb, lstm_dim=64, proposal_mixture_components=10), seed=1)
    eng.add_addresses([(a + '__Normal__1', 'Normal', None) for a in 'abc'])
    net = InferenceNetworkLSTM(observe_embeddings=emb, lstm_dim=64, device='cpu')
    net._obs_names = list(emb)
    net._engine = eng
    net._is = ISRunner(eng)
    net._layers_initialized = True
    model._inference_network = net
    return model


def test_an_address_at_two_statement_indices_is_one_latent_over_all_its_particles():
    """The statement log is keyed by statement index first: after `if a > 0: b = sample(...)` the shared 'c' sits at index 2 for
    one path and at index 1 for the other. marginal / joint / resample_joint answer for ALL the particles that executed it."""
    _register_cpu_double()
    R.register_cpu_doubles()
    model = _skipping_branch_model()
    n = 200
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(n, IC, observe={'obs0': 0.5}, lock_step=True, seed=11, offset=0)
    A, B, C = ('{}__Normal__1'.format(a) for a in 'abc')
    log, rows = post.statement_log, post.statement_rows
    assert [sorted(e) for e in log] == [[A], [B, C], [C]]
    a = log[0][A][0].numpy()
    took, skipped = np.nonzero(a > 0)[0], np.nonzero(~(a > 0))[0]
    assert 0 < len(took) < n
    assert np.array_equal(rows[1][B].numpy(), took) and np.array_equal(rows[2][C].numpy(), took)
    assert np.array_equal(rows[1][C].numpy(), skipped)
    c = np.empty(n, np.float32)
    c[skipped], c[took] = log[1][C][0].numpy()[skipped], log[2][C][0].numpy()[took]
    lw = post._all_log_weights.numpy()
    assert sorted(post.addresses) == [A, B, C] and post.addresses[0] == A
    mc = post.marginal('c')
    assert mc.length == n and np.array_equal(mc._values.numpy(), c) and mc._log_weights is post._log_weights
    mean, cov = MR.mean_cov_ref(lw, np.stack([a, c]))
    assert mc.mean == pytest.approx(mean[1], rel=1e-10) and mc.variance == pytest.approx(cov[1, 1], rel=1e-8)
    assert np.array_equal(post._all_values.numpy(), c) and mc.mean == pytest.approx(post.mean, rel=1e-6)      # c is the return value
    j = post.joint()
    assert j.addresses == [A, C] and j.count == n       # every particle executed 'c'; 'b' is the branch's
    np.testing.assert_allclose(j.mean, mean, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(j.cov, cov, rtol=1e-10)
    assert post.joint(['c']).mean[0] == pytest.approx(j.mean[1], rel=1e-12)
    with pytest.raises(ValueError, match=re.escape(B)):
        post.joint(['a', 'b'])
    mb = post.marginal('b')
    b = log[1][B][0].numpy()[took]
    assert mb.length == len(took) and np.array_equal(mb._values.numpy(), b)
    assert mb.mean == pytest.approx(MR.mean_cov_ref(lw[took], b[None])[0][0], rel=1e-10)
    draws = post.resample_joint(100, seed=2)
    assert set(draws) == {A, C, 'index'} and np.array_equal(draws[C].numpy(), c[draws['index'].numpy()])
    # the log's own tensors are not written to by the merge
    assert np.array_equal(log[1][C][0].numpy()[skipped], c[skipped]) and np.array_equal(log[2][C][0].numpy()[took], c[took])


def test_a_grown_empirical_no_longer_serves_the_old_particles_latents():
    _register_cpu_double()
    model = _two_statement_model()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        post = model.posterior_results(16, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
    assert post.joint().count == 16 and post.marginal('a').length == 16
    post.add(torch.tensor(0.25), log_weight=-1.0)
    post.finalize()
    assert post.length == 17
    for call in (lambda: post.addresses, lambda: post.marginal('a'), lambda: post.joint(), lambda: post.resample_joint(5),
                 lambda: post.statement_rows):
        with pytest.raises(AttributeError, match='grew'):
            call()


def test_resample_joint_after_dropped_particles_indexes_all_particles_of_the_call():
    """Where the call dropped particles with a non-finite log-weight, the indices point into ALL particles of the call (the rows of
    the log's columns), never at a dropped one, and every column is gathered by the same index; the stream is then not resample()'s
    (which numbers the kept particles) - the docstring's restriction."""
    _register_cpu_double()
    R.register_cpu_doubles()
    model = _two_statement_model()
    n = 64
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        full = model.posterior_results(n, IC, observe={'obs0': 2.0, 'obs1': 1.5}, lock_step=True, seed=7, offset=100)
    from pyprob_amd.distributions import Empirical
    lw = full._all_log_weights.clone()
    dropped = [0, 5, 63]
    lw[0], lw[5], lw[63] = float('-inf'), float('nan'), float('-inf')
    keep = torch.isfinite(lw)
    post = Empirical.from_device(full._all_values[keep].contiguous(), lw[keep].contiguous(), None)
    post._all_values, post._all_log_weights = full._all_values, lw
    post.statement_log, post._statement_rows_raw, post.statement_names = full.statement_log, full._statement_rows_raw, {}
    A, B = 'a__Normal__1', 'b__Normal__1'
    draws = post.resample_joint(400, seed=5, offset=3)
    idx = draws['index'].numpy()
    assert idx.min() >= 0 and idx.max() < n and not np.isin(idx, dropped).any() and len(np.unique(idx)) > 1
    for j, a in enumerate((A, B)):
        assert np.array_equal(draws[a].numpy(), full.statement_log[j][a][0].numpy()[idx])
    assert post.joint().count == n - 3
