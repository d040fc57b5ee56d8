"""Batched posteriors of multi-statement straight-line programs on the device (csrc/is_batch.hip pp_is_batch_bias /
pp_is_statement_groups, the GROUPED instantiations of csrc/is_step_fused.hip and csrc/is_step_small.hip; ISRunner.bias_batch /
statement_groups; BatchLockStepState.later_statement; Model._traces_lockstep_batch):
 1. the grouped statement indexes particles, groups, bias rows, state rows and Philox counters exactly: group g of an M-group call
    is bit-equal (values, log-weights, (h, c) rows) to the one-group call on row g at offset + g n_per, two identical calls are
    bit-equal, and nothing outside [0, M n_per) is written - both state modes, H = 64 / 256 / 512;
 2. pp_is_batch_bias rows and the y_out / (h, c) / log q of a grouped statement against the float64 oracle;
 3. the draws as a distribution: every particle's value under ITS OWN float64 mixture CDF (built from y_out) is uniform;
 4. end to end: two- and three-statement programs whose later priors depend on earlier draws, every particle re-scored by the
    oracle with its group's observation - the test that fails without the feature (`_batch_ok` is False there);
 5. a call sharded by PP_BATCH_STATE_BYTES returns the unsharded call's particles bit for bit;
 6. programs and networks outside the fast path return the loop's results bit for bit.
Batched and single-call particles are not compared value by value (tests/test_gpu_is_batch.py says why)."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from helpers import IS_EMB as EMB, is_engine
from is_helpers import lockstep_network
from oracle import ic_oracle as O
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine
from test_gpu_is_step_fused import _oracle_statement

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK

SHAPES = [(1, 1), (3, 1), (257, 1), (5, 31), (5, 32), (5, 33), (5, 63), (5, 64), (5, 65), (7, 1000), (2, 4097)]
PAD = 3            # poisoned rows behind M n_per (and around the bias / c0 blocks)
DIST = {'a_normal': 'Normal', 'a_uniform': 'Uniform'}
_ENGINES = {}


def _eng(H, K=10):
    if (H, K) not in _ENGINES:
        _ENGINES[(H, K)] = is_engine(H, seed=3, K=K)
    return _ENGINES[(H, K)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _prior(dist, n, rng):
    if dist == 'Normal':
        return np.stack([rng.normal(0, 1, n), rng.uniform(0.5, 2.0, n)], 1).astype(np.float32)
    lo = rng.uniform(-2, 0, n)
    return np.stack([lo, lo + rng.uniform(0.5, 3, n)], 1).astype(np.float32)


def _workspace(run, eng, M):
    need = eng.lib.pp_is_batch_workspace_bytes(C.byref(eng.net), M)
    if getattr(run, '_t_ws', None) is None or run._t_ws.numel() < need:
        run._t_ws = torch.empty(need, dtype=torch.uint8, device=run.dev)
    return run._t_ws


def _groups_call(eng, run, cur, prev, M, n_per, bias, c0, pv, prior, h0, c0p, seed, offset, want_y=False, lw0=None):
    """One pp_is_statement_groups call on host arrays. bias [M, 4H]; c0 [M, H] (group-shared state) or None (per-particle
    state h0 / c0p [n, H]); pv [n]; prior [n, 2] or [2]; lw0 [n]: the log-weights the term is added to (default zeros). Every
    device buffer carries PAD poisoned (NaN) rows behind the live ones, the bias and c0 blocks also in front. Returns host
    copies (value, lw, h, c, y) INCLUDING the padding."""
    dev, H, n = run.dev, eng.spec.lstm_dim, M * n_per
    nan = float('nan')

    def padded(a, rows, front=0):
        a = np.asarray(a, np.float32).reshape(rows, -1)
        t = torch.full((front + rows + PAD, a.shape[1]), nan, dtype=torch.float32, device=dev)
        t[front:front + rows] = torch.from_numpy(a).to(dev)
        return t
    tb = padded(bias, M, front=PAD)
    tc0 = padded(c0, M, front=PAD) if c0 is not None else None
    tpv = padded(pv, n)
    shared_prior = np.asarray(prior).size == 2
    tpr = torch.from_numpy(np.asarray(prior, np.float32).reshape(-1, 2)).to(dev) if shared_prior else padded(prior, n)
    th = padded(h0, n) if h0 is not None else torch.full((n + PAD, H), nan, device=dev)
    tc = padded(c0p, n) if c0p is not None else torch.full((n + PAD, H), nan, device=dev)
    lw0 = np.zeros(n, np.float32) if lw0 is None else lw0
    tv = torch.full((n + PAD,), nan, device=dev)
    tl = padded(lw0, n)
    a, p = eng.spec.address_id[cur], eng.spec.address_id[prev]
    ldy = (int(eng.net.addrs[a].n_out) + 3) & ~3
    ty = torch.full((n + PAD, ldy), nan, device=dev) if want_y else None
    ws = _workspace(run, eng, M)
    rc = eng.lib.pp_is_statement_groups(C.byref(eng.net), eng.params.data_ptr(), a, p, M, n_per, tb[PAD:].data_ptr(),
                                        None if tc0 is None else tc0[PAD:].data_ptr(), tpv.data_ptr(), tpr.data_ptr(),
                                        0 if shared_prior else 1, th.data_ptr(), tc.data_ptr(), tv.data_ptr(), tl.data_ptr(),
                                        0 if DIST[cur] == 'Normal' else 1, seed, offset, L.ptr(ty), ldy, ws.data_ptr(), ws.numel(),
                                        L.stream_ptr())
    L.check(rc, 'pp_is_statement_groups')
    torch.cuda.synchronize()
    return tv.cpu().numpy(), tl.cpu().numpy().reshape(-1), th.cpu().numpy(), tc.cpu().numpy(), None if ty is None else ty.cpu().numpy()


# ---- 1. indexing, exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', SHAPES)
@pytest.mark.parametrize('shared', [True, False], ids=['group_state', 'particle_state'])
@pytest.mark.parametrize('H,cur', [(64, 'a_uniform'), (256, 'a_normal'), (512, 'a_uniform')])
def test_group_of_a_grouped_statement_is_the_one_group_call(H, cur, shared, M, N):
    eng, run, sd = _eng(H)
    prev = 'a_normal'
    n = M * N
    rng = np.random.default_rng(1000 * H + 10 * M + N + int(shared))
    bias = rng.normal(0.0, 1.0, (M, 4 * H)).astype(np.float32)
    c0 = rng.standard_normal((M, H)).astype(np.float32) if shared else None
    h0 = None if shared else (0.5 * rng.standard_normal((n, H))).astype(np.float32)
    c0p = None if shared else rng.standard_normal((n, H)).astype(np.float32)
    pv = rng.normal(0, 1.5, n).astype(np.float32)
    prior = _prior(DIST[cur], n, rng)
    seed, offset = 31 + H, 5 * 4096 + 3
    v, lw, h, c, _ = _groups_call(eng, run, cur, prev, M, N, bias, c0, pv, prior, h0, c0p, seed, offset)
    v2, lw2, h2, c2, _ = _groups_call(eng, run, cur, prev, M, N, bias, c0, pv, prior, h0, c0p, seed, offset)
    # nothing behind M n_per is written, everything in front of it is
    assert np.isnan(v[n:]).all() and np.isnan(lw[n:]).all() and np.isnan(h[n:]).all() and np.isnan(c[n:]).all()
    assert np.isfinite(v[:n]).all() and np.isfinite(lw[:n]).all() and np.isfinite(h[:n]).all() and np.isfinite(c[:n]).all()
    if DIST[cur] == 'Uniform':
        assert ((v[:n] >= prior[:, 0]) & (v[:n] < prior[:, 1])).all()
    for a, b in ((v, v2), (lw, lw2), (h, h2), (c, c2)):
        assert np.array_equal(_bits(a[:n]), _bits(b[:n]))
    # group g against the one-group call on row g (M = 257: a spread of groups, the first and the last among them)
    groups = range(M) if M <= 7 else [0, 1, 31, 32, 33, 128, 255, 256]
    for g in groups:
        sl = slice(g * N, (g + 1) * N)
        v1, lw1, h1, c1, _ = _groups_call(eng, run, cur, prev, 1, N, bias[g:g + 1], None if c0 is None else c0[g:g + 1], pv[sl],
                                             prior[sl], None if h0 is None else h0[sl], None if c0p is None else c0p[sl], seed,
                                             offset + g * N)
        assert np.array_equal(_bits(v[sl]), _bits(v1[:N])), (g, int(np.argmax(_bits(v[sl]) != _bits(v1[:N]))))
        assert np.array_equal(_bits(lw[sl]), _bits(lw1[:N])), (g, int(np.argmax(_bits(lw[sl]) != _bits(lw1[:N]))))
        assert np.array_equal(_bits(h[sl]), _bits(h1[:N])) and np.array_equal(_bits(c[sl]), _bits(c1[:N])), g


def test_networks_without_a_grouped_statement_kernel_are_rejected_without_a_launch():
    for H, depth in ((1024, 1), (64, 2), (96, 1)):
        eng, run, sd = is_engine(H, seed=3, depth=depth)
        M, N = 2, 8
        dev = run.dev
        ws = _workspace(run, eng, M)
        z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
        v = torch.full((M * N,), 7.0, device=dev)
        rc = eng.lib.pp_is_statement_groups(C.byref(eng.net), eng.params.data_ptr(), eng.spec.address_id['a_normal'],
                                            eng.spec.address_id['a_uniform'], M, N, z(M, 4 * H).data_ptr(), z(M, H).data_ptr(),
                                            z(M * N).data_ptr(), z(2).data_ptr(), 0, z(depth * M * N, H).data_ptr(),
                                            z(depth * M * N, H).data_ptr(), v.data_ptr(), z(M * N).data_ptr(), 0, 1, 0, None, 0,
                                            ws.data_ptr(), ws.numel(), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and bool((v == 7.0).all()), (H, depth, rc)          # PP_EINVAL, nothing written


# ---- 2. the network part against the oracle -------------------------------------------------------------------------------------
def _bias_oracle(net, sd, E_g, prev, cur, h_g):
    """float64 bias row of one group and the sum of the absolute products behind every entry (the error scale of an fp32 sum)."""
    a_prev, d_prev = prev
    a_cur, d_cur = cur
    W_ih, W_hh, b_ih, b_hh = net.lstm_layer(0)
    x = np.zeros(W_ih.shape[1])
    col = E_g.shape[0]
    S, Ed, Ea = 4, 8, 64
    x[:col] = E_g
    x[col + S:col + S + Ed] = net.P['_layers_distribution_type_embedding.' + d_prev]
    x[col + S + Ed:col + S + Ed + Ea] = net.P['_layers_address_embedding.' + a_prev]
    c2 = col + S + Ed + Ea
    x[c2:c2 + Ed] = net.P['_layers_distribution_type_embedding.' + d_cur]
    x[c2 + Ed:] = net.P['_layers_address_embedding.' + a_cur]
    ref = b_ih + b_hh + W_ih @ x + W_hh @ h_g
    scale = np.abs(b_ih) + np.abs(b_hh) + np.abs(W_ih) @ np.abs(x) + np.abs(W_hh) @ np.abs(h_g)
    return ref, scale, np.abs(W_ih[:, :col]) @ np.abs(E_g)


@pytest.mark.parametrize('H,cur,K', [(64, 'a_normal', 1), (64, 'a_uniform', 10), (256, 'a_normal', 10), (512, 'a_normal', 10),
                                     (512, 'a_uniform', 1), (512, 'a_uniform', 10), (64, 'a_normal', 10), (64, 'a_uniform', 1)])
def test_bias_rows_and_grouped_statement_against_the_oracle(H, cur, K):
    """Tolerances: (h, c) 4e-6 / 2e-5 absolute and log q 1e-4 relative to max(1, |ref|) are tests/test_gpu_is_step_fused.py's for
    the same statement. The bias row is an fp32 sum of T = lstm_in + H products, per lane T / 64 of them in sequence and a
    six-step butterfly: |error| <= (T / 64 + 8) 2^-24 sum |products| (the float64 reference's own error is 2^-29 of that); the
    device's embedding rows E_g are themselves fp32 results of four layers of at most 64 + 2 terms: 4 * 66 * 2^-24 relative, times
    the products they enter. y_out is
    checked through the quantity it exists for - log q of the drawn value under the oracle's own y - and directly to 1e-4 relative
    to max(1, |y|): the bar of everything derived from it."""
    eng, run, sd = _eng(H, K)
    prev = ('a_uniform', 'Uniform') if cur == 'a_normal' else ('a_normal', 'Normal')
    curp = (cur, DIST[cur])
    M, N = 3, 40                       # 120 particles: panels that straddle groups
    n = M * N
    rng = np.random.default_rng(H + K)
    obs = rng.uniform(5.0, 11.0, (M, 2)).astype(np.float32)
    run.init_batch(obs)
    run.first_batch(eng.spec.address_id[prev[0]])
    bias = run.bias_batch(eng.spec.address_id[cur], eng.spec.address_id[prev[0]], True)
    torch.cuda.synchronize()
    hg, cg = run._b_h.cpu().numpy(), run._b_c.cpu().numpy()
    onet = O.Net(sd, list(EMB), K=K)
    got = bias.cpu().numpy().astype(np.float64)
    T = eng.spec.lstm_in + H
    for g in range(M):
        E, _ = O.embed_observe(onet, obs[g].astype(np.float64).reshape(1, -1))
        # (the reference takes the oracle's E and the device's own h_g)
        ref, scale, scale_obs = _bias_oracle(onet, sd, E[0], prev, curp, hg[g].astype(np.float64))
        bound = (T / 64 + 8) * 2.0 ** -24 * scale + 4 * 66 * 2.0 ** -24 * scale_obs
        err = np.abs(got[g] - ref)
        assert (err <= bound).all(), (g, float((err / bound).max()))
    # the grouped statement on these rows: second statement (group-shared state), then a third one (per-particle state)
    pv = rng.normal(0, 1.5, n).astype(np.float32)
    prior = _prior(DIST[cur], n, rng)
    lw0 = np.linspace(-1.0, 1.0, n).astype(np.float32)       # (the term is ADDED to what the log-weights hold)
    v, lw, h, c, y = _groups_call(eng, run, cur, prev[0], M, N, bias.cpu().numpy(), cg, pv, prior, None, None, 5, 100, want_y=True,
                                  lw0=lw0)
    for g in range(M):
        sl = slice(g * N, (g + 1) * N)
        href, cref, lq_ref, yref = _oracle_statement(sd, H, obs[g].astype(np.float64), prev, curp, pv[sl],
                                                     np.repeat(hg[g:g + 1], N, 0), np.repeat(cg[g:g + 1], N, 0),
                                                     v[sl].astype(np.float64), prior[sl].astype(np.float64), K=K)
        assert np.abs(h[sl] - href).max() < 4e-6 and np.abs(c[sl] - cref).max() < 2e-5, g
        ey = np.abs(y[sl, :3 * K] - yref) / np.maximum(1.0, np.abs(yref))
        assert ey.max() < 1e-4 and np.isnan(y[n:]).all(), (g, float(ey.max()))
        # lw - lw0 = log p(v) - log q(v)
        lp = O.prior_log_prob(DIST[cur], prior[sl].astype(np.float64), v[sl].astype(np.float64))
        ref = lp - lq_ref
        ok = np.isfinite(ref)
        assert ok.mean() > 0.99
        err = np.abs(lw[sl][ok] - (lw0[sl].astype(np.float64)[ok] + ref[ok])) / np.maximum(1.0, np.abs(ref[ok]))
        assert err.max() < 1e-4, (g, float(err.max()))
    # third statement: per-particle state = the rows the second statement left, bias without the recurrent part
    bias3 = run.bias_batch(eng.spec.address_id[prev[0]], eng.spec.address_id[cur], False)
    prior3 = _prior(prev[1], n, rng)
    v3, _, h3, c3, y3 = _groups_call(eng, run, prev[0], cur, M, N, bias3.cpu().numpy(), None, v[:n], prior3, h[:n], c[:n], 6, 100,
                                        want_y=True)
    for g in range(M):
        sl = slice(g * N, (g + 1) * N)
        href, cref, lq_ref, yref = _oracle_statement(sd, H, obs[g].astype(np.float64), curp, prev, v[sl], h[sl], c[sl],
                                                     v3[sl].astype(np.float64), prior3[sl].astype(np.float64), K=K)
        assert np.abs(h3[sl] - href).max() < 4e-6 and np.abs(c3[sl] - cref).max() < 2e-5, g
        ey = np.abs(y3[sl, :3 * K] - yref) / np.maximum(1.0, np.abs(yref))
        assert ey.max() < 1e-4, (g, float(ey.max()))


# ---- 3. the draws as a distribution ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,cur', [(64, 'a_normal'), (512, 'a_uniform')])
def test_draws_follow_each_particles_own_proposal(H, cur):
    """Probability integral transform: u_i = F_i(v_i) with F_i the float64 mixture CDF of particle i's head outputs (y_out). The
    u_i are i.i.d. U(0, 1) whatever the F_i are; sup |F_n - F| exceeds 1.95 / sqrt(n) with probability 1e-3."""
    K = 10
    eng, run, sd = _eng(H, K)
    M, N = 5, 4000
    n = M * N
    rng = np.random.default_rng(H)
    bias = rng.normal(0.0, 1.0, (M, 4 * H)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((n, H))).astype(np.float32)
    c0p = rng.standard_normal((n, H)).astype(np.float32)
    pv = rng.normal(0, 1.5, n).astype(np.float32)
    prior = _prior(DIST[cur], n, rng)
    v, _, _, _, y = _groups_call(eng, run, cur, 'a_normal', M, N, bias, None, pv, prior, h0, c0p, 77, 0, want_y=True)
    v64 = v[:n].astype(np.float64)
    onet = O.Net(sd, list(EMB), K=K)
    _, _, (mu, sdv, p) = O.head_forward(onet, cur, DIST[cur], None, prior.astype(np.float64), v64, y=y[:n, :3 * K].astype(np.float64))
    z = O.std_normal_cdf((v64[:, None] - mu) / sdv)
    if DIST[cur] == 'Uniform':
        lo, hi = prior[:, :1].astype(np.float64), prior[:, 1:].astype(np.float64)
        a, b = O.std_normal_cdf((lo - mu) / sdv), O.std_normal_cdf((hi - mu) / sdv)
        z = np.clip((z - a) / (b - a), 0.0, 1.0)
    u = np.sort((p * z).sum(1))
    i = np.arange(1, n + 1)
    D = max(np.abs(i / n - u).max(), np.abs((i - 1) / n - u).max())
    print('KS distance of the PIT values: %.5f (bar %.5f)' % (D, 1.95 / math.sqrt(n)))
    assert D < 1.95 / math.sqrt(n)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
SIGMA = math.sqrt(2.0)
_MODELS = {}


def _program(statements):
    """a ~ Normal(1, sqrt 5); observe obs0 ~ Normal(a, .); b ~ Normal(a, 0.7); [c ~ Uniform(b - 1, b + 1);] observe obs1 ~
    Normal(last, .). `runs` counts the executions of forward()."""
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal, Uniform

    class StraightLine(Model):
        runs = 0

        def forward(self):
            type(self).runs += 1
            a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a')
            pyprob.observe(Normal(a, SIGMA), name='obs0')
            last = pyprob.sample(Normal(a, 0.7), address='b')
            if statements == 3:
                last = pyprob.sample(Uniform(last - 1.0, last + 1.0), address='c')
            pyprob.observe(Normal(last, SIGMA), name='obs1')
            return last
    return StraightLine()


def _attach_network(model, kind, H, depth=1):
    """An inference network with proposal layers for the program's addresses and trained-looking weights (helpers.is_engine's
    scaling), constructed - not trained. Returns the state dict."""
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkFeedForward, InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec
    from pyprob_amd.state import TraceMode
    tr = next(model._trace_generator(trace_mode=TraceMode.PRIOR))
    addrs = [(v.address, v.distribution.name, getattr(v.distribution, 'num_categories', None) if v.distribution.name == 'Categorical' else None)
             for v in tr.variables_controlled]
    spec = NetSpec(EMB, lstm_dim=H, lstm_depth=depth, proposal_mixture_components=10, network=kind)
    eng = ICEngine(spec, device='cuda:0', seed=2)
    eng.add_addresses(addrs)
    rng = np.random.default_rng(9)
    sd = {k: (v.numpy() * (3.0 if ('lstm' in k or 'proposal' in k) else 1.0)).astype(np.float32) for k, v in eng.state_dict().items()}
    for k in sd:
        if k.endswith('bias') or 'bias_' in k:
            sd[k] = (sd[k] + 0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
    eng.load_state_dict(sd)
    cls = InferenceNetworkFeedForward if kind == 'feedforward' else InferenceNetworkLSTM
    net = cls(observe_embeddings=EMB, lstm_dim=H, lstm_depth=depth, device='cuda:0')
    net._obs_names = list(EMB)
    net._engine = eng
    net._is = ISRunner(eng)
    net._layers_initialized = True
    model._inference_network = net
    return sd, [a for a, _, _ in addrs]


def _model(statements, kind, H, depth=1):
    key = (statements, kind, H, depth)
    if key not in _MODELS:
        model = _program(statements)
        _MODELS[key] = (model,) + _attach_network(model, kind, H, depth)
    return _MODELS[key]


def _observations(M, rng):
    return [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]


def _stats64(lw, x):
    lw, x = lw.astype(np.float64), x.astype(np.float64)
    m = lw.max()
    w = np.exp(lw - m)
    return m, w.sum(), (w * w).sum(), (w * x).sum(), (w * x * x).sum(), (w * np.abs(x)).sum()


def _rescore_group(onet, kind, addresses, post, obs, N):
    """Oracle log-weights of one group's particles under ITS observation, from the statement log of the posterior."""
    log = post.statement_log
    vals = []
    for j, a in enumerate(addresses):
        (addr, (v, _)), = log[j].items()
        assert addr == a
        vals.append(v.cpu().numpy().astype(np.float64))
    names = ['Normal', 'Normal', 'Uniform'][:len(addresses)]
    priors = [np.tile(np.array([[1.0, float(np.float32(math.sqrt(5.0)))]]), (N, 1)),
              np.stack([vals[0].astype(np.float32).astype(np.float64), np.full(N, float(np.float32(0.7)))], 1)]
    if len(addresses) == 3:
        b32 = vals[1].astype(np.float32)
        priors.append(np.stack([(b32 - np.float32(1.0)).astype(np.float64), (b32 + np.float32(1.0)).astype(np.float64)], 1))
    y = [obs['obs0'], obs['obs1']]
    if kind == 'feedforward':
        T = len(addresses)
        pr = np.zeros((N * T, 3))
        pr[:, :2] = np.stack(priors, 1).reshape(N * T, 2)
        _, _, _, lw = O.is_rescore_feedforward(onet, y, np.full(N, T, np.int64), np.tile(np.arange(T), N), np.stack(vals, 1).reshape(-1),
                                               pr, addresses, names)
    else:
        steps = [dict(address=a, dist_name=d, values=v, prior=p) for a, d, v, p in zip(addresses, names, vals, priors)]
        _, lw = O.is_rescore_lockstep(onet, y, steps, N)
    s = float(np.float32(SIGMA))
    lw = lw + np.asarray(O.normal_log_prob(y[0], vals[0], s), np.float32).astype(np.float64)
    return lw + np.asarray(O.normal_log_prob(y[1], vals[-1], s), np.float32).astype(np.float64), vals[-1]


@pytest.mark.parametrize('M,N', [(7, 300), (3, 4097)])
@pytest.mark.parametrize('statements', [2, 3])
@pytest.mark.parametrize('kind,H', [('lstm', 64), ('lstm', 512), ('feedforward', 64)])
def test_straight_line_programs_in_one_execution(kind, H, statements, M, N):
    """FAILS WITHOUT THE FEATURE: the parent raises BatchUnsupported at the second sample statement and `_batch_ok` is False."""
    model, sd, addresses = _model(statements, kind, H)
    onet = O.Net(sd, list(EMB), K=10)
    observes = _observations(M, np.random.default_rng(11 + M))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model.posterior_results_batch(N, observes, seed=13, offset=64)
        before = type(model).runs
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
    assert model._batch_ok is True and len(posts) == M
    assert type(model).runs - before == 1          # ONE execution of forward() for all M * N particles
    for g, (post, obs) in enumerate(zip(posts, observes)):
        v = post._all_values.cpu().numpy()
        lw = post._all_log_weights.cpu().numpy().astype(np.float64)
        assert v.shape == (N,) and post.length == N and np.isfinite(v).all() and len(post.statement_log) == statements
        ref, last = _rescore_group(onet, kind, addresses, post, obs, N)
        assert np.array_equal(last.astype(np.float32), v) and np.isfinite(ref).all()
        err = np.abs(lw - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() < 1e-4, (g, float(err.max()), int(err.argmax()))
        m, sw, sw2, swx, swx2, swax = _stats64(lw, v)
        st = post.device_stats
        assert st['max_lw'] == m and st['count'] == N
        assert abs(st['sum_w'] - sw) <= 1e-10 * sw and abs(st['sum_w2'] - sw2) <= 1e-10 * sw2, (g, st)
        assert abs(st['sum_wx'] - swx) <= 1e-10 * swax and abs(st['sum_wx2'] - swx2) <= 1e-10 * swx2, (g, st)
    assert len(set(round(p.mean, 3) for p in posts)) == M          # the groups see different observations


# ---- 5. sharding ----------------------------------------------------------------------------------------------------------------
def test_a_call_sharded_by_the_state_budget_returns_the_same_particles(monkeypatch):
    model, sd, addresses = _model(3, 'lstm', 64)
    M, N, H = 7, 300, 64
    observes = _observations(M, np.random.default_rng(3))
    shards = []
    run = model._run_lockstep_batch

    def recorded(obs, m, *args, **kwargs):
        shards.append(m)
        return run(obs, m, *args, **kwargs)
    monkeypatch.setattr(model, '_run_lockstep_batch', recorded)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model._batch_keeps_state = False
        whole = model.posterior_results_batch(N, observes, seed=5, offset=1000)
        assert shards == [7]
        del shards[:]
        monkeypatch.setenv('PP_BATCH_STATE_BYTES', str(3 * 8 * N * H + 100))      # (h, c) of three groups
        model._batch_keeps_state = False
        parts = model.posterior_results_batch(N, observes, seed=5, offset=1000)
        assert shards == [7, 3, 3, 1]              # the first execution stops at its second statement, then three shards
        del shards[:]
        again = model.posterior_results_batch(N, observes, seed=5, offset=1000)
        assert shards == [3, 3, 1] and model._batch_ok is True
    for a, b, c in zip(whole, parts, again):
        assert torch.equal(a._all_values, b._all_values) and torch.equal(a._all_log_weights, b._all_log_weights)
        assert torch.equal(a._all_values, c._all_values) and torch.equal(a._all_log_weights, c._all_log_weights)
        assert a.mean == b.mean and a.effective_sample_size == b.effective_sample_size
    model._batch_keeps_state = False


# ---- 6. fallbacks -----------------------------------------------------------------------------------------------------------------
def _equals_the_loop(model, observes, N, seed, offset):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=seed, offset=offset, lock_step=True)
        assert model._batch_ok is False and len(posts) == len(observes)
        for g, post in enumerate(posts):
            ref = model.posterior_results(N, IC, observe=observes[g], seed=seed, offset=offset + g * N, lock_step=True)
            assert torch.equal(post._all_values, ref._all_values) and torch.equal(post._all_log_weights, ref._all_log_weights)
            assert post.mean == ref.mean and post.effective_sample_size == ref.effective_sample_size


def test_second_statement_categorical_equals_the_loop():
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Categorical, Normal

    class NormalThenCategorical(Model):
        def forward(self):
            a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a')
            k = pyprob.sample(Categorical([0.2, 0.3, 0.5]), address='k')
            pyprob.observe(Normal(a + k, SIGMA), name='obs0')
            pyprob.observe(Normal(a, SIGMA), name='obs1')
            return a
    model = NormalThenCategorical()
    _attach_network(model, 'lstm', 64)
    _equals_the_loop(model, _observations(3, np.random.default_rng(1)), 300, 3, 10)


def test_branch_after_the_second_statement_equals_the_loop():
    model, net, meta, params = lockstep_network('cuda:0')       # Marsaglia: x, y, then `while s >= 1`
    _equals_the_loop(model, [{'obs0': 8.0, 'obs1': 9.0}, {'obs0': 7.0, 'obs1': 7.5}], 400, 3, 77)


@pytest.mark.parametrize('H,depth', [(1024, 1), (64, 2)])
def test_networks_without_a_grouped_statement_equal_the_loop(H, depth):
    model = _program(2)
    _attach_network(model, 'lstm', H, depth)
    _equals_the_loop(model, _observations(3, np.random.default_rng(2)), 300, 4, 9)
