"""pp_is_fused (csrc/is_kernels.hip is_fused_kernel: draw from the shared proposal, - log q, up to eight log-weight terms and the
importance statistics in one pass) at the C ABI, through ISRunner.step_net / ISRunner.fused and the `pyprob_hip::is_fused`
operator - every template axis (KIND -1 / 0 / 1 / 2, LEAN / general term loop, K = 10 / run-time K), every term kind and flag
word, the statistics on ill-conditioned weights and the argument checks - against the float64 restatement of the operation
(tests/oracle_ops.py `_term`, `_is_stats_cpu`; oracle/ic_oracle.py). tests/test_fused_term_matrix.py runs the term matrix
through the CPU stand-ins."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import (IS_EMB, check_fused_terms, fused_device_terms, fused_mixed_sets, fused_single_term_cases, fused_sum_ref,
                     fused_values, is_engine)
from oracle import ic_oracle as O
from pyprob_amd import lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

H = 64
OBSERVE = [8.0, 9.0]                 # what helpers.is_engine hands to ISRunner.init
FUSED_BLOCKS, FUSED_PT = 1024, 4     # is_kernels.hip: workgroups at most, particles per thread (grid sizing)
BIG = 2 ** 20 + 4097                 # more particles than FUSED_BLOCKS * 256 * FUSED_PT: every workgroup loops
_ENGINES = {}


def _eng(K=10):
    """One engine per mixture size for the whole module."""
    if K not in _ENGINES:
        _ENGINES[K] = _narrow_uniform_head(*is_engine(H, seed=3, K=K), K)
    return _ENGINES[K]


def _narrow_uniform_head(eng, run, sd, K):
    """The TruncatedNormal head scales its components with 10 x (high - low) x sigmoid(y): with weights of this size the mixture
    is flat over the interval and log q nearly a constant. A bias of -5 on the scale outputs makes the components narrower
    than the interval, so that log q depends on every component's mean, scale and truncation mass."""
    name = '_layers_proposal.a_uniform._ff._layers.1.bias'
    sd[name] = sd[name].copy()
    sd[name][K:2 * K] -= 5.0
    eng.load_state_dict(sd)
    return eng, run, sd


def _dev(a, run):
    return torch.tensor(a, dtype=torch.float32, device=run.dev)


# ---- a. the term matrix, values given -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', range(6))
def test_single_terms_without_a_draw(kind):
    """Every term kind x shared / per-particle parameters and x x every legal flag word, one term per call (KIND -1): the LEAN
    instantiation takes the Normal terms with a shared sigma and the identity, the general one everything else."""
    run = _eng()[1]
    n = 1025
    rng = np.random.default_rng(100)
    value = fused_values(n, rng)
    cases = [t for t in fused_single_term_cases(n, rng, value) if t['kind'] == kind]
    assert len(cases) >= 3
    for t in cases:
        check_fused_terms(run, [t], value, rng)


@pytest.mark.parametrize('n', [1, 1025, 70001])
def test_eight_terms_without_a_draw(n):
    """Eight terms in one call: all-LEAN, general because of ONE term (Poisson; a per-particle sigma) - the same seven Normal /
    identity terms in both instantiations -, and every kind at once with planted out-of-support particles."""
    run = _eng()[1]
    rng = np.random.default_rng(200 + n)
    value = fused_values(n, rng)
    sets = fused_mixed_sets(n, rng, value)
    for name, terms in sets.items():
        check_fused_terms(run, terms, value, rng, label=name)
    # KIND -1 with general terms AND the statistics (the planted particles' infinite weights are dropped)
    for name in ('general_poisson', 'all_kinds'):
        direct, operator, ref, back = _fused_stats_both_ways(run, fused_device_terms(sets[name], run.dev), value)
        assert ref['count'] == np.isfinite(back).sum() >= n - 8
        for st in (direct, operator):
            _assert_stats(st, ref, (name, n))


# ---- b. draw and log q -----------------------------------------------------------------------------------------------------------
HEADS = {'a_normal': ('Normal', (1.0, math.sqrt(5.0))), 'a_uniform': ('Uniform', (5.0, 9.0)), 'a_poisson': ('Poisson', (0.0, 40.0))}
_ORACLE = {}


def _proposal_oracle(K, address):
    """Float64 head outputs y [1, 3K] of the shared first statement and the oracle network."""
    if (K, address) not in _ORACLE:
        sd = _eng(K)[2]
        net = O.Net(sd, list(IS_EMB), K=K)
        dist, prior = HEADS[address]
        with np.errstate(all='ignore'):      # (the prior term of the re-scoring is not used here)
            _, _, (h, _) = O.is_rescore_lockstep(net, OBSERVE, [dict(address=address, dist_name=dist, values=np.array([6.0]),
                                                                    prior=np.array([prior]))], 1, return_state=True)
        Wp, bp = net.ff('_layers_proposal.%s._ff' % address)
        _ORACLE[(K, address)] = (net, O.ff_forward(h[:1], Wp, bp, False)[0])
    return _ORACLE[(K, address)]


def _oracle_log_q(K, address, values):
    """(float64 log q of every value, smallest truncation mass Phi(beta) - Phi(alpha) over the components with weight > 1e-6)."""
    net, y = _proposal_oracle(K, address)
    dist, prior = HEADS[address]
    n = len(values)
    lq = np.empty(n)
    params = None
    for lo in range(0, n, 1 << 17):
        v = values[lo:lo + (1 << 17)].astype(np.float64)
        lq[lo:lo + len(v)], _, params = O.head_forward(net, address, dist, None, np.tile(np.array([prior]), (len(v), 1)), v,
                                                       y=np.tile(y, (len(v), 1)))
    mass = 1.0
    if dist != 'Normal':
        mu, sd, p = (a[0] for a in params[:3])
        z = O.std_normal_cdf((prior[1] - mu) / sd) - O.std_normal_cdf((prior[0] - mu) / sd)
        mass = float(z[p > 1e-6].min())
    return lq, mass


def _term(kind, n, p0=None, p1=None, x=None, scale=1.0, flags=0, s0=0, s1=0):
    f = np.float32
    return dict(kind=kind, p0=None if p0 is None else np.asarray(p0, f).reshape(-1), s0=s0, p1=None if p1 is None else np.asarray(p1, f).reshape(-1),
                s1=s1, x=None if x is None else np.asarray(x, f).reshape(-1), scale=float(f(scale)), flags=flags, out=np.zeros(n, bool),
                label='kind%d flags%d' % (kind, flags))


def _draw_terms(address, lean, n, rng):
    """The terms of a GaussianUnknownMean-shaped call: the prior at the drawn value and two Normal observes around it. LEAN:
    Normal terms with one sigma each. General: the prior term of the head's own family (Uniform / Poisson), or a Normal with a
    per-particle sigma."""
    dist, prior = HEADS[address]
    observes = [_term(0, n, p1=[math.sqrt(2.0)], x=[8.0], flags=1), _term(0, n, p1=[1.1], x=[9.0], flags=1, scale=0.37)]
    if lean:
        return [_term(0, n, p0=[1.0], p1=[math.sqrt(5.0)], flags=4)] + observes
    if dist == 'Normal':
        return [_term(0, n, p0=[1.0], p1=rng.uniform(1.0, 3.0, n), s1=1, flags=4, scale=-1.0)] + observes
    if dist == 'Uniform':
        return [_term(1, n, p0=[prior[0]], p1=[prior[1]], flags=4)] + observes
    return [_term(3, n, p0=[4.2], flags=4)] + observes


def _slice_terms(terms, lo):
    out = []
    for t in terms:
        t = dict(t)
        for k, s in (('p0', t['s0']), ('p1', t['s1']), ('x', 1)):
            if t[k] is not None and t[k].size > 1 and s == 1:
                t[k] = t[k][lo:].copy()
        t['out'] = t['out'][lo:]
        out.append(t)
    return out


def _fused_draw(run, a, prior, terms, n, offset, seed, stats=False):
    run.begin(n, offset=offset)
    run.step_net(a, None)
    value = torch.full((n,), float('nan'), device=run.dev)
    lw = torch.full((n,), float('nan'), device=run.dev)
    st = run.fused(a, prior, fused_device_terms(terms, run.dev), value, lw, True, seed=seed, stats=stats)
    return value.cpu().numpy(), lw.cpu().numpy(), st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _draw_case(address, K, lean, n):
    eng, run, sd = _eng(K)
    dist, pr = HEADS[address]
    a = eng.spec.address_id[address]
    prior = torch.tensor([pr], dtype=torch.float32, device=run.dev)
    rng = np.random.default_rng(1000 * K + n)
    seed, offset = 17 + K, 3 * 4096 + 5
    terms = _draw_terms(address, lean, n, rng)
    # the per-term path: pp_is_step, the same Philox stream
    run.begin(n, offset=offset)
    v_step, lq_step = (t.cpu().numpy() for t in run.step(a, None, prior, seed=seed))
    # the fused pass with every scale zero: the instantiation the terms select, lw = - log q and nothing else
    zero = [dict(t, scale=0.0) for t in terms]
    v0, lw0, _ = _fused_draw(run, a, prior, zero, n, offset, seed)
    assert np.array_equal(_bits(v0), _bits(v_step))
    assert np.isfinite(v0).all() and np.isfinite(lw0).all()
    np.testing.assert_allclose(-lw0, lq_step, rtol=1e-5, atol=1e-5)
    ref, mass = _oracle_log_q(K, address, v0)
    # (asserted on the float64 oracle alone: below this mass the fp32 difference of two CDFs does not carry log Z to 1e-4)
    assert mass >= 1e-3, (address, K, mass)
    assert np.isfinite(ref).all()
    err = np.abs(-lw0.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() < 1e-4, (address, K, lean, n, float(err.max()), int(err.argmax()))
    # ... and with the terms' own scales: the same values, lw = - log q + the float64 sum of the terms
    want_stats = dist != 'Normal'          # (values of one sign: the bound of the statistics holds)
    v1, lw1, st = _fused_draw(run, a, prior, terms, n, offset, seed, stats=want_stats)
    assert np.array_equal(_bits(v1), _bits(v0))
    want, tol = fused_sum_ref(terms, v1, lw0, False)
    e1 = np.abs(lw1.astype(np.float64) - want)
    assert (e1 <= tol).all(), (address, K, lean, n, float((e1 / tol).max()), int((e1 / tol).argmax()))
    if want_stats:
        _assert_stats(st, _host_stats(lw1, v1), (address, K, lean, n))
    # the counter offset: the second half of the call is a call of its own
    h = n // 2
    v2, lw2, _ = _fused_draw(run, a, prior, _slice_terms(terms, h), n - h, offset + h, seed)
    assert np.array_equal(_bits(v2), _bits(v1[h:])) and np.array_equal(_bits(lw2), _bits(lw1[h:]))


@pytest.mark.parametrize('n', [1, 255, 1025, 70001])
@pytest.mark.parametrize('lean', [True, False], ids=['lean', 'general'])
@pytest.mark.parametrize('K', [1, 3, 10, 16])
@pytest.mark.parametrize('address', list(HEADS))
def test_draw_and_log_q(address, K, lean, n):
    """KIND 0 / 1 / 2 x K x LEAN / general: values bit-identical to pp_is_step, - log q against the float64 oracle (1e-4 on every
    particle) and against pp_is_step's log q, the terms on top of it, the Philox counter offset. K = 10 with LEAN terms is the
    KC = 10 instantiation (KIND 0 and 1)."""
    _draw_case(address, K, lean, n)


@pytest.mark.parametrize('address', list(HEADS))
def test_draw_and_log_q_when_every_workgroup_loops(address):
    assert BIG > FUSED_BLOCKS * 256 * FUSED_PT
    _draw_case(address, 10, True, BIG)


# ---- c. the statistics of the fused pass ---------------------------------------------------------------------------------------
def _host_stats(lw, value):
    """_is_stats_cpu's definition in float64 on what the device wrote back (non-finite weights dropped)."""
    import oracle_ops
    from pyprob_amd.is_engine import ISRunner
    out = oracle_ops._is_stats_cpu(torch.from_numpy(np.ascontiguousarray(lw)), torch.from_numpy(np.ascontiguousarray(value)), None)
    return ISRunner._stats_dict(out.numpy())


def _assert_stats(st, ref, what):
    """Each weight is expf of an exact fp32 difference, within 2 ulp (1.2e-7) of exact: the four sums are within 2.4e-7 relative
    (x of one sign), ess = sum_w^2 / sum_w2 and mean = sum_wx / sum_w within 1e-6 - the figure tests/test_gpu_is_fused.py uses
    between its two device paths. var = sum_wx2 / sum_w - mean^2: both parts are within 4.8e-7 and 9.6e-7 of sum_wx2 / sum_w
    (mean^2 <= sum_wx2 / sum_w), bound 2e-6 relative to sum_wx2 / sum_w. max_lw and count are exact."""
    assert st['count'] == ref['count'] and st['max_lw'] == ref['max_lw'], (what, st, ref)
    if ref['count'] == 0:
        assert st['sum_w'] == 0.0 and st['sum_w2'] == 0.0 and st['ess'] == 0.0 and math.isnan(st['mean']) and st['max_lw'] == -math.inf, (what, st)
        return
    for k in ('sum_w', 'sum_w2', 'sum_wx', 'sum_wx2', 'ess', 'mean'):
        assert abs(st[k] - ref[k]) <= 1e-6 * abs(ref[k]), (what, k, st[k], ref[k])
    assert abs(st['var'] - ref['var']) <= 2e-6 * ref['sum_wx2'] / ref['sum_w'], (what, st['var'], ref['var'])


def _fused_stats_both_ways(run, dterms, value):
    """pp_is_fused with the values given and the statistics, both ways the product asks for them: ISRunner.fused(stats=True) - on
    the device the pinned, polled record of _fused_stats_direct - and the `pyprob_hip::is_fused` operator with a device scratch
    tensor, which copies the record back. Returns (direct, operator, float64 statistics of the log-weights and values the
    device wrote back, those log-weights)."""
    from pyprob_amd.ops import ops
    n = len(value)
    run.begin(n)
    tv = _dev(value, run)
    lw = torch.full((n,), 7.0, device=run.dev)
    direct = run.fused(None, None, dterms, tv, lw, True, stats=True)
    back = lw.cpu().numpy()
    lw2 = torch.full((n,), 7.0, device=run.dev)
    cols = [[int(t[0][0]) for t in dterms], [t[0][1] for t in dterms], [int(t[0][2]) for t in dterms], [t[0][3] for t in dterms],
            [int(t[0][4]) for t in dterms], [t[1] for t in dterms], [float(t[2]) for t in dterms], [int(t[3]) for t in dterms]]
    out = ops.is_fused(run.ws, run.eng.net_handle, -1, None, *cols, tv, lw2, True, 0, 0, run._stats_scratch)
    operator = run._stats_dict(out)
    assert np.array_equal(_bits(lw2.cpu().numpy()), _bits(back))
    assert np.array_equal(_bits(tv.cpu().numpy()), _bits(value))
    return direct, operator, _host_stats(back, value), back


def _blocks(n):
    return min(FUSED_BLOCKS, -(-n // (256 * FUSED_PT)))


def _weights(layout, n, rng):
    i = np.arange(n)
    base = (3.0 * rng.standard_normal(n) - 40.0).astype(np.float32)
    if layout == 'ascending':          # every thread's maximum rises at every particle
        return (-3e4 + 3e4 * i / max(n - 1, 1)).astype(np.float32)
    if layout == 'descending':
        return (-3e4 * i / max(n - 1, 1)).astype(np.float32)
    if layout == 'ascending_30':       # ... and the particles before the new maximum still count after the rescale
        return (-30.0 + 30.0 * i / max(n - 1, 1)).astype(np.float32)
    if layout == 'descending_30':
        return (-30.0 * i / max(n - 1, 1)).astype(np.float32)
    if layout == 'one_dominates':
        lw = np.full(n, -200.0, np.float32)
        lw[n // 3] = 0.0
        return lw
    if layout == 'equal':
        return np.full(n, -12.5, np.float32)
    if layout == 'non_finite_mix':     # 5 % -inf, a few NaN, one +inf
        base[::20] = -np.inf
        if n > 8:
            base[[3, n // 2, n - 2]] = np.nan
            base[n // 3] = np.inf
        return base
    if layout == 'workgroup_non_finite':      # every particle of ONE workgroup's grid stride
        b = _blocks(n) - 1
        base[((i // 256) % _blocks(n)) == b] = np.where(i[((i // 256) % _blocks(n)) == b] % 2 == 0, -np.inf, np.nan)
        return base
    if layout == 'all_non_finite':
        return np.where(i % 3 == 0, np.nan, np.where(i % 3 == 1, -np.inf, np.inf)).astype(np.float32)
    raise ValueError(layout)


LAYOUTS = ['ascending', 'descending', 'ascending_30', 'descending_30', 'one_dominates', 'equal', 'non_finite_mix', 'workgroup_non_finite',
           'all_non_finite']


@pytest.mark.parametrize('n', [1, 1000, 70001, BIG])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_fused_statistics(layout, n):
    """Values given and ONE identity term: the test chooses the log-weights exactly. Both ways the product asks for the
    statistics - ISRunner.fused(stats=True) (the pinned, polled record) and the operator with a device scratch tensor - against
    the float64 statistics of what the device wrote back."""
    run = _eng()[1]
    rng = np.random.default_rng(n % 1000 + len(layout))
    weights = _weights(layout, n, rng)
    value = fused_values(n, rng)
    direct, operator, ref, back = _fused_stats_both_ways(run, [((2, None, 0, None, 0), _dev(weights, run), 1.0, 0)], value)
    assert np.array_equal(back, weights, equal_nan=True)
    finite = np.isfinite(weights)
    assert ref['count'] == finite.sum()
    for st in (direct, operator):
        _assert_stats(st, ref, (layout, n))
        if layout == 'one_dominates':
            assert abs(st['ess'] - 1.0) <= 1e-6
        if layout == 'equal':
            assert abs(st['ess'] - n) <= 1e-6 * n
        if layout == 'all_non_finite' or (layout == 'workgroup_non_finite' and _blocks(n) == 1):
            assert st['count'] == 0 and st['ess'] == 0.0 and math.isnan(st['mean'])


# ---- d. the argument checks (all rejected before any launch) ------------------------------------------------------------------
def test_argument_checks():
    eng, run, sd = _eng()
    lib = run.lib
    n = 64
    run.begin(n)
    value, lw = _dev(np.linspace(5, 9, n), run), _dev(np.linspace(-3, 3, n), run)
    v0, l0 = value.cpu().numpy().copy(), lw.cpu().numpy().copy()
    p = _dev(np.full(n * 4, 0.5), run)
    prior = _dev([0.0, 1.0], run)
    stats = torch.zeros(8, dtype=torch.float64, device=run.dev)
    good = dict(kind=0, p0=p, p1=p, x=p, s0=1, s1=1, sx=1, flags=0)

    def call(terms, addr_id=-1, stats_out=None, scratch=None):
        arr = (L.pp_lw_term * max(len(terms), 1))()
        fl = (C.c_int32 * max(len(terms), 1))()
        for q, t in enumerate(terms):
            t = dict(good, **t)
            arr[q].kind, arr[q].p0_stride, arr[q].p1_stride, arr[q].x_stride = t['kind'], t['s0'], t['s1'], t['sx']
            arr[q].p0, arr[q].p1, arr[q].x, arr[q].scale = L.ptr(t['p0']), L.ptr(t['p1']), L.ptr(t['x']), 1.0
            fl[q] = t['flags']
        return lib.pp_is_fused(C.byref(eng.net), addr_id, n, L.ptr(prior), arr, fl, len(terms), value.data_ptr(), lw.data_ptr(), 0, 1, 0,
                               L.ptr(stats_out), L.ptr(scratch), run.ws.data_ptr(), run.ws_bytes, L.stream_ptr())
    cases = {
        'nine terms': dict(terms=[{}] * 9),
        'kind 6': dict(terms=[dict(kind=6)]),
        'kind -1': dict(terms=[dict(kind=-1)]),
        'flag 1 on Poisson': dict(terms=[dict(kind=3, flags=1)]),
        'flag 2 on Poisson': dict(terms=[dict(kind=3, flags=2)]),
        'no x and no flag 4': dict(terms=[dict(x=None)]),
        'Categorical with p1_stride 0': dict(terms=[dict(kind=5, s0=4, s1=0)]),
        'statistics without scratch': dict(terms=[{}], stats_out=stats),
        'draw at a Categorical address': dict(terms=[{}], addr_id=eng.spec.address_id['a_cat']),
        'draw at a Bernoulli address': dict(terms=[{}], addr_id=eng.spec.address_id['a_bern']),
    }
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc == -1, (name, rc)                       # PP_EINVAL (include/pyprob_amd.h)
        assert b'pp_is_fused' in lib.pp_last_error(), (name, lib.pp_last_error())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(value.cpu().numpy()), _bits(v0)) and np.array_equal(_bits(lw.cpu().numpy()), _bits(l0)), name
    assert call([{}]) == 0 and call([{}] * 8, stats_out=stats, scratch=run._stats_scratch) == 0      # the accepted neighbours
    torch.cuda.synchronize()
    assert not np.array_equal(lw.cpu().numpy(), l0)
