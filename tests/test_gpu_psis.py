"""pp_is_psis_groups (csrc/is_psis.hip) on the device against tests/psis_ref.py, on the READ-BACK output of the device sort keyed on
the log-weights (the sort is pinned by tests/test_gpu_order_stats.py: this isolates the new kernels).

1. EXACT: n, m, f, c and the cutoff; every particle outside the tail, and every particle of a group without a fit, leaves with its
   input bits (non-finite ones and NaN payloads included); no-fit groups report k-hat = +inf and sigma NaN; smoothed log-weights
   ascend with tail rank and stay at or below the maximum; poisoned rows around lw_out and out survive; lw_out = NULL writes only
   `out` and the same bits; two calls are bit-equal; group g of an M-group call equals the one-group call on its slice.
2. FP64: k-hat and sigma against psis_ref in numpy.longdouble. The bound per case is 16 times the error the float64 psis_ref itself
   shows against the long-double one on that case (the two differ in summation order and libm, as the kernel does), never below
   64 ulp of fp64. PP_PSIS_ERRORS=<file> makes the test append kernel error, float64-restatement error and bound per case, and the
   share of tail particles whose smoothed float32 log-weight is not bit-equal (all are within 1 ulp of float32), to that file:
   profiles/psis_errors.jsonl.
3. END TO END on the three-statement straight-line program at H = 64 of tests/test_gpu_intervals.py.

The 66000-group shape repeats a block of PERIOD groups: the reference is computed for one block and every group must carry the
bits of its twin in the first block - which is also the statement that a result does not depend on M or on the launch chunk."""
import json
import os
import warnings

import numpy as np
import pytest

import psis_ref as PR
from pyprob_amd import lib as L

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 2
POISON = -12345.5
WIDTH = 8
KINDS = 9
PERIOD = 27
# (M, N, tail): first kind of the cycle
SHAPES = [(1, 1, 0), (1, 20, 0), (1, 24, 0), (3, 257, 0), (2, 2048, 0), (2, 2049, 0), (1, 70001, 0), (1, 600001, 0),
          (1, 70001, 10000), (1, 600001, 100000), (66000, 30, 0)]
FIRST_KIND = {(1, 1, 0): 0, (1, 20, 0): 0, (1, 24, 0): 0, (3, 257, 0): 3, (2, 2048, 0): 6, (2, 2049, 0): 7, (1, 70001, 0): 1,
              (1, 600001, 0): 2, (1, 70001, 10000): 7, (1, 600001, 100000): 0, (66000, 30, 0): 0}
KIND_NAMES = ('pareto k=0.2', 'pareto k=0.7', 'pareto k=1.2', 'bounded tail', 'five integer values', 'all equal',
              'spread above 1500', 'non-finite scattered', 'nothing finite')
NAN_PAYLOAD = 0x7FC12345
_CASES = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _group(kind, N, rng):
    U = 1.0 - rng.random(N)                      # (0, 1]
    if kind in (0, 1, 2):
        lw = (-(0.2, 0.7, 1.2)[kind] * np.log(U) + 3.0).astype(np.float32)
    elif kind == 3:
        lw = (np.log(U) - 1.0).astype(np.float32)                  # weights uniform on (0, 1]: a bounded tail
    elif kind == 4:
        lw = rng.integers(0, 5, N).astype(np.float32)
    elif kind == 5:
        lw = np.full(N, 1.5, np.float32)
    elif kind == 6:
        lw = (-20000.0 - 1500.0 * U).astype(np.float32)            # exp(lw - max) underflows in the whole tail but its top, in
                                                                   # fp64 and in the long-double restatement alike: y_0 = 0
        lw[int(rng.integers(N))] = 0.0
    elif kind == 7:
        lw = (-0.5 * np.log(U)).astype(np.float32)
        hit = np.nonzero(rng.random(N) < 0.1)[0]
        lw[hit[0::3]] = -np.inf
        lw[hit[1::3]] = np.inf
        lw.view(np.uint32)[hit[2::3]] = NAN_PAYLOAD
    else:
        lw = np.full(N, -np.inf, np.float32)
        lw[1::3] = np.inf
        lw.view(np.uint32)[2::3] = NAN_PAYLOAD
    return lw


def _inputs(M, N, tail):
    rng = np.random.default_rng(1000 * N + tail + M)
    block = min(M, PERIOD)
    first = np.stack([_group((FIRST_KIND[(M, N, tail)] + g) % KINDS, N, rng) for g in range(block)])
    reps = -(-M // block)
    return np.tile(first, (reps, 1))[:M].copy(), block


def _call(ls, index, counted, M, N, tail, want_weights=True, stats=None):
    """One pp_is_psis_groups call on device tensors; lw_out and out carry PAD poisoned rows on either side. Host copies of the live
    rows (lw_out as float32 [M, N] or None)."""
    lib = L.load()
    out = torch.full((PAD + M + PAD, WIDTH), POISON, dtype=torch.float64, device=DEV)
    lw_out = torch.full((PAD + M + PAD, N), POISON, dtype=torch.float32, device=DEV)
    need = lib.pp_is_psis_workspace_bytes(M, N, tail)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_psis_groups(ls.data_ptr(), index.data_ptr(), counted.data_ptr(), M, N, L.ptr(stats), tail,
                                  lw_out[PAD:].data_ptr() if want_weights else None, out[PAD:].data_ptr(), ws.data_ptr(), need,
                                  L.stream_ptr()), 'pp_is_psis_groups')
    torch.cuda.synchronize()
    out, lw_out = out.cpu().numpy(), lw_out.cpu().numpy()
    assert (out[:PAD] == POISON).all() and (out[PAD + M:] == POISON).all()
    assert (lw_out[:PAD] == POISON).all() and (lw_out[PAD + M:] == POISON).all()
    if not want_weights:
        assert (lw_out == POISON).all()
    return (lw_out[PAD:PAD + M] if want_weights else None), out[PAD:PAD + M]


def _case(M, N, tail):
    """The inputs, the device sort and its read-back, the device call and the two restatements of a shape: computed once, never
    modified."""
    key = (M, N, tail)
    if key not in _CASES:
        from pyprob_amd import ops as P
        lw, block = _inputs(M, N, tail)
        d_lw = _dev(lw.reshape(-1))
        _, ls, index, counted = P.ops.is_sort_groups(d_lw, d_lw, N, None)
        torch.cuda.synchronize()
        h_ls, h_index, h_counted = ls.cpu().numpy().reshape(M, N), index.cpu().numpy().reshape(M, N), counted.cpu().numpy()
        got_lw, got = _call(ls, index, counted, M, N, tail)
        ref64 = PR.psis_ref(h_ls[:block], h_index[:block], h_counted[:block], tail, np.float64)
        refL = PR.psis_ref(h_ls[:block], h_index[:block], h_counted[:block], tail, np.longdouble)
        _CASES[key] = dict(lw=lw, block=block, ls=ls, index=index, counted=counted, h_ls=h_ls, h_index=h_index, h_counted=h_counted,
                           got_lw=got_lw, got=got, ref64=ref64, refL=refL)
    return _CASES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _ordinal(a):
    """float32 -> integers whose difference counts the representable numbers between two values."""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _ulps(err, ref):
    return float(err / np.spacing(np.float64(max(abs(float(ref)), 2.0 ** -1000))))


def _record(rec):
    print('psis %s' % json.dumps(rec))
    path = os.environ.get('PP_PSIS_ERRORS')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')


@pytest.mark.parametrize('M,N,tail', SHAPES)
def test_fit_and_smoothed_weights_against_the_restatement(M, N, tail):
    c = _case(M, N, tail)
    block, got, got_lw = c['block'], c['got'], c['got_lw']
    lw_ref64, out64 = c['ref64']
    lw_refL, outL = c['refL']
    # every group carries the bits of its twin in the first block
    twins = np.arange(M) % block
    assert np.array_equal(_bits(got), _bits(got[twins])) and np.array_equal(_bits(got_lw), _bits(got_lw[twins]))
    fitted = 0
    for g in range(block):
        kind = (FIRST_KIND[(M, N, tail)] + g) % KINDS
        row, r64, rL = got[g], out64[g], outL[g]
        # integers and the cutoff, exactly (NaN where there is none)
        for k in (2, 3, 4, 6):
            assert row[k] == float(rL[k]) == r64[k], (g, k, row, rL)
        for k in (5, 7):
            assert _bits(np.float64(row[k]).reshape(1))[0] == _bits(np.float64(rL[k]).reshape(1))[0] or \
                (np.isnan(row[k]) and np.isnan(float(rL[k]))), (g, k, row, rL)
        n, m, f, cnt = int(row[2]), int(row[3]), int(row[4]), int(row[6])
        assert cnt == int(c['h_counted'][g, 0]) == int(np.isfinite(c['lw'][g]).sum())
        order = c['h_index'][g].astype(np.int64)
        tail_particles = order[f:cnt] if (m > 0 and np.isfinite(row[0])) else order[:0]
        outside = np.ones(N, bool)
        outside[tail_particles] = False
        # outside the tail (everything, without a fit): the input bits
        assert np.array_equal(_bits(got_lw[g])[outside], _bits(c['lw'][g])[outside]), (g, kind)
        if m == 0:
            assert row[0] == np.inf and np.isnan(row[1]) and float(rL[0]) == np.inf, (g, kind, row)
            assert np.array_equal(_bits(got_lw[g]), _bits(c['lw'][g]))
            continue
        fitted += 1
        assert m == 30 + int(np.floor(np.sqrt(n))) and n == cnt - f and n > 4
        rec = {'shape': [M, N, tail], 'group': g, 'kind': KIND_NAMES[kind], 'n': n, 'm': m}
        ok = True
        for k, name in ((0, 'khat'), (1, 'sigma')):
            err = abs(np.longdouble(row[k]) - rL[k])
            e64 = abs(np.longdouble(r64[k]) - rL[k])
            bound = max(16 * e64, 64 * np.longdouble(np.spacing(np.float64(abs(float(rL[k]))))))
            rec[name] = float(row[k])
            rec[name + '_err_ulp'] = _ulps(err, rL[k])
            rec[name + '_f64_restatement_err_ulp'] = _ulps(e64, rL[k])
            rec[name + '_bound_ulp'] = _ulps(bound, rL[k])
            ok = ok and bool(err <= bound)
        sm, want = got_lw[g][tail_particles], lw_refL[g][tail_particles]
        rec['tail_not_bit_equal_share'] = float(np.mean(_bits(sm) != _bits(want))) if len(sm) else 0.0
        rec['tail_max_ulp32'] = int(np.abs(_ordinal(sm) - _ordinal(want)).max()) if len(sm) else 0
        _record(rec)
        assert ok, rec
        assert rec['tail_max_ulp32'] <= 1, rec
        assert (np.diff(sm.astype(np.float64)) >= 0).all() and sm.max() <= np.float32(row[7]), (g, kind)
    if (M, N, tail) in ((1, 1, 0), (1, 20, 0)):
        assert fitted == 0
    elif M == 1 or (M, N, tail) == (66000, 30, 0):
        assert fitted >= 1


@pytest.mark.parametrize('M,N,tail', SHAPES)
def test_bit_identity_of_calls_groups_and_the_diagnostic_only_call(M, N, tail):
    c = _case(M, N, tail)
    again_lw, again = _call(c['ls'], c['index'], c['counted'], M, N, tail)
    assert np.array_equal(_bits(again), _bits(c['got'])) and np.array_equal(_bits(again_lw), _bits(c['got_lw']))
    none, only = _call(c['ls'], c['index'], c['counted'], M, N, tail, want_weights=False)
    assert none is None and np.array_equal(_bits(only), _bits(c['got']))
    # with the statistics of the groups (their maxima): the same bits
    stats = np.zeros((M, 6))
    stats[:, 0] = np.where(np.isfinite(c['lw']), c['lw'], -np.inf).astype(np.float64).max(axis=1)
    with_lw, with_stats = _call(c['ls'], c['index'], c['counted'], M, N, tail, stats=_dev(stats))
    assert np.array_equal(_bits(with_stats), _bits(c['got'])) and np.array_equal(_bits(with_lw), _bits(c['got_lw']))
    for g in sorted({0, M // 2, M - 1, min(M - 1, 65535), min(M - 1, 65536)}):
        if M == 1:
            break
        sl = slice(g * N, (g + 1) * N)
        one_lw, one = _call(c['ls'][sl], c['index'][sl], c['counted'][g:g + 1], 1, N, tail)
        assert np.array_equal(_bits(one[0]), _bits(c['got'][g])) and np.array_equal(_bits(one_lw[0]), _bits(c['got_lw'][g])), g


def test_operator_shapes_types_and_argument_checks():
    from pyprob_amd import ops as P
    M, N = 3, 257
    c = _case(M, N, 0)
    lw_out, out = P.ops.is_psis_groups(c['ls'], c['index'], c['counted'], N, None, 0, True)
    assert lw_out.dtype == torch.float32 and lw_out.shape == (M * N,) and out.dtype == torch.float64 and out.shape == (M, WIDTH)
    assert np.array_equal(_bits(lw_out.cpu().numpy().reshape(M, N)), _bits(c['got_lw']))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(c['got']))
    none, only = P.ops.is_psis_groups(c['ls'], c['index'], c['counted'], N, None, 0, False)
    assert none is None and torch.equal(only.view(torch.int64), out.view(torch.int64))
    for bad in (lambda: P.ops.is_psis_groups(c['ls'].double(), c['index'], c['counted'], N, None, 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'].long(), c['counted'], N, None, 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'][:-1], c['counted'], N, None, 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'], c['counted'][:2], N, None, 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'], c['counted'].long(), N, None, 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'], c['counted'], N + 1, None, 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'], c['counted'], N, torch.zeros(2, device=DEV), 0, True),
                lambda: P.ops.is_psis_groups(c['ls'], c['index'], c['counted'], N, None, -1, True)):
        with pytest.raises(RuntimeError):
            bad()


@pytest.mark.parametrize('N', [300, 4097])
def test_straight_line_program_end_to_end(N):
    from pyprob_amd.distributions import Empirical, PsisFit
    from test_gpu_joint_moments import _log_columns, _posterior, _straight_line_model
    _straight_line_model()
    post = _posterior(N)
    assert post._device_backed() and post.length == N
    lw, values = post._log_weights.cpu().numpy(), post._values.cpu().numpy()
    host = Empirical(values=list(values.astype(np.float64)), log_weights=list(lw.astype(np.float64)))
    k = post.pareto_k()
    assert isinstance(k, float) and np.isfinite(k) and '_dev_lw_sorted' in post.__dict__
    assert abs(k - host.pareto_k()) <= 1e-12 * max(1.0, abs(k))
    assert post.pareto_k() == k
    for tail in (None, 40):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sm, hs = post.psis(tail), host.psis(tail)
        assert sm._device_backed() and sm.length == N and isinstance(sm.fit, PsisFit) and sm.metadata['op'] == 'psis'
        assert sm.fit.khat == post.pareto_k(tail) and (tail is None or sm.fit.tail == tail)
        assert (sm.fit.tail, sm.fit.grid, sm.fit.count, sm.fit.log_cutoff) == (hs.fit.tail, hs.fit.grid, hs.fit.count, hs.fit.log_cutoff)
        assert abs(sm.fit.khat - hs.fit.khat) <= 1e-12 * max(1.0, abs(hs.fit.khat))
        assert abs(sm.fit.sigma - hs.fit.sigma) <= 1e-12 * abs(hs.fit.sigma)
        got, want = sm._log_weights.cpu().numpy(), hs.log_weights_numpy().astype(np.float32)
        assert np.abs(_ordinal(got) - _ordinal(want)).max() <= 1
        changed = np.nonzero(_bits(got) != _bits(lw))[0]
        assert len(changed) <= sm.fit.tail and (lw[changed] > sm.fit.log_cutoff).all()
        assert torch.equal(sm._values, post._values)
        assert abs(sm.fit.ess_before - post.effective_sample_size) == 0 and abs(sm.fit.ess_after - hs.fit.ess_after) <= 1e-6 * hs.fit.ess_after
        assert sm._all_log_weights.data_ptr() == sm._log_weights.data_ptr()            # (no particle dropped: the kernel's tensor)
    # the statement log travels: marginal / joint answer under the smoothed weights
    a = _log_columns(post)[0][1].cpu().numpy().astype(np.float64)
    ma = sm.marginal('mu')
    w = np.exp(got.astype(np.float64) - got.astype(np.float64).max())
    assert ma._device_backed() and abs(ma.mean - float((w * a).sum() / w.sum())) <= 1e-6 * max(1.0, abs(ma.mean))
    assert sm.joint().count == N and len(sm.resample_joint(16, seed=3)['index']) == 16


def test_batch_calls_are_one_operator_call_each_and_equal_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from test_gpu_joint_moments import _straight_line_model
    model, full = _straight_line_model()
    M, N = 3, 300
    rng = np.random.default_rng(5)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
        loop_k = np.array([p.pareto_k() for p in posts])
        loop = [p.psis() for p in posts]
    assert model._batch_ok is True and len(posts) == M
    names = ('sort', 'psis')
    count = {k: 0 for k in names}
    real = {k: getattr(P.ops, 'is_%s_groups' % k) for k in names}

    def counted(name):
        def call(*a):
            count[name] += 1
            return real[name](*a)
        return call
    for name in real:
        monkeypatch.setattr(P.ops, 'is_%s_groups' % name, counted(name), raising=False)
    fast_k = pyprob_amd.pareto_k_batch(posts)
    assert count == {'sort': 1, 'psis': 1} and fast_k.dtype == np.float64 and fast_k.shape == (M,)
    assert np.array_equal(_bits(fast_k), _bits(loop_k))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fast = pyprob_amd.psis_batch(posts)
        assert count == {'sort': 2, 'psis': 2} and len(fast) == M
        for f, l in zip(fast, loop):
            assert torch.equal(f._log_weights.view(torch.int32), l._log_weights.view(torch.int32)) and f.fit.khat == l.fit.khat
            assert f.fit.sigma == l.fit.sigma and f.fit.ess_after == l.fit.ess_after and f.metadata['op'] == 'psis'
            assert abs(f.marginal('mu').mean - l.marginal('mu').mean) == 0
        mixed = pyprob_amd.pareto_k_batch([posts[i] for i in (2, 0, 1)])
    assert np.array_equal(mixed, loop_k[[2, 0, 1]]) and count['psis'] == 2 + M
    assert pyprob_amd.pareto_k_batch([]).shape == (0,) and pyprob_amd.psis_batch([]) == []
