"""pp_is_reobserve_groups (csrc/is_reobserve.hip) straight through the C ABI: out[g N + j] = lw[j] + (sum_t scale_t lp_t(g, j) -
old[j]) must have the BITS of the float32 composition of pp_obs_logweight's lp_out (called per group, the group's row as one
shared row) and the accumulate route's `old` - for every family, every width (several rows per wave, the U = 4 trip, the slot
wrap, cut groups, unaligned rows), particle tiles and group chunks that are crossed, 1 / 2 / 8 terms and every parameter form;
then the identity, float64, the edge values, untouched memory and the refusals."""
import numpy as np
import pytest

import obs_logweight_ref as OR
import reobserve_ref as RR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

KS = (1, 3, 4, 5, 129, 257, 1030)
MN = ((1, 7), (2, 1), (5, 3), (3, 64), (2, 67), (3, 300), (70, 5))      # (M groups, N particles)
NMAX, KMAX = 300, 1030
SENTINEL = -12345.5


def bar(ref):
    """The project's bar for these kernels (tests/test_gpu_obs_logweight.py): rtol 1e-4, atol 1e-4 * max(1, |ref|max)."""
    return dict(rtol=1e-4, atol=1e-4 * max(1.0, float(np.max(np.abs(ref)))))


@pytest.fixture(scope='module')
def lib():
    from pyprob_amd import lib as L
    return L.load()


def pool(kind):
    """Parameters p0..p3 and values x, [NMAX, KMAX] float32: ANY pairing of a value row with the parameters of any particle lies
    inside the support and every log-density is finite (tests/test_gpu_obs_logweight_groups.py:pool, at this file's sizes)."""
    g = np.random.RandomState(177 + kind)
    u = lambda a, b: g.uniform(a, b, (NMAX, KMAX)).astype(np.float32)  # noqa: E731
    z = np.zeros((NMAX, KMAX), np.float32)
    table = {0: lambda: ([u(-2, 2), u(0.3, 2), z, z], u(-3, 3)),
             1: lambda: ([u(-2, -1), u(1, 3), z, z], u(-0.9, 0.9)),
             3: lambda: ([u(0.5, 6), z, z, z], np.floor(u(0, 9))),
             4: lambda: ([u(0.1, 0.9), z, z, z], np.floor(u(0, 2)).clip(0, 1)),
             6: lambda: ([u(0.5, 3), z, z, z], u(0.05, 3)),
             7: lambda: ([u(0.5, 4), u(0.5, 3), z, z], u(0.05, 4)),
             8: lambda: ([u(0.5, 4), u(0.5, 4), u(-2, -1), u(1, 2)], u(-0.9, 0.9)),
             9: lambda: ([u(-1, 1), u(0.3, 1.5), z, z], u(0.1, 4)),
             10: lambda: ([u(0.5, 2), u(0.5, 3), z, z], u(0.1, 3)),
             11: lambda: ([np.floor(u(10, 21)), u(-2, 2), z, z], np.floor(u(0, 11)).clip(0, 10)),
             12: lambda: ([u(-3, 3), u(0.2, 8), z, z], u(-3.1, 3.1)),
             13: lambda: ([u(-1, 1), u(0.5, 2), u(-3, -2), u(2, 3)], u(-1.9, 1.9))}
    return table[kind]()


_pools = {}


def dev_pool(kind):
    """The pool on the device, made once per family and left unchanged."""
    if kind not in _pools:
        p, x = pool(kind)
        _pools[kind] = ([torch.from_numpy(q).cuda() for q in p], torch.from_numpy(x).cuda())
    return _pools[kind]


def fill(o, t, rs, es, row0=0):
    o.p, o.row_stride, o.elem_stride = t.data_ptr() + 4 * row0 * rs, rs, es


def make_term(kind, k, M, N, scale, form='full', x_shared=False, row0=0):
    """One term over the pool's corner: ps = [(tensor, row stride, element stride)] in the parameter form `full` ([N, k]),
    `particle` ([N, 1]: one value per particle) or `shared` ([k]: one row for all particles); x [M, k] from the pool's rows
    row0 .. row0 + M (x_shared: ONE row for all groups, row stride 0); x_old: the row the original call observed."""
    P, X = dev_pool(kind)
    if form == 'full':
        ps = [(q[:N, :k].contiguous(), k, 1) for q in P]
    elif form == 'particle':
        ps = [(q[:N, :1].contiguous(), 1, 0) for q in P]
    else:
        ps = [(q[5, :k].contiguous(), 0, 1) for q in P]
    x = X[row0:row0 + (1 if x_shared else M), :k].contiguous()
    return dict(kind=kind, k=k, scale=scale, ps=ps, x=(x, 0 if x_shared else k, 1), x_old=X[NMAX - 1, :k].contiguous())


def reobs(lib, terms, lw, old, out, M, N, check=True):
    """pp_is_reobserve_groups on torch's current stream."""
    from pyprob_amd import lib as L
    arr = (L.pp_reobs_term * max(len(terms), 1))()
    for t, T in enumerate(terms):
        arr[t].kind, arr[t].k, arr[t].scale = T['kind'], T['k'], T['scale']
        for q in range(OR.N_PARAMS.get(T['kind'], 2)):
            if T['ps'][q] is not None:
                fill(arr[t].params[q], *T['ps'][q])
        if T['x'] is not None:
            fill(arr[t].x, *T['x'])
    rc = lib.pp_is_reobserve_groups(arr, len(terms), L.ptr(lw), L.ptr(old), L.ptr(out), M, N, L.stream_ptr())
    if check:
        L.check(rc, 'pp_is_reobserve_groups')
    return rc


def obs_lp(lib, T, x_row, N):
    """lp_out [N] of pp_obs_logweight for the term's parameters and ONE shared row of values."""
    from pyprob_amd import lib as L
    arr = (L.pp_obs_operand * 4)()
    for q in range(OR.N_PARAMS[T['kind']]):
        fill(arr[q], *T['ps'][q])
    xo = L.pp_obs_operand()
    fill(xo, x_row, 0, 1)
    lp = torch.full((N,), SENTINEL, device='cuda')
    L.check(lib.pp_obs_logweight(T['kind'], arr, xo, T['k'], 1.0, None, L.ptr(lp), None, N, N, L.stream_ptr()), 'pp_obs_logweight')
    return lp


def old_chain(lib, terms, N, scales=None):
    """`old` as the accumulate route makes it: a zeroed vector, lw += scale * lp per term in order (pp_obs_logweight)."""
    from pyprob_amd import lib as L
    old = torch.zeros(N, device='cuda')
    for t, T in enumerate(terms):
        arr = (L.pp_obs_operand * 4)()
        for q in range(OR.N_PARAMS[T['kind']]):
            fill(arr[q], *T['ps'][q])
        xo = L.pp_obs_operand()
        fill(xo, T['x_old'], 0, 1)
        L.check(lib.pp_obs_logweight(T['kind'], arr, xo, T['k'], T['scale'] if scales is None else scales[t], L.ptr(old), None,
                                     None, N, N, L.stream_ptr()), 'pp_obs_logweight')
    return old


def start_lw(N):
    return torch.linspace(-3.0, 5.0, N, device='cuda')


def expected(lib, terms, lw, old, M, N):
    """The float32 composition of pp_obs_logweight's lp_out, one call per group and term."""
    lps = []
    for T in terms:
        x, rs, _ = T['x']
        rows = [obs_lp(lib, T, x[g if rs else 0], N) for g in range(M)]
        lps.append(torch.stack(rows).cpu().numpy())
    return RR.compose32(lw.cpu().numpy(), None if old is None else old.cpu().numpy(), lps, [T['scale'] for T in terms])


def run(lib, terms, M, N, lw=None, with_old=True):
    lw = start_lw(N) if lw is None else lw
    old = old_chain(lib, terms, N) if with_old else None
    out = torch.full((M * N,), SENTINEL, device='cuda')
    reobs(lib, terms, lw, old, out, M, N)
    return out.cpu().numpy().reshape(M, N), lw, old


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_bits_of_the_composition_at_every_width(lib, k):
    for M, N in MN:
        terms = [make_term(0, k, M, N, 0.37)]
        got, lw, old = run(lib, terms, M, N)
        want = expected(lib, terms, lw, old, M, N)
        assert np.all(np.isfinite(want)) and not np.any(got == SENTINEL), (k, M, N)
        assert np.array_equal(got, want), (k, M, N, np.argwhere(got != want)[:5])


@pytest.mark.parametrize('kind', OR.KINDS)
def test_bits_of_every_family(lib, kind):
    for k in (1, 5, 257):
        for M, N in ((5, 3), (2, 67)):
            terms = [make_term(kind, k, M, N, 0.81)]
            got, lw, old = run(lib, terms, M, N)
            want = expected(lib, terms, lw, old, M, N)
            assert np.all(np.isfinite(want)), (kind, k, M, N)
            assert np.array_equal(got, want), (kind, k, M, N, np.argwhere(got != want)[:5])


@pytest.mark.parametrize('form', ('full', 'particle', 'shared'))
@pytest.mark.parametrize('count', (1, 2, 8))
def test_bits_of_several_terms_and_parameter_forms(lib, count, form):
    """1, 2 and 8 terms - of one family, and of different families and widths (the kernel that switches per term) -, with [N, k],
    per-particle and shared parameters; a term whose value is the same for every group (row stride 0); no `old` (NULL)."""
    mixed = [(0, 5), (7, 1), (13, 129), (3, 4), (1, 3), (9, 257), (12, 1), (4, 5)]
    for M, N in ((5, 3), (3, 300), (70, 5)):
        for plan in ([(0, 5)] * count, mixed[:count]):
            terms = [make_term(kind, k, M, N, 0.25 + 0.125 * t, form=form, x_shared=(t == 1), row0=t)
                     for t, (kind, k) in enumerate(plan)]
            got, lw, old = run(lib, terms, M, N)
            want = expected(lib, terms, lw, old, M, N)
            assert np.all(np.isfinite(want)), (count, form, M, N)
            assert np.array_equal(got, want), (count, form, M, N, plan, np.argwhere(got != want)[:5])
    terms = [make_term(0, 5, 5, 3, 0.5, form=form)]
    got, lw, _ = run(lib, terms, 5, 3, with_old=False)
    assert np.array_equal(got, expected(lib, terms, lw, None, 5, 3))


@pytest.mark.parametrize('kind', OR.KINDS)
def test_k1_instance_has_the_bits_of_the_general_kernel(lib, kind, monkeypatch):
    """Terms of one family with k = 1 take the kernel that keeps the particles' parameters in registers and evaluates one
    log-density per term; PP_REOBS_PLAIN=1 sends the same call through the general kernel. 1, 2 and 8 terms, per-particle and
    shared parameters, a particle tile (256) and a group chunk that are crossed - and the composition of pp_obs_logweight."""
    for count, form, (M, N) in ((1, 'full', (5, 3)), (2, 'particle', (3, 300)), (8, 'full', (70, 5)), (8, 'shared', (2, 67))):
        terms = [make_term(kind, 1, M, N, 0.25 + 0.125 * t, form=form, x_shared=(t == 1), row0=t) for t in range(count)]
        monkeypatch.delenv('PP_REOBS_PLAIN', raising=False)
        got, lw, old = run(lib, terms, M, N)
        monkeypatch.setenv('PP_REOBS_PLAIN', '1')
        plain, _, _ = run(lib, terms, M, N)
        monkeypatch.delenv('PP_REOBS_PLAIN')
        want = expected(lib, terms, lw, old, M, N)
        assert np.all(np.isfinite(want)) and not np.any(got == SENTINEL), (kind, count, form)
        assert np.array_equal(got, plain), (kind, count, form, np.argwhere(got != plain)[:5])
        assert np.array_equal(got, want), (kind, count, form, np.argwhere(got != want)[:5])


# ---- 2. the identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 5, 1030))
def test_the_original_values_at_the_original_scale_return_lw(lib, k):
    M, N = 3, 67
    plan = [(0, k), (7, 1), (13, k)]
    terms = [make_term(kind, kk, M, N, 0.5 + 0.25 * t) for t, (kind, kk) in enumerate(plan)]
    for T in terms:      # every group observes the original row again
        T['x'] = (T['x_old'].reshape(1, -1), 0, 1)
    got, lw, _ = run(lib, terms, M, N)
    for g in range(M):
        assert np.array_equal(got[g], lw.cpu().numpy()), (k, g)


# ---- 3. float64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', OR.KINDS)
def test_against_float64(lib, kind):
    for k, (M, N) in ((1, (5, 3)), (129, (3, 64)), (1030, (2, 67))):
        terms = [make_term(kind, k, M, N, 0.6), make_term(0, 3, M, N, 1.0, form='particle')]
        got, lw, old = run(lib, terms, M, N)
        ref_old = np.zeros(N)
        for T in terms:
            ref_old += float(np.float32(T['scale'])) * RR.term_lp64(T['kind'], [p[0] for p in T['ps']], T['x_old'], 1, N, T['k'])[0][0]
        ref = RR.reobserve64(lw.cpu().numpy(), ref_old, [(T['kind'], T['k'], T['scale'], [p[0] for p in T['ps']], T['x'][0])
                                                          for T in terms], M)
        np.testing.assert_allclose(got, ref, err_msg=str((kind, k, M, N)), **bar(ref))


# ---- 4. edge values -------------------------------------------------------------------------------------------------------------
def test_a_particle_the_call_dropped_stays_dropped_for_every_group(lib):
    M, N = 5, 67
    lw = start_lw(N)
    lw[3], lw[40], lw[66] = float('-inf'), float('nan'), float('inf')
    terms = [make_term(0, 5, M, N, 0.7)]
    got, _, old = run(lib, terms, M, N, lw=lw)
    want = expected(lib, terms, lw, old, M, N)
    assert np.all(np.isneginf(got[:, 3])) and np.all(np.isnan(got[:, 40])) and np.all(np.isposinf(got[:, 66]))
    keep = np.isfinite(lw.cpu().numpy())
    assert np.array_equal(got[:, keep], want[:, keep]) and np.all(np.isfinite(got[:, keep]))


def test_a_value_outside_the_support_is_minus_infinity_for_that_pair_only(lib):
    M, N, k = 5, 67, 5
    P, X = dev_pool(1)      # Uniform(low in [-2, -1], high in [1, 3]); particle 9 gets high = 0.5, group 2 holds a 0.75
    high = P[1][:N, :k].contiguous()
    high[9, :] = 0.5
    x = (X[:M, :k] * 0.4).contiguous()
    x[2, 3] = 0.75
    T = dict(kind=1, k=k, scale=1.0, ps=[(P[0][:N, :k].contiguous(), k, 1), (high, k, 1), None, None], x=(x, k, 1),
             x_old=(X[NMAX - 1, :k] * 0.4).contiguous())
    got, _, _ = run(lib, [T], M, N)
    bad = np.zeros((M, N), bool)
    bad[2, 9] = True
    assert np.all(np.isneginf(got[bad])) and np.all(np.isfinite(got[~bad]))


def test_nan_parameters_give_nan(lib):
    M, N, k = 3, 64, 4
    T = make_term(0, k, M, N, 1.0)
    T['ps'][1][0][17, 2] = float('nan')
    got, _, _ = run(lib, [T], M, N)
    assert np.all(np.isnan(got[:, 17])) and np.all(np.isfinite(np.delete(got, 17, axis=1)))


def test_memory_around_out_is_untouched_and_two_runs_agree(lib):
    M, N, pad = 3, 300, 64
    terms = [make_term(0, 129, M, N, 0.4), make_term(7, 1, M, N, 0.9)]
    lw, old = start_lw(N), old_chain(lib, terms, N)
    bufs = []
    for _ in range(2):
        buf = torch.full((M * N + 2 * pad,), SENTINEL, device='cuda')
        reobs(lib, terms, lw, old, buf[pad:pad + M * N], M, N)
        bufs.append(buf.cpu().numpy())
    assert np.all(bufs[0][:pad] == SENTINEL) and np.all(bufs[0][pad + M * N:] == SENTINEL)
    assert not np.any(bufs[0][pad:pad + M * N] == SENTINEL)
    assert np.array_equal(bufs[0], bufs[1])


def test_a_group_row_is_the_same_alone_and_inside_five(lib):
    N = 300
    for k in (1, 5, 257):
        terms = [make_term(0, k, 5, N, 0.37)]
        five, lw, old = run(lib, terms, 5, N)
        for g in (0, 3):
            x = terms[0]['x'][0]
            alone = dict(terms[0], x=(x[g:g + 1].contiguous(), k, 1))
            out = torch.full((N,), SENTINEL, device='cuda')
            reobs(lib, [alone], lw, old, out, 1, N)
            assert np.array_equal(out.cpu().numpy(), five[g]), (k, g)


def test_no_group_is_no_launch(lib):
    T = make_term(0, 5, 1, 7, 1.0)
    out = torch.full((7,), SENTINEL, device='cuda')
    assert reobs(lib, [T], start_lw(7), None, out, 0, 7, check=False) == 0
    assert np.all(out.cpu().numpy() == SENTINEL)


def test_refusals(lib):
    M, N = 2, 7
    lw, out = start_lw(N), torch.full((M * N,), SENTINEL, device='cuda')
    good = lambda **kw: dict(make_term(0, 5, M, N, 1.0), **kw)  # noqa: E731
    neg = lambda T, which: (T[0], -1 if which == 'rs' else T[1], -1 if which == 'es' else T[2])  # noqa: E731
    g = good()
    cases = [([good(kind=2)], lw, out, M, N), ([good(kind=5)], lw, out, M, N), ([good(kind=14)], lw, out, M, N),
             ([good(kind=-1)], lw, out, M, N), ([], lw, out, M, N), ([good()] * 9, lw, out, M, N),
             ([good(k=0)], lw, out, M, N), ([good()], lw, out, M, 0), ([good()], lw, out, -1, N),
             ([good(ps=[g['ps'][0], None, None, None])], lw, out, M, N),
             ([good(ps=[neg(g['ps'][0], 'rs'), g['ps'][1], None, None])], lw, out, M, N),
             ([good(ps=[g['ps'][0], neg(g['ps'][1], 'es'), None, None])], lw, out, M, N),
             ([good(x=None)], lw, out, M, N), ([good(x=neg(g['x'], 'rs'))], lw, out, M, N),
             ([good(x=neg(g['x'], 'es'))], lw, out, M, N),
             ([good()], None, out, M, N), ([good()], lw, None, M, N)]
    for i, (terms, a, b, m, n) in enumerate(cases):
        assert reobs(lib, terms, a, None, b, m, n, check=False) != 0, i
        assert b'pp_is_reobserve_groups' in lib.pp_last_error(), i
    assert np.all(out.cpu().numpy() == SENTINEL)
