"""Weighted histograms and quantiles of latents on the device (csrc/is_hist.hip pp_is_hist_groups / pp_is_extent_groups; the
is_hist_groups / is_extent_groups operators; Empirical.histogram / histogram2d / min / max; pyprob_amd.histogram_batch):
 1. the kernel's rows against the float64 restatement (tests/histogram_ref.py): counts exactly, every fixed-point slot within the
    DERIVED bound |slot - sum w 2^S| <= 0.5 count + 2^-48 sum w 2^S - one particle, a part of a wave, several groups, a tile + 1,
    2048 bins, more than 65535 groups; shared, per-group and non-uniform edges; 1-D and 2-D. Particles with lw = -inf / +inf / NaN
    carry NaN values and appear in no slot; particles with a finite weight carry x = NaN, -inf, +inf and values exactly on the
    first, an inner and the last edge; one group has no finite weight (its row is zero); poison around the output survives;
 2. the slot total of a row is the same integer for every bin count and for 1-D and 2-D of the same particles;
 3. bit identity: two calls, with and without `stats`, group g of an M-group call against the one-group call on its slice;
 4. pp_is_extent_groups against numpy exactly, with the same identities;
 5. end to end on the three-statement straight-line program: histogram and marginal().histogram against numpy.histogram of the
    read-back columns (counts equal, masses within n 2^-(S+1) / W + 1e-12), the median within a bin width, min / max without host
    weights; 6. histogram_batch is one extent and one histogram operator call and equals the loop bit for bit.
All of them FAIL WITHOUT THE FEATURE: the parent has neither the symbols nor the methods.
If pyprob_amd/libpyprob_amd.so is missing or stale here nothing below can run: L.load() raises instead of skipping."""
import warnings

import numpy as np
import pytest

import histogram_ref as H
from pyprob_amd import lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SHAPES = [(1, 1, 1), (1, 63, 7), (3, 257, 64), (7, 300, 50), (2, 2049, 2048), (1, 4097, 33), (66000, 2, 4)]
SHAPES_2D = [(1, 300, 5, 3), (2, 2049, 32, 64)]
PAD = 2            # poisoned rows in front of and behind the live rows of the output
POISON = -0x0123456789ABCDEF
DEV = 'cuda:0'
_INPUTS, _CASES = {}, {}


def _inputs(M, N):
    """lw ~ normal(0, 3), x ~ normal(0, 1.5), y ~ normal(0.5, 1) - a function of (M, N) alone, so that every binning sees the same
    particles. Where the group is long enough: particles with lw = -inf, +inf, NaN whose x and y are NaN; particles with a finite
    weight and x = NaN, -inf, +inf; x exactly -4, 0 and 4 (the first, the middle and the last of the edges below). The last group of
    M >= 2 (M small) has no finite weight at all."""
    if (M, N) not in _INPUTS:
        rng = np.random.default_rng(1000 * N + M)
        lw = rng.normal(0.0, 3.0, (M, N)).astype(np.float32)
        x = rng.normal(0.0, 1.5, (M, N)).astype(np.float32)
        y = rng.normal(0.5, 1.0, (M, N)).astype(np.float32)
        if N >= 63:
            for g in range(M):
                at = rng.choice(N, 12, replace=False)
                lw[g, at[:6]] = np.array([-np.inf, np.inf, np.nan, -np.inf, np.inf, np.nan], np.float32)
                x[g, at[:6]] = y[g, at[:6]] = np.nan
                x[g, at[6:]] = np.array([np.nan, -np.inf, np.inf, -4.0, 0.0, 4.0], np.float32)
        if 2 <= M <= 100:
            lw[M - 1] = rng.choice(np.array([-np.inf, np.nan, np.inf], np.float32), N)
            x[M - 1, ::2] = np.nan
        _INPUTS[(M, N)] = (lw, x, y)
    return _INPUTS[(M, N)]


def _edges(kind, M, bins, lo=-4.0, hi=4.0):
    if kind == 'shared':
        return np.linspace(lo, hi, bins + 1)
    if kind == 'per_group':          # every group its own range, the first the shared one
        return np.stack([np.linspace(lo - 0.125 * g, hi + 0.25 * g, bins + 1) for g in range(M)])
    t = np.linspace(-1.0, 1.0, bins + 1)         # non-uniform: narrow bins around the middle, the same end points
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * np.sign(t) * t * t


def _call(lw, x, y, ex, ey, stats=None):
    """One pp_is_hist_groups call on host arrays; the output buffer carries PAD poisoned rows in front of and behind the live rows.
    Returns the host copy of the whole output [PAD + M + PAD, 2, slots]."""
    lib = L.load()
    M, N = lw.shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    tl, tx, ty, tex, tey = dev(lw.reshape(-1)), dev(x.reshape(-1)), dev(None if y is None else y.reshape(-1)), dev(ex), dev(ey)
    bx, by = ex.shape[-1] - 1, 1 if ey is None else ey.shape[-1] - 1
    slots = bx + 3 if y is None else bx * by + 2
    out = torch.full((PAD + M + PAD, 2, slots), POISON, dtype=torch.int64, device=DEV)
    need = lib.pp_is_hist_workspace_bytes(M, N, bx, by)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_hist_groups(tl.data_ptr(), tx.data_ptr(), L.ptr(ty), M, N, tex.data_ptr(), bx, 0 if ex.ndim == 1 else bx + 1,
                                  L.ptr(tey), by, 0 if (ey is None or ey.ndim == 1) else by + 1, L.ptr(stats), out[PAD:].data_ptr(),
                                  ws.data_ptr(), need, L.stream_ptr()), 'pp_is_hist_groups')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _call_extent(lw, x):
    lib = L.load()
    M, N = lw.shape
    tl, tx = torch.from_numpy(lw.reshape(-1)).to(DEV), torch.from_numpy(x.reshape(-1)).to(DEV)
    out = torch.full((PAD + M + PAD, 4), float('nan'), dtype=torch.float64, device=DEV)
    need = lib.pp_is_extent_workspace_bytes(M, N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_extent_groups(tl.data_ptr(), tx.data_ptr(), M, N, out[PAD:].data_ptr(), ws.data_ptr(), need, L.stream_ptr()),
            'pp_is_extent_groups')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _stats(lw, x):
    """pp_is_stats per group: device double [M, 6]."""
    from pyprob_amd import ops as P
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    rows = [P.ops.is_stats(torch.from_numpy(lw[g]).to(DEV), torch.from_numpy(x[g]).to(DEV), scratch)[:6] for g in range(lw.shape[0])]
    return torch.stack(rows).contiguous()


def _case(M, N, bx, by=None, kind='shared'):
    """The device rows and the float64 reference of a shape and an edge kind, computed once and shared by the tests (never
    modified). by None: 1-D."""
    key = (M, N, bx, by, kind)
    if key not in _CASES:
        lw, x, y = _inputs(M, N)
        ex = _edges(kind, M, bx)
        ey = None if by is None else _edges(kind, M, by, -2.0, 3.0)
        yy = None if by is None else y
        ref, real = H.hist_ref(lw, x, yy, ex, ey)
        _CASES[key] = (lw, x, yy, ex, ey, _call(lw, x, yy, ex, ey), ref, real)
    return _CASES[key]


def _check_rows(whole, ref, real, lw, label):
    M = ref.shape[0]
    assert whole.shape == (PAD + M + PAD,) + ref.shape[1:], label
    assert (whole[:PAD] == POISON).all() and (whole[PAD + M:] == POISON).all(), label          # the poison survives
    got = whole[PAD:PAD + M]
    assert np.array_equal(got[:, 1], ref[:, 1]), (label, 'counts')
    assert np.array_equal(got[:, 1].sum(1), np.isfinite(lw).sum(1)), label          # a particle without a finite weight is in no slot
    assert (got[:, 0] >= 0).all() and (got[:, 0].sum(1) <= 2 ** 62).all(), label
    err = np.abs(got[:, 0].astype(np.longdouble) - real)
    bound = np.longdouble(0.5) * got[:, 1] + np.longdouble(2.0 ** -48) * real
    print('%s: max |slot - sum w 2^S| / bound = %.3g; slots that differ from the numpy emulation: %d' % (
        label, float((err / np.maximum(bound, np.longdouble(1e-300))).max()), int((got[:, 0] != ref[:, 0]).sum())))
    assert (err <= bound).all(), (label, np.argwhere(~(err <= bound))[:5].tolist())
    assert (got[:, 0][got[:, 1] == 0] == 0).all(), label


# ---- 1. the kernel against float64 numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,bins', SHAPES)
def test_rows_against_the_float64_restatement(M, N, bins):
    lw, x, _, ex, _, whole, ref, real = _case(M, N, bins)
    _check_rows(whole, ref, real, lw, str((M, N, bins)))
    got = whole[PAD:PAD + M]
    if 2 <= M <= 100:            # the group without a finite weight: its row is all zero
        assert (got[M - 1] == 0).all()
    if N >= 63:
        for g in range(M - 1 if 2 <= M <= 100 else M):
            fin = np.isfinite(lw[g])
            xs = x[g].astype(np.float64)
            # NaN, -inf, +inf under a finite weight have their slots; the values on the first and the last edge are INSIDE
            assert got[g, 1, bins + 2] == (fin & np.isnan(xs)).sum() >= 1
            assert got[g, 1, bins] == (fin & (xs < ex[0])).sum() >= 1 and got[g, 1, bins + 1] == (fin & (xs > ex[-1])).sum() >= 1
            assert got[g, 1, 0] >= (fin & (xs == ex[0])).sum() >= 1 and got[g, 1, bins - 1] >= (fin & (xs == ex[-1])).sum() >= 1
            if bins in (4, 64, 2048):      # (a step that is a power of two) 0.0 is the inner edge bins / 2: it opens the bin to its right
                assert ex[bins // 2] == 0.0
                assert got[g, 1, bins // 2] == (fin & (xs >= 0.0) & (xs < ex[bins // 2 + 1])).sum() >= 1


@pytest.mark.parametrize('M,N,bins', [s for s in SHAPES if s[0] <= 100])
@pytest.mark.parametrize('kind', ['per_group', 'nonuniform'])
def test_per_group_and_non_uniform_edges(M, N, bins, kind):
    lw, _, _, ex, _, whole, ref, real = _case(M, N, bins, kind=kind)
    assert ex.ndim == (2 if kind == 'per_group' else 1)
    _check_rows(whole, ref, real, lw, str((M, N, bins, kind)))


@pytest.mark.parametrize('M,N,bx,by', SHAPES_2D)
@pytest.mark.parametrize('kind', ['shared', 'per_group', 'nonuniform'])
def test_two_dimensional_rows(M, N, bx, by, kind):
    lw, x, y, ex, ey, whole, ref, real = _case(M, N, bx, by, kind)
    assert ref.shape == (M, 2, bx * by + 2)
    _check_rows(whole, ref, real, lw, str((M, N, bx, by, kind)))
    got = whole[PAD:PAD + M]
    for g in range(M - 1 if M >= 2 else M):
        fin = np.isfinite(lw[g])
        assert got[g, 1, bx * by + 1] == (fin & (np.isnan(x[g]) | np.isnan(y[g]))).sum() >= 1 and got[g, 1, bx * by] >= 2
    if M >= 2:
        assert (got[M - 1] == 0).all()


# ---- 2. one total per group, whatever the binning --------------------------------------------------------------------------------------
def test_the_slot_total_does_not_depend_on_the_binning():
    M, N = 2, 2049
    lw, x, y = _inputs(M, N)
    totals = [_case(M, N, 2048)[5][PAD:PAD + M, 0].sum(1), _case(M, N, 32, 64)[5][PAD:PAD + M, 0].sum(1),
              _case(M, N, 2048, kind='nonuniform')[5][PAD:PAD + M, 0].sum(1)]
    for bins in (1, 7, 50):
        totals.append(_call(lw, x, None, _edges('shared', M, bins), None)[PAD:PAD + M, 0].sum(1))
    totals.append(_call(lw, x, y, _edges('shared', M, 5), _edges('per_group', M, 3, -2.0, 3.0))[PAD:PAD + M, 0].sum(1))
    for t in totals[1:]:
        assert np.array_equal(t, totals[0]), (t, totals[0])
    ref_total = H.hist_ref(lw, x, None, _edges('shared', M, 1), None)[1].sum(1)
    assert totals[0][1] == 0 and abs(np.longdouble(totals[0][0]) - ref_total[0]) <= 0.5 * N + 2.0 ** -48 * ref_total[0]
    assert 2 ** H.shift(N) <= totals[0][0] <= 2 ** 62          # (the heaviest particle alone is 2^S)


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,bx,by', [(3, 257, 64, None), (7, 300, 50, None), (2, 2049, 2048, None), (2, 2049, 32, 64),
                                       (2, 20000, 100, None), (2, 20000, 300, None), (1, 4097, 256, None), (1, 4097, 257, None),
                                       (2, 9000, 17, 16)])
def test_bit_identity_of_calls_groups_and_statistics(M, N, bx, by):
    """Also the shapes at which the launch sequence changes: the tile is 2048 particles up to 256 bins and 8192 above, so (2, 20000)
    is ten tiles per group at 100 bins and three at 300, (1, 4097) three tiles at 256 bins and one at 257, (2, 9000, 17 x 16) two of
    8192 - the maximum comes from the tile-maximum launch or from `stats`, the rows from the sum of the partial rows."""
    lw, x, y, ex, ey, whole, ref, real = _case(M, N, bx, by, 'per_group')
    _check_rows(whole, ref, real, lw, str((M, N, bx, by, 'per_group')))
    got = whole[PAD:PAD + M]
    assert np.array_equal(_call(lw, x, y, ex, ey)[PAD:PAD + M], got)                              # two calls
    stats = _stats(lw, x)
    assert np.array_equal(_call(lw, x, y, ex, ey, stats)[PAD:PAD + M], got)                       # the maxima of pp_is_stats
    for g in range(M):
        one = _call(lw[g:g + 1], x[g:g + 1], None if y is None else y[g:g + 1], ex[g], None if ey is None else ey[g])
        assert np.array_equal(one[PAD], got[g]), g
        one = _call(lw[g:g + 1], x[g:g + 1], None if y is None else y[g:g + 1], ex[g], None if ey is None else ey[g],
                    stats[g:g + 1].contiguous())
        assert np.array_equal(one[PAD], got[g]), g


# ---- 4. the extent -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', sorted(set((s[0], s[1]) for s in SHAPES)) + [(2, 20000)])
def test_extent_against_numpy(M, N):
    lw, x, _ = _inputs(M, N)
    whole = _call_extent(lw, x)
    assert np.isnan(whole[:PAD]).all() and np.isnan(whole[PAD + M:]).all()
    got = whole[PAD:PAD + M]
    ref = H.extent_ref(lw, x)
    assert np.array_equal(got, ref)
    if N >= 63:
        assert got[0, 0] == -np.inf and got[0, 1] == np.inf and got[0, 3] == 1          # (the infinite values count, the NaN does not)
    if 2 <= M <= 100:
        assert got[M - 1].tolist() == [np.inf, -np.inf, 0.0, 0.0]
    assert np.array_equal(_call_extent(lw, x)[PAD:PAD + M], got)
    for g in range(min(M, 3)):
        assert np.array_equal(_call_extent(lw[g:g + 1], x[g:g + 1])[PAD], got[g])
    if M == 1 and N >= 63:      # without the infinite values: the exact fp32 extremes of what is left, widened to double
        x2 = np.where(np.isinf(x), np.float32(0.25), x)
        got2 = _call_extent(lw, x2)[PAD]
        ok = np.isfinite(lw[0]) & ~np.isnan(x2[0])
        assert got2[0] == float(x2[0][ok].min()) and got2[1] == float(x2[0][ok].max()) and np.isfinite(got2[:2]).all()


def test_operators_shapes_and_types():
    from pyprob_amd import ops as P
    M, N = 3, 257
    lw, x, y = _inputs(M, N)
    tl, tx, ty = (torch.from_numpy(a.reshape(-1)).to(DEV) for a in (lw, x, y))
    e1 = torch.from_numpy(_edges('shared', M, 64)).to(DEV)
    eg = torch.from_numpy(_edges('per_group', M, 64)).to(DEV)
    out = P.ops.is_hist_groups(tl, tx, None, N, e1, None, None)
    assert out.dtype == torch.int64 and out.shape == (M, 2, 67) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), _case(M, N, 64)[5][PAD:PAD + M])
    assert np.array_equal(P.ops.is_hist_groups(tl, tx, None, N, eg, None, None).cpu().numpy(), _case(M, N, 64, kind='per_group')[5][PAD:PAD + M])
    e2 = torch.from_numpy(_edges('shared', M, 4, -2.0, 3.0)).to(DEV)
    assert P.ops.is_hist_groups(tl, tx, ty, N, e1[:9].contiguous(), e2, None).shape == (M, 2, 8 * 4 + 2)
    ext = P.ops.is_extent_groups(tl, tx, N)
    assert ext.dtype == torch.float64 and ext.shape == (M, 4) and np.array_equal(ext.cpu().numpy(), H.extent_ref(lw, x))
    for bad in (lambda: P.ops.is_hist_groups(tl, tx, ty, N, e1, None, None), lambda: P.ops.is_hist_groups(tl, tx, None, N, e1.float(), None, None),
                lambda: P.ops.is_hist_groups(tl, tx[:-1], None, N, e1, None, None), lambda: P.ops.is_hist_groups(tl, tx, None, N, eg[:2], None, None),
                lambda: P.ops.is_hist_groups(tl, tx, ty, N, e1, e1, None), lambda: P.ops.is_extent_groups(tl, tx, N + 1)):
        with pytest.raises(RuntimeError):
            bad()


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------
def _weights(lw):
    w = np.exp(lw.astype(np.float64) - lw.astype(np.float64).max())
    return w, w.sum()


def _against_numpy(h, v, lw, bins, rg=None):
    """Counts equal numpy.histogram's; masses within n 2^-(S+1) / W + 1e-12, W = the float64 sum of exp(lw - max lw)."""
    n = len(v)
    w, W = _weights(lw)
    v = v.astype(np.float64)
    c, e = np.histogram(v, bins, range=rg)
    m, _ = np.histogram(v, bins, range=rg, weights=w / W)
    assert np.array_equal(h.edges, e) and np.array_equal(h.count, c) and h.particles == n and h.nan == 0
    tol = n * 2.0 ** -(H.shift(n) + 1) / W + 1e-12
    print('masses: max error %.3g (tolerance %.3g)' % (float(np.abs(h.mass - m).max()), tol))
    assert np.abs(h.mass - m).max() <= tol
    assert abs(h.mass.sum() + h.below + h.above + h.nan - 1.0) <= 1e-12
    # the median to the resolution of the histogram: one bin width around the exact weighted median (sorted on the host)
    if h.below < 0.5 < 1.0 - h.above:
        order = np.argsort(v, kind='stable')
        exact = v[order][np.searchsorted(np.cumsum(w[order]) / W, 0.5)]
        assert abs(h.quantile(0.5) - exact) <= np.diff(h.edges).max(), (h.quantile(0.5), exact)


@pytest.mark.parametrize('N', [300, 4097])
def test_straight_line_program_end_to_end(N):
    from test_gpu_joint_moments import _log_columns, _posterior, _straight_line_model
    _straight_line_model()
    post = _posterior(N)
    assert post._device_backed() and post.length == N
    lw = post._log_weights.cpu().numpy()
    c = post._values.cpu().numpy()
    h = post.histogram()
    assert len(h.mass) == 50 and h.below == 0 and h.above == 0
    _against_numpy(h, c, lw, 50)
    _against_numpy(post.histogram(2048), c, lw, 2048)
    _against_numpy(post.histogram(20, range=(0.0, 2.5)), c, lw, 20, (0.0, 2.5))
    log = _log_columns(post)
    a = log[0][1].cpu().numpy()
    ha = post.marginal('mu').histogram(64)
    _against_numpy(ha, a, post._all_log_weights.cpu().numpy(), 64)
    edges = np.array([-10.0, -1.0, 0.0, 0.5, 1.0, 1.25, 1.5, 2.0, 3.0, 10.0])
    he = post.marginal('a').histogram(edges=edges)
    w, W = _weights(post._all_log_weights.cpu().numpy())
    assert np.array_equal(he.count, np.histogram(a.astype(np.float64), edges)[0])
    assert np.abs(he.mass - np.histogram(a.astype(np.float64), edges, weights=w / W)[0]).max() <= N * 2.0 ** -(H.shift(N) + 1) / W + 1e-12
    lo, hi = ha.credible_interval(0.9)
    assert ha.edges[0] <= lo < ha.quantile(0.5) < hi <= ha.edges[-1] and ha.edges[0] < ha.mode < ha.edges[-1]
    # a 2-D histogram of two latents: its margins are the 1-D histograms' counts
    h2 = post.histogram2d('mu', 'c', bins=(16, 8))
    c2 = np.histogram2d(a.astype(np.float64), c.astype(np.float64), (16, 8))[0]
    assert np.array_equal(h2.count, c2.astype(np.int64)) and h2.outside == 0 and h2.particles == N
    assert abs(h2.mass.sum() - 1.0) <= 1e-12
    # min / max from the extent kernel: numpy's floats, no host weights materialised
    fresh = post.marginal('b')
    b = log[1][1].cpu().numpy()
    assert fresh.min == float(b.min()) and fresh.max == float(b.max()) and not fresh._host_weights_ready()
    assert post.min == float(c.min()) and post.max == float(c.max())


# ---- 6. the batched form -------------------------------------------------------------------------------------------------------------------
def _same_histogram(f, l):
    for name in ('edges', 'mass', 'density', 'count'):
        assert np.array_equal(getattr(f, name), getattr(l, name)), name
    assert (f.below, f.above, f.nan, f.particles) == (l.below, l.above, l.nan, l.particles)


def test_histogram_batch_is_one_launch_pair_and_equals_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from test_gpu_joint_moments import _straight_line_model
    model, full = _straight_line_model()
    M, N = 7, 300
    rng = np.random.default_rng(3)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(N, observes, seed=13, offset=64)
    assert model._batch_ok is True and len(posts) == M
    count = {'hist': 0, 'extent': 0}
    hist_op, extent_op = P.ops.is_hist_groups, P.ops.is_extent_groups

    def hist_counted(*a):
        count['hist'] += 1
        return hist_op(*a)

    def extent_counted(*a):
        count['extent'] += 1
        return extent_op(*a)
    monkeypatch.setattr(P.ops, 'is_hist_groups', hist_counted, raising=False)
    monkeypatch.setattr(P.ops, 'is_extent_groups', extent_counted, raising=False)
    loop = [p.histogram(40) for p in posts]
    assert count == {'hist': M, 'extent': M}
    fast = pyprob_amd.histogram_batch(posts, 40)
    assert count == {'hist': M + 1, 'extent': M + 1} and len(fast) == M          # ONE operator call each for the M groups
    for f, l, p in zip(fast, loop, posts):
        _same_histogram(f, l)
        _against_numpy(f, p._values.cpu().numpy(), p._log_weights.cpu().numpy(), 40)
    assert len(set(float(f.edges[0]) for f in fast)) == M                          # every group its own extent
    # a latent of the statement log, with a shared range: no extent launch
    before = dict(count)
    lat = pyprob_amd.histogram_batch(posts, 25, range=(-3.0, 5.0), address='mu')
    assert count == {'hist': before['hist'] + 1, 'extent': before['extent']}
    lat_loop = [p.marginal('mu').histogram(25, range=(-3.0, 5.0)) for p in posts]
    lat_auto, lat_auto_loop = pyprob_amd.histogram_batch(posts, 25, address='a'), [p.marginal('a').histogram(25) for p in posts]
    for g, p in enumerate(posts):
        _same_histogram(lat[g], lat_loop[g])
        _same_histogram(lat_auto[g], lat_auto_loop[g])
        _against_numpy(lat[g], p.statement_log[0][full[0]][0].cpu().numpy(), p._all_log_weights.cpu().numpy(), 25, (-3.0, 5.0))
    # a shuffled list takes the loop and still matches it
    before = dict(count)
    mixed = pyprob_amd.histogram_batch([posts[i] for i in (2, 0, 1)], 40)
    assert count['hist'] - before['hist'] == 3
    for m, i in zip(mixed, (2, 0, 1)):
        _same_histogram(m, loop[i])
