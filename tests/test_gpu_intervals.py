"""HPD interval, cdf at a point and low-variance resampling on the device (csrc/is_hpd.hip pp_is_hpd_groups / pp_is_ecdf_groups,
csrc/is_resample.hip pp_is_resample_scheme_groups; the is_hpd_groups / is_ecdf_groups / is_resample_scheme_groups operators;
Empirical.hpd_interval / cdf / resample(scheme=); pyprob_amd.hpd_batch / cdf_batch / resample_batch(scheme=)):
 1. the HPD search EXACTLY (values and positions) against tests/interval_ref.py on the read-back sorted values, cumulative weights
    and counts of the device sort and cdf (both pinned by tests/test_gpu_order_stats.py and tests/test_gpu_resample.py: this isolates
    the new search) - one particle, a part of a wave, several groups, the tile edge (2048 and 2049), three tiles, 35 tile records,
    293 tile records (more than the second launch has threads), more than 65535 groups. The groups are those of
    tests/test_gpu_order_stats.py (normal values, five-integer ties, all-equal values, +-0.0, +-inf under a finite weight, NaN values,
    non-finite log-weights, one group with nothing counted) with, in addition, log-weights that underflow to weight 0 at the start
    of and inside the sorted order. Levels 2^-30, 0.5, 0.9, 1; the bad levels 0, 1.5 and NaN give NaN; index_out = NULL works;
    poison around every output survives;
 2. the cdf at points given per group EXACTLY, with the rank, for both values of `strict`;
 3. the three schemes EXACTLY against the reference at n_out 1, 7, 1000, 4099, with a sub-range and an offset near 2^64; scheme 0
    bit-equal to pp_is_resample_groups;
 4. bit identity of the three calls: two calls, and group g of an M-group call against the one-group call on its slice;
 5. end to end on the three-statement straight-line program (H = 64).
All of them FAIL WITHOUT THE FEATURE: the parent has neither the symbols nor the methods.
If pyprob_amd/libpyprob_amd.so is missing or stale here nothing below can run: L.load() raises instead of skipping."""
import warnings

import numpy as np
import pytest

import interval_ref as I
from pyprob_amd import lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SHAPES = [(1, 1), (1, 63), (3, 257), (2, 2048), (2, 2049), (1, 4097), (1, 70001), (1, 600001), (66000, 2)]
LEVELS = np.array([2.0 ** -30, 0.5, 0.9, 1.0, 0.0, 1.5, np.nan])
PAD = 2            # poisoned rows in front of and behind the live rows of every output
POISON32 = -0x01234568
POISON64 = -0x0123456789ABCDEF
DEV = 'cuda:0'
_PREPARED = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(M, N):
    """The groups of tests/test_gpu_order_stats.py (copies), with log-weights of -2000 - weight exp(-2000 - max) = 0 in float64 -
    on the particle of value -inf (the start of the sorted order) and on one particle in sixteen (inside it)."""
    from test_gpu_order_stats import _inputs as order_stats_inputs
    lw, x = (a.copy() for a in order_stats_inputs(M, N))
    rng = np.random.default_rng(77 * N + M)
    if N >= 63:
        lw[np.isfinite(lw) & (x == -np.inf)] = -2000.0
        lw[np.isfinite(lw) & (rng.random((M, N)) < 1.0 / 16)] = -2000.0
    elif M > 100:
        lw[(np.arange(M) % 7 == 2) & np.isfinite(lw[:, 0]), 0] = -2000.0
    return lw, x


def _prepared(M, N):
    """(lw, x) and the device sort and cdf of a shape, computed once (never modified): device tensors value [M N], cdf [M N], counted
    [M, 2] and their host copies as [M, N] / [M, 2]."""
    if (M, N) not in _PREPARED:
        from pyprob_amd import ops as P
        lw, x = _inputs(M, N)
        value, lws, _, counted = P.ops.is_sort_groups(_dev(lw.reshape(-1)), _dev(x.reshape(-1)), N, None)
        cdf = P.ops.is_cdf_groups(lws, N, None)
        torch.cuda.synchronize()
        _PREPARED[(M, N)] = dict(lw=lw, x=x, value=value, cdf=cdf, counted=counted, h_value=value.cpu().numpy().reshape(M, N),
                                 h_cdf=cdf.cpu().numpy().reshape(M, N), h_counted=counted.cpu().numpy())
    return _PREPARED[(M, N)]


def _call_hpd(value, cdf, counted, M, N, levels, want_index=True):
    """One pp_is_hpd_groups call; out and index_out carry PAD poisoned rows on either side. Host copies of the live rows."""
    lib = L.load()
    nl = len(levels)
    out = torch.full((PAD + M + PAD, nl, 2), float(POISON32), dtype=torch.float64, device=DEV)
    index = torch.full((PAD + M + PAD, nl, 2), POISON32, dtype=torch.int32, device=DEV)
    need = lib.pp_is_hpd_workspace_bytes(M, N, nl)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_hpd_groups(value.data_ptr(), cdf.data_ptr(), counted.data_ptr(), M, N, _dev(levels).data_ptr(), nl,
                                 out[PAD:].data_ptr(), index[PAD:].data_ptr() if want_index else None, ws.data_ptr(), need,
                                 L.stream_ptr()), 'pp_is_hpd_groups')
    torch.cuda.synchronize()
    out, index = out.cpu().numpy(), index.cpu().numpy()
    assert (out[:PAD] == float(POISON32)).all() and (out[PAD + M:] == float(POISON32)).all()
    assert (index[:PAD] == POISON32).all() and (index[PAD + M:] == POISON32).all()
    if not want_index:
        assert (index == POISON32).all()
    return out[PAD:PAD + M], index[PAD:PAD + M]


def _call_ecdf(value, cdf, counted, M, N, x, strict, want_rank=True):
    lib = L.load()
    Q = x.shape[1]
    out = torch.full((PAD + M + PAD, Q), float(POISON32), dtype=torch.float64, device=DEV)
    rank = torch.full((PAD + M + PAD, Q), POISON32, dtype=torch.int32, device=DEV)
    L.check(lib.pp_is_ecdf_groups(value.data_ptr(), cdf.data_ptr(), counted.data_ptr(), M, N, _dev(x).data_ptr(), Q, strict,
                                  out[PAD:].data_ptr(), rank[PAD:].data_ptr() if want_rank else None, L.stream_ptr()),
            'pp_is_ecdf_groups')
    torch.cuda.synchronize()
    out, rank = out.cpu().numpy(), rank.cpu().numpy()
    assert (out[:PAD] == float(POISON32)).all() and (out[PAD + M:] == float(POISON32)).all()
    assert (rank[:PAD] == POISON32).all() and (rank[PAD + M:] == POISON32).all()
    return out[PAD:PAD + M], rank[PAD:PAD + M]


def _call_scheme(cdf, values, M, N, lo, hi, n_out, scheme, seed, offset, multinomial_entry=False):
    lib = L.load()
    index = torch.full((PAD + M + PAD, n_out), POISON64, dtype=torch.int64, device=DEV)
    value = torch.full((PAD + M + PAD, n_out), POISON32, dtype=torch.int32, device=DEV)
    if multinomial_entry:
        rc = lib.pp_is_resample_groups(cdf.data_ptr(), values.data_ptr(), M, N, lo, hi, n_out, seed, offset & (2 ** 64 - 1),
                                       index[PAD:].data_ptr(), value[PAD:].data_ptr(), L.stream_ptr())
    else:
        rc = lib.pp_is_resample_scheme_groups(cdf.data_ptr(), values.data_ptr(), M, N, lo, hi, n_out, scheme, seed,
                                              offset & (2 ** 64 - 1), index[PAD:].data_ptr(), value[PAD:].data_ptr(), L.stream_ptr())
    L.check(rc, 'pp_is_resample_scheme_groups')
    torch.cuda.synchronize()
    index, value = index.cpu().numpy(), value.cpu().numpy()
    assert (index[:PAD] == POISON64).all() and (index[PAD + M:] == POISON64).all()
    assert (value[:PAD] == POISON32).all() and (value[PAD + M:] == POISON32).all()
    return index[PAD:PAD + M], value[PAD:PAD + M]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1. the HPD interval ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', SHAPES)
def test_hpd_is_exactly_the_reference_search_on_the_device_cdf(M, N):
    p = _prepared(M, N)
    out, index = _call_hpd(p['value'], p['cdf'], p['counted'], M, N, LEVELS)
    ref_out, ref_index = I.hpd_ref(p['h_value'], p['h_cdf'], p['h_counted'], LEVELS)
    assert np.array_equal(index, ref_index)
    assert np.array_equal(out, ref_out, equal_nan=True)
    assert (index[:, 4:] == -1).all() and np.isnan(out[:, 4:]).all()                    # the bad levels
    live = index[:, 0, 0] >= 0
    assert live.any() and (index[live][:, :4, 0] <= index[live][:, :4, 1]).all()
    with np.errstate(invalid='ignore'):
        width = out[live][:, :4, 1] - out[live][:, :4, 0]
        assert (np.nan_to_num(np.diff(width, axis=1), nan=0.0) >= 0).all()              # more mass, no shorter interval
    if 2 <= M <= 100:
        assert not live[M - 1]                                                         # (nothing counted)
    if 63 <= N <= 4097:
        c = p['h_counted'][0, 0]
        cd = p['h_cdf'][0, :c]
        first = int(np.argmax(cd > 0))
        assert first > 0 and (np.diff(cd) == 0).sum() > first                          # weight 0 at the start and inside
        assert index[0, 3, 0] == first and cd[index[0, 3, 1]] == cd[-1]                # level 1 skips the weight-0 start
    again, none = _call_hpd(p['value'], p['cdf'], p['counted'], M, N, LEVELS, want_index=False)
    assert np.array_equal(again, out, equal_nan=True)


# ---- 2. the cdf ------------------------------------------------------------------------------------------------------------------------------
def _points(p, M, N):
    """[M, 12] points per group: particle values, midpoints, below the minimum, above the maximum, +-inf, NaN."""
    v, c = p['h_value'].astype(np.float64), np.maximum(p['h_counted'][:, 0], 1)
    g = np.arange(M)
    with np.errstate(invalid='ignore', over='ignore'):
        fin = np.where(np.isfinite(v), v, 0.0)
        cols = [v[g, 0], v[g, c // 2], v[g, c - 1], v[g, np.minimum(1, c - 1)], 0.5 * (fin[g, c // 2] + fin[g, np.maximum(c // 2 - 1, 0)]),
                0.5 * (fin[g, c // 3] + fin[g, np.minimum(c // 3 + 1, c - 1)]), fin.min(1) - 1.0, fin.max(1) + 1.0,
                np.full(M, np.inf), np.full(M, -np.inf), np.full(M, np.nan), np.zeros(M)]
    return np.ascontiguousarray(np.stack(cols, 1))


@pytest.mark.parametrize('M,N', SHAPES)
def test_ecdf_is_exactly_the_reference_rank_and_ratio(M, N):
    p = _prepared(M, N)
    x = _points(p, M, N)
    got = {}
    for strict in (0, 1):
        out, rank = got[strict] = _call_ecdf(p['value'], p['cdf'], p['counted'], M, N, x, strict)
        ref_out, ref_rank = I.ecdf_ref(p['h_value'], p['h_cdf'], p['h_counted'], x, bool(strict))
        assert np.array_equal(rank, ref_rank)
        assert np.array_equal(out, ref_out, equal_nan=True)
        live = rank[:, 0] >= 0
        assert live.any() and np.isnan(out[:, 10]).all() and (rank[:, 10] == -1).all()   # NaN x
        assert np.isnan(out[~live]).all() and (rank[~live] == -1).all()
        if strict:          # nothing lies below -inf
            assert (out[live][:, 9] == 0.0).all() and (rank[live][:, 9] == 0).all()
        else:               # everything counted lies at or below +inf
            assert (out[live][:, 8] == 1.0).all() and (rank[live][:, 8] == np.minimum(p['h_counted'][live, 0], N)).all()
        assert (out[live][:, :10] >= 0).all() and (out[live][:, :10] <= 1).all()
    # P(X < x) <= P(X <= x), and at a particle's own value fewer particles lie below than at or below
    assert (got[1][0][live][:, :10] <= got[0][0][live][:, :10]).all() and (got[1][1][live][:, 1] < got[0][1][live][:, 1]).all()
    none, _ = _call_ecdf(p['value'], p['cdf'], p['counted'], M, N, x, 0, want_rank=False)
    assert np.array_equal(none, got[0][0], equal_nan=True)


# ---- 3. the schemes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', SHAPES)
def test_schemes_are_exactly_the_reference_draws(M, N):
    p = _prepared(M, N)
    cdf, values = p['h_cdf'], p['h_value']
    for n_out in ((1, 7) if M > 100 else (1, 7, 1000, 4099)):
        for scheme in (I.MULTINOMIAL, I.STRATIFIED, I.SYSTEMATIC):
            index, value = _call_scheme(p['cdf'], p['value'], M, N, 0, N, n_out, scheme, 2024, 31)
            ref_index, ref_value = I.resample_scheme_ref(cdf, values, 0, N, n_out, scheme, 2024, 31)
            assert np.array_equal(index, ref_index), (n_out, scheme)
            assert np.array_equal(value, _bits(ref_value)), (n_out, scheme)
            if scheme != I.MULTINOMIAL:
                assert (np.diff(index, axis=1) >= 0).all()                              # never decreasing within a group
            if scheme == I.MULTINOMIAL:
                old = _call_scheme(p['cdf'], p['value'], M, N, 0, N, n_out, scheme, 2024, 31, multinomial_entry=True)
                assert np.array_equal(old[0], index) and np.array_equal(old[1], value)


def test_schemes_on_a_sub_range_and_at_an_offset_near_two_to_the_64():
    M, N = 3, 257
    p = _prepared(M, N)
    for scheme in (I.MULTINOMIAL, I.STRATIFIED, I.SYSTEMATIC):
        for lo, hi, offset in ((5, 200, 31), (0, N, 2 ** 64 - 3), (100, 101, 2 ** 64 - 1)):
            index, value = _call_scheme(p['cdf'], p['value'], M, N, lo, hi, 1000, scheme, 99, offset)
            ref_index, ref_value = I.resample_scheme_ref(p['h_cdf'], p['h_value'], lo, hi, 1000, scheme, 99, offset)
            assert np.array_equal(index, ref_index) and np.array_equal(value, _bits(ref_value)), (scheme, lo, hi, offset)
            live = index[:, 0] >= 0
            assert ((index[live] >= lo) & (index[live] < hi)).all()
    lib = L.load()
    assert lib.pp_is_resample_scheme_groups(p['cdf'].data_ptr(), p['value'].data_ptr(), M, N, 0, N, 5, 3, 1, 0, None, None, None) == -1


# ---- 4. bit identity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', [s for s in SHAPES if s[1] <= 70001])
def test_bit_identity_of_calls_and_groups(M, N):
    p = _prepared(M, N)
    x = _points(p, M, N)
    n_out = 7 if M > 100 else 1000
    first = (_call_hpd(p['value'], p['cdf'], p['counted'], M, N, LEVELS), _call_ecdf(p['value'], p['cdf'], p['counted'], M, N, x, 0),
             _call_scheme(p['cdf'], p['value'], M, N, 0, N, n_out, I.STRATIFIED, 5, 1000),
             _call_scheme(p['cdf'], p['value'], M, N, 0, N, n_out, I.SYSTEMATIC, 5, 1000))
    again = (_call_hpd(p['value'], p['cdf'], p['counted'], M, N, LEVELS), _call_ecdf(p['value'], p['cdf'], p['counted'], M, N, x, 0),
             _call_scheme(p['cdf'], p['value'], M, N, 0, N, n_out, I.STRATIFIED, 5, 1000),
             _call_scheme(p['cdf'], p['value'], M, N, 0, N, n_out, I.SYSTEMATIC, 5, 1000))
    for a, b in zip(first, again):
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    for g in sorted(set([0, M // 2, M - 1])):
        v, c, k = p['value'][g * N:(g + 1) * N], p['cdf'][g * N:(g + 1) * N], p['counted'][g:g + 1].contiguous()
        one = (_call_hpd(v, c, k, 1, N, LEVELS), _call_ecdf(v, c, k, 1, N, x[g:g + 1], 0),
               _call_scheme(c, v, 1, N, 0, N, n_out, I.STRATIFIED, 5, 1000 + g * n_out),
               _call_scheme(c, v, 1, N, 0, N, n_out, I.SYSTEMATIC, 5, 1000 + g))
        for a, b in zip(one, first):
            assert np.array_equal(a[0][0], b[0][g], equal_nan=True) and np.array_equal(a[1][0], b[1][g]), g


def test_operators_shapes_types_and_argument_checks():
    from pyprob_amd import ops as P
    M, N = 3, 257
    p = _prepared(M, N)
    out, index = P.ops.is_hpd_groups(p['value'], p['cdf'], p['counted'], N, _dev(LEVELS))
    assert (out.dtype, index.dtype) == (torch.float64, torch.int32) and out.shape == index.shape == (M, len(LEVELS), 2) and out.is_cuda
    ref = _call_hpd(p['value'], p['cdf'], p['counted'], M, N, LEVELS)
    assert np.array_equal(out.cpu().numpy(), ref[0], equal_nan=True) and np.array_equal(index.cpu().numpy(), ref[1])
    x = _points(p, M, N)
    out, rank = P.ops.is_ecdf_groups(p['value'], p['cdf'], p['counted'], N, _dev(x), True)
    assert (out.dtype, rank.dtype) == (torch.float64, torch.int32) and out.shape == rank.shape == x.shape
    ref = _call_ecdf(p['value'], p['cdf'], p['counted'], M, N, x, 1)
    assert np.array_equal(out.cpu().numpy(), ref[0], equal_nan=True) and np.array_equal(rank.cpu().numpy(), ref[1])
    index, value = P.ops.is_resample_scheme_groups(p['cdf'], p['value'], N, 0, N, 7, I.SYSTEMATIC, 5, 2 ** 63 - 2, True)
    assert (index.dtype, value.dtype) == (torch.int64, torch.float32) and index.shape == value.shape == (M * 7,)
    ref = _call_scheme(p['cdf'], p['value'], M, N, 0, N, 7, I.SYSTEMATIC, 5, 2 ** 63 - 2)
    assert np.array_equal(index.cpu().numpy().reshape(M, 7), ref[0]) and np.array_equal(_bits(value.cpu().numpy()).reshape(M, 7), ref[1])
    index, value = P.ops.is_resample_scheme_groups(p['cdf'], None, N, 0, N, 7, I.STRATIFIED, 5, 0, True)
    assert index.numel() == M * 7 and value.numel() == 0
    for bad in (lambda: P.ops.is_hpd_groups(p['value'], p['cdf'].float(), p['counted'], N, _dev(LEVELS)),
                lambda: P.ops.is_hpd_groups(p['value'], p['cdf'], p['counted'].long(), N, _dev(LEVELS)),
                lambda: P.ops.is_hpd_groups(p['value'], p['cdf'], p['counted'], N, _dev(LEVELS).float()),
                lambda: P.ops.is_hpd_groups(p['value'], p['cdf'], p['counted'], N + 1, _dev(LEVELS)),
                lambda: P.ops.is_ecdf_groups(p['value'], p['cdf'], p['counted'], N, _dev(x[:2]), False),
                lambda: P.ops.is_ecdf_groups(p['value'], p['cdf'], p['counted'], N, _dev(x).float(), False),
                lambda: P.ops.is_resample_scheme_groups(p['cdf'], p['value'], N, 0, N, 7, 3, 5, 0, True),
                lambda: P.ops.is_resample_scheme_groups(p['cdf'].float(), p['value'], N, 0, N, 7, 1, 5, 0, True)):
        with pytest.raises(RuntimeError):
            bad()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
def _weights(lw):
    lw = lw.astype(np.float64)
    return np.exp(lw - lw.max())


@pytest.mark.parametrize('N', [300, 4097])
def test_straight_line_program_end_to_end(N):
    from test_gpu_joint_moments import _log_columns, _posterior, _straight_line_model
    _straight_line_model()
    post = _posterior(N)
    assert post._device_backed() and post.length == N
    lw, c = post._log_weights.cpu().numpy(), post._values.cpu().numpy().astype(np.float64)
    w = _weights(lw)
    W = w.sum()
    tau = (N * 2.0 ** -53 + 2.0 ** -48) * W          # the sequential-sum bound of the cdf and the 16 ulp of the device exp
    levels = [0.5, 0.9, 1.0]
    got = post.hpd_interval(levels)
    assert got.dtype == np.float64 and got.shape == (3, 2)
    value, _, _, counted, cdf = post._device_sorted()
    hv, hc, hk = value.cpu().numpy()[None], cdf.cpu().numpy()[None], counted.cpu().numpy()
    ref_out, ref_index = I.hpd_ref(hv, hc, hk, levels)
    assert np.array_equal(got, ref_out[0])                                               # the definition on the read-back columns
    T = hc[0, -1]
    prev = np.concatenate([[0.0], hc[0, :-1]])
    for (lo, hi), level in zip(got, levels):
        mass = w[(c >= lo) & (c <= hi)].sum()
        print('N %d level %.2f: [%.6f, %.6f] mass / W %.6f' % (N, level, lo, hi, mass / W))
        assert c.min() <= lo <= hi <= c.max() and mass >= level * W - tau
        # no valid window is shorter: every valid start's width, straight from the definition
        t = prev + level * T
        starts = np.nonzero((hc[0] > prev) & (t <= T))[0]
        ends = np.maximum(starts, np.searchsorted(hc[0], t[starts], side='left'))
        assert hi - lo == (hv[0, ends].astype(np.float64) - hv[0, starts].astype(np.float64)).min()
    one = post.hpd_interval(0.9)
    assert one == tuple(got[1]) and isinstance(one[0], float)
    elo, ehi = post.credible_interval(0.9)
    assert one[1] - one[0] <= ehi - elo
    # the cdf against float64 sums over the original arrays
    pts = np.array([got[1, 0], got[1, 1], float(np.median(c)), c.min() - 1.0, c.max() + 1.0])
    F = post.cdf(pts)
    want = np.array([w[c <= t].sum() for t in pts]) / W
    assert F.dtype == np.float64 and np.abs(F - want).max() <= 2 * tau / W and F[3] == 0.0 and F[4] == 1.0
    assert np.array_equal(F, I.ecdf_ref(hv, hc, hk, pts[None], False)[0][0])
    assert post.cdf(pts[0], strict=True) < post.cdf(pts[0]) and isinstance(post.cdf(0.5), float)
    assert post.cdf(post.quantile(0.3)) >= 0.3 * (1 - 2.0 ** -51)
    a = _log_columns(post)[0][1].cpu().numpy().astype(np.float64)
    ma = post.marginal('mu')
    mlo, mhi = ma.hpd_interval(0.9)
    wa = _weights(post._all_log_weights.cpu().numpy())
    assert wa[(a >= mlo) & (a <= mhi)].sum() >= 0.9 * wa.sum() - (N * 2.0 ** -53 + 2.0 ** -48) * wa.sum()
    # systematic resampling: device-backed, the drawn indices (recovered through resample_joint) never decrease
    r = post.resample(500, seed=11, offset=3, scheme='systematic')
    assert r._device_backed() and r.length == 500 and r.metadata['scheme'] == 'systematic'
    j = post.resample_joint(500, seed=11, offset=3, scheme='systematic')
    idx = j['index'].cpu().numpy()
    assert (np.diff(idx) >= 0).all() and np.array_equal(r._values.cpu().numpy(), post._values.cpu().numpy()[idx])
    counts = np.bincount(idx, minlength=N)
    assert (counts >= np.floor(500 * w / W - 1e-9)).all() and (counts <= np.ceil(500 * w / W + 1e-9)).all()
    s = post.resample(500, seed=11, offset=3, scheme='stratified')
    assert s.metadata['scheme'] == 'stratified' and 'scheme' not in post.resample(5, seed=1).metadata
    assert abs(r.mean - post.mean) < abs(post.stddev) and abs(s.mean - post.mean) < abs(post.stddev)


def test_batch_calls_are_one_operator_call_each_and_equal_the_loop(monkeypatch):
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
    names = ('sort', 'cdf', 'hpd', 'ecdf', 'resample_scheme', 'resample')
    count = {k: 0 for k in names}
    real = {k: getattr(P.ops, 'is_%s_groups' % k) for k in names}

    def counted(name):
        def call(*a):
            count[name] += 1
            return real[name](*a)
        return call
    for name in real:
        monkeypatch.setattr(P.ops, 'is_%s_groups' % name, counted(name), raising=False)
    levels = [0.5, 0.9]
    loop = np.stack([p.hpd_interval(levels) for p in posts])
    truths = np.array([[o['obs1'], o['obs0']] for o in observes])
    cloop = np.stack([p.cdf(truths[g]) for g, p in enumerate(posts)])
    assert count['hpd'] == M and count['ecdf'] == M and count['sort'] == M
    before = dict(count)
    fast = pyprob_amd.hpd_batch(posts, levels)
    assert {k: count[k] - before[k] for k in names} == {'sort': 1, 'cdf': 1, 'hpd': 1, 'ecdf': 0, 'resample_scheme': 0, 'resample': 0}
    assert fast.shape == (M, 2, 2) and fast.dtype == np.float64 and np.array_equal(fast, loop)
    assert np.array_equal(pyprob_amd.hpd_batch(posts, 0.9), loop[:, 1])
    before = dict(count)
    fast = pyprob_amd.cdf_batch(posts, truths)
    assert {k: count[k] - before[k] for k in names} == {'sort': 1, 'cdf': 1, 'hpd': 0, 'ecdf': 1, 'resample_scheme': 0, 'resample': 0}
    assert fast.shape == (M, 2) and np.array_equal(fast, cloop) and ((fast > 0) & (fast < 1)).any()
    assert np.array_equal(pyprob_amd.cdf_batch(posts, truths[:, 0]), cloop[:, 0])
    lat = pyprob_amd.hpd_batch(posts, levels, address='mu')
    assert np.array_equal(lat, np.stack([p.marginal('mu').hpd_interval(levels) for p in posts]))
    assert np.array_equal(pyprob_amd.cdf_batch(posts, truths[:, 1], address='mu'),
                          np.array([p.marginal('mu').cdf(truths[g, 1]) for g, p in enumerate(posts)]))
    # resample_batch(scheme=): one draw call for the M groups, the values of the loop at offset + g (systematic) / offset + g n
    n = 64
    for scheme, step in (('systematic', 1), ('stratified', n)):
        before = dict(count)
        fast = pyprob_amd.resample_batch(posts, n, seed=9, offset=500, scheme=scheme)
        assert count['resample_scheme'] - before['resample_scheme'] == 1 and count['resample'] == before['resample']
        for g, (r, p) in enumerate(zip(fast, posts)):
            one = p.resample(n, seed=9, offset=500 + g * step, scheme=scheme)
            assert torch.equal(r._values, one._values) and r.metadata['scheme'] == scheme and r._device_backed()
    before = dict(count)
    out = pyprob_amd.resample_batch(posts, n, seed=9, offset=500)
    assert count['resample'] - before['resample'] == 1 and count['resample_scheme'] == before['resample_scheme']
    assert 'scheme' not in out[0].metadata
    # a shuffled list takes the loop and still matches it
    mixed = pyprob_amd.hpd_batch([posts[i] for i in (2, 0, 1)], levels)
    assert np.array_equal(mixed, loop[[2, 0, 1]])
