"""Exact weighted quantiles and combine_duplicates on the device (csrc/is_sort.hip pp_is_sort_groups / pp_is_quantile_groups /
pp_is_unique_groups; the is_sort_groups / is_quantile_groups / is_unique_groups operators; Empirical.quantile / credible_interval /
argsort / combine_duplicates; pyprob_amd.quantile_batch):
 1. the sort against numpy's stable argsort of the reference keys (tests/order_stats_ref.py): index, value bits, log-weight bits and
    the two counts EXACTLY - one particle, a part of a wave, several groups, a tile + 1, three tiles, 35 tiles, 2^20 + 3 particles,
    more than 65535 groups. The groups hold normal values, values from five integers, all-equal, ascending and descending values,
    negatives and denormals, -0.0 / +0.0 pairs, +-inf under a finite weight, NaN x under a finite weight, non-finite lw with NaN x,
    and one group with nothing counted; poison around every output survives;
 2. bit identity: two calls, with and without `stats`, group g of an M-group call against the one-group call on its slice;
 3. the quantile search EXACTLY against the reference search on the read-back cdf of the sorted log-weights (pp_is_cdf_groups is
    pinned by tests/test_gpu_resample.py: this isolates the new search);
 4. the quantile against float64 numpy sums over the ORIGINAL arrays: a returned v has W(x < v) <= q W + tau and
    W(x <= v) >= q W - tau with tau = (n_per 2^-53 + 2^-48) W - the sequential-sum bound of the cdf and the 16 ulp of the device exp
    the histogram bound already uses;
 5. the runs: number, values (bits) and counts exactly, every mass within |mass - sum w 2^S| <= 0.5 count + 2^-48 sum w 2^S, the
    masses of a row adding up to the same integer as the 1-bin histogram row of the same particles, poison beyond `runs` intact;
 6. end to end on the three-statement straight-line program (H = 64): quantile / credible_interval by property 4 on the read-back
    columns, combine_duplicates on a latent the program rounds to five values, quantile_batch one operator call each and bit-equal
    to the loop.
All of them FAIL WITHOUT THE FEATURE: the parent has neither the symbols nor the methods.
If pyprob_amd/libpyprob_amd.so is missing or stale here nothing below can run: L.load() raises instead of skipping."""
import math
import warnings

import numpy as np
import pytest

import histogram_ref as H
import order_stats_ref as R
from pyprob_amd import lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SHAPES = [(1, 1), (1, 63), (3, 257), (7, 300), (2, 2049), (1, 4097), (1, 70001), (1, 2 ** 20 + 3), (66000, 2)]
QS = np.array([0.0, 2.0 ** -30, 0.025, 0.5, 0.975, 1.0])
PAD = 2            # poisoned rows in front of and behind the live rows of every output
POISON32 = -0x01234568
POISON64 = -0x0123456789ABCDEF
DEV = 'cuda:0'
_INPUTS, _SORTED = {}, {}


def _pattern(kind, n, rng):
    if kind == 0:
        return rng.normal(0.0, 1.5, n)
    if kind == 1:
        return rng.integers(-2, 3, n).astype(np.float64)            # five integers: heavy ties
    if kind == 2:
        return np.full(n, 0.75)
    if kind == 3:
        return np.linspace(-3.0, 3.0, n)
    if kind == 4:
        return np.linspace(3.0, -3.0, n)
    v = -np.abs(rng.normal(0.0, 1.0, n))                             # negatives, and denormals of either sign
    v[::3] = rng.integers(-40, 40, len(v[::3])) * 1.4e-45
    return v


def _inputs(M, N):
    """lw ~ normal(0, 3) and x - a function of (M, N) alone. Group 0 is six stretches, one per pattern; group g > 0 is pattern
    g % 6 throughout. Where the group is long enough, 13 particles chosen at random become -0.0 / +0.0 pairs, -inf and +inf under a
    finite weight, NaN under a finite weight, and lw = -inf, +inf, NaN with x = NaN. The last group of 2 <= M <= 100 has nothing
    counted (no finite weight, or a NaN value). Groups of two particles get their special values by the group's number."""
    if (M, N) not in _INPUTS:
        rng = np.random.default_rng(1000 * N + M)
        lw = rng.normal(0.0, 3.0, (M, N)).astype(np.float32)
        x = np.empty((M, N), np.float32)
        if M > 100:
            for kind in range(6):
                rows = np.arange(kind, M, 6)
                x[rows] = _pattern(kind, len(rows) * N, rng).reshape(len(rows), N).astype(np.float32)
            g = np.arange(M)
            x[g % 11 == 3, 0] = np.nan
            lw[g % 13 == 5, 1] = -np.inf
            x[g % 13 == 5, 1] = np.nan
            x[g % 17 == 1] = np.array([0.0, -0.0], np.float32)
            x[g % 19 == 2] = np.array([np.inf, -np.inf], np.float32)
        else:
            cuts = np.linspace(0, N, 7).astype(int)
            for kind in range(6):
                x[0, cuts[kind]:cuts[kind + 1]] = _pattern(kind, cuts[kind + 1] - cuts[kind], rng).astype(np.float32)
            for g in range(1, M):
                x[g] = _pattern(g % 6, N, rng).astype(np.float32)
            if N >= 63:
                for g in range(M):
                    at = rng.choice(N, 13, replace=False)
                    x[g, at[:4]] = np.array([-0.0, 0.0, 0.0, -0.0], np.float32)
                    x[g, at[4:8]] = np.array([-np.inf, np.inf, np.nan, np.nan], np.float32)
                    lw[g, at[8:]] = np.array([-np.inf, np.inf, np.nan, -np.inf, np.nan], np.float32)
                    x[g, at[8:]] = np.nan
            if 2 <= M:
                lw[M - 1, ::2] = rng.choice(np.array([-np.inf, np.nan, np.inf], np.float32), len(lw[M - 1, ::2]))
                x[M - 1, 1::2] = np.nan
        _INPUTS[(M, N)] = (lw, x)
    return _INPUTS[(M, N)]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call_sort(lw, x, stats=None):
    """One pp_is_sort_groups call on host arrays; every output carries PAD poisoned rows in front of and behind its live rows.
    Returns the host copies (value as int32 bits [P + M + P, N], lw bits, index, counted [P + M + P, 2]) and the device tensors."""
    lib = L.load()
    M, N = lw.shape
    tl, tx = _dev(lw.reshape(-1)), _dev(x.reshape(-1))
    rows = PAD + M + PAD
    value = torch.full((rows, N), POISON32, dtype=torch.int32, device=DEV)
    lwo = torch.full((rows, N), POISON32, dtype=torch.int32, device=DEV)
    index = torch.full((rows, N), POISON32, dtype=torch.int32, device=DEV)
    counted = torch.full((rows, 2), POISON32, dtype=torch.int32, device=DEV)
    need = lib.pp_is_sort_workspace_bytes(M, N)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_sort_groups(tl.data_ptr(), tx.data_ptr(), M, N, L.ptr(stats), value[PAD:].data_ptr(), lwo[PAD:].data_ptr(),
                                  index[PAD:].data_ptr(), counted[PAD:].data_ptr(), ws.data_ptr(), need, L.stream_ptr()),
            'pp_is_sort_groups')
    torch.cuda.synchronize()
    return (value.cpu().numpy(), lwo.cpu().numpy(), index.cpu().numpy(), counted.cpu().numpy()), (value, lwo, index, counted)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _sorted(M, N):
    """The device outputs (host copies and device tensors) and the reference of a shape, computed once (never modified)."""
    if (M, N) not in _SORTED:
        lw, x = _inputs(M, N)
        _SORTED[(M, N)] = _call_sort(lw, x) + (R.sort_ref(lw, x),)
    return _SORTED[(M, N)]


def _stats(lw, x):
    """pp_is_stats per group: device double [M, 6]."""
    from pyprob_amd import ops as P
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    rows = [P.ops.is_stats(torch.from_numpy(lw[g]).to(DEV), torch.from_numpy(x[g]).to(DEV), scratch)[:6] for g in range(lw.shape[0])]
    return torch.stack(rows).contiguous()


def _live(t, M):
    """The live rows of a padded device tensor as one flat contiguous tensor of its own dtype's float view where it holds floats."""
    return t[PAD:PAD + M].reshape(-1)


# ---- 1. the sort ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', SHAPES)
def test_sort_equals_the_stable_argsort_of_the_keys(M, N):
    lw, x = _inputs(M, N)
    (value, lwo, index, counted), _, (rv, rl, ri, rc) = _sorted(M, N)
    for a in (value, lwo, index, counted):
        assert (a[:PAD] == POISON32).all() and (a[PAD + M:] == POISON32).all()          # the poison survives
    assert np.array_equal(counted[PAD:PAD + M], rc)
    assert np.array_equal(index[PAD:PAD + M], ri)
    assert np.array_equal(value[PAD:PAD + M], _bits(rv)) and np.array_equal(lwo[PAD:PAD + M], _bits(rl))
    if N >= 63 and M <= 100:
        live = M - 1 if M >= 2 else M
        assert (rc[:live, 1] == 2).all() and (rc[:live, 0] == N - 7).all()
        for g in range(live):            # -inf first, +inf last of the counted, the zeros adjacent in particle order
            c = rc[g, 0]
            v = rv[g, :c]
            assert v[0] == -np.inf and v[c - 1] == np.inf
            z = np.nonzero(v == 0)[0]
            assert len(z) >= 4 and (np.diff(z) == 1).all() and (np.diff(ri[g, z]) > 0).all()
            assert np.signbit(v[z]).any() and not np.signbit(v[z]).all()          # (the original bits, both signs)
    if 2 <= M <= 100:
        assert rc[M - 1, 0] == 0 and rc[M - 1, 1] > 0 and np.array_equal(ri[M - 1], np.arange(N))


# ---- 2. bit identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', [s for s in SHAPES if s[1] <= 70001])
def test_bit_identity_of_calls_groups_and_statistics(M, N):
    lw, x = _inputs(M, N)
    got = [a[PAD:PAD + M] for a in _sorted(M, N)[0]]
    again = [a[PAD:PAD + M] for a in _call_sort(lw, x)[0]]
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    groups = sorted(set([0, M // 2, M - 1]))
    if M <= 100:
        stats = _stats(lw, x)
        with_stats = [a[PAD:PAD + M] for a in _call_sort(lw, x, stats)[0]]
        assert all(np.array_equal(a, b) for a, b in zip(got, with_stats))
    for g in groups:
        one = [a[PAD] for a in _call_sort(lw[g:g + 1], x[g:g + 1])[0]]
        assert all(np.array_equal(a, b[g]) for a, b in zip(one, got)), g


# ---- 3. / 4. the quantile ------------------------------------------------------------------------------------------------------------------
def _quantiles(M, N):
    from pyprob_amd import ops as P
    lib = L.load()
    _, (value, lwo, _, counted), _ = _sorted(M, N)
    v = _live(value, M).view(torch.float32).contiguous()
    l = _live(lwo, M).view(torch.float32).contiguous()
    c = counted[PAD:PAD + M].contiguous()
    cdf = P.ops.is_cdf_groups(l, N, None)
    out = torch.full((PAD + M + PAD, len(QS)), float(POISON32), dtype=torch.float64, device=DEV)
    L.check(lib.pp_is_quantile_groups(v.data_ptr(), cdf.data_ptr(), c.data_ptr(), M, N, _dev(QS).data_ptr(), len(QS),
                                      out[PAD:].data_ptr(), L.stream_ptr()), 'pp_is_quantile_groups')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:PAD] == float(POISON32)).all() and (out[PAD + M:] == float(POISON32)).all()
    return out[PAD:PAD + M], cdf.cpu().numpy().reshape(M, N)


def _property(got, lw, x, qs, label):
    """W(x < v) <= q W + tau and W(x <= v) >= q W - tau over the ORIGINAL arrays in float64 numpy; nothing counted: NaN."""
    M, N = lw.shape
    ok = np.isfinite(lw) & ~np.isnan(x)
    top = R.group_max(lw)
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.where(ok, np.exp(np.where(ok, lw.astype(np.float64), 0.0) - np.where(np.isfinite(top), top, 0.0)[:, None]), 0.0)
    W = w.sum(1)
    tau = (N * 2.0 ** -53 + 2.0 ** -48) * W
    xs = np.where(ok, x.astype(np.float64), np.inf)
    none = ok.sum(1) == 0
    assert np.isnan(got[none]).all() and not np.isnan(got[~none]).any(), label
    worst = 0.0
    for j, q in enumerate(qs):
        v = got[:, j][:, None]
        with np.errstate(invalid='ignore'):
            below, upto = (w * (xs < v)).sum(1), (w * (xs <= v)).sum(1)
        low, high = below - q * W, q * W - upto
        worst = max(worst, float(np.max(np.where(none, 0.0, np.maximum(low, high) / np.maximum(tau, 1e-300)))))
        assert (none | ((low <= tau) & (high <= tau))).all(), (label, q, np.argwhere(~(none | ((low <= tau) & (high <= tau))))[:5].tolist())
    print('%s: worst excess over q W in units of tau: %.3g' % (label, worst))


@pytest.mark.parametrize('M,N', SHAPES)
def test_quantile_search_is_exact_on_the_device_cdf_and_holds_the_weight_property(M, N):
    lw, x = _inputs(M, N)
    (value, _, _, counted), _, _ = _sorted(M, N)
    got, cdf = _quantiles(M, N)
    ref = R.quantile_ref(value[PAD:PAD + M].view(np.float32), cdf, counted[PAD:PAD + M], QS)
    assert np.array_equal(got, ref, equal_nan=True)
    _property(got, lw, x, QS, str((M, N)))
    live = ~np.isnan(got[:, 0])
    assert (got[live][:, 1:] >= got[live][:, :-1]).all()              # quantiles do not decrease in q
    if N >= 63 and M == 1:
        assert got[0, -1] == np.inf                                    # (+inf carries weight: it is the last quantile)


# ---- 5. the runs ---------------------------------------------------------------------------------------------------------------------------
def _call_unique(M, N, stats=None):
    lib = L.load()
    _, (value, lwo, _, counted), _ = _sorted(M, N)
    v = _live(value, M).view(torch.float32).contiguous()
    l = _live(lwo, M).view(torch.float32).contiguous()
    c = counted[PAD:PAD + M].contiguous()
    rows = PAD + M + PAD
    uv = torch.full((rows, N), POISON32, dtype=torch.int32, device=DEV)
    mass = torch.full((rows, N), POISON64, dtype=torch.int64, device=DEV)
    count = torch.full((rows, N), POISON32, dtype=torch.int32, device=DEV)
    runs = torch.full((rows,), POISON32, dtype=torch.int32, device=DEV)
    need = lib.pp_is_unique_workspace_bytes(M, N)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.pp_is_unique_groups(v.data_ptr(), l.data_ptr(), c.data_ptr(), M, N, L.ptr(stats), uv[PAD:].data_ptr(),
                                    mass[PAD:].data_ptr(), count[PAD:].data_ptr(), runs[PAD:].data_ptr(), ws.data_ptr(), need,
                                    L.stream_ptr()), 'pp_is_unique_groups')
    torch.cuda.synchronize()
    return uv.cpu().numpy(), mass.cpu().numpy(), count.cpu().numpy(), runs.cpu().numpy()


@pytest.mark.parametrize('M,N', SHAPES)
def test_runs_values_counts_and_fixed_point_masses(M, N):
    from pyprob_amd import ops as P
    lw, x = _inputs(M, N)
    _, _, (rv, rl, _, rc) = _sorted(M, N)
    uv, mass, count, runs = _call_unique(M, N)
    for a, p in ((uv, POISON32), (mass, POISON64), (count, POISON32), (runs, POISON32)):
        assert (a[:PAD] == p).all() and (a[PAD + M:] == p).all()
    ref = R.unique_ref(rv, rl, rc)
    r = np.array([len(t[0]) for t in ref])
    assert np.array_equal(runs[PAD:PAD + M], r)
    col = np.arange(N)[None, :]
    beyond = col >= r[:, None]
    uvl, ml, cl = uv[PAD:PAD + M], mass[PAD:PAD + M], count[PAD:PAD + M]
    assert (uvl[beyond] == POISON32).all() and (ml[beyond] == POISON64).all() and (cl[beyond] == POISON32).all()
    assert np.array_equal(uvl[~beyond], np.concatenate([_bits(t[0]) for t in ref]))
    assert np.array_equal(cl[~beyond], np.concatenate([t[2] for t in ref]))
    got = ml[~beyond]
    real = np.concatenate([t[3] for t in ref])
    err = np.abs(got.astype(np.longdouble) - real)
    bound = np.longdouble(0.5) * cl[~beyond] + np.longdouble(2.0 ** -48) * real
    print('%s: max |mass - sum w 2^S| / bound = %.3g; masses that differ from the numpy emulation: %d' % (
        (M, N), float((err / bound).max()) if len(err) else 0.0, int((got != np.concatenate([t[1] for t in ref])).sum())))
    assert (err <= bound).all() and (got >= 0).all()
    # the same integer as the 1-bin histogram row of the same particles (bin, below, above; the NaN slot holds the NaN values)
    row = P.ops.is_hist_groups(_dev(lw.reshape(-1)), _dev(x.reshape(-1)), None, N, _dev(np.array([-1.0, 1.0])), None, None).cpu().numpy()
    totals = np.where(beyond, 0, ml).sum(1)
    assert np.array_equal(totals, row[:, 0, :3].sum(1)) and np.array_equal(np.where(beyond, 0, cl).sum(1), row[:, 1, :3].sum(1))
    if M <= 100:            # the maxima of pp_is_stats instead of the kernel's own: the same bits
        assert all(np.array_equal(a, b) for a, b in zip(_call_unique(M, N, _stats(lw, x)), (uv, mass, count, runs)))
    if 2 <= M <= 100:
        assert r[M - 1] == 0
    if N >= 63 and M == 1:
        assert r[0] < rc[0, 0]                                         # (ties: fewer runs than particles)


def test_operators_shapes_types_and_argument_checks():
    from pyprob_amd import ops as P
    M, N = 3, 257
    lw, x = _inputs(M, N)
    (value, lwo, index, counted), _, _ = _sorted(M, N)
    tl, tx = _dev(lw.reshape(-1)), _dev(x.reshape(-1))
    v, l, i, c = P.ops.is_sort_groups(tl, tx, N, None)
    assert (v.dtype, l.dtype, i.dtype, c.dtype) == (torch.float32, torch.float32, torch.int32, torch.int32)
    assert v.shape == l.shape == i.shape == (M * N,) and c.shape == (M, 2) and v.is_cuda
    assert np.array_equal(_bits(v.cpu().numpy()).reshape(M, N), value[PAD:PAD + M])
    assert np.array_equal(i.cpu().numpy().reshape(M, N), index[PAD:PAD + M]) and np.array_equal(c.cpu().numpy(), counted[PAD:PAD + M])
    cdf = P.ops.is_cdf_groups(l, N, None)
    out = P.ops.is_quantile_groups(v, cdf, c, N, _dev(QS))
    assert out.dtype == torch.float64 and out.shape == (M, len(QS))
    assert np.array_equal(out.cpu().numpy(), _quantiles(M, N)[0], equal_nan=True)
    uv, mass, count, runs = P.ops.is_unique_groups(v, l, c, N, None)
    assert (uv.dtype, mass.dtype, count.dtype, runs.dtype) == (torch.float32, torch.int64, torch.int32, torch.int32)
    assert uv.shape == mass.shape == count.shape == (M, N) and runs.shape == (M,)
    assert np.array_equal(runs.cpu().numpy(), _call_unique(M, N)[3][PAD:PAD + M])
    for bad in (lambda: P.ops.is_sort_groups(tl, tx[:-1], N, None), lambda: P.ops.is_sort_groups(tl, tx, N + 1, None),
                lambda: P.ops.is_sort_groups(tl.double(), tx, N, None), lambda: P.ops.is_quantile_groups(v, cdf.float(), c, N, _dev(QS)),
                lambda: P.ops.is_quantile_groups(v, cdf, c.long(), N, _dev(QS)), lambda: P.ops.is_quantile_groups(v, cdf, c, N, _dev(QS).float()),
                lambda: P.ops.is_unique_groups(v, l[:-1], c, N, None), lambda: P.ops.is_unique_groups(v, l, c[:2], N, None),
                lambda: P.ops.is_unique_groups(v, l, c, N, torch.zeros(5, dtype=torch.float64, device=DEV))):
        with pytest.raises(RuntimeError):
            bad()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------
_ROUNDED = []


def _rounded_model():
    """The straight-line program of tests/test_gpu_joint_moments.py (its constructed H = 64 network), returning c rounded to the
    five values -1 .. 3."""
    if not _ROUNDED:
        import pyprob_amd as pyprob
        from pyprob_amd import Model
        from pyprob_amd.distributions import Normal, Uniform
        from test_gpu_joint_moments import SIGMA, _straight_line_model
        base, _ = _straight_line_model()

        class Rounded(Model):
            def forward(self):
                a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a', name='mu')
                pyprob.observe(Normal(a, SIGMA), name='obs0')
                b = pyprob.sample(Normal(a, 0.7), address='b')
                c = pyprob.sample(Uniform(b - 1.0, b + 1.0), address='c')
                pyprob.observe(Normal(c, SIGMA), name='obs1')
                return torch.clamp(torch.round(c), -1.0, 3.0)
        model = Rounded()
        model._inference_network = base._inference_network
        _ROUNDED.append(model)
    return _ROUNDED[0]


@pytest.mark.parametrize('N', [300, 4097])
def test_straight_line_program_end_to_end(N):
    from pyprob_amd.state import InferenceEngine
    from test_gpu_joint_moments import _log_columns, _posterior, _straight_line_model
    _straight_line_model()
    post = _posterior(N)
    assert post._device_backed() and post.length == N
    lw = post._log_weights.cpu().numpy()[None]
    c = post._values.cpu().numpy()[None]
    qs = [0.0, 0.025, 0.25, 0.5, 0.975, 1.0]
    got = post.quantile(qs)
    assert got.dtype == np.float64 and got.shape == (6,) and c.min() <= got[0] <= got[-1] <= c.max()
    _property(got[None], lw, c, qs, 'posterior %d' % N)
    assert post.quantile(0.5) == got[3] and isinstance(post.quantile(0.5), float)
    lo, hi = post.credible_interval(0.9)
    _property(np.array([[lo, hi]]), lw, c, [0.05, 0.95], 'interval %d' % N)
    assert lo <= post.quantile(0.5) <= hi and lo <= post.credible_interval(0.5)[0]
    assert '_dev_sorted' in post.__dict__ and not post._host_weights_ready()          # sorted once, no host weights
    order = post.argsort()
    assert order.dtype == torch.int64 and order.is_cuda and order.numel() == N
    assert np.array_equal(order.cpu().numpy(), np.argsort(c[0], kind='stable'))
    a = _log_columns(post)[0][1]
    ma = post.marginal('mu')
    _property(ma.quantile(qs)[None], post._all_log_weights.cpu().numpy()[None], a.cpu().numpy()[None], qs, 'marginal %d' % N)
    # a latent the program rounds to five values
    model = _rounded_model()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        rp = model.posterior_results(N, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, observe={'obs0': 2.0, 'obs1': 1.5},
                                     lock_step=True, seed=13, offset=64)
    assert rp._device_backed()
    d = rp.combine_duplicates()
    v, l = rp._values.cpu().numpy().astype(np.float64), rp._log_weights.cpu().numpy().astype(np.float64)
    w = np.exp(l - l.max())
    W = w.sum()
    distinct = np.unique(v)
    assert d._device_backed() and d.metadata['op'] == 'combine_duplicates' and 2 <= len(distinct) <= 5
    assert np.array_equal(d._values.cpu().numpy().astype(np.float64), distinct)          # ascending
    want = np.array([w[v == t].sum() for t in distinct]) / W
    tol = N * 2.0 ** -(H.shift(N) + 1) / W + 1e-12
    print('combine_duplicates: max weight error %.3g (tolerance %.3g)' % (float(np.abs(d.weights_numpy() - want).max()), tol))
    assert np.abs(d.weights_numpy() - want).max() <= tol
    assert float(d.mode) == distinct[int(np.argmax(want))]
    assert abs(d.mean - rp.mean) <= 1e-6 * max(1.0, abs(rp.mean))


def test_quantile_batch_is_one_operator_call_each_and_equals_the_loop(monkeypatch):
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
    count = {'sort': 0, 'cdf': 0, 'quantile': 0}
    real = {'sort': P.ops.is_sort_groups, 'cdf': P.ops.is_cdf_groups, 'quantile': P.ops.is_quantile_groups}

    def counted(name):
        def call(*a):
            count[name] += 1
            return real[name](*a)
        return call
    for name in real:
        monkeypatch.setattr(P.ops, 'is_%s_groups' % name, counted(name), raising=False)
    qs = [0.05, 0.5, 0.95]
    loop = np.stack([p.quantile(qs) for p in posts])
    assert count == {'sort': M, 'cdf': M, 'quantile': M}
    fast = pyprob_amd.quantile_batch(posts, qs)
    assert count == {'sort': M + 1, 'cdf': M + 1, 'quantile': M + 1}                     # ONE operator call each for the M groups
    assert fast.shape == (M, 3) and fast.dtype == np.float64 and np.array_equal(fast, loop)
    for g, p in enumerate(posts):
        _property(fast[g:g + 1], p._log_weights.cpu().numpy()[None], p._values.cpu().numpy()[None], qs, 'group %d' % g)
    before = dict(count)
    lat = pyprob_amd.quantile_batch(posts, qs, address='mu')
    assert count == {k: before[k] + 1 for k in before}
    assert np.array_equal(lat, np.stack([p.marginal('mu').quantile(qs) for p in posts]))
    assert np.array_equal(pyprob_amd.quantile_batch(posts, 0.5), loop[:, 1:2])
    # a shuffled list takes the loop and still matches it
    before = dict(count)
    mixed = pyprob_amd.quantile_batch([posts[i] for i in (2, 0, 1)], qs)
    assert count['quantile'] - before['quantile'] == 3 and count['sort'] == before['sort']          # (sorted before: kept)
    assert np.array_equal(mixed, loop[[2, 0, 1]])
