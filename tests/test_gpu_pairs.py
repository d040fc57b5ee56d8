"""pp_is_pairs_groups (csrc/is_pairs.hip), Empirical.compare_joint and pyprob_amd.compare_joint_batch on the device against a float64
numpy restatement of the six pair sums. The bound is the one derived at the head of csrc/is_pairs.hip (u = 2^-24, K = J + 2 rounded up
to even, alpha^2 = log2(e) / h^2), computed pair by pair from the restatement itself:
    Gaussian   sum_ij w_i v_j k_ij expm1(ln 2 (2 K + 9) S_ij u + 130 u) + (n_a + n_b + 64) 2^-53 k_sum + n_r n_c 2^-126 / (W_r W_c)
               S_ij = alpha^2 (sum_j |z_j z'_j| + |z|^2 + |z'|^2) + log2(e) (|lw_i - max| + |lw'_j - max'|)
    distance   sum_ij w_i v_j (d_ij (J / 2 + 133) + |z_i| + |z'_j|) u + (n_a + n_b + 64) 2^-53 d_sum
PP_PAIRS_ERRORS=<file> appends every case's worst error / bound ratio (profiles/pairs_errors.jsonl). All of it fails without the
feature: the parent has neither the symbols nor the methods."""
import json
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

DEV = 'cuda:0'
U, LOG2E = 2.0 ** -24, 1.4426950408889634
NAMES = ('k_aa', 'k_bb', 'k_ab', 'd_aa', 'd_bb', 'd_ab')


def _six_sums(lw_a, x_a, lw_b, x_b, center, inv_scale, h):
    """(the ten numbers of a row of pp_is_pairs_groups in float64, the bound of each of the six sums). lw: [n]; x: [n, J]."""
    J = x_a.shape[1]
    K = (J + 3) & ~1
    sides = []
    for lw, x in ((lw_a, x_a), (lw_b, x_b)):
        lw = lw.astype(np.float64)
        with np.errstate(invalid='ignore'):
            z = (x.astype(np.float64) - center) * inv_scale
        keep = np.isfinite(lw) & np.isfinite(z).all(1)
        top = lw[np.isfinite(lw)].max() if np.isfinite(lw).any() else 0.0
        sides.append((z[keep], np.exp(lw[keep] - top), LOG2E * np.abs(lw[keep] - top), len(lw)))
    row, bound = np.full(10, np.nan), np.full(6, np.nan)
    with np.errstate(invalid='ignore', divide='ignore'):
        for p, (r, c) in enumerate(((0, 0), (1, 1), (0, 1))):
            (zr, wr, lr, nr), (zc, wc, lc, nc) = sides[r], sides[c]
            r2 = sum((zr[:, None, j] - zc[None, :, j]) ** 2 for j in range(J))
            cross = sum(np.abs(zr[:, None, j] * zc[None, :, j]) for j in range(J))
            norm_r, norm_c = np.sqrt((zr * zr).sum(1)), np.sqrt((zc * zc).sum(1))
            ww = wr[:, None] * wc[None, :] / (wr.sum() * wc.sum())
            S = LOG2E / (h * h) * (cross + norm_r[:, None] ** 2 + norm_c[None, :] ** 2) + lr[:, None] + lc[None, :]
            k, d = ww * np.exp(-0.5 * r2 / (h * h)), ww * np.sqrt(r2)
            slack = (sides[0][3] + sides[1][3] + 64) * 2.0 ** -53
            row[p], row[3 + p] = k.sum(), d.sum()
            bound[p] = (k * np.expm1(np.log(2.0) * (2 * K + 9) * S * U + 130 * U)).sum() + slack * row[p] + \
                nr * nc * 2.0 ** -126 / (wr.sum() * wc.sum())
            bound[3 + p] = ((d * (J / 2 + 133) + ww * (norm_r[:, None] + norm_c[None, :])) * U).sum() + slack * row[3 + p]
        for s, (z, w, _, _) in enumerate(sides):
            row[6 + s], row[8 + s] = (w * w).sum() / w.sum() ** 2, len(w)
    return row, bound


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _op(lw_a, x_a, lw_b, x_b, center, inv_scale, h):
    """One pp_is_pairs_groups call on host arrays lw [M, n], x [M, n, J] (float32), center / inv_scale [M, J], h [M]."""
    from pyprob_amd import ops as P
    side = lambda lw, x: (_dev(lw.reshape(-1)), [_dev(x[:, :, j].reshape(-1)) for j in range(x.shape[2])], lw.shape[1], None)  # noqa: E731
    return P.ops.is_pairs_groups(*side(lw_a, x_a), *side(lw_b, x_b), _dev(center), _dev(inv_scale), _dev(h)).cpu().numpy()


def _side(rng, n, J, center, scale, shift):
    """lw [n] within 20 of its maximum and x [n, J] with |z| <= 4, float32; from five particles on, three of them dropped: lw = -inf,
    lw = NaN and a NaN coordinate under a finite weight."""
    z = np.clip(shift + rng.standard_normal((n, J)), -3.9, 3.9)
    x = (center + scale * z).astype(np.float32)
    lw = (-20.0 * rng.random(n)).astype(np.float32)
    if n >= 5:
        lw[1], lw[n // 2], x[n - 2, J - 1] = -np.inf, np.nan, np.nan
    return lw, x


def _record(rec):
    print('pairs', json.dumps(rec))
    if os.environ.get('PP_PAIRS_ERRORS'):
        with open(os.environ['PP_PAIRS_ERRORS'], 'a') as f:
            f.write(json.dumps(rec) + '\n')


CASES = [(na, nb, J, 'plain') for na, nb in ((1, 1), (31, 33), (127, 129), (300, 2049)) for J in (1, 2, 3, 8)] + [(127, 129, 2, 'narrow')]


@pytest.mark.parametrize('na,nb,J,kind', CASES)
def test_pair_sums_stay_within_the_derived_bound(na, nb, J, kind):
    rng = np.random.default_rng(1000 * na + 10 * J + (kind == 'narrow'))
    center = np.full(J, 1000.0) if kind == 'narrow' else rng.uniform(-2.0, 2.0, J)
    scale = np.full(J, 1e-2) if kind == 'narrow' else rng.uniform(0.5, 2.0, J)
    h = np.sqrt(J)
    (lw_a, x_a), (lw_b, x_b) = _side(rng, na, J, center, scale, 0.0), _side(rng, nb, J, center, scale, 0.5)
    args = (lw_a[None], x_a[None], lw_b[None], x_b[None], center[None], 1.0 / scale[None], np.array([h]))
    got = _op(*args)[0]
    want, bound = _six_sums(lw_a, x_a, lw_b, x_b, center, 1.0 / scale, h)
    ratio = np.abs(got[:6] - want[:6]) / bound
    rel = bound / np.where(want[:6] > 0, want[:6], np.inf)
    _record(dict(case='%d x %d, J = %d, %s' % (na, nb, J, kind), worst_ratio=dict(zip(NAMES, ratio.tolist())),
                 relative_bound=dict(zip(NAMES, rel.tolist()))))
    assert (rel < 1e-3).all(), rel                              # (a looser derivation is not a test)
    assert (ratio <= 1.0).all(), (got, want, bound)
    assert got[8] == want[8] == (na - 3 if na >= 5 else na) and got[9] == want[9]
    assert np.allclose(got[6:8], want[6:8], rtol=1e-12, atol=0)
    assert np.array_equal(_op(*args).view(np.int64)[0], got.view(np.int64))          # the same bits again
    if (na, J) == (31, 3):       # a side with no counted particle: NaN where it enters, the other side's own sums stand
        dead = _op(np.full_like(args[0], -np.inf), *args[1:])[0]
        assert np.isnan(dead[[0, 2, 3, 5, 6]]).all() and dead[8] == 0 and np.array_equal(dead[[1, 4, 7, 9]], got[[1, 4, 7, 9]])


def test_compare_joint_on_lock_step_posteriors_and_the_batch_is_one_operator_call(monkeypatch):
    import pyprob_amd
    from pyprob_amd import ops as P
    from pyprob_amd.distributions import TwoSampleJoint
    from test_gpu_density_joint import _two_statement_model
    model, M = _two_statement_model(), 3
    rng = np.random.default_rng(5)
    observes = [{'obs0': float(np.float32(rng.uniform(-2.0, 4.0))), 'obs1': float(np.float32(rng.uniform(-2.0, 4.0)))} for _ in range(M)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pa = model.posterior_results_batch(300, observes, seed=13, offset=64)
        pb = model.posterior_results_batch(2300, observes, seed=14, offset=64)
    loop = [a.compare_joint(b) for a, b in zip(pa, pb)]
    calls, real = [], P.ops.is_pairs_groups
    monkeypatch.setattr(P.ops, 'is_pairs_groups', lambda *args: calls.append(1) or real(*args), raising=False)
    fast = pyprob_amd.compare_joint_batch(pa, pb)
    assert len(calls) == 1 and len(fast) == M and isinstance(fast[0], TwoSampleJoint)
    fields = ('k_aa', 'k_bb', 'k_ab', 'd_aa', 'd_bb', 'd_ab', 'mmd2', 'mmd2_unbiased', 'mmd', 'energy', 'scale', 'center', 'ess')
    for f, l in zip(fast, loop):
        assert all(np.array_equal(np.float64(getattr(f, k)).view(np.int64), np.float64(getattr(l, k)).view(np.int64)) for k in fields)
        assert f.count == l.count == (300, 2300) and f.addresses == l.addresses and f.bandwidth == np.sqrt(2.0)
    assert len({f.mmd2 for f in fast}) == M and all(f.mmd2 > 0 and f.energy > 0 for f in fast)
    # one pair against the restatement and the host route on the same particles; a posterior against itself
    a, b, r = pa[0], pb[0], loop[0]
    particles = lambda p: (p._pair_columns(None)[1].cpu().numpy(), np.stack([c.cpu().numpy() for c in p._pair_columns(None)[2]], 1))  # noqa: E731
    (lw_a, x_a), (lw_b, x_b) = particles(a), particles(b)
    want, bound = _six_sums(lw_a, x_a, lw_b, x_b, r.center, 1.0 / r.scale, r.bandwidth)
    got = np.array([getattr(r, k) for k in NAMES])
    _record(dict(case='public 300 x 2300, J = 2', worst_ratio=dict(zip(NAMES, (np.abs(got - want[:6]) / bound).tolist()))))
    assert (np.abs(got - want[:6]) <= bound).all() and (bound < 1e-3 * want[:6]).all()
    monkeypatch.setenv('PP_EMPIRICAL_DEVICE', '0')
    host = a.compare_joint(b)
    monkeypatch.delenv('PP_EMPIRICAL_DEVICE')
    assert (np.abs(got - np.array([getattr(host, k) for k in NAMES])) <= bound).all() and host.count == r.count
    assert np.allclose(host.center, r.center, rtol=1e-9) and np.allclose(host.scale, r.scale, rtol=1e-9)
    same = a.compare_joint(a)
    _, own = _six_sums(lw_a, x_a, lw_a, x_a, same.center, 1.0 / same.scale, same.bandwidth)
    assert abs(same.mmd2) <= own[0] + own[1] + 2 * own[2] and abs(same.energy) <= own[3] + own[4] + 2 * own[5]
    drawn = b.compare_joint(a, num_samples=500, seed=3)
    assert drawn.count == (500, 500) and drawn.ess == pytest.approx((500.0, 500.0)) and drawn.mmd2 > 0 and drawn.energy > 0
