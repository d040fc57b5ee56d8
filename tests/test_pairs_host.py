"""Empirical.compare_joint on the chunked float64 numpy route (empirical_host._host_twosample_joint) against a plain double loop and
closed forms, and its refusals. Fails on the parent commit: the method does not exist there."""
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from pyprob_amd import compare_joint_batch                          # noqa: E402
from pyprob_amd.distributions import Empirical, TwoSampleJoint     # noqa: E402
from pyprob_amd.empirical_host import _host_twosample_joint         # noqa: E402


def _emp(x, lw=None):
    return Empirical(values=[np.asarray(v, np.float64) for v in x], log_weights=None if lw is None else [float(v) for v in lw])


@pytest.mark.parametrize('na,nb,J', [(1, 1, 1), (7, 40, 2), (40, 13, 8)])
def test_host_route_against_a_double_loop(na, nb, J):
    rng = np.random.default_rng(na + J)
    xa, xb = rng.normal(0.0, 1.0, (na, J)), rng.normal(0.5, 2.0, (nb, J))
    la, lb = -3.0 * rng.random(na), -3.0 * rng.random(nb)
    if na > 2:
        la[1], xa[2, 0] = -np.inf, np.nan          # both dropped; the NaN needs scale= (the moments of that side are NaN)
    scale = np.full(J, 1.5)
    with pytest.raises(ValueError) if na > 2 else np.errstate():
        _host_twosample_joint(la, xa, lb, xb)
    center = np.zeros(J) if na > 2 else None
    row, c, s, h = _host_twosample_joint(la, np.nan_to_num(xa) if na > 2 else xa, lb, xb, 0.7, scale, chunk=5)
    keep = np.isfinite(la)
    za, zb, wa, wb = (np.nan_to_num(xa)[keep] - c) / s, (xb - c) / s, np.exp(la[keep]) / np.exp(la[keep]).sum(), np.exp(lb) / np.exp(lb).sum()
    want = np.zeros(6)
    for p, (zr, wr, zc, wc) in enumerate(((za, wa, za, wa), (zb, wb, zb, wb), (za, wa, zb, wb))):
        for i in range(len(wr)):
            for j in range(len(wc)):
                d = math.sqrt(sum((zr[i] - zc[j]) ** 2))
                want[p] += wr[i] * wc[j] * math.exp(-d * d / (2 * 0.7 ** 2))
                want[3 + p] += wr[i] * wc[j] * d
    assert h == 0.7 and center is None or np.array_equal(s, scale)
    assert np.allclose(row[:6], want, rtol=1e-12, atol=1e-15) and (row[8], row[9]) == (keep.sum(), nb)
    assert row[6] == pytest.approx((wa * wa).sum(), rel=1e-12) and row[7] == pytest.approx((wb * wb).sum(), rel=1e-12)


def test_two_point_masses_and_a_set_against_itself():
    r = _emp([[0.0, 0.0]]).compare_joint(_emp([[1.0, 2.0]]), bandwidth=1.0)
    assert isinstance(r, TwoSampleJoint) and list(r.center) == [0.5, 1.0] and list(r.scale) == [0.5, 1.0] and r.addresses == [0, 1]
    assert (r.k_aa, r.k_bb, r.d_aa, r.d_bb, r.count, r.ess) == (1, 1, 0, 0, (1, 1), (1, 1))          # z = (-1, -1) and (1, 1)
    assert r.k_ab == pytest.approx(math.exp(-4.0)) and r.mmd2 == pytest.approx(2 - 2 * math.exp(-4.0)) and r.mmd == math.sqrt(r.mmd2)
    assert r.energy == pytest.approx(2 * math.sqrt(8.0)) and math.isnan(r.mmd2_unbiased)
    x = np.random.default_rng(0).normal(size=(30, 3))
    same = _emp(x).compare_joint(_emp(x))
    assert same.bandwidth == math.sqrt(3.0) and abs(same.mmd2) < 1e-15 and abs(same.energy) < 1e-14 and same.mmd2_unbiased < 0
    assert vars(compare_joint_batch([_emp(x)], [_emp(x + 1.0)])[0]).keys() == vars(same).keys()


def test_refusals():
    x = np.random.default_rng(1).normal(size=(6, 9))
    a = _emp(x)
    for kw in (dict(addresses=[]), dict(), dict(addresses=[0, 1], bandwidth=0.0), dict(addresses=[0, 1], bandwidth=-1.0),
               dict(addresses=[0, 1], scale=[1.0, 0.0]), dict(addresses=[0, 1], scale=[1.0]), dict(addresses=[0], num_samples=4)):
        with pytest.raises(ValueError):
            a.compare_joint(a, **kw)
    with pytest.raises(ValueError, match='scale='):          # no spread on either side
        _emp([[1.0, 2.0], [1.0, 3.0]]).compare_joint(_emp([[1.0, 5.0]]))
    with pytest.raises(AttributeError):                      # scalars and no statement log: as joint()
        Empirical(values=[1.0, 2.0]).compare_joint(a)
    with pytest.raises(TypeError):
        a.compare_joint([1.0])
    with pytest.raises(ValueError):
        compare_joint_batch([a], [])
    # a statement log with a branch: the address only some particles executed raises joint()'s error
    post = Empirical(values=[0.0, 1.0, 2.0])
    post.statement_log = [{'a': (torch.tensor([0.0, 1.0, 2.0]),)}, {'b': (torch.tensor([1.0, 0.0, 3.0]),)}]
    post._statement_rows_raw = [{'a': None}, {'b': [torch.tensor([0, 2])]}]
    with pytest.raises(ValueError, match='branch'):
        post.compare_joint(post, addresses=['a', 'b'])
    assert post.compare_joint(post).addresses == ['a'] and post.compare_joint(post, scale=[1.0]).mmd2 == 0
