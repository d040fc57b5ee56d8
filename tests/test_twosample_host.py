"""Empirical.compare on the float64 numpy route (empirical_host._host_twosample) against closed forms."""
import numpy as np
import pytest

from pyprob_amd import compare_batch
from pyprob_amd.distributions import Empirical, TwoSample
from pyprob_amd.empirical_host import _kolmogorov_sf


def _emp(values, weights=None):
    return Empirical(values=[float(v) for v in values], weights=weights)


def test_point_masses_at_zero_and_one():
    r = _emp([0.0]).compare(_emp([1.0]))
    assert isinstance(r, TwoSample)
    assert (r.ks, r.ks_location, r.wasserstein1, r.wasserstein2, r.energy, r.count, r.ess) == (1, 0, 1, 1, 2, (1, 1), (1, 1))
    assert r.ks_pvalue == _kolmogorov_sf(np.sqrt(0.5))


@pytest.mark.parametrize('c', [0.5, -3.0])
def test_a_shifted_copy_is_at_wasserstein_distance_of_the_shift(c):
    x = np.random.default_rng(1).integers(-50, 50, 400) / 8.0      # (a grid of eighths: every difference is exact)
    w = np.random.default_rng(2).integers(1, 9, 400) / 8.0
    r = _emp(x, w).compare(_emp(x + c, w))
    assert abs(r.wasserstein1 - abs(c)) <= 1e-13 and abs(r.wasserstein2 - abs(c)) <= 1e-13 and 0 < r.ks <= 1
    same = _emp(x, w).compare(_emp(x, w))
    assert (same.ks, same.wasserstein1, same.wasserstein2, same.energy, same.ks_pvalue) == (0, 0, 0, 0, 1)


def test_a_doubled_weight_is_the_particle_repeated():
    other = _emp([0.25, 1.5, 2.0, 7.0])
    weighted = _emp([1.0, 2.0, 3.0], [2.0, 1.0, 1.0]).compare(other)
    repeated = _emp([1.0, 1.0, 2.0, 3.0]).compare(other)
    for k in ('ks', 'ks_location', 'wasserstein1', 'wasserstein2', 'energy'):
        assert abs(getattr(weighted, k) - getattr(repeated, k)) <= 1e-15, k
    assert weighted.ks == 0.25 and weighted.ks_location == 0.25 and weighted.count == (3, 4) and repeated.count == (4, 4)
    assert [vars(t) for t in compare_batch([_emp([1.0, 1.0, 2.0, 3.0])], [other])] == [vars(repeated)]


def test_the_kolmogorov_series_and_the_refusals():
    assert abs(_kolmogorov_sf(1.0) - 0.26999967167735456) <= 1e-15 and _kolmogorov_sf(0.0) == 1 and _kolmogorov_sf(0.05) == 1
    assert abs(_kolmogorov_sf(1.18) - _kolmogorov_sf(1.18 - 1e-9)) <= 1e-8 and _kolmogorov_sf(9.0) < 1e-60
    assert 'asymptotic' in TwoSample.__doc__.lower() and 'ess' in TwoSample.__doc__.lower()
    with pytest.raises(ValueError):
        _emp([1.0]).compare(Empirical().finalize())
    with pytest.raises(ValueError):
        _emp([1.0]).compare(Empirical(values=[np.zeros(2), np.ones(2)]))
    with pytest.raises(TypeError):
        _emp([1.0]).compare([1.0])
    with pytest.raises(ValueError):
        compare_batch([_emp([1.0])], [])
