"""The term matrix of tests/test_gpu_is_fused_kernel.py without a device: the generator (tests/helpers.py), its flag handling
and the out-of-support bookkeeping of the float64 reference, run through the CPU stand-ins of the operators
(`pyprob_hip::is_fused`, `pyprob_hip::logweight_terms`: tests/oracle_ops.py) with the very check the device test applies."""
import numpy as np
import pytest

import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from helpers import (FUSED_PLANT_MIN_N, check_fused_terms, fused_mixed_sets, fused_single_term_cases, fused_term_refs, fused_values,
                     is_engine)


@pytest.fixture(scope='module')
def run():
    return is_engine(32, seed=1, device='cpu')[1]


@pytest.mark.parametrize('n', [1, 300])
def test_single_term_matrix_through_the_stand_in_operators(run, n):
    rng = np.random.default_rng(n)
    value = fused_values(n, rng)
    cases = fused_single_term_cases(n, rng, value)
    assert {t['kind'] for t in cases} == set(range(6))
    assert {t['flags'] for t in cases if t['kind'] == 0} == set(range(8))
    assert {t['flags'] for t in cases if t['kind'] == 1} == {0, 1, 2, 4, 5, 6}
    assert all({t['flags'] for t in cases if t['kind'] == k} == {0, 4} for k in (2, 3, 4, 5))
    assert {t['scale'] < 0 for t in cases} == {True, False} and any(abs(abs(t['scale']) - 1.0) > 0.1 for t in cases)
    for kind in (0, 1, 3, 4, 5):      # parameters shared and per particle, x shared and per particle
        assert {(t['s0'] != 0, t['x'] is not None and t['x'].size == n) for t in cases if t['kind'] == kind and not t['flags']} >= \
            ({(False, True), (True, True)} if n == 1 else {(False, False), (False, True), (True, False), (True, True)})
    for t in cases:
        check_fused_terms(run, [t], value, rng)
    if n >= FUSED_PLANT_MIN_N:
        planted = [t for t in cases if t['out'].any() and not t['out'].all()]
        assert {t['kind'] for t in planted} == {1, 5}
        # x == low is inside, x == high is outside: the two particles sit next to each other in a planted Uniform term
        t = [t for t in planted if t['kind'] == 1 and t['flags'] == 0 and t['x'].size == n][0]
        i = int(np.nonzero(t['out'])[0][0])
        assert t['x'][i] == np.broadcast_to(t['p1'], n)[i] and t['x'][i - 1] == np.broadcast_to(t['p0'], n)[i - 1] and not t['out'][i - 1]


@pytest.mark.parametrize('n', [1, 300])
def test_eight_term_calls_through_the_stand_in_operators(run, n):
    rng = np.random.default_rng(7 + n)
    value = fused_values(n, rng)
    sets = fused_mixed_sets(n, rng, value)
    assert all(len(terms) == 8 for terms in sets.values())
    for name, terms in sets.items():
        check_fused_terms(run, terms, value, rng, label=name)
    # the seven shared Normal / identity terms are the same numbers in the all-LEAN and in the general sets
    a, b = fused_term_refs(sets['lean'][:7], value), fused_term_refs(sets['general_poisson'][:7], value)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    if n >= FUSED_PLANT_MIN_N:
        refs = fused_term_refs(sets['all_kinds'], value)
        assert sum(np.isneginf(r).any() for r in refs) == 3 and not np.logical_and.reduce([np.isneginf(r) for r in refs if np.isneginf(r).any()]).any()
