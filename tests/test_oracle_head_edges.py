"""The oracle's proposal heads at saturated outputs (tests/head_edge_cases.py) against the reference's float64 record
(tests/golden/head_edges.npz, written by tests/golden/make_head_edges_golden.py) and, where the reference tree exists, against
the live reference; and the yardstick of tests/test_gpu_head_edges.py: the error of the reference's own fp32 run.

Settled here: oracle.ic_oracle agrees with the reference's float64 run at the clamp to 1e-13 - on rows whose leading weight
lies above 1 - eps too, where both take log(1 - 2^-23). The float64 run keeps eps = finfo(float32).eps (the golden script's
docstring); a float64 run that lets util.clamp_probs pick finfo(float64).eps never clamps these weights and is not what an
fp32 computation is measured against.

On rescued rows (value outside the support, log_prob -inf replaced by log(1e-8)) the reference's autograd leaves NaN in dy
(0 x exp(-inf + inf) in the logsumexp's backward); the project defines dy = 0 there, as the oracle does, and the record is
read with zeros on those rows."""
import os

import numpy as np
import pytest

import head_edge_cases as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_edges.npz')
REFERENCE = '/root/reference'
ORACLE_TOL = 1e-10        # of scale: lp over max(1, |lp|), dy over the block's largest element
FP32_CAP = 1e-2           # no case may ask the device for less than this accuracy of the reference's own fp32 run


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _record(G, name, prec):
    lp = G['%s_lp%d' % (name, prec)].astype(np.float64)
    dy = G['%s_dy%d' % (name, prec)].astype(np.float64)
    resc = np.isneginf(lp)
    assert not (~np.isfinite(dy).all(1) & ~resc).any(), 'non-finite reference gradient on a row that is not rescued'
    return lp, np.where(resc[:, None], 0.0, dy)


def test_cases_cover_the_branches():
    """Each clamp branch and value kind is present where the GPU file's docstring says (head_edge_cases asserts the factor 2
    between every weight and both thresholds itself)."""
    cases = E.head_edge_cases()
    assert sorted(c['kind'] for c in cases.values() if c['name'].endswith('ordinary')) == [3, 4]
    for name, c in cases.items():
        p = E.weights(c)
        below, above = E.clamp_masks(p)
        assert E.weight_margin(p) >= 2.0
        if 'ordinary' in name:
            assert not below.any() and not above.any()
            continue
        if c['head'] == 'Bernoulli':
            assert below.any() and above.any() and (~below & ~above).any()
            assert {'n1_zero', 'n1_all', 'n1_between'} == set(c['tag'])
            assert np.abs(c['y']).max() >= 29.5
        elif c['head'] == 'Categorical':
            pv = p[np.arange(len(p)), c['value'].astype(np.int64)]
            assert (pv < E.EPS).any() and below.any()
            assert (pv > 1 - E.EPS).any() == (c['C'] == 2)      # 1 - p >= (C - 1) 1e-8 / (1 + C 1e-8): out of reach from C = 7 on
            assert {0.0, c['C'] - 1.0} <= set(c['value'])
        else:
            K = c['K']
            assert above.any() and (below.any() or K == 1)
            assert (below.any(1) & ~above.any(1)).any() or K == 1       # a weight below eps next to a leading one inside
            y = c['y']
            lim = {'Normal': (29.5, 5.5, 11.5), 'Uniform': (19.5, 19.5, 19.5), 'Poisson': (19.5, 3.9, 7.5)}[c['head']]
            if 'tt1000' not in name:
                assert y[:, :K].max() >= lim[0] and y[:, :K].min() <= -lim[0]
                assert y[:, K:2 * K].min() <= -lim[1] and y[:, K:2 * K].max() >= lim[2]
            if c['head'] != 'Normal' and 'tt1000' not in name:
                lo, hi, v = c['prior'][:, 0], c['prior'][:, 1], c['value']
                assert (v == lo).any() and (v == hi).any() and (v < lo).any() and (v > hi).any()
            if 'tt1000' in name:
                mu, sd = E.component_params(c['head'], y, c['prior'], K)
                tt = np.abs(c['value'][:, None] - mu) / sd           # one component (a leading one) sits 1000 scales away
                assert np.abs(tt - 1000).min(1).max() < 10


@pytest.mark.parametrize('name', sorted(E.head_edge_cases()))
def test_oracle_against_float64_record(golden, name):
    case = E.head_edge_cases()[name]
    for k in ('y', 'value', 'prior'):
        assert np.array_equal(golden[name + '_' + k], case[k].astype(np.float32)), 'head_edges.npz is stale'
    lp64, dy64 = _record(golden, name, 64)
    lp, dy = E.oracle_head(case)
    assert E.lp_error(lp, lp64) <= ORACLE_TOL       # (the -inf pattern - the rescued rows - is compared inside)
    for block, err in E.dy_errors(case, dy, dy64).items():
        assert err <= ORACLE_TOL, (name, block, err)
    resc = np.isneginf(lp64)
    assert np.all(dy[resc] == 0.0)
    if case['head'] in ('Uniform', 'Poisson') and 'tt1000' not in name:
        assert resc.any() and np.array_equal(resc, np.isin(case['tag'], ('below', 'above')))
    # the clamp masks: where every weight of a row is clamped the logits get no gradient at all, in the record as in the oracle
    p = E.weights(case)
    below, above = E.clamp_masks(p)
    sl = E.blocks(case)['logits']
    if case['head'] == 'Categorical':
        pv = p[np.arange(len(p)), case['value'].astype(np.int64)]
        out = (pv < E.EPS) | (pv > 1 - E.EPS)
        np.testing.assert_allclose(lp64[pv < E.EPS], np.log(E.EPS), rtol=1e-12)
        np.testing.assert_allclose(lp64[pv > 1 - E.EPS], np.log1p(-E.EPS), rtol=1e-9)
    else:
        out = (below | above).all(1)
    assert np.all(dy64[out][:, sl] == 0.0) and np.all(dy[out][:, sl] == 0.0)
    if case['head'] != 'Categorical' and 'ordinary' not in name:
        assert np.any(dy64[~out & ~resc][:, sl] != 0.0) or case.get('K') == 1 or case['head'] == 'Bernoulli'


@pytest.mark.parametrize('name', sorted(E.head_edge_cases()))
def test_reference_fp32_error_is_capped(golden, name):
    """The yardstick: per case and output block the fp32 record's error against float64 in the GPU file's metric. The cap is a
    condition on the inputs of tests/head_edge_cases.py (its scale floors), not on any kernel."""
    case = E.head_edge_cases()[name]
    lp64, dy64 = _record(golden, name, 64)
    lp32, dy32 = _record(golden, name, 32)
    errs = dict(lp=E.lp_error(lp32, lp64), **E.dy_errors(case, dy32, dy64))
    print(name, {k: '%.2e' % v for k, v in errs.items()})
    for block, err in errs.items():
        assert err <= FP32_CAP, (name, block, err)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, 'pyprob')), reason='the reference tree is not on this machine')
def test_oracle_against_live_reference(golden):
    """The same comparison against the reference run now, and the record against that run (the fixture is what the committed
    script writes)."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location('make_head_edges_golden', os.path.join(os.path.dirname(GOLDEN), 'make_head_edges_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import sys
    saved, saved_validate = list(sys.path), torch.distributions.Distribution._validate_args
    try:
        run = mod.reference_heads(REFERENCE)
        for name, case in E.head_edge_cases().items():
            lp_ref, dy_ref = run(case, torch.float64)
            assert np.array_equal(lp_ref, golden[name + '_lp64']) or np.allclose(lp_ref, golden[name + '_lp64'], rtol=1e-12, atol=0)
            resc = np.isneginf(lp_ref)
            dy_ref = np.where(resc[:, None], 0.0, dy_ref)
            lp, dy = E.oracle_head(case)
            assert E.lp_error(lp, lp_ref) <= ORACLE_TOL, name
            for block, err in E.dy_errors(case, dy, dy_ref).items():
                assert err <= ORACLE_TOL, (name, block, err)
            lp32, _ = run(case, torch.float32)
            assert np.array_equal(lp32, golden[name + '_lp32'], equal_nan=True), name
    finally:
        sys.path[:] = saved
        torch.distributions.Distribution.set_default_validate_args(saved_validate)
