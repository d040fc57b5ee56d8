"""The host side of proposal IS (csrc/is_proposal.hip, state.ProposalISState, Model.posterior_results_from_proposal): the C ABI's
exports and argument checks, the CPU-device route against a float64 re-score of the statement log, and the refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import proposal_ref as PR

torch = pytest.importorskip('torch')

GOOD = dict(fit=1, ld=12, M=1, J=2, K=2, n_per=10, mode=0, cols=8, neg=1, status=1, ws=1, ws_bytes=1 << 20)
A1, A2 = 'x1__Normal__1', 'x2__Normal__1'


def _c_call(**change):
    """pp_is_proposal_groups on HOST addresses: only for calls that return before a launch."""
    from pyprob_amd import lib as L
    lib, a = L.load(), dict(GOOD, **change)
    buf = (C.c_double * 64)()
    at = C.addressof(buf)
    cols = C.cast((C.c_void_p * 8)(*([at] * a['cols'])), C.c_void_p) if a['cols'] is not None else None
    rc = lib.pp_is_proposal_groups(at if a['fit'] else None, a['ld'], a['M'], a['J'], a['K'], a['n_per'], a['mode'], 1, 0, cols,
                                   at if a['neg'] else None, at if a['status'] else None, at if a['ws'] else None, a['ws_bytes'], None)
    return rc, lib.pp_last_error()


def test_symbols_are_exported_prototyped_and_declared():
    from pyprob_amd import lib as L
    lib = L.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pyprob_amd.h')).read()
    for name in ('pp_is_proposal_workspace_bytes', 'pp_is_proposal_groups'):
        assert name in L.PROTOTYPES and hasattr(lib, name) and name + '(' in header
    assert lib.pp_abi_version() == 15 and L.PP_ABI_VERSION == 15
    assert lib.pp_is_proposal_workspace_bytes(2, 8, 16) >= 2 * 1313 * 8
    assert [lib.pp_is_proposal_workspace_bytes(*a) for a in ((-1, 2, 2), (1, 0, 2), (1, 9, 2), (1, 2, 0), (1, 2, 17))] == [0] * 5
    assert _c_call(M=0)[0] == 0 and _c_call(n_per=0)[0] == 0            # nothing to do: 0 without a launch


@pytest.mark.parametrize('change', [dict(J=0), dict(J=9), dict(K=0), dict(K=17), dict(fit=0), dict(cols=1), dict(cols=None),
                                    dict(neg=0), dict(status=0), dict(ws=0), dict(mode=2), dict(mode=-1), dict(ws_bytes=64),
                                    dict(n_per=-1), dict(M=-1), dict(ld=11)])
def test_argument_errors_are_rejected_before_any_launch(change):
    rc, message = _c_call(**change)
    assert rc == -1 and b'pp_is_proposal_groups' in message            # PP_EINVAL


def _fit(addresses, covs=None):
    from pyprob_amd import JointMixtureFit
    covs = np.array([[[0.6, 0.2], [0.2, 0.3]], [[0.5, 0.1], [0.1, 0.4]]]) if covs is None else covs
    return JointMixtureFit(addresses, np.array([0.6, 0.4]), np.array([[1.2, 2.5], [1.6, 2.9]]), covs, 0.0, 1, True, False, 1, {})


def _program(branch=False):
    import pyprob_amd
    from pyprob_amd import Model
    from pyprob_amd import distributions as D

    class Program(Model):
        def forward(self):
            x1 = pyprob_amd.sample(D.Normal(0.0, 1.0), address='x1')
            if branch and x1 > 1.4:
                x2 = pyprob_amd.sample(D.Normal(x1, 2.0), address='x2')
            else:
                x2 = pyprob_amd.sample(D.Normal(x1, 1.0), address='x2')
            pyprob_amd.observe(D.Normal(x2, 0.5), name='y')
            return x2
    return Program()


@pytest.fixture
def cpu_doubles():
    import oracle_ops
    from test_dist_families import _register_dist_cpu_doubles
    oracle_ops.register()
    _register_dist_cpu_doubles()


def test_cpu_route_matches_the_float64_rescore_of_the_statement_log(cpu_doubles):
    fit, n = _fit([A1, A2]), 4000
    post = _program().posterior_results_from_proposal(n, fit, observe={'y': 3.0}, seed=5, device='cpu')
    assert post.length == n and post.metadata['op'] == 'proposal_is' and post.num_paths == 1
    x1, x2 = (post.statement_log[j][a][0].double().numpy() for j, a in ((0, A1), (1, A2)))
    want = PR.normal_lp(x1, 0.0, 1.0) + PR.normal_lp(x2, x1, 1.0) + PR.normal_lp(3.0, x2, 0.5) + \
        PR.neg_log_q(np.stack([x1, x2], 1), fit.weights, fit.means, fit.covariances)
    lw = post._all_log_weights.double().numpy()
    assert np.abs(lw - want).max() <= 2e-4
    w = np.exp(lw - lw.max())
    ess = w.sum() ** 2 / (w * w).sum()
    assert ess > n / 4          # (the prior's is ~ n / 14 at y = 3: this proposal sits on the posterior)
    assert abs((w * x2).sum() / w.sum() - 6.0 / 2.25) <= 5 * math.sqrt((2.0 - 4.0 / 2.25) / ess)      # the conjugate posterior mean


def test_refusals(cpu_doubles):
    from pyprob_amd import distributions as D
    from pyprob_amd import state
    fit, run = _fit([A1, A2]), dict(observe={'y': 3.0}, seed=2, device='cpu')
    with pytest.raises(NotImplementedError, match='inside a branch'):
        _program(branch=True).posterior_results_from_proposal(256, fit, **run)
    with pytest.raises(RuntimeError, match='never reached'):
        _program().posterior_results_from_proposal(64, _fit([A1, 'nowhere__Normal__1']), **run)
    bad = fit.covariances.copy()
    bad[1] = [[1.0, 2.0], [2.0, 1.0]]
    with pytest.raises(ValueError, match='component 1'):
        _program().posterior_results_from_proposal(64, _fit([A1, A2], bad), **run)
    # reached twice, and a family without a device term: a statement executes once per trace, so these are met at the state
    ls = state.ProposalISState(_program()._prior_is_runner_on('cpu'), 16, 3, 0, fit)
    ls.prior_statement(A1, D.Normal(0.0, 1.0))
    with pytest.raises(NotImplementedError, match='reached twice'):
        ls.prior_statement(A1, D.Normal(0.0, 1.0))
    with pytest.raises(NotImplementedError, match='no device log-density'):
        ls.prior_statement(A2, D.Factor(log_prob=0.0))
