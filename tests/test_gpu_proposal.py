"""pp_is_proposal_groups (csrc/is_proposal.hip) and the proposal-IS route built on it, against the plain restatement of
tests/proposal_ref.py. The density is checked AT the float32 values the kernel returned, in numpy.longdouble: the bound per particle is
one float32 ulp of the value plus 16 times the error the float64 restatement itself shows. PP_PROPOSAL_ERRORS=<file> appends the worst
figures per case and the effective sample sizes of the end-to-end runs (profiles/proposal_errors.jsonl)."""
import json
import math
import os
import warnings

import numpy as np
import pytest

import proposal_ref as PR

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N_PER = 2500          # crosses a tile of 2048, no multiple of 64
SEED, OFFSET = 0x5EED5EED, 12345


def _record(rec):
    path = os.environ.get('PP_PROPOSAL_ERRORS')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(rec) + '\n')


def _fits(J, K):
    """Two groups with different fits; component 0 of group 1 is narrow (width 1e-3) and sits at 1000."""
    rng = np.random.default_rng(100 * J + K)
    a, b = PR.random_fit(rng, J, K), PR.random_fit(rng, J, K, center=-2.0, width=0.7)
    b[1][0], b[2][0] = 1000.0, b[2][0] * 1e-6
    return [a, b]


def _call(fits, n_per, cols=(), seed=SEED, offset=OFFSET):
    from pyprob_amd.ops import ops
    K, J = fits[0][1].shape
    rows = torch.from_numpy(np.stack([PR.fit_row(*f) for f in fits])).to(DEV)
    out, neg, status = ops.is_proposal_groups(rows, J, K, n_per, list(cols), seed, offset)
    return [c.cpu().numpy() for c in out], neg.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('J,K', [(1, 1), (2, 3), (3, 16), (8, 2), (8, 16)])
def test_density_at_the_returned_value_score_mode_and_counter_contract(J, K):
    fits = _fits(J, K)
    cols, neg, status = _call(fits, N_PER)
    assert status.tolist() == [0, 0] and all(np.isfinite(c).all() for c in cols) and np.isfinite(neg).all()
    x = np.stack(cols, 1)
    rec = dict(case='density', J=J, K=K)
    for g, f in enumerate(fits):
        xg, got = x[g * N_PER:(g + 1) * N_PER], neg[g * N_PER:(g + 1) * N_PER].astype(np.longdouble)
        refL = PR.neg_log_q(xg, *f, dtype=np.longdouble)
        e64 = np.abs(PR.neg_log_q(xg, *f, dtype=np.float64) - refL)
        ulp = np.spacing(np.abs(refL).astype(np.float32)).astype(np.longdouble)
        err = np.abs(got - refL)
        rec['group%d' % g] = dict(max_err_ulp32=float((err / ulp).max()), max_f64_restatement_err_ulp32=float((e64 / ulp).max()))
        assert (err <= ulp + 16 * e64).all(), rec
    assert (np.abs(x[N_PER:] - 1000.0) < 0.1).any()           # the narrow component was drawn from
    _record(rec)
    # score mode: the bits the draw wrote
    assert np.array_equal(_call(fits, N_PER, [torch.from_numpy(c).to(DEV) for c in cols])[1], neg)
    # the counter contract: a repeat; group 0 alone; the second half of group 0 by its offset
    again = _call(fits, N_PER)
    assert all(np.array_equal(a, c) for a, c in zip(again[0], cols)) and np.array_equal(again[1], neg)
    alone = _call(fits[:1], N_PER)
    assert all(np.array_equal(a, c[:N_PER]) for a, c in zip(alone[0], cols)) and np.array_equal(alone[1], neg[:N_PER])
    half = N_PER // 2
    tail = _call(fits[:1], N_PER - half, offset=OFFSET + half)
    assert all(np.array_equal(a, c[half:N_PER]) for a, c in zip(tail[0], cols)) and np.array_equal(tail[1], neg[half:N_PER])


def test_the_draw_is_the_distribution():
    """Mean and second moments within 6 standard errors of the analytic ones, and mean(p / q) = 1 for p = the same components under
    other weights rho: p / q <= R = max rho_k / pi_k, so Var(p / q) <= E_q (p / q)^2 - 1 <= R - 1 - a finite, analytic bound."""
    n, J, K = 200000, 3, 4
    w, means, covs = PR.random_fit(np.random.default_rng(7), J, K)
    cols, neg, _ = _call([(w, means, covs)], n)
    x = np.stack(cols, 1).astype(np.float64)
    m1, m2, v1, v2 = PR.moments(w, means, covs)
    assert (np.abs(x.mean(0) - m1) <= 6 * np.sqrt(v1 / n)).all()
    assert (np.abs(np.einsum('nj,nm->jm', x, x) / n - m2) <= 6 * np.sqrt(v2 / n)).all()
    rho = w[::-1].copy()
    R = ((rho / rho.sum()) / (w / w.sum())).max()
    ratio = np.exp(neg.astype(np.float64) - PR.neg_log_q(x, rho, means, covs))
    assert abs(ratio.mean() - 1.0) <= 6 * math.sqrt((R - 1.0) / n)
    # the numpy route of the host passes the same check (another stream of the same distribution)
    from pyprob_amd import JointMixtureFit
    fit = JointMixtureFit(['a', 'b', 'c'], w / w.sum(), means, covs, 0.0, 1, True, False, n, {})
    xh = fit.sample(n, seed=3)
    ratio = np.exp(-fit.log_prob(xh) - PR.neg_log_q(xh, rho, means, covs))
    assert abs(ratio.mean() - 1.0) <= 6 * math.sqrt((R - 1.0) / n)
    assert (np.abs(xh.mean(0) - m1) <= 6 * np.sqrt(v1 / n)).all()


def test_status_marks_the_group_that_is_no_density():
    fits = _fits(3, 4)
    good = _call(fits, N_PER)
    fits[1][2][2] = -fits[1][2][2]                            # component 2 of group 1: not positive definite
    cols, neg, status = _call(fits, N_PER)
    assert status.tolist() == [0, 3]
    assert np.isnan(neg[N_PER:]).all() and all(np.isnan(c[N_PER:]).all() for c in cols)
    assert np.array_equal(neg[:N_PER], good[1][:N_PER]) and all(np.array_equal(c[:N_PER], d[:N_PER]) for c, d in zip(cols, good[0]))


@pytest.mark.parametrize('program', ['A', 'B'])
def test_run_fit_run_again_from_the_fit(program):
    import pyprob_amd
    from pyprob_amd import InferenceEngine, Model
    from pyprob_amd import distributions as D

    class Program(Model):
        def forward(self):
            x1 = pyprob_amd.sample(D.Normal(0.0, 1.0))
            x2 = pyprob_amd.sample(D.Normal(x1, 1.0))
            pyprob_amd.observe(D.Normal(x2, 0.5), name='y')
            if program == 'B':
                u = pyprob_amd.sample(D.Uniform(0.0, 4.0))
                pyprob_amd.observe(D.Normal(x1 + u, 1.0), name='z')
            return x2

    n = 20000
    observe = {'y': 3.0, 'z': 3.5} if program == 'B' else {'y': 3.0}
    model = Program()
    prior = model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, observe=observe, lock_step=True, seed=11)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fit = prior.density_estimate_joint(2, addresses=prior.addresses[:2])
    post = model.posterior_results_from_proposal(n, fit, observe=observe, seed=12, offset=n)
    assert post.length == n and post.metadata['op'] == 'proposal_is'
    a1, a2 = fit.addresses
    log = post.statement_log
    x1, x2 = (log[j][a][0].double().cpu().numpy() for j, a in ((0, a1), (1, a2)))
    want = PR.normal_lp(x1, 0.0, 1.0) + PR.normal_lp(x2, x1, 1.0) + PR.normal_lp(3.0, x2, 0.5) + \
        PR.neg_log_q(np.stack([x1, x2], 1), fit.weights, fit.means, fit.covariances)
    if program == 'B':
        u = log[2][post.addresses[2]][0].double().cpu().numpy()
        assert ((u >= 0) & (u < 4)).all()
        want = want + PR.normal_lp(3.5, x1 + u, 1.0)
    lw = post._all_log_weights.double().cpu().numpy()
    assert np.abs(lw - want).max() <= 2e-4
    _record(dict(case='end to end', program=program, n=n, ess_prior=float(prior.effective_sample_size),
                 ess_proposal=float(post.effective_sample_size), max_lw_err=float(np.abs(lw - want).max())))
    assert post.effective_sample_size > prior.effective_sample_size
    if program == 'A':          # the conjugate posterior: x | y = 3 with Var y = 2.25
        for a, mean, var in ((a1, 3.0 / 2.25, 1.0 - 1.0 / 2.25), (a2, 6.0 / 2.25, 2.0 - 4.0 / 2.25)):
            assert abs(float(post.marginal(a).mean) - mean) <= 5 * math.sqrt(var / post.effective_sample_size)
    assert post.joint().count == n and np.isfinite(float(post.pareto_k()))
