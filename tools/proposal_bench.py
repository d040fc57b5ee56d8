"""Time of pp_is_proposal_groups (csrc/is_proposal.hip) and of Model.posterior_results_from_proposal next to three other routes:
    operator  the draw + log-density of N particles of one fitted mixture, and the score mode alone, for (J, K) = (2, 3), (4, 8), (8, 16)
    torch     the same draw + log-density in torch float64 on the device (multinomial, randn, a batched triangular solve per component)
    cpu       JointMixtureFit.sample + log_prob in float64 numpy, and the copy of the result to the device
    call      posterior_results_from_proposal against posterior_results(IMPORTANCE_SAMPLING, lock_step=True) - the prior as the
              proposal - on the two-latent program of tests/test_gpu_proposal.py at the same N, with both effective sample sizes
Device events around one call, medians of --reps after --warmup. Writes profiles/proposal_bench.json. Nothing here asserts a time."""
import argparse
import json
import math
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import InferenceEngine, JointMixtureFit, Model  # noqa: E402
from pyprob_amd import distributions as D  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'proposal_bench.json'))
    return ap.parse_args()


args = _args()
DEV = 'cuda'


def event_timed(fn, reps=None, warmup=None):
    """Median, minimum and maximum over event pairs around ONE call of fn, in ms, after the warm-up calls."""
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    ts = []
    for _ in range(args.reps if reps is None else reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def wall_timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def mixture(J, K, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(K, J, J))
    w = rng.uniform(0.5, 2.0, K)
    return JointMixtureFit(['x%d' % j for j in range(J)], w / w.sum(), 3.0 * rng.normal(size=(K, J)),
                           a @ a.transpose(0, 2, 1) / J + 0.5 * np.eye(J), 0.0, 1, True, False, 1, {})


def torch_route(fit, n):
    """Draw + log q in torch float64 on the device."""
    w, mu = torch.from_numpy(fit.weights).to(DEV), torch.from_numpy(fit.means).to(DEV)
    L = torch.linalg.cholesky(torch.from_numpy(fit.covariances).to(DEV))
    K, J = mu.shape
    c = torch.log(w) - 0.5 * J * math.log(2 * math.pi) - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)

    def run():
        k = torch.multinomial(w, n, True)
        z = torch.randn(n, J, dtype=torch.float64, device=DEV)
        x = (mu[k] + torch.einsum('nij,nj->ni', L[k], z)).float()
        d = (x.double()[None] - mu[:, None]).transpose(1, 2)                       # [K, J, n]
        y = torch.linalg.solve_triangular(L, d, upper=False)
        return x, torch.logsumexp(c[:, None] - 0.5 * (y * y).sum(1), 0).float()
    return run


def operator_rows():
    rows = []
    for J, K in ((2, 3), (4, 8), (8, 16)):
        fit, n = mixture(J, K, 10 * J + K), args.N
        row = fit.fit_row(DEV)
        cols = ops.is_proposal_groups(row, J, K, n, [], 1, 0)[0]
        rec = dict(J=J, K=K, N=n,
                   operator_draw=event_timed(lambda: ops.is_proposal_groups(row, J, K, n, [], 1, 0)),
                   operator_score=event_timed(lambda: ops.is_proposal_groups(row, J, K, n, list(cols), 0, 0)),
                   sample_device=event_timed(lambda: fit.sample_device(n, seed=1)),
                   torch_float64=event_timed(torch_route(fit, n)))

        def cpu():
            x = fit.sample(n, seed=1)
            return torch.from_numpy(x.astype(np.float32)).to(DEV), torch.from_numpy(fit.log_prob(x).astype(np.float32)).to(DEV)
        rec['numpy_and_copy'] = wall_timed(cpu, reps=3)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    return rows


class Program(Model):
    def forward(self):
        x1 = pyprob_amd.sample(D.Normal(0.0, 1.0))
        x2 = pyprob_amd.sample(D.Normal(x1, 1.0))
        pyprob_amd.observe(D.Normal(x2, 0.5), name='y')
        return x2


def call_rows():
    model, n, obs = Program(), args.N, {'y': 3.0}
    prior = model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, observe=obs, lock_step=True, seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fit = prior.density_estimate_joint(2)
    post = model.posterior_results_from_proposal(n, fit, observe=obs, seed=2)
    rec = dict(N=n, ess_prior=float(prior.effective_sample_size), ess_proposal=float(post.effective_sample_size),
               prior_lock_step=event_timed(lambda: model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING, observe=obs,
                                                                           lock_step=True, seed=1)),
               from_proposal=event_timed(lambda: model.posterior_results_from_proposal(n, fit, observe=obs, seed=2)))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, operator=operator_rows(), call=call_rows())
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
