"""Time of Empirical.density_estimate_joint and pyprob_amd.density_estimate_joint_batch (csrc/is_gmm_joint.hip) next to two other
routes to the same fit on the same machine, neither of which is the code under test:
    torch   the same weighted full-covariance EM (the definition of pp_is_gmm_joint_groups, same start, same stop rule) in torch
            float64 on the device: component by component (torch.linalg.cholesky, a product with the inverse factor), one .item()
            per iteration. Plain torch, not tuned: its fp64 products of [J, 10^6] by [10^6, J] matrices dominate it;
    cpu     cpu() of the log-weights and the J columns, then the float64 numpy route (empirical_host._host_gmm_joint) from the
            same start. One numpy iteration over 10^6 particles takes seconds, so this route is timed at --iterations iterations
            (tol = 0) over min(--reps, 3) runs after one, and compared per iteration.
The posteriors are built from synthetic columns (three correlated Gaussian modes) the way a lock-step call leaves them
(Empirical.from_device plus a statement log of whole columns; for the batch the call's whole tensors and its [M, 6] statistics).
Cases: (J, K) = (2, 3), (4, 8), (8, 16) on ONE group of --N particles (a fresh object per call: the sort behind the initial means and
the moments behind the initial covariances are part of the call), the operator alone at a fixed number of iterations (tol = 0: time
per EM iteration, 4 (J + 1) bytes read per particle and iteration), and density_estimate_joint_batch at --batch M N with J = 2,
K = 3 against the loop of single calls. Every device figure is the median of --reps device-event timings of ONE call after --warmup
calls. Writes one JSON document to profiles/density_joint_bench.json (--out PATH).

    python tools/density_joint_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
import argparse
import json
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyprob_amd  # noqa: E402
from pyprob_amd import lib as L  # noqa: E402
from pyprob_amd.distributions import Empirical  # noqa: E402
from pyprob_amd.empirical import _joint_gmm_init_rows, _joint_rows, _joint_start_means, _moment_rows  # noqa: E402
from pyprob_amd.empirical_host import _host_gmm_joint  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--iterations', type=int, default=4, help='EM iterations of the fixed-iteration rows (tol = 0)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'density_joint_bench.json'))
    return ap.parse_args()


args = _args()
DEV = 'cuda'
TOL, MAX_ITER, REG = 1e-3, 100, 1e-6


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


def columns(M, N, J, seed):
    """Three correlated modes per group (shifted from group to group) in J columns; log-weights of spread 1."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    comp = torch.multinomial(torch.tensor([0.3, 0.45, 0.25], device=DEV), M * N, True, generator=g).float()
    shift = (torch.arange(M, device=DEV).float() * 0.1).repeat_interleave(N)
    z = torch.randn(J, M * N, device=DEV, generator=g)
    cols = [(shift + 3.0 * comp * (1.0 - 0.1 * j) + 0.5 * z[j] + (0.35 * z[j - 1] * (comp - 1.0) if j else 0.0)).contiguous()
            for j in range(J)]
    return torch.randn(M * N, device=DEV, generator=g).contiguous(), cols


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, cols, stats_row):
    """An Empirical as a lock-step call leaves it: the last column is the value forward() returned, the log holds every column."""
    from pyprob_amd.is_engine import DistRunner
    p = Empirical.from_device(cols[-1], lw, DistRunner._stats_dict(stats_row))
    p.statement_log = [{'x%d' % j: (c,)} for j, c in enumerate(cols)]
    p._statement_rows = [{'x%d' % j: None} for j in range(len(cols))]
    return p


def start(lw, cols, n_per, stats, K):
    chosen = ['x%d' % j for j in range(len(cols))]
    return _joint_gmm_init_rows(K, len(cols), REG, None, None, None, lambda: _joint_start_means(lw, cols, n_per, stats, K),
                                lambda: [j.cov for j in _joint_rows(chosen, _moment_rows(lw, cols, n_per, stats))])


def torch_em(lw, cols, init, K, max_iter=MAX_ITER, tol=TOL):
    """The EM of pp_is_gmm_joint_groups for one group in torch float64 on the device: (pi, mu, cov, lower bound, n_iter)."""
    J = len(cols)
    x = torch.stack(cols, 1).double()
    l = lw.double()
    w = torch.exp(l - l.max())
    W = w.sum()
    iu = torch.triu_indices(J, J, device=lw.device)
    pi, mu = init[:K].clone(), init[K:K + K * J].view(K, J).clone()
    cov = torch.zeros(K, J, J, dtype=torch.float64, device=lw.device)
    cov[:, iu[0], iu[1]] = init[K + K * J:].view(K, -1)
    cov = torch.triu(cov) + torch.triu(cov, 1).transpose(1, 2)
    eye = torch.eye(J, dtype=torch.float64, device=lw.device)
    before, lb, t = -float('inf'), None, 0
    for t in range(1, max_iter + 1):
        F = torch.linalg.cholesky(cov)
        Fi = torch.linalg.inv(F)
        ell = torch.empty(K, x.shape[0], dtype=torch.float64, device=lw.device)
        for k in range(K):
            z = Fi[k] @ (x - mu[k]).T
            ell[k] = torch.log(pi[k]) - 0.5 * J * np.log(2.0 * np.pi) - torch.log(torch.diagonal(F[k])).sum() - 0.5 * (z * z).sum(0)
        Lse = torch.logsumexp(ell, 0)
        lb = float(((w * Lse).sum() / W).item())
        Nk = torch.empty(K, dtype=torch.float64, device=lw.device)
        new_mu, new_cov = torch.empty_like(mu), torch.empty_like(cov)
        for k in range(K):
            r = w * torch.exp(ell[k] - Lse)
            Nk[k] = r.sum() + 10.0 * np.finfo(np.float64).eps
            d = x - mu[k]
            rd = r[:, None] * d
            s = rd.sum(0) / Nk[k]
            new_mu[k] = mu[k] + s
            new_cov[k] = rd.T @ d / Nk[k] - torch.outer(s, s) + REG * eye
        pi, mu, cov = Nk / Nk.sum(), new_mu, new_cov
        if abs(lb - before) < tol:
            break
        before = lb
    return pi.cpu().numpy(), mu.cpu().numpy(), cov.cpu().numpy(), lb, t


def cpu_route(lw, cols, init, K, iterations):
    return _host_gmm_joint(lw.cpu().numpy(), np.stack([c.cpu().numpy() for c in cols]), init, K, iterations, 0.0, REG)


def operator_alone(lw, cols, K, n_per, stats, init, n_particles):
    its = max(args.iterations, 2)
    J = len(cols)
    alone = event_timed(lambda: ops.is_gmm_joint_groups(lw, cols, K, n_per, stats, init, its, 0.0, REG))
    one = event_timed(lambda: ops.is_gmm_joint_groups(lw, cols, K, n_per, stats, init, 1, 0.0, REG))
    per_iter = (alone['median_ms'] - one['median_ms']) / (its - 1)
    return dict(iterations=its, call=alone, one_iteration_call=one, ms_per_iteration=round(per_iter, 4),
                bytes_per_particle_and_iteration=4 * (J + 1),
                effective_GB_per_s=round(n_particles * 4 * (J + 1) / (per_iter * 1e-3) / 1e9, 1) if per_iter > 0 else None,
                particle_components_per_s=round(n_particles * K / (per_iter * 1e-3), 0) if per_iter > 0 else None)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('density_joint_bench: needs a ROCm device (nothing is measured without one)')
    warnings.simplefilter('ignore')
    records = []
    N, its = args.N, max(args.iterations, 2)
    for J, K in ((2, 3), (4, 8), (8, 16)):
        lw, cols = columns(1, N, J, 31 + J)
        row = group_stats(lw, cols[-1], 1, N)[0].cpu().numpy()
        fit = posterior(lw, cols, row).density_estimate_joint(K)
        init_host = start(lw, cols, N, None, K)
        init = torch.from_numpy(init_host).to(DEV)
        ref = torch_em(lw, cols, init[0], K)
        apart = float(max(np.abs(fit.weights / ref[0] - 1).max(), np.abs(fit.means - ref[1]).max(), np.abs(fit.covariances - ref[2]).max()))
        rec = dict(case='density_estimate_joint(%d) over %d addresses, fresh object: sort, moments, EM, one copy' % (K, J), M=1, N=N, J=J,
                   K=K, n_iter=fit.n_iter, converged=fit.converged, degenerate=fit.degenerate, torch_n_iter=ref[4],
                   max_difference_to_torch=apart,
                   ours=event_timed(lambda: posterior(lw, cols, row).density_estimate_joint(K)),
                   torch_float64_em=event_timed(lambda: torch_em(lw, cols, init[0], K), reps=min(args.reps, 5), warmup=1),
                   operator_alone=operator_alone(lw, cols, K, N, None, init, N))
        t_fixed = event_timed(lambda: torch_em(lw, cols, init[0], K, its, 0.0), reps=min(args.reps, 5), warmup=1)
        c_fixed = event_timed(lambda: cpu_route(lw, cols, init_host[0], K, its), reps=min(args.reps, 3), warmup=1)
        rec['torch_float64_em_fixed_iterations'] = dict(t_fixed, ms_per_iteration=round(t_fixed['median_ms'] / its, 4))
        rec['cpu_route_fixed_iterations'] = dict(c_fixed, ms_per_iteration=round(c_fixed['median_ms'] / its, 4))
        rec['torch_over_ours'] = round(rec['torch_float64_em']['median_ms'] / rec['ours']['median_ms'], 2)
        per = rec['operator_alone']['ms_per_iteration']
        rec['cpu_over_operator_per_iteration'] = round(rec['cpu_route_fixed_iterations']['ms_per_iteration'] / per, 1) if per > 0 else None
        print(json.dumps(rec), flush=True)
        records.append(rec)
    M, Nb = args.batch
    J, K = 2, 3
    lw, cols = columns(M, Nb, J, 7)
    stats = group_stats(lw, cols[-1], M, Nb)
    host_stats = stats.cpu().numpy()
    whole_log = [{'x%d' % j: (c,)} for j, c in enumerate(cols)]
    posts = []
    for g in range(M):
        sl = slice(g * Nb, (g + 1) * Nb)
        p = posterior(lw[sl], [c[sl] for c in cols], host_stats[g])
        p._batch, p._batch_log = (cols[-1], lw, stats, g, Nb), whole_log
        posts.append(p)
    fast = pyprob_amd.density_estimate_joint_batch(posts, K)
    loop = [p.density_estimate_joint(K) for p in posts]
    assert all(np.array_equal(a.means, b.means) and np.array_equal(a.covariances, b.covariances) and a.n_iter == b.n_iter
               for a, b in zip(fast, loop)), 'the batch must be bit-equal to the loop'
    iters = [f.n_iter for f in fast]
    init = torch.from_numpy(start(lw, cols, Nb, stats, K)).to(DEV)
    rec = dict(case='density_estimate_joint_batch(posts, 3) over 2 addresses', M=M, N=Nb, J=J, K=K, n_iter_min=min(iters),
               n_iter_max=max(iters), ours=event_timed(lambda: pyprob_amd.density_estimate_joint_batch(posts, K)),
               loop_of_single_calls=event_timed(lambda: [p.density_estimate_joint(K) for p in posts], reps=min(args.reps, 5), warmup=1),
               operator_alone=operator_alone(lw, cols, K, Nb, stats, init, M * Nb))
    rec['loop_over_ours'] = round(rec['loop_of_single_calls']['median_ms'] / rec['ours']['median_ms'], 2)
    print(json.dumps(rec), flush=True)
    records.append(rec)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, tol=TOL, max_iter=MAX_ITER, reg_covar=REG,
               check_every=os.environ.get('PP_GMM_CHECK', '8'),
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup; the torch '
                      'route over at most 5 runs after one, the cpu route over at most 3 after one',
               inputs='synthetic columns (three correlated Gaussian modes) and log-weights (normal), attached to Empiricals as a '
                      'lock-step call attaches them',
               ours='Empirical.density_estimate_joint / pyprob_amd.density_estimate_joint_batch: the particles at the quantiles of the '
                    'sorted first address and joint().cov for the start, pp_is_gmm_joint_groups (two launches per EM iteration, fp64), '
                    'one copy of the rows',
               torch_float64_em='the same EM, start and stop rule in torch float64 on the device, component by component',
               cpu_route='cpu() of the log-weights and the columns, then the float64 numpy route from the same start, --iterations '
                         'iterations at tol = 0',
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
