"""Time of Empirical.density_estimate and pyprob_amd.density_estimate_batch (csrc/is_gmm.hip) next to two other routes to a mixture
fit on the same machine, neither of which is the code under test:
    torch   the same weighted EM (the definition of pp_is_gmm_groups, same start, same stop rule) written in torch float64 on the
            device: [M, N, K] arrays, one .item() per iteration for the stop;
    cpu     what the reference does: cpu() of the log-weights and the values, 1000 values resampled by the weights, and
            scikit-learn's GaussianMixture(covariance_type='diag') on those (where scikit-learn is absent: the float64 numpy EM on
            the 1000 values, and the document says so). It fits 1000 unweighted draws, not the particles: another estimator.
The posteriors are built from synthetic columns (three Gaussian modes) the way a lock-step call leaves them (Empirical.from_device;
for the batch the call's whole tensors and its [M, 6] statistics). Cases: K = 1, 3 and 16 on ONE group of --N particles (a fresh
object per call: the sort behind the initial means is part of the call), density_estimate_batch at --batch M N with K = 3 against
the loop of single calls, and the operator alone at a fixed number of iterations (tol = 0): time per EM iteration and the bytes per
second it reads (8 bytes per particle and iteration: lw and x). Every figure is the median of --reps device-event timings of ONE
call after --warmup calls. Writes one JSON document to profiles/density_bench.json (--out PATH).

    python tools/density_bench.py [--reps 20] [--warmup 3] [--N 1000000] [--batch 256 10000]"""
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
from pyprob_amd.empirical_host import _host_gmm  # noqa: E402
from pyprob_amd.ops import ops  # noqa: E402

try:
    from sklearn.mixture import GaussianMixture
except ImportError:      # (the cpu route then runs the numpy EM on the resampled values)
    GaussianMixture = None


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=10 ** 6)
    ap.add_argument('--batch', type=int, nargs=2, default=[256, 10 ** 4], metavar=('M', 'N'))
    ap.add_argument('--iterations', type=int, default=10, help='EM iterations of the operator-alone rows (tol = 0)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'density_bench.json'))
    return ap.parse_args()


args = _args()
DEV = 'cuda'
TOL, MAX_ITER, REG = 1e-3, 100, 1e-6


def event_timed(fn, per=1):
    """Median, minimum and maximum over --reps event pairs around `per` calls of fn, in ms per call, after --warmup calls."""
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / per)
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def columns(M, N, seed):
    """Three modes (weights 0.3, 0.45, 0.25) per group, shifted from group to group; log-weights of spread 1."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    comp = torch.multinomial(torch.tensor([0.3, 0.45, 0.25], device=DEV), M * N, True, generator=g).float()
    shift = (torch.arange(M, device=DEV).float() * 0.1).repeat_interleave(N)
    x = shift + 3.0 * comp + torch.randn(M * N, device=DEV, generator=g) * (0.5 + 0.2 * comp)
    lw = torch.randn(M * N, device=DEV, generator=g)
    return lw.contiguous(), x.contiguous()


def group_stats(lw, x, M, N):
    scratch = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=DEV)
    return torch.stack([ops.is_stats(lw[g * N:(g + 1) * N], x[g * N:(g + 1) * N], scratch)[:6] for g in range(M)]).contiguous()


def posterior(lw, x, stats_row):
    from pyprob_amd.is_engine import DistRunner
    return Empirical.from_device(x, lw, DistRunner._stats_dict(stats_row))


# ---- the two other routes ---------------------------------------------------------------------------------------------------
def torch_em(lw, x, M, N, init, max_iter=MAX_ITER, tol=TOL):
    """The EM of pp_is_gmm_groups in torch float64 on the device, all groups until every one has stopped; rows [M, 3 K + 3]."""
    K = init.shape[1] // 3
    l, xs = lw.view(M, N).double(), x.view(M, N).double()
    w = torch.exp(l - l.max(1, keepdim=True)[0])
    W = w.sum(1)
    pi, mu, v = (init[:, j * K:(j + 1) * K].clone() for j in range(3))
    before = torch.full((M,), -float('inf'), dtype=torch.float64, device=lw.device)
    done = torch.zeros(M, dtype=torch.bool, device=lw.device)
    n_iter = torch.zeros(M, dtype=torch.float64, device=lw.device)
    lb = before.clone()
    for t in range(1, max_iter + 1):
        d = xs[:, :, None] - mu[:, None, :]
        ell = (torch.log(pi) - 0.5 * torch.log(2.0 * np.pi * v))[:, None, :] - d * d / (2.0 * v[:, None, :])
        Lse = torch.logsumexp(ell, 2)
        r = w[:, :, None] * torch.exp(ell - Lse[:, :, None])
        new_lb = (w * Lse).sum(1) / W
        Nk = r.sum(1) + 10.0 * np.finfo(np.float64).eps
        dk = (r * d).sum(1) / Nk
        live = ~done
        mu = torch.where(live[:, None], mu + dk, mu)
        v = torch.where(live[:, None], ((r * d * d).sum(1) / Nk - dk * dk).clamp(min=0.0) + REG, v)
        pi = torch.where(live[:, None], Nk / Nk.sum(1, keepdim=True), pi)
        lb = torch.where(live, new_lb, lb)
        n_iter = torch.where(live, torch.full_like(n_iter, t), n_iter)
        done = done | ((new_lb - before).abs() < tol)
        before = torch.where(live, new_lb, before)
        if bool(done.all().item()):
            break
    return torch.cat([pi, mu, v, lb[:, None], n_iter[:, None], done.double()[:, None]], 1).cpu().numpy()


def cpu_reference_route(lw, x, M, N, K, rng):
    """cpu() + 1000 values resampled by the weights + scikit-learn (the reference's density_estimate), group by group."""
    l, v = lw.cpu().numpy().reshape(M, N).astype(np.float64), x.cpu().numpy().reshape(M, N).astype(np.float64)
    out = []
    for g in range(M):
        w = np.exp(l[g] - l[g].max())
        draws = v[g][rng.choice(N, 1000, p=w / w.sum())]
        if GaussianMixture is not None:
            m = GaussianMixture(n_components=K, covariance_type='diag').fit(draws.reshape(-1, 1))
            out.append((m.weights_, m.means_[:, 0], m.covariances_[:, 0]))
        else:
            start = np.concatenate([np.full(K, 1.0 / K), np.quantile(draws, (np.arange(K) + 0.5) / K), np.full(K, draws.var() / K ** 2 + REG)])
            row = _host_gmm(np.zeros(1000), draws, start, MAX_ITER, TOL, REG)
            out.append((row[:K], row[K:2 * K], row[2 * K:3 * K]))
    return out


def default_init(posts, K):
    qs = (np.arange(K) + 0.5) / K
    rows = [np.concatenate([np.full(K, 1.0 / K), p.quantile(qs), np.full(K, p.variance / K ** 2 + REG)]) for p in posts]
    return torch.from_numpy(np.stack(rows)).to(DEV)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('density_bench: needs a ROCm device (nothing is measured without one)')
    warnings.simplefilter('ignore')
    rng = np.random.default_rng(0)
    records = []
    N = args.N
    lw, x = columns(1, N, 31)
    row = group_stats(lw, x, 1, N)[0].cpu().numpy()
    for K in (1, 3, 16):
        post = posterior(lw, x, row)
        fit = post.density_estimate(K).fit
        init = default_init([post], K)
        ref = torch_em(lw, x, 1, N, init)[0]
        apart = float(np.abs(np.concatenate([fit.weights, fit.means, fit.stddevs ** 2]) / ref[:3 * K] - 1).max())
        rec = dict(case='density_estimate(%d), fresh object: sort, quantiles, EM, one copy' % K, M=1, N=N, K=K, n_iter=fit.n_iter,
                   converged=fit.converged, torch_n_iter=int(ref[3 * K + 1]), max_relative_difference_to_torch=apart,
                   ours=event_timed(lambda: posterior(lw, x, row).density_estimate(K)),
                   ours_object_already_sorted=event_timed(lambda: post.density_estimate(K)),
                   torch_float64_em=event_timed(lambda: torch_em(lw, x, 1, N, init)),
                   cpu_reference_route=event_timed(lambda: cpu_reference_route(lw, x, 1, N, K, rng)))
        its = args.iterations
        alone = event_timed(lambda: ops.is_gmm_groups(lw, x, K, N, None, init, its, 0.0, REG))
        one = event_timed(lambda: ops.is_gmm_groups(lw, x, K, N, None, init, 1, 0.0, REG))
        per_iter = (alone['median_ms'] - one['median_ms']) / (its - 1)
        rec['operator_alone'] = dict(iterations=its, call=alone, one_iteration_call=one, ms_per_iteration=round(per_iter, 4),
                                     bytes_per_particle_and_iteration=8,
                                     effective_GB_per_s=round(N * 8 / (per_iter * 1e-3) / 1e9, 1) if per_iter > 0 else None,
                                     particle_components_per_s=round(N * K / (per_iter * 1e-3), 0) if per_iter > 0 else None)
        torch_its = event_timed(lambda: torch_em(lw, x, 1, N, init, its, 0.0))
        rec['torch_float64_em_fixed_iterations'] = dict(torch_its, ms_per_iteration=round(torch_its['median_ms'] / its, 4))
        rec['torch_over_ours'] = round(rec['torch_float64_em']['median_ms'] / rec['ours']['median_ms'], 2)
        rec['cpu_over_ours'] = round(rec['cpu_reference_route']['median_ms'] / rec['ours']['median_ms'], 2)
        print(json.dumps(rec), flush=True)
        records.append(rec)
    M, Nb = args.batch
    K = 3
    lw, x = columns(M, Nb, 7)
    stats = group_stats(lw, x, M, Nb)
    host_stats = stats.cpu().numpy()
    posts, whole_log = [], []
    for g in range(M):
        sl = slice(g * Nb, (g + 1) * Nb)
        p = posterior(lw[sl], x[sl], host_stats[g])
        p._batch, p._batch_log = (x, lw, stats, g, Nb), whole_log
        posts.append(p)
    from pyprob_amd.empirical_batch import _batch_column
    assert _batch_column(posts, None) is not None, 'the posteriors must be recognised as one batched execution'
    fast = pyprob_amd.density_estimate_batch(posts, K)
    loop = [p.density_estimate(K) for p in posts]
    assert all(np.array_equal(a.fit.means, b.fit.means) and np.array_equal(a.fit.stddevs, b.fit.stddevs) and a.fit.n_iter == b.fit.n_iter
               for a, b in zip(fast, loop))
    init = default_init(posts, K)

    def fresh_loop():
        for p in posts:
            p.__dict__.pop('_dev_sorted', None)
        return [p.density_estimate(K) for p in posts]
    iters = [m.fit.n_iter for m in fast]
    levels = (np.arange(K) + 0.5) / K

    def rows_only():      # (what the other two routes return: numbers, no Mixture objects)
        start = np.concatenate([np.full((M, K), 1.0 / K), pyprob_amd.quantile_batch(posts, levels),
                                np.repeat(np.array([[p.variance / K ** 2 + REG] for p in posts]), K, 1)], 1)
        return ops.is_gmm_groups(lw, x, K, Nb, stats, torch.from_numpy(start).to(DEV), MAX_ITER, TOL, REG).cpu().numpy()
    rec = dict(case='density_estimate_batch(posts, 3)', M=M, N=Nb, K=K, n_iter_min=min(iters), n_iter_max=max(iters),
               ours=event_timed(lambda: pyprob_amd.density_estimate_batch(posts, K)),
               ours_rows_only_no_mixture_objects=event_timed(rows_only),
               loop_of_single_calls=event_timed(fresh_loop),
               torch_float64_em=event_timed(lambda: torch_em(lw, x, M, Nb, init)),
               cpu_reference_route=event_timed(lambda: cpu_reference_route(lw, x, M, Nb, K, rng)))
    its = args.iterations
    alone = event_timed(lambda: ops.is_gmm_groups(lw, x, K, Nb, stats, init, its, 0.0, REG))
    one = event_timed(lambda: ops.is_gmm_groups(lw, x, K, Nb, stats, init, 1, 0.0, REG))
    per_iter = (alone['median_ms'] - one['median_ms']) / (its - 1)
    rec['operator_alone'] = dict(iterations=its, call=alone, one_iteration_call=one, ms_per_iteration=round(per_iter, 4),
                                 bytes_per_particle_and_iteration=8,
                                 effective_GB_per_s=round(M * Nb * 8 / (per_iter * 1e-3) / 1e9, 1) if per_iter > 0 else None)
    for k in ('loop_of_single_calls', 'torch_float64_em', 'cpu_reference_route'):
        rec[k.split('_')[0] + '_over_ours'] = round(rec[k]['median_ms'] / rec['ours']['median_ms'], 2)
    print(json.dumps(rec), flush=True)
    records.append(rec)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, tol=TOL, max_iter=MAX_ITER, reg_covar=REG,
               check_every=os.environ.get('PP_GMM_CHECK', '8'),
               timing='device events around ONE call (launches, copies, host arithmetic), medians of --reps after --warmup',
               inputs='synthetic values (three Gaussian modes) and log-weights (normal), attached to Empiricals as a lock-step call '
                      'attaches them',
               ours='Empirical.density_estimate / pyprob_amd.density_estimate_batch: quantiles of the sorted particles for the start, '
                    'pp_is_gmm_groups (two launches per EM iteration, fp64), one copy of the rows',
               torch_float64_em='the same EM, start and stop rule in torch float64 on the device ([M, N, K] arrays, .item() per iteration)',
               cpu_reference_route='cpu() of the columns, 1000 values resampled by the weights, %s' % (
                   'scikit-learn GaussianMixture(covariance_type="diag").fit' if GaussianMixture is not None else
                   'the float64 numpy EM (scikit-learn is absent on this machine)'),
               records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
