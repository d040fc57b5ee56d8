"""The *_batch functions: a statistic of every posterior of a list - and, where the list is the M groups of ONE
Model.posterior_results_batch execution in order, the same result bit for bit from one operator call over all groups."""
import numpy as np
import torch

from .empirical import (_device_ecdf, _device_histograms, _device_hpd, _device_psis, _device_quantiles, _device_stats_row,
                        _gmm_arguments, _gmm_init_rows, _hpd_levels, _joint_rows, _lw_sorted_groups, _mixtures_from_rows,
                        _moment_rows, _philox_key, _psis_tail, _quantile_levels, _resample_op, _scheme_id, _sorted_groups)


def _one_execution(posteriors, shared='_batch_log'):
    """(values, lw, group statistics, N, the shared object) where the posteriors are the M groups of ONE
    Model.posterior_results_batch execution in order - every member holds the call's whole tensors and its own group index (_batch:
    model.py sets it where the call dropped none of the group's particles), the call's one object under `shared` and still takes
    the device route, which PP_EMPIRICAL_DEVICE=0 closes; else None. `shared` is the call's statement log for every caller but
    one: the parameter exists only for resample_batch, which needs no log but the call's runner ('_batch_runner')."""
    own = posteriors[0].__dict__
    first, also = own.get('_batch'), own.get(shared)
    if first is None or also is None or first[0].numel() != len(posteriors) * first[4]:
        return None
    for g, p in enumerate(posteriors):
        b = p.__dict__.get('_batch')
        if b is None or b[0] is not first[0] or b[1] is not first[1] or b[2] is not first[2] or b[3] != g or \
                p.__dict__.get(shared) is not also or not p._device_backed():
            return None
    values, lw, group_stats, _, N = first
    return values, lw, group_stats, N, also


def _log_columns(log):
    """{address: the column of ALL particles of the call} of a batched call's statement log."""
    return {a: rec[0] for entry in log for a, rec in entry.items()}


def _batch_column(posteriors, address):
    """(lw, column, N, group statistics) where the posteriors are the M groups of ONE Model.posterior_results_batch execution in
    order (_one_execution) and `address` names the value forward() returned (None) or a column of the call's statement log that
    every particle executed; else None."""
    found = _one_execution(posteriors)
    if found is None or found[2] is None:       # (the kernels take every group's maximum from the call's [M, 6] statistics)
        return None
    column, lw, group_stats, N, log = found
    if address is not None:
        a, _, rows = posteriors[0]._latent(address)
        column = _log_columns(log).get(a) if rows is None else None       # (a branch's address: each group's marginal has its own particles)
        if column is None or column.dtype != torch.float32 or column.numel() != lw.numel() or not column.is_contiguous():
            return None
    return lw, column, N, group_stats


def _target(p, address):
    return p if address is None else p.marginal(address)


def histogram_batch(posteriors, bins=50, range=None, address=None):
    """[p.histogram(bins, range) for p in posteriors], or with address= [p.marginal(address).histogram(bins, range) ...] - and,
    where the posteriors are the M groups of ONE Model.posterior_results_batch execution in order (recognised as joint_batch
    recognises them), the same Histograms bit for bit from one pp_is_extent_groups launch (range=None: every group gets edges over
    its own extent), ONE pp_is_hist_groups launch sequence over all groups (the maxima from the call's own [M, 6] statistics) and
    one device-to-host copy of the rows. address=None: the value forward() returned; else an address (or statement name) of the
    call's statement log that every particle executed. Anything else is served by the loop."""
    posteriors = list(posteriors)
    if not posteriors:
        return []
    found = _batch_column(posteriors, address)
    if found is None:
        return [_target(p, address).histogram(bins, range) for p in posteriors]
    lw, column, N, group_stats = found
    return _device_histograms(lw, column, N, bins, range, None, group_stats)


def quantile_batch(posteriors, q, address=None):
    """numpy.stack([p.quantile(q) for p in posteriors]) as float64 [M, Q] (a scalar q: Q = 1), or with address=
    [p.marginal(address).quantile(q) ...] - and, where the posteriors are the M groups of ONE Model.posterior_results_batch
    execution in order, the same numbers bit for bit from ONE pp_is_sort_groups launch sequence over all groups, one
    pp_is_cdf_groups call over the sorted log-weights, one pp_is_quantile_groups launch and one device-to-host copy. address=None:
    the value forward() returned; else an address (or statement name) of the call's statement log that every particle executed.
    Anything else is served by the loop."""
    posteriors = list(posteriors)
    qs = _quantile_levels(q)[0]
    if not posteriors:
        return np.zeros((0, len(qs)))
    found = _batch_column(posteriors, address)
    if found is None:
        return np.stack([_target(p, address).quantile(qs) for p in posteriors])
    return _device_quantiles(_sorted_groups(*found), found[2], qs)


def hpd_batch(posteriors, level=0.9, address=None):
    """numpy.stack([p.hpd_interval(level) for p in posteriors]) as float64 [M, 2] (a scalar level) or [M, L, 2], or with address=
    [p.marginal(address).hpd_interval(level) ...] - and, where the posteriors are the M groups of ONE
    Model.posterior_results_batch execution in order (recognised as quantile_batch recognises them), the same numbers bit for bit
    from one pp_is_sort_groups call, one pp_is_cdf_groups call over the sorted log-weights, ONE pp_is_hpd_groups call and one
    device-to-host copy. Anything else is served by the loop."""
    posteriors = list(posteriors)
    levels, scalar = _hpd_levels(level)
    if not posteriors:
        return np.zeros((0, 2) if scalar else (0, len(levels), 2))
    found = _batch_column(posteriors, address)
    if found is None:
        out = np.stack([np.asarray(_target(p, address).hpd_interval(levels)) for p in posteriors])
    else:
        out = _device_hpd(_sorted_groups(*found), found[2], levels)
    return out[:, 0] if scalar else out


def cdf_batch(posteriors, x, address=None, strict=False):
    """[p.cdf(x[g], strict) for g, p in enumerate(posteriors)] as float64 numpy of x's shape - x is [M] (one point per posterior: the
    ground truth of a calibration check) or [M, Q] - or with address= [p.marginal(address).cdf(x[g], strict) ...]; and, where the
    posteriors are the M groups of ONE Model.posterior_results_batch execution in order, the same numbers bit for bit from one
    sort, one cdf over the sorted log-weights, ONE pp_is_ecdf_groups call (every group with its own points) and one copy."""
    posteriors = list(posteriors)
    xs = np.asarray(x, np.float64)
    if xs.ndim not in (1, 2) or xs.shape[0] != len(posteriors):
        raise ValueError('x is [M] or [M, Q]: one row of points per posterior')
    if not posteriors:
        return np.zeros(xs.shape)
    pts = np.ascontiguousarray(xs.reshape(len(posteriors), -1))
    found = _batch_column(posteriors, address)
    if found is None:
        out = np.stack([np.asarray(_target(p, address).cdf(pts[g], strict)) for g, p in enumerate(posteriors)])
    else:
        out = _device_ecdf(_sorted_groups(*found), found[2], pts, strict)
    return out.reshape(xs.shape)


def _psis_batch_call(posteriors, tail, want_weights):
    """(lw_out or None, out rows in numpy, N) from one sort by log-weight and ONE pp_is_psis_groups call where the posteriors are
    the M groups of one Model.posterior_results_batch execution in order (as quantile_batch recognises them); else None."""
    found = _batch_column(posteriors, None)
    if found is None:
        return None
    lw, _, N, group_stats = found
    return _device_psis(_lw_sorted_groups(lw, N, group_stats), N, group_stats, tail, want_weights) + (N,)


def pareto_k_batch(posteriors, tail=None):
    """numpy.array([p.pareto_k(tail) for p in posteriors]) as float64 [M]: one k-hat per observation - the amortisation gap of the
    trained network, observation by observation - and, where the posteriors are the M groups of ONE Model.posterior_results_batch
    execution in order, the same numbers bit for bit from one pp_is_sort_groups call keyed on the log-weights, ONE
    pp_is_psis_groups call (without the smoothing launch) and one device-to-host copy. Anything else is served by the loop."""
    posteriors = list(posteriors)
    t = _psis_tail(tail)
    if not posteriors:
        return np.zeros(0)
    got = _psis_batch_call(posteriors, t, False)
    if got is None:
        return np.array([p.pareto_k(tail) for p in posteriors], np.float64)
    return np.ascontiguousarray(got[1][:, 0])


def psis_batch(posteriors, tail=None):
    """[p.psis(tail) for p in posteriors] - and, where the posteriors are the M groups of ONE Model.posterior_results_batch execution
    in order, the same log-weights and fits bit for bit from one sort, ONE pp_is_psis_groups call over all groups and one copy of
    the rows of `out` (the statistics of each smoothed group are reduced by pp_is_stats as in the loop, and travel in one more copy)."""
    posteriors = list(posteriors)
    t = _psis_tail(tail)
    if not posteriors:
        return []
    got = _psis_batch_call(posteriors, t, True)
    if got is None:
        return [p.psis(tail) for p in posteriors]
    lw_out, rows, N = got
    from .is_engine import DistRunner
    parts = lw_out.split(N)
    # (no particle was dropped in a recognised batch: the statistics of every smoothed group by the loop's call, ONE copy)
    stats = torch.stack([_device_stats_row(part, p._values) for p, part in zip(posteriors, parts)]).cpu().numpy()
    return [p._psis_result(part, rows[g], DistRunner._stats_dict(stats[g])) for g, (p, part) in enumerate(zip(posteriors, parts))]


def density_estimate_batch(posteriors, num_mixture_components=1, address=None, num_samples=None, tol=1e-3, max_iter=100,
                           reg_covar=1e-6, weights_init=None, means_init=None, stddevs_init=None):
    """[p.density_estimate(num_mixture_components, ...) for p in posteriors], or with address=
    [p.marginal(address).density_estimate(...) ...] - and, where the posteriors are the M groups of ONE
    Model.posterior_results_batch execution in order (recognised as quantile_batch recognises them) and num_samples is None, the
    same Mixtures bit for bit from ONE quantile_batch call for the initial means, one pp_is_gmm_groups call over all groups (the
    maxima from the call's own [M, 6] statistics; groups that converge early are frozen while the others go on) and one
    device-to-host copy of the rows. The initial variances are each group's own `variance` (address=None: the statistics of the
    call; an address: the statistics of its marginal, one small reduction per group). Anything else is served by the loop."""
    posteriors = list(posteriors)
    K = _gmm_arguments(num_mixture_components, tol, max_iter, reg_covar)
    if not posteriors:
        return []
    found = _batch_column(posteriors, address) if num_samples is None else None
    if found is None:
        return [_target(p, address).density_estimate(K, num_samples, tol, max_iter, reg_covar, weights_init, means_init,
                                                     stddevs_init) for p in posteriors]
    from .ops import ops
    lw, column, N, group_stats = found
    levels = (np.arange(K) + 0.5) / K
    init = _gmm_init_rows(K, reg_covar, weights_init, means_init, stddevs_init, lambda: quantile_batch(posteriors, levels, address),
                          lambda: [_target(p, address)._skipping_variance() for p in posteriors])
    init = np.array(np.broadcast_to(init, (len(posteriors), 3 * K)))
    rows = ops.is_gmm_groups(lw, column, K, N, group_stats, torch.from_numpy(init).to(lw.device), int(max_iter), float(tol),
                             float(reg_covar)).cpu().numpy()
    return _mixtures_from_rows(rows, K, [p._metadata for p in posteriors], N, tol, max_iter, reg_covar)


def joint_batch(posteriors, addresses=None):
    """[p.joint(addresses) for p in posteriors] - and, where the posteriors are the M groups of ONE
    Model.posterior_results_batch execution in order, the same numbers bit for bit from ONE pp_is_moments_groups launch over all
    groups (the maxima from the call's own [M, 6] statistics) and one device-to-host copy."""
    posteriors = list(posteriors)
    if not posteriors:
        return []
    found = _batch_column(posteriors, None)
    if found is None:
        return [p.joint(addresses) for p in posteriors]
    lw, _, N, group_stats = found
    chosen, _ = posteriors[0]._joint_columns(addresses)
    whole = _log_columns(posteriors[0]._batch_log)
    if any(a not in whole for a in chosen):      # (reobserve_batch: the members share the [N] columns of ONE posterior)
        return [p.joint(addresses) for p in posteriors]
    return _joint_rows(chosen, _moment_rows(lw, [whole[a] for a in chosen], N, group_stats))


def resample_batch(posteriors, num_samples, seed=None, offset=0, scheme='multinomial'):
    """[p.resample(num_samples, seed=seed, offset=offset + g * num_samples) for g, p in enumerate(posteriors)] (scheme='systematic',
    which takes ONE uniform per group: offset + g; scheme as for Empirical.resample) - and, where the
    posteriors are the M groups of ONE Model.posterior_results_batch execution in order, the same values bit for bit from one
    pp_is_cdf_groups and one pp_is_resample_groups launch over all groups, with the statistics of the M resampled groups from the
    grouped statistics pass in one device-to-host copy. seed=None: one key from torch's global generator for the whole list."""
    posteriors = list(posteriors)
    n = int(num_samples)
    _scheme_id(scheme)
    if not posteriors:
        return []
    key = _philox_key(seed)       # (before the route is decided: either route spends the same one number of torch's generator)
    found = _one_execution(posteriors, '_batch_runner') if n >= 1 and len(posteriors) * n <= 0x7fffffff else None
    if found is None:
        step = 1 if scheme == 'systematic' else n
        return [p.resample(n, seed=key, offset=int(offset) + g * step, scheme=scheme) for g, p in enumerate(posteriors)]
    from .ops import ops
    values, lw, group_stats, N, runner = found
    cdf = posteriors[0].__dict__.get('_batch_cdf')
    if cdf is None:       # (once per batched call, kept by its first group; every group's own cdf is its slice - the same bits)
        cdf = posteriors[0].__dict__['_batch_cdf'] = ops.is_cdf_groups(lw, N, group_stats)
        for p, part in zip(posteriors, cdf.split(N)):
            p.__dict__.setdefault('_dev_cdf', part)
    drawn = _resample_op(cdf, values, N, 0, N, n, scheme, key, int(offset), False)[1]
    zeros = torch.zeros_like(drawn)
    stats = runner.fused_groups(None, n, None, [], drawn, zeros, False, stats=True).cpu().numpy()
    d_parts, z_parts = drawn.split(n), zeros.split(n)
    return [p._resampled(d_parts[g], z_parts[g], runner._stats_dict(stats[g]), n, p.effective_sample_size, scheme)
            for g, p in enumerate(posteriors)]


def reobserve_batch(post, observes, likelihood_funcs=None, likelihood_importance=None):
    """[post.reobserve(observes[g], likelihood_funcs, likelihood_importance) for g in range(M)] - the posteriors of ONE set of
    particles under M observations - bit for bit from ONE replay of the program, ONE pp_is_reobserve_groups call over all M N rows,
    one grouped statistics pass (one pp_is_stats launch per group where the model has no inference network) and ONE
    device-to-host copy of the statistics. `observes` as posterior_results_batch takes
    them: a list of M observe dicts with equal keys, or one dict name -> tensor with a leading dimension M.

    The members hold the call's [M, N] log-weights, the values expanded to [M, N] and the [M, 6] statistics (`_batch`), so with
    address=None quantile_batch, hpd_batch, cdf_batch, histogram_batch, pareto_k_batch, psis_batch, density_estimate_batch and
    (where the posterior came from an inference-network call) resample_batch recognise them as one execution; the address= forms
    and joint_batch take their loop - every member's own marginal / joint answer from the shared [N] columns of the statement
    log. `pareto_k_batch(reobserve_batch(post, observes))` says observation by observation whether the particles still cover the
    new posterior."""
    from .is_engine import DistRunner
    from .model import Model
    names, dicts, cols = Model._normalise_observes(observes)
    M = len(dicts)
    post._check_finalized()
    out, seen, origin = post._reobserve_weights(cols, M, likelihood_funcs, likelihood_importance)
    N = int(out.shape[1])
    # (the values expanded to [M N]: what the grouped kernels behind the *_batch functions index; materialised once per call)
    group_stats, values, runner = post._reobserve_stats(origin, out)
    stats = group_stats.cpu().numpy()          # the one device-to-host copy
    lw_all = out.reshape(-1)
    log = []      # (the call's own [M N] columns do not exist: joint_batch and the address= forms take their loop)
    members = []
    for g in range(M):
        emp = post._reobserve_result(out[g], DistRunner._stats_dict(stats[g]), origin, dicts[g], seen)
        if emp.length == N:      # (no particle dropped) the call's whole tensors: the *_batch functions serve all groups at once
            emp._batch, emp._batch_log = (values, lw_all, group_stats, g, N), log
            if runner is not None:
                emp._batch_runner = runner
        members.append(emp)
    return members
