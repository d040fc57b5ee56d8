"""Float64 restatement of pp_is_cdf_groups / pp_is_resample_groups (include/pyprob_amd.h) for the tests: the weights, the cdf,
the 53-bit uniform from obs_draw_ref's numpy Philox4x32-10, the target in two roundings and numpy.searchsorted - and CPU doubles
of the two operators."""
import numpy as np
import torch

from obs_draw_ref import philox4x32_10

STREAM = 0x52


def weights_ref(lw):
    """w = exp(lw - max of the finite lw) per row in float64, 0 where lw is not finite. lw [M, N]."""
    lw = np.asarray(lw, np.float64)
    fin = np.isfinite(lw)
    m = np.where(fin, lw, -np.inf).max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.exp(np.where(fin, lw, 0.0) - np.where(np.isfinite(m), m, 0.0))
    return np.where(fin, w, 0.0)


def cdf_ref(lw):
    return np.cumsum(weights_ref(lw), axis=1)


def uniform53(seed, counters):
    """u of draw `counter`: words 0 and 1 of the Philox block (key seed, counter words lo, hi, stream 0x52, 0) give 27 + 26 bits;
    u = (bits + 0.5) 2^-53 in float64 arithmetic (the + 0.5 rounds to even above 2^52, as on the device)."""
    c = np.asarray(counters, np.uint64)
    w = philox4x32_10(seed, c & np.uint64(0xFFFFFFFF), c >> np.uint64(32), np.uint64(STREAM), np.uint64(0))
    bits = ((w[..., 0] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1] >> np.uint64(6))
    return (bits.astype(np.float64) + 0.5) * 2.0 ** -53


def targets_ref(cdf_g, lo, hi, u):
    """(target per draw, total): base + u * total with each operation rounded on its own (numpy does)."""
    base = cdf_g[lo - 1] if lo > 0 else 0.0
    total = cdf_g[hi - 1] - base
    return base + u * total, total


def resample_ref(cdf, values, lo, hi, n_out, seed, offset):
    """index [M, n_out] (int64) and value [M, n_out] (float32; None without values) of pp_is_resample_groups on a cdf [M, N]."""
    cdf = np.asarray(cdf, np.float64)
    M, N = cdf.shape
    index = np.full((M, n_out), -1, np.int64)
    first = np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(M, dtype=np.uint64)[:, None] * np.uint64(n_out)      # (wraps mod 2^64)
    u = uniform53(seed, first + np.arange(n_out, dtype=np.uint64))
    target, total = targets_ref(cdf.T, lo, hi, u.T)      # (the group is the LAST axis of both: [n_out, M] targets, [M] totals)
    target = target.T
    live = (total > 0) & np.isfinite(total)
    if M * n_out * (hi - lo) <= 2 ** 26:      # searchsorted(side='right') = the number of entries <= target, for all groups at once
        found = lo + (cdf[:, None, lo:hi] <= target[:, :, None]).sum(2)
        index[live] = np.minimum(found, hi - 1)[live]
    else:
        for g in np.nonzero(live)[0]:
            index[g] = np.minimum(lo + np.searchsorted(cdf[g, lo:hi], target[g], side='right'), hi - 1)
    value = None
    if values is not None:
        v = np.asarray(values, np.float32).reshape(M, N)
        value = np.where(index >= 0, np.take_along_axis(v, np.maximum(index, 0), 1), np.float32('nan')).astype(np.float32)
    return index, value


calls = {'is_cdf_groups': 0, 'is_resample_groups': 0}      # how often the CPU doubles ran


def is_cdf_groups_cpu(lw, n_per, stats):
    calls['is_cdf_groups'] += 1
    return torch.from_numpy(np.ascontiguousarray(cdf_ref(lw.numpy().reshape(-1, int(n_per))).reshape(-1)))


def is_resample_groups_cpu(cdf, values, n_per, lo, hi, n_out, seed, offset, want_index):
    calls['is_resample_groups'] += 1
    index, value = resample_ref(cdf.numpy().reshape(-1, int(n_per)), None if values is None else values.numpy(), int(lo), int(hi),
                                int(n_out), int(seed), int(offset))
    return (torch.from_numpy(index.reshape(-1)) if want_index else torch.empty(0, dtype=torch.int64),
            torch.from_numpy(value.reshape(-1)) if value is not None else torch.empty(0, dtype=torch.float32))


_registered = False


def register_cpu_doubles():
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_cdf_groups', is_cdf_groups_cpu, 'CPU')
        P._lib.impl('is_resample_groups', is_resample_groups_cpu, 'CPU')
        _registered = True
