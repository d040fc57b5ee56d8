"""Float64 / uint32 numpy restatement of pp_is_sort_groups / pp_is_quantile_groups / pp_is_unique_groups (include/pyprob_amd.h) for
the tests: the 32-bit keys, numpy's stable argsort of them, the inverted-cdf search on a given cdf, the runs of equal keys with the
histogram's fixed-point masses q = rint(min(w, 1) 2^S) summed as integers - next to them the real-valued sums (numpy.longdouble)
the derived bound |mass - sum w 2^S| <= 0.5 count + 2^-48 sum w 2^S is measured against; CPU doubles of the three operators with
call counters."""
import numpy as np
import torch

from histogram_ref import shift

EXCLUDED = np.uint32(0xFFFFFFFF)


def keys_ref(lw, x):
    """uint32 keys of lw, x (float32, any shape): EXCLUDED where lw is not finite or x is NaN, else the order-preserving map of the
    bits of x with -0.0 made +0.0."""
    lw = np.asarray(lw, np.float32)
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    b = x.view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isfinite(lw) & ~np.isnan(x), k, EXCLUDED).astype(np.uint32)


def sort_ref(lw, x):
    """lw, x [M, N] float32 -> (value [M, N] float32, lw [M, N] float32, index [M, N] int32, counted [M, 2] int32)."""
    lw = np.asarray(lw, np.float32)
    x = np.asarray(x, np.float32)
    k = keys_ref(lw, x)
    index = np.argsort(k, axis=1, kind='stable')
    counted = np.stack([(k != EXCLUDED).sum(1), (np.isfinite(lw) & np.isnan(x)).sum(1)], 1).astype(np.int32)
    return np.take_along_axis(x, index, 1), np.take_along_axis(lw, index, 1), index.astype(np.int32), counted


def quantile_ref(value_sorted, cdf_sorted, counted, q):
    """[M, Q] float64 by the header's rule on a GIVEN cdf [M, N] (float64)."""
    v = np.asarray(value_sorted, np.float32)
    cdf = np.asarray(cdf_sorted, np.float64)
    q = np.asarray(q, np.float64)
    out = np.full((v.shape[0], len(q)), np.nan)
    for g in range(v.shape[0]):
        c = int(counted[g][0])
        if c <= 0:
            continue
        T = cdf[g, c - 1]
        if not (T > 0 and np.isfinite(T)):
            continue
        t = q * T
        k = np.where(t > 0, np.searchsorted(cdf[g, :c], t, side='left'), np.count_nonzero(cdf[g, :c] <= 0))
        out[g] = v[g][np.minimum(k, c - 1)].astype(np.float64)
    return out


def group_max(lw):
    """The maximum of the finite log-weights per row in float64 (-inf where there is none)."""
    lw = np.asarray(lw, np.float64)
    return np.where(np.isfinite(lw), lw, -np.inf).max(axis=1)


def unique_ref(value_sorted, lw_sorted, counted):
    """Per group: (values float32 [r], mass int64 [r], count int64 [r], real longdouble [r]) over the runs of equal keys among the
    first c_g sorted particles; real = the sum of w 2^S in numpy.longdouble."""
    v = np.asarray(value_sorted, np.float32)
    lw = np.asarray(lw_sorted, np.float32)
    M, N = v.shape
    S = shift(N)
    top = group_max(lw)
    out = []
    for g in range(M):
        c = int(counted[g][0])
        if c <= 0:
            out.append((np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.longdouble)))
            continue
        k = keys_ref(lw[g, :c], v[g, :c])
        heads = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
        w = np.exp(lw[g, :c].astype(np.float64) - top[g])
        fixed = np.rint(np.minimum(w, 1.0) * 2.0 ** S).astype(np.int64)
        out.append((v[g, heads], np.add.reduceat(fixed, heads), np.diff(np.concatenate([heads, [c]])).astype(np.int64),
                    np.add.reduceat((w * 2.0 ** S).astype(np.longdouble), heads)))
    return out


calls = {'is_sort_groups': 0, 'is_quantile_groups': 0, 'is_unique_groups': 0}      # how often the CPU doubles ran


def is_sort_groups_cpu(lw, x, n_per, stats):
    calls['is_sort_groups'] += 1
    n = int(n_per)
    value, l, index, counted = sort_ref(lw.numpy().reshape(-1, n), x.numpy().reshape(-1, n))
    return (torch.from_numpy(np.ascontiguousarray(value.reshape(-1))), torch.from_numpy(np.ascontiguousarray(l.reshape(-1))),
            torch.from_numpy(np.ascontiguousarray(index.reshape(-1))), torch.from_numpy(counted))


def is_quantile_groups_cpu(value_sorted, cdf_sorted, counted, n_per, q):
    calls['is_quantile_groups'] += 1
    n = int(n_per)
    return torch.from_numpy(quantile_ref(value_sorted.numpy().reshape(-1, n), cdf_sorted.numpy().reshape(-1, n), counted.numpy(),
                                         q.numpy()))


def is_unique_groups_cpu(value_sorted, lw_sorted, counted, n_per, stats):
    calls['is_unique_groups'] += 1
    n = int(n_per)
    runs = unique_ref(value_sorted.numpy().reshape(-1, n), lw_sorted.numpy().reshape(-1, n), counted.numpy())
    M = len(runs)
    value, mass, count = np.zeros((M, n), np.float32), np.zeros((M, n), np.int64), np.zeros((M, n), np.int32)
    for g, (v, m, c, _) in enumerate(runs):
        value[g, :len(v)], mass[g, :len(v)], count[g, :len(v)] = v, m, c
    return (torch.from_numpy(value), torch.from_numpy(mass), torch.from_numpy(count),
            torch.tensor([len(r[0]) for r in runs], dtype=torch.int32))


_registered = False


def register_cpu_doubles():
    """The product has no CPU implementation of the operators: the tests register the numpy restatements as their CPU kernels."""
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_sort_groups', is_sort_groups_cpu, 'CPU')
        P._lib.impl('is_quantile_groups', is_quantile_groups_cpu, 'CPU')
        P._lib.impl('is_unique_groups', is_unique_groups_cpu, 'CPU')
        _registered = True
