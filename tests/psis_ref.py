"""pp_is_psis_groups restated in numpy from the header comment of include/pyprob_amd.h (Pareto-smoothed importance weights: the
Zhang-Stephens profile estimate of a generalised Pareto tail, its shape k-hat and the smoothed tail weights), in float64 or in
numpy.longdouble (the dtype argument), and the CPU double of the operator. Sums are numpy.sum over one 1-D array each."""
import math

import numpy as np
import torch

WIDTH = 8          # PP_IS_PSIS_WIDTH: k-hat, sigma, n, m, f, cutoff log-weight, c, maximum


def tail_length(c, tail):
    return int(tail) if tail > 0 else int(math.ceil(min(c / 5.0, 3.0 * math.sqrt(float(c)))))


def gpd_fit(y, dtype=np.float64):
    """(kappa before the prior, sigma, m) of the profile estimate over ascending exceedances y (n > 4, y[0] > 0)."""
    T = dtype
    y = np.asarray(y, T)
    n = len(y)
    m = 30 + int(math.floor(math.sqrt(float(n))))
    q = y[int(n / 4.0 + 0.5) - 1]
    with np.errstate(all='ignore'):
        j = np.arange(1, m + 1).astype(T)
        theta = T(1) / y[n - 1] + (T(1) - np.sqrt(T(m) / (j - T(0.5)))) / (T(3) * q)
        kap = np.array([np.sum(np.log1p(-theta[k] * y)) / T(n) for k in range(m)], T)
        L = T(n) * (np.log(-theta / kap) - kap - T(1))
        omega = np.array([T(1) / np.sum(np.exp(L - L[k])) for k in range(m)], T)
        that = np.sum(omega * theta)
        kappa = np.sum(np.log1p(-that * y)) / T(n)
        sigma = -kappa / that
    return kappa, sigma, m


def fit_group(s32, tail, dtype=np.float64):
    """One group: s32 = its c counted log-weights in ascending order (float32). Returns (row [WIDTH] of dtype, f, smoothed float32 [n]
    or None where the weights stay unchanged)."""
    T = dtype
    s32 = np.asarray(s32, np.float32)
    c = len(s32)
    row = np.array([np.inf, np.nan, 0, 0, 0, np.nan, c, np.nan], T)
    if c == 0:
        return row, 0, None
    s = s32.astype(T)
    Mg = s[c - 1]
    row[7] = Mg
    b = c - tail_length(c, tail) - 1
    if b < 0:
        return row, 0, None
    f = int(np.count_nonzero(s32 <= s32[b]))
    n = c - f
    u = np.exp(s[b] - Mg)
    row[2], row[4], row[5] = n, f, s[b]
    if n <= 4:
        return row, f, None
    y = np.exp(s[f:] - Mg) - u
    if not y[0] > 0:
        return row, f, None
    kappa, sigma, m = gpd_fit(y, T)
    khat = (T(n) * kappa + T(5)) / (T(n) + T(10))
    row[0], row[1], row[3] = khat, sigma, m
    if not np.isfinite(khat):
        return row, f, None
    with np.errstate(all='ignore'):
        lp = np.log1p(-(np.arange(n).astype(T) + T(0.5)) / T(n))
        w = u - sigma * lp if khat == 0 else u + sigma * np.expm1(-khat * lp) / khat
        new = np.minimum(np.log(w), T(0)) + Mg
    return row, f, new.astype(np.float32)


def psis_ref(lw_sorted, index_sorted, counted, tail, dtype=np.float64, want_weights=True):
    """lw_sorted [M, N] float32, index_sorted [M, N] int32, counted [M, 2] -> (lw_out [M, N] float32 in particle order or None,
    out [M, WIDTH] of dtype)."""
    ls = np.ascontiguousarray(np.asarray(lw_sorted, np.float32))
    idx = np.asarray(index_sorted).astype(np.int64)
    M, N = ls.shape
    out = np.zeros((M, WIDTH), dtype)
    bits = np.zeros((M, N), np.uint32)
    for g in range(M):
        c = max(0, min(int(np.asarray(counted)[g, 0]), N))
        row, f, new = fit_group(ls[g, :c], tail, dtype)
        out[g] = row
        if want_weights:
            sorted_bits = ls[g].view(np.uint32).copy()          # (bits, so that NaN payloads travel unchanged)
            if new is not None:
                sorted_bits[f:c] = new.view(np.uint32)
            bits[g, idx[g]] = sorted_bits
    return (bits.view(np.float32) if want_weights else None), out


def sort_by_lw(lw):
    """pp_is_sort_groups(lw, x = lw) on lw [M, N] float32: (lw_sorted, index int32, counted int32 [M, 2]) - stable ascending order of
    the finite log-weights (-0.0 == +0.0), every other particle behind them in particle order."""
    lw = np.asarray(lw, np.float32)
    M, N = lw.shape
    ls, index, counted = np.empty_like(lw), np.empty((M, N), np.int32), np.zeros((M, 2), np.int32)
    for g in range(M):
        fin = np.isfinite(lw[g])
        a = np.nonzero(fin)[0]
        order = np.concatenate([a[np.argsort(lw[g, a] + np.float32(0), kind='stable')], np.nonzero(~fin)[0]])
        index[g] = order
        ls[g] = lw[g].view(np.uint32)[order].view(np.float32)
        counted[g, 0] = len(a)
    return ls, index, counted


def fit_loop(s32, tail):
    """fit_group's row in float64 by plain loops over j and r (the terms one by one; every sum is numpy.sum over the collected terms,
    as in fit_group): the check of the vectorised restatement."""
    s32 = np.asarray(s32, np.float32)
    c = len(s32)
    row = [np.inf, np.nan, 0.0, 0.0, 0.0, np.nan, float(c), np.nan]
    if c == 0:
        return row
    s = [np.float64(v) for v in s32]
    Mg = s[c - 1]
    row[7] = Mg
    b = c - tail_length(c, tail) - 1
    if b < 0:
        return row
    f = sum(1 for i in range(c) if s[i] <= s[b])
    n = c - f
    u = np.exp(s[b] - Mg)
    row[2], row[4], row[5] = float(n), float(f), s[b]
    if n <= 4:
        return row
    y = [np.exp(s[f + r] - Mg) - u for r in range(n)]
    if not y[0] > 0:
        return row
    m = 30 + int(math.floor(math.sqrt(float(n))))
    q = y[int(n / 4.0 + 0.5) - 1]
    theta, L = [], []
    with np.errstate(all='ignore'):
        for j in range(1, m + 1):
            th = np.float64(1) / y[n - 1] + (np.float64(1) - np.sqrt(np.float64(m) / (np.float64(j) - np.float64(0.5)))) / (np.float64(3) * q)
            kap = np.sum(np.array([np.log1p(-th * y[r]) for r in range(n)])) / np.float64(n)
            theta.append(th)
            L.append(np.float64(n) * (np.log(-th / kap) - kap - np.float64(1)))
        omega = [np.float64(1) / np.sum(np.array([np.exp(L[l] - L[j]) for l in range(m)])) for j in range(m)]
        that = np.sum(np.array([omega[j] * theta[j] for j in range(m)]))
        kappa = np.sum(np.array([np.log1p(-that * y[r]) for r in range(n)])) / np.float64(n)
    row[0] = (np.float64(n) * kappa + 5.0) / (np.float64(n) + 10.0)
    row[1] = -kappa / that
    row[3] = float(m)
    return row


calls = {'is_psis_groups': 0}      # how often the CPU double ran


def is_psis_groups_cpu(lw_sorted, index_sorted, counted, n_per, stats, tail, want_weights):
    calls['is_psis_groups'] += 1
    n = int(n_per)
    lw_out, out = psis_ref(lw_sorted.numpy().reshape(-1, n), index_sorted.numpy().reshape(-1, n), counted.numpy(), int(tail),
                           np.float64, bool(want_weights))
    return (torch.from_numpy(lw_out.reshape(-1).copy()) if want_weights else None), torch.from_numpy(out)


_registered = False


def register_cpu_doubles():
    """The product has no CPU implementation of the operator: the tests register the numpy restatement as its CPU kernel."""
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_psis_groups', is_psis_groups_cpu, 'CPU')
        _registered = True
