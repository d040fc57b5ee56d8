"""Float64 numpy restatement of pp_is_hpd_groups / pp_is_ecdf_groups / pp_is_resample_scheme_groups (include/pyprob_amd.h) for the
tests: the valid starts, their ends by numpy.searchsorted on a GIVEN cdf, the first minimum of the widths; the rank of a point among
the sorted values; the stratified and systematic positions from obs_draw_ref's numpy Philox4x32-10 - and CPU doubles of the three
operators with call counters."""
import numpy as np
import torch

from obs_draw_ref import philox4x32_10
from resample_ref import resample_ref

MULTINOMIAL, STRATIFIED, SYSTEMATIC = 0, 1, 2
SCHEMES = {'multinomial': MULTINOMIAL, 'stratified': STRATIFIED, 'systematic': SYSTEMATIC}


def _live(cdf_g, c):
    return c > 0 and cdf_g[c - 1] > 0 and np.isfinite(cdf_g[c - 1])


def _level_ok(L):
    return bool(L > 0 and L <= 1)          # (NaN fails both)


def hpd_ref(value_sorted, cdf_sorted, counted, levels):
    """(out float64 [M, L, 2], index int32 [M, L, 2]) by the header's rule on a GIVEN cdf [M, N] (float64) of sorted values [M, N]."""
    v = np.asarray(value_sorted, np.float32)
    cdf = np.asarray(cdf_sorted, np.float64)
    levels = np.asarray(levels, np.float64).reshape(-1)
    M, N = v.shape
    out = np.full((M, len(levels), 2), np.nan)
    index = np.full((M, len(levels), 2), -1, np.int32)
    cs = np.minimum(np.asarray(counted)[:, 0].astype(np.int64), N)
    if M * N * N <= 2 ** 24:          # every group at once: the count of cdf[k] < t_i by comparison instead of a search
        col = np.arange(N)[None, :]
        inside = col < cs[:, None]
        T = np.where(cs > 0, cdf[np.arange(M), np.maximum(cs, 1) - 1], np.nan)
        alive = (cs > 0) & (T > 0) & np.isfinite(T)
        prev = np.concatenate([np.zeros((M, 1)), cdf[:, :-1]], 1)
        vd = v.astype(np.float64)
        for l, L in enumerate(levels):
            if not _level_ok(L):
                continue
            with np.errstate(invalid='ignore'):
                t = prev + (L * T)[:, None]
                valid = inside & (cdf > prev) & (t <= T[:, None]) & alive[:, None]
                ends = np.maximum(col, ((cdf[:, None, :] < t[:, :, None]) & inside[:, None, :]).sum(2))
                ends = np.minimum(ends, N - 1)
                width = np.take_along_axis(vd, ends, 1) - vd
            width = np.where(np.isnan(width), np.inf, width)
            least = np.where(valid, width, np.inf).min(1)
            first = np.argmax(valid & (width == least[:, None]), 1)          # the first VALID start of the smallest width
            won = np.nonzero(valid.any(1))[0]
            k = first[won]
            index[won, l, 0], index[won, l, 1] = k, ends[won, k]
            out[won, l, 0], out[won, l, 1] = vd[won, k], vd[won, ends[won, k]]
        return out, index
    for g in range(M):
        c = int(cs[g])
        if not _live(cdf[g], c):
            continue
        cd, vd = cdf[g, :c], v[g, :c].astype(np.float64)
        T = cd[-1]
        prev = np.concatenate([[0.0], cd[:-1]])
        for l, L in enumerate(levels):
            if not _level_ok(L):
                continue
            t = prev + L * T
            starts = np.nonzero((cd > prev) & (t <= T))[0]
            ends = np.maximum(starts, np.searchsorted(cd, t[starts], side='left'))
            with np.errstate(invalid='ignore'):
                width = vd[ends] - vd[starts]
            width = np.where(np.isnan(width), np.inf, width)
            k = int(np.argmin(width))          # (numpy's argmin: the first minimum)
            index[g, l] = starts[k], ends[k]
            out[g, l] = vd[starts[k]], vd[ends[k]]
    return out, index


def hpd_brute(v, cdf, c, L):
    """(i, j) of one group and one level by an O(n^2) loop written from the definition; None where the result is NaN."""
    if c <= 0 or not (cdf[c - 1] > 0 and np.isfinite(cdf[c - 1])) or not _level_ok(L):
        return None
    T = cdf[c - 1]
    m = L * T
    best = None
    for i in range(c):
        prev = cdf[i - 1] if i > 0 else 0.0
        t = prev + m
        if not (cdf[i] > prev and t <= T):
            continue
        j = max(i, sum(1 for k in range(c) if cdf[k] < t))
        with np.errstate(invalid='ignore'):
            w = np.float64(v[j]) - np.float64(v[i])
        w = np.inf if np.isnan(w) else float(w)
        if best is None or w < best[0]:
            best = (w, i, j)
    return best[1], best[2]


def ecdf_ref(value_sorted, cdf_sorted, counted, x, strict):
    """(out float64 [M, Q], rank int32 [M, Q]) by the header's rule; x [M, Q] per group."""
    v = np.asarray(value_sorted, np.float32)
    cdf = np.asarray(cdf_sorted, np.float64)
    x = np.asarray(x, np.float64)
    M, N = v.shape
    out = np.full(x.shape, np.nan)
    rank = np.full(x.shape, -1, np.int32)
    cs = np.minimum(np.asarray(counted)[:, 0].astype(np.int64), N)
    for g in range(M):
        c = int(cs[g])
        if not _live(cdf[g], c):
            continue
        vd = v[g, :c].astype(np.float64)
        ok = ~np.isnan(x[g])
        k = np.searchsorted(vd, np.where(ok, x[g], 0.0), side='left' if strict else 'right')
        val = np.where(k == 0, 0.0, cdf[g, np.maximum(k, 1) - 1] / cdf[g, c - 1])
        out[g] = np.where(ok, val, np.nan)
        rank[g] = np.where(ok, k, -1)
    return out, rank


def uniform53(seed, counters, stream):
    """The 53-bit uniform of resample_ref.uniform53 on another Philox stream id."""
    c = np.asarray(counters, np.uint64)
    w = philox4x32_10(seed, c & np.uint64(0xFFFFFFFF), c >> np.uint64(32), np.uint64(stream), np.uint64(0))
    bits = ((w[..., 0] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1] >> np.uint64(6))
    return (bits.astype(np.float64) + 0.5) * 2.0 ** -53


def positions_ref(M, n_out, scheme, seed, offset):
    """p [M, n_out]: min(fl(fl(j + u) / n_out), 1 - 2^-53); u per draw (stratified) or per group (systematic). Counters wrap mod
    2^64."""
    off = np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF)
    g = np.arange(M, dtype=np.uint64)[:, None]
    j = np.arange(n_out, dtype=np.uint64)[None, :]
    with np.errstate(over='ignore'):
        if scheme == STRATIFIED:
            u = uniform53(seed, off + g * np.uint64(n_out) + j, 0x52)
        else:
            u = uniform53(seed, off + g, 0x53)
    return np.minimum((j.astype(np.float64) + u) / np.float64(n_out), 1.0 - 2.0 ** -53)


def resample_scheme_ref(cdf, values, lo, hi, n_out, scheme, seed, offset):
    """index [M, n_out] (int64) and value [M, n_out] (float32; None without values) of pp_is_resample_scheme_groups on a cdf [M, N]."""
    if scheme == MULTINOMIAL:
        return resample_ref(cdf, values, lo, hi, n_out, seed, offset)
    cdf = np.asarray(cdf, np.float64)
    M, N = cdf.shape
    index = np.full((M, n_out), -1, np.int64)
    p = positions_ref(M, n_out, scheme, seed, offset)
    for g in range(M):
        base = cdf[g, lo - 1] if lo > 0 else 0.0
        total = cdf[g, hi - 1] - base
        if total > 0 and np.isfinite(total):
            target = base + p[g] * total
            index[g] = np.minimum(lo + np.searchsorted(cdf[g, lo:hi], target, side='right'), hi - 1)
    value = None
    if values is not None:
        v = np.asarray(values, np.float32).reshape(M, N)
        value = np.where(index >= 0, np.take_along_axis(v, np.maximum(index, 0), 1), np.float32('nan')).astype(np.float32)
    return index, value


calls = {'is_hpd_groups': 0, 'is_ecdf_groups': 0, 'is_resample_scheme_groups': 0}      # how often the CPU doubles ran


def is_hpd_groups_cpu(value_sorted, cdf_sorted, counted, n_per, level):
    calls['is_hpd_groups'] += 1
    n = int(n_per)
    out, index = hpd_ref(value_sorted.numpy().reshape(-1, n), cdf_sorted.numpy().reshape(-1, n), counted.numpy(), level.numpy())
    return torch.from_numpy(out), torch.from_numpy(index)


def is_ecdf_groups_cpu(value_sorted, cdf_sorted, counted, n_per, x, strict):
    calls['is_ecdf_groups'] += 1
    n = int(n_per)
    out, rank = ecdf_ref(value_sorted.numpy().reshape(-1, n), cdf_sorted.numpy().reshape(-1, n), counted.numpy(), x.numpy(), bool(strict))
    return torch.from_numpy(out), torch.from_numpy(rank)


def is_resample_scheme_groups_cpu(cdf, values, n_per, lo, hi, n_out, scheme, seed, offset, want_index):
    calls['is_resample_scheme_groups'] += 1
    index, value = resample_scheme_ref(cdf.numpy().reshape(-1, int(n_per)), None if values is None else values.numpy(), int(lo),
                                       int(hi), int(n_out), int(scheme), int(seed), int(offset))
    return (torch.from_numpy(index.reshape(-1)) if want_index else torch.empty(0, dtype=torch.int64),
            torch.from_numpy(value.reshape(-1)) if value is not None else torch.empty(0, dtype=torch.float32))


_registered = False


def register_cpu_doubles():
    """The product has no CPU implementation of the operators: the tests register the numpy restatements as their CPU kernels."""
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_hpd_groups', is_hpd_groups_cpu, 'CPU')
        P._lib.impl('is_ecdf_groups', is_ecdf_groups_cpu, 'CPU')
        P._lib.impl('is_resample_scheme_groups', is_resample_scheme_groups_cpu, 'CPU')
        _registered = True
