"""Float64 restatement of pp_is_hist_groups / pp_is_extent_groups (include/pyprob_amd.h) for the tests: the weights about the
maximum of the finite log-weights, the skipped particles, the bin rule (numpy.searchsorted(edges, x, 'right') - 1 with the last bin
closed), the slots, the fixed-point masses q = rint(w 2^S) summed as integers - and next to them the real-valued sums (in numpy.longdouble) the
derived bound |slot - sum w 2^S| <= 0.5 count + 2^-48 sum w 2^S is measured against; CPU doubles of the two operators with call counters."""
import numpy as np
import torch


def shift(n_per):
    """S = 62 - ceil(log2(n_per)): n_per 2^S <= 2^62."""
    return 62 - (int(n_per) - 1).bit_length()


def bins_of(edges, v):
    """Bin index of every v (no NaN among them) in strictly increasing edges [bins + 1]: -1 below, bins above, the last bin closed."""
    bins = len(edges) - 1
    b = np.searchsorted(edges, v, side='right') - 1
    return np.where(v < edges[0], -1, np.where(v > edges[-1], bins, np.minimum(b, bins - 1)))


def slots_of(x, y, ex, ey):
    """The slot of every particle: 1-D [bins ..., below, above, NaN]; 2-D [ix by + iy ..., outside, either NaN]."""
    bx = len(ex) - 1
    x = x.astype(np.float64)
    with np.errstate(invalid='ignore'):
        if y is None:
            b = bins_of(ex, np.where(np.isnan(x), ex[0], x))
            return np.where(np.isnan(x), bx + 2, np.where(b < 0, bx, np.where(b == bx, bx + 1, b))), bx + 3
        by = len(ey) - 1
        y = y.astype(np.float64)
        nan = np.isnan(x) | np.isnan(y)
        ix, iy = bins_of(ex, np.where(nan, ex[0], x)), bins_of(ey, np.where(nan, ey[0], y))
        out = (ix < 0) | (ix == bx) | (iy < 0) | (iy == by)
        return np.where(nan, bx * by + 1, np.where(out, bx * by, ix * by + iy)), bx * by + 2


def hist_ref(lw, x, y, edges_x, edges_y):
    """lw, x, y [M, N] (y None: 1-D), edges [bins + 1] shared or [M, bins + 1] -> (rows int64 [M, 2, slots], real [M, slots]): the
    output rows and, per slot, the real-valued sum of w 2^S, accumulated in numpy.longdouble (64 bits of mantissa where the host
    has them: the sum of n terms is then good to n 2^-64, far inside the 2^-48 of the bound). A particle whose lw is not finite is
    left out BEFORE its x / y enter anything."""
    lw = np.asarray(lw, np.float32)
    x = np.asarray(x, np.float32)
    y = None if y is None else np.asarray(y, np.float32)
    ex = np.asarray(edges_x, np.float64)
    ey = None if y is None else np.asarray(edges_y, np.float64)
    M, N = lw.shape
    S = shift(N)
    fin = np.isfinite(lw)
    l = lw.astype(np.float64)
    m = np.where(fin, l, -np.inf).max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.where(fin, np.exp(np.where(fin, l, 0.0) - np.where(np.isfinite(m), m, 0.0)), 0.0)
    if ex.ndim == 1 and (ey is None or ey.ndim == 1):
        slot, n_slots = slots_of(x.reshape(-1), None if y is None else y.reshape(-1), ex, ey)
        slot = slot.reshape(M, N)
    else:
        parts = [slots_of(x[g], None if y is None else y[g], ex[g] if ex.ndim == 2 else ex,
                          None if y is None else (ey[g] if ey.ndim == 2 else ey)) for g in range(M)]
        slot, n_slots = np.stack([p[0] for p in parts]), parts[0][1]
    flat = (np.arange(M)[:, None] * n_slots + slot)[fin]
    q = np.rint(np.minimum(w, 1.0) * 2.0 ** S).astype(np.int64)[fin]
    mass, count = np.zeros(M * n_slots, np.int64), np.zeros(M * n_slots, np.int64)
    real = np.zeros(M * n_slots, np.longdouble)
    np.add.at(mass, flat, q)
    np.add.at(count, flat, 1)
    np.add.at(real, flat, (w[fin] * 2.0 ** S).astype(np.longdouble))
    return np.stack([mass.reshape(M, n_slots), count.reshape(M, n_slots)], 1), real.reshape(M, n_slots)


def extent_ref(lw, x):
    """lw, x [M, N] -> [M, 4] float64: min x, max x over the particles with a finite lw and a non-NaN x, their number, and the
    number of particles with a finite lw whose x is NaN; nothing counted: +inf, -inf, 0, k."""
    lw = np.asarray(lw, np.float32)
    x = np.asarray(x, np.float32)
    fin = np.isfinite(lw)
    nan = np.isnan(x)
    ok = fin & ~nan
    v = x.astype(np.float64)
    return np.stack([np.where(ok, v, np.inf).min(axis=1), np.where(ok, v, -np.inf).max(axis=1), ok.sum(axis=1).astype(np.float64),
                     (fin & nan).sum(axis=1).astype(np.float64)], 1)


calls = {'is_hist_groups': 0, 'is_extent_groups': 0}      # how often the CPU doubles ran


def is_hist_groups_cpu(lw, x, y, n_per, edges_x, edges_y, stats):
    calls['is_hist_groups'] += 1
    n_per = int(n_per)
    rows, _ = hist_ref(lw.numpy().reshape(-1, n_per), x.numpy().reshape(-1, n_per), None if y is None else y.numpy().reshape(-1, n_per),
                       edges_x.numpy(), None if edges_y is None else edges_y.numpy())
    return torch.from_numpy(rows)


def is_extent_groups_cpu(lw, x, n_per):
    calls['is_extent_groups'] += 1
    return torch.from_numpy(extent_ref(lw.numpy().reshape(-1, int(n_per)), x.numpy().reshape(-1, int(n_per))))


_registered = False


def register_cpu_doubles():
    """The product has no CPU implementation of the operators: the tests register the float64 restatements as their CPU kernels."""
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('is_hist_groups', is_hist_groups_cpu, 'CPU')
        P._lib.impl('is_extent_groups', is_extent_groups_cpu, 'CPU')
        _registered = True
