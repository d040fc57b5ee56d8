"""Float64 restatement of pp_obs_draw (include/pyprob_amd.h) for the tests: a numpy Philox4x32-10 from the constants of
csrc/is_draw.hpp, the counter scheme of the header comment, and a CPU double of the `obs_draw` operator."""
import numpy as np
import torch

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed, c0, c1, c2, c3):
    """Four uint32 words per counter: key = (lo, hi) of `seed`, counter words c0..c3 (arrays of one shape, or scalars)."""
    x = [np.asarray(c, np.uint64) & _MASK for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * x[0], np.uint64(_M1) * x[2]
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ x[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(x, -1)


def _u01(w):
    """is_draw.hpp u01, in the kernel's fp32 arithmetic (the + 0.5 rounds to even above 2^23), as float64."""
    return ((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def _param(p, n, k):
    """A parameter shaped scalar, [k], [1, k], [n], [n, 1] or [n, k] as a float64 [n, k] array."""
    a = np.asarray(p.detach().cpu().numpy() if torch.is_tensor(p) else p, np.float64)
    if a.size == 1:
        return np.broadcast_to(a.reshape(1, 1), (n, k))
    if a.shape in ((k,), (1, k)):
        return np.broadcast_to(a.reshape(1, k), (n, k))
    if a.shape in ((n,), (n, 1)):
        return np.broadcast_to(a.reshape(n, 1), (n, k))
    assert a.shape == (n, k), (a.shape, n, k)
    return a


def obs_draw_ref(kind, p0, p1, n, k, seed, offset, stream_id):
    """out[r, e] of pp_obs_draw in float64: element group q = e >> 2 of row r takes the block of counter
    (lo(offset + r), hi(offset + r), stream_id, q); Uniform element e uses word e & 3; Normal elements 4q, 4q + 1 are the
    cos / sin branches of Box-Muller on words (0, 1), 4q + 2, 4q + 3 those on words (2, 3)."""
    a, b = _param(p0, n, k), _param(p1, n, k)
    g = (k + 3) // 4
    ctr = [(int(offset) + r) & 0xFFFFFFFFFFFFFFFF for r in range(n)]
    lo = np.asarray([c & 0xFFFFFFFF for c in ctr], np.uint64).reshape(n, 1)
    hi = np.asarray([c >> 32 for c in ctr], np.uint64).reshape(n, 1)
    w = philox4x32_10(seed, lo, hi, np.uint64(int(stream_id) & 0xFFFFFFFF), np.arange(g, dtype=np.uint64).reshape(1, g))    # [n, g, 4]
    if kind == 1:
        u = (w >> np.uint64(8)).astype(np.float64).reshape(n, 4 * g)[:, :k] / 16777216.0
        v = a + (b - a) * u
        return np.where(v.astype(np.float32) < b.astype(np.float32), v, a)      # the `v < b ? v : a` fold of [a, b)
    u = _u01(w).astype(np.float64)
    two_pi = float(np.float32(6.28318530717958647692))
    rad = np.sqrt(-2.0 * np.log(u[..., [0, 0, 2, 2]]))
    ang = (np.float32(two_pi) * u[..., [1, 1, 3, 3]].astype(np.float32)).astype(np.float64)      # fp32 product, as the kernel forms it
    z = rad * np.where(np.arange(4) % 2 == 0, np.cos(ang), np.sin(ang))
    return a + b * z.reshape(n, 4 * g)[:, :k]


calls = [0]      # how often the CPU double ran


def obs_draw_cpu(kind, p0, p1, n, k, seed, offset, stream_id):
    """The operator's CPU double (the product registers the device implementation only); counts its calls."""
    calls[0] += 1
    return torch.from_numpy(np.ascontiguousarray(obs_draw_ref(kind, p0, p1, n, k, seed, offset, stream_id), np.float32).reshape(n, k))


_registered = False


def register_cpu_double():
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('obs_draw', obs_draw_cpu, 'CPU')
        _registered = True
