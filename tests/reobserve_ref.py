"""pp_is_reobserve_groups restated in numpy (include/pyprob_amd.h states the formula): float32 for the bit contracts - the
composition of per-term log-densities, every operation rounded on its own -, float64 for accuracy, and a CPU double of the
`reobserve_groups` operator (the product registers the device implementation only)."""
import numpy as np
import torch

import obs_logweight_ref as OR

F32 = np.float32


def compose32(lw, old, lps, scales):
    """out [M, N] in float32 from lw [N], old [N] (or None), the terms' log-densities lps[t] [M, N] float32 and their scales:
    s_0 = +0, s_t = s_{t-1} + (scale_t * lp_t) (the product rounded, then the sum), out = lw + (s_T - old) (the difference rounded,
    then the sum), and lw itself where lw is not finite."""
    lw = np.asarray(lw, F32)
    old = np.zeros_like(lw) if old is None else np.asarray(old, F32)
    with np.errstate(all='ignore'):
        s = np.zeros(np.asarray(lps[0]).shape, F32)
        for lp, scale in zip(lps, scales):
            s = s + F32(scale) * np.asarray(lp, F32)
        out = lw[None, :] + (s - old[None, :])
    return np.where(np.isfinite(lw)[None, :], out, lw[None, :]).astype(F32)


def term_lp64(kind, params, x, M, N, k):
    """lp [M, N] float64 and the sum of |element terms| [M, N]: x [M, k] (or one row for all groups), params rows by particle."""
    ps = [OR.operand(q, N, k) for q in params[:OR.N_PARAMS[kind]]]      # [N, k]
    xs = OR.operand(x, M, k)                                            # [M, k]
    with np.errstate(all='ignore'):
        e = OR.elem_lp(kind, [p[None, :, :] for p in ps], xs[:, None, :])
        return e.sum(2), np.abs(e).sum(2)


def reobserve64(lw, old, terms, M):
    """float64 [M, N] of the definition; terms = [(kind, k, scale, params, x)] with float32 data."""
    lw = np.asarray(lw, np.float64)
    N = lw.size
    s = np.zeros((M, N))
    with np.errstate(all='ignore'):
        for kind, k, scale, params, x in terms:
            s = s + float(F32(scale)) * term_lp64(kind, params, x, M, N, k)[0]
        out = lw[None, :] + (s - (0.0 if old is None else np.asarray(old, np.float64)[None, :]))
    return np.where(np.isfinite(lw)[None, :], out, lw[None, :])


def reobserve_groups_cpu(lw, old, kinds, ks, scales, params, xs, n_groups):
    """The operator's CPU double: every term's log-density in float64 rounded to float32, then compose32."""
    M, N = int(n_groups), int(lw.numel())
    lps = [term_lp64(int(kind), list(params[4 * t:4 * t + 4]), xs[t], M, N, int(ks[t]))[0].astype(F32)
           for t, kind in enumerate(kinds)]
    out = compose32(lw.numpy(), None if old is None else old.numpy(), lps, scales)
    return torch.from_numpy(np.ascontiguousarray(out))


_registered = False


def register_cpu():
    global _registered
    if not _registered:
        from pyprob_amd import ops as P
        P._lib.impl('reobserve_groups', reobserve_groups_cpu, 'CPU')
        _registered = True
