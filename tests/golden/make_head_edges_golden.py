"""Record tests/golden/head_edges.npz: the reference's proposal heads on the saturated head outputs of
tests/head_edge_cases.py, once in float64 and once in float32 (the reference's own precision).

Per case the reference's proposal layer (pyprob/nn/proposal_*.py) runs with its feed-forward part replaced by the identity,
so that the case's y is what the layer's transforms receive; the layer returns the reference's Mixture / Categorical /
Bernoulli, whose log_prob scores the case's values; util.replace_negative_inf rescues -inf rows as `_loss` does
(inference_network_lstm.py:207-218) and torch autograd gives d sum(log_prob) / d y. The Bernoulli head is scored as `_loss`
scores it: the row's proposal against all n values of its sub-batch step (prior = (n, n1)), summed.

The float64 run is the yardstick of an fp32 computation, so it keeps the fp32 run's thresholds: util.to_tensor's default
dtype and the default dtype become float64, and util.clamp_probs / torch.distributions.utils.clamp_probs keep eps =
finfo(float32).eps (as written they would take finfo(float64).eps and never clamp). Nothing else is patched.

The file holds, per case name N: N_y, N_value, N_prior (inputs, fp32), N_lp64, N_dy64 (float64), N_lp32, N_dy32 (float32).
Runs only where the reference tree exists (default /root/reference; --reference PATH); the tests read the .npz alone.
"""
import argparse
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def reference_heads(reference='/root/reference'):
    """Import the reference and return run(case, dtype) -> (lp, dy) as numpy arrays of that dtype."""
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
    sys.path.insert(1, reference)
    import pyprob  # noqa: F401
    import pyprob.nn as RN
    from pyprob import util
    import torch.distributions.utils as TU
    torch.distributions.Distribution.set_default_validate_args(False)
    eps32 = torch.finfo(torch.float32).eps

    def clamp32(probs):
        return probs.clamp(min=eps32, max=1 - eps32)

    @contextlib.contextmanager
    def precision(dtype):
        saved = (util.to_tensor.__defaults__, util.clamp_probs, TU.clamp_probs, torch.get_default_dtype())
        try:
            if dtype == torch.float64:
                util.to_tensor.__defaults__ = (torch.float64,)
                util.clamp_probs = clamp32
                TU.clamp_probs = clamp32
                torch.set_default_dtype(torch.float64)
            yield
        finally:
            util.to_tensor.__defaults__, util.clamp_probs, TU.clamp_probs = saved[:3]
            torch.set_default_dtype(saved[3])

    def layer(case):
        head = case['head']
        if head == 'Normal':
            m = RN.ProposalNormalNormalMixture(4, mixture_components=case['K'])
        elif head == 'Uniform':
            m = RN.ProposalUniformTruncatedNormalMixture(4, mixture_components=case['K'])
        elif head == 'Poisson':
            m = RN.ProposalPoissonTruncatedNormalMixture(4, mixture_components=case['K'])
        elif head == 'Categorical':
            m = RN.ProposalCategoricalCategorical(4, num_categories=case['C'])
        else:
            m = RN.ProposalBernoulliBernoulli(4)
        m._ff = torch.nn.Identity()
        return m

    def run(case, dtype):
        np_dtype = np.float64 if dtype == torch.float64 else np.float32
        with precision(dtype), warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter('ignore')
            y = torch.tensor(case['y'], dtype=dtype, requires_grad=True)
            value = torch.tensor(case['value'], dtype=dtype)
            prior = torch.tensor(case['prior'], dtype=dtype)
            head = case['head']
            m = layer(case)
            if head == 'Bernoulli':
                lp = torch.zeros(y.shape[0], dtype=dtype)
                groups = sorted({(float(a), float(b)) for a, b in case['prior']})
                parts = []
                for cnt, ones in groups:
                    rows = torch.tensor(np.nonzero((case['prior'][:, 0] == cnt) & (case['prior'][:, 1] == ones))[0])
                    vals = torch.zeros(int(cnt), dtype=dtype)
                    vals[:int(ones)] = 1
                    dist = m.forward(y[rows], None)                  # probs [m, 1]
                    parts.append((rows, dist.log_prob(vals).sum(1)))    # [m, n] as in `_loss`, summed over the values
                for rows, part in parts:
                    lp = lp.index_add(0, rows, part)
            else:
                if head == 'Normal':
                    variables = [types.SimpleNamespace(distribution=types.SimpleNamespace(mean=p[0], stddev=p[1])) for p in prior]
                elif head == 'Uniform':
                    variables = [types.SimpleNamespace(distribution=types.SimpleNamespace(low=p[0], high=p[1])) for p in prior]
                else:
                    variables = [None] * y.shape[0]
                lp = m.forward(y, variables).log_prob(value)
            fixed = util.replace_negative_inf(lp)
            torch.sum(fixed).backward()
            return lp.detach().numpy().astype(np_dtype), y.grad.numpy().astype(np_dtype)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    from head_edge_cases import head_edge_cases
    run = reference_heads(args.reference)
    out = {}
    for name, case in head_edge_cases().items():
        lp64, dy64 = run(case, torch.float64)
        lp32, dy32 = run(case, torch.float32)
        out[name + '_y'] = case['y'].astype(np.float32)
        out[name + '_value'] = case['value'].astype(np.float32)
        out[name + '_prior'] = case['prior'].astype(np.float32)
        out[name + '_lp64'], out[name + '_dy64'] = lp64, dy64
        out[name + '_lp32'], out[name + '_dy32'] = lp32, dy32
        print('%-24s rows %4d  rescued %3d  non-finite lp64 %d lp32 %d dy64 %d dy32 %d' % (
            name, len(lp64), int(np.isneginf(lp64).sum()), int((~np.isfinite(lp64) & ~np.isneginf(lp64)).sum()),
            int((~np.isfinite(lp32) & ~np.isneginf(lp32)).sum()), int((~np.isfinite(dy64)).sum()), int((~np.isfinite(dy32)).sum())))
    path = os.path.join(HERE, 'head_edges.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
