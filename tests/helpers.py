"""Shared helpers of the parity tests: build an ICEngine / PackedBatch from the golden vectors."""
import numpy as np

from pyprob_amd.spec import NetSpec


def spec_from_golden(meta, params):
    depths = meta.get('observe_embedding_depths', {})
    obs = {n: {'dim': meta['observe_embedding_dims'][n], 'input_dim': 1, 'depth': depths.get(n, 2)} for n in meta['obs_names']}
    spec = NetSpec(obs, lstm_dim=meta['lstm_dim'], proposal_mixture_components=meta['mixture_components'],
                   network=meta.get('network', 'lstm'), lstm_depth=meta.get('lstm_depth', 1))
    pairs = list(zip(meta['addresses'], meta['dist_names']))
    # addresses the network knows but this batch does not contain (GUMM): dist type from the address suffix
    for k in params:
        if k.startswith('_layers_proposal.') and k.endswith('._ff._layers.0.weight'):
            a = k[len('_layers_proposal.'):-len('._ff._layers.0.weight')]
            if a not in meta['addresses']:
                suffix = a.split('__')[-2]
                pairs.append((a, [d for d in ('Normal', 'Uniform', 'Categorical', 'Poisson', 'Bernoulli') if suffix.startswith(d)][0]))
    for a, d in pairs:
        ncat = None
        if d == 'Categorical':
            ncat = params['_layers_proposal.%s._ff._layers.1.weight' % a].shape[0]
        spec.add_address(a, d, ncat)
    return spec


def engine_from_golden(meta, params, device='cuda:0'):
    from pyprob_amd.engine import ICEngine
    spec = spec_from_golden(meta, params)
    eng = ICEngine(spec, device=device, seed=0)
    assert set(spec.tensors.keys()) == set(params.keys()), set(spec.tensors.keys()) ^ set(params.keys())
    for n in spec.tensors:
        assert spec.tensors[n][1] == params[n].shape, (n, spec.tensors[n][1], params[n].shape)
    eng.load_state_dict(params)
    return eng


def packed_from_golden(meta, batch, spec):
    from pyprob_amd.packed import PackedBatch
    from pyprob_amd.packed import bernoulli_group_stats
    ids = np.array([spec.address_id[meta['addresses'][i]] for i in batch['addr_idx']], np.int64)
    prior = head_prior(meta, batch['addr_idx'], batch['prior'])
    bernoulli = [a for a, info in enumerate(spec.addresses) if info.dist_name == 'Bernoulli']
    if bernoulli:
        prior = bernoulli_group_stats(batch['trace_len'], ids, batch['values'], prior, bernoulli)
    return PackedBatch.from_ragged(batch['trace_len'], ids, batch['values'], prior, batch['obs'], len(spec.addresses))


def head_prior(meta, addr_idx, prior, dist_names=None):
    """Prior parameters as the proposal heads read them: the golden files hold the prior's own parameters (Poisson:
    the rate), the Poisson head works on the fixed interval [0, 40] (pyprob_amd.packed.distribution_params)."""
    from pyprob_amd.packed import POISSON_LOW_HIGH
    names = np.asarray(meta['dist_names'] if dist_names is None else dist_names)[np.asarray(addr_idx)]
    out = np.zeros((len(prior), 2), np.float32)
    w = min(2, prior.shape[1])
    out[:, :w] = prior[:, :w]
    out[names == 'Poisson'] = POISSON_LOW_HIGH
    return out


def rel_err(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12))


def grad_check(label, got, ref, bar, abs_floor=0.0):
    """Gradient tensor against the float64 oracle: max |got - ref| < bar * max |ref| + abs_floor. The bars of the callers are
    <= 10x the error MEASURED on MI355X (profiles/r04_grad_errors.jsonl, recorded with PP_TEST_RECORD_ERRORS=<file>: every
    check appends its error there), not a generic tolerance: a dropped small contribution shows up. abs_floor: the ragged
    cases run on freshly initialised networks whose gradients are ~1e-6 - their fp32 summation error (measured 5e-9, the
    same absolute size as in the cases with gradients of 1e-2) is not small RELATIVE to such a tensor."""
    import json
    import os
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    abs_err = float(np.abs(got - ref).max())
    ref_max = float(np.abs(ref).max())
    path = os.environ.get('PP_TEST_RECORD_ERRORS')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(check=label, err=abs_err / max(ref_max, 1e-30), abs_err=abs_err, bar=bar, abs_floor=abs_floor,
                                    ref_max=ref_max)) + '\n')
        return abs_err
    assert abs_err < bar * ref_max + abs_floor, (label, abs_err, ref_max, bar, abs_floor)
    return abs_err


def synthetic_gum_arrays(n, seed=0):
    """GaussianUnknownMean prior traces in trace-major arrays: mu ~ N(1, sqrt5), y0,y1 ~ N(mu, sqrt2)
    (the model of the reference's tests/test_inference.py:97-109)."""
    rng = np.random.default_rng(seed)
    mu = (1.0 + np.sqrt(5.0) * rng.standard_normal(n)).astype(np.float32)
    obs = (mu[:, None] + np.sqrt(2.0) * rng.standard_normal((n, 2))).astype(np.float32)
    prior = np.tile(np.array([[1.0, np.sqrt(5.0)]], np.float32), (n, 1))
    return dict(trace_len=np.ones(n, np.int32), addr_idx=np.zeros(n, np.int32), values=mu, prior=prior, obs=obs)


def synthetic_cat_arrays(n, C, seed=0):
    """Categorical-then-Normal traces at any width C (the `cat` golden's program, tests/golden/make_golden.py
    CategoricalThenNormal, has C = 3): c ~ U{0..C-1} with every category present (n >= C), mu under the prior
    N(4 c / (C - 1) - 1, 1.5) (= 2 c - 1 at C = 3) but drawn twice as wide, two observations N(mu, 0.8).
    Returns arrays + address list."""
    assert n >= C
    rng = np.random.default_rng(seed)
    c = rng.integers(0, C, n)
    c[rng.permutation(n)[:C]] = np.arange(C)
    m = 4.0 * c / max(C - 1, 1) - 1.0
    mu = m + 3.0 * rng.standard_normal(n)
    obs = mu[:, None] + 0.8 * rng.standard_normal((n, 2))
    prior = np.zeros((2 * n, 2), np.float32)
    prior[1::2, 0], prior[1::2, 1] = m, 1.5
    addresses = ['c__Categorical(len_probs:%d)__1' % C, 'mu__Normal__1']
    return dict(trace_len=np.full(n, 2, np.int32), addr_idx=np.tile(np.array([0, 1], np.int32), n),
                values=np.stack([c, mu], 1).reshape(-1).astype(np.float32), prior=prior, obs=obs.astype(np.float32)), addresses


def chi2_p(counts, probs):
    """Pearson chi-square p-value of category counts against probabilities; categories expected fewer than 5 times are
    pooled into one bin."""
    import torch
    n = counts.sum()
    e = probs * n
    keep = e >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(e[keep], n - e[keep].sum())
    if exp[-1] < 5:
        obs, exp = obs[:-1], exp[:-1]
        obs[-1] += counts[~keep].sum()
        exp[-1] = n - exp[:-1].sum()
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    df = len(obs) - 1
    return float(torch.special.gammaincc(torch.tensor(df / 2, dtype=torch.float64), torch.tensor(chi2 / 2, dtype=torch.float64)))


def synthetic_gumm_arrays(n, seed=0, max_iter=6):
    """GaussianUnknownMeanMarsaglia traces (tests/test_inference.py:252-275): pairs x,y ~ U(-1,1) until
    x^2+y^2 < 1; addresses alternate x_k, y_k with k the loop iteration. Returns arrays + address list."""
    rng = np.random.default_rng(seed)
    trace_len, addr_idx, values, obs = [], [], [], []
    for _ in range(n):
        k = 0
        while True:
            x, y = rng.uniform(-1, 1, 2)
            addr_idx += [2 * k, 2 * k + 1]
            values += [x, y]
            k += 1
            s = x * x + y * y
            if s < 1 or k >= max_iter:
                break
        if s >= 1:
            s = 0.5
        trace_len.append(2 * k)
        mu = 1.0 + np.sqrt(5.0) * x * np.sqrt(-2 * np.log(s) / s)
        obs.append(mu + np.sqrt(2.0) * rng.standard_normal(2))
    R = len(values)
    prior = np.tile(np.array([[-1.0, 1.0]], np.float32), (R, 1))
    n_addr = 2 * max_iter
    addresses = ['a%d__%s__Uniform__%d' % (i, 'xy'[i % 2], i // 2 + 1) for i in range(n_addr)]
    return dict(trace_len=np.array(trace_len, np.int32), addr_idx=np.array(addr_idx, np.int32),
                values=np.array(values, np.float32), prior=prior, obs=np.array(obs, np.float32)), addresses


KINK_MARGIN = 2e-6


def away_from_relu_kinks(eng, arrays, addresses, dist_names, n):
    """The first n traces of `arrays` whose proposal layer-0 pre-activations all lie further than KINK_MARGIN (relative to
    the sum of |terms|) from the ReLU kink in float64. Nearer, the fp32 summation order decides the ReLU mask, and a flipped
    unit moves every gradient upstream of it by the unit's whole contribution: measured on MI355X with trained-looking
    weights, one unit at a margin of 9e-9 in 277 000 put the head's dW0 3e-3 off on every path (tiles, both panels,
    PP_DETERMINISTIC=1) - a property of the data, not of a kernel."""
    from oracle import ic_oracle as O
    params = {k: v.numpy() for k, v in eng.state_dict().items()}
    net = O.Net(params, [o[0] for o in eng.spec.obs], K=eng.spec.K)
    out = O.loss_and_grads(net, arrays, addresses, dist_names, want_grads=False)
    off = np.concatenate([[0], np.cumsum(arrays['trace_len'])])
    bad = np.zeros(len(arrays['trace_len']), bool)
    for sb, hs in zip(out['sub_batches'], out['lstm_out']):
        sb = np.asarray(sb)
        for t in range(hs.shape[0]):
            Ws, bs = net.ff('_layers_proposal.%s._ff' % addresses[arrays['addr_idx'][off[sb[0]] + t]])
            z = hs[t] @ Ws[0].T + bs[0]
            bad[sb[(np.abs(z) < KINK_MARGIN * (np.abs(hs[t]) @ np.abs(Ws[0]).T + np.abs(bs[0]))).any(1)]] = True
    keep = np.nonzero(~bad)[0][:n]
    assert len(keep) == n, (len(keep), n)
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in keep])
    return dict(trace_len=arrays['trace_len'][keep], addr_idx=arrays['addr_idx'][rows], values=arrays['values'][rows],
                prior=arrays['prior'][rows], obs=arrays['obs'][keep])
