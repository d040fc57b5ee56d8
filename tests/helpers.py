"""Shared helpers of the parity tests: build an ICEngine / PackedBatch from the golden vectors, the importance-sampling test
engine and the term matrix of the fused posterior pass (pp_is_fused)."""
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


def _near_kink(x, W, b):
    """[n] bool: a unit of relu(x W^T + b) whose float64 pre-activation lies within KINK_MARGIN of zero, relative to the sum of
    |terms|."""
    z = x @ W.T + b
    return (np.abs(z) < KINK_MARGIN * (np.abs(x) @ np.abs(W).T + np.abs(b))).any(1)


def away_from_relu_kinks(eng, arrays, addresses, dist_names, n, embedding=False):
    """The first n traces of `arrays` whose proposal layer-0 pre-activations all lie further than KINK_MARGIN (relative to
    the sum of |terms|) from the ReLU kink in float64. Nearer, the fp32 summation order decides the ReLU mask, and a flipped
    unit moves every gradient upstream of it by the unit's whole contribution: measured on MI355X with trained-looking
    weights, one unit at a margin of 9e-9 in 277 000 put the head's dW0 3e-3 off on every path (tiles, both panels,
    PP_DETERMINISTIC=1) - a property of the data, not of a kernel. embedding=True: the same for every ReLU layer of the
    observe embedding (the observables' layers and the two final ones). A FeedForward network's heads read the observe
    embedding at every time step."""
    from oracle import ic_oracle as O
    params = {k: v.numpy() for k, v in eng.state_dict().items()}
    net = O.Net(params, [o[0] for o in eng.spec.obs], K=eng.spec.K)
    off = np.concatenate([[0], np.cumsum(arrays['trace_len'])])
    bad = np.zeros(len(arrays['trace_len']), bool)
    if eng.spec.feedforward:
        subs, _ = O.split_sub_batches(arrays['trace_len'], arrays['addr_idx'])
        E = O.embed_observe(net, np.asarray(arrays['obs'], np.float64))[0]
        heads_in = [np.broadcast_to(E[np.asarray(sb)], (int(arrays['trace_len'][sb[0]]), len(sb), E.shape[1])) for sb in subs]
    else:
        out = O.loss_and_grads(net, arrays, addresses, dist_names, want_grads=False)
        subs, heads_in = out['sub_batches'], out['lstm_out']
    for sb, hs in zip(subs, heads_in):
        sb = np.asarray(sb)
        for t in range(hs.shape[0]):
            Ws, bs = net.ff('_layers_proposal.%s._ff' % addresses[arrays['addr_idx'][off[sb[0]] + t]])
            bad[sb[_near_kink(hs[t], Ws[0], bs[0])]] = True
    if embedding:
        _, (caches, acts_final) = O.embed_observe(net, np.asarray(arrays['obs'], np.float64))
        for prefix, acts in [('_layers_observe_embedding.' + o[0], c) for o, c in zip(eng.spec.obs, caches)] + \
                            [('_layers_observe_embedding_final', acts_final)]:
            for x, W, b in zip(acts, *net.ff(prefix)):
                bad |= _near_kink(x, W, b)
    keep = np.nonzero(~bad)[0][:n]
    assert len(keep) == n, (len(keep), n)
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in keep])
    return dict(trace_len=arrays['trace_len'][keep], addr_idx=arrays['addr_idx'][rows], values=arrays['values'][rows],
                prior=arrays['prior'][rows], obs=arrays['obs'][keep])


# ---- the training step against the float64 oracle (tests/test_gpu_path.py, tests/test_gpu_depth.py) -------------------------------
# gradient bars against the float64 oracle: <= 10x the largest error measured on MI355X (profiles/r04_grad_errors.jsonl:
# 8.6e-7 relative on the single-statement shapes; 5.0e-9 ABSOLUTE on the ragged ones, whose gradients are ~1e-6)
GRAD_BAR = 1e-5
GRAD_ABS_RAGGED = 5e-8
# absolute floors of the trained-looking cases with TruncatedNormal heads, whose head gradients are sums over ~1 000 rows that
# cancel. Largest absolute error of a tensor beyond 1e-5 of its max |gradient|, measured on MI355X on the tile path
# (PP_PANEL=0) / with PP_DETERMINISTIC=1 / on the default path - the same on every path, so fp32 summation order:
#   single statements (GRAD_ABS_UNIFORM_TRAINED): K = 3 2.3e-8 / 2.1e-8 / 2.2e-8 (dW2 of the head, max 5e-5);
#     K = 15 5.8e-9 / 5.9e-9 / 5.5e-9; K = 16 5.4e-9 / 6.1e-9 / 5.4e-9
#   ragged GUMM (GRAD_ABS_RAGGED_TRAINED): H = 512 K = 1 5.2e-8 / 5.1e-8 / 5.2e-8 (dW2 of a head, max 5e-5);
#     H = 512 K = 16 8.1e-9 / 9.4e-9 / 8.1e-9; H = 256 depth 2 K = 16 4.6e-9 / 4.7e-9 / 4.6e-9
# (the ragged FeedForward cases keep GRAD_ABS_RAGGED: K = 1 3.8e-8, K = 16 1.3e-8 on all three paths)
GRAD_ABS_UNIFORM_TRAINED = 5e-8
GRAD_ABS_RAGGED_TRAINED = 1.5e-7
DEFAULT_OBS = {'obs0': {'dim': 32}, 'obs1': {'dim': 32}}


def unpack_lp(pb, lp_rows):
    """per-row log_prob (packed row order) -> trace-major order of the batch arrays"""
    out = np.empty(pb.n_rows, np.float64)
    out[pb.src_row] = lp_rows
    return out


def check_golden_step(case, meta, params, batch, loss):
    """One golden case through the C ABI against the reference's records: loss, per-row log_prob, every parameter gradient,
    the presence map and the status word."""
    import torch
    eng = engine_from_golden(meta, params)
    pb = packed_from_golden(meta, batch, eng.spec).to(eng.device)
    l, lp = eng.loss(pb, backward=True, keep_lp=True)
    torch.cuda.synchronize()
    assert int(eng.status_buf[0].item()) == 0
    ref_loss = float(loss['loss'])
    assert abs(float(l.item()) - ref_loss) <= 1e-5 * abs(ref_loss), (float(l.item()), ref_loss)
    # per-row log_prob against the reference's Mixture/Categorical.log_prob outputs
    lp_tm = unpack_lp(pb, lp.cpu().numpy())
    off = np.concatenate([[0], np.cumsum(batch['trace_len'])])
    for k, (si, t) in enumerate(meta['lp_index']):
        rows = off[np.array(meta['sub_batches'][si])] + t
        ref = loss['lp_%d_%d' % (si, t)]
        if ref.size == len(rows) ** 2 and len(rows) > 1:   # Bernoulli proposal: the reference's [n, n] broadcast matrix
            ref = ref.reshape(len(rows), len(rows)).sum(1)
        np.testing.assert_allclose(lp_tm[rows], ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref).max()))
    # every parameter gradient against loss.backward() of the reference
    # (the reference's gradients are fp32 themselves: the bar is 1e-5 of a tensor's largest element + the 5e-8 absolute fp32
    # summation floor of helpers.grad_check - measured against these goldens on MI355X: profiles/r06_grad_errors.jsonl)
    g = eng.grad_dict()
    for i, n in enumerate(meta['param_names']):
        ref = loss['g%d' % i]
        if not meta['has_grad'][i]:
            assert np.all(g[n] == 0), n
            continue
        grad_check('golden_%s/%s' % (case, n), g[n], ref, 1e-5, 5e-8)
    # presence map = which tensors had grad != None in the reference
    act = eng.presence().cpu().numpy()
    names = list(eng.spec.tensors.keys())
    ref_has = dict(zip(meta['param_names'], meta['has_grad']))
    assert [bool(a) for a in act] == [bool(ref_has[n]) for n in names]


def oracle_run(spec, params, arrays, addresses, dist_names, want_grads=True):
    from oracle import ic_oracle as O
    net = O.Net(params, [o[0] for o in spec.obs], K=spec.K)
    fn = O.loss_and_grads_feedforward if spec.feedforward else O.loss_and_grads
    return fn(net, arrays, addresses, dist_names, want_grads=want_grads)


def fresh_engine(lstm_dim, addresses, dist, seed=0, K=10, lstm_depth=1, network='lstm', extra=(), obs=None, device='cuda:0',
                 smp_dim=4, addr_dim=64, dtype_dim=8):
    """extra: (address, dist, num_categories) added after `addresses`. obs: the observe embeddings (DEFAULT_OBS).
    smp_dim / addr_dim / dtype_dim: the sample, address and distribution-type embedding widths (the reference's defaults).
    device='cpu': the engine's buffers on the host (tests/oracle_ops.py CpuBufferEngine) - the initialisation is numpy's, the
    weights are the same on either device."""
    spec = NetSpec(obs or DEFAULT_OBS, lstm_dim=lstm_dim, proposal_mixture_components=K, network=network, lstm_depth=lstm_depth,
                   sample_embedding_dim=smp_dim, address_embedding_dim=addr_dim, distribution_type_embedding_dim=dtype_dim)
    for a in addresses:
        spec.add_address(a, dist)
    for a, d, ncat in extra:
        spec.add_address(a, d, ncat)
    if device == 'cpu':
        import oracle_ops
        return oracle_ops.CpuBufferEngine(spec, seed=seed)
    from pyprob_amd.engine import ICEngine
    return ICEngine(spec, device=device, seed=seed)


def trained_looking(eng, seed):
    """LSTM and proposal weights x3 plus noisy biases (as test_gpu_is_step_fused._engine): the mixtures are far from uniform,
    so a wrong component index moves log_prob and not only the gradients."""
    rng = np.random.default_rng(seed)
    sd = {k: (v.numpy() * (3.0 if ('lstm' in k or 'proposal' in k) else 1.0)).astype(np.float32) for k, v in eng.state_dict().items()}
    for k in sd:
        if k.endswith('bias') or 'bias_' in k:
            sd[k] = (sd[k] + 0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
    eng.load_state_dict(sd)
    return eng


def packed(arrays, spec):
    from pyprob_amd.packed import PackedBatch
    return PackedBatch.from_ragged(arrays['trace_len'], arrays['addr_idx'], arrays['values'], arrays['prior'],
                                   arrays['obs'], len(spec.addresses))


def single_statement_arrays(B, dist, seed):
    """One statement per trace, values spread wider than the prior: Normal N(1, 2 sqrt5) under the prior N(1, sqrt5); Uniform
    U(-4, 6) with every 97th value outside the support (log_prob -inf -> rescued row); Poisson counts 0..40 (the head's
    TruncatedNormal mixture on the fixed [0, 40], pyprob_amd.packed.POISSON_LOW_HIGH)."""
    from pyprob_amd.packed import POISSON_LOW_HIGH
    arr = synthetic_gum_arrays(B, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if dist == 'Normal':
        arr['values'] = (1.0 + 2.0 * np.sqrt(5.0) * rng.standard_normal(B)).astype(np.float32)
    elif dist == 'Uniform':
        arr['prior'] = np.tile(np.array([[-4.0, 6.0]], np.float32), (B, 1))
        arr['values'] = rng.uniform(-4.0, 6.0, B).astype(np.float32)
        arr['values'][::97] = 7.5
    else:
        arr['prior'] = np.tile(np.array([POISSON_LOW_HIGH], np.float32), (B, 1))
        arr['values'] = rng.integers(0, 41, B).astype(np.float32)
    return arr


def oracle_lp_rows(out, arrays):
    """The oracle's log_prob lists (one per sub-batch and time step) -> one value per row of the trace-major arrays."""
    off = np.concatenate([[0], np.cumsum(arrays['trace_len'])])
    ref = np.full(int(off[-1]), np.nan)
    k = 0
    for sb in out['sub_batches']:
        sb = np.asarray(sb)
        for t in range(int(arrays['trace_len'][sb[0]])):
            ref[off[sb] + t] = out['lp'][k]
            k += 1
    assert k == len(out['lp']) and not np.isnan(ref).any()
    return ref


def check_lp(lp_tm, ref, label):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(lp_tm), fin), label
    np.testing.assert_allclose(lp_tm[fin], ref[fin], rtol=1e-4, atol=1e-4, err_msg=label)


def check_grads(label, eng, out, abs_floor=0.0, grads=None):
    """Every gradient tensor against the oracle's (GRAD_BAR of its largest element + abs_floor); a tensor the batch does not
    touch - identically zero in the oracle - is identically zero on the device. grads: the device gradients by name (default:
    the engine's current ones)."""
    g = eng.grad_dict() if grads is None else grads
    for n in eng.spec.tensors:
        if np.abs(out['grads'][n]).max() >= 1e-7:
            grad_check('%s/%s' % (label, n), g[n], out['grads'][n], GRAD_BAR, abs_floor)
        elif not np.any(out['grads'][n]):
            assert not np.any(g[n]), (label, n)        # a tensor the batch does not touch


def first_launch_workgroups(eng, pb):
    """Workgroups of the fused first launch (obs_embed.hip) that one step started: pp_debug_wgtrace mode 4 stamps them."""
    import torch
    from pyprob_amd import lib as L
    lib, cap = L.load(), 4096
    trace = torch.zeros(8 * cap, dtype=torch.int64, device=eng.device)
    torch.cuda.synchronize()
    lib.pp_debug_wgtrace(trace.data_ptr(), cap, 4)
    try:
        eng.loss(pb, backward=True)
        torch.cuda.synchronize()
    finally:
        lib.pp_debug_wgtrace(None, 0, 0)
    return int((trace.cpu().numpy().reshape(cap, 8)[:, 0] > 0).sum())


# ---- the importance-sampling test network (tests/test_gpu_is_step_fused.py, tests/test_gpu_is_fused_kernel.py) -----------------
IS_EMB = {'obs0': {'dim': 32}, 'obs1': {'dim': 32}}
IS_ADDRS = [('a_normal', 'Normal', None), ('a_uniform', 'Uniform', None), ('a_cat', 'Categorical', 7), ('a_poisson', 'Poisson', None),
            ('a_bern', 'Bernoulli', None)]


def is_engine(H, seed=0, depth=1, emb=None, K=10, addrs=IS_ADDRS, device='cuda:0', smp_dim=4, addr_dim=64, dtype_dim=8):
    """(engine, ISRunner, state dict) of a network with one address per proposal head and trained-looking weights.
    smp_dim / addr_dim / dtype_dim: the sample, address and distribution-type embedding widths (the reference's defaults).
    device='cpu': the engine's buffers on the host (tests/oracle_ops.py CpuBufferEngine; the operators are then the oracle-backed
    stand-ins) - the initialisation is numpy's, the weights are the same on either device."""
    from pyprob_amd.is_engine import ISRunner
    spec = NetSpec(emb or IS_EMB, lstm_dim=H, lstm_depth=depth, proposal_mixture_components=K, sample_embedding_dim=smp_dim,
                   address_embedding_dim=addr_dim, distribution_type_embedding_dim=dtype_dim)
    if device == 'cpu':
        import oracle_ops
        eng = oracle_ops.CpuBufferEngine(spec, seed=seed)
    else:
        from pyprob_amd.engine import ICEngine
        eng = ICEngine(spec, device=device, seed=seed)
    eng.add_addresses(addrs)
    rng = np.random.default_rng(seed + 1)
    # trained-looking weights: larger than the default initialisation so that gates and mixtures are not near-uniform
    sd = {k: (v.numpy() * (3.0 if ('lstm' in k or 'proposal' in k) else 1.0)).astype(np.float32) for k, v in eng.state_dict().items()}
    for k in sd:
        if k.endswith('bias') or 'bias_' in k:
            sd[k] = (sd[k] + 0.1 * rng.standard_normal(sd[k].shape)).astype(np.float32)
    eng.load_state_dict(sd)
    run = ISRunner(eng)
    run.init([8.0, 9.0])
    return eng, run, sd


# ---- the term matrix of pp_is_fused ------------------------------------------------------------------------------------------------
# A term on the host: dict(kind, p0, s0, p1, s1, x, scale, flags, out, label) - float32 arrays (None where the flag word says "the
# particle's value": the product passes no pointer there), strides as the C ABI reads them (Categorical: s0 = row stride, s1 = C),
# `out` = the particles PLANTED outside the term's support (the bookkeeping the reference is checked against).
# Per-term tolerance of tests/test_gpu_logweight.py::test_prior_log_prob_kernels_against_oracle (rtol = atol; Poisson 2e-5).
FUSED_TERM_TOL = {0: 1e-5, 1: 1e-5, 2: 1e-5, 3: 2e-5, 4: 1e-5, 5: 1e-5}
FUSED_SCALES = (1.0, -1.0, 0.37, -2.5)
FUSED_CAT = 12             # categories: a value in [5, 9] is a legal index (flag 4 on a Categorical term)
FUSED_PLANT_MIN_N = 128    # smaller runs carry no planted particles


def fused_values(n, rng):
    """The particles' values: positive, one sign, away from 0 (they also serve as sigma under flag 2)."""
    return rng.uniform(5.0, 9.0, n).astype(np.float32)


def fused_term(kind, n, rng, value, flags=0, per_p=0, per_x=0, scale=1.0, slot=0, per_p1=None, plant=True):
    """One term of kind 0 Normal / 1 Uniform / 2 identity / 3 Poisson / 4 Bernoulli / 5 Categorical. per_p / per_x: parameters / x
    per particle (stride 1; Categorical: n probability rows) or shared (stride 0); per_p1: the second parameter on its own.
    flags bit 1 / 2 / 4: p0 / p1 / x IS the particle's value. slot: moves the planted particles (and the shared constants) so
    that the terms of one call differ."""
    f32 = np.float32
    per_p1 = per_p if per_p1 is None else per_p1

    def vec(lo, hi):
        return rng.uniform(lo, hi, n).astype(f32)

    def one(v):
        return np.array([v], f32)
    assert not (flags & 3) or kind in (0, 1)
    p0 = p1 = x = None
    s0 = s1 = 0
    out = np.zeros(n, bool)
    base = 7 + 11 * slot
    planting = plant and n >= FUSED_PLANT_MIN_N
    if kind == 0:
        p0, s0 = (vec(5.5, 8.5), 1) if per_p else (one(6.5 + 0.125 * slot), 0)
        p1, s1 = (vec(1.0, 3.0), 1) if per_p1 else (one(1.3 + 0.2 * slot), 0)      # sigma positive and away from 0
        x = vec(5.0, 9.0) if per_x else one(7.25 - 0.25 * slot)
    elif kind == 1:
        assert (flags & 3) != 3, 'low = high = value: an empty interval'
        # low < x < high whichever of them is the particle's value (in [5, 9])
        xl, xh = (9.25, 9.9) if flags & 1 else ((3.5, 4.9) if flags & 2 else (4.0, 9.5))
        p0, s0 = (vec(0.0, 3.0), 1) if per_p else (one(2.0), 0)
        p1, s1 = (vec(10.0, 14.0), 1) if per_p1 else (one(12.0), 0)
        x = vec(xl, xh) if per_x else one(0.5 * (xl + xh))
        if (flags & 6) == 6:
            out[:] = True      # x = high = value: outside [low, high) everywhere
        elif planting:
            # x == low (inside), x == high (outside), x > high (outside): written into whichever side is a per-particle array
            def eff(a, s, bit):
                return value if flags & bit else (a if s else np.full(n, a[0], f32))
            lo_e, hi_e, x_e = eff(p0, s0, 1), eff(p1, s1, 2), eff(x, per_x, 4)
            x_mod, lo_mod, hi_mod = per_x and not flags & 4, s0 == 1 and not flags & 1, s1 == 1 and not flags & 2
            i = base
            if x_mod:
                x[i] = lo_e[i]
            elif lo_mod:
                p0[i] = x_e[i]
            i = base + 1
            if x_mod:
                x[i], out[i] = hi_e[i], True
            elif hi_mod and x_e[i] > lo_e[i]:
                p1[i], out[i] = x_e[i], True
            i = base + 2
            if x_mod:
                x[i], out[i] = hi_e[i] + f32(1.5), True
            elif hi_mod and x_e[i] > lo_e[i]:
                mid = f32(0.5) * (lo_e[i] + x_e[i])
                if lo_e[i] < mid < x_e[i]:
                    p1[i], out[i] = mid, True
    elif kind == 2:
        x = vec(-3.0, 3.0) if per_x else one(0.75 + slot)
    elif kind == 3:
        p0, s0 = (vec(0.2, 9.0), 1) if per_p else (one(4.2), 0)
        if per_x:      # counts and reals, zeros among them
            x = np.where(rng.random(n) < 0.5, rng.poisson(4.0, n), rng.uniform(0.0, 12.0, n)).astype(f32)
            x[::7] = 0.0
        else:
            x = one(3.0)
    elif kind == 4:
        p0, s0 = (vec(0.0, 1.0), 1) if per_p else (one(0.3), 0)
        if per_p and n >= 3:
            p0[:3] = [0.0, 1.0, 0.5]      # clamped to [eps, 1 - eps]
        x = (rng.random(n) < 0.5).astype(f32) if per_x else one(1.0)
    elif kind == 5:
        C = FUSED_CAT
        s1 = C
        p0, s0 = (rng.uniform(0.01, 1.0, (n, C)).astype(f32).reshape(-1), C) if per_p else (rng.uniform(0.01, 1.0, C).astype(f32), 0)
        if per_x:
            x = rng.integers(0, C, n).astype(f32)
            x[1::5] += f32(0.4)           # the index is the truncated value
            if planting and not flags & 4:
                x[base], out[base] = C, True
                x[base + 1], out[base + 1] = -1.0, True
                x[base + 2], out[base + 2] = C + 0.5, True
                x[base + 3] = C - 1
        else:
            x = one(3.0)
    else:
        raise ValueError(kind)
    if flags & 1:
        p0, s0 = None, 0
    if flags & 2:
        p1, s1 = None, 0
    if flags & 4:
        x = None
    label = 'kind%d flags%d p%s%s x%s scale%g' % (kind, flags, 'n' if per_p else '1', 'n' if per_p1 else '1',
                                                   'v' if flags & 4 else ('n' if per_x else '1'), scale)
    return dict(kind=kind, p0=p0, s0=s0, p1=p1, s1=s1, x=x, scale=float(f32(scale)), flags=flags, out=out, label=label)


def fused_single_term_cases(n, rng, value):
    """Every term kind x parameters shared / per particle x `x` shared / per particle / the value x every legal flag word:
    bit 4 on all kinds, bits 1 and 2 on Normal and Uniform (not both on a Uniform: low = high = value is an empty interval, which
    torch's Uniform rejects and whose float64 log-density is log 0 - log 0). Scales cycle through FUSED_SCALES."""
    cases = []
    for kind in range(6):
        flag_words = range(8) if kind == 0 else ((0, 1, 2, 4, 5, 6) if kind == 1 else (0, 4))
        for flags in flag_words:
            for per_p in (0, 1):
                for per_x in (0, 1):
                    if (flags & 4 and per_x) or (kind == 2 and per_p) or ((flags & 3) == 3 and per_p):
                        continue      # (the array would not be read)
                    cases.append(fused_term(kind, n, rng, value, flags, per_p, per_x, FUSED_SCALES[len(cases) % 4], slot=len(cases) % 8))
    return cases


def fused_mixed_sets(n, rng, value):
    """Calls of eight terms (the ABI's maximum). The first seven terms of `lean`, `general_poisson` and `general_sigma` are the
    SAME Normal / identity terms (one scale per term for all particles: the LEAN instantiation takes them); the eighth makes the
    call all-LEAN or general, so both instantiations evaluate the same Normal terms. `all_kinds`: every kind, per-particle
    sigma, sigma = value, Uniform bounds = value, planted out-of-support particles (at different particles per term)."""
    def common():
        r = np.random.default_rng(11)      # the same seven terms in every set
        return [fused_term(0, n, r, value, 0, per_p=1, per_x=0, scale=1.0, slot=0, per_p1=0),
                fused_term(0, n, r, value, 1, per_p=0, per_x=0, scale=1.0, slot=1),          # an observe: Normal(value, s), y
                fused_term(0, n, r, value, 4, per_p=0, per_x=0, scale=-1.0, slot=2),         # a prior: Normal(m, s) at the value
                fused_term(0, n, r, value, 0, per_p=1, per_x=1, scale=0.37, slot=3, per_p1=0),
                fused_term(0, n, r, value, 1, per_p=0, per_x=1, scale=-2.5, slot=4),
                fused_term(2, n, r, value, 0, per_x=1, scale=-1.0, slot=5),                  # - log q of an earlier statement
                fused_term(0, n, r, value, 4, per_p=1, per_x=0, scale=1.0, slot=6, per_p1=0)]
    sets = {
        'lean': common() + [fused_term(2, n, rng, value, 0, per_x=0, scale=0.37, slot=7)],
        'general_poisson': common() + [fused_term(3, n, rng, value, 0, per_p=1, per_x=1, scale=1.0, slot=7)],
        'general_sigma': common() + [fused_term(0, n, rng, value, 0, per_p=1, per_x=1, scale=1.0, slot=7)],
        'all_kinds': [fused_term(0, n, rng, value, 0, per_p=1, per_x=1, scale=1.0, slot=0),
                      fused_term(0, n, rng, value, 2, per_p=0, per_x=1, scale=0.37, slot=1),
                      fused_term(1, n, rng, value, 1, per_p=1, per_x=1, scale=1.0, slot=2),
                      fused_term(1, n, rng, value, 4, per_p=1, per_x=0, scale=1.0, slot=3),
                      fused_term(3, n, rng, value, 4, per_p=1, per_x=0, scale=-1.0, slot=4),
                      fused_term(4, n, rng, value, 0, per_p=1, per_x=1, scale=-2.5, slot=5),
                      fused_term(5, n, rng, value, 0, per_p=1, per_x=1, scale=-1.0, slot=6),
                      fused_term(2, n, rng, value, 4, scale=1.0, slot=7)],
    }
    for name in ('lean', 'general_poisson', 'general_sigma'):
        lean = all(t['kind'] == 2 or (t['kind'] == 0 and not t['flags'] & 2 and t['s1'] == 0) for t in sets[name])
        assert lean == (name == 'lean'), name      # pp_is_fused's own rule for the LEAN instantiation
        assert sum(not (t['kind'] == 2 or (t['kind'] == 0 and not t['flags'] & 2 and t['s1'] == 0)) for t in sets[name]) <= 1
    return sets


def fused_term_refs(terms, value):
    """Float64 log-density of every term at every particle: oracle_ops._term (the CPU stand-in's restatement on the oracle) on the
    fp32 inputs, the flagged arguments replaced by the particles' values. Asserts the out-of-support bookkeeping: the
    reference is -inf exactly at the planted particles and finite everywhere else."""
    import torch
    import oracle_ops
    n = len(value)
    tv = torch.from_numpy(value)
    refs = []
    for t in terms:
        f = t['flags']
        a0, s0 = (tv, 1) if f & 1 else (None if t['p0'] is None else torch.from_numpy(t['p0']), t['s0'])
        a1, s1 = (tv, 1) if f & 2 else (None if t['p1'] is None else torch.from_numpy(t['p1']), t['s1'])
        xx = tv if f & 4 else torch.from_numpy(t['x'])
        with np.errstate(divide='ignore'):
            r = np.asarray(oracle_ops._term(t['kind'], a0, s0, a1, s1, xx, n), np.float64).reshape(n)
        assert np.array_equal(np.isneginf(r), t['out']), (t['label'], np.nonzero(np.isneginf(r) != t['out'])[0][:8])
        assert np.isfinite(r[~t['out']]).all(), t['label']
        refs.append(r)
    return refs


def fused_sum_ref(terms, value, lw0, overwrite):
    """(float64 log-weight, tolerance) per particle: lw0 (unless overwritten) + sum_t scale_t ref_t, the tolerance of a sum =
    sum_t |scale_t| x the per-term tolerance tol_t (1 + |ref_t|) (non-finite terms add none: their pattern is compared)."""
    n = len(value)
    ref = np.zeros(n) if overwrite else lw0.astype(np.float64)
    tol = np.zeros(n)
    for t, r in zip(terms, fused_term_refs(terms, value)):
        with np.errstate(invalid='ignore'):
            ref = ref + t['scale'] * r
        tol += abs(t['scale']) * FUSED_TERM_TOL[t['kind']] * (1.0 + np.where(np.isfinite(r), np.abs(r), 0.0))
    assert not np.isnan(ref).any()
    return ref, tol


def _t(a, dev):
    import torch
    return None if a is None else torch.tensor(a, dtype=torch.float32, device=dev)


def fused_device_terms(terms, dev):
    """The host terms as ISRunner.fused reads them: [((kind, p0, s0, p1, s1), x, scale, flags)] on `dev`."""
    return [((t['kind'], _t(t['p0'], dev), t['s0'], _t(t['p1'], dev), t['s1']), _t(t['x'], dev), t['scale'], t['flags']) for t in terms]


def run_fused_terms(run, terms, value, lw0, overwrite):
    """pp_is_fused with the values given (no draw): returns the log-weights; the values must come back bit-unchanged."""
    n = len(value)
    run.begin(n)
    tv, tl = _t(value, run.dev), _t(lw0, run.dev)
    run.fused(None, None, fused_device_terms(terms, run.dev), tv, tl, overwrite)
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), value.view(np.uint32))
    return tl.cpu().numpy()


def run_per_term_kernels(run, terms, value, lw0, overwrite):
    """The same terms through pp_logweight_terms in calls of at most four (it has no flag word: the value vector is passed
    where a flag says so)."""
    tv, tl = _t(value, run.dev), _t(lw0, run.dev)
    for lo in range(0, len(terms), 4):
        items = []
        for t in terms[lo:lo + 4]:
            f = t['flags']
            p0, s0 = (tv, 1) if f & 1 else (_t(t['p0'], run.dev), t['s0'])
            p1, s1 = (tv, 1) if f & 2 else (_t(t['p1'], run.dev), t['s1'])
            items.append(((t['kind'], p0, s0, p1, s1), tv if f & 4 else _t(t['x'], run.dev), t['scale']))
        run.accumulate_terms(tl, items, overwrite=overwrite and lo == 0)
    return tl.cpu().numpy()


def check_fused_terms(run, terms, value, rng, label=''):
    """One call of pp_is_fused (values given) with `terms`, overwriting and accumulating onto a random lw, against the float64
    sum of the terms and against the per-term kernels (rtol = atol = 1e-5, tests/test_gpu_is_fused.py). Infinite results must
    sit exactly where the reference has them."""
    n = len(value)
    lw0 = (3.0 * rng.standard_normal(n)).astype(np.float32)
    for overwrite in (True, False):
        ref, tol = fused_sum_ref(terms, value, lw0, overwrite)
        got = run_fused_terms(run, terms, value, lw0, overwrite)
        what = (label, [t['label'] for t in terms], 'overwrite' if overwrite else 'accumulate')
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)), what
        assert not np.isnan(got).any(), what
        ok = np.isfinite(ref)
        err = np.abs(got[ok].astype(np.float64) - ref[ok])
        assert (err <= tol[ok]).all(), what + (float((err / tol[ok]).max()), int(np.nonzero(ok)[0][(err / tol[ok]).argmax()]))
        per_term = run_per_term_kernels(run, terms, value, lw0, overwrite)
        assert np.array_equal(np.isneginf(per_term), np.isneginf(ref)) and np.array_equal(np.isposinf(per_term), np.isposinf(ref)), what
        np.testing.assert_allclose(got[ok], per_term[ok], rtol=1e-5, atol=1e-5, err_msg=str(what))
