#!/usr/bin/env python3
"""Generate the CNN2D5C golden vectors under tests/golden/ by RUNNING THE REFERENCE (pyprob v1.5.0) on CPU.

Runs only in the build container (needs /root/reference):

    python tests/golden/make_cnn_golden.py [unit]

Nothing from the reference is copied: its public classes are called and inputs / outputs recorded. Weights are never
stored: they come from tests/cnn_ref.py seeded_cnn_params(shape, dim, seed); the meta file holds the seed and, per
tensor, its float64 sum and sum of squares so that a drifting generator is caught. All images are selected by
cnn_ref.select_images (kink margin above CNN_KINK_MARGIN with the network's own weights).

  * cnn_unit.npz / cnn_unit_meta.json   pyprob.nn.EmbeddingCNN2D5C itself in float32, [1, 20, 20] at B = 32 (the
        smallest legal side) and [3, 21, 23] at B = 8 (several channels, odd sides, floor pooling): the images, a seeded
        upstream gradient, the features, the embedding, the gradient at the features, the bias gradients, and for each
        weight gradient its sums over the output-channel axis and over all other axes.
  * cnnl_*   InferenceNetworkLSTM, H = 64, an image observable 'img' [1, 20, 20] (CNN2D5C, dim 32) next to a scalar
        FEEDFORWARD observable 'y', a program with a Categorical(10) and a Normal address and traces of length 1 and 2,
        B = 32 traces whose images are replaced by margin-selected ones: the files of make_golden.py (<case>_meta.json,
        _net.npz WITHOUT the five convolution weights - those come from the seed in the meta file -, _batch.npz, _loss.npz
        with every gradient except the four large convolution gradients, _is.npz) and cnnl_gconv{2..5}.npz, one large
        gradient each.
  * cnnf_*   the same with InferenceNetworkFeedForward; no files for the four large gradients.

Before it writes, the script asserts that the float32 reference passes the tests' bars against tests/cnn_ref.py in
float64 on the same inputs and stores the per-tensor errors it saw in the meta file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
sys.path.insert(1, '/root/reference')
sys.path.insert(2, os.path.join(REPO, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import pyprob  # noqa: E402
from pyprob import Model, InferenceEngine, InferenceNetwork, ObserveEmbedding  # noqa: E402
from pyprob.distributions import Normal, Categorical, Mixture  # noqa: E402
from pyprob.nn import Batch, EmbeddingCNN2D5C  # noqa: E402

import cnn_ref  # noqa: E402

torch.set_num_threads(8)

GRAD_RTOL, GRAD_FLOOR = 1e-5, 5e-8     # helpers.grad_check(label, got, ref, 1e-5, 5e-8)
UNIT_CASES = [dict(key='s20', shape=[1, 20, 20], dim=32, B=32, weight_seed=11, image_seed=12, grad_seed=13),
              dict(key='c3', shape=[3, 21, 23], dim=32, B=8, weight_seed=21, image_seed=22, grad_seed=23)]


def rel_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def check_bar(label, got, ref, errors):
    ref = np.asarray(ref, np.float64)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    errors[label] = rel_err(got, ref)
    assert err <= GRAD_RTOL * np.abs(ref).max() + GRAD_FLOOR, (label, err, np.abs(ref).max())


def unit_case(c):
    shape, dim, B = c['shape'], c['dim'], c['B']
    params = cnn_ref.seeded_cnn_params(shape, dim, c['weight_seed'])
    images = cnn_ref.select_images(params, shape, B, c['image_seed'])
    gy = (np.random.default_rng(c['grad_seed']).standard_normal((B, dim)) / B).astype(np.float32)
    m = EmbeddingCNN2D5C(torch.Size(shape), torch.Size([dim]))
    m.load_state_dict({n: torch.from_numpy(v) for n, v in params.items()})
    x = torch.from_numpy(images)
    feat = m._forward_cnn(x.view(B, *shape)).view(B, -1)
    feat.retain_grad()
    emb = torch.relu(m._lin2(torch.relu(m._lin1(feat))))
    assert torch.equal(emb, m(x))
    emb.backward(torch.from_numpy(gy))
    ref = cnn_ref.forward_backward(params, images, shape, d_embedding=gy)
    errors = {}
    check_bar('features', feat.detach().numpy(), ref['features'], errors)
    check_bar('embedding', emb.detach().numpy(), ref['embedding'], errors)
    check_bar('d_features', feat.grad.numpy(), ref['d_features'], errors)
    out = {'images': images, 'd_embedding': gy, 'features': feat.detach().numpy(), 'embedding': emb.detach().numpy(),
           'd_features': feat.grad.numpy()}
    for n, p in m.named_parameters():
        g = p.grad.numpy()
        check_bar(n, g, ref['grads'][n], errors)
        if n.endswith('bias') or g.size <= 4096:
            out['g.' + n] = g
        else:
            out['gsum0.' + n] = g.astype(np.float64).sum(axis=0)
            out['gsumr.' + n] = g.astype(np.float64).reshape(g.shape[0], -1).sum(axis=1)
    meta = dict(c, margin=cnn_ref.CNN_KINK_MARGIN, checksums=cnn_ref.param_checksums(params),
                names=list(params.keys()), reference_f32_vs_f64=errors,
                min_margin=float(cnn_ref.kink_margin(params, images, shape).min()))
    print(c['key'], 'worst tensor error of the float32 reference: %.2e' % max(errors.values()))
    return out, meta


def make_unit():
    arrays, metas = {}, {}
    for c in UNIT_CASES:
        out, meta = unit_case(c)
        arrays.update({c['key'] + '.' + k: v for k, v in out.items()})
        metas[c['key']] = meta
    np.savez_compressed(os.path.join(HERE, 'cnn_unit.npz'), **arrays)
    metas['torch'] = torch.__version__
    with open(os.path.join(HERE, 'cnn_unit_meta.json'), 'w') as f:
        json.dump(metas, f, indent=1)


# ---- whole networks ---------------------------------------------------------------------------------------------------
IMG_SHAPE, IMG_DIM, NET_B = [1, 20, 20], 32, 32
LARGE = ('_conv2.weight', '_conv3.weight', '_conv4.weight', '_conv5.weight')     # gradients kept one file each (cnnl only)
CONV_W = tuple('_conv%d.weight' % l for l in range(1, 6))                        # weights never stored: from the seed


class DigitImage(Model):
    """d ~ Categorical(10); for d >= 5 also s ~ Normal(0, 1); a 20 x 20 image with a digit-dependent bar pattern plus
    Normal pixel noise and a scalar are observed: traces of one and of two controlled statements."""

    def __init__(self):
        super().__init__('Digit image')

    def forward(self):
        d = pyprob.sample(Categorical([0.1] * 10))
        s = pyprob.sample(Normal(0., 1.)) if int(d) >= 5 else torch.zeros(())
        yy, xx = torch.meshgrid(torch.arange(20.), torch.arange(20.), indexing='ij')
        mean = 0.5 + 0.4 * torch.sin((yy * (1 + int(d) % 5) + xx * (1 + int(d) // 5)) * 0.3 + s)
        pyprob.observe(Normal(mean, 0.1), name='img')
        pyprob.observe(Normal(d.float() + s, 1.0), name='y')
        return d


def prior_params(dist):
    if isinstance(dist, Normal):
        return [float(dist.mean), float(dist.stddev)]
    return [float(p) for p in dist.probs.view(-1)]


def net_case(case, network):
    print('=' * 30, case)
    weight_seed, image_seed = (41, 42) if network == 'lstm' else (51, 52)
    pyprob.seed(321 if network == 'lstm' else 322)
    model = DigitImage()
    obs_emb = {'img': {'dim': IMG_DIM, 'reshape': IMG_SHAPE, 'embedding': ObserveEmbedding.CNN2D5C}, 'y': {'dim': 8}}
    model.learn_inference_network(num_traces=64, batch_size=32, observe_embeddings=obs_emb,
                                  inference_network=(InferenceNetwork.LSTM if network == 'lstm' else InferenceNetwork.FEEDFORWARD),
                                  lstm_dim=64, proposal_mixture_components=10, learning_rate_init=1e-3, weight_decay=0.)
    net = model._inference_network
    net.train()
    # the image embedding's weights from the seed; images selected with those weights
    cnn_params = cnn_ref.seeded_cnn_params(IMG_SHAPE, IMG_DIM, weight_seed)
    net._layers_observe_embedding['img'].load_state_dict({n: torch.from_numpy(v) for n, v in cnn_params.items()})
    images = cnn_ref.select_images(cnn_params, IMG_SHAPE, NET_B, image_seed)

    gen = model._trace_generator(trace_mode=pyprob.TraceMode.PRIOR_FOR_INFERENCE_NETWORK)
    traces = [next(gen) for _ in range(NET_B)]
    assert {tr.length_controlled for tr in traces} == {1, 2}
    for tr, im in zip(traces, images):
        tr.named_variables['img'].value = torch.from_numpy(im).view(20, 20)
    batch = Batch(traces)
    net._polymorph(batch)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}

    rec = {'log_prob': []}
    sub_rec = []       # per sub-batch (_loss embeds one at a time): [image embedding, its gradient]
    orig_mix_lp, orig_cat_lp = Mixture.log_prob, Categorical.log_prob

    def mix_lp(self, value, sum=False):
        lp = orig_mix_lp(self, value, sum=sum)
        rec['log_prob'].append(lp.detach().numpy().copy().reshape(-1))
        return lp

    def cat_lp(self, value, sum=False):
        lp = orig_cat_lp(self, value, sum=sum)
        rec['log_prob'].append(lp.detach().numpy().copy().reshape(-1))
        return lp

    def emb_hook(m, i, o):
        slot = [o.detach().numpy().copy(), None]
        sub_rec.append(slot)
        o.register_hook(lambda g: slot.__setitem__(1, g.detach().numpy().copy()))

    hook = net._layers_observe_embedding['img'].register_forward_hook(emb_hook)
    Mixture.log_prob, Categorical.log_prob = mix_lp, cat_lp
    net.zero_grad()
    ok, loss = net._loss(batch)
    assert ok
    loss.backward()
    Mixture.log_prob, Categorical.log_prob = orig_mix_lp, orig_cat_lp
    hook.remove()
    names = [n for n, _ in net.named_parameters()]
    grads = {n: (p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(p.shape, np.float32))
             for n, p in net.named_parameters()}
    has_grad = [int(p.grad is not None) for _, p in net.named_parameters()]

    # the float32 reference against the float64 comparator on the same inputs: the image embedding of every sub-batch and
    # the gradients of its tensors (the comparator is driven with the reference's gradient at the embedding)
    index_of = {id(t): i for i, t in enumerate(traces)}
    errors = {}
    prefix = '_layers_observe_embedding.img.'
    ref_grads = {n: np.zeros(v.shape, np.float64) for n, v in cnn_params.items()}
    assert len(sub_rec) == len(batch.sub_batches)
    for sb, (e, de) in zip(batch.sub_batches, sub_rec):
        idx = np.array([index_of[id(t)] for t in sb])
        r = cnn_ref.forward_backward(cnn_params, images[idx], IMG_SHAPE, d_embedding=de)
        check_bar('embedding', e, r['embedding'], errors)
        for n in cnn_params:
            ref_grads[n] += r['grads'][n]
    for n in cnn_params:
        check_bar(n, grads[prefix + n], ref_grads[n], errors)
    print(case, 'worst tensor error of the float32 reference: %.2e' % max(errors.values()))

    # ---- files -------------------------------------------------------------------------------------------------------
    obs_names = list(obs_emb.keys())
    addresses, dist_names, trace_len, addr_idx, values, prior = [], [], [], [], [], []
    for tr in traces:
        trace_len.append(tr.length_controlled)
        for v in tr.variables_controlled:
            if v.address not in addresses:
                addresses.append(v.address)
                dist_names.append(v.distribution.name)
            addr_idx.append(addresses.index(v.address))
            values.append(float(v.value))
            prior.append(prior_params(v.distribution))
    width = max(len(p) for p in prior)
    prior_arr = np.zeros((len(prior), width), np.float32)
    for i, p in enumerate(prior):
        prior_arr[i, :len(p)] = p
    obs = np.stack([np.concatenate([np.asarray(tr.named_variables[n].value, np.float32).reshape(-1) for n in obs_names])
                    for tr in traces]).astype(np.float32)
    arrays = dict(trace_len=np.array(trace_len, np.int32), addr_idx=np.array(addr_idx, np.int32),
                  values=np.array(values, np.float32), prior=prior_arr, obs=obs)
    meta = dict(addresses=addresses, dist_names=dist_names, obs_names=obs_names)
    meta['sub_batches'] = [[index_of[id(t)] for t in sb] for sb in batch.sub_batches]
    meta['param_names'] = names
    meta['has_grad'] = has_grad
    meta['lstm_dim'] = 64 if network == 'lstm' else 0
    meta['lstm_depth'] = 1
    meta['network'] = network
    meta['mixture_components'] = 10
    meta['observe_embedding_dims'] = {k: v['dim'] for k, v in obs_emb.items()}
    meta['observe_embeddings'] = {'img': {'dim': IMG_DIM, 'reshape': IMG_SHAPE, 'embedding': 'CNN2D5C'}, 'y': {'dim': 8}}
    meta['obs_widths'] = [int(np.prod(IMG_SHAPE)), 1]
    meta['num_params'] = int(sum(p.numel() for p in net.parameters()))
    meta['cnn'] = dict(weight_seed=weight_seed, image_seed=image_seed, margin=cnn_ref.CNN_KINK_MARGIN,
                       checksums=cnn_ref.param_checksums(cnn_params), generated=[prefix + n for n in CONV_W],
                       reference_f32_vs_f64=errors,
                       min_margin=float(cnn_ref.kink_margin(cnn_params, images, IMG_SHAPE).min()))
    meta['python'], meta['torch'], meta['pyprob'] = sys.version.split()[0], torch.__version__, pyprob.__version__
    stored = [n for n in sd.keys() if n not in meta['cnn']['generated']]
    meta['state_dict_names'] = list(sd.keys())
    meta['stored_names'] = stored
    np.savez_compressed(os.path.join(HERE, case + '_net.npz'), **{'p%d' % i: sd[n] for i, n in enumerate(stored)})
    np.savez_compressed(os.path.join(HERE, case + '_batch.npz'), **arrays)
    loss_arrays = {'loss': np.array(float(loss), np.float64)}
    lp_index, k = [], 0
    for si, sb in enumerate(batch.sub_batches):
        for t in range(sb[0].length_controlled):
            loss_arrays['lp_%d_%d' % (si, t)] = rec['log_prob'][k]
            lp_index.append([si, t])
            k += 1
    assert k == len(rec['log_prob'])
    meta['large_grads'] = {}
    for i, n in enumerate(names):
        if n in [prefix + x for x in LARGE]:
            if network == 'lstm':
                f = '%s_g%s.npz' % (case, n[len(prefix) + 1:-len('.weight')])
                np.savez_compressed(os.path.join(HERE, f), g=grads[n])
                meta['large_grads'][n] = f
            continue
        loss_arrays['g%d' % i] = grads[n]
    np.savez_compressed(os.path.join(HERE, case + '_loss.npz'), **loss_arrays)
    meta['lp_index'] = lp_index
    print(case, 'loss', float(loss), 'params', meta['num_params'], 'sub-batches', len(batch.sub_batches))

    # ---- importance sampling with the inference network -----------------------------------------------------------------
    net.eval()
    steps = []
    orig_infer_step = net._infer_step

    def infer_step(variable, prev_variable=None, proposal_min_train_iterations=None):
        d = orig_infer_step(variable, prev_variable=prev_variable, proposal_min_train_iterations=proposal_min_train_iterations)
        steps.append((variable.address, d))
        return d

    net._infer_step = infer_step
    pyprob.seed(7)
    observe = {'img': torch.from_numpy(images[3]).view(20, 20), 'y': 6.3}
    rows = dict(trace_len=[], addr=[], value=[], prior=[], prior_lp=[], prop_lp=[], lw=[], obs_lw=[])
    gen = model._trace_generator(trace_mode=pyprob.TraceMode.POSTERIOR,
                                 inference_engine=InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK,
                                 inference_network=net, observe=observe)
    is_addresses = []
    with torch.no_grad():
        for _ in range(24):
            steps.clear()
            tr = next(gen)
            assert len(steps) == tr.length_controlled
            rows['trace_len'].append(tr.length_controlled)
            rows['lw'].append(float(tr.log_importance_weight))
            rows['obs_lw'].append(sum(float(v.log_importance_weight) for v in tr.variables_observed))
            for v, (addr, d) in zip(tr.variables_controlled, steps):
                if addr not in is_addresses:
                    is_addresses.append(addr)
                rows['addr'].append(is_addresses.index(addr))
                rows['value'].append(float(v.value))
                pp = prior_params(v.distribution)[:3]
                rows['prior'].append(pp + [0.0] * (3 - len(pp)))
                rows['prior_lp'].append(float(v.log_prob))
                rows['prop_lp'].append(float(d.log_prob(v.value, sum=True)))
    net._infer_step = orig_infer_step
    np.savez_compressed(os.path.join(HERE, case + '_is.npz'),
                        trace_len=np.array(rows['trace_len'], np.int32), addr=np.array(rows['addr'], np.int32),
                        value=np.array(rows['value'], np.float32), prior=np.array(rows['prior'], np.float32),
                        prior_lp=np.array(rows['prior_lp'], np.float64), prop_lp=np.array(rows['prop_lp'], np.float64),
                        lw=np.array(rows['lw'], np.float64), obs_lw=np.array(rows['obs_lw'], np.float64),
                        observe=np.concatenate([images[3], [6.3]]).astype(np.float32))
    meta['is_addresses'] = is_addresses
    with open(os.path.join(HERE, case + '_meta.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print(case, 'IS particles 24, mean lw', float(np.mean(rows['lw'])))


if __name__ == '__main__':
    only = sys.argv[1] if len(sys.argv) > 1 else None
    if only in (None, 'unit'):
        make_unit()
    if only in (None, 'cnnl'):
        net_case('cnnl', 'lstm')
    if only in (None, 'cnnf'):
        net_case('cnnf', 'feedforward')
