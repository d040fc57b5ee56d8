"""Loaders of the CNN2D5C network goldens (tests/golden/make_cnn_golden.py: cnnl, cnnf). The convolution weights are not
stored: they are regenerated from the seed in the meta file (cnn_ref.seeded_cnn_params) and checked against the recorded
sums."""
import json
import os

import numpy as np

import cnn_ref
from conftest import GOLDEN

PREFIX = '_layers_observe_embedding.img.'


def load_cnn_golden(case):
    """(meta, params, batch, loss, isr) like conftest.load_golden; loss['g<i>'] includes the large gradients kept in their own
    files (cnnl)."""
    with open(os.path.join(GOLDEN, case + '_meta.json')) as f:
        meta = json.load(f)
    net = np.load(os.path.join(GOLDEN, case + '_net.npz'))
    stored = {n: net['p%d' % i] for i, n in enumerate(meta['stored_names'])}
    emb = meta['observe_embeddings']['img']
    gen = cnn_ref.seeded_cnn_params(emb['reshape'], emb['dim'], meta['cnn']['weight_seed'])
    for n, (s, q) in cnn_ref.param_checksums(gen).items():
        rs, rq = meta['cnn']['checksums'][n]
        assert abs(s - rs) <= 1e-9 * max(1.0, abs(rs)) and abs(q - rq) <= 1e-9 * max(1.0, rq), 'generator drift: ' + n
    params = {}
    for n in meta['state_dict_names']:
        if n in stored:
            params[n] = stored[n]
            if n.startswith(PREFIX):
                assert np.array_equal(stored[n], gen[n[len(PREFIX):]]), n
        else:
            assert n in meta['cnn']['generated'], n
            params[n] = gen[n[len(PREFIX):]]
    batch = dict(np.load(os.path.join(GOLDEN, case + '_batch.npz')))
    loss = dict(np.load(os.path.join(GOLDEN, case + '_loss.npz')))
    for n, fname in meta.get('large_grads', {}).items():
        loss['g%d' % meta['param_names'].index(n)] = np.load(os.path.join(GOLDEN, fname))['g']
    isr = dict(np.load(os.path.join(GOLDEN, case + '_is.npz')))
    return meta, params, batch, loss, isr


def observe_embeddings_from_meta(meta):
    from pyprob_amd import ObserveEmbedding
    out = {}
    for name in meta['obs_names']:
        v = dict(meta['observe_embeddings'][name])
        if 'embedding' in v:
            v['embedding'] = ObserveEmbedding[v['embedding']]
        out[name] = v
    return out


def spec_from_cnn_golden(meta):
    from pyprob_amd.spec import NetSpec
    spec = NetSpec(observe_embeddings_from_meta(meta), lstm_dim=meta['lstm_dim'] or 512,
                   proposal_mixture_components=meta['mixture_components'], network=meta['network'])
    for a, d in zip(meta['addresses'], meta['dist_names']):
        spec.add_address(a, d, 10 if d == 'Categorical' else None)
    return spec
