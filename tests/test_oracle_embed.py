"""The oracle's observe embedding (oracle/ic_oracle.py embed_observe) with VECTOR observables, against torch autograd in float64:
observable j reads the w_j columns behind those of the observables before it, w_j the input width of its first layer. The stack
is the reference's (pyprob/nn/inference_network.py:80-139): per observable Linear-ReLU-Linear-ReLU, concat, two e x e
Linear-ReLU. The forward value E and - through ff_backward walked as loss_and_grads walks it - every parameter gradient for a
random upstream dE; both sides are float64, the bar is 1e-12 of each tensor's largest element. CPU only."""
import numpy as np
import pytest

from oracle import ic_oracle as O

torch = pytest.importorskip('torch')

# (dim, input width) per observable
WIDTHS = {'w8_w3': ((32, 8), (32, 3)), 'w1_w1_w5': ((6, 1), (10, 1), (14, 5)), 'scalars': ((12, 1), (8, 1))}
BAR = 1e-12


def _params(emb, rng):
    P = {}

    def lin(prefix, l, out, inp):
        P['%s._layers.%d.weight' % (prefix, l)] = rng.standard_normal((out, inp)) / np.sqrt(inp)
        P['%s._layers.%d.bias' % (prefix, l)] = 0.3 * rng.standard_normal(out)
    for j, (d, w) in enumerate(emb):
        hid = (w + d) // 2
        lin('_layers_observe_embedding.obs%d' % j, 0, hid, w)
        lin('_layers_observe_embedding.obs%d' % j, 1, d, hid)
    e = sum(d for d, _ in emb)
    lin('_layers_observe_embedding_final', 0, e, e)
    lin('_layers_observe_embedding_final', 1, e, e)
    return P


def _oracle(net, obs, dE):
    """E and the embedding's parameter gradients, the backward as in O.loss_and_grads (final layers, then each observable on
    its columns of d cat)."""
    E, (caches, acts_final) = O.embed_observe(net, obs)
    grads = {}
    Ws, _ = net.ff('_layers_observe_embedding_final')
    dcat, dWs, dbs = O.ff_backward(dE, acts_final, Ws, True)
    for i in range(len(Ws)):
        grads['_layers_observe_embedding_final._layers.%d.weight' % i] = dWs[i]
        grads['_layers_observe_embedding_final._layers.%d.bias' % i] = dbs[i]
    c = 0
    for j, name in enumerate(net.obs_names):
        Ws, _ = net.ff('_layers_observe_embedding.' + name)
        w = Ws[-1].shape[0]
        _, dWs, dbs = O.ff_backward(dcat[:, c:c + w], caches[j], Ws, True)
        c += w
        for i in range(len(Ws)):
            grads['_layers_observe_embedding.%s._layers.%d.weight' % (name, i)] = dWs[i]
            grads['_layers_observe_embedding.%s._layers.%d.bias' % (name, i)] = dbs[i]
    return E, grads


def _autograd(P, emb, obs, dE):
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P.items()}
    x = torch.tensor(obs, dtype=torch.float64)

    def ff(prefix, h):
        for l in range(2):
            h = torch.relu(torch.nn.functional.linear(h, T['%s._layers.%d.weight' % (prefix, l)], T['%s._layers.%d.bias' % (prefix, l)]))
        return h
    parts = []
    for j, cols in enumerate(torch.split(x, [w for _, w in emb], dim=1)):
        parts.append(ff('_layers_observe_embedding.obs%d' % j, cols))
    E = ff('_layers_observe_embedding_final', torch.cat(parts, dim=1))
    E.backward(torch.tensor(dE, dtype=torch.float64))
    return E.detach().numpy(), {k: v.grad.numpy() for k, v in T.items()}


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('name', list(WIDTHS))
def test_embed_observe_and_its_backward_match_autograd(name):
    emb = WIDTHS[name]
    rng = np.random.default_rng(5 + len(emb))
    P = _params(emb, rng)
    B, width, e = 9, sum(w for _, w in emb), sum(d for d, _ in emb)
    obs = 3.0 + 2.0 * rng.standard_normal((B, width))
    dE = rng.standard_normal((B, e))
    net = O.Net(P, ['obs%d' % j for j in range(len(emb))])
    E, grads = _oracle(net, obs, dE)
    E_ref, grads_ref = _autograd(P, emb, obs, dE)
    assert E.shape == (B, e) and np.count_nonzero(E_ref) > E_ref.size // 8      # not a dead network
    assert _rel(E, E_ref) < BAR
    assert set(grads) == set(grads_ref) == set(P)
    for k in P:
        assert grads[k].shape == P[k].shape and np.any(grads_ref[k]), k
        assert _rel(grads[k], grads_ref[k]) < BAR, (k, _rel(grads[k], grads_ref[k]))


def test_a_column_of_a_vector_observable_reaches_only_its_own_layers():
    """Moving one input column moves the first layer of its own observable's block of `cat` and nothing of the others'."""
    emb = WIDTHS['w1_w1_w5']
    rng = np.random.default_rng(1)
    net = O.Net(_params(emb, rng), ['obs0', 'obs1', 'obs2'])
    obs = 3.0 + 2.0 * rng.standard_normal((4, 7))
    base = O.embed_observe(net, obs)[1][1][0]          # cat: the input of the final layers
    for col, block in ((0, slice(0, 6)), (1, slice(6, 16)), (2, slice(16, 30)), (6, slice(16, 30))):
        moved = obs.copy()
        moved[:, col] += 1.0
        cat = O.embed_observe(net, moved)[1][1][0]
        changed = np.zeros(30, bool)
        changed[block] = True
        assert np.array_equal(cat[:, ~changed], base[:, ~changed]), col
        assert not np.array_equal(cat[:, changed], base[:, changed]), col
