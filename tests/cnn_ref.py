"""Float64 comparator of the CNN2D5C observe embedding: a restatement of the standard architecture
(conv1 C->64, conv2 64->64, max-pool 2, conv3 64->128, conv4 128->128, conv5 128->128, max-pool 2, flatten (c, y, x),
lin1 F->dim, lin2 dim->dim; 3x3 valid convolutions, ReLU after every convolution and linear) on torch.nn.functional, with
autograd for the backward, a seeded weight generator and the kink margin that selects test images.

Why a margin: the stack has ~1e5 ReLU units and ~1e4 pool windows per image. Where a pre-activation is within float32
summation error of zero, or a pool window's two largest values are that close, the order of a float32 sum decides the
mask, and one flipped unit moves every gradient below it by its whole contribution. That is a property of the input, not
of an implementation, so gradient comparisons use images whose margin is above CNN_KINK_MARGIN (it may be raised, never
lowered). Forward values are continuous in the inputs and need no selection."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

CNN_KINK_MARGIN = 1e-5
MAX_CANDIDATES = 4096
CHANNELS = (64, 64, 128, 128, 128)
NAMES = tuple('_conv%d.%s' % (l, s) for l in range(1, 6) for s in ('weight', 'bias')) + \
    ('_lin1.weight', '_lin1.bias', '_lin2.weight', '_lin2.bias')


def feature_shape(shape):
    return tuple(((int(s) - 4) // 2 - 6) // 2 for s in shape[1:])


def tensor_shapes(shape, dim):
    """State-dict order: name -> shape."""
    h5, w5 = feature_shape(shape)
    out = OrderedDict()
    cin = int(shape[0])
    for l, cout in enumerate(CHANNELS):
        out['_conv%d.weight' % (l + 1)] = (cout, cin, 3, 3)
        out['_conv%d.bias' % (l + 1)] = (cout,)
        cin = cout
    out['_lin1.weight'] = (dim, 128 * h5 * w5)
    out['_lin1.bias'] = (dim,)
    out['_lin2.weight'] = (dim, dim)
    out['_lin2.bias'] = (dim,)
    return out


def seeded_cnn_params(shape, dim, seed):
    """Every tensor from numpy.random.default_rng(seed) in state-dict order, U(+-1/sqrt(fan_in)) for weight and bias
    (fan_in = Cin * 9 for a convolution, the input width for a linear layer). float32 arrays."""
    rng = np.random.default_rng(seed)
    shapes = tensor_shapes(shape, dim)
    out = OrderedDict()
    for name, s in shapes.items():
        ws = shapes[name[:-len('bias')] + 'weight'] if name.endswith('bias') else s
        k = 1.0 / np.sqrt(float(np.prod(ws[1:])))
        out[name] = rng.uniform(-k, k, s).astype(np.float32)
    return out


def param_checksums(params):
    """name -> [float64 sum, float64 sum of squares]: what the goldens store instead of the weights."""
    return {n: [float(np.asarray(v, np.float64).sum()), float((np.asarray(v, np.float64) ** 2).sum())] for n, v in params.items()}


def _t(params, dtype, requires_grad=False):
    return OrderedDict((n, torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad)) for n, v in params.items())


def _stack(p, x, keep=None):
    """x [B, C, H, W] -> (features [B, F], embedding [B, dim]). keep: list that receives (kind, input, pre-activation or
    pool input, weight, bias) per stage for kink_margin."""
    def conv(x, l):
        z = F.conv2d(x, p['_conv%d.weight' % l], p['_conv%d.bias' % l])
        if keep is not None:
            keep.append(('conv', x, z, p['_conv%d.weight' % l], p['_conv%d.bias' % l]))
        return torch.relu(z)

    def pool(x):
        if keep is not None:
            keep.append(('pool', x, None, None, None))
        return F.max_pool2d(x, 2)

    def lin(x, l):
        z = F.linear(x, p['_lin%d.weight' % l], p['_lin%d.bias' % l])
        if keep is not None:
            keep.append(('lin', x, z, p['_lin%d.weight' % l], p['_lin%d.bias' % l]))
        return torch.relu(z)

    x = conv(conv(x, 1), 2)
    x = pool(x)
    x = conv(conv(conv(x, 3), 4), 5)
    x = pool(x)
    feat = x.reshape(x.shape[0], -1)
    return feat, lin(lin(feat, 1), 2)


def forward(params, images, shape, dtype=torch.float64):
    """images [B, C*H*W] -> dict(features [B, F], embedding [B, dim]) as numpy arrays of `dtype`."""
    p = _t(params, dtype)
    x = torch.as_tensor(np.asarray(images), dtype=dtype).reshape(-1, *shape)
    with torch.no_grad():
        feat, emb = _stack(p, x)
    return {'features': feat.numpy(), 'embedding': emb.numpy()}


def forward_backward(params, images, shape, d_embedding=None, d_features=None, dtype=torch.float64):
    """Backward of sum(embedding * d_embedding) (or of sum(features * d_features): then the linear layers take no part).
    Returns dict(features, embedding, d_features, grads {name: array})."""
    p = _t(params, dtype, requires_grad=True)
    x = torch.as_tensor(np.asarray(images), dtype=dtype).reshape(-1, *shape)
    feat, emb = _stack(p, x)
    feat.retain_grad()
    if d_features is not None:
        (feat * torch.as_tensor(np.asarray(d_features), dtype=dtype)).sum().backward()
    else:
        (emb * torch.as_tensor(np.asarray(d_embedding), dtype=dtype)).sum().backward()
    grads = OrderedDict((n, t.grad.numpy() if t.grad is not None else None) for n, t in p.items())
    return {'features': feat.detach().numpy(), 'embedding': emb.detach().numpy(), 'd_features': feat.grad.numpy(), 'grads': grads}


def kink_margin(params, images, shape):
    """Per image, in float64: the minimum over all seven layers of |z| / sum |terms| (z = pre-activation, terms = the
    products and the bias that make it) and over all pool windows whose maximum is positive of
    (largest - second largest) / sum |terms| of the largest. float64 array [B]."""
    p = _t(params, torch.float64)
    x = torch.as_tensor(np.asarray(images), dtype=torch.float64).reshape(-1, *shape)
    keep = []
    with torch.no_grad():
        _stack(p, x, keep)
        B = x.shape[0]
        margin = torch.full((B,), float('inf'), dtype=torch.float64)
        last_sumabs = None
        for kind, inp, z, w, b in keep:
            if kind == 'conv':
                sumabs = F.conv2d(inp.abs(), w.abs(), b.abs())
            elif kind == 'lin':
                sumabs = F.linear(inp.abs(), w.abs(), b.abs())
            else:
                # pool over the ReLU outputs `inp` of the convolution before it (whose sum |terms| is last_sumabs)
                Hp, Wp = inp.shape[2] // 2, inp.shape[3] // 2
                win = inp[:, :, :2 * Hp, :2 * Wp].reshape(B, inp.shape[1], Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, inp.shape[1], Hp, Wp, 4)
                sab = last_sumabs[:, :, :2 * Hp, :2 * Wp].reshape(B, inp.shape[1], Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, inp.shape[1], Hp, Wp, 4)
                top, idx = win.sort(dim=-1, descending=True)
                gap = (top[..., 0] - top[..., 1]) / sab.gather(-1, idx[..., :1])[..., 0]
                gap = torch.where(top[..., 0] > 0, gap, torch.full_like(gap, float('inf')))
                margin = torch.minimum(margin, gap.reshape(B, -1).min(dim=1).values)
                continue
            margin = torch.minimum(margin, (z.abs() / sumabs).reshape(B, -1).min(dim=1).values)
            last_sumabs = sumabs
    return margin.numpy()


def select_images(params, shape, count, seed, margin=None):
    """The first `count` images with a kink margin above `margin` from a seeded stream of at most MAX_CANDIDATES
    U[0, 1) candidates. float32 [count, C*H*W]; asserts that `count` were found."""
    margin = CNN_KINK_MARGIN if margin is None else margin
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    found = []
    for _ in range(MAX_CANDIDATES // 256):
        cand = rng.random((256, n), dtype=np.float32)
        m = kink_margin(params, cand, shape)
        found.extend(cand[i] for i in np.nonzero(m > margin)[0])
        if len(found) >= count:
            break
    assert len(found) >= count, 'only %d of %d images with margin > %g among %d candidates' % (len(found), count, margin, MAX_CANDIDATES)
    return np.stack(found[:count]).astype(np.float32)
