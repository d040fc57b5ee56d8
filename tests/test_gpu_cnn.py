"""GPU tests of the CNN2D5C observe embedding (csrc/cnn2d.hip): the convolution stack at the C ABI against the float64
comparator tests/cnn_ref.py and the vectors recorded from the reference (tests/golden/make_cnn_golden.py).

Gradient accuracy is tested on small images selected by their kink margin (cnn_ref.py says why); at 28 x 28 and large
batches the tests are the ones a flipped ReLU or pool argmax cannot touch: the forward against float64, bit-equality of an
image's features whatever batch it sits in, additivity of the gradients over a split of the batch. Bars are the
project's own: gradients helpers.grad_check(label, got, ref, 1e-5, 5e-8); features 1e-5 of the largest feature."""
import json
import os

import numpy as np
import pytest

import cnn_ref
from conftest import GOLDEN
from helpers import grad_check

pytestmark = pytest.mark.gpu

GRAD_BAR, GRAD_FLOOR = 1e-5, 5e-8
CONV_NAMES = [n for n in cnn_ref.NAMES if n.startswith('_conv')]


def _unit_case(key):
    with open(os.path.join(GOLDEN, 'cnn_unit_meta.json')) as f:
        meta = json.load(f)[key]
    z = np.load(os.path.join(GOLDEN, 'cnn_unit.npz'))
    arrays = {k[len(key) + 1:]: z[k] for k in z.files if k.startswith(key + '.')}
    params = cnn_ref.seeded_cnn_params(meta['shape'], meta['dim'], meta['weight_seed'])
    for n, (s, q) in cnn_ref.param_checksums(params).items():      # a drifting generator is caught here
        assert abs(s - meta['checksums'][n][0]) <= 1e-9 * max(1.0, abs(s)) and abs(q - meta['checksums'][n][1]) <= 1e-9 * max(1.0, q), n
    return meta, arrays, params


def _stack(shape, dim, params):
    """(CNN2D5CStack, flat parameter buffer, zeroed gradient buffer) for one image observable with these weights."""
    import torch
    from pyprob_amd import ObserveEmbedding
    from pyprob_amd.cnn import CNN2D5CStack
    from pyprob_amd.spec import NetSpec
    spec = NetSpec({'img': {'dim': dim, 'reshape': list(shape), 'embedding': ObserveEmbedding.CNN2D5C}}, network='feedforward')
    flat = np.zeros(spec.n_params, np.float32)
    for n, v in params.items():
        off, s = spec.tensors['_layers_observe_embedding.img.' + n]
        assert tuple(s) == v.shape
        flat[off:off + v.size] = v.reshape(-1)
    st = CNN2D5CStack(spec, 'img')
    return st, torch.from_numpy(flat).to(st.device), torch.zeros(spec.n_params, dtype=torch.float32, device=st.device)


def _grads(st, gbuf):
    g = gbuf.cpu().numpy()
    out = {}
    for n in CONV_NAMES:
        off, s = st.spec.tensors['_layers_observe_embedding.img.' + n]
        out[n] = g[off:off + int(np.prod(s))].reshape(s).copy()
    return out


@pytest.mark.parametrize('key', ['s20', 'c3'])
def test_cnn_unit_forward_backward_against_float64_and_reference(key):
    import torch
    meta, a, params = _unit_case(key)
    shape = meta['shape']
    ref = cnn_ref.forward_backward(params, a['images'], shape, d_embedding=a['d_embedding'])
    st, P, G = _stack(shape, meta['dim'], params)
    feat = st.forward(P, torch.from_numpy(a['images']))
    st.backward(P, torch.from_numpy(ref['d_features'].astype(np.float32)), G)
    torch.cuda.synchronize()
    feat = feat.cpu().numpy()
    grad_check('cnn_unit %s features vs float64' % key, feat, ref['features'], GRAD_BAR, GRAD_FLOOR)
    grad_check('cnn_unit %s features vs reference' % key, feat, a['features'], GRAD_BAR, GRAD_FLOOR)
    g = _grads(st, G)
    for n in CONV_NAMES:
        r = ref['grads'][n]
        grad_check('cnn_unit %s %s vs float64' % (key, n), g[n], r, GRAD_BAR, GRAD_FLOOR)
        # the reference's own float32 gradients (bias: whole; weight: sums over the output-channel axis and over all other
        # axes - device and reference are each within the element bar of float64, so a sum of N elements differs by at most
        # 2 N element bars)
        elem = GRAD_BAR * np.abs(r).max() + GRAD_FLOOR
        if 'g.' + n in a:
            assert np.abs(g[n] - a['g.' + n]).max() < 2 * elem, n
        else:
            s0, sr = g[n].astype(np.float64).sum(axis=0), g[n].astype(np.float64).reshape(g[n].shape[0], -1).sum(axis=1)
            assert np.abs(s0 - a['gsum0.' + n]).max() < 2 * elem * g[n].shape[0], n
            assert np.abs(sr - a['gsumr.' + n]).max() < 2 * elem * (g[n].size // g[n].shape[0]), n
    # gradients are ADDED: a second backward doubles them exactly
    st.backward(P, torch.from_numpy(ref['d_features'].astype(np.float32)), G)
    g2 = _grads(st, G)
    for n in CONV_NAMES:
        assert np.array_equal(g2[n], 2 * g[n]), n


@pytest.mark.parametrize('key', ['s20', 'c3'])
def test_cnn_unit_two_runs_are_bit_equal(key):
    """The split-K partial weight gradients are stored and added in a fixed order: two runs give the same bits. Runs in the
    default mode here and with PP_DETERMINISTIC=1 in the child process of test_cnn_deterministic_mode_in_a_child_process."""
    import torch
    meta, a, params = _unit_case(key)
    d = torch.from_numpy(np.random.default_rng(5).standard_normal((meta['B'], a['features'].shape[1])).astype(np.float32))
    runs = []
    for _ in range(2):
        st, P, G = _stack(meta['shape'], meta['dim'], params)
        feat = st.forward(P, torch.from_numpy(a['images']))
        st.backward(P, d, G)
        runs.append((feat.cpu().numpy(), _grads(st, G)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for n in CONV_NAMES:
        assert np.array_equal(runs[0][1][n], runs[1][1][n]), n


def test_cnn_28x28_features_batch_independence_and_gradient_additivity():
    """[1, 28, 28], B = 1, 64 and 259 on unfiltered U[0, 1) images: features against float64; every image's features
    bit-equal whether it is computed in the batch of 259, in a part (64 + 64 + 64 + 67) or alone; the gradients of the
    batch equal the sum over the parts (equal masks by the previous property, so only the summation order differs)."""
    import torch
    shape, dim, B = [1, 28, 28], 32, 259
    params = cnn_ref.seeded_cnn_params(shape, dim, 31)
    rng = np.random.default_rng(32)
    images = rng.random((B, 28 * 28), dtype=np.float32)
    d = (rng.standard_normal((B, 1152)) / B).astype(np.float32)
    ref = cnn_ref.forward(params, images, shape)['features']
    st, P, G = _stack(shape, dim, params)
    feat = st.forward(P, torch.from_numpy(images))
    st.backward(P, torch.from_numpy(d), G)
    full, gfull = feat.cpu().numpy(), _grads(st, G)
    assert full.shape == (B, 1152)
    bar = 1e-5 * np.abs(ref).max()
    assert np.abs(full - ref).max() < bar, (np.abs(full - ref).max(), bar)
    gsum = {n: np.zeros_like(v, dtype=np.float64) for n, v in gfull.items()}
    b0 = 0
    for nb in (64, 64, 64, 67):
        sl = slice(b0, b0 + nb)
        Gp = torch.zeros_like(G)
        fp = st.forward(P, torch.from_numpy(images[sl]))
        st.backward(P, torch.from_numpy(d[sl]), Gp)
        fp = fp.cpu().numpy()
        assert np.array_equal(fp, full[sl]), 'features of images %d..%d depend on the batch' % (b0, b0 + nb)
        if nb == 64 and b0 == 0:
            assert np.abs(fp - ref[sl]).max() < bar
        for n, v in _grads(st, Gp).items():
            gsum[n] += v
        b0 += nb
    for i in range(B):
        f1 = st.forward(P, torch.from_numpy(images[i:i + 1])).cpu().numpy()
        assert np.array_equal(f1[0], full[i]), 'features of image %d alone differ from the batch' % i
        if i == 0:
            assert np.abs(f1[0] - ref[0]).max() < bar
    for n in CONV_NAMES:
        grad_check('cnn 28x28 B=259 %s vs sum of parts' % n, gfull[n], gsum[n], GRAD_BAR, GRAD_FLOOR)


# ---- whole networks: the convolution stack inside pp_ic_loss / pp_is_init ----------------------------------------------
def _engine(case):
    from cnn_golden import load_cnn_golden, spec_from_cnn_golden
    from pyprob_amd.engine import ICEngine
    meta, params, batch, loss, isr = load_cnn_golden(case)
    spec = spec_from_cnn_golden(meta)
    eng = ICEngine(spec, seed=0)
    assert set(spec.tensors.keys()) == set(params.keys())
    eng.load_state_dict(params)
    return eng, meta, params, batch, loss, isr


def _unpack_lp(pb, lp_rows):
    out = np.empty(pb.n_rows, np.float64)
    out[pb.src_row] = lp_rows
    return out


@pytest.mark.parametrize('case', ['cnnl', 'cnnf'])
def test_cnn_golden_loss_logprob_gradients_and_presence(case):
    """As test_gpu_path.test_golden_loss_logprob_and_gradients: loss, per-row log_prob, every gradient and the presence map
    against the reference's records (cnnf: all gradients except the four large ones, which have no file)."""
    import torch
    from helpers import packed_from_golden
    eng, meta, params, batch, loss, isr = _engine(case)
    pb = packed_from_golden(meta, batch, eng.spec).to(eng.device)
    l, lp = eng.loss(pb, backward=True, keep_lp=True)
    torch.cuda.synchronize()
    assert int(eng.status_buf[0].item()) == 0
    ref_loss = float(loss['loss'])
    assert abs(float(l.item()) - ref_loss) <= 1e-5 * abs(ref_loss), (float(l.item()), ref_loss)
    lp_tm = _unpack_lp(pb, lp.cpu().numpy())
    off = np.concatenate([[0], np.cumsum(batch['trace_len'])])
    for si, t in meta['lp_index']:
        rows = off[np.array(meta['sub_batches'][si])] + t
        ref = loss['lp_%d_%d' % (si, t)]
        np.testing.assert_allclose(lp_tm[rows], ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref).max()))
    g = eng.grad_dict()
    checked = 0
    for i, n in enumerate(meta['param_names']):
        if 'g%d' % i not in loss:
            assert case == 'cnnf' and n.endswith(('_conv2.weight', '_conv3.weight', '_conv4.weight', '_conv5.weight')), n
            continue
        if not meta['has_grad'][i]:
            assert np.all(g[n] == 0), n
            continue
        grad_check('golden_%s/%s' % (case, n), g[n], loss['g%d' % i], GRAD_BAR, GRAD_FLOOR)
        checked += 1
    assert checked == sum(meta['has_grad']) - (4 if case == 'cnnf' else 0)
    act = eng.presence().cpu().numpy()
    ref_has = dict(zip(meta['param_names'], meta['has_grad']))
    assert [bool(a) for a in act] == [bool(ref_has[n]) for n in eng.spec.tensors]
    # the single-statement traces alone (a batch that the row-panel kernels would take from a FEEDFORWARD network steps aside
    # to the tile path): the loss is minus the mean of the same rows' log_prob
    one = np.nonzero(batch['trace_len'] == 1)[0]
    assert 0 < len(one) < len(batch['trace_len'])
    rows = off[one]
    sub = dict(trace_len=batch['trace_len'][one], addr_idx=batch['addr_idx'][rows], values=batch['values'][rows],
               prior=batch['prior'][rows], obs=batch['obs'][one])
    l1 = float(eng.loss(packed_from_golden(meta, sub, eng.spec).to(eng.device), backward=True).item())
    assert int(eng.status_buf[0].item()) == 0
    assert abs(l1 + lp_tm[rows].mean()) <= 1e-5 * abs(l1), (l1, -lp_tm[rows].mean())


@pytest.mark.parametrize('case', ['cnnl', 'cnnf'])
def test_cnn_is_rescoring_matches_reference_records(case):
    """The reference's particles re-scored (test_gpu_path.test_is_rescoring_matches_reference_records): pp_is_init embeds
    the image through the same stack (one image per posterior call); the one-launch first statement steps aside."""
    import ctypes as C
    import torch
    from pyprob_amd.is_engine import ISRunner
    eng, meta, params, batch, loss, isr = _engine(case)
    for a in range(len(eng.spec.addresses)):
        assert eng.lib.pp_is_first_statement_supported(C.byref(eng.net), a) == 0
    run = ISRunner(eng)
    run.init(isr['observe'])
    addresses = meta['is_addresses']
    off = np.concatenate([[0], np.cumsum(isr['trace_len'])])
    q_all = np.zeros(len(isr['value']))
    for b in range(len(isr['trace_len'])):
        run.begin(1)
        prev = None
        for t in range(int(isr['trace_len'][b])):
            r = off[b] + t
            a = eng.spec.address_id[addresses[isr['addr'][r]]]
            v = torch.tensor([isr['value'][r]], dtype=torch.float32, device=eng.device)
            pr = torch.tensor(isr['prior'][r, :2].reshape(1, 2), dtype=torch.float32, device=eng.device)
            _, logq = run.step(a, prev, pr, value_in=v)
            q_all[r] = float(logq.item())
            prev = a
    np.testing.assert_allclose(q_all, isr['prop_lp'], rtol=1e-4, atol=1e-4)
    lw = np.array([np.sum(isr['prior_lp'][off[b]:off[b + 1]] - q_all[off[b]:off[b + 1]]) for b in range(len(off) - 1)])
    np.testing.assert_allclose(lw + isr['obs_lw'], isr['lw'], rtol=1e-4, atol=1e-4)


def test_cnn_minibatch_of_64_equals_the_mean_of_four_parts():
    """64 traces (the golden batch twice, the second half with fresh unfiltered images): the loss equals the mean of the
    losses of its four quarters (forward only: continuous in the inputs, no selection needed)."""
    from helpers import packed_from_golden
    eng, meta, params, batch, loss, isr = _engine('cnnl')
    obs2 = batch['obs'].copy()
    obs2[:, :400] = np.random.default_rng(3).random((len(obs2), 400), dtype=np.float32)
    arrays = {k: np.concatenate([batch[k], batch[k]]) for k in ('trace_len', 'addr_idx', 'values', 'prior')}
    arrays['obs'] = np.concatenate([batch['obs'], obs2])
    off = np.concatenate([[0], np.cumsum(arrays['trace_len'])])

    def piece(b0, b1):
        r0, r1 = off[b0], off[b1]
        return dict(trace_len=arrays['trace_len'][b0:b1], addr_idx=arrays['addr_idx'][r0:r1], values=arrays['values'][r0:r1],
                    prior=arrays['prior'][r0:r1], obs=arrays['obs'][b0:b1])

    full = float(eng.loss(packed_from_golden(meta, arrays, eng.spec).to(eng.device)).item())
    parts = [float(eng.loss(packed_from_golden(meta, piece(16 * k, 16 * k + 16), eng.spec).to(eng.device)).item()) for k in range(4)]
    assert abs(full - np.mean(parts)) <= 1e-5 * abs(full), (full, parts)


def test_cnn_adam_tracks_the_oracle_and_state_dict_round_trip():
    """Adam over every tensor, the convolutions included, against the oracle's Adam fed with the same gradients
    (test_gpu_path.test_adam_matches_torch_semantics); a second engine loaded from the first one's state_dict gives the
    same loss bit for bit."""
    import torch
    from helpers import packed_from_golden, rel_err
    from oracle import ic_oracle as O
    from pyprob_amd.engine import ICEngine
    eng, meta, params, batch, loss, isr = _engine('cnnl')
    pb = packed_from_golden(meta, batch, eng.spec).to(eng.device)
    P = {k: v.astype(np.float64).copy() for k, v in params.items()}
    M = {k: np.zeros_like(v) for k, v in P.items()}
    V = {k: np.zeros_like(v) for k, v in P.items()}
    names = list(eng.spec.tensors.keys())
    act = eng.spec.active_mask(pb.cur_counts, pb.prev_counts)
    roles = eng.spec.tensor_roles()[2]
    for n in names:
        if '._conv' in n or '._lin' in n:
            assert act[names.index(n)] == 1 and roles[names.index(n)] == 4, n      # core tensors: always active
    for step in range(1, 4):
        eng.loss(pb, backward=True)
        g = eng.grad_dict()
        eng.adam_step(1e-3)
        torch.cuda.synchronize()
        for i, n in enumerate(names):
            if act[i]:
                O.adam_step(P[n], g[n].astype(np.float64), M[n], V[n], step, 1e-3)
        sd = eng.state_dict()
        worst = max(rel_err(sd[n].numpy(), P[n]) for n in names)
        assert worst < 2e-6, (step, worst)
    other = ICEngine(eng.spec, seed=9)
    other.load_state_dict(eng.state_dict())
    la = float(eng.loss(pb).item())
    lb = float(other.loss(packed_from_golden(meta, batch, other.spec).to(other.device)).item())
    assert la == lb


# ---- end to end through the host API --------------------------------------------------------------------------------
def _captcha_model():
    import torch
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Categorical, Normal

    class Captcha(Model):
        """d ~ Categorical(6); for odd d also a Normal brightness; a 28 x 28 image with a digit-dependent stripe pattern plus
        Normal pixel noise is observed."""

        def __init__(self):
            super().__init__('captcha-like')
            yy, xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing='ij')
            self.patterns = torch.stack([0.5 + 0.4 * torch.sin((yy * (1 + k % 3) + xx * (1 + k // 3)) * 0.35) for k in range(6)])

        def forward(self):
            d = int(pyprob.sample(Categorical([1 / 6.] * 6)))
            gain = pyprob.sample(Normal(1.0, 0.1)) if d % 2 else 1.0
            pyprob.observe(Normal(self.patterns[d] * gain, 0.1), name='img')
            return d

    return Captcha()


def test_cnn_end_to_end_training_inference_and_checkpoint(tmp_path):
    """Model.learn_inference_network with an image observable: the loss falls, posterior_results gives finite weights on
    both host paths that carry vector observations (particle coroutines and one particle per forward()), and a saved
    network reloads to the same loss bit for bit."""
    import torch
    from pyprob_amd import InferenceEngine, InferenceNetwork, ObserveEmbedding
    from pyprob_amd.nn import Batch, OnlineDataset
    IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
    model = _captcha_model()
    emb = {'img': {'dim': 32, 'reshape': [1, 28, 28], 'embedding': ObserveEmbedding.CNN2D5C}}
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=3200, observe_embeddings=emb, batch_size=64,
                                  lstm_dim=64, seed=1)
    net = model._inference_network
    assert net._engine.spec.obs_feat['img'] == 1152
    assert np.isfinite(net._loss_previous) and net._loss_previous < net._loss_init, (net._loss_init, net._loss_previous)
    observe = {'img': model.patterns[3] + 0.1 * torch.randn(28, 28, generator=torch.Generator().manual_seed(4))}
    co = model.posterior_results(64, IC, lock_step=False, observe=observe, seed=2)
    assert co.length == 64 and np.all(np.isfinite(co.log_weights))
    one = model.posterior_results(16, IC, lock_step='per_trace', observe=observe)
    assert np.all(np.isfinite(one.log_weights))
    auto = model.posterior_results(32, IC, observe=observe, seed=3)       # auto-detection settles on a path that can carry an image
    assert np.all(np.isfinite(auto.log_weights))
    # checkpoint round trip: the same minibatch gives the same loss, bit for bit
    ds = OnlineDataset(model=model)
    batch = Batch([ds[i] for i in range(16)])
    f = str(tmp_path / 'captcha.network')
    model.save_inference_network(f)
    other = _captcha_model()
    other.load_inference_network(f)
    ok1, l1 = net._loss(batch)
    ok2, l2 = other._inference_network._loss(batch)
    assert ok1 and ok2 and float(l1.item()) == float(l2.item())
    sd1, sd2 = net.state_dict(), other._inference_network.state_dict()
    assert list(sd1) == list(sd2) and all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert sd1['_layers_observe_embedding.img._conv4.weight'].shape == (128, 128, 3, 3)
    # offline: packed shards carry an image as C*H*W floats of the observation row
    d = str(tmp_path / 'shards')
    model.save_dataset(d, 256, 128)
    third = _captcha_model()
    third.learn_inference_network(inference_network=InferenceNetwork.FEEDFORWARD, num_traces=512, observe_embeddings=emb, batch_size=64,
                                  dataset_dir=d, seed=2)
    n3 = third._inference_network
    assert n3._engine.spec.obs == [('img', 784, 32, 32)] and np.isfinite(n3._loss_previous)


# ---- PP_DETERMINISTIC=1 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['cnnl', 'cnnf'])
def test_cnn_engine_two_runs(case):
    """Loss and gradients of two fresh engines on the golden batch: bit-equal with PP_DETERMINISTIC=1 (the child process of the
    test below); in the default mode the products around the stack add K splits with float atomics, so the runs agree
    within the gradient bar."""
    import torch
    from helpers import packed_from_golden
    det = os.environ.get('PP_DETERMINISTIC', '0') not in ('', '0')
    runs = []
    for _ in range(2):
        eng, meta, params, batch, loss, isr = _engine(case)
        l = eng.loss(packed_from_golden(meta, batch, eng.spec).to(eng.device), backward=True)
        torch.cuda.synchronize()
        runs.append((float(l.item()), eng.grad_dict()))
    if det:
        assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        if det:
            assert np.array_equal(runs[0][1][n], runs[1][1][n]), n
        elif np.any(runs[1][1][n]):
            grad_check('cnn two runs %s/%s' % (case, n), runs[0][1][n], runs[1][1][n], GRAD_BAR, GRAD_FLOOR)


def test_cnn_deterministic_mode_in_a_child_process():
    """The cnn_unit cases (accuracy and two bit-equal runs) and the cnnl / cnnf engine losses again with PP_DETERMINISTIC=1.
    The mode is read once per process, so the cases run in a fresh child process with the variable set."""
    import subprocess
    import sys
    env = dict(os.environ, PP_DETERMINISTIC='1')
    env.pop('PP_TEST_RECORD_ERRORS', None)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-q', '-p', 'no:cacheprovider',
                        '-k', 'cnn_unit or golden_loss or engine_two_runs'], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    tail = r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert '8 passed' in r.stdout and 'skipped' not in r.stdout and 'failed' not in r.stdout, tail


# ---- lock step -----------------------------------------------------------------------------------------------------------
def test_cnn_lockstep_posterior_equals_the_per_trace_path():
    """A lock-step posterior_results call with an image observation: every particle's log-weight equals what the per-trace
    path (batch-1 network calls on the same image embedding) gives for the same sampled values - log p - log q of both
    statements plus the image's summed log-likelihood (computed here in float64)."""
    import torch
    import pyprob_amd as pyprob
    from pyprob_amd import InferenceEngine, InferenceNetwork, Model, ObserveEmbedding
    from pyprob_amd.distributions import Categorical, Normal
    from pyprob_amd.is_engine import ISRunner

    yy, xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing='ij')
    patterns = torch.stack([0.5 + 0.4 * torch.sin((yy * (1 + k % 3) + xx * (1 + k // 3)) * 0.35) for k in range(6)])

    class Captcha(Model):
        """Lock-step safe: no sampled value becomes a Python scalar. d ~ Categorical(6), gain ~ Normal(1, 0.1), the image is
        the d-th pattern times the gain plus Normal pixel noise."""

        def forward(self):
            d = pyprob.sample(Categorical([1 / 6.] * 6))
            gain = pyprob.sample(Normal(1.0, 0.1))
            mean = patterns.to(d.device)[d.long()] * gain.reshape(-1, 1, 1)
            pyprob.observe(Normal(mean, 0.1), name='img')
            return d

    model = Captcha('captcha-like, lock step')
    emb = {'img': {'dim': 32, 'reshape': [1, 28, 28], 'embedding': ObserveEmbedding.CNN2D5C}}
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=1280, observe_embeddings=emb, batch_size=64,
                                  lstm_dim=64, seed=1)
    net = model._inference_network
    image = patterns[2] * 1.05 + 0.1 * torch.randn(28, 28, generator=torch.Generator().manual_seed(6))
    n = 512
    post = model.posterior_results(n, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, lock_step=True,
                                   observe={'img': image}, seed=5)
    lw = post._all_log_weights.cpu().numpy().astype(np.float64)
    assert lw.shape == (n,) and np.all(np.isfinite(lw))
    (a0, (v0, id0)), = post.statement_log[0].items()
    (a1, (v1, id1)), = post.statement_log[1].items()
    d, gain = v0.cpu().numpy().astype(np.float64), v1.cpu().numpy().astype(np.float64)
    assert set(np.unique(d)) <= set(range(6))
    # the per-trace path on the same values
    run = ISRunner(net._engine)
    run.init(image.reshape(-1).numpy())
    dev = net._engine.device
    pr0 = torch.tensor([[1 / 6., 1 / 6.]], dtype=torch.float32, device=dev)
    pr1 = torch.tensor([[1.0, 0.1]], dtype=torch.float32, device=dev)
    m = 64
    want = np.zeros(m)
    img64, pat64 = image.double().numpy(), patterns.double().numpy()
    for b in range(m):
        run.begin(1)
        _, q0 = run.step(int(id0), None, pr0, value_in=v0[b:b + 1].contiguous())
        _, q1 = run.step(int(id1), int(id0), pr1, value_in=v1[b:b + 1].contiguous())
        mean = pat64[int(d[b])] * gain[b]
        like = np.sum(-0.5 * ((img64 - mean) / 0.1) ** 2 - np.log(0.1) - 0.5 * np.log(2 * np.pi))
        prior = np.log(1 / 6.) + (-0.5 * ((gain[b] - 1.0) / 0.1) ** 2 - np.log(0.1) - 0.5 * np.log(2 * np.pi))
        want[b] = prior + like - float(q0.item()) - float(q1.item())
    np.testing.assert_allclose(lw[:m], want, rtol=1e-4, atol=1e-4)
    # and the reference's loop itself, one particle per forward(): finite weights from the same network
    one = model.posterior_results(16, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, lock_step='per_trace',
                                  observe={'img': image})
    assert np.all(np.isfinite(one.log_weights))
