"""pp_obs_draw (csrc/obs_draw.hip) on the device: bit-equality with pp_prior_draw at k = 1, the float64 restatement of the
counter scheme (tests/obs_draw_ref.py), independence of a row from how rows are split, bounds at odd k and unaligned outputs,
error returns, the distribution of the draws; then the lock-step generator and online training on an image observable."""
import ctypes as C
import math

import numpy as np
import pytest

from obs_draw_ref import obs_draw_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SEED, OFFSET, STREAM = 0x1234567890ABCDEF, (7 << 32) + 11, 0x4003


@pytest.fixture(scope='module')
def ops():
    from pyprob_amd.ops import ops
    return ops


def _params(kind, shape, gen):
    """(p0, p1) of one shape on the device: Normal(mean in [-2, 2], sigma in [0.5, 2]) | Uniform(a in [-2, 0], a + [0.5, 3])."""
    u, v = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    if kind == 0:
        return (4 * u - 2).cuda(), (0.5 + 1.5 * v).cuda()
    a = -2 * u
    return a.cuda(), (a + 0.5 + 2.5 * v).cuda()


def _shapes(n, k):
    return {'scalar': (), 'row': (1, k), 'per trace': (n, 1), 'block': (n, k)}


def test_k1_is_bit_identical_to_prior_draw(ops):
    n = 300
    gen = torch.Generator().manual_seed(1)
    for kind in (0, 1):
        for shape in ((1,), (n,)):
            p0, p1 = _params(kind, shape, gen)
            if kind == 1 and shape == (1,):
                p0, p1 = torch.tensor([-1.0]).cuda(), torch.tensor([3.0]).cuda()
            want = ops.prior_draw(kind, p0, p1, n, SEED, OFFSET, STREAM)
            got = ops.obs_draw(kind, p0, p1, n, 1, SEED, OFFSET, STREAM)
            assert got.shape == (n, 1) and torch.equal(got.reshape(-1), want), (kind, shape)
            # element 0 of a wider row is the same value again
            p0k = p0 if p0.numel() == 1 else p0.reshape(n, 1)
            p1k = p1 if p1.numel() == 1 else p1.reshape(n, 1)
            assert torch.equal(ops.obs_draw(kind, p0k, p1k, n, 7, SEED, OFFSET, STREAM)[:, 0], want), (kind, shape)


@pytest.mark.parametrize('n', [1, 3, 257])
@pytest.mark.parametrize('k', [1, 3, 4, 5, 400])
def test_against_the_float64_restatement(ops, n, k):
    """Uniform: one rounding of the product and one of the sum, fused or not: <= 2 * 2^-23 * max(|a|, |b|). Normal: the radius
    sqrt(-2 ln u) is <= 5.8 for a 24-bit u, the fp32 rounding of 2 pi u moves the cosine by <= 5e-7, logf / cosf / sinf are good to
    a few ulp: together < 4e-6 |b|; the bar is 1e-5 |b| + 2^-22 |a|. A sine and a cosine branch swapped would miss it by ~|b|."""
    gen = torch.Generator().manual_seed(100 * n + k)
    shapes = _shapes(n, k)
    for kind in (0, 1):
        for n0, s0 in shapes.items():
            for n1, s1 in shapes.items():
                p0, _ = _params(kind, s0, gen)
                _, p1 = _params(kind, s1, gen)
                if kind == 1:
                    p1 = p1 + 2.0      # (the two shapes were drawn independently: keep high above low)
                got = ops.obs_draw(kind, p0, p1, n, k, SEED, OFFSET, STREAM).cpu().numpy().astype(np.float64)
                ref = obs_draw_ref(kind, p0, p1, n, k, SEED, OFFSET, STREAM)
                a = np.broadcast_to(p0.cpu().numpy().astype(np.float64).reshape(s0 if s0 else (1, 1)), (n, k))
                b = np.broadcast_to(p1.cpu().numpy().astype(np.float64).reshape(s1 if s1 else (1, 1)), (n, k))
                bar = 2 * 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) if kind == 1 else 1e-5 * np.abs(b) + 2.0 ** -22 * np.abs(a)
                err = np.abs(got - ref)
                assert got.shape == (n, k) and np.all(err <= bar), (kind, n0, n1, float((err / bar).max()))


def test_rows_do_not_depend_on_the_split(ops):
    gen = torch.Generator().manual_seed(2)
    for kind in (0, 1):
        k = 12
        p0, p1 = _params(kind, (300, k), gen)
        whole = ops.obs_draw(kind, p0, p1, 300, k, SEED, OFFSET, STREAM)
        part = ops.obs_draw(kind, p0[100:200].contiguous(), p1[100:200].contiguous(), 100, k, SEED, OFFSET + 100, STREAM)
        assert torch.equal(whole[100:200], part)
        q0, q1 = _params(kind, (), gen)
        five, eight = (ops.obs_draw(kind, q0, q1, 300, kk, SEED, OFFSET, STREAM) for kk in (5, 8))
        assert torch.equal(five[:, :4], eight[:, :4])


def _c_call(kind, p0, p1, n, k, out_ptr, r=(0, 0, 0, 0)):
    from pyprob_amd import lib as L
    lib = L.load()
    rc = lib.pp_obs_draw(kind, p0, r[0], r[1], p1, r[2], r[3], n, k, SEED, OFFSET, STREAM, out_ptr, None)
    torch.cuda.synchronize()
    return rc, lib


@pytest.mark.parametrize('k', [4, 7])
def test_unaligned_output_stays_in_bounds(ops, k):
    n = 5
    p0, p1 = torch.tensor([0.5]).cuda(), torch.tensor([2.0]).cuda()
    buf = torch.full((1 + n * k + 8,), float('nan'), device='cuda')
    assert buf.data_ptr() % 16 == 0
    rc, _ = _c_call(0, p0.data_ptr(), p1.data_ptr(), n, k, buf.data_ptr() + 4)
    assert rc == 0
    aligned = ops.obs_draw(0, p0, p1, n, k, SEED, OFFSET, STREAM)
    body = buf[1:1 + n * k]
    assert bool(torch.isfinite(body).all()) and torch.equal(body.reshape(n, k), aligned)
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + n * k:]).all())


def test_error_returns_launch_nothing(ops):
    p0, p1 = torch.tensor([0.5]).cuda(), torch.tensor([2.0]).cuda()
    out = torch.full((64,), float('nan'), device='cuda')
    for kind, k, n, o in ((2, 4, 4, out.data_ptr()), (0, 0, 4, out.data_ptr()), (0, 4, -1, out.data_ptr()), (0, 4, 4, None)):
        rc, lib = _c_call(kind, p0.data_ptr(), p1.data_ptr(), n, k, o)
        assert rc != 0 and b'pp_obs_draw' in lib.pp_last_error(), (kind, k, n, o)
    rc, lib = _c_call(0, None, p1.data_ptr(), 4, 4, out.data_ptr())
    assert rc != 0 and b'pp_obs_draw' in lib.pp_last_error()
    rc, _ = _c_call(0, p0.data_ptr(), p1.data_ptr(), 0, 4, out.data_ptr())
    assert rc == 0
    rc, _ = _c_call(0, None, None, 0, 4, None)
    assert rc == 0
    assert bool(torch.isnan(out).all())
    with pytest.raises(RuntimeError, match='obs_draw'):
        ops.obs_draw(0, torch.zeros(3, 5).cuda(), p1, 4, 5, 1, 0, 0)


def _ks(x, cdf):
    x = np.sort(np.asarray(x, np.float64))
    f, i = cdf(x), np.arange(1, x.size + 1, dtype=np.float64)
    return max(float((i / x.size - f).max()), float((f - (i - 1) / x.size).max()))


def test_distribution_of_the_draws(ops):
    n, k = 64, 784
    N = n * k
    dkw = math.sqrt(math.log(2 / 1e-9) / (2 * N))          # Dvoretzky-Kiefer-Wolfowitz at alpha = 1e-9: 0.0146
    assert abs(dkw - 0.0146) < 1e-4
    mean, sigma = torch.full((1, k), 0.3).cuda(), torch.tensor([2.0]).cuda()
    x = ops.obs_draw(0, mean, sigma, n, k, 99, 0, 0x4000).cpu().numpy().astype(np.float64)
    z = (x - 0.3) / 2
    d_normal = _ks(z.reshape(-1), lambda t: torch.special.ndtr(torch.from_numpy(t)).numpy())
    g = z.reshape(n, k // 4, 4)
    c01 = abs(np.corrcoef(g[..., 0].reshape(-1), g[..., 1].reshape(-1))[0, 1])
    c02 = abs(np.corrcoef(g[..., 0].reshape(-1), g[..., 2].reshape(-1))[0, 1])
    lo, hi = torch.tensor([-1.0]).cuda(), torch.tensor([3.0]).cuda()
    u = ops.obs_draw(1, lo, hi, n, k, 99, 0, 0x4001).cpu().numpy()
    d_uniform = _ks(u.reshape(-1), lambda t: (t + 1) / 4)
    print('KS normal %.5f uniform %.5f (bar %.5f); |corr| cos/sin %.5f pair/pair %.5f (bar %.5f)'
          % (d_normal, d_uniform, dkw, c01, c02, 6 / math.sqrt(N / 4)))
    assert d_normal <= dkw and d_uniform <= dkw
    assert c01 <= 6 / math.sqrt(N / 4) and c02 <= 6 / math.sqrt(N / 4)
    assert u.min() >= -1.0 and not np.any(u == np.float32(3.0))


def test_generator_on_the_device():
    from test_prior_vector_obs import N, TwoPath, check_two_path
    model = TwoPath('two paths, device')
    chunks = []
    for seed in (0, 0, None):
        if seed is not None:
            torch.manual_seed(seed)
        cols = model.prior_traces_packed(N, ['img', 'y'], device='cuda:0')
        check_two_path(cols, model._last_prior_obs_widths)
        chunks.append(cols)
    for a, b in zip(chunks[0], chunks[1]):
        if isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a, b)
    assert not np.array_equal(chunks[1][5], chunks[2][5])


def _captcha():
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Categorical, Normal
    yy, xx = torch.meshgrid(torch.arange(20.), torch.arange(20.), indexing='ij')
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

    return Captcha('captcha-like, lock step'), patterns


def _learn(model, monkeypatch, **kw):
    from pyprob_amd import InferenceNetwork, ObserveEmbedding
    from pyprob_amd import dataset as D
    made = []
    init = D.VectorisedOnlineDataset.__init__

    def recording_init(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(D.VectorisedOnlineDataset, '__init__', recording_init)
    emb = {'img': {'dim': 32, 'reshape': [1, 20, 20], 'embedding': ObserveEmbedding.CNN2D5C}}
    model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=1280, observe_embeddings=emb, batch_size=64,
                                  lstm_dim=64, seed=1, **kw)
    return made


def test_online_training_on_an_image_observable(monkeypatch):
    from pyprob_amd import InferenceEngine
    from pyprob_amd.dataset import VectorisedOnlineDataset
    torch.manual_seed(3)
    model, patterns = _captcha()
    made = _learn(model, monkeypatch, vectorised_prior=True)
    assert len(made) == 1 and isinstance(made[0], VectorisedOnlineDataset) and made[0].obs_widths == [400]
    net = model._inference_network
    print('loss %.4f -> %.4f' % (net._loss_init, net._loss_previous))
    assert math.isfinite(net._loss_previous) and net._loss_previous < net._loss_init
    image = patterns[2] * 1.05 + 0.1 * torch.randn(20, 20, generator=torch.Generator().manual_seed(6))
    post = model.posterior_results(256, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK, lock_step=True,
                                   observe={'img': image}, seed=5)
    lw = post._all_log_weights.cpu().numpy()
    assert lw.shape == (256,) and np.all(np.isfinite(lw))


def test_the_default_route_no_longer_falls_back_per_trace(monkeypatch, capsys):
    torch.manual_seed(4)
    model, _ = _captcha()
    made = _learn(model, monkeypatch)
    assert 'one forward() at a time' not in capsys.readouterr().out
    assert len(made) == 1 and made[0].obs_widths == [400]
