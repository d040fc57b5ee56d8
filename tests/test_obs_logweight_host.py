"""pp_obs_logweight without a device: the ABI additions, the float64 restatement against the reference's recorded values, the
stride classification, and the host route of a vector-valued observe in lock step (PP_VEC_LIKELIHOOD) on a CPU double of the
operator."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

import obs_logweight_ref as OR
import pyprob_amd
from pyprob_amd import distributions as D
from pyprob_amd.model import Model

HAVE_REFERENCE = os.path.isdir('/root/reference/pyprob')


def bar(ref):
    """The project's log-weight bar (tests/test_gpu_cnn.py): rtol 1e-4, atol 1e-4 * max(1, |ref|max)."""
    return dict(rtol=1e-4, atol=1e-4 * max(1.0, float(np.max(np.abs(ref)))))


@pytest.fixture(scope='module')
def lib():
    from pyprob_amd import build as B
    B.build()
    from pyprob_amd import lib as L
    return L.load()


@pytest.fixture()
def cpu_doubles():
    import oracle_ops
    from test_dist_families import _register_dist_cpu_doubles
    oracle_ops.register()
    _register_dist_cpu_doubles()
    OR.register_cpu_double()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_symbol_prototype_and_header(lib):
    from pyprob_amd import build as B, lib as L
    assert lib.pp_abi_version() == 15 == L.PP_ABI_VERSION
    assert hasattr(lib, 'pp_obs_logweight') and 'pp_obs_logweight' in L.PROTOTYPES and 'obs_logweight.hip' in B.SOURCES
    res, args = L.PROTOTYPES['pp_obs_logweight']
    assert res is C.c_int and len(args) == 11 and args[2] is L.pp_obs_operand and args[1] is C.POINTER(L.pp_obs_operand)
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    assert re.search(r'#define PP_ABI_VERSION 15\b', hdr)
    assert re.search(r'int pp_obs_logweight\(int32_t kind, const pp_obs_operand params\[4\], pp_obs_operand x, int32_t k, float scale,', hdr)
    assert 'typedef struct pp_obs_operand { const float* p; int64_t row_stride; int32_t elem_stride; int32_t _pad; } pp_obs_operand;' in hdr
    for words in ('FIXED SUMMATION ORDER', 'e & 255', 'ONE FORMULA', 'ADDRESSING', 'bit-identical to pp_dist_logweight'):
        assert words in hdr, words
    import pyprob_amd.ops  # noqa: F401
    assert hasattr(torch.ops.pyprob_hip, 'obs_logweight')


def test_operand_struct_layout():
    from pyprob_amd import lib as L
    o = L.pp_obs_operand
    assert C.sizeof(o) == 24
    assert (o.p.offset, o.row_stride.offset, o.elem_stride.offset, o._pad.offset) == (0, 8, 16, 20)
    assert (o.p.size, o.row_stride.size, o.elem_stride.size) == (8, 8, 4)


def test_refusals_come_before_any_launch(lib):
    """Every refused call has host pointers and returns before a launch; so do the accepted ones (m = 0)."""
    from pyprob_amd import lib as L
    buf = np.ones(64, np.float32)
    rows = np.zeros(4, np.int64)
    ptr = buf.ctypes.data

    def call(kind=0, k=4, lw=ptr, lp=None, rows_=None, m=0, n=0, drop=None, x=True, neg=None):
        arr = (L.pp_obs_operand * 4)()
        for q in range(OR.N_PARAMS.get(kind, 2)):
            if q != drop:
                arr[q].p, arr[q].row_stride, arr[q].elem_stride = ptr, 0, (-1 if neg == q else 1)
        xo = L.pp_obs_operand()
        if x:
            xo.p, xo.row_stride, xo.elem_stride = ptr, 0, 1
        return lib.pp_obs_logweight(kind, arr, xo, k, 1.0, lw, lp, rows_, m, n, None)
    for kind in OR.KINDS:
        assert call(kind=kind) == 0, kind
    assert call(lw=None, lp=ptr) == 0 and call(rows_=rows.ctypes.data, m=0, n=4) == 0
    bad = [dict(kind=2), dict(kind=5), dict(kind=14), dict(kind=-1), dict(k=0), dict(k=-3), dict(m=0, n=-1), dict(m=-1, n=0),
           dict(m=1, n=0), dict(m=0, n=4), dict(rows_=rows.ctypes.data, m=5, n=4), dict(kind=0, drop=1), dict(kind=13, drop=3),
           dict(kind=6, drop=0), dict(x=False), dict(lw=None, lp=None), dict(neg=0)]
    for kw in bad:
        before = buf.copy()
        assert call(**kw) != 0, kw
        assert b'pp_obs_logweight' in lib.pp_last_error(), kw
        assert np.array_equal(buf, before)


# ---- the restatement against the reference -----------------------------------------------------------------------------------
def _golden():
    return dict(np.load(os.path.join(GOLDEN, 'vec_lp.npz')))


@pytest.mark.parametrize('kind', OR.KINDS)
def test_restatement_matches_the_recorded_reference(kind):
    g = _golden()
    p, x, want = g['k%d_p' % kind], g['k%d_x' % kind], g['k%d_lp' % kind]
    n, k = x.shape
    assert (n, k) == (5, 67) and want.shape == (5,) and want.dtype == np.float32 and np.all(np.isfinite(want))
    got, _ = OR.row_lp(kind, list(p), x, n, k)
    np.testing.assert_allclose(got, want.astype(np.float64), **bar(want))


@pytest.mark.skipif(not HAVE_REFERENCE, reason='needs the live reference')
@pytest.mark.parametrize('kind', OR.KINDS)
def test_restatement_matches_the_live_reference(kind):
    import importlib.util
    import sys
    saved_path, saved_validate = list(sys.path), torch.distributions.Distribution._validate_args
    try:
        sys.path.insert(0, os.path.join(REPO, 'oracle', 'refstubs'))
        sys.path.insert(1, '/root/reference')
        import pyprob.distributions as R
        spec = importlib.util.spec_from_file_location('make_vec_lp_golden', os.path.join(GOLDEN, 'make_vec_lp_golden.py'))
        mk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mk)
        torch.distributions.Distribution.set_default_validate_args(False)
        p, x = mk.inputs(kind, np.random.RandomState(100 + kind))
        d = mk.reference_object(R, kind, p)
        want = d.log_prob(torch.from_numpy(x)).sum(-1).numpy()
    finally:
        sys.path[:] = saved_path
        torch.distributions.Distribution.set_default_validate_args(saved_validate)
    if kind == 11:
        p = [p[0], d.logits.numpy()]
    got, _ = OR.row_lp(kind, p, x, mk.N, mk.K)
    np.testing.assert_allclose(got, want.astype(np.float64), **bar(want))


# ---- stride classification ---------------------------------------------------------------------------------------------------
def test_stride_classification():
    from pyprob_amd.ops import obs_draw_strides
    n, k = 6, 24
    z = torch.zeros
    for what in ('obs_draw', 'obs_logweight'):
        cls = lambda t, n_=n, k_=k: obs_draw_strides(t, n_, k_, 'p', what)  # noqa: E731
        assert cls(z(())) == (0, 0) and cls(z(1)) == (0, 0) and cls(z(1, 1)) == (0, 0)
        assert cls(z(k)) == (0, 1) and cls(z(1, k)) == (0, 1)
        assert cls(z(n)) == (1, 0) and cls(z(n, 1)) == (1, 0)
        assert cls(z(n, k)) == (k, 1)
        assert cls(z(k), k, k) == (0, 1) and cls(z(k, 1), k, k) == (1, 0) and cls(z(k, k), k, k) == (k, 1)      # n == k
        for shape in ((n, k + 1), (k + 1,), (2, k), (n, 2, 3)):
            with pytest.raises(RuntimeError, match='must be a scalar'):
                cls(z(*shape))
    wide = lambda t: obs_draw_strides(t, n, k, 'p', 'obs_logweight')  # noqa: E731
    assert wide(z(n, 2, 3, 4)) == (k, 1) and wide(z(n, 4, 6)) == (k, 1)          # [n, *event]
    assert wide(z(n, 32)[:, :k]) == (32, 1)                                     # a padded [n, k] view
    for t in (z(n, 6, 4).transpose(1, 2), z(k, n).t(), z(n, 2 * k)[:, ::2], z(2 * k)[::2]):
        with pytest.raises(RuntimeError, match='must be contiguous'):          # its elements are not where the strides say
            wide(t)
    for t in (z(n, 2, 3, 4), z(n, 4, 6)):                                        # obs_draw takes what it took
        with pytest.raises(RuntimeError, match='must be a scalar'):
            obs_draw_strides(t, n, k)


def _runner():
    from pyprob_amd.is_engine import DistRunner
    r = DistRunner.__new__(DistRunner)
    r.dev = torch.device('cpu')
    r._consts = {}
    r._const = lambda v: torch.tensor([v], dtype=torch.float32)
    return r


def test_vec_term_reads_parameters_as_torch_broadcasts_them():
    from pyprob_amd.is_engine import VecTerm
    r, n = _runner(), 7
    img = torch.rand(n, 4, 5)
    t = r.vec_term(D.Normal(img, 0.1), (4, 5), n)
    assert type(t) is VecTerm and not t.fused and (t.kind, t.k) == (0, 20) and not t.shared
    assert t.p0[1:] == (20, 1) and t.p0[0].shape == (n, 20) and t.p1[1:] == (0, 0) and t.p2 is None and t.p3 is None
    assert t.p0[0].data_ptr() == img.data_ptr()                   # nothing was copied
    t = r.vec_term(D.Normal(torch.rand(4, 5), torch.rand(n, 1, 1) + 0.5), (4, 5), n)
    assert t.p0[1:] == (0, 1) and t.p1[1:] == (1, 0) and t.p1[0].shape == (n, 1)
    t = r.vec_term(D.Normal(torch.rand(4, 5), 0.3), (1, 4, 5), n)
    assert t.shared and t.p0[1:] == (0, 1) and t.k == 20
    t = r.vec_term(D.TruncatedNormal(torch.rand(n, 20), 1.0, -1.0, torch.full((20,), 3.0)), (20,), n)
    assert t.kind == 13 and [o[1:] for o in t.operands] == [(20, 1), (0, 0), (0, 0), (0, 1)]
    t = r.vec_term(D.Normal(torch.rand(n), 1.0), (n,), n)         # n == k: a 1-D tensor of k elements is the shared row
    assert t.shared and t.p0[1:] == (0, 1)
    # only a view that is not contiguous is copied, and `before_read` (the executor's flush) runs once before the first copy
    seen = []
    r.vec_term(D.Normal(img, torch.rand(n, 1, 1) + 0.5), (4, 5), n, before_read=lambda: seen.append(1))
    assert seen == []
    t = r.vec_term(D.TruncatedNormal(img.transpose(1, 2), 1.0, torch.rand(4, 5).t() - 3, 3.0), (5, 4), n, before_read=lambda: seen.append(1))
    assert seen == [1] and t.p0[1:] == (20, 1) and t.p2[1:] == (0, 1)
    assert torch.equal(t.p0[0], img.transpose(1, 2).reshape(n, 20))
    # what has no place in it: other families, and parameters that torch would broadcast in another way
    assert r.vec_term(D.Mixture([D.Normal(0.0, 1.0), D.Normal(1.0, 1.0)]), (20,), n) is None
    assert r.vec_term(D.Categorical(torch.rand(20, 3)), (20,), n) is None
    assert r.vec_term(D.Factor(log_prob=torch.zeros(20)), (20,), n) is None
    assert r.vec_term(D.Normal(torch.rand(5), 1.0), (4, 5), n) is None         # a row broadcast along the last dimension
    assert r.vec_term(D.Normal(torch.rand(n), 1.0), (20,), n) is None          # [n] against [k]: torch refuses it
    with pytest.raises(RuntimeError, match='k = 20'):
        r._check(t._replace(k=20), torch.zeros(19), n)


# ---- the lock-step route on the CPU double -----------------------------------------------------------------------------------
H = W = 20
yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing='ij')
PATTERNS = torch.stack([0.5 + 0.4 * torch.sin((yy * (1 + c % 3) + xx * (1 + c // 3)) * 0.35) for c in range(6)])
IMAGE = PATTERNS[2] * 1.05 + 0.1 * torch.randn(H, W, generator=torch.Generator().manual_seed(6))
ROW = torch.linspace(-1.0, 1.0, 37)
VEC = ROW * 0.9 + 0.2 * torch.randn(37, generator=torch.Generator().manual_seed(7))


class Captcha(Model):
    """d = floor(Uniform(0, 6)) (the CPU double of the draw operator has no Categorical), gain ~ Normal(1, 0.1); the image is the
    d-th pattern times the gain plus Normal pixel noise."""
    def forward(self):
        d = pyprob_amd.sample(D.Uniform(0.0, 6.0)).floor().clamp(0, 5)
        gain = pyprob_amd.sample(D.Normal(1.0, 0.1))
        pyprob_amd.observe(D.Normal(PATTERNS.to(d.device)[d.long()] * gain.reshape(-1, 1, 1), 0.1), name='img')
        return d


class TwoPath(Model):
    """The vector observe with a per-particle mean sits in one branch; the other branch scores the same observation under
    parameters shared by all particles."""
    def forward(self):
        u = pyprob_amd.sample(D.Uniform(0.0, 1.0))
        if u < 0.4:
            g = pyprob_amd.sample(D.Normal(1.0, 0.3))
            pyprob_amd.observe(D.Normal(ROW.to(u.device) * g.reshape(-1, 1), 0.2), name='vec')
        else:
            pyprob_amd.observe(D.Normal(ROW.to(u.device) * 0.5, 0.4), name='vec')
        return u


def normal_sum64(x, mean, sd):
    x, mean = np.asarray(x, np.float64), np.asarray(mean, np.float64)
    return np.sum(-0.5 * ((x - mean) / sd) ** 2 - np.log(sd) - 0.5 * np.log(2 * np.pi), axis=-1)


def captcha_want(post, m=None):
    d, gain = (next(iter(post.statement_log[j].values()))[0].double().cpu().numpy() for j in range(2))
    m = len(d) if m is None else m
    mean = PATTERNS.double().numpy()[np.clip(np.floor(d[:m]), 0, 5).astype(int)] * gain[:m, None, None]
    return normal_sum64(IMAGE.double().numpy().reshape(1, -1), mean.reshape(m, -1), 0.1)


def two_path_want(post):
    u, g = (next(iter(post.statement_log[j].values()))[0].double().cpu().numpy() for j in range(2))
    row, vec = ROW.double().numpy(), VEC.double().numpy()
    a = normal_sum64(vec[None], row[None] * g[:, None], 0.2)
    b = normal_sum64(vec, row * 0.5, 0.4)
    return np.where(u < 0.4, a, b), u


def _run(model, n, observe, route, monkeypatch, seed=3):
    if route is None:
        monkeypatch.delenv('PP_VEC_LIKELIHOOD', raising=False)
    else:
        monkeypatch.setenv('PP_VEC_LIKELIHOOD', route)
    before = OR.calls[0]
    post = model._traces_prior_lockstep(n, observe, seed=seed, device='cpu')
    return post, OR.calls[0] - before


def test_captcha_prior_is_goes_through_the_operator(cpu_doubles, monkeypatch):
    n = 96
    torch.manual_seed(4)
    post, calls = _run(Captcha(), n, {'img': IMAGE}, 'kernel', monkeypatch)
    assert calls >= 1 and post.num_paths == 1
    lw = post._all_log_weights.double().numpy()
    want = captcha_want(post)
    assert lw.shape == (n,) and np.all(np.isfinite(lw))
    np.testing.assert_allclose(lw, want, **bar(want))
    torch.manual_seed(4)
    ref, ref_calls = _run(Captcha(), n, {'img': IMAGE}, 'torch', monkeypatch)
    assert ref_calls == 0
    assert np.array_equal(captcha_want(ref), want)                # the same draws
    np.testing.assert_allclose(lw, ref._all_log_weights.double().numpy(), **bar(want))


def _copy_rows_cpu(self, src, dst, rows):
    """TEST DOUBLE of DistRunner.copy_rows (a direct C-ABI launch): dst[rows] = src[rows]."""
    src = src.as_subclass(torch.Tensor).reshape(-1).float()
    dst[rows] = src.expand(dst.numel())[rows]


def test_two_path_program_passes_the_rows_of_the_branch(cpu_doubles, monkeypatch):
    from pyprob_amd.is_engine import DistRunner
    monkeypatch.setattr(DistRunner, 'copy_rows', _copy_rows_cpu)
    n = 200
    torch.manual_seed(5)
    post, calls = _run(TwoPath(), n, {'vec': VEC}, 'kernel', monkeypatch)
    assert post.num_paths == 2 and calls >= 2                     # one call per observe: the branch's rows, the shared row
    want, u = two_path_want(post)
    assert 0 < (u < 0.4).sum() < n
    lw = post._all_log_weights.double().numpy()
    np.testing.assert_allclose(lw, want, **bar(want))
    torch.manual_seed(5)
    ref, ref_calls = _run(TwoPath(), n, {'vec': VEC}, 'torch', monkeypatch)
    assert ref_calls == 0 and np.array_equal(two_path_want(ref)[0], want)
    np.testing.assert_allclose(lw, ref._all_log_weights.double().numpy(), **bar(want))


def test_auto_keeps_the_torch_route_on_the_cpu_device(cpu_doubles, monkeypatch):
    torch.manual_seed(4)
    post, calls = _run(Captcha(), 32, {'img': IMAGE}, None, monkeypatch)
    assert calls == 0
    want = captcha_want(post)
    np.testing.assert_allclose(post._all_log_weights.double().numpy(), want, **bar(want))
    torch.manual_seed(4)
    post, calls = _run(Captcha(), 32, {'img': IMAGE}, 'auto', monkeypatch)
    assert calls == 0


class MixtureImage(Model):
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(0.0, 1.0))
        m = mu.reshape(-1, 1)
        pyprob_amd.observe(D.Mixture([D.Normal(m, 0.5), D.Normal(-m, 0.5)], probs=[0.3, 0.7]), name='vec')
        return mu


class CategoricalVector(Model):
    def forward(self):
        mu = pyprob_amd.sample(D.Normal(0.0, 1.0))
        w = torch.stack([torch.sigmoid(mu), 1 - torch.sigmoid(mu)], -1).reshape(-1, 1, 2)
        pyprob_amd.observe(D.Categorical(w.expand(-1, 5, 2)), name='c')
        return mu


def test_mixture_and_categorical_vectors_take_the_torch_route(cpu_doubles, monkeypatch):
    n = 40
    torch.manual_seed(8)
    post, calls = _run(MixtureImage(), n, {'vec': VEC}, 'kernel', monkeypatch)
    assert calls == 0
    mu = next(iter(post.statement_log[0].values()))[0].double().numpy()
    x = VEC.double().numpy()[None]
    comp = [np.log(w) - 0.5 * ((x - s * mu[:, None]) / 0.5) ** 2 - np.log(0.5) - 0.5 * np.log(2 * np.pi) for w, s in ((0.3, 1), (0.7, -1))]
    want = np.logaddexp(comp[0], comp[1]).sum(1)
    np.testing.assert_allclose(post._all_log_weights.double().numpy(), want, **bar(want))
    post, calls = _run(CategoricalVector(), n, {'c': torch.tensor([0., 1., 1., 0., 1.])}, 'kernel', monkeypatch)
    assert calls == 0
    p = 1 / (1 + np.exp(-next(iter(post.statement_log[0].values()))[0].double().numpy()))
    want = 2 * np.log(p) + 3 * np.log1p(-p)
    np.testing.assert_allclose(post._all_log_weights.double().numpy(), want, **bar(want))
