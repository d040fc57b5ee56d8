"""Device resampling on the host side: the entry points of csrc/is_resample.hip (pp_is_cdf_workspace_bytes, pp_is_cdf_groups,
pp_is_resample_groups) and the PP_IS_CDF_TILE constant are declared, prototyped and exported; bad arguments are rejected before
anything touches a device; the float64 restatement's uniform for a known Philox block; the operators' schemas (through their CPU
doubles); a host-backed Empirical keeps its torch-generator draws and never reaches the new operators. The kernels are the
GPU's: tests/test_gpu_resample.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import resample_ref as R
from obs_draw_ref import philox4x32_10
from pyprob_amd import lib as L

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pp_is_cdf_workspace_bytes', 'pp_is_cdf_groups', 'pp_is_resample_groups')


def test_entry_points_are_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.PROTOTYPES, name
        assert hasattr(lib, name), name
        decl = hdr[hdr.index('%s(' % name):]
        decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
        assert decl.count(',') + 1 == len(L.PROTOTYPES[name][1]), name
    assert int(re.search(r'#define PP_IS_CDF_TILE (\d+)', hdr).group(1)) == L.PP_IS_CDF_TILE == 2048
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15          # additions only
    block = hdr[hdr.index('Resampling the particles of a lock-step posterior call'):hdr.index('#define PP_IS_CDF_TILE')]
    for ref in ('empirical.py:392-408', 'empirical.py:617-637', 'empirical.py:298-309'):
        assert ref in block, ref


def test_workspace_bytes_are_monotone():
    lib = L.load()
    T = L.PP_IS_CDF_TILE
    per = (1, 63, T - 1, T, T + 1, 2 * T + 1, 70001, 10 ** 6)
    for M in (0, 1, 3, 257, 70000):
        sizes = [lib.pp_is_cdf_workspace_bytes(M, n) for n in per if M * n <= 2 ** 31 - 1]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (M, sizes)
    for n in per:
        sizes = [lib.pp_is_cdf_workspace_bytes(M, n) for M in (0, 1, 2, 7, 64, 257, 2000) if M * n <= 2 ** 31 - 1]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0, (n, sizes)
    assert lib.pp_is_cdf_workspace_bytes(4, 10 ** 6) > lib.pp_is_cdf_workspace_bytes(1, 10 ** 6) > lib.pp_is_cdf_workspace_bytes(1, T)


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    M, N, K = 3, 5000, 7
    lw = torch.zeros(M * N)
    cdf = torch.zeros(M * N, dtype=torch.float64)
    stats = torch.zeros(M, 6, dtype=torch.float64)
    idx = torch.zeros(M * K, dtype=torch.int64)
    val = torch.zeros(M * K)
    ws_bytes = lib.pp_is_cdf_workspace_bytes(M, N)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8)

    def cdf_call(lw_p=lw.data_ptr(), m=M, n_per=N, out=cdf.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.pp_is_cdf_groups(lw_p, m, n_per, stats.data_ptr(), out, w, wb, None)

    def draw(c=cdf.data_ptr(), v=lw.data_ptr(), m=M, n_per=N, lo=0, hi=N, n_out=K, io=idx.data_ptr(), vo=val.data_ptr()):
        return lib.pp_is_resample_groups(c, v, m, n_per, lo, hi, n_out, 1, 0, io, vo, None)
    EINVAL, ENOSPACE = -1, -2
    assert cdf_call(lw_p=None) == EINVAL and cdf_call(out=None) == EINVAL and cdf_call(w=None) == EINVAL
    assert cdf_call(n_per=0) == EINVAL and cdf_call(n_per=-2) == EINVAL and cdf_call(m=-1) == EINVAL
    assert cdf_call(m=2 ** 20, n_per=2 ** 11, wb=2 ** 40) == EINVAL          # M n_per = 2^31
    assert b'pp_is_cdf_groups' in lib.pp_last_error()
    assert cdf_call(wb=ws_bytes - 1) == ENOSPACE and cdf_call(wb=0) == ENOSPACE
    assert b'workspace too small' in lib.pp_last_error()
    assert cdf_call(m=0) == 0                                                # no group: nothing to launch
    assert draw(c=None) == EINVAL
    assert draw(n_per=0) == EINVAL and draw(m=-1) == EINVAL and draw(n_out=-1) == EINVAL
    for lo, hi in ((-1, N), (0, N + 1), (5, 5), (6, 5), (N, N), (0, 0)):
        assert draw(lo=lo, hi=hi) == EINVAL, (lo, hi)
    assert draw(m=2 ** 20, n_per=2 ** 11, hi=2 ** 11) == EINVAL                # M n_per = 2^31
    assert draw(m=2 ** 16, n_per=1, hi=1, n_out=2 ** 15) == EINVAL             # M n_out = 2^31
    assert draw(io=None, vo=None) == EINVAL                                  # both outputs NULL
    assert draw(v=None) == EINVAL                                            # value_out without values
    assert b'pp_is_resample_groups' in lib.pp_last_error()
    assert draw(m=0) == 0 and draw(n_out=0) == 0                             # nothing to draw: no launch
    for t in (lw, cdf, idx, val):
        assert float(t.double().abs().sum()) == 0.0


def test_reference_uniform_for_a_known_philox_block():
    # Random123's known answer for Philox4x32-10 at counter 0, key 0
    w = philox4x32_10(0, 0, 0, 0, 0)
    assert [int(x) for x in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # the block uniform53 reads: counter words (lo, hi, 0x52, 0); 27 + 26 bits, + 0.5, 2^-53 - against exact rational arithmetic
    for seed, ctr in ((0, 0), (7, 1), (2 ** 61 + 5, 2 ** 40 + 3), (123456789, 2 ** 32 - 1)):
        w = [int(x) for x in philox4x32_10(seed, ctr & 0xFFFFFFFF, ctr >> 32, R.STREAM, 0)]
        bits = ((w[0] >> 5) << 26) + (w[1] >> 6)
        assert 0 <= bits < 2 ** 53
        u = float(R.uniform53(seed, np.asarray([ctr], np.uint64))[0])
        exact = Fraction(2 * bits + 1, 2 ** 54)
        assert abs(Fraction(u) - exact) <= Fraction(1, 2 ** 54) and 0.0 < u <= 1.0      # (bits + 0.5 rounds once above 2^52)
        if bits < 2 ** 52:
            assert Fraction(u) == exact
    # a uniform of 24 bits cannot tell these neighbours apart; this one can
    u = R.uniform53(11, np.arange(4096, dtype=np.uint64))
    assert len(np.unique(u)) == 4096 and len(np.unique(np.floor(u * 2 ** 53).astype(np.int64) & (2 ** 29 - 1))) > 4000


def test_operator_schemas_through_the_cpu_doubles():
    from pyprob_amd import ops as P
    R.register_cpu_doubles()
    rng = np.random.default_rng(0)
    M, N, K = 3, 70, 9
    lw = rng.normal(0, 3, (M, N)).astype(np.float32)
    lw[0, 3], lw[1, 5], lw[2, :] = -np.inf, np.nan, np.inf
    x = rng.normal(size=(M, N)).astype(np.float32)
    cdf = P.ops.is_cdf_groups(torch.from_numpy(lw.reshape(-1)), N, None)
    assert cdf.dtype == torch.float64 and cdf.shape == (M * N,)
    c = cdf.numpy().reshape(M, N)
    assert (np.diff(c, axis=1) >= 0).all() and c[0, 3] == c[0, 2] and c[1, 5] == c[1, 4] and (c[2] == 0).all()
    idx, val = P.ops.is_resample_groups(cdf, torch.from_numpy(x.reshape(-1)), N, 10, 60, K, 5, 100, True)
    assert idx.dtype == torch.int64 and idx.shape == (M * K,) and val.dtype == torch.float32 and val.shape == (M * K,)
    i = idx.numpy().reshape(M, K)
    assert ((i[:2] >= 10) & (i[:2] < 60)).all() and (i[2] == -1).all() and np.isnan(val.numpy().reshape(M, K)[2]).all()
    assert np.array_equal(val.numpy().reshape(M, K)[:2], np.take_along_axis(x[:2], i[:2], 1))
    none, only = P.ops.is_resample_groups(cdf, torch.from_numpy(x.reshape(-1)), N, 10, 60, K, 5, 100, False)
    assert none.numel() == 0 and torch.equal(only[:2 * K], val[:2 * K])
    # an M-group call consumes the counters of the M one-group calls at offset + g n_out
    for g in range(2):
        one, _ = P.ops.is_resample_groups(cdf[g * N:(g + 1) * N].contiguous(), None, N, 10, 60, K, 5, 100 + g * K, True)
        assert np.array_equal(one.numpy(), i[g])


def _forbid_new_operators(monkeypatch):
    from pyprob_amd import ops as P

    def boom(*a, **k):
        raise AssertionError('a host-backed Empirical reached a device resampling operator')
    monkeypatch.setattr(P.ops, 'is_cdf_groups', boom, raising=False)
    monkeypatch.setattr(P.ops, 'is_resample_groups', boom, raising=False)


def test_host_backed_empirical_keeps_its_torch_generator_draws(monkeypatch):
    from pyprob_amd.distributions import Empirical
    _forbid_new_operators(monkeypatch)
    rng = np.random.default_rng(3)
    n = 500
    vals = rng.normal(size=n)
    lw = rng.normal(0, 2, n)
    w = np.exp(lw - lw.max())
    cum = np.cumsum(w / w.sum())

    def expected(k, lo, hi):
        u = torch.rand(k, dtype=torch.float64).numpy()
        base = cum[lo - 1] if lo > 0 else 0.0
        return np.minimum(np.searchsorted(cum, base + u * (cum[hi - 1] - base), side='right'), hi - 1)
    for make in (lambda: Empirical(values=[float(v) for v in vals], log_weights=lw),
                 lambda: Empirical(values=[torch.tensor(float(v)) for v in vals], log_weights=lw),
                 # tensors that are not on a device: the host route as well
                 lambda: Empirical.from_device(torch.from_numpy(vals.astype(np.float32)), torch.from_numpy(lw.astype(np.float32)), None)):
        emp = make()
        if torch.is_tensor(emp._log_weights):
            w32 = np.exp(emp._log_weights.double().numpy() - emp._log_weights.double().numpy().max())
            cum = np.cumsum(w32 / w32.sum())
        ref_vals = emp.values_numpy()
        for lo, hi in ((0, n), (n // 3, n - n // 4)):
            torch.manual_seed(3)
            want = expected(64, lo, hi)
            torch.manual_seed(3)
            r = emp.resample(64, min_index=None if lo == 0 else lo, max_index=None if hi == n else hi)
            assert isinstance(r._values, list) and r.length == 64
            assert np.array_equal(r.values_numpy(), ref_vals[want])
            assert r.metadata['op'] == 'resample' and r.metadata['num_samples'] == 64 and r.metadata['length'] == n
            torch.manual_seed(3)
            want1 = expected(1, lo, hi)
            torch.manual_seed(3)
            assert float(emp.sample(min_index=lo, max_index=hi)) == ref_vals[want1[0]]
        assert np.isfinite(emp.median)          # weighted: resample(1000).median on the host route


def test_resample_batch_of_host_backed_posteriors_is_the_loop(monkeypatch):
    import pyprob_amd
    from pyprob_amd.distributions import Empirical
    _forbid_new_operators(monkeypatch)
    rng = np.random.default_rng(4)
    posts = [Empirical(values=[float(v) for v in rng.normal(g, 1, 50)], log_weights=rng.normal(0, 1, 50)) for g in range(3)]
    torch.manual_seed(8)
    out = pyprob_amd.resample_batch(posts, 20)
    torch.manual_seed(8)
    torch.randint(0, 2 ** 62, (1,))          # (the key resample_batch takes from the generator)
    ref = [p.resample(20) for p in posts]
    assert len(out) == 3 and all(o.length == 20 for o in out)
    for o, r in zip(out, ref):
        assert np.array_equal(o.values_numpy(), r.values_numpy())
    assert pyprob_amd.resample_batch([], 5) == []
