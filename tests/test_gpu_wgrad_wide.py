"""The weight-gradient launch alone (pp_debug_wgrad_run: csrc/wgrad_t1.hip without reduction jobs) with its 16-byte loop
(PP_WGRAD_WIDE=1, the default: float4 / float2 operand loads on v_mfma_f32_16x16x4_f32, tile edges in units of 16, the b128
LDS epilogue) and with the dword loop (PP_WGRAD_WIDE=0), both against init + A^T B in float64 on uniform(-1, 1) inputs with C
prefilled with random values. Bar, both arms: max |error| / max |reference| < 3e-6, the bar of
tests/test_gpu_kernels.py::test_gemm_grouped_launch for K = 1024 (every K here is smaller). The shapes are the smallest at
which the loop can go wrong: 16-wide edges on both sides, K no multiple of 4, several row ranges, fewer quad-rows than the
ring is deep, waves without rows, a NaN in the pad column, zero blocks, a row gather that crosses a 64-row index block, and
operands the 16-byte loop must refuse (odd pitch, pointer off by one float). One child process runs every case with both
switches (the switch is read per call) and hands the tensors back; the references are computed here once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 3e-6

# name: M, N, K, lda, ldb, ldc, then options (seed_of: the inputs of that case again)
CASES = {
    'a': dict(M=271, N=80, K=203, lda=272, ldb=80, ldc=80),
    'b': dict(M=30, N=271, K=64, lda=32, ldb=272, ldc=271),
    'c': dict(M=64, N=64, K=7, lda=64, ldb=64, ldc=64),
    'd': dict(M=271, N=80, K=203, lda=272, ldb=80, ldc=80, nan_col=271, seed_of='a'),
    'e': dict(M=256, N=68, K=200, lda=256, ldb=68, ldc=212, holes=[(0, 256, 64, 68, 0, 200), (64, 128, 0, 68, 0, 200)]),
    'f': dict(M=2048, N=512, K=700, lda=2048, ldb=512, ldc=512, gather=800),
    'g_pitch': dict(M=64, N=80, K=203, lda=67, ldb=80, ldc=80),
    'g_shift': dict(M=271, N=80, K=203, lda=272, ldb=80, ldc=80, a_shift=1),
    'h': dict(M=271, N=80, K=203, lda=272, ldb=80, ldc=80, twice=True, seed_of='a'),
}

SCRIPT = r'''
import os, sys, ctypes as C, numpy as np, torch
sys.path.insert(0, %(repo)r)
from pyprob_amd import lib as L
lib = L.load()
CASES = %(cases)r
dev = torch.device('cuda:0')
out = {}
for ci, (name, c) in enumerate(CASES.items()):
    g = torch.Generator().manual_seed(100 + list(CASES).index(c.get('seed_of', name)))
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    M, N, K, lda, ldb, ldc = (c[k] for k in ('M', 'N', 'K', 'lda', 'ldb', 'ldc'))
    shift = c.get('a_shift', 0)
    a_buf = u(K * lda + shift)
    A = a_buf[shift:].view(K, lda)
    if 'nan_col' in c:
        A[:, c['nan_col']] = float('nan')
    rows_b = c.get('gather', K)
    B = u(rows_b, ldb)
    idx = torch.randint(0, rows_b, (K,), generator=g, dtype=torch.int32) if 'gather' in c else None
    if idx is not None:
        idx[1::7] = idx[0::7][:idx[1::7].numel()]          # repeats
    init = u(M, ldc)
    out[name + '|A'], out[name + '|B'], out[name + '|init'] = A.numpy().copy(), B.numpy().copy(), init.numpy().copy()
    if idx is not None:
        out[name + '|idx'] = idx.numpy().copy()
    a_dev, b_dev = a_buf.to(dev), B.to(dev)
    idx_dev = idx.to(dev) if idx is not None else None
    zb = None
    if 'holes' in c:
        zb = np.ascontiguousarray(np.array(c['holes'], np.int32).reshape(1, 2, 6))
    for sw in ('1', '0'):
        os.environ['PP_WGRAD_WIDE'] = sw
        c_dev = init.to(dev)
        q = (L.pp_gemm_args * 1)()
        q[0].A, q[0].lda, q[0].B, q[0].ldb, q[0].C, q[0].ldc = a_dev.data_ptr() + 4 * shift, lda, b_dev.data_ptr(), ldb, c_dev.data_ptr(), ldc
        q[0].b_idx = idx_dev.data_ptr() if idx_dev is not None else None
        q[0].M, q[0].N, q[0].K, q[0].a_kmajor, q[0].b_kmajor, q[0].accumulate, q[0].split_k = M, N, K, 1, 1, 1, 1
        wide = np.full(64, -1, np.int32)
        torch.cuda.synchronize()
        for rep in range(2 if c.get('twice') else 1):
            k = lib.pp_debug_wgrad_run(q, zb.ctypes.data if zb is not None else None, 1, 1,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream), wide.ctypes.data, 64)
            assert k > 0, (name, sw, k)
        torch.cuda.synchronize()
        out['%%s|C|%%s' %% (name, sw)] = c_dev.cpu().numpy()
        out['%%s|wide|%%s' %% (name, sw)] = wide[:k].copy()
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    f = str(tmp_path_factory.mktemp('wgrad_wide') / 'out.npz')
    e = dict(os.environ, PP_DETERMINISTIC='0')
    e.pop('PP_WGRAD_WIDE', None)
    subprocess.run([sys.executable, '-c', SCRIPT % dict(repo=REPO, cases=CASES), f], check=True, env=e, timeout=300)
    return dict(np.load(f))


@pytest.fixture(scope='module')
def refs(run):
    """init + A^T B in float64 (the pad columns of the operands left out), once per case."""
    r = {}
    for name, c in CASES.items():
        M, N = c['M'], c['N']
        A = run[name + '|A'].astype(np.float64)[:, :M]
        B = run[name + '|B'].astype(np.float64)[:, :N]
        if name + '|idx' in run:
            B = B[run[name + '|idx']]
        prod = A.T @ B
        for (m0, m1, n0, n1, k0, k1) in c.get('holes', []):
            assert (k0, k1) == (0, c['K'])
            prod[m0:m1, n0:n1] = 0.0
        ref = run[name + '|init'].astype(np.float64)
        ref[:, :N] += (2 if c.get('twice') else 1) * prod
        r[name] = ref
    return r


def _errors(run, refs, name):
    """Both arms' max |error| / max |reference| over the product's columns, printed; the columns of C beyond N untouched."""
    c = CASES[name]
    N = c['N']
    ref = refs[name]
    scale = np.abs(ref[:, :N]).max()
    errs = {}
    for sw in ('1', '0'):
        got = run['%s|C|%s' % (name, sw)]
        assert np.all(np.isfinite(got)), (name, sw)
        np.testing.assert_array_equal(got[:, N:], run[name + '|init'][:, N:])
        errs[sw] = float(np.abs(got[:, :N].astype(np.float64) - ref[:, :N]).max() / scale)
    print('wgrad_wide case %s: max |error| / max |reference|: 16-byte loop %.3e, dword loop %.3e (bar %.1e)'
          % (name, errs['1'], errs['0'], BAR))
    return errs


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'f', 'h'])
def test_both_loops_against_float64(run, refs, name):
    """(a) 16-wide edges on both sides, K = 203, three row ranges; (b) M = 30 in a pitch of 32, one range of 64 rows: two
    quad-rows per wave under a ring of five; (c) K = 7: six of eight waves have no rows; (f) the row gather with repeated
    indices, 88 rows per wave: a wave crosses a 64-row index block; (h) two launches into the same C: init + 2 A^T B."""
    errs = _errors(run, refs, name)
    assert errs['1'] < BAR and errs['0'] < BAR, errs
    assert np.all(run[name + '|wide|0'] == 0)
    if name in ('a', 'b', 'f'):
        assert run[name + '|wide|1'].size >= 1 and np.all(run[name + '|wide|1'] == 1)


def test_nan_in_the_pad_column_stays_out(run, refs):
    """(d) = (a) with column 271 of A (the pad of lda = 272, which the 16-wide edge tile's lanes may load) filled with NaN:
    the stored result is finite and meets (a)'s bar against the reference of the same inputs without the pad."""
    errs = _errors(run, refs, 'd')
    assert np.array_equal(refs['d'], refs['a'])
    assert errs['1'] < BAR and errs['0'] < BAR, errs
    assert np.all(run['d|wide|1'] == 1)


def test_zero_blocks_are_left_bitwise_alone(run, refs):
    """(e) dW_ih-like: 256 x 68 in a tensor of pitch 212, the columns [64, 68) and the rows [64, 128) are zero blocks over all
    rows: C inside the holes (and beyond column 68) equals its prefill bitwise, outside it meets the bar."""
    errs = _errors(run, refs, 'e')
    assert errs['1'] < BAR and errs['0'] < BAR, errs
    init = run['e|init']
    for sw in ('1', '0'):
        got = run['e|C|%s' % sw]
        for (m0, m1, n0, n1, _, _) in CASES['e']['holes']:
            assert np.array_equal(got[m0:m1, n0:n1].view(np.uint32), init[m0:m1, n0:n1].view(np.uint32)), sw
    assert run['e|wide|1'].size >= 2 and np.all(run['e|wide|1'] == 1) and np.all(run['e|wide|0'] == 0)


@pytest.mark.parametrize('name', ['g_pitch', 'g_shift'])
def test_refused_operands_take_the_dword_loop(run, refs, name):
    """(g) lda = 67, and an A pointer one float past a 16-byte boundary: not wide under the default, and still right."""
    errs = _errors(run, refs, name)
    assert errs['1'] < BAR and errs['0'] < BAR, errs
    assert np.all(run[name + '|wide|1'] == 0) and np.all(run[name + '|wide|0'] == 0)
