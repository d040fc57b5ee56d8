"""Host rule of the weight-gradient launch's 16-byte loop (csrc/wgrad_t1.hip, wgrad_t1_build), no device work: a problem is
`wide` when both operand pointers are 16-byte aligned after the zero-block cuts, both pitches are multiples of 4 floats and
every float2 / float4 of its last tile ends inside the row pitch; PP_WGRAD_WIDE=0 (read per call) clears every flag.
pp_debug_wgrad_run with launch = 0 on fake pointers, as tests/test_host.py drives pp_debug_wgrad_plan."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    from pyprob_amd import build as B
    B.build()
    from pyprob_amd import lib as L
    return L.load()


def _wide(lib, products, zero_blocks=None, a_shift=0):
    """products: dicts M, N, K, lda, ldb, ldc [, gather] -> ([(M, N, wide)] in the plan's order)."""
    from pyprob_amd import lib as L
    n = len(products)
    arr = (L.pp_gemm_args * n)()
    for i, p in enumerate(products):
        base = 0x10000000 * (i + 1)                      # fake device addresses: never dereferenced with launch = 0
        a = arr[i]
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc = base + 4 * a_shift, p['lda'], base + 0x4000000, p['ldb'], base + 0x8000000, p['ldc']
        a.b_idx = base + 0xC000000 if p.get('gather') else None
        a.M, a.N, a.K, a.a_kmajor, a.b_kmajor, a.accumulate, a.split_k = p['M'], p['N'], p['K'], 1, 1, 1, 1
    zb = None
    if zero_blocks is not None:
        zb = np.ascontiguousarray(zero_blocks, np.int32).reshape(n, 2, 6)
    plan = np.zeros((64, 10), np.int64)
    nb = C.c_int32(0)
    k = lib.pp_debug_wgrad_plan(arr, zb.ctypes.data if zb is not None else None, n, plan.ctypes.data, 64, C.byref(nb))
    wide = np.full(64, -1, np.int32)
    k2 = lib.pp_debug_wgrad_run(arr, zb.ctypes.data if zb is not None else None, n, 0, None, wide.ctypes.data, 64)
    assert k == k2 and k > 0
    assert set(wide[:k].tolist()) <= {0, 1} and np.all(wide[k:] == -1)
    return [(int(plan[i, 0]), int(plan[i, 1]), int(wide[i])) for i in range(k)]


def _step_products(H=512, B=1024, I=212):
    prods = [dict(M=4 * H, N=68, K=B, lda=4 * H, ldb=68, ldc=I), dict(M=30, N=271, K=B, lda=32, ldb=272, ldc=271),
             dict(M=271, N=512, K=B, lda=272, ldb=512, ldc=512), dict(M=64, N=64, K=B, lda=64, ldb=64, ldc=64),
             dict(M=32, N=16, K=B, lda=64, ldb=16, ldc=16)]
    zb = np.zeros((5, 2, 6), np.int32)
    zb[0, 0] = (0, 4 * H, 64, 68, 0, B)                  # columns [64, 68): no previous variable at t = 0
    zb[0, 1] = (H, 2 * H, 0, 68, 0, B)                   # forget gate: c_{-1} = 0
    return prods, zb


def test_single_statement_step_is_all_wide(lib, monkeypatch):
    """The six problems of a GUM step (B = 1024, H = 512; the products of tests/test_host.py's plan test)."""
    monkeypatch.delenv('PP_DETERMINISTIC', raising=False)
    monkeypatch.delenv('PP_WGRAD_WIDE', raising=False)
    prods, zb = _step_products()
    plan = _wide(lib, prods, zb)
    assert len(plan) == 6 and all(w == 1 for _, _, w in plan), plan
    monkeypatch.setenv('PP_WGRAD_WIDE', '1')
    assert _wide(lib, prods, zb) == plan


def test_switch_clears_every_flag(lib, monkeypatch):
    monkeypatch.delenv('PP_DETERMINISTIC', raising=False)
    prods, zb = _step_products()
    monkeypatch.setenv('PP_WGRAD_WIDE', '0')
    plan = _wide(lib, prods, zb)
    assert len(plan) == 6 and all(w == 0 for _, _, w in plan), plan
    monkeypatch.delenv('PP_WGRAD_WIDE')                  # read per call: the same process, the flags are back
    assert all(w == 1 for _, _, w in _wide(lib, prods, zb))


def test_what_is_not_wide(lib, monkeypatch):
    monkeypatch.delenv('PP_DETERMINISTIC', raising=False)
    monkeypatch.delenv('PP_WGRAD_WIDE', raising=False)
    ok = dict(M=271, N=80, K=203, lda=272, ldb=80, ldc=80)
    assert _wide(lib, [ok]) == [(271, 80, 1)]
    # a cut that starts at an odd column: the hole [0, M) x [0, 3) leaves columns [3, 80) - the B pointer moves by 3 floats
    zb = np.zeros((1, 2, 6), np.int32)
    zb[0, 0] = (0, 271, 0, 3, 0, 203)
    assert _wide(lib, [ok], zb) == [(271, 77, 0)]
    # the same cut at a multiple of 4 stays wide
    zb[0, 0] = (0, 271, 0, 4, 0, 203)
    assert _wide(lib, [ok], zb) == [(271, 76, 1)]
    # an odd pitch, an operand pointer off by one float
    assert _wide(lib, [dict(ok, lda=271)]) == [(271, 80, 0)]
    assert _wide(lib, [dict(ok, M=64, lda=67)]) == [(64, 80, 0)]
    assert _wide(lib, [ok], a_shift=1) == [(271, 80, 0)]
    # a float4 of the last tile that would end outside the row: M = 40 is a 64-wide tile (vectors up to column 63), lda = 44
    assert _wide(lib, [dict(ok, M=40, lda=44)]) == [(40, 80, 0)]
    assert _wide(lib, [dict(ok, M=40, lda=64)]) == [(40, 80, 1)]
    # a 16-wide edge loads single clamped floats: M = 257 in a pitch of 260
    assert _wide(lib, [dict(ok, M=257, lda=260)]) == [(257, 80, 1)]
    # the row gather is no obstacle
    assert _wide(lib, [dict(M=2048, N=512, K=700, lda=2048, ldb=512, ldc=512, gather=True)]) == [(2048, 512, 1)]
