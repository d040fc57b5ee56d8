"""The host side of the live-chunk Adam launch (csrc/adam_live.hpp): the run builder over a tensor layout - all live; the first,
a middle or the last tensor dead; two adjacent dead tensors; more runs than the kernel-argument table holds (full grid); weight
decay (everything live) - and the per-buffer record: marks are sticky, a table is built once per state of the marks and reused.
No device is touched: the bound "buffers" are host arrays whose addresses only key the record. The kernels are the GPU's:
tests/test_gpu_adam_live.py."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from pyprob_amd import lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RUNS = 4
CHUNKS = (1, 3, 33, 2, 40)          # the layout of tests/test_gpu_adam_live.py
SYMBOLS = ('pp_adam_step_live', 'pp_adam_live_bind', 'pp_adam_live_unbind', 'pp_adam_live_mark_touched', 'pp_adam_live_mark_range',
           'pp_adam_live_info',
           'pp_adam_live_plan', 'pp_adam_live_table')


def firsts(chunks):
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(chunks)]), np.int32)


def unpack(out):
    n_runs, blocks, n_gaps = (int(x) for x in out[:3])
    runs = [(int(out[3 + 2 * r]), int(out[4 + 2 * r])) for r in range(n_runs)]           # (first workgroup, first chunk)
    gaps = [(int(out[11 + 2 * g]), int(out[12 + 2 * g])) for g in range(n_gaps)]         # [first tensor, end tensor)
    return dict(blocks=blocks, runs=runs, gaps=gaps)


def plan(chunks, live):
    lib = L.load()
    first = firsts(chunks)
    lv = np.ascontiguousarray(live, np.uint8)
    out = np.full(21, -7, np.int32)
    rc = lib.pp_adam_live_plan(first.ctypes.data, len(chunks), lv.ctypes.data, out.ctypes.data)
    return rc, (unpack(out) if rc == 0 else None)


def expected(chunks, live):
    """Restated from the definition: workgroup i of the launch owns the i-th live chunk; a gap is a maximal dead tensor range."""
    first = firsts(chunks)
    owner = [c for t in range(len(chunks)) if live[t] for c in range(first[t], first[t + 1])]
    dead = [t for t in range(len(chunks)) if not live[t]]
    return owner, dead


def chunk_of_block(p, i):
    r = max(k for k, (blk, _) in enumerate(p['runs']) if blk <= i)
    return p['runs'][r][1] + i - p['runs'][r][0]


@pytest.mark.parametrize('dead', [(), (0,), (2,), (4,), (1, 2), (0, 4), (1, 3), (0, 2, 4), (0, 1, 2, 3, 4)])
def test_runs_cover_exactly_the_live_chunks(dead):
    live = [0 if t in dead else 1 for t in range(len(CHUNKS))]
    rc, p = plan(CHUNKS, live)
    assert rc == 0
    owner, dead_t = expected(CHUNKS, live)
    assert p['blocks'] == len(owner)
    assert [chunk_of_block(p, i) for i in range(p['blocks'])] == owner
    assert sorted(t for a, b in p['gaps'] for t in range(a, b)) == dead_t
    assert all(a < b for a, b in p['gaps'])
    # maximal runs: adjacent live tensors share one, adjacent dead tensors share one gap
    n_runs = sum(1 for t in range(len(CHUNKS)) if live[t] and (t == 0 or not live[t - 1]))
    n_gaps = sum(1 for t in range(len(CHUNKS)) if not live[t] and (t == 0 or live[t - 1]))
    assert (len(p['runs']), len(p['gaps'])) == (n_runs, n_gaps)


def test_more_runs_than_the_table_holds_is_the_full_grid():
    chunks = [2] * 9
    rc, p = plan(chunks, [1, 0, 1, 0, 1, 0, 1, 0, 0])        # four runs, four gaps: fits
    assert rc == 0 and len(p['runs']) == MAX_RUNS and len(p['gaps']) == 4
    rc, p = plan(chunks, [1, 0, 1, 0, 1, 0, 1, 0, 1])        # five runs
    assert rc == 1 and p is None
    rc, p = plan([2] * 11, [0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0])   # four runs, five gaps: the gap table's last slot
    assert rc == 0 and len(p['gaps']) == 5
    rc, p = plan([2] * 11, [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0])   # five runs, six gaps
    assert rc == 1


def test_bad_arguments():
    lib = L.load()
    out = np.zeros(21, np.int32)
    first = firsts(CHUNKS)
    lv = np.ones(5, np.uint8)
    assert lib.pp_adam_live_plan(None, 5, lv.ctypes.data, out.ctypes.data) < 0
    assert lib.pp_adam_live_plan(first.ctypes.data, 0, lv.ctypes.data, out.ctypes.data) < 0
    g = np.zeros(1024, np.float32)
    ok = np.array([0, 1, 1], np.int32)
    assert lib.pp_adam_live_bind(g.ctypes.data, g.ctypes.data, g.ctypes.data, 1000, ok.ctypes.data, 2, 1) != 0    # not padded
    desc = np.array([0, 2, 1], np.int32)     # descends
    assert lib.pp_adam_live_bind(g.ctypes.data, g.ctypes.data, g.ctypes.data, 1024, desc.ctypes.data, 2, 1) != 0
    beyond = np.array([0, 1, 2], np.int32)   # ends past the buffer's single chunk
    assert lib.pp_adam_live_bind(g.ctypes.data, g.ctypes.data, g.ctypes.data, 1024, beyond.ctypes.data, 2, 1) != 0
    info = np.zeros(4, np.int64)
    assert lib.pp_adam_live_info(g.ctypes.data, info.ctypes.data, None) == 0 and info[0] == 0    # none of them was bound


class Record:
    """Host arrays standing in for an engine's gradient / moment buffers (their addresses key the record; nothing reads them)."""

    def __init__(self, chunks, clean=True):
        self.lib = L.load()
        self.chunks = chunks
        self.n = 1024 * int(sum(chunks))
        self.g, self.m, self.v = (np.zeros(self.n, np.float32) for _ in range(3))
        self.first = firsts(chunks)
        assert self.lib.pp_adam_live_bind(self.g.ctypes.data, self.m.ctypes.data, self.v.ctypes.data, self.n,
                                          self.first.ctypes.data, len(chunks), 1 if clean else 0) == 0

    def close(self):
        self.lib.pp_adam_live_unbind(self.g.ctypes.data)

    def info(self):
        out = np.zeros(4, np.int64)
        touched = np.zeros(len(self.chunks), np.uint8)
        assert self.lib.pp_adam_live_info(self.g.ctypes.data, out.ctypes.data, touched.ctypes.data) == 0
        return dict(bound=int(out[0]), version=int(out[1]), builds=int(out[2]), untouched=int(out[3])), touched.astype(bool)

    def table(self, wd=0.0, m=None):
        out = np.full(21, -7, np.int32)
        rc = self.lib.pp_adam_live_table(self.g.ctypes.data, (self.m if m is None else m).ctypes.data, self.v.ctypes.data, self.n,
                                         len(self.chunks), wd, out.ctypes.data)
        return rc, (unpack(out) if rc == 0 else None)


def test_marks_are_sticky_and_the_table_is_cached():
    r = Record(CHUNKS)
    try:
        info, touched = r.info()
        assert info['bound'] == 1 and info['untouched'] == 5 and not touched.any()
        rc, p = r.table()
        assert rc == 0 and p['blocks'] == 0 and p['gaps'] == [(0, 5)]
        # a pointer into tensor 2 (the ABI calls that take a destination mark ALL tensors of the buffer it lies in)
        assert r.lib.pp_adam_live_mark_touched(r.g.ctypes.data + 4 * 1024 * 5) == 0
        info, touched = r.info()
        assert touched.all() and info['untouched'] == 0
        v0 = info['version']
        r.lib.pp_adam_live_mark_touched(r.g.ctypes.data)
        assert r.info()[0]['version'] == v0          # nothing new: the state of the marks stands
        b0 = r.info()[0]['builds']
        rc, p = r.table()
        assert rc == 0 and p['blocks'] == sum(CHUNKS) and p['runs'] == [(0, 0)] and p['gaps'] == []
        assert r.info()[0]['builds'] == b0 + 1
        for _ in range(5):
            assert r.table()[1] == p
        assert r.info()[0]['builds'] == b0 + 1       # the steady state builds nothing
    finally:
        r.close()
    r = Record(CHUNKS)
    try:      # one tensor at a time: floats of tensor 2's last chunk and tensor 3's first one
        first = firsts(CHUNKS)
        assert r.lib.pp_adam_live_mark_range(r.g.ctypes.data, 1024 * int(first[3]) - 1, 2) == 0
        assert r.info()[1].tolist() == [False, False, True, True, False]
        rc, p = r.table()
        assert rc == 0 and p['runs'] == [(0, int(first[2]))] and p['blocks'] == 35 and p['gaps'] == [(0, 2), (4, 5)]
        r.lib.pp_adam_live_mark_range(r.g.ctypes.data, -5, 3)            # outside the buffer: nothing
        r.lib.pp_adam_live_mark_range(r.g.ctypes.data, r.n, 10)
        assert r.info()[1].tolist() == [False, False, True, True, False]
    finally:
        r.close()
    assert r.info()[0]['bound'] == 0
    assert r.table()[0] == 1                         # not bound: the full grid


def test_weight_decay_makes_every_tensor_live_for_good():
    r = Record(CHUNKS)
    try:
        rc, p = r.table(wd=0.0)
        assert rc == 0 and p['blocks'] == 0
        rc, p = r.table(wd=1e-4)
        assert rc == 0 and p['blocks'] == sum(CHUNKS) and p['gaps'] == []
        assert r.info()[1].all()                     # a decayed step moves every tensor's moments: none is zero afterwards
        rc, p = r.table(wd=0.0)
        assert rc == 0 and p['blocks'] == sum(CHUNKS)
    finally:
        r.close()


def test_moments_in_the_gradient_or_moment_buffers_and_foreign_moment_buffers_mark_everything():
    r = Record(CHUNKS)
    try:
        assert r.lib.pp_adam_live_mark_touched(r.v.ctypes.data + 4 * 77) == 0       # a pointer into exp_avg_sq
        assert r.info()[1].all()
    finally:
        r.close()
    r = Record(CHUNKS)
    try:
        other = np.zeros(r.n, np.float32)
        rc, p = r.table(m=other)                     # Adam called with moment buffers the record does not know
        assert rc == 0 and p['blocks'] == sum(CHUNKS) and r.info()[1].all()
    finally:
        r.close()
    r = Record(CHUNKS, clean=False)                  # bound over buffers with unknown contents
    try:
        assert r.info()[1].all()
    finally:
        r.close()


def test_rebinding_replaces_the_record():
    r = Record(CHUNKS)
    try:
        r.lib.pp_adam_live_mark_touched(r.g.ctypes.data)
        assert r.info()[1].all()
        assert r.lib.pp_adam_live_bind(r.g.ctypes.data, r.m.ctypes.data, r.v.ctypes.data, r.n, r.first.ctypes.data, len(CHUNKS), 1) == 0
        assert not r.info()[1].any()
    finally:
        r.close()


def test_entry_points_are_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.PROTOTYPES, name
        assert hasattr(lib, name), name
        decl = hdr[hdr.rindex('int %s(' % name):]
        decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
        assert decl.count(',') + 1 == len(L.PROTOTYPES[name][1]), name
    assert len(L.PROTOTYPES['pp_adam_step_live'][1]) == len(L.PROTOTYPES['pp_adam_step'][1])
    assert lib.pp_abi_version() == L.PP_ABI_VERSION          # additions only
    assert C.sizeof(C.c_void_p) == 8
