"""Batched posteriors for image and vector observations without a device: pp_obs_logweight_groups is declared, prototyped and
exported (ABI 15); pp_is_batch_workspace_bytes grows by the feature block and the convolution scratch for a CNN2D5C observable
and keeps, byte for byte, the size it had for a network without one; the operator's operand classification; the observe dict
Model._traces_lockstep_batch hands to the program. The device side is tests/test_gpu_obs_logweight_groups.py and
tests/test_gpu_is_batch_image.py."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from conftest import load_golden
from helpers import spec_from_golden
from is_helpers import lockstep_network
from pyprob_amd import lib as L
from pyprob_amd import state

torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    lib = L.load()
    name = 'pp_obs_logweight_groups'
    assert name in set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr)) and name in L.PROTOTYPES and hasattr(lib, name)
    res, args = L.PROTOTYPES[name]
    assert res is C.c_int and len(args) == 11 and args[1] is C.POINTER(L.pp_obs_operand) and args[2] is L.pp_obs_operand
    decl = hdr[hdr.index('int %s(' % name):]
    decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
    assert decl.count(',') + 1 == len(args)
    assert int(re.search(r'#define PP_OBS_PER_GROUP_X (\d+)', hdr).group(1)) == L.PP_OBS_PER_GROUP_X == 16
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15
    assert hasattr(torch.ops.pyprob_hip, 'obs_logweight_groups')
    # refused on the host, before any launch: the pointers are host addresses no kernel may see
    buf = torch.zeros(64)
    arr = (L.pp_obs_operand * 4)()
    for q in range(2):
        arr[q].p, arr[q].row_stride, arr[q].elem_stride = buf.data_ptr(), 0, 0
    xo = L.pp_obs_operand()
    xo.p, xo.row_stride, xo.elem_stride = buf.data_ptr(), 4, 1
    for kind, mask, k, m, n_per, lw in ((5, 16, 4, 2, 3, buf), (0, 32, 4, 2, 3, buf), (0, 16, 0, 2, 3, buf), (0, 16, 4, 2, 0, buf),
                                        (0, 16, 4, -1, 3, buf), (0, 16, 4, 2, 3, None)):
        rc = lib.pp_obs_logweight_groups(kind, arr, xo, mask, k, 1.0, None if lw is None else lw.data_ptr(), None, m, n_per, None)
        assert rc != 0 and b'pp_obs_logweight_groups' in lib.pp_last_error(), (kind, mask, k, m, n_per)
    assert lib.pp_obs_logweight_groups(0, arr, xo, 16, 4, 1.0, buf.data_ptr(), None, 0, 3, None) == 0      # no group: no launch
    assert float(buf.abs().sum()) == 0.0


def _cnn_engine(emb, H=32):
    from pyprob_amd.spec import NetSpec
    return oracle_ops.CpuBufferEngine(NetSpec(emb, lstm_dim=H), seed=1)


def test_workspace_bytes_of_networks_with_an_image_observable():
    from pyprob_amd import ObserveEmbedding
    lib = L.load()
    img = {'dim': 16, 'reshape': [1, 20, 20], 'embedding': ObserveEmbedding.CNN2D5C}
    for emb in ({'img': img}, {'y': {'dim': 8}, 'img': img}, {'a': dict(img, reshape=[2, 20, 21]), 'b': img}):
        eng = _cnn_engine(emb)
        net = C.byref(eng.net)
        cnn = [o for o in range(eng.net.n_obs) if eng.net.obs_kind[o] == L.PP_OBS_CNN2D5C]
        sizes = []
        for M in (1, 2, 7, 64, 257):
            size = int(lib.pp_is_batch_workspace_bytes(net, M))
            stack = sum(int(lib.pp_cnn2d5c_workspace_bytes(net, o, M)) for o in cnn)
            feat = sum(4 * M * ((int(eng.net.obs_feat[o]) + 3) & ~3) for o in cnn)
            assert stack > 0 and size > stack + feat, (list(emb), M, size, stack, feat)
            sizes.append(size)
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes


def _parent_rows_bytes(net, M):
    """The blocks of the batch workspace in front of the fragment images as the carve laid them out before image observables
    existed (csrc/is_batch.hip batch_carve): every block starts at a multiple of 256 bytes and holds at least 4."""
    off = 0

    def take(nbytes):
        nonlocal off
        off = ((off + 255) & ~255) + max(int(nbytes), 4)
    r4 = lambda v: (int(v) + 3) & ~3      # noqa: E731
    M = max(M, 1)
    take(max(M, 256) * 48)
    Hd = max(1, int(net.lstm_dim))
    e4, i4 = r4(net.e_obs), r4(net.lstm_in)
    hid4 = r4(max([1] + [int(net.addrs[a].hid) for a in range(net.n_addr)]))
    ohid4 = max([4] + [r4(net.obs_hid[o]) for o in range(net.n_obs)])
    for floats in (M * ohid4, M * ohid4, M * e4, M * e4, M * e4, M * i4, M * 4 * Hd, M * hid4, M * Hd, M * Hd):
        take(4 * floats)
    return (off + 255) & ~255


def test_workspace_bytes_without_an_image_observable_are_unchanged():
    """The gum golden network: the sizes the library gave before this entry point knew image observables (recorded from that
    build), and their growth with M restated from that carve."""
    lib = L.load()
    meta, params, batch, loss, isr = load_golden('gum')
    eng = oracle_ops.CpuBufferEngine(spec_from_golden(meta, params))
    before = {1: 112896, 7: 133632, 257: 1001984, 4096: 14514432}
    for M, want in before.items():
        got = int(lib.pp_is_batch_workspace_bytes(C.byref(eng.net), M))
        assert got == want, (M, got, want)
        assert got - before[1] == _parent_rows_bytes(eng.net, M) - _parent_rows_bytes(eng.net, 1), M


def test_operand_classification_of_the_grouped_operator():
    from pyprob_amd.ops import obs_group_operands
    M, N, k = 3, 5, 12
    n = M * N
    sd = torch.ones(1)
    mean = torch.zeros(n, k)

    def classify(x, mask=L.PP_OBS_PER_GROUP_X, p0=mean):
        return [None if o is None else o[1:] for o in obs_group_operands([p0, sd, None, None], x, mask, M, N, k)]
    assert classify(torch.zeros(M, k)) == [(k, 1), (0, 0), None, None, (k, 1)]
    assert classify(torch.zeros(M, 1, 3, 4))[4] == (k, 1)                      # [M, *event]
    assert classify(torch.zeros(M, k + 4)[:, :k])[4] == (k + 4, 1)             # a padded [M, k] view
    assert classify(torch.zeros(k))[4] == (0, 1)                               # one row for every group
    assert classify(torch.zeros(M, 1))[4] == (1, 0)
    assert classify(torch.zeros(n, 3, 4), mask=0)[4] == (k, 1)                 # x per particle
    assert classify(torch.zeros(M, k), p0=torch.zeros(n, 1))[0] == (1, 0)
    assert classify(torch.zeros(M, k), p0=torch.zeros(n, k + 3)[:, :k])[0] == (k + 3, 1)
    assert classify(torch.zeros(M, k), mask=L.PP_OBS_PER_GROUP_X | 1, p0=torch.zeros(M, k))[0] == (k, 1)
    for bad in (dict(x=torch.zeros(n, k)),                                     # a per-group operand with M N rows
                dict(x=torch.zeros(M, k), mask=L.PP_OBS_PER_GROUP_X | 1),      # ... and the mean marked per group
                dict(x=torch.zeros(M, k), mask=0),                             # M rows where M N are read
                dict(x=torch.zeros(M, k + 1)), dict(x=torch.zeros(M, k).double()),
                dict(x=torch.zeros(M, 2 * k)[:, ::2])):
        with pytest.raises(RuntimeError):
            classify(**bad)


def test_the_program_sees_group_tensors_of_the_event_shape(monkeypatch):
    model, net, meta, params = lockstep_network()
    M, N = 5, 8
    rng = np.random.default_rng(1)
    cols = {'obs0': rng.random((M, 1), dtype=np.float32), 'obs1': rng.random((M, 1), dtype=np.float32),
            'img': rng.random((M, 6), dtype=np.float32), 'vec': rng.random((M, 4), dtype=np.float32)}
    seen = []

    def recorded(obs, m, *args, **kwargs):
        seen.append((m, dict(obs), obs.matrix))
        return []
    monkeypatch.setattr(model, '_run_lockstep_batch', recorded)
    model._traces_lockstep_batch(N, list(cols), cols, 3, 0, 1.0, event_shapes={'obs0': (), 'obs1': (), 'img': (1, 2, 3)})
    (m, obs, matrix), = seen
    assert m == M and matrix.shape == (M, 2)
    assert all(type(t) is state.GroupTensor for t in obs.values())
    shapes = {k: tuple(t.as_subclass(torch.Tensor).shape) for k, t in obs.items()}
    assert shapes == {'obs0': (M,), 'obs1': (M,), 'img': (M, 1, 2, 3), 'vec': (M, 4)}      # (no shape given: a flat vector)
    np.testing.assert_array_equal(obs['img'].as_subclass(torch.Tensor).numpy().reshape(M, 6), cols['img'])
    assert obs['img'].numel() == 6 * M and obs['img'].dim() == 4      # metadata may be asked for
    for compute in (lambda t: t + 1.0, lambda t: t.sum(), lambda t: torch.zeros(M * N, 1, 2, 3) - t, lambda t: t[0], lambda t: bool(t[0, 0, 0, 0])):
        with pytest.raises(state.BatchUnsupported):
            compute(obs['img'])


def test_normalise_observes_keeps_its_results_and_posterior_results_batch_passes_the_event_shapes(monkeypatch):
    from pyprob_amd.model import Model
    images = torch.arange(24.0).reshape(2, 1, 3, 4)
    names, dicts, cols = Model._normalise_observes({'img': images})
    assert cols['img'].shape == (2, 12) and tuple(dicts[1]['img'].shape) == (1, 3, 4)
    model, net, meta, params = lockstep_network()
    got = {}

    def recorded(num_traces, names, cols, *args, event_shapes=None, **kwargs):
        got.update(event_shapes)
        raise state.BatchUnsupported('recorded')
    monkeypatch.setattr(model, '_traces_lockstep_batch', recorded)
    monkeypatch.setattr(net._is, 'batch_supported', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())      # (the stand-in runner is on the host)
    monkeypatch.setattr(model, 'posterior_results', lambda *a, **k: None)
    observes = [{'obs0': 1.0, 'obs1': torch.zeros(3, 4)}, {'obs0': 2.0, 'obs1': torch.ones(3, 4)}]
    assert model.posterior_results_batch(4, observes, lock_step=True) == [None, None]
    assert got == {'obs0': (), 'obs1': (3, 4)} and model._batch_ok is False
