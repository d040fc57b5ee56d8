"""Batched posteriors on the host: the three C-ABI entry points (pp_is_batch_workspace_bytes, pp_is_batch_first,
pp_is_fused_groups) are declared, prototyped and exported; Model.posterior_results_batch normalises both forms of `observes`,
rejects unequal keys and M = 0, and - on the oracle-backed CPU stand-ins of the IS operators (tests/oracle_ops.py) - serves a
two-statement program by the loop of posterior_results calls with the counter offsets offset + g * num_traces. The device
side is tests/test_gpu_is_batch.py."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from conftest import load_golden
from helpers import spec_from_golden
from is_helpers import lockstep_network
from pyprob_amd import lib as L
from pyprob_amd.model import Model
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pp_is_batch_workspace_bytes', 'pp_is_batch_first', 'pp_is_fused_groups')
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK


def test_entry_points_are_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert len(L.PROTOTYPES['pp_is_batch_first'][1]) == 12 and len(L.PROTOTYPES['pp_is_fused_groups'][1]) == 19
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15
    # every entry cites the reference lines it replaces
    block = hdr[hdr.index('Batched posteriors'):hdr.index('size_t pp_is_batch_workspace_bytes')]
    for ref in ('pyprob/model.py', 'pyprob/nn/inference_network.py', 'pyprob/nn/inference_network_lstm.py', 'pyprob/state.py',
                'pyprob/distributions/empirical.py'):
        assert ref in block, ref


def test_workspace_bytes_of_the_gum_golden_network():
    meta, params, batch, loss, isr = load_golden('gum')
    eng = oracle_ops.CpuBufferEngine(spec_from_golden(meta, params))
    lib = L.load()
    one = lib.pp_is_batch_workspace_bytes(C.byref(eng.net), 1)
    many = lib.pp_is_batch_workspace_bytes(C.byref(eng.net), 4096)
    assert one > 0 and many > one
    assert lib.pp_is_batch_workspace_bytes(None, 1) == 0


def test_observes_are_normalised_from_both_forms():
    as_list = [{'obs0': 8.0, 'obs1': 9.0}, {'obs0': 7.5, 'obs1': torch.tensor(6.0)}, {'obs0': 1, 'obs1': 2}]
    names, dicts, cols = Model._normalise_observes(as_list)
    assert names == ['obs0', 'obs1'] and len(dicts) == 3 and dicts[1] is as_list[1]
    assert cols['obs0'].dtype == np.float32 and cols['obs0'].shape == (3, 1)
    np.testing.assert_array_equal(cols['obs1'][:, 0], [9.0, 6.0, 2.0])
    as_dict = {'obs0': torch.tensor([8.0, 7.5, 1.0]), 'obs1': np.array([9.0, 6.0, 2.0])}
    names2, dicts2, cols2 = Model._normalise_observes(as_dict)
    assert names2 == names and len(dicts2) == 3
    for k in names:
        np.testing.assert_array_equal(cols2[k], cols[k])
        assert [float(d[k]) for d in dicts2] == [float(d[k]) for d in as_list]
    # a leading dimension M in front of a vector observable: [M, k]
    _, dicts3, cols3 = Model._normalise_observes({'img': torch.arange(12.0).reshape(2, 2, 3)})
    assert cols3['img'].shape == (2, 6) and tuple(dicts3[1]['img'].shape) == (2, 3)


@pytest.mark.parametrize('bad', [[], {}, {'obs0': torch.zeros(0)}, [{'obs0': 1.0, 'obs1': 2.0}, {'obs0': 1.0}],
                                 [{'obs0': 1.0}, {'obs1': 1.0}], {'obs0': torch.zeros(2), 'obs1': torch.zeros(3)},
                                 {'obs0': 1.0}],
                         ids=['empty list', 'empty dict', 'M = 0', 'missing key', 'other key', 'unequal M', 'no leading dimension'])
def test_bad_observes_are_rejected(bad):
    model, net, meta, params = lockstep_network()
    with pytest.raises(ValueError):
        model.posterior_results_batch(8, bad)


def test_two_statement_program_takes_the_loop_with_group_offsets(monkeypatch):
    """Marsaglia's program samples twice per iteration and branches: not the fast path. The batched call is the loop of single
    calls - recorded here - with offset + g * num_traces, and returns what those calls return."""
    model, net, meta, params = lockstep_network()
    observes = [{'obs0': 8.0, 'obs1': 9.0}, {'obs0': 7.0, 'obs1': 7.5}, {'obs0': 9.5, 'obs1': 8.5}]
    calls = []
    single = model.posterior_results

    def recorded(num_traces, *args, **kwargs):
        calls.append((num_traces, dict(kwargs)))
        return single(num_traces, *args, **kwargs)
    monkeypatch.setattr(model, 'posterior_results', recorded)
    n, seed, offset = 24, 11, 1000
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(n, observes, seed=seed, offset=offset, lock_step=True)
    assert model._batch_ok is False
    assert len(posts) == 3 and len(calls) == 3
    for g, (num, kw) in enumerate(calls):
        assert num == n and kw['observe'] is observes[g] and kw['seed'] == seed and kw['offset'] == offset + g * n
        assert kw['lock_step'] is True and kw['inference_engine'] == IC
    monkeypatch.undo()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for g, post in enumerate(posts):
            ref = model.posterior_results(n, IC, observe=observes[g], lock_step=True, seed=seed, offset=offset + g * n)
            assert post.length == ref.length
            np.testing.assert_array_equal(post._all_values.numpy(), ref._all_values.numpy())
            np.testing.assert_array_equal(post._all_log_weights.numpy(), ref._all_log_weights.numpy())
    # the decision is remembered: the second call goes straight to the loop, also in the tensor form of `observes`
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        again = model.posterior_results_batch(n, {'obs0': torch.tensor([8.0, 7.0]), 'obs1': torch.tensor([9.0, 7.5])}, seed=seed,
                                              offset=offset, lock_step=True)
    assert len(again) == 2
    np.testing.assert_array_equal(again[1]._all_values.numpy(), posts[1]._all_values.numpy())
