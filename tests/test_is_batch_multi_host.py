"""Batched posteriors of multi-statement programs on the host: the two C-ABI entry points of the later statements
(pp_is_batch_bias, pp_is_statement_groups) are declared, prototyped and exported and reject bad arguments before they touch a
device; the batch workspace grows with M; on the CPU device (the oracle-backed stand-ins of tests/oracle_ops.py) a two-statement
straight-line program through Model.posterior_results_batch is the loop of posterior_results calls, bit for bit - the fast path
is the GPU's (tests/test_gpu_is_batch_multi.py)."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

import oracle_ops  # noqa: F401  registers the CPU kernels of pyprob_hip::*
from helpers import is_engine
from pyprob_amd import lib as L
from pyprob_amd.state import InferenceEngine

torch = pytest.importorskip('torch')

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IC = InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK
SYMBOLS = ('pp_is_batch_bias', 'pp_is_statement_groups')


def test_entry_points_are_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, 'include', 'pyprob_amd.h')).read()
    declared = set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', hdr))
    lib = L.load()
    for name in SYMBOLS:
        assert name in declared and name in L.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert len(L.PROTOTYPES['pp_is_batch_bias'][1]) == 12 and len(L.PROTOTYPES['pp_is_statement_groups'][1]) == 23
    # the header's parameter lists have as many entries as the prototypes
    for name in SYMBOLS:
        decl = hdr[hdr.index('int %s(' % name):]
        decl = re.sub(r'/\*.*?\*/', '', decl[:decl.index(';')], flags=re.S)
        assert decl.count(',') + 1 == len(L.PROTOTYPES[name][1]), name
    assert lib.pp_abi_version() == L.PP_ABI_VERSION == 15
    # the entries cite the reference lines they replace
    block = hdr[hdr.index('Later statements of a batched posterior call'):hdr.index('int pp_is_batch_bias')]
    for ref in ('pyprob/nn/inference_network_lstm.py', 'pyprob/state.py', 'pyprob/distributions/mixture.py', 'pyprob/model.py'):
        assert ref in block, ref


def test_workspace_bytes_are_monotone_in_the_number_of_groups():
    lib = L.load()
    for H in (64, 512, 1024):
        eng, run, sd = is_engine(H, device='cpu')
        sizes = [lib.pp_is_batch_workspace_bytes(C.byref(eng.net), m) for m in (1, 2, 7, 64, 257, 4096)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (H, sizes)


def test_bad_arguments_are_rejected_without_a_device():
    """Every rejected call returns before its first launch: the pointers below are host addresses no kernel may see."""
    lib = L.load()
    eng, run, sd = is_engine(64, device='cpu')
    net, P = C.byref(eng.net), eng.params.data_ptr()
    H, M, N = 64, 3, 5
    buf = torch.zeros(M * N * 4 * H)
    p = buf.data_ptr()
    ws_bytes = lib.pp_is_batch_workspace_bytes(net, M)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8)
    a, prev, cat = (eng.spec.address_id[k] for k in ('a_normal', 'a_uniform', 'a_cat'))

    def groups(addr=a, prev_addr=prev, m=M, n_per=N, bias=p, prior_kind=0, prior_stride=0):
        return lib.pp_is_statement_groups(net, P, addr, prev_addr, m, n_per, bias, p, p, p, prior_stride, p, p, p, p, prior_kind, 1, 0,
                                          None, 0, ws.data_ptr(), ws_bytes, None)

    def bias(addr=a, prev_addr=prev, m=M, out=p, ws_groups=M, first=0):
        return lib.pp_is_batch_bias(net, P, addr, prev_addr, m, ws_groups, first, None, out, ws.data_ptr(), ws_bytes, None)
    assert groups(n_per=0) != 0 and groups(n_per=-3) != 0
    assert groups(bias=None) != 0 and bias(out=None) != 0
    assert groups(prev_addr=-1) != 0 and bias(prev_addr=-1) != 0
    assert groups(addr=cat) != 0 and bias(addr=cat) != 0                      # not a mixture head
    assert groups(addr=eng.spec.address_id['a_poisson']) != 0                 # a mixture head without a Normal / Uniform prior
    assert groups(addr=len(eng.spec.addresses)) != 0 and bias(addr=-1) != 0   # address ids out of range
    assert bias(first=1) != 0 and bias(first=-1) != 0 and bias(ws_groups=M - 1) != 0      # a window outside the embedded rows
    assert groups(prior_kind=2) != 0 and groups(prior_stride=2) != 0 and groups(m=-1) != 0 and bias(m=-1) != 0
    assert 'pp_is_' in lib.pp_last_error().decode()
    # no fused statement kernel for the network: H = 1024, two layers
    for Hn, depth in ((1024, 1), (64, 2)):
        e2, r2, _ = is_engine(Hn, depth=depth, device='cpu')
        wb = lib.pp_is_batch_workspace_bytes(C.byref(e2.net), M)
        w2 = torch.zeros(max(wb, 8), dtype=torch.uint8)
        rc = lib.pp_is_statement_groups(C.byref(e2.net), e2.params.data_ptr(), e2.spec.address_id['a_normal'],
                                        e2.spec.address_id['a_uniform'], M, N, p, p, p, p, 0, p, p, p, p, 0, 1, 0, None, 0,
                                        w2.data_ptr(), wb, None)
        assert rc != 0, (Hn, depth)
    assert float(buf.abs().sum()) == 0.0


def test_two_statement_program_on_the_cpu_device_equals_the_loop():
    import pyprob_amd as pyprob
    from pyprob_amd import Model
    from pyprob_amd.distributions import Normal
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.nn import InferenceNetworkLSTM
    from pyprob_amd.spec import NetSpec
    from pyprob_amd.state import TraceMode

    class TwoStatements(Model):
        def forward(self):
            a = pyprob.sample(Normal(1.0, math.sqrt(5.0)), address='a')
            pyprob.observe(Normal(a, math.sqrt(2.0)), name='obs0')
            b = pyprob.sample(Normal(a, 0.7), address='b')
            pyprob.observe(Normal(b, math.sqrt(2.0)), name='obs1')
            return b
    model = TwoStatements()
    tr = next(model._trace_generator(trace_mode=TraceMode.PRIOR))
    emb = {'obs0': {'dim': 32}, 'obs1': {'dim': 32}}
    eng = oracle_ops.CpuBufferEngine(NetSpec(emb, lstm_dim=64, proposal_mixture_components=10), seed=1)
    eng.add_addresses([(v.address, v.distribution.name, None) for v in tr.variables_controlled])
    net = InferenceNetworkLSTM(observe_embeddings=emb, lstm_dim=64, device='cpu')
    net._obs_names = list(emb)
    net._engine = eng
    net._is = ISRunner(eng)
    net._layers_initialized = True
    model._inference_network = net
    observes = [{'obs0': 2.0, 'obs1': 1.5}, {'obs0': -0.5, 'obs1': 0.25}, {'obs0': 3.5, 'obs1': 3.0}]
    n, seed, offset = 16, 7, 100
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        posts = model.posterior_results_batch(n, observes, seed=seed, offset=offset, lock_step=True)
        assert model._batch_ok is False and len(posts) == 3
        for g, post in enumerate(posts):
            ref = model.posterior_results(n, IC, observe=observes[g], lock_step=True, seed=seed, offset=offset + g * n)
            assert post.length == ref.length == n
            np.testing.assert_array_equal(post._all_values.numpy(), ref._all_values.numpy())
            np.testing.assert_array_equal(post._all_log_weights.numpy(), ref._all_log_weights.numpy())
