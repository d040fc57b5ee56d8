"""Lock-step prior traces of programs with vector-valued observes (state.PriorLockStep records of [n, k]): images for the
CNN2D5C embedding, k-vectors for FEEDFORWARD, through Model.prior_traces_packed, VectorisedOnlineDataset, save_dataset and
learn_inference_network's chunk sizing. CPU only (the device draws: tests/test_gpu_obs_draw.py)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle_ops  # noqa: F401  the stock CPU doubles of the operators
import obs_draw_ref
import pyprob_amd as pyprob
from pyprob_amd import Model
from pyprob_amd.distributions import Categorical, Normal

obs_draw_ref.register_cpu_double()

PAT = torch.rand(6, 4, 4, generator=torch.Generator().manual_seed(11))
N = 64
Z_MEAN_BAR = 6 / np.sqrt(1024.)                 # six standard errors of the mean of 64 * 16 unit normals
Z_VAR_BAR = 6 * np.sqrt(2 / 1024.)              # ... and of their variance


class TwoPath(Model):
    """d ~ Categorical(6), gain ~ Normal(1, 0.1); for d >= 3 a second gain; the image is the d-th pattern times the gains plus
    pixel noise; y is the first gain plus noise."""

    def forward(self):
        d = pyprob.sample(Categorical([1 / 6.] * 6))
        g = pyprob.sample(Normal(1.0, 0.1))
        mean = PAT.to(d.device)[d.long()] * g.reshape(-1, 1, 1)
        if d >= 3:
            g2 = pyprob.sample(Normal(1.0, 0.1))
            mean = mean * g2.reshape(-1, 1, 1)
        pyprob.observe(Normal(mean, 0.1), name='img')
        pyprob.observe(Normal(g, 0.1), name='y')
        return d


def recover(cols):
    """Per trace: (d, product of the gains, image [16], y, trace length) from the ragged columns."""
    lens, table, ids, vals, prior, obs = cols[:6]
    off = np.concatenate([[0], np.cumsum(lens)])
    d = vals[off[:-1]].astype(np.int64)
    gain = np.asarray([np.prod(vals[off[t] + 1:off[t + 1]].astype(np.float64)) for t in range(len(lens))])
    return d, gain, obs[:, :16].astype(np.float64), obs[:, 16], lens


def check_two_path(cols, widths):
    """Shape, grouping by path, and the moments of the standardised pixel noise (shared with the device test)."""
    lens, table, ids, vals, prior, obs = cols[:6]
    assert obs.shape == (N, 17) and list(widths) == [16, 1]
    d, gain, img, y, lens = recover(cols)
    assert set(np.unique(d)) <= set(range(6)) and (d >= 3).any() and (d < 3).any()
    np.testing.assert_array_equal(lens, np.where(d >= 3, 3, 2))             # a path's statement count
    assert np.count_nonzero(np.diff(lens)) == 1                             # traces are grouped by path
    z = (img - PAT.double().numpy()[d].reshape(N, 16) * gain[:, None]) / 0.1
    print('two-path z: mean %.4f var %.4f' % (z.mean(), z.var()))
    assert abs(z.mean()) <= Z_MEAN_BAR and abs(z.var() - 1) <= Z_VAR_BAR
    first_gain = vals[np.concatenate([[0], np.cumsum(lens)])[:-1] + 1]
    assert np.abs(y - first_gain).max() < 0.1 * 6                            # y belongs to its own trace


def test_two_path_program_shape_and_values():
    torch.manual_seed(0)
    model = TwoPath('two paths')
    cols = model.prior_traces_packed(N, ['img', 'y'])
    check_two_path(cols, model._last_prior_obs_widths)


def test_shared_plain_tensor_mean_draws_one_row_per_particle():
    class Shared(Model):
        def forward(self):
            g = pyprob.sample(Normal(1.0, 0.1))
            pyprob.observe(Normal(PAT[0], 0.1), name='img')

    torch.manual_seed(1)
    obs = Shared('shared').prior_traces_packed(N, ['img'])[5]
    assert obs.shape == (N, 16)
    z = (obs.astype(np.float64) - PAT[0].double().numpy().reshape(1, 16)) / 0.1
    assert abs(z.mean()) <= Z_MEAN_BAR and abs(z.var() - 1) <= Z_VAR_BAR
    assert len({tuple(r) for r in obs.tolist()}) == N                        # rows pairwise different


def test_fixed_value_is_one_shared_row():
    fixed = torch.arange(16.).reshape(4, 4)

    class Fixed(Model):
        def forward(self):
            g = pyprob.sample(Normal(1.0, 0.1))
            pyprob.observe(Normal(PAT[0] * g.reshape(-1, 1, 1), 0.1), value=fixed, name='img')

    model = Fixed('fixed')
    obs = model.prior_traces_packed(8, ['img'])[5]
    assert model._last_prior_obs_widths == [16]
    np.testing.assert_array_equal(obs, np.tile(np.arange(16, dtype=np.float32), (8, 1)))


def test_plain_tensor_with_leading_width_is_shared():
    mean = torch.rand(8, 4)

    class Plain(Model):
        def forward(self):
            g = pyprob.sample(Normal(1.0, 0.1))
            pyprob.observe(Normal(mean, 0.1), name='v')

    model = Plain('plain')
    for n in (8, 16):
        obs = model.prior_traces_packed(n, ['v'])[5]
        assert obs.shape == (n, 32) and model._last_prior_obs_widths == [32]
    # ... but next to a per-particle parameter the two readings differ: refused
    class Both(Model):
        def forward(self):
            g = pyprob.sample(Normal(1.0, 0.1))
            pyprob.observe(Normal(mean, (g * g + 0.1).reshape(-1, 1)), name='v')

    with pytest.raises(RuntimeError, match="'v'"):
        Both('both').prior_traces_packed(8, ['v'])


def test_mismatched_event_shapes_raise():
    class Bad(Model):
        def forward(self):
            g = pyprob.sample(Normal(1.0, 0.1))
            pyprob.observe(Normal(PAT[0] * g.reshape(-1, 1, 1), torch.full((3,), 0.1)), name='img')

    with pytest.raises(RuntimeError, match="'img'"):
        Bad('bad').prior_traces_packed(8, ['img'])


def test_a_name_with_two_widths_raises():
    class Widths(Model):
        def forward(self):
            g = pyprob.sample(Normal(0.0, 1.0))
            if g >= 0:
                pyprob.observe(Normal(PAT[0] * g.reshape(-1, 1, 1), 0.1), name='img')
            else:
                pyprob.observe(Normal(PAT[0, 0] * g.reshape(-1, 1), 0.1), name='img')

    torch.manual_seed(2)
    with pytest.raises(RuntimeError, match="'img'"):
        Widths('widths').prior_traces_packed(32, ['img'])


def test_feedforward_vector_observable_through_the_online_dataset():
    from pyprob_amd.dataset import VectorisedOnlineDataset
    from pyprob_amd.spec import NetSpec
    torch.manual_seed(3)
    ds = VectorisedOnlineDataset(TwoPath('ff'), ['img', 'y'], chunk_traces=N)
    assert ds.obs_widths == [16, 1] and ds.obs_width == 17
    spec = NetSpec({'img': {'dim': 8, 'input_dim': 16}, 'y': {'dim': 4}}, lstm_dim=16)
    for a, dname, nc in ds.addresses:
        spec.add_address(a, dname, nc)
    ids = ds.sorted_indices()[:8]
    pb = ds.batch(ids, spec)
    lens, addr, value, prior, obs = ds.gather(ids)
    assert obs.shape == (8, 17)
    np.testing.assert_array_equal(np.asarray(pb.obs).reshape(8, 17), obs)    # the image floats, then y, per row
    off = np.concatenate([[0], np.cumsum(lens)])
    d = value[off[:-1]].astype(np.int64)
    gain = np.asarray([np.prod(value[off[t] + 1:off[t + 1]].astype(np.float64)) for t in range(8)])
    assert np.abs(obs[:, :16] - PAT.numpy()[d].reshape(8, 16) * gain[:, None]).max() < 0.1 * 6
    assert np.abs(obs[:, 16] - value[off[:-1] + 1]).max() < 0.1 * 6
    before = ds.gather(ds.sorted_indices()[:8])[4].copy()
    ds.refresh()
    assert ds.obs_widths == [16, 1] and not np.array_equal(ds.gather(ds.sorted_indices()[:8])[4], before)


def test_save_dataset_writes_the_true_widths(tmp_path, monkeypatch):
    from pyprob_amd.dataset import PackedTraceDataset, PackedTraceWriter

    def no_per_trace_route(self, trace):
        raise AssertionError('save_dataset took the per-trace branch')
    monkeypatch.setattr(PackedTraceWriter, 'add_trace', no_per_trace_route)
    torch.manual_seed(4)
    shards = TwoPath('shards').save_dataset(str(tmp_path / 'd'), 96, 64, obs_names=['img', 'y'])
    assert shards == 2
    metas = [json.load(open(os.path.join(tmp_path, 'd', s, 'meta.json'))) for s in sorted(os.listdir(tmp_path / 'd'))]
    assert [m['n_traces'] for m in metas] == [64, 32] and all(m['obs_widths'] == [16, 1] for m in metas)
    ds = PackedTraceDataset(str(tmp_path / 'd'))
    assert len(ds) == 96 and ds.obs_widths == [16, 1]
    lens, addr, value, prior, obs = ds.gather(np.arange(96))
    stored = np.concatenate([np.load(os.path.join(tmp_path, 'd', s, 'obs.npy')) for s in sorted(os.listdir(tmp_path / 'd'))])
    np.testing.assert_array_equal(obs, stored)
    off = np.concatenate([[0], np.cumsum(lens)])
    d = value[off[:-1]].astype(np.int64)
    gain = np.asarray([np.prod(value[off[t] + 1:off[t + 1]].astype(np.float64)) for t in range(96)])
    assert np.abs(obs[:, :16] - PAT.numpy()[d].reshape(96, 16) * gain[:, None]).max() < 0.1 * 6


class _Stop(Exception):
    pass


def _chunk_learn_builds(model, monkeypatch, **kw):
    from pyprob_amd import dataset as D
    seen = {}

    def init(self, model, obs_names, chunk_traces=65536, device='cpu', prior_inflation=None):
        seen['chunk'] = chunk_traces
        raise _Stop()
    monkeypatch.setattr(D.VectorisedOnlineDataset, '__init__', init)
    with pytest.raises(_Stop):
        model.learn_inference_network(num_traces=64, batch_size=8, vectorised_prior=True, device='cpu', **kw)
    return seen['chunk']


def test_chunk_is_capped_by_bytes(monkeypatch):
    monkeypatch.setenv('PP_PRIOR_CHUNK_BYTES', '65536')
    chunk = _chunk_learn_builds(TwoPath('cap'), monkeypatch, observe_embeddings={'img': {'dim': 8, 'input_dim': 16}, 'y': {'dim': 4}})
    assert chunk % 8 == 0 and chunk >= 8 and chunk * 17 * 4 <= 65536
    assert chunk == (65536 // 68) // 8 * 8
    # an explicit chunk is honoured as given
    assert _chunk_learn_builds(TwoPath('cap'), monkeypatch, prior_chunk_traces=4000,
                               observe_embeddings={'img': {'dim': 8, 'input_dim': 16}, 'y': {'dim': 4}}) == 4000


def test_scalar_programs_keep_their_chunk(monkeypatch):
    from models import GaussianWithUnknownMean
    chunk = _chunk_learn_builds(GaussianWithUnknownMean(), monkeypatch, observe_embeddings={'obs0': {'dim': 8}, 'obs1': {'dim': 8}})
    assert chunk == max(64 * 8, 16384)


def test_exports_and_abi_version():
    from pyprob_amd import lib as L
    lib = L.load()
    assert 'pp_obs_draw' in L.PROTOTYPES and hasattr(lib, 'pp_obs_draw')
    assert lib.pp_abi_version() == 15 == L.PP_ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'pyprob_amd.h')).read()
    assert 'int pp_obs_draw(' in header


def test_scalar_chunks_are_unchanged_and_draw_no_rows():
    from models import GaussianWithUnknownMean
    model = GaussianWithUnknownMean()
    calls = obs_draw_ref.calls[0]
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        runs.append(model.prior_traces_packed(256, ['obs0', 'obs1']))
    for a, b in zip(runs[0], runs[1]):
        if isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a, b)
        else:
            assert a == b
    assert runs[0][5].shape == (256, 2) and model._last_prior_obs_widths == [1, 1]
    assert obs_draw_ref.calls[0] == calls


def test_philox_known_answer():
    """Random123's known-answer vectors of Philox4x32-10: the numpy restatement the device tests compare against."""
    w = obs_draw_ref.philox4x32_10(0, 0, 0, 0, 0)
    assert [int(x) for x in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    w = obs_draw_ref.philox4x32_10(0xffffffffffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)
    assert [int(x) for x in w] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
