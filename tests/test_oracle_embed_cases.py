"""The cases of tests/test_gpu_embed_envelope.py (tests/embed_cases.py), built with the oracle alone: each finds its B traces away
from the ReLU kinks among B + 64 candidates, its batch has the shape the case is there for, and the three groups of embeddings
lie where their names say - inside the fused envelope with an image that fits, inside it with an image that does not, and just
outside. CPU only."""
import numpy as np
import pytest

import embed_cases as EC
from helpers import packed


def test_the_groups_lie_where_they_should():
    for name, emb in EC.FIT.items():
        assert EC.inside_envelope(emb) and EC.image_words(emb) <= 10240, (name, EC.image_words(emb))
    for name, emb in EC.OVERFLOW.items():
        assert EC.inside_envelope(emb) and EC.image_words(emb) > 10240, (name, EC.image_words(emb))
    for name, emb in EC.OUTSIDE.items():
        assert not EC.inside_envelope(emb), name
    assert EC.image_words(EC.OVERFLOW['scalar_e64']) == 10721 and EC.image_words(EC.OVERFLOW['two_vec8_e64']) == 10257
    assert EC.image_words(EC.FIT['wide_8_3']) == 10240 - 194
    # the template instantiations NOBS = 1, 2, 4 (one slot empty), 8 (three empty) and 8 (full)
    assert sorted({len(emb) for emb in EC.FIT.values()}) == [1, 2, 3, 5, 8]
    assert EC.width_of(EC.FIT['eight_vec8']) == 64 and sum(d for d, _ in EC.FIT['eight_vec8']) == 64


def test_observations_have_the_networks_width_and_are_not_the_models_columns():
    arrays, _, _ = EC.candidates('single', 50, 11)
    assert arrays['obs'].shape == (50, 11) and arrays['obs'].dtype == np.float32
    assert len(np.unique(arrays['obs'])) == arrays['obs'].size      # no column repeats another


def _reaches(kind, B, arrays, pb):
    assert len(arrays['trace_len']) == B and int(arrays['trace_len'].max()) == pb.t_max
    if kind == 'ragged':
        assert pb.t_max >= 4 and pb.n_active[-1] <= 8      # a recurrence; few traces in the late time steps
        assert np.isin(1.25, arrays['values'])             # rescued rows
    elif kind == 'len2':
        assert (arrays['trace_len'] == 2).all()
    else:
        assert pb.t_max == 1


@pytest.mark.parametrize('label', list(EC.all_builds()))
def test_kink_filter_keeps_enough_traces(label):
    """Every case finds its B traces among B + 64 candidates (the filter asserts it), on the host copy of the engine's buffers:
    the initial weights are the same on either device."""
    name, kind, H, B, network = EC.all_builds()[label]
    eng, arrays, addresses, dists = EC.build(name, kind, H, B, network=network, device='cpu')
    assert arrays['obs'].shape == (B, EC.width_of(EC.CASES[name])) and eng.spec.e_obs == sum(d for d, _ in EC.CASES[name])
    assert [(o[3], o[1]) for o in eng.spec.obs] == list(EC.CASES[name])
    _reaches(kind, B, arrays, packed(arrays, eng.spec))


def test_kink_filter_keeps_enough_traces_in_the_sequence():
    name, batches = EC.SEQUENCE
    eng = EC.engine(name, 'ragged', 64, device='cpu')
    for k, (kind, B) in enumerate(batches):
        arrays = EC.batch(eng, kind, B, seed=10 * k)[0]
        assert len(arrays['trace_len']) == B and (int(arrays['trace_len'].max()) == 1) == (kind == 'single_a0')
