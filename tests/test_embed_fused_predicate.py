"""obs_fused_supported (csrc/obs_embed.hip), the one predicate of the fused observe-embedding route, seen through
pp_is_first_statement_supported - a host function: it holds exactly where the shapes lie inside the kernels' bounds AND the LDS
weight image fits (tests/embed_cases.py image_words restates the image's size). An embedding inside the bounds whose image
does not fit - one scalar observable of dim 64 - takes the generic path instead of failing in the launch. CPU only."""
import ctypes as C

import pytest

import embed_cases as EC
from pyprob_amd import lib as L
from pyprob_amd.spec import NetSpec


def _supported(emb, lstm_dim=64):
    spec = NetSpec(EC.obs_of(emb), lstm_dim=lstm_dim)
    spec.add_address('mu', 'Normal')
    net = spec.c_struct(1)       # (a non-null address table: the predicate only asks whether there is one)
    return L.load().pp_is_first_statement_supported(C.byref(net), 0)


@pytest.mark.parametrize('name', list(EC.CASES))
def test_predicate_is_the_shape_bounds_and_the_image_fit(name, monkeypatch):
    monkeypatch.delenv('PP_IS_FIRST', raising=False)
    emb = EC.CASES[name]
    assert _supported(emb) == int(EC.inside_envelope(emb) and EC.image_words(emb) <= 10240) == int(name in EC.FIT)


def test_the_image_limit_between_the_nearest_shapes():
    """Two observables (dim, 8) + (dim', 1) with e_obs = 64 around the limit: the largest image of at most 10 240 words is taken, the smallest above is not."""
    found = {}
    for d in range(8, 57):
        for w in range(1, 9):
            emb = ((d, w), (64 - d, 1))
            if EC.inside_envelope(emb):
                found.setdefault(EC.image_words(emb), emb)
    below = max(n for n in found if n <= 10240)
    above = min(n for n in found if n > 10240)
    assert below > 10240 - 64 and above <= 10240 + 64, (below, above)      # the grid does reach the limit's neighbourhood
    assert _supported(found[below]) == 1 and _supported(found[above]) == 0, (below, found[below], above, found[above])
