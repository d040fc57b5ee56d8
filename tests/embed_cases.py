"""The cases of tests/test_gpu_embed_envelope.py: the fused observe-embedding kernels (csrc/obs_embed.hip) over the envelope that
obs_fused_supported accepts - 1..8 observables, e_obs <= 64, input width 1..8 and hidden width 1..32 per observable, hidden
widths summing to at most 64, a weight image of at most 10 239 words - and the embeddings next to its edges, which take the
generic path. Shared between the GPU tests and the CPU check that the ReLU-kink filter leaves enough traces
(tests/test_oracle_embed_cases.py), so that both build the same network and the same batch.

Observables are (dim, input width), all of depth 2; the hidden width of one is (width + dim) // 2 (pyprob_amd/spec.py). Every
case uses trained-looking weights and B traces out of B + 64 candidates away from the ReLU kinks, as tests/depth_cases.py."""
import numpy as np

import depth_cases as D
from helpers import away_from_relu_kinks, fresh_engine, synthetic_gumm_arrays, trained_looking

# inside the envelope, the image fits
FIT = {
    'one_e32': ((32, 1),),                         # NOBS = 1
    'three': ((16, 1), (16, 1), (32, 1)),          # NOBS = 4, one slot empty; e_obs = 64
    'five_e60': ((12, 1),) * 5,                    # NOBS = 8, three slots empty
    'eight_e64': ((8, 1),) * 8,                    # NOBS = 8, full
    'eight_vec8': ((8, 8),) * 8,                   # hidden widths sum to 64, e_obs = 64, 64 observation columns: every lane loads one
    'wide_8_3': ((32, 8), (32, 3)),                # hid = 20 and 17 (leading dimension 20); 194 words under the image limit
    'odd_e30': ((20, 1), (10, 1)),                 # e_obs = 30 (leading dimension 32), hid = 10 and 5: padding in every leading dimension
    'tiny_e3': ((2, 1), (1, 1)),
}
# inside every width bound, but the image (sum_o [hid (in + 2) + out (hid + 2)] + 2 e (e + 2) words, + 1) is over 10 240
OVERFLOW = {
    'scalar_e64': ((64, 1),),                      # 10 721
    'two_vec8_e64': ((32, 8), (32, 8)),            # 10 257
    'e56_e8': ((56, 1), (8, 1)),                   # 10 273
}
# just outside: the generic path
OUTSIDE = {
    'hid33': ((64, 2),),                           # hidden width 33
    'in9': ((32, 9),),                             # input width 9
    'e68': ((36, 1), (32, 1)),                     # e_obs = 68
}
CASES = dict(FIT, **OVERFLOW, **OUTSIDE)

B_STEP = 130                                      # more than one workgroup of four waves; n_split > 1 on a single-statement batch
LEN2 = ('three', 'odd_e30', 'eight_vec8')         # every trace of length 2: the t >= 1 branch of obs_build_rows
TWO_PER_WAVE = ('odd_e30', 'eight_vec8')          # B = 1030 single statements: two traces per wave, the last wave partial
B_TWO_PER_WAVE = 1030
H512 = ('three', 'eight_e64', 'scalar_e64')       # e_obs = 64 at H = 512, B = 40: the panel predicates are consulted
B_H512 = 40
FEEDFORWARD = ('odd_e30', 'five_e60')
SEQUENCE = ('wide_8_3', (('ragged', 300), ('single_a0', 17), ('ragged', 40)))   # one engine, one workspace


def all_builds():
    """{label: (case, kind, H, B, network)} of every engine + batch that the tests build."""
    builds = {}
    for name in CASES:
        for kind in ('single', 'ragged'):
            builds['step_%s_%s' % (name, kind)] = (name, kind, 64, B_STEP, 'lstm')
    for name in LEN2:
        builds['len2_' + name] = (name, 'len2', 64, B_STEP, 'lstm')
    for name in TWO_PER_WAVE:
        builds['two_per_wave_' + name] = (name, 'single', 64, B_TWO_PER_WAVE, 'lstm')
    for name in H512:
        builds['h512_' + name] = (name, 'single', 512, B_H512, 'lstm')
    for name in FEEDFORWARD:
        for kind in ('single', 'ragged'):
            builds['ff_%s_%s' % (name, kind)] = (name, kind, 64, B_STEP, 'feedforward')
    return builds


def obs_of(emb):
    return {'obs%d' % i: {'dim': d, 'input_dim': w} for i, (d, w) in enumerate(emb)}


def width_of(emb):
    return sum(w for _, w in emb)


def image_words(emb):
    """Words of the fused kernels' LDS weight image (obs_embed.hip obs_fused_args: rows of stride cols + 1, then the bias), the
    spare word behind it included; it fits if this is at most 10 240."""
    e = sum(d for d, _ in emb)
    return sum(((w + d) // 2) * (w + 2) + d * ((w + d) // 2 + 2) for d, w in emb) + 2 * e * (e + 2) + 1


def inside_envelope(emb):
    """The width bounds of obs_fused_supported (without the image size)."""
    hid = [(w + d) // 2 for d, w in emb]
    return len(emb) <= 8 and sum(d for d, _ in emb) <= 64 and max(w for _, w in emb) <= 8 and 1 <= min(hid) and max(hid) <= 32 and \
        sum(hid) <= 64


def observations(model_obs, width, seed):
    """[n, width] observations around the model's own: even columns m + sqrt(2) noise, m the mean of a trace's two model
    observations (about its mu); odd columns 3 + 2 noise."""
    rng = np.random.default_rng(1000 + seed)
    n = len(model_obs)
    noise = rng.standard_normal((n, width))
    obs = 3.0 + 2.0 * noise
    obs[:, ::2] = model_obs.mean(1, keepdims=True) + np.sqrt(2.0) * noise[:, ::2]
    return np.ascontiguousarray(obs, np.float32)


def candidates(kind, n, width, seed=0):
    """(arrays of n candidate traces, addresses, distribution names): the kinds of depth_cases.candidates, and 'len2' - the
    Marsaglia program cut after one iteration, every trace of length 2."""
    if kind == 'len2':
        arrays, addresses = synthetic_gumm_arrays(n, seed=21 + seed, max_iter=1)
        dists = ['Uniform'] * len(addresses)
    else:
        arrays, addresses, dists = D.candidates(kind, n, seed=seed)
    arrays['obs'] = observations(arrays['obs'], width, seed)
    return arrays, addresses, dists


def engine(name, kind, H, network='lstm', device='cuda:0'):
    emb = CASES[name]
    _, addresses, _ = candidates(kind, 1, width_of(emb))
    eng = fresh_engine(H, addresses, 'Normal' if kind == 'single' else 'Uniform', network=network, obs=obs_of(emb), device=device)
    return trained_looking(eng, seed=H + len(emb))


def batch(eng, kind, B, seed=0):
    """B traces of B + 64 candidates, away from the ReLU kinks of the proposal layers and of every embedding layer."""
    arrays, addresses, dists = candidates(kind, B + 64, eng.spec.obs_width, seed=seed)
    return away_from_relu_kinks(eng, arrays, addresses, dists, B, embedding=True), addresses, dists


def build(name, kind, H, B, network='lstm', device='cuda:0'):
    eng = engine(name, kind, H, network, device)
    return (eng,) + batch(eng, kind, B)
