"""The cases of tests/test_gpu_dims.py and of the off-grid cases of tests/test_gpu_is_step_fused.py: the training step and the
importance-sampling statement at network dimensions off the grid the rest of the suite builds its networks on (lstm_dim in
{32, 64, 128, 256, 512, 1024, 1536}, sample / address / distribution-type embeddings of 4 / 64 / 8). Every fused route of the
engine stands behind a predicate on these dimensions; `routes` restates those predicates, so that each case is known to lie in
the class its name says (tests/test_oracle_dim_cases.py asserts it flag by flag). Shared between the GPU tests and that CPU
check, so that both build the same network and the same batch; imports no device code.

A case is (lstm_dim, lstm_depth, smp_dim, addr_dim, dtype_dim, obs), obs as embed_cases.obs_of reads it - ((dim, input width),
...) - or None for helpers.DEFAULT_OBS. Weights are trained-looking (helpers.trained_looking), batches B traces of B + 64
candidates away from the ReLU kinks (depth_cases.batch), as in tests/depth_cases.py and tests/embed_cases.py."""
import depth_cases as D
import embed_cases as EC
from helpers import DEFAULT_OBS, fresh_engine, trained_looking

OBS_DEFAULT = ((32, 1), (32, 1))
assert EC.obs_of(OBS_DEFAULT) == {k: dict(v, input_dim=1) for k, v in DEFAULT_OBS.items()}


def case(H, depth=1, smp=4, addr=64, dtype=8, obs=None):
    return (H, depth, smp, addr, dtype, obs)


# hidden sizes at the default embedding dims (e_obs 64, lstm_in 212, c2 = e_obs + smp_dim = 68, ne = addr_dim + dtype_dim = 72)
HIDDEN = {
    'h96': case(96),               # % 32, not % 64: compact rows and the cell epilogues, no lean cell, no fast input launch
    'h48': case(48),               # % 16, not % 32
    'h100': case(100),             # % 4, not % 16: full-width rows, no cell epilogue in the recurrent product; dh as partials
    'h50': case(50),               # even, not % 4: dh by atomics, every ld = H operand on the scalar stagers; head hidden width 40
    'h33': case(33),               # odd; head hidden width 31
    'h384': case(384),             # % 64, but neither a tail width nor a panel width: the per-step recurrence at a large H
    'h100_d2': case(100, 2),
    'h50_d3': case(50, 3),
}
HIDDEN_RAGGED_ONLY = ('h100_d2', 'h50_d3')
# embedding dims at H = 64
EMBED = {
    'smp1': case(64, smp=1),                      # c2 = 65: full-width rows; the IS slab holds one column
    'smp8': case(64, smp=8),                      # compact rows; the IS slab exactly full
    'smp9': case(64, smp=9),                      # c2 = 73, lstm_in = 217; over the fused IS statements' slab
    'addr10': case(64, addr=10),                  # ne = 18, lstm_in = 104
    'addr128': case(64, addr=128),                # ne = 136 > 128, lstm_in = 340 > 256
    'dtype7': case(64, dtype=7),                  # ne = 71 odd, lstm_in = 210
    'ne2': case(64, addr=1, dtype=1),             # ne = 2: the lower edge; lstm_in = 72
    'all_odd': case(33, 3, 1, 7, 3, ((5, 1), (6, 1))),      # e_obs = 11, lstm_in = 32, every dimension odd
}
# panel widths with compact rows on: the panel kernels read W_ih rows of another length (ldw = lstm_in) than 212
PANEL = {
    'h512_smp8': case(512, smp=8),                # lstm_in = 216
    'h512_addr10': case(512, addr=10),            # lstm_in = 104
    'h512_addr32_dtype4': case(512, addr=32, dtype=4),      # lstm_in = 140
    'h1024_addr10': case(1024, addr=10),
    'h512_smp3': case(512, smp=3),                # the control: c2 = 67, full-width rows - the panels must step aside
}
PANEL_B = {'h512_smp8': (40, 130), 'h512_addr10': (40, 130), 'h512_addr32_dtype4': (40, 130), 'h1024_addr10': (40,),
           'h512_smp3': (40, 130)}
CASES = dict(HIDDEN, **EMBED, **PANEL)
# IS-only networks (tests/test_gpu_is_step_fused.py)
IS_ONLY = {
    'h64_smp5': case(64, smp=5), 'h96_smp8_d2': case(96, 2, smp=8), 'h512_smp1': case(512, smp=1), 'h1024_smp8': case(1024, smp=8),
    'h512_smp9': case(512, smp=9),
}
ALL = dict(CASES, **IS_ONLY)

B_STEP = 130                                      # more than one workgroup of four waves; n_split > 1 on a single-statement batch
SEQUENCE = ('h50', (('ragged', 300), ('single_a0', 17), ('ragged', 40)))      # one engine, one workspace
ADAM = (('h33', 'single'), ('all_odd', 'ragged'))      # three Adam steps each
ADAM_LR = 0.05                                    # tests/test_gpu_optim.py's


def obs_pairs(c):
    return c[5] or OBS_DEFAULT


def lstm_in(c):
    H, depth, smp, addr, dtype, _ = c
    return sum(d for d, _ in obs_pairs(c)) + smp + 2 * (addr + dtype)


def routes(c):
    """The dimension predicates of the engine's routes, restated: which of them the network of case c passes.
    compact            engine.hip compact_rows: lstm_in % 4, (e_obs + smp_dim) % 4, lstm_dim % 16, ne = dtype_dim + addr_dim even, 2..128
    rec_cell_epilogue  engine.hip lstm_recurrence: the recurrent product with the cell in its epilogue, H % 16
    lean               engine.hip plan_step lean_cell (and lstm_input.hip lstm_input_fast_ok): compact rows, one layer, H % 64
    dh_partials        engine.hip lstm_backward: dh_{t-1} as stored split partials, H % 4 (else float atomics)
    tail               lstm_tail.hip tail_dim_ok: H in {256, 512, 1024}
    panel_dims         panel16.hip panel16_supported / panel.hip panel_t1_supported: H in {512, 1024} (512), behind lean
    is_small           is_step_small.hip is_small_network + is_step_small_supported: H % 32, 32..256 (256 from two layers on), smp_dim 1..8
    is_fused           is_step_fused.hip is_step_fused_supported: is_small, or one layer of H in {256, 512, 1024} and smp_dim 1..8
    is_first           is_kernels.hip is_first_statement_supported: one layer, lstm_in <= 256, H % 4, the fused observe embedding
    (What a batch or an address adds - T = 1 and one address for the panels, n_out <= 32 for the IS statements - is the test's.)"""
    H, depth, smp, addr, dtype, _ = c
    emb = obs_pairs(c)
    e, I, ne = sum(d for d, _ in emb), lstm_in(c), addr + dtype
    compact = I % 4 == 0 and (e + smp) % 4 == 0 and H % 16 == 0 and ne % 2 == 0 and 2 <= ne <= 128
    lean = compact and depth == 1 and H % 64 == 0
    small = H % 32 == 0 and 32 <= H <= 256 and not (H == 256 and depth == 1) and 1 <= smp <= 8
    return dict(compact=compact, rec_cell_epilogue=H % 16 == 0, lean=lean, dh_partials=H % 4 == 0, tail=H in (256, 512, 1024),
                panel_dims=lean and H in (512, 1024), is_small=small,
                is_fused=small or (H in (256, 512, 1024) and depth == 1 and 1 <= smp <= 8),
                is_first=depth == 1 and I <= 256 and H % 4 == 0 and EC.inside_envelope(emb) and EC.image_words(emb) <= 10240)


def _flags(word):
    names = ('compact', 'rec_cell_epilogue', 'lean', 'dh_partials', 'tail', 'panel_dims', 'is_small', 'is_fused', 'is_first')
    return dict(zip(names, (ch == '1' for ch in word)))


# what each case is there for: compact | rec_cell_epilogue | lean | dh_partials | tail | panel_dims | is_small | is_fused | is_first
EXPECTED = {
    'h96': '110100111', 'h48': '110100001', 'h100': '000100001', 'h50': '000000000', 'h33': '000000000', 'h384': '111100001',
    'h100_d2': '000100000', 'h50_d3': '000000000',
    'smp1': '010100111', 'smp8': '111100111', 'smp9': '010100001', 'addr10': '111100111', 'addr128': '010100110',
    'dtype7': '010100111', 'ne2': '111100111', 'all_odd': '000000000',
    'h512_smp8': '111111011', 'h512_addr10': '111111011', 'h512_addr32_dtype4': '111111011', 'h1024_addr10': '111111011',
    'h512_smp3': '010110011',
    'h64_smp5': '010100111', 'h96_smp8_d2': '110100110', 'h512_smp1': '010110011', 'h1024_smp8': '111111011',
    'h512_smp9': '010110001',
}
# route classes among CASES: h96 | h48 | h100 | h50, h33, h50_d3, all_odd | h384 | h100_d2 | smp1, dtype7 | smp8, addr10, ne2 | smp9 |
# addr128 | the four panel cases | h512_smp3
N_CLASSES = 12


def expected(name):
    return _flags(EXPECTED[name])


def all_builds():
    """{label: (case name, kind, B)} of every engine + batch that the training-step tests build."""
    builds = {}
    for name in HIDDEN:
        for kind in ('single', 'ragged'):
            if kind == 'ragged' or name not in HIDDEN_RAGGED_ONLY:
                builds['%s_%s' % (name, kind)] = (name, kind, B_STEP)
    for name in EMBED:
        for kind in ('single', 'ragged'):
            builds['%s_%s' % (name, kind)] = (name, kind, B_STEP)
    for name in PANEL:
        for B in PANEL_B[name]:
            builds['%s_single_b%d' % (name, B)] = (name, 'single', B)
    return builds


def dims_kw(c):
    return dict(smp_dim=c[2], addr_dim=c[3], dtype_dim=c[4])


def engine(name, kind, device='cuda:0'):
    c = ALL[name]
    H, depth = c[0], c[1]
    addresses = D.candidates(kind, 1)[1]
    eng = fresh_engine(H, addresses, 'Normal' if kind == 'single' else 'Uniform', lstm_depth=depth,
                       obs=EC.obs_of(c[5]) if c[5] else None, device=device, **dims_kw(c))
    spec = eng.spec
    assert (spec.lstm_dim, spec.lstm_depth, spec.smp_dim, spec.addr_dim, spec.dtype_dim, spec.lstm_in) == c[:5] + (lstm_in(c),)
    return trained_looking(eng, seed=H + depth)


def build(name, kind, B, device='cuda:0'):
    eng = engine(name, kind, device)
    return (eng,) + D.batch(eng, kind, B)


# ---- the importance-sampling statement (tests/test_gpu_is_step_fused.py) ------------------------------------------------------------
NORMAL, UNIFORM, CAT = ('a_normal', 'Normal'), ('a_uniform', 'Uniform'), ('a_cat', 'Categorical')
# (case name, particles, previous address, current address): particle counts 257 or 300 and one n = 1; the previous address a
# Normal one, and Categorical(7) - a one-hot sample embedding input of width 7 - once per smp_dim (4, 1, 5, 8, 9)
IS_STATEMENTS = [
    ('h50', 257, NORMAL, UNIFORM), ('h100', 300, CAT, NORMAL), ('h33', 257, NORMAL, UNIFORM),      # the chain of GEMM launches
    ('smp1', 300, CAT, UNIFORM), ('smp1', 1, NORMAL, NORMAL), ('h64_smp5', 257, CAT, NORMAL), ('h64_smp5', 300, NORMAL, UNIFORM),
    ('smp8', 257, CAT, UNIFORM), ('smp8', 300, NORMAL, NORMAL),                                     # the small kernel
    ('h96_smp8_d2', 300, NORMAL, UNIFORM),
    ('h512_smp1', 257, NORMAL, UNIFORM), ('h512_smp8', 300, NORMAL, NORMAL),                        # the big kernel
    ('h1024_smp8', 300, NORMAL, UNIFORM),
    ('smp9', 257, CAT, UNIFORM), ('h512_smp9', 300, NORMAL, NORMAL),                                # unsupported: the chain
    ('addr128', 300, NORMAL, UNIFORM), ('dtype7', 257, NORMAL, NORMAL),
    ('all_odd', 257, NORMAL, UNIFORM),
]
IS_FIRST = ('addr128', 'h50', 'h33', 'addr10', 'smp8')      # pp_is_first_statement_supported: 0, 0, 0, 1, 1
IS_FIRST_N = 257
IS_FIRST_PRIOR = (-1.5, 2.0)                                  # the Uniform prior of the first statement's address (a_uniform)
IS_SECOND = ('smp8', 'h100')                                 # the second statement on the shared first state


def is_kw(name):
    """Keyword arguments of helpers.is_engine for the network of an IS case."""
    c = ALL[name]
    return dict(depth=c[1], emb=EC.obs_of(c[5]) if c[5] else None, **dims_kw(c))
