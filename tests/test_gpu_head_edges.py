"""The proposal heads at saturated outputs (tests/head_edge_cases.py) on the device, against the float64 record of the
reference (tests/golden/head_edges.npz, which tests/test_oracle_head_edges.py pins oracle.ic_oracle to).

Metric: lp |got - ref64| / max(1, |ref64|) over finite rows with an equal -inf pattern; dy |got - ref64| over the largest
|ref64| of the case and output block (mean outputs, scale outputs, logits); dy exactly 0 on rescued rows; loss_acc against
the float64 sum; nonfinite == 0. Bar, per case and block: the larger of the suite's bar for the heads (lp 1e-4, dy 2e-4,
loss_acc 1e-5 relative; test_gpu_kernels._check_head) and 4 x the error of the reference's own fp32 run of that case
(head_edges.npz; capped at 1e-2 per case by the CPU test). The 4 is for the device's expf / erff / logf and evaluation
order, a few ulp each from torch's; no bar comes from a kernel's output. For loss_acc the reference's error is taken
as the sum of its rows' |lp32 - lp64| over |sum lp64|: a sum's error is at most that, and signed row errors that happen to
cancel in the record must not tighten the bar.

With PP_HEAD_EDGES_ERRORS=<file> every check appends {case, route, block, kernel_err, reference_fp32_err, bar}
(profiles/head_edges_errors.jsonl).

Which case runs which branch (weight pattern names: head_edge_cases.WEIGHTS; value tags: head_edge_cases.VALUE_TAGS):
  weight below eps (log_clamped's lower bound, gradient mask off)   *_K3 / *_K16 patterns lead_above_*, one_below, many_below,
                                                                     inside_one_below, tie_*; categorical_C* many_below and
                                                                     value tag cat_clamped (pv below eps: lp = log eps, dy = 0)
  weight above 1 - eps (upper bound, mask off)                      *_K1 (p = 1), *_K3 / *_K16 lead_above_*; categorical_C2
                                                                     lead_above_rest_below with tag cat_lead
  Bernoulli p clamped below / above                                 bernoulli_edges, y <= -20 / y >= 20
  scale floor range / 1000, ceiling, mean on an edge                uniform_K*, poisson_K* (every other row's leading component)
  value on / one fp32 step outside a bound (rescued)                uniform_K*, poisson_K* tags low, high, count0, count40, below,
                                                                     above
  |tt| near 1000                                                    *_K3_tt1000
  N(0, 1) outputs for kinds 3 and 4                                 poisson_K3_ordinary, bernoulli_ordinary
  a NaN output / Z = 0 on the Poisson head                          test_flag_*: `nonfinite`, dy = 0, other rows bit-equal

Routes (the `route` of a record line) and the kernel that carries the head there:
  direct                 pp_head_logprob: head_mixture_kernel / head_categorical_kernel / head_bernoulli_kernel, every case
  panel16, panel8        single statements at H = 512, K = 3: csrc/panel16.hip, csrc/panel.hip (PP_PANEL=1, a child process)
  tiles_h512             the same batch at K = 16, which no panel takes: head_tail_kernel behind the tile kernels
  ragged_h64             a short ragged batch at H = 64, K = 3 and 16: head_tail_kernel, one job per address
  feedforward            the FeedForward network, Normal, K = 3
  is_fused_one_kernel, is_fused_split (H = 512), is_small (H = 64, two layers), is_chain (H = 48): ops.is_step re-scoring
                         given values; test_is_draw draws on each of them
The network routes run two patterns per head and K (ROUTE_PATTERNS): the collapsed one - leading weight above 1 - eps, every
other below eps, the leading mean on the edge of the support with the scale on its floor - and one with a leading weight
inside and others below eps. Categorical and Bernoulli heads have one implementation of the training head, the direct one; in
importance sampling they are scored by kernels of their own behind every statement (test_is_rescore_discrete_heads: a
category above 1 - eps, values on categories below eps, the Bernoulli probability clamped on either side).
"""
import json
import os

import numpy as np
import pytest

import head_edge_cases as E

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_edges.npz')
LP_BAR, DY_BAR, LOSS_BAR = 1e-4, 2e-4, 1e-5     # the suite's bars for the heads (test_gpu_kernels._check_head)
LOG_EPSILON = float(np.log(1e-8))
CASES = sorted(E.head_edge_cases())


@pytest.fixture(scope='module')
def env():
    from pyprob_amd import lib as L
    lib = L.load()
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return L, lib, torch.device('cuda:0')


@pytest.fixture(scope='module')
def record():
    """name -> (lp64, dy64 with exact zeros on rescued rows, yardstick): the float64 record and the reference's own fp32
    error in this file's metric {lp, loss, mean, scale, logits}. Computed once, read-only."""
    G = np.load(GOLDEN)
    out = {}
    for name, case in E.head_edge_cases().items():
        assert np.array_equal(G[name + '_y'], case['y'].astype(np.float32)), 'head_edges.npz is stale: rerun make_head_edges_golden.py'
        lp64 = G[name + '_lp64']
        resc = np.isneginf(lp64)[:, None]
        dy64 = np.where(resc, 0.0, G[name + '_dy64'])
        yard = {'lp': E.lp_error(G[name + '_lp32'], lp64)}
        yard.update(E.dy_errors(case, np.where(resc, 0.0, G[name + '_dy32']), dy64))
        fin = np.isfinite(lp64)
        yard['loss'] = float(np.abs(G[name + '_lp32'].astype(np.float64)[fin] - lp64[fin]).sum() / abs(loss_sum(lp64)))
        for a in (lp64, dy64):
            a.setflags(write=False)
        out[name] = (lp64, dy64, yard)
    return out


def loss_sum(lp):
    return float(-np.where(np.isneginf(lp), LOG_EPSILON, lp).sum())


def bar_for(block, yard):
    if block == 'lp_mean':          # the mean of the rows' log_prob (a training step's loss): the rows' own bar
        block = 'lp'
    floor = LP_BAR if block == 'lp' else LOSS_BAR if block == 'loss' else DY_BAR
    return max(floor, 4.0 * yard[block])


def check(case, route, errs, yard):
    """errs: block -> measured error. Writes the record lines, then asserts every block against its bar."""
    lines = [dict(case=case, route=route, block=b, kernel_err=float(e), reference_fp32_err=float(yard['lp' if b == 'lp_mean' else b]), bar=bar_for(b, yard))
             for b, e in errs.items()]
    path = os.environ.get('PP_HEAD_EDGES_ERRORS')
    if path:
        with open(path, 'a') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')
    for ln in lines:
        print(json.dumps(ln))
        assert ln['kernel_err'] <= ln['bar'], ln


def dev(a, device, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(device)


GRAD_SCALE = -1.0 / 64


def run_direct(env, case, y=None, seed=0):
    """pp_head_logprob on the case with a row permutation (row i of Y belongs to trace row rows[i]), ldy padded beyond
    n_out to a multiple of 4 (NaN in Y's padding, a sentinel in dY's), grad_scale != 1. Returns lp, dy / grad_scale in the
    case's row order, loss_acc, nonfinite."""
    L, lib, device = env
    y = case['y'] if y is None else y
    n, n_out = y.shape
    assert n % 64 != 0
    ldy = (n_out // 4 + 1) * 4
    rows = np.random.default_rng(seed).permutation(n).astype(np.int32)
    Y = np.full((n, ldy), np.nan, np.float32)
    Y[:, :n_out] = y
    value = np.zeros(n, np.float32); value[rows] = case['value']
    pr = np.zeros((n, 2), np.float32); pr[rows] = case['prior']
    dY, dR, dV, dP = dev(Y, device), dev(rows, device, np.int32), dev(value, device), dev(pr, device)
    lp = torch.full((n,), 7.0, device=device)
    dyo = torch.full((n, ldy), 7.0, device=device)
    acc = torch.zeros(1, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    L.check(lib.pp_head_logprob(case['kind'], dY.data_ptr(), ldy, dR.data_ptr(), dV.data_ptr(), dP.data_ptr(), n, n_out,
                                GRAD_SCALE, lp.data_ptr(), dyo.data_ptr(), acc.data_ptr(), flag.data_ptr(), L.stream_ptr()),
            'pp_head_logprob')
    torch.cuda.synchronize()
    dy = dyo.cpu().numpy()
    assert np.all(dy[:, n_out:] == 7.0), 'pp_head_logprob wrote into the padding of dy'
    return lp.cpu().numpy()[rows], dy[:, :n_out] / GRAD_SCALE, float(acc.item()), int(flag.item())


@pytest.mark.parametrize('name', CASES)
def test_direct_abi(env, record, name):
    """pp_head_logprob, kinds 0-4, on every case."""
    case = E.head_edge_cases()[name]
    lp64, dy64, yard = record[name]
    lp, dy, acc, flag = run_direct(env, case)
    assert flag == 0
    errs = {'lp': E.lp_error(lp, lp64)}
    resc = np.isneginf(lp64)
    assert np.all(dy[resc] == 0.0), 'dy on a rescued row'
    errs.update(E.dy_errors(case, dy, dy64))
    errs['loss'] = abs(acc - loss_sum(lp64)) / abs(loss_sum(lp64))
    check(name, 'direct', errs, yard)
    # the clamp masks, asserted exactly: a weight outside [eps, 1 - eps] gets no gradient through the clamp, so where every
    # weight of a row is outside, the row's logit gradients are exactly zero (and not merely small) ...
    p = E.weights(case)
    below, above = E.clamp_masks(p)
    sl = E.blocks(case)['logits']
    if case['head'] == 'Categorical':
        pv = p[np.arange(len(p)), case['value'].astype(np.int64)]
        out = (pv < E.EPS) | (pv > 1 - E.EPS)
        assert out.any() and np.all(dy[out][:, sl] == 0.0)
        np.testing.assert_allclose(lp[pv < E.EPS], np.log(E.EPS), rtol=1e-6)
    else:
        out = (below | above).all(1)
        if 'ordinary' not in name:
            assert out.any()
        assert np.all(dy[out][:, sl] == 0.0)


def _flag_case(env, record, name, row, bad):
    """bad: {column: head output} planted in one row."""
    case = E.head_edge_cases()[name]
    lp0, dy0, _, flag0 = run_direct(env, case)
    assert flag0 == 0
    y = case['y'].astype(np.float32).copy()
    for col, x in bad.items():
        y[row, col] = x
    lp1, dy1, _, flag1 = run_direct(env, case, y=y)
    assert flag1 != 0, 'nonfinite not set'
    assert not np.isfinite(lp1[row]) and not np.isneginf(lp1[row])
    assert np.all(dy1[row] == 0.0)
    keep = np.arange(len(lp0)) != row
    assert np.array_equal(lp0[keep].view(np.int32), lp1[keep].view(np.int32))
    assert np.array_equal(dy0[keep].view(np.int32), dy1[keep].view(np.int32))


@pytest.mark.parametrize('name,col', [('normal_K3', 8), ('normal_K1', 0), ('uniform_K16', 19), ('poisson_K3', 2),
                                      ('categorical_C7', 6), ('bernoulli_edges', 0)])
def test_flag_nan_output(env, record, name, col):
    """A NaN head output in one row sets `nonfinite`, zeroes that row's dy and leaves every other row bit-equal: a NaN logit
    (normal_K3: every weight of the row turns NaN, which a clamp by fmaxf / fminf alone turns into eps), the only mean of a
    one-component head (every component NaN: fmaxf leaves the running maximum at -inf, the mark of a rescued row), a scale, a
    mean, a categorical logit, the Bernoulli output."""
    row = int(np.nonzero(np.isfinite(record[name][0]))[0][5])
    _flag_case(env, record, name, row, {col: np.nan})


def test_flag_poisson_wide_scale(env, record):
    """ysd = 20 on the Poisson head, the component's mean at 40 sigmoid(-1) = 10.8: Z = Phi(beta) - Phi(alpha) cancels to 0 in
    fp32, as in the reference, and log(sd Z) = -inf makes the component +inf. (sd = e^20: |alpha|, beta < 8.3e-8. Both Phi
    round to 0.5 exactly where erf(alpha / sqrt2) > -2^-25 and erf(beta / sqrt2) < 2^-24, that is for a mean between 4 and 18;
    nearer to a bound one of them keeps a last bit and Z = 2^-25.)"""
    name = 'poisson_K3'
    K = 3
    row = int(np.nonzero(np.isfinite(record[name][0]))[0][7])
    _flag_case(env, record, name, row, {1: -1.0, K + 1: 20.0})


# ---- the other training implementations: the heads inside a training step ------------------------------------------------------------
# The head's last layer is patched to b2 := a pattern row of a case and W2 := 0.05 x its initial value: every row of the batch
# gets the pattern plus a small row-dependent part, so dW2 / dz1 still carry signal. Two patterns per head and K:
#   collapsed   the leading weight above 1 - eps with every other below eps (both clamp bounds, every mask off: the logit
#               gradients are exactly zero), the leading component saturated (SATURATED_LEAD)
#   one below   a leading weight inside [eps, 1 - eps] with others below eps (mask on and off within one row), the leading
#               component at moderate outputs (MODERATE_LEAD), so that every output block carries a gradient of ordinary size
# Metric of a route's head-layer gradients (dW2 and db2 of every address, rows of the block): |got - oracle| over the largest
# |oracle| of that block and tensor kind in the route's two runs and all addresses - the "largest of the case and block" of the
# dy metric, with the two runs as the case. (One run alone will not do: in the collapsed pattern the mean block of a
# TruncatedNormal head is ~1e-7, all of it through sigmoids saturated at 1 - sm ~ 1e-6, which fp32 holds to a few percent - in
# the reference too - and an address that only two rows reach has blocks at the size of the summation noise.)
# The loss of a step is -mean(lp): its error is measured like the rows', |got - oracle| over the mean of max(1, |lp_i|), with
# the rows' bar (block `lp_mean`); relative to the loss itself it means nothing where positive and negative rows cancel (the
# Normal runs: loss -0.075 from rows of +1.4 and -4.9).
ROUTE_PATTERNS = {3: ('lead_above_rest_below', 'inside_one_below'), 16: ('lead_above_rest_below', 'many_below')}
# the leading component's (mean, scale) outputs in the collapsed pattern: the mean on the lower edge of the support with the scale
# on its floor (Uniform: range / 1000; Poisson: exp(-8), allowed next to the lower edge); Normal: see ROUTE_NORMAL_MIN_YSD
SATURATED_LEAD = {'Normal': (2.5, -4.0), 'Uniform': (-20.0, -20.0), 'Poisson': (-20.0, -8.0)}
MODERATE_LEAD = {'Normal': (0.5, 0.0), 'Uniform': (1.0, -3.0), 'Poisson': (-2.0, 1.0)}
# Inside a network the head outputs are themselves fp32 results: y = b2 + W2 a1 carries about ulp(|y|) = 4.8e-7 at |y| ~ 6 from
# the product alone (and ~1e-6 behind the IS statements' LSTM cell on the hardware exp / rcp, h to 4e-6 absolute, asserted in
# tests/test_gpu_is_step_fused.py). The yardstick, the reference's fp32 run on EXACT head outputs, does not contain that term. A
# Normal component of scale exp(ysd) pb turns it into an error of tt of ulp(y) pb / sd = 4.8e-7 exp(-ysd): 1.9e-4 at ysd = -6,
# the whole dy bar, 2.6e-5 at ysd = -4. So the Normal components of the pattern rows keep ysd >= -4; the direct tests above, whose
# y is exact, keep exp(-6). (TruncatedNormal: the floor range / 1000 sits under a sigmoid saturated at -20, where y's rounding
# does not reach the scale or the mean.)
ROUTE_NORMAL_MIN_YSD = -4.0


def pattern_row(head, K, which):
    case = E.head_edge_cases()['%s_K%d' % (head.lower(), K)]
    i = int(np.nonzero(case['weights'] == which)[0][0])
    y = case['y'][i].astype(np.float32)
    lead = int(np.argmax(y[2 * K:]))
    y[lead], y[K + lead] = (SATURATED_LEAD if which == 'lead_above_rest_below' else MODERATE_LEAD)[head]
    if head == 'Normal':
        y[K:2 * K] = np.maximum(y[K:2 * K], ROUTE_NORMAL_MIN_YSD)
    return case['name'], y


def edge_values(head, K, b2, prior, seed):
    """The part 1 values for rows whose head outputs are (close to) b2: at the leading component's mean, near it, on and one
    fp32 step outside the bounds of the support (counts 0 / 40, -1 and the step above 40 for Poisson), at another mean."""
    rng = np.random.default_rng(seed)
    n = len(prior)
    prior = prior.astype(np.float64)
    mu, sd = E.component_params(head, np.tile(b2.astype(np.float64), (n, 1)), prior, K)
    lead = int(np.argmax(b2[2 * K:]))
    tags = ('lead_mean', 'near', 'other_mean', 'near') if head == 'Normal' else \
        ('lead_mean', 'near', 'low', 'high', 'below', 'above', 'other_mean', 'near')
    v = np.zeros(n)
    for i in range(n):
        t = tags[i % len(tags)]
        lo, hi = prior[i]
        if t == 'lead_mean':
            x = mu[i, lead]
        elif t == 'near':
            x = mu[i, lead] + rng.uniform(-2, 2) * sd[i, lead]
        elif t == 'other_mean':
            x = mu[i, (lead + 1) % K]
        elif t == 'low':
            x = lo
        elif t == 'high':
            x = hi
        elif t == 'below':
            x = -1.0 if head == 'Poisson' else np.nextafter(np.float32(lo), np.float32(-np.inf))
        else:
            x = np.nextafter(np.float32(hi), np.float32(np.inf))
        if head != 'Normal' and t in ('lead_mean', 'near', 'other_mean'):
            x = min(max(x, lo), hi)
        v[i] = x
    return v.astype(np.float32)


def route_setup(route, head, K, which, device='cuda:0'):
    """(engine with patched heads, its state dict, batch arrays, addresses, name of the case whose yardstick applies)"""
    import helpers as Hh
    from pyprob_amd.packed import POISSON_LOW_HIGH
    seed = 7 + K
    if route == 'ragged_h64':
        arrays, addresses = Hh.synthetic_gumm_arrays(24, seed=seed, max_iter=3)
        H, network = 64, 'lstm'
    else:
        arrays, addresses = Hh.synthetic_gum_arrays(40, seed=seed), ['mu']
        H, network = (64, 'feedforward') if route == 'feedforward' else (512, 'lstm')
    n = len(arrays['values'])
    if head == 'Poisson':
        arrays['prior'] = np.tile(np.array([POISSON_LOW_HIGH], np.float32), (n, 1))
    elif head == 'Uniform' and route != 'ragged_h64':
        arrays['prior'] = np.tile(np.array([[-4.0, 6.0]], np.float32), (n, 1))
    elif head == 'Normal' and route == 'ragged_h64':
        arrays['prior'] = np.tile(np.array([[1.0, 2.0]], np.float32), (n, 1))
    eng = Hh.fresh_engine(H, addresses, head, seed=seed, K=K, network=network, device=device)
    case_name, b2 = pattern_row(head, K, which)
    sd = {k: v.numpy().copy() for k, v in eng.state_dict().items()}
    for a in addresses:
        p = '_layers_proposal.%s._ff._layers.1.' % a
        sd[p + 'weight'] = (0.05 * sd[p + 'weight']).astype(np.float32)
        sd[p + 'bias'] = b2.copy()
    eng.load_state_dict(sd)
    arrays['values'] = edge_values(head, K, b2, arrays['prior'], seed)
    return eng, sd, arrays, addresses, case_name


def measure_route(route, head, K, which):
    """One loss + backward of an engine with patched heads against helpers.oracle_run on the same state dict. Returns
    (name of the case whose yardstick applies, {block: error}); asserts the route's predicates, the status word and the
    per-row log_prob (helpers.check_lp)."""
    import dim_cases as DC
    import helpers as Hh
    eng, sd, arrays, addresses, case_name = route_setup(route, head, K, which)
    H = 512 if route in ('panel16', 'panel8', 'tiles_h512') else 64
    dists = [head] * len(addresses)
    pb = Hh.packed(arrays, eng.spec).to(eng.device)
    # the route: the predicates the suite has (dim_cases.routes, the first launch's image jobs)
    c = DC.case(H)
    if route in ('panel16', 'panel8', 'tiles_h512'):
        assert DC.routes(c)['panel_dims'] and pb.t_max == 1 and pb.n_traces == 40
    elif route == 'ragged_h64':
        assert not DC.routes(c)['panel_dims'] and pb.t_max >= 2 and eng.spec.lstm_dim == 64
    else:
        assert eng.spec.feedforward
    l, lp = eng.loss(pb, backward=True, keep_lp=True)
    torch.cuda.synchronize()
    assert int(eng.status_buf[0].item()) == 0
    if route in ('panel16', 'panel8', 'tiles_h512'):
        trace = torch.zeros(8 * 4096, dtype=torch.int64, device=eng.device)
        from pyprob_amd import lib as L
        lib = L.load()
        lib.pp_debug_wgtrace(trace.data_ptr(), 4096, 4)
        try:
            eng.loss(pb, backward=True)
            torch.cuda.synchronize()
        finally:
            lib.pp_debug_wgtrace(None, 0, 0)
        t = trace.cpu().numpy().reshape(4096, 8)
        image_jobs = int(((t[:, 0] > 0) & (t[:, 7] == 2)).sum())      # (tests/test_gpu_dims.py _first_launch_trace)
        assert (image_jobs > 0) == (route != 'tiles_h512'), (route, K, image_jobs)
        assert (os.environ.get('PP_PANEL', '2') == '1') == (route == 'panel8')
    out = Hh.oracle_run(eng.spec, sd, arrays, addresses, dists)
    ref_lp = Hh.oracle_lp_rows(out, arrays)
    assert np.isneginf(ref_lp).any() == (head != 'Normal')
    Hh.check_lp(Hh.unpack_lp(pb, lp.cpu().numpy()), ref_lp, '%s/%s/K%d/%s' % (route, head, K, which))
    terms = np.where(np.isneginf(ref_lp), LOG_EPSILON, ref_lp)
    raw = {'lp_mean': abs(float(l.item()) - out['loss']) / float(np.maximum(1.0, np.abs(terms)).mean())}
    g = eng.grad_dict()
    for b, sl in (('mean', slice(0, K)), ('scale', slice(K, 2 * K)), ('logits', slice(2 * K, 3 * K))):
        for s in ('weight', 'bias'):
            names = ['_layers_proposal.%s._ff._layers.1.%s' % (a, s) for a in addresses]
            raw['%s.%s.err' % (b, s)] = float(max(np.abs(g[nme][sl] - out['grads'][nme][sl]).max() for nme in names))
            raw['%s.%s.max' % (b, s)] = float(max(np.abs(out['grads'][nme][sl]).max() for nme in names))
    return case_name, raw


def route_errors(raws):
    """raws: the raw figures of a route's two runs -> per run {block: error} in the metric above."""
    out = []
    for raw in raws:
        errs = {'lp_mean': raw['lp_mean']}
        for b in ('mean', 'scale', 'logits'):
            errs[b] = 0.0
            for s in ('weight', 'bias'):
                scale = max(r['%s.%s.max' % (b, s)] for r in raws)
                e = raw['%s.%s.err' % (b, s)]
                errs[b] = max(errs[b], e / scale if scale > 0 else e)
        out.append(errs)
    return out


def _check_route(route, head, K, record, measured=None):
    measured = measured or [measure_route(route, head, K, which) for which in ROUTE_PATTERNS[K]]
    collapsed = measured[0][1]
    assert collapsed['logits.weight.err'] == 0.0 and collapsed['logits.bias.err'] == 0.0 and collapsed['logits.bias.max'] == 0.0
    assert measured[1][1]['logits.bias.max'] > 1e-3
    for which, (case_name, _), errs in zip(ROUTE_PATTERNS[K], measured, route_errors([m[1] for m in measured])):
        check(case_name, '%s/%s' % (route, which), errs, record[case_name][2])


@pytest.mark.parametrize('head', ['Normal', 'Uniform', 'Poisson'])
def test_panel16_h512(record, head):
    """Single statements, H = 512, B = 40 (three 16-row panels, the last one half full), K = 3: lane_mixture_logprob /
    lane_mixture_grad in csrc/panel16.hip."""
    _check_route('panel16', head, 3, record)


@pytest.mark.parametrize('head', ['Normal', 'Uniform', 'Poisson'])
def test_head_tail_h512_k16(record, head):
    """The same batch at K = 16: no panel takes 48 outputs (the first launch builds no panel images), the fused tail
    head_tail_kernel does."""
    _check_route('tiles_h512', head, 16, record)


@pytest.mark.parametrize('head', ['Normal', 'Uniform', 'Poisson'])
@pytest.mark.parametrize('K', [3, 16])
def test_head_tail_ragged_h64(record, head, K):
    """A short ragged batch (24 traces of 2-6 statements, six addresses) at H = 64: head_tail_kernel per address and step."""
    _check_route('ragged_h64', head, K, record)


def test_feedforward_network(record):
    """The FeedForward network once (Normal, K = 3)."""
    _check_route('feedforward', 'Normal', 3, record)


PANEL8_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(repo)r + '/tests')
import test_gpu_head_edges as T
out = {head: [T.measure_route('panel8', head, 3, which) for which in T.ROUTE_PATTERNS[3]] for head in ('Normal', 'Uniform', 'Poisson')}
print('PANEL8 ' + json.dumps(out))
'''


def test_panel8_h512_in_a_child_process(record):
    """The 8-row panel (csrc/panel.hip) takes these batches only under PP_PANEL=1, which is read once per process: the three
    heads at K = 3 in one child process, measured there and asserted here."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PP_PANEL='1')
    r = subprocess.run([sys.executable, '-c', PANEL8_SCRIPT % dict(repo=repo)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('PANEL8 ')][-1]
    for head, measured in json.loads(line[7:]).items():
        _check_route('panel8', head, 3, record, measured=[tuple(m) for m in measured])


# ---- importance sampling: the statement re-scores given values (value_in) and draws -----------------------------------------------
# route -> (H, LSTM depth): the fused statement (is_step_fused.hip; one kernel and the two-launch split), the small statement
# (is_step_small.hip) and the chain of GEMM launches with the draw of is_kernels.hip / is_draw.hpp
IS_ROUTES = {'fused_one_kernel': (512, 1), 'fused_split': (512, 1), 'small': (64, 2), 'chain': (48, 1)}
IS_ADDR = {'Normal': ('a_normal', 'Normal'), 'Uniform': ('a_uniform', 'Uniform'), 'Poisson': ('a_poisson', 'Poisson')}
IS_K = 3


def is_setup(route, head, which, monkeypatch, device='cuda:0'):
    """(engine, runner, state dict with the head of `head`'s address patched as in route_setup, case name, current and previous
    address); asserts which statement the network takes."""
    import ctypes as C
    import dim_cases as DC
    import helpers as Hh
    H, depth = IS_ROUTES[route]
    if route.startswith('fused'):
        monkeypatch.setenv('PP_IS_STEP_FUSED', '2' if route == 'fused_one_kernel' else '3')
    eng, run, sd = Hh.is_engine(H, seed=4, depth=depth, K=IS_K, device=device)
    cur = IS_ADDR[head]
    prev = IS_ADDR['Uniform' if head == 'Normal' else 'Normal']
    case_name, b2 = pattern_row(head, IS_K, which)
    p = '_layers_proposal.%s._ff._layers.1.' % cur[0]
    sd = dict(sd)
    sd[p + 'weight'] = (0.05 * sd[p + 'weight']).astype(np.float32)
    sd[p + 'bias'] = b2.copy()
    eng.load_state_dict(sd)
    r = DC.routes(DC.case(H, depth))
    if device == 'cpu':
        return eng, run, sd, case_name, cur, prev
    supported = eng.lib.pp_is_step_fused_supported(C.byref(eng.net), eng.spec.address_id[cur[0]], 257)
    assert (r['is_fused'], r['is_small'], supported) == {'fused': (True, False, 1), 'small': (True, True, 1),
                                                         'chain': (False, False, 0)}[route.split('_')[0]]
    return eng, run, sd, case_name, cur, prev


def is_prior(head, n, rng):
    if head == 'Normal':
        return np.stack([rng.choice([-3.0, 0.0, 0.75], n), rng.choice([0.5, 1.0, 3.0], n)], 1).astype(np.float32)
    if head == 'Uniform':
        lo = rng.choice([-3.0, 0.25, 1.5], n)
        return np.stack([lo, lo + rng.choice([0.5, 1.0, 4.0], n)], 1).astype(np.float32)
    return np.tile(np.array([[0.0, 40.0]], np.float32), (n, 1))


def is_statement(eng, run, cur, prev, h0, c0, pv, prior, value_in, seed):
    from pyprob_amd.ops import ops
    dev_, n = eng.device, len(pv)
    h = torch.from_numpy(h0.copy()).to(dev_).contiguous()
    c = torch.from_numpy(c0.copy()).to(dev_).contiguous()
    run._ensure_ws(n)
    pt = torch.tensor([[0.0, 40.0]], device=dev_) if cur[1] == 'Poisson' else torch.from_numpy(prior).to(dev_)
    vin = None if value_in is None else torch.from_numpy(value_in).to(dev_)
    value, logq = ops.is_step(eng.params, run.ws, eng.net_handle, eng.spec.address_id[cur[0]], eng.spec.address_id[prev[0]], n,
                              run.e_obs, torch.from_numpy(pv).to(dev_), pt, h, c, n, vin, seed, 0)
    torch.cuda.synchronize()
    return value.cpu().numpy(), logq.cpu().numpy()


@pytest.mark.parametrize('head', ['Normal', 'Uniform', 'Poisson'])
@pytest.mark.parametrize('route', sorted(IS_ROUTES))
def test_is_rescore(record, monkeypatch, route, head):
    """ops.is_step with value_in on 257 particles: log q of the part 1 values against the oracle's statement."""
    from test_gpu_is_step_fused import _oracle_statement, statement_inputs
    H, depth = IS_ROUTES[route]
    n = 257
    for which in ROUTE_PATTERNS[IS_K]:
        eng, run, sd, case_name, cur, prev = is_setup(route, head, which, monkeypatch)
        h0, c0, pv, _ = statement_inputs(H, depth, n, prev, cur)
        prior = is_prior(head, n, np.random.default_rng(3))
        values = edge_values(head, IS_K, sd['_layers_proposal.%s._ff._layers.1.bias' % cur[0]], prior, 5)
        v, lq = is_statement(eng, run, cur, prev, h0, c0, pv, prior, values, 77)
        assert np.array_equal(v, values)
        o_h0, o_c0 = (h0[0], c0[0]) if depth == 1 else (h0, c0)
        _, _, lq_ref, _ = _oracle_statement(sd, H, [8.0, 9.0], prev, cur, pv, o_h0, o_c0, values.astype(np.float64),
                                            prior.astype(np.float64), depth=depth, K=IS_K)
        assert np.isneginf(lq_ref).any() == (head != 'Normal')
        check(case_name, 'is_%s/%s' % (route, which), {'lp': E.lp_error(lq, lq_ref)}, record[case_name][2])


@pytest.mark.parametrize('route', sorted(IS_ROUTES))
def test_is_draw(monkeypatch, route):
    """The draw of a collapsed Uniform head: leading weight above 1 - eps, its mean on the lower edge of the support, its scale
    on the floor range / 1000. 40 000 particles share one state, so one proposal: the values are finite and inside [low, high),
    and their Kolmogorov-Smirnov distance to the float64 mixture CDF stays below 1.95 / sqrt(n) (exceeded with probability
    1e-3 by n i.i.d. draws; tests/test_gpu_is_step_fused.py)."""
    from oracle import ic_oracle as O
    from helpers import IS_EMB
    from test_gpu_is_step_fused import _mixture_cdf, _oracle_statement
    H, depth = IS_ROUTES[route]
    n = 40000
    eng, run, sd, _, cur, prev = is_setup(route, 'Uniform', 'lead_above_rest_below', monkeypatch)
    rng = np.random.default_rng(11)
    h0 = np.tile((0.5 * rng.standard_normal((depth, 1, H))).astype(np.float32).clip(-0.99, 0.99), (1, n, 1))
    c0 = np.tile(rng.standard_normal((depth, 1, H)).astype(np.float32), (1, n, 1))
    pv = np.full(n, 0.37, np.float32)
    prior = np.tile(np.array([[-1.0, 1.5]], np.float32), (n, 1))
    v, lq = is_statement(eng, run, cur, prev, h0, c0, pv, prior, None, 4242)
    v = v.astype(np.float64)
    lo, hi = -1.0, 1.5
    assert np.all(np.isfinite(v)) and np.all((v >= lo) & (v < hi))
    _, _, _, y = _oracle_statement(sd, H, [8.0, 9.0], prev, cur, pv[:1], h0[0, :1] if depth == 1 else h0[:, :1],
                                   c0[0, :1] if depth == 1 else c0[:, :1], None, None, depth=depth, K=IS_K)
    net = O.Net(sd, list(IS_EMB), K=IS_K)
    lq_ref, _, params = O.head_forward(net, cur[0], cur[1], None, prior.astype(np.float64), v, y=np.broadcast_to(y[:1], (n, y.shape[1])))
    mu, sdv, p = (np.asarray(a)[0] for a in params)
    assert p.max() > 1 - E.EPS and sdv[p.argmax()] < 1.001 * (hi - lo) / 1000 and mu[p.argmax()] - lo < 1e-6
    xs = np.sort(v)
    F = _mixture_cdf(xs, (mu, sdv, p), 'Uniform', lo, hi)
    i = np.arange(1, n + 1)
    D = max(np.abs(i / n - F).max(), np.abs((i - 1) / n - F).max())
    assert D < 1.95 / np.sqrt(n), (D, 1.95 / np.sqrt(n))


# the Categorical and Bernoulli heads of the IS statements are scored and drawn by kernels of their own (is_kernels.hip) behind
# every statement route: (head, categories, b2 source). Categorical: a row of the case with that weight pattern; Bernoulli: the
# one output, clamped above / below / inside.
IS_DISCRETE = [('Categorical', 2, 'lead_above_rest_below'), ('Categorical', 7, 'many_below'), ('Bernoulli', None, 30.0),
               ('Bernoulli', None, -30.0), ('Bernoulli', None, -14.0)]


def is_discrete_setup(route, head, ncat, src, monkeypatch, device='cuda:0'):
    import helpers as Hh
    H, depth = IS_ROUTES[route]
    if route.startswith('fused'):
        monkeypatch.setenv('PP_IS_STEP_FUSED', '2' if route == 'fused_one_kernel' else '3')
    addrs = [(a, d, ncat if d == 'Categorical' and ncat else c) for a, d, c in Hh.IS_ADDRS]
    eng, run, sd = Hh.is_engine(H, seed=4, depth=depth, K=IS_K, addrs=addrs, device=device)
    cur = ('a_cat', 'Categorical') if head == 'Categorical' else ('a_bern', 'Bernoulli')
    if head == 'Categorical':
        case = E.head_edge_cases()['categorical_C%d' % ncat]
        b2 = case['y'][int(np.nonzero(case['weights'] == src)[0][0])].astype(np.float32)
    else:
        case = E.head_edge_cases()['bernoulli_edges']
        b2 = np.array([src], np.float32)
    p = '_layers_proposal.%s._ff._layers.1.' % cur[0]
    sd = dict(sd)
    sd[p + 'weight'] = (0.05 * sd[p + 'weight']).astype(np.float32)
    sd[p + 'bias'] = b2.copy()
    eng.load_state_dict(sd)
    return eng, run, sd, case['name'], cur, ('a_normal', 'Normal'), addrs, b2


@pytest.mark.parametrize('head,ncat,src', IS_DISCRETE)
@pytest.mark.parametrize('route', ['chain', 'fused_split', 'small'])
def test_is_rescore_discrete_heads(record, monkeypatch, route, head, ncat, src):
    """log q of given Categorical / Bernoulli values behind three statement routes: the leading category above 1 - eps (C = 2),
    categories below eps with the value on them (C = 7: log q = log eps), the Bernoulli probability clamped on either side."""
    from test_gpu_is_step_fused import _oracle_statement, statement_inputs
    H, depth = IS_ROUTES[route]
    n = 257
    eng, run, sd, case_name, cur, prev, addrs, b2 = is_discrete_setup(route, head, ncat, src, monkeypatch)
    h0, c0, pv, _ = statement_inputs(H, depth, n, prev, cur)
    prior = np.zeros((n, 2), np.float32)
    if head == 'Categorical':
        picks = np.array([0, ncat - 1, int(b2.argmax()), int(b2.argmin())], np.float32)
        values = picks[np.arange(n) % 4]
    else:
        values = (np.arange(n) % 2).astype(np.float32)
    from pyprob_amd.ops import ops
    dev_ = eng.device
    h = torch.from_numpy(h0.copy()).to(dev_).contiguous()
    c = torch.from_numpy(c0.copy()).to(dev_).contiguous()
    run._ensure_ws(n)
    v, lq = ops.is_step(eng.params, run.ws, eng.net_handle, eng.spec.address_id[cur[0]], eng.spec.address_id[prev[0]], n,
                        run.e_obs, torch.from_numpy(pv).to(dev_), None, h, c, n, torch.from_numpy(values).to(dev_), 77, 0)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), values)
    o_h0, o_c0 = (h0[0], c0[0]) if depth == 1 else (h0, c0)
    _, _, lq_ref, y = _oracle_statement(sd, H, [8.0, 9.0], prev, cur, pv, o_h0, o_c0, values.astype(np.float64),
                                        prior.astype(np.float64), depth=depth, K=IS_K, addrs=addrs)
    # the clamp branch the case is there for is taken (in float64, with the factor 2 of head_edge_cases)
    p = E.weights({'head': head, 'y': y})
    assert E.weight_margin(p) >= 2.0
    below, above = E.clamp_masks(p)
    if head == 'Categorical':
        pv_ = p[np.arange(n), values.astype(np.int64)]
        assert ((pv_ > 1 - E.EPS).any() and (pv_ < E.EPS).any()) if ncat == 2 else (pv_ < E.EPS).any()
    else:
        assert above.all() if src == 30.0 else below.all() if src == -30.0 else not (below | above).any()
    check(case_name, 'is_%s/%s' % (route, src), {'lp': E.lp_error(lq.cpu().numpy(), lq_ref)}, record[case_name][2])
