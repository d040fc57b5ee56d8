"""Saturated proposal-head inputs shared by tests/test_oracle_head_edges.py (CPU), tests/test_gpu_head_edges.py (GPU) and
tests/golden/make_head_edges_golden.py: head outputs of a network that has collapsed onto one component. Numpy only and
deterministic; every number is fp32-representable, so the float64 oracle, the fp32 reference and the device read the same
inputs.

A case is a dict {name, head, kind, K (components) or C (categories), y [n, n_out], value [n], prior [n, 2], tag [n]}:
  head    'Normal' | 'Uniform' | 'Poisson' | 'Categorical' | 'Bernoulli'; kind is the pp_head_logprob kind (0..4)
  prior   (mean, stddev) for Normal, (low, high) for Uniform, (0, 40) for Poisson, (n, n1) for Bernoulli (the sub-batch
          step's size and its number of ones, oracle.ic_oracle.head_bernoulli), zeros for Categorical
  tag     what the row's value is: see VALUE_TAGS

Weights. Mixture and categorical logits are a row maximum plus fixed gaps (0, -3, -10, -12, -14, -18, -25, -40; never -16) and
a jitter of at most 0.1, so that every normalised weight p keeps a factor 2 from both clamp thresholds of
util.clamp_probs, eps = 2^-23 and 1 - eps: p <= eps / 2 or p >= 2 eps, and 1 - p <= eps / 2 or 1 - p >= 2 eps
(weight_margin; asserted for every case by head_edge_cases). fp32 and float64 then agree on which weights are clamped and no
row has to be left out. The Bernoulli probabilities sigmoid(y) + 1e-8 keep the same factor.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)
KIND = {'Normal': 0, 'Uniform': 1, 'Categorical': 2, 'Poisson': 3, 'Bernoulli': 4}
POISSON_LOW, POISSON_HIGH = 0.0, 40.0

VALUE_TAGS = ('lead_mean',    # exactly at the leading component's mean (as fp32 computes it from the fp32 inputs)
              'near',         # within two scales of the leading component
              'other_mean',   # at another component's mean
              'ordinary',     # a plain draw: prior sample (Normal), uniform in the support, a count
              'low', 'high',  # exactly on a bound of the support (inside for TruncatedNormal)
              'below', 'above',   # one fp32 step outside a bound: -inf, rescued (loss term -log(1e-8), dy exactly 0)
              'tt1000',       # |value - mean| / scale near 1000 for the leading component
              'count0', 'count40',          # Poisson counts on the bounds
              'cat_first', 'cat_last', 'cat_lead', 'cat_clamped',   # Categorical values
              'n1_zero', 'n1_all', 'n1_between')                    # Bernoulli (n, n1)

# gaps to the row maximum; the first entry is the leading weight. Names say which clamp branches the pattern runs.
WEIGHTS = {
    1: [('single', [0.0])],                                             # p = 1: above 1 - eps
    2: [('inside', [0.0, -3.0]), ('inside_far', [0.0, -14.0]), ('lead_above_rest_below', [0.0, -25.0]),
        ('tie', [0.0, 0.0])],
    3: [('inside', [0.0, -3.0, -10.0]), ('lead_above_rest_below', [0.0, -18.0, -25.0]),
        ('one_below', [0.0, -14.0, -40.0]), ('tie_one_below', [0.0, 0.0, -25.0]), ('inside_one_below', [0.0, -3.0, -18.0]),
        ('lead_above_far', [0.0, -40.0, -40.0])],
    7: [('inside', [0.0, -3.0, -10.0, -3.0, -10.0, -14.0, -10.0]),
        ('many_below', [0.0, -14.0, -18.0, -25.0, -40.0, -25.0, -40.0]),
        ('tie_rest_below', [0.0, 0.0, -25.0, -25.0, -40.0, -40.0, -40.0]),
        ('inside_some_below', [0.0, -3.0, -25.0, -10.0, -40.0, -14.0, -18.0])],
    16: [('inside', [0.0, -3.0, -10.0, -14.0] + [-3.0, -10.0, -12.0] * 4),
         ('lead_above_rest_below', [0.0] + [-25.0, -40.0, -40.0] * 5),
         ('lead_above_one_near', [0.0, -18.0] + [-40.0] * 14),
         ('many_below', [0.0, -3.0, -10.0, -14.0] + [-25.0, -40.0] * 6),
         ('tie_rest_below', [0.0, 0.0, 0.0, -12.0] + [-40.0, -25.0, -40.0] * 4)],
    33: [('inside', [0.0, -14.0] + [-3.0, -10.0, -12.0, -10.0] * 7 + [-10.0, -12.0, -10.0]),
         ('many_below', [0.0, -3.0, -14.0] + [-25.0, -40.0, -18.0] * 10),
         ('lead_rest_below', [0.0] + [-40.0, -25.0] * 16)],
}

# raw outputs of the mean and scale layers (fp32-exact). The last entries saturate the transforms.
YMU = {'Normal': [0.0, 0.5, -1.0, 2.5, -5.0, 12.0, -30.0, 30.0],
       'Uniform': [0.0, 1.0, -2.0, 5.0, -8.0, 13.0, -20.0, 20.0],
       'Poisson': [0.0, 1.0, -2.0, 5.0, -8.0, 13.0, -20.0, 20.0]}
YSD = {'Normal': [0.0, 1.0, -2.0, 4.0, -6.0, 9.0, -12.0, 12.0],
       'Uniform': [0.0, 1.0, -3.0, 6.0, -8.0, 13.0, -20.0, 20.0],
       'Poisson': [0.0, 1.0, -1.0, 2.5, -4.0, 5.5, -8.0, 8.0]}
MIX_VALUES = {'Normal': ['lead_mean', 'near', 'other_mean', 'ordinary', 'near'],
              'Uniform': ['lead_mean', 'near', 'other_mean', 'ordinary', 'low', 'high', 'below', 'above'],
              'Poisson': ['lead_mean', 'near', 'other_mean', 'ordinary', 'count0', 'count40', 'below', 'above']}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def component_params(head, y, prior, K):
    """means and scales [n, K] of the mixture components in float64 (the reference's formulas)."""
    ymu, ysd = y[:, :K], y[:, K:2 * K]
    pa, pb = prior[:, 0:1], prior[:, 1:2]
    if head == 'Normal':
        return pa + ymu * pb, np.exp(ysd) * pb
    rng = pb - pa
    mu = pa + sigmoid(ymu) * rng
    return mu, (np.exp(ysd) if head == 'Poisson' else rng / 1000 + sigmoid(ysd) * rng * 10)


def weights(case):
    """The normalised probabilities that the clamp sees, float64: [n, K] / [n, C] / [n, 1]."""
    y, head = case['y'], case['head']
    if head == 'Bernoulli':
        return sigmoid(y) + 1e-8
    z = y if head == 'Categorical' else y[:, 2 * case['K']:]
    e = np.exp(z - z.max(1, keepdims=True))
    pi = e / e.sum(1, keepdims=True)
    if head == 'Categorical':
        pi = pi + 1e-8
    return pi / pi.sum(1, keepdims=True)


def weight_margin(p):
    """Smallest factor between a probability (or its complement) and the clamp thresholds eps / 1 - eps."""
    q = 1.0 - p
    with np.errstate(divide='ignore'):
        lo = np.maximum(p / EPS, EPS / p)
        hi = np.maximum(q / EPS, np.where(q > 0, EPS / np.where(q > 0, q, 1.0), np.inf))
    return float(min(lo.min(), hi.min()))


def clamp_masks(p):
    """(below eps, above 1 - eps) in float64 - what both precisions must agree on."""
    return p < EPS, p > 1.0 - EPS


def _logits(rng, n, width, patterns):
    """[n, width] logits: pattern i % len(patterns), rotated so that the leading weight moves through the columns, on a
    per-row offset (softmax is shift invariant; the kernels subtract the row maximum) with a small jitter."""
    z = np.zeros((n, width))
    lead = np.zeros(n, np.int64)
    names = []
    for i in range(n):
        name, gaps = patterns[i % len(patterns)]
        shift = (i // len(patterns)) % width
        z[i] = np.roll(np.asarray(gaps), shift)
        lead[i] = shift
        names.append(name)
    z += rng.uniform(-0.1, 0.1, z.shape)
    z[np.arange(n), lead] += 0.1            # the first entry of the pattern stays the row maximum (ties: within 0.2)
    z += rng.choice([-5.0, 0.0, 7.0], n)[:, None]
    return f32(z), lead, names


def _mixture_case(head, K, seed, tt1000=False, ordinary=False):
    rng = np.random.default_rng(seed)
    tags = ['tt1000'] if tt1000 else MIX_VALUES[head]
    pats = WEIGHTS[K]
    n = 100 if tt1000 else max(240, len(pats) * len(tags) * 7)
    z, lead, wnames = _logits(rng, n, K, pats)
    if ordinary:                                    # y ~ N(0, 1): what the suite tested before, for kinds 3 and 4
        ymu, ysd, z = f32(rng.normal(0, 1, (n, K))), f32(rng.normal(0, 1, (n, K))), f32(rng.normal(0, 1, (n, K)))
        lead = z.argmax(1)
    else:
        ymu = f32(rng.choice(YMU[head], (n, K)) + rng.uniform(-0.25, 0.25, (n, K)))
        ysd = f32(rng.choice(YSD[head], (n, K)) + rng.uniform(-0.25, 0.25, (n, K)))
        # the saturated entries exactly, in the leading component of every other row: the mean on an edge of the support
        # with the scale on its floor / ceiling is the corner the transforms' gradients vanish in
        for i in range(0, n, 2):
            ymu[i, lead[i]] = YMU[head][-1 - (i // 2) % 2]
            ysd[i, lead[i]] = YSD[head][-1 - (i // 4) % 2]
    if head == 'Normal':
        prior = np.stack([rng.choice([-3.0, 0.0, 0.75, 10.0], n), rng.choice([0.5, 1.0, 3.0], n)], 1)
    elif head == 'Uniform':
        low = rng.choice([-3.0, 0.25, 1.5], n)
        prior = np.stack([low, low + rng.choice([0.5, 1.0, 4.0], n)], 1)
    else:
        prior = np.tile([POISSON_LOW, POISSON_HIGH], (n, 1))
    row = np.arange(n)
    if not ordinary:
        # The components that a row's value is placed at (the leading one and its neighbour, 'other_mean') keep a scale
        # that fp32 can resolve at their mean: tt = (v - mu) / sd carries the rounding of mu, ulp(mu) / sd, and below these
        # floors the reference's own fp32 log_prob is off by more than 1e-2 (tests/test_oracle_head_edges.py keeps that
        # cap). Normal: ysd >= -6, and a scale below a tenth of the prior's only around |mean| <= 3 + 2.5 stddev;
        # The other components keep the whole range.
        for j in (lead, (lead + 1) % K):
            if head == 'Normal':
                ysd[row, j] = np.maximum(ysd[row, j], -6.0)
                narrow = ysd[row, j] < -2.3
                ymu[row, j] = np.where(narrow, np.clip(ymu[row, j], -2.5, 2.5), ymu[row, j])
                prior[:, 0] = np.where(narrow, np.clip(prior[:, 0], -3.0, 3.0), prior[:, 0])
        if head == 'Poisson':
            # every component: the means pile up on the upper edge (sigmoid saturated), where a count of 40 sits at the
            # mean of all of them at once; ulp(40) / exp(-8) = 1e-2. Scales below exp(-4) only next to the lower edge.
            ysd = np.where(ymu > -4.5, np.maximum(ysd, -4.0), ysd)
    y = np.concatenate([ymu, ysd, z], 1)
    if tt1000:
        # leading component: mean on the lower edge with a small scale, value at 1000 scales from it
        if head == 'Normal':
            ysd[row, lead] = f32(rng.uniform(-3, 1, n))
        else:
            ymu[row, lead] = -20.0
            ysd[row, lead] = -20.0 if head == 'Uniform' else f32(np.log(0.04) + rng.uniform(-0.01, 0, n))
        y = np.concatenate([ymu, ysd, z], 1)
    mu, sd = component_params(head, y, prior, K)
    # the component means as fp32 arithmetic gives them (what 'at a component mean' means to a kernel)
    mu32 = f32(mu)
    low, high = prior[:, 0], prior[:, 1]
    value = np.zeros(n)
    tag = []
    for i in range(n):
        t = tags[(i // len(pats)) % len(tags)]
        j = lead[i]
        if t == 'lead_mean':
            v = mu32[i, j]
        elif t == 'near':
            v = mu[i, j] + rng.uniform(-2, 2) * sd[i, j]
        elif t == 'other_mean':
            v = mu32[i, (j + 1) % K]
        elif t == 'ordinary':
            v = (low[i] + high[i] * rng.normal() if head == 'Normal' else
                 float(rng.integers(1, 40)) if head == 'Poisson' else rng.uniform(low[i], high[i]))
        elif t in ('low', 'count0'):
            v = low[i]
        elif t in ('high', 'count40'):
            v = high[i]
        elif t == 'below':
            v = np.nextafter(np.float32(low[i]), np.float32(-np.inf)) if head == 'Uniform' else -1.0
        elif t == 'above':
            v = np.nextafter(np.float32(high[i]), np.float32(np.inf))
        else:   # tt1000
            v = mu[i, j] + 1000.0 * sd[i, j] * (1.0 if head != 'Normal' else rng.choice([-1.0, 1.0]))
        if head != 'Normal' and t in ('lead_mean', 'near', 'other_mean', 'tt1000'):
            v = min(max(v, low[i]), high[i])         # stays inside the support; 'below' / 'above' are the outside rows
        value[i] = v
        tag.append(t)
    name = '%s_K%d%s' % (head.lower(), K, '_tt1000' if tt1000 else '_ordinary' if ordinary else '')
    return {'name': name, 'head': head, 'kind': KIND[head], 'K': K, 'y': y, 'value': f32(value), 'prior': f32(prior),
            'tag': np.asarray(tag), 'weights': np.asarray(wnames if not ordinary else ['ordinary'] * n)}


def _categorical_case(C, seed):
    rng = np.random.default_rng(seed)
    pats = WEIGHTS[C]
    tags = ['cat_first', 'cat_last', 'cat_lead', 'cat_clamped']
    n = 240
    y, lead, wnames = _logits(rng, n, C, pats)
    value = np.zeros(n)
    tag = []
    for i in range(n):
        t = tags[(i // len(pats)) % len(tags)]
        value[i] = {'cat_first': 0, 'cat_last': C - 1, 'cat_lead': lead[i], 'cat_clamped': int(y[i].argmin())}[t]
        tag.append(t)
    return {'name': 'categorical_C%d' % C, 'head': 'Categorical', 'kind': 2, 'C': C, 'y': y, 'value': value,
            'prior': np.zeros((n, 2)), 'tag': np.asarray(tag), 'weights': np.asarray(wnames)}


def _bernoulli_case(seed, ordinary=False):
    rng = np.random.default_rng(seed)
    n = 234
    if ordinary:
        y = f32(rng.normal(0, 1, (n, 1)))
    else:
        # y = -14: inside with p ~ 1e-6; |y| >= 20: sigmoid(y) + 1e-8 clamped below eps / above 1 - eps. No y in (10.2, 20):
        # there 1 - p is a few fp32 steps of 1 and the reference's own fp32 log(1 - p) is off by percents.
        base = np.asarray([0.0, 1.0, -1.0, 3.0, -3.0, 10.0, -10.0, 6.0, -14.0, 20.0, -20.0, 30.0, -30.0])
        y = f32(base[np.arange(n) % len(base)] + rng.uniform(-0.2, 0.2, n))[:, None]
    cnt = np.asarray([1.0, 5.0, 64.0])[(np.arange(n) // 13) % 3]
    tags = np.asarray(['n1_zero', 'n1_all', 'n1_between'])[(np.arange(n) // 39) % 3]
    ones = np.where(tags == 'n1_zero', 0.0, np.where(tags == 'n1_all', cnt, np.floor(cnt / 2)))
    # value: the row's own Bernoulli outcome is not an input of the row sum (oracle.ic_oracle.head_bernoulli); recorded as 0
    return {'name': 'bernoulli_ordinary' if ordinary else 'bernoulli_edges', 'head': 'Bernoulli', 'kind': 4, 'C': 1, 'y': y,
            'value': np.zeros(n), 'prior': np.stack([cnt, ones], 1), 'tag': tags,
            'weights': np.asarray(['ordinary' if ordinary else 'edges'] * n)}


_CASES = None


def head_edge_cases():
    """All cases by name, built once. Asserts the factor 2 between every weight and the clamp thresholds."""
    global _CASES
    if _CASES is None:
        cases = []
        for h, head in enumerate(('Normal', 'Uniform', 'Poisson')):
            for K in (1, 3, 16):
                cases.append(_mixture_case(head, K, 1000 + 100 * h + K))
            cases.append(_mixture_case(head, 3, 2000 + h, tt1000=True))
        cases.append(_mixture_case('Poisson', 3, 3000, ordinary=True))
        for C in (2, 7, 33):
            cases.append(_categorical_case(C, 4000 + C))
        cases.append(_bernoulli_case(5000))
        cases.append(_bernoulli_case(5001, ordinary=True))
        for c in cases:
            for k in ('y', 'value', 'prior'):
                assert np.array_equal(c[k], f32(c[k])), (c['name'], k)
            assert weight_margin(weights(c)) >= 2.0, (c['name'], weight_margin(weights(c)))
            assert 100 <= c['y'].shape[0] <= 1000
        _CASES = {c['name']: c for c in cases}
    return _CASES


def blocks(case):
    """Output blocks of dy: name -> column slice."""
    if case['head'] in ('Categorical', 'Bernoulli'):
        return {'logits': slice(0, case['y'].shape[1])}
    K = case['K']
    return {'mean': slice(0, K), 'scale': slice(K, 2 * K), 'logits': slice(2 * K, 3 * K)}


def lp_error(got, ref):
    """|got - ref| / max(1, |ref|) over the rows where ref is finite; the -inf pattern must be equal."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), 'the -inf (rescued) rows differ'
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all(), 'non-finite log_prob on a row whose float64 log_prob is finite'
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max())


def dy_errors(case, got, ref):
    """Per output block: max |got - ref| / the block's largest |ref| of the case (0 where the block is all zero and equal)."""
    out = {}
    for name, sl in blocks(case).items():
        g, r = np.asarray(got, np.float64)[:, sl], np.asarray(ref, np.float64)[:, sl]
        assert np.isfinite(g).all(), (case['name'], name, 'non-finite gradient')
        scale = np.abs(r).max()
        err = np.abs(g - r).max()
        out[name] = float(err / scale) if scale > 0 else float(err)
    return out


def oracle_head(case, y=None, value=None, prior=None):
    """oracle.ic_oracle's head on the case (or on replaced inputs): lp [n] with -inf on rescued rows, dy [n, n_out] with
    exact zeros there."""
    from oracle import ic_oracle as O
    y = case['y'] if y is None else np.asarray(y, np.float64)
    value = case['value'] if value is None else np.asarray(value, np.float64)
    prior = case['prior'] if prior is None else np.asarray(prior, np.float64)
    head = case['head']
    with np.errstate(all='ignore'):
        if head == 'Normal':
            lp, dy, _ = O.head_normal_mixture(y, prior, value, case['K'])
        elif head == 'Uniform':
            lp, dy, _ = O.head_truncated_normal_mixture(y, prior, value, case['K'])
        elif head == 'Poisson':
            lp, dy, _ = O.head_poisson_truncated_normal_mixture(y, value, case['K'])
        elif head == 'Categorical':
            lp, dy, _ = O.head_categorical(y, value)
        else:
            cnt, ones = prior[:, 0], prior[:, 1]
            lp, dy = np.zeros(len(y)), np.zeros_like(y)
            for c, o in sorted({(float(a), float(b)) for a, b in prior}):
                rows = np.nonzero((cnt == c) & (ones == o))[0]
                vals = np.zeros(int(c))
                vals[:int(o)] = 1.0
                lp[rows], dy[rows], _ = O.head_bernoulli(y[rows], vals)
    return lp, np.where(np.isneginf(lp)[:, None], 0.0, dy)
