"""Priors / likelihoods of the host-side trace runtime. The weighted-sample container Empirical lives in empirical.py (its batch
calls in empirical_batch.py) and is re-exported at the end of this file.

Mirrors the slice of pyprob.distributions that the hot path touches (pyprob/distributions/{distribution,normal,
uniform,categorical,empirical}.py): thin objects carrying `name`, parameters, `sample()` and
`log_prob(value, sum=False)`. They are evaluated on the host like in the reference; the
proposal distributions themselves (Mixture / TruncatedNormal) live in the HIP kernels.
"""
import copy
import math

import torch


# pp_dist kinds of the families beyond the five the inference network proposes for (include/pyprob_amd.h, ABI 15), and the
# attributes their parameters are read from, in p0..p3 order (pyprob/distributions/<family>.py)
DIST_KINDS = {'Factor': 2, 'Exponential': 6, 'Gamma': 7, 'Beta': 8, 'LogNormal': 9, 'Weibull': 10, 'Binomial': 11, 'VonMises': 12,
              'TruncatedNormal': 13}
DIST_PARAMS = {'Exponential': ('rate',), 'Gamma': ('concentration', 'rate'),
               'Beta': ('concentration1', 'concentration0', 'low', 'high'), 'LogNormal': ('loc', 'scale'),
               'Weibull': ('scale', 'concentration'), 'Binomial': ('total_count', 'logits'), 'VonMises': ('loc', 'concentration'),
               'TruncatedNormal': ('mean_non_truncated', 'stddev_non_truncated', 'low', 'high')}


def _t(x):
    return x if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float32)


class Distribution:
    def __init__(self, name, address_suffix, torch_dist=None):
        self.name = name
        self._address_suffix = address_suffix
        self._td = torch_dist

    # The torch.distributions object behind a prior is built on first use: constructing one costs ~45 us of host time
    # (parameter broadcasting), and a particle of an importance-sampling run with the inference network never asks its
    # priors for samples or log-probs - the device does (measured: a fifth of a coroutine worker's time).
    @property
    def _torch_dist(self):
        if self._td is None:
            self._td = self._make_torch_dist()
        return self._td

    def _make_torch_dist(self):
        raise NotImplementedError

    def sample(self):
        return self._torch_dist.sample()

    def log_prob(self, value, sum=False):
        lp = self._torch_dist.log_prob(_t(value).to(self._device()))
        return torch.sum(lp) if sum else lp

    def _device(self):
        return torch.device('cpu')

    @property
    def mean(self):
        return self._torch_dist.mean

    @property
    def variance(self):
        return self._torch_dist.variance

    @property
    def stddev(self):
        return self.variance.sqrt()


class Normal(Distribution):
    """pyprob/distributions/normal.py:7-31"""

    def __init__(self, loc, scale):
        # A state.ParticleTensor (per-particle value of a lock-step run) pays a Python __torch_function__ round trip for EVERY
        # torch call and attribute read (~4 us each; a posterior call builds two of these objects per statement): the
        # constructor only looks at metadata, so it runs with the subclass dispatch off, and a float32 tensor is taken as it is.
        with torch._C.DisableTorchFunctionSubclass():
            if not (torch.is_tensor(loc) and loc.dtype == torch.float32):
                loc = _t(loc).float()
            if not (torch.is_tensor(scale) and scale.dtype == torch.float32):
                scale = _t(scale).float()
            if scale.device != loc.device and not (scale.numel() == 1 and scale.device.type == 'cpu'):
                scale = scale.to(loc.device)      # (a host scalar next to device locations stays where it is: the device kernels
                                                  #  take it as a cached constant, and a posterior call pays no copy for it)
            if scale.numel() == 1 and scale.device.type == 'cpu' and not float(scale) > 0.0:   # (what torch's validation rejects)
                raise ValueError('Normal: the scale must be positive, got {}'.format(float(scale)))
            # per-particle parameters are handed out as they are (see _raw_params)
            self._raw = loc.shape == scale.shape or type(loc).__name__ == 'ParticleTensor' or type(scale).__name__ == 'ParticleTensor'
        self._loc, self._scale = loc, scale
        super().__init__('Normal', 'Normal')

    def _make_torch_dist(self):
        # per-particle parameters of a lock-step run may hold stale (even NaN) entries for particles that are not on the
        # current control-flow path: no argument validation for vectors
        scale = self._scale if self._scale.device == self._loc.device else self._scale.to(self._loc.device)
        return torch.distributions.Normal(self._loc, scale, validate_args=None if self._loc.numel() == 1 else False)

    def _device(self):
        return self._loc.device

    def _raw_params(self):
        # per-particle parameters of a lock-step run (state.ParticleTensor) are handed out as they are: building the
        # torch.distributions object would broadcast - i.e. READ - a value whose draw may still be deferred
        return self._td is None and getattr(self, '_raw', False)

    @property
    def mean(self):
        return self._loc if self._raw_params() else self._torch_dist.mean

    @property
    def stddev(self):
        return self._scale if self._raw_params() else self._torch_dist.stddev

    @property
    def variance(self):
        return self.stddev ** 2

    def __repr__(self):
        return 'Normal({}, {})'.format(self.mean.tolist(), self.stddev.tolist())


class Uniform(Distribution):
    """pyprob/distributions/uniform.py:7-25"""

    def __init__(self, low, high):
        self._low, self._high = _t(low).float(), _t(high).float()
        super().__init__('Uniform', 'Uniform')

    def _make_torch_dist(self):
        return torch.distributions.Uniform(self._low, self._high, validate_args=False)

    def _device(self):
        return self._low.device

    @property
    def low(self):
        return self._low if self._td is None and self._low.shape == self._high.shape else self._torch_dist.low

    @property
    def high(self):
        return self._high if self._td is None and self._low.shape == self._high.shape else self._torch_dist.high


class Poisson(Distribution):
    """pyprob/distributions/poisson.py:7-21. The inference network proposes a continuous TruncatedNormal mixture on
    [0, 40] for a Poisson variable (proposal_poisson_truncated_normal_mixture.py), so log_prob must accept non-integer
    values like the reference's torch did: no argument validation."""

    def __init__(self, rate):
        rate = _t(rate).float()
        super().__init__('Poisson', 'Poisson', torch.distributions.Poisson(rate, validate_args=False))

    @property
    def rate(self):
        return self._torch_dist.mean


class Categorical(Distribution):
    """pyprob/distributions/categorical.py:7-39"""

    def __init__(self, probs):
        probs = _t(probs).float()
        if probs.dim() == 0:
            raise ValueError('probs cannot be a scalar.')
        td = torch.distributions.Categorical(probs=probs)
        self._probs = td.probs
        self._num_categories = self._probs.size(-1)
        super().__init__('Categorical', 'Categorical(len_probs:{})'.format(self._num_categories), td)

    @property
    def num_categories(self):
        return self._num_categories

    @property
    def probs(self):
        return self._probs


class Bernoulli(Distribution):
    """pyprob/distributions/bernoulli.py"""

    def __init__(self, probs):
        probs = _t(probs).float()
        super().__init__('Bernoulli', 'Bernoulli', torch.distributions.Bernoulli(probs=probs, validate_args=False))

    @property
    def probs(self):
        return self._torch_dist.probs


class _Family(Distribution):
    """A family whose parameters are kept as they were given (float32 tensors; per-particle ParticleTensors of a lock-step run
    are not broadcast or validated: stale entries of particles off the current path may be anything). log_prob is torch's,
    with -inf outside the support like the device kernels (pp_dist_logweight)."""
    _params = ()

    def __init__(self, name, address_suffix, *params):
        with torch._C.DisableTorchFunctionSubclass():
            self._p = tuple(v if (torch.is_tensor(v) and v.dtype == torch.float32) else _t(v).float() for v in params)
        super().__init__(name, address_suffix)

    def _device(self):
        return self._p[0].device

    def _in_support(self, value):
        return torch.ones_like(value, dtype=torch.bool)

    def log_prob(self, value, sum=False):
        value = _t(value).float().to(self._device())
        lp = self._torch_dist.log_prob(value)
        lp = torch.where(self._in_support(value), lp, torch.full_like(lp, float('-inf')))
        return torch.sum(lp) if sum else lp

    def __repr__(self):
        return '{}({})'.format(self.name, ', '.join('{}={}'.format(n, p.tolist()) for n, p in zip(self._params, self._p)))


class Exponential(_Family):
    """pyprob/distributions/exponential.py"""
    _params = ('rate',)

    def __init__(self, rate):
        super().__init__('Exponential', 'Exponential', rate)

    def _make_torch_dist(self):
        return torch.distributions.Exponential(self._p[0], validate_args=False)

    def _in_support(self, value):
        return value >= 0

    @property
    def rate(self):
        return self._p[0]


class Gamma(_Family):
    """pyprob/distributions/gamma.py"""
    _params = ('concentration', 'rate')

    def __init__(self, concentration, rate):
        super().__init__('Gamma', 'Gamma', concentration, rate)

    def _make_torch_dist(self):
        return torch.distributions.Gamma(self._p[0], self._p[1], validate_args=False)

    def _in_support(self, value):
        return value >= 0

    @property
    def concentration(self):
        return self._p[0]

    @property
    def rate(self):
        return self._p[1]


class Beta(_Family):
    """pyprob/distributions/beta.py: Beta(concentration1, concentration0) stretched onto [low, high]. log_prob is that of
    the unit-interval Beta at (x - low) / (high - low), without the -log(high - low) Jacobian, as pyprob computes it."""
    _params = ('concentration1', 'concentration0', 'low', 'high')

    def __init__(self, concentration1, concentration0, low=0, high=1):
        super().__init__('Beta', 'Beta', concentration1, concentration0, low, high)

    def _make_torch_dist(self):
        return torch.distributions.Beta(self._p[0], self._p[1], validate_args=False)

    def _unit(self, value):
        return (value - self._p[2]) / (self._p[3] - self._p[2])

    def _in_support(self, value):
        y = self._unit(value)
        return (y >= 0) & (y <= 1)

    def log_prob(self, value, sum=False):
        value = _t(value).float().to(self._device())
        y = self._unit(value)
        lp = self._torch_dist.log_prob(y)
        lp = torch.where((y >= 0) & (y <= 1), lp, torch.full_like(lp, float('-inf')))
        return torch.sum(lp) if sum else lp

    def sample(self):
        return self._p[2] + self._torch_dist.sample() * (self._p[3] - self._p[2])

    @property
    def concentration1(self):
        return self._p[0]

    @property
    def concentration0(self):
        return self._p[1]

    @property
    def low(self):
        return self._p[2]

    @property
    def high(self):
        return self._p[3]

    @property
    def mean(self):
        return self._p[2] + self._torch_dist.mean * (self._p[3] - self._p[2])

    @property
    def variance(self):
        r = self._p[3] - self._p[2]
        return self._torch_dist.variance * r * r


class LogNormal(_Family):
    """pyprob/distributions/log_normal.py"""
    _params = ('loc', 'scale')

    def __init__(self, loc, scale):
        super().__init__('LogNormal', 'LogNormal', loc, scale)

    def _make_torch_dist(self):
        return torch.distributions.LogNormal(self._p[0], self._p[1], validate_args=False)

    def _in_support(self, value):
        return value > 0

    @property
    def loc(self):
        return self._p[0]

    @property
    def scale(self):
        return self._p[1]


class Weibull(_Family):
    """pyprob/distributions/weibull.py"""
    _params = ('scale', 'concentration')

    def __init__(self, scale, concentration):
        super().__init__('Weibull', 'Weibull', scale, concentration)

    def _make_torch_dist(self):
        return torch.distributions.Weibull(self._p[0], self._p[1], validate_args=False)

    def _in_support(self, value):
        return value > 0

    def log_prob(self, value, sum=False):
        """log k - log l + (k - 1) log z - z^k with z^k = exp(k log z), z = x / l: lp_weibull of csrc/dist_math.hpp. torch's
        transform chain takes z^k first and the Jacobian's log of it afterwards: -inf where z^k underflows (Weibull(1, 50) at 1e-6),
        NaN where it overflows."""
        l, k = self._p
        value = _t(value).float().to(self._device())
        lz = torch.log(value / l)
        lp = torch.log(k) - torch.log(l) + (k - 1) * lz - torch.exp(k * lz)
        lp = torch.where(value > 0, lp, torch.full_like(lp, float('-inf')))
        return torch.sum(lp) if sum else lp

    @property
    def scale(self):
        return self._p[0]

    @property
    def concentration(self):
        return self._p[1]


class Binomial(_Family):
    """pyprob/distributions/binomial.py: total_count with probs or logits; the log-density is torch's, from the logits."""
    _params = ('total_count', 'logits')

    def __init__(self, total_count=1, probs=None, logits=None):
        if (probs is None) == (logits is None):
            raise ValueError('Either `probs` or `logits` must be specified, but not both.')
        if logits is None:
            with torch._C.DisableTorchFunctionSubclass():
                p = _t(probs).float()
                eps = torch.finfo(torch.float32).eps
                pc = p.clamp(eps, 1 - eps)
                logits = torch.log(pc) - torch.log1p(-pc)         # torch's probs_to_logits (is_binary)
        self._probs = None if probs is None else _t(probs).float()
        super().__init__('Binomial', 'Binomial', total_count, logits)

    def _make_torch_dist(self):
        return torch.distributions.Binomial(total_count=self._p[0], logits=self._p[1], validate_args=False)

    def _in_support(self, value):
        return (value >= 0) & (value <= self._p[0]) & (value == torch.floor(value))

    @property
    def total_count(self):
        return self._p[0]

    @property
    def logits(self):
        return self._p[1]

    @property
    def probs(self):
        return self._probs if self._probs is not None else torch.sigmoid(self._p[1])


class VonMises(_Family):
    """pyprob/distributions/von_mises.py"""
    _params = ('loc', 'concentration')

    def __init__(self, loc, concentration):
        super().__init__('VonMises', 'VonMises', loc, concentration)

    def _make_torch_dist(self):
        return torch.distributions.VonMises(self._p[0], self._p[1], validate_args=False)

    def _in_support(self, value):
        return torch.isfinite(value)

    @property
    def loc(self):
        return self._p[0]

    @property
    def concentration(self):
        return self._p[1]


def _std_cdf(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2)))


class TruncatedNormal(_Family):
    """pyprob/distributions/truncated_normal.py: a Normal restricted to [low, high]; log_prob scores the closed interval
    (:40-45), sample draws by the inverse CDF between Phi(alpha) and Phi(beta) (:94-112). clamp_mean_between_low_high
    moves the mean into [low, high] at construction, as pyprob does."""
    _params = ('mean_non_truncated', 'stddev_non_truncated', 'low', 'high')

    def __init__(self, mean_non_truncated, stddev_non_truncated, low, high, clamp_mean_between_low_high=False):
        super().__init__('TruncatedNormal', 'TruncatedNormal', mean_non_truncated, stddev_non_truncated, low, high)
        if clamp_mean_between_low_high:
            with torch._C.DisableTorchFunctionSubclass():
                m = torch.max(torch.min(self._p[0], self._p[3]), self._p[2])
            self._p = (m,) + self._p[1:]

    def _ab(self):
        mu, sd, low, high = self._p
        return (low - mu) / sd, (high - mu) / sd

    def _tail(self, tail_from):
        """(upper, lower, ta, tb, log Z + ta^2 / 2): where the whole interval lies beyond tail_from standard deviations on one side
        (alpha >= tail_from / beta <= -tail_from) the mass Z is taken in that tail's own coordinates [ta, tb] as
        Q(ta) - Q(tb), Q(t) = erfcx(t / sqrt 2) exp(-t^2 / 2) / 2, with exp(-ta^2 / 2) left out - lp_truncnormal of
        csrc/dist_math.hpp. The fp32 difference of two 0.5 (1 + erf) is 0 from 5.5 sigma on. (Elements outside the tails carry
        placeholders.)"""
        a, b = self._ab()
        upper, lower = a >= tail_from, b <= -tail_from
        tail = upper | lower
        ta = torch.where(tail, torch.where(upper, a, -b), torch.full_like(a, tail_from))
        tb = torch.where(tail, torch.where(upper, b, -a), torch.full_like(a, tail_from + 1))
        ea, eb = torch.special.erfcx(ta / math.sqrt(2)), torch.special.erfcx(tb / math.sqrt(2))
        ratio = torch.exp(-0.5 * ((tb - ta) * (tb + ta))) * (eb / ea)
        return upper, lower, ta, tb, torch.log(0.5 * ea) + torch.log1p(-ratio)

    TAIL_FROM = 3.0             # log_prob: kTruncTailFrom of csrc/dist_math.hpp
    MOMENTS_TAIL_FROM = 4.0     # _Z (mean, variance): the reference's own fp32 Z up to where the device sampler turns to Robert's tail
                                # sampler - the reference's fp32 mean / stddev of a row such as (5, 1, 0, 2) are reproduced to 1e-5

    def _Z(self):
        a, b = self._ab()
        upper, lower, ta, _, lz = self._tail(self.MOMENTS_TAIL_FROM)
        return torch.where(upper | lower, torch.exp(lz - 0.5 * ta * ta), _std_cdf(b) - _std_cdf(a))

    def log_prob(self, value, sum=False):
        mu, sd, low, high = self._p
        value = _t(value).float().to(self._device())
        z = (value - mu) / sd
        a, b = self._ab()
        lp = -(z * z) / 2 - 0.5 * math.log(2 * math.pi) - torch.log(sd * (_std_cdf(b) - _std_cdf(a)))
        upper, lower, ta, _, lz = self._tail(self.TAIL_FROM)
        zt = torch.where(lower, -z, z)
        lp = torch.where(upper | lower, -0.5 * ((zt - ta) * (zt + ta)) - 0.5 * math.log(2 * math.pi) - torch.log(sd) - lz, lp)
        lp = torch.where((value >= low) & (value <= high), lp, torch.full_like(lp, float('-inf')))
        return torch.sum(lp) if sum else lp

    def sample(self):
        """The inverse CDF between Phi(alpha) and Phi(beta) in float64 on the parameters' device (torch.special.ndtr / ndtri keep
        the tails that 2 p - 1 in fp32 loses); an element that rounds outside [low, high] is redrawn, the others are kept."""
        mu, sd, low, high = (t.double() for t in self._p)
        shape = torch.broadcast_shapes(mu.shape, sd.shape, low.shape, high.shape)
        mu, sd, low, high = (t.expand(shape) for t in (mu, sd, low, high))
        ca, cb = torch.special.ndtr((low - mu) / sd), torch.special.ndtr((high - mu) / sd)
        out = torch.full(shape, float('nan'), dtype=torch.float64, device=mu.device)
        todo = torch.ones(shape, dtype=torch.bool, device=mu.device)
        for _ in range(64):
            u = torch.rand(shape, dtype=torch.float64, device=mu.device)
            v = (torch.special.ndtri(ca + u * (cb - ca)) * sd + mu).float().double()
            ok = todo & (v >= low) & (v <= high)
            out = torch.where(ok, v, out)
            todo = todo & ~ok
            if not bool(todo.any()):
                return out.float()
        raise RuntimeError('TruncatedNormal.sample: no draw inside [low, high]')

    @property
    def mean_non_truncated(self):
        return self._p[0]

    @property
    def stddev_non_truncated(self):
        return self._p[1]

    @property
    def low(self):
        return self._p[2]

    @property
    def high(self):
        return self._p[3]

    def _pdf_ab(self):
        a, b = self._ab()
        c = 1 / math.sqrt(2 * math.pi)
        return a, b, c * torch.exp(-0.5 * a * a), c * torch.exp(-0.5 * b * b)

    @property
    def mean(self):
        a, b, pa, pb = self._pdf_ab()
        return self._p[0] + self._p[1] * (pa - pb) / self._Z()

    @property
    def variance(self):
        a, b, pa, pb = self._pdf_ab()
        Z = self._Z()
        return self._p[1] ** 2 * (1 + (a * pa - b * pb) / Z - ((pa - pb) / Z) ** 2)


def _plain(t):
    return t.as_subclass(torch.Tensor) if type(t) is not torch.Tensor else t


def _draw_n(d, n):
    """n draws of a scalar family, one per particle: independent draws for shared parameters, elementwise for per-particle ones."""
    if isinstance(d, _Family):
        c = copy.copy(d)
        with torch._C.DisableTorchFunctionSubclass():
            c._p = tuple(_plain(q).reshape(-1).expand(n) if q.numel() == 1 else _plain(q).reshape(-1) for q in d._p)
        c._td = None
        return c.sample().reshape(-1).float()
    td = d._torch_dist
    batch = td.batch_shape.numel() if len(td.batch_shape) else 1
    return _plain(td.sample((n,)) if batch == 1 else td.sample()).reshape(-1).float()


def _moved(d, device):
    """A copy of a scalar family with every tensor attribute on `device`."""
    c = copy.copy(d)
    for k, v in list(c.__dict__.items()):
        if torch.is_tensor(v):
            c.__dict__[k] = v.to(device)
        elif isinstance(v, tuple) and v and all(torch.is_tensor(q) for q in v):
            c.__dict__[k] = tuple(q.to(device) for q in v)
    if c._td is not None:
        c._td = None
        if d.name == 'Poisson':
            c._td = torch.distributions.Poisson(d.rate.to(device), validate_args=False)
        elif d.name == 'Bernoulli':
            c._td = torch.distributions.Bernoulli(probs=d.probs.to(device), validate_args=False)
    return c


# the families a Mixture may hold (the scalar kinds of pp_mixture: every family but Factor, Categorical and Mixture itself)
MIXTURE_COMPONENT_KINDS = dict(DIST_KINDS, Normal=0, Uniform=1, Poisson=3, Bernoulli=4)
del MIXTURE_COMPONENT_KINDS['Factor']


class Mixture(Distribution):
    """pyprob/distributions/mixture.py: K component distributions and K weights, one row (1-D probs) or one row per batch element
    / particle (2-D probs). log_prob is logsumexp_k(log clamp(probs_k / sum probs) + log p_k(x)) with the clamp of
    util.clamp_probs; sample picks a component from Categorical(probs), then draws from it. The weights are kept as they were
    given (a device tensor or a per-particle ParticleTensor is neither read nor copied here: the device kernels normalise a
    row themselves, pp_mix_logweight / pp_mix_draw); `probs` is the normalised tensor, made on first use."""

    def __init__(self, distributions, probs=None):
        self._distributions = list(distributions)
        self.length = len(self._distributions)
        if self.length < 1:
            raise ValueError('Expecting at least one component distribution.')
        with torch._C.DisableTorchFunctionSubclass():
            if probs is None:
                raw = torch.full((self.length,), 1. / self.length)
            else:
                raw = probs if (torch.is_tensor(probs) and probs.dtype == torch.float32) else _t(probs).float()
            if raw.dim() == 1:
                self._batch_length = 0
            elif raw.dim() == 2:
                self._batch_length = raw.size(0)
            else:
                raise ValueError('Expecting a 1d or 2d (batched) mixture probabilities.')
            if raw.size(-1) != self.length:
                raise ValueError('Expecting one probability per component distribution.')
        self._raw_probs = raw
        self._probs = None
        self._mean = None
        self._variance = None
        super().__init__('Mixture', 'Mixture({})'.format(', '.join(d._address_suffix for d in self._distributions)))

    def __repr__(self):
        return 'Mixture(distributions=[{}], probs={})'.format(', '.join(repr(d) for d in self._distributions),
                                                             self.probs.detach().cpu().numpy().tolist())

    def __len__(self):
        return self.length

    def _device(self):
        return self._raw_probs.device

    @property
    def probs(self):
        if self._probs is None:
            raw = _plain(self._raw_probs)
            self._probs = raw / raw.sum(-1, keepdim=True)
        return self._probs

    @property
    def distributions(self):
        return self._distributions

    def _log_probs(self):
        eps = torch.finfo(torch.float32).eps
        return torch.log(self.probs.clamp(min=eps, max=1 - eps))        # util.clamp_probs

    def log_prob(self, value, sum=False):
        value = _plain(_t(value).float())
        lw = self._log_probs()
        if self._batch_length == 0:
            value = value.squeeze()
            lps = torch.stack(torch.broadcast_tensors(*[_plain(d.log_prob(value)).to(lw.device) for d in self._distributions]))
            lp = torch.logsumexp(lw.reshape((self.length,) + (1,) * (lps.dim() - 1)) + lps, dim=0)
        else:
            value = value.reshape(self._batch_length)
            lps = torch.stack([_plain(d.log_prob(value)).to(lw.device).reshape(-1).expand(self._batch_length)
                               for d in self._distributions], 1)
            lp = torch.logsumexp(lw + lps, dim=1)
        return torch.sum(lp) if sum else lp

    def sample(self):
        if self._batch_length == 0:
            i = int(torch.distributions.Categorical(probs=self.probs).sample())
            return self._distributions[i].sample()
        return self.sample_n(self._batch_length)

    def sample_n(self, n):
        """One draw per particle / batch element, vectorised: the component index of every row, then a gather from the components' draws."""
        p = _plain(self._raw_probs).reshape(-1, self.length)
        idx = torch.multinomial(p.expand(n, self.length) if p.size(0) == 1 else p, 1)
        draws = torch.stack([_draw_n(d, n).to(idx.device) for d in self._distributions], 1)
        return draws.gather(1, idx).reshape(-1)

    @property
    def mean(self):
        if self._mean is None:
            means = torch.stack(torch.broadcast_tensors(*[_plain(_t(d.mean)).float() for d in self._distributions]))
            if self._batch_length == 0:
                self._mean = torch.tensordot(self.probs, means, dims=([0], [0]))
            else:
                self._mean = (self.probs * means.reshape(self.length, -1).t()).sum(1)
        return self._mean

    @property
    def variance(self):
        if self._variance is None:
            m = self.mean
            var = torch.stack(torch.broadcast_tensors(*[(_plain(_t(d.mean)).float() - m).pow(2) + _plain(_t(d.variance)).float()
                                                        for d in self._distributions]))
            if self._batch_length == 0:
                self._variance = torch.tensordot(self.probs, var, dims=([0], [0]))
            else:
                self._variance = (self.probs * var.reshape(self.length, -1).t()).sum(1)
        return self._variance

    def to(self, device):
        return Mixture([_moved(d, device) for d in self._distributions], probs=self._raw_probs.to(device))


class Factor(Distribution):
    """pyprob/distributions/factor.py: the pseudo-distribution behind pyprob.factor - its log_prob is the given log-density
    (or log_prob_func(value)); it has no sample."""

    def __init__(self, log_prob=None, log_prob_func=None):
        if (log_prob is None) == (log_prob_func is None):
            raise RuntimeError('Expecting one of log_prob, log_prob_func' if log_prob is None else
                               'Expecting only one of log_prob, log_prob_func')
        self._log_prob = None if log_prob is None else (log_prob if torch.is_tensor(log_prob) else _t(log_prob).float())
        self._log_prob_func = log_prob_func
        super().__init__('Factor', 'Factor')

    def log_prob(self, value=None, sum=False):
        return self._log_prob if self._log_prob is not None else self._log_prob_func(value)

    def sample(self):
        return None

    def __repr__(self):
        return 'Factor()'


# The weighted-sample container and its batch calls live in modules of their own; their public names stay importable from here.
from .empirical import (PSIS_KHAT_THRESHOLD, Empirical, Histogram, Histogram2D, JointMoments, MixtureFit,  # noqa: E402,F401
                        PsisFit, joint_from_moments)
from .empirical_batch import (cdf_batch, density_estimate_batch, histogram_batch, hpd_batch, joint_batch,  # noqa: E402,F401
                              pareto_k_batch, psis_batch, quantile_batch, reobserve_batch, resample_batch)
