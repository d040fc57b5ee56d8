"""Empirical, the weighted-sample container behind Model.prior / posterior (pyprob/distributions/empirical.py), the result types
of its statistics and the decoders of the device kernels' output rows. The *_batch functions over the groups of one batched
posterior call live in empirical_batch.py, the float64 numpy routes in empirical_host.py."""
import contextlib
import math
import os
import warnings

import numpy as np
import torch

from .empirical_host import (_host_ecdf, _host_extent, _host_gmm, _host_hist_row, _host_hpd, _host_order, _host_psis,
                             _host_quantiles)


_NO_STATEMENT_LOG = ('this Empirical has no statement log: only the result of a lock-step posterior call '
                     '(posterior_results(..., lock_step=True), posterior_results_batch) keeps its latents per address')
_STALE_STATEMENT_LOG = ('this Empirical grew (add) after its lock-step posterior call: the statement log describes the particles of '
                        'that call only, so addresses / marginal / joint / resample_joint are not served')


_SCHEMES = {'multinomial': 0, 'stratified': 1, 'systematic': 2}      # PP_RESAMPLE_* (include/pyprob_amd.h)


def _scheme_id(scheme):
    if scheme not in _SCHEMES:
        raise ValueError('scheme is one of {}'.format(', '.join(repr(k) for k in _SCHEMES)))
    return _SCHEMES[scheme]


def _scheme_meta(scheme):
    return {} if scheme == 'multinomial' else {'scheme': scheme}


def _resample_op(cdf, values, n_per, lo, hi, n_out, scheme, key, offset, want_index):
    """The draw operator of a scheme: the default keeps the operator (and the bits) it always took."""
    from .ops import ops
    if _scheme_id(scheme) == 0:
        return ops.is_resample_groups(cdf, values, n_per, lo, hi, n_out, key, offset, want_index)
    return ops.is_resample_scheme_groups(cdf, values, n_per, lo, hi, n_out, _SCHEMES[scheme], key, offset, want_index)


def _flat_argument(a, message, ok=None):
    """(float64 [n] numbers, whether a scalar was given) of an argument that is a scalar or a sequence; more dimensions, or a number
    outside ok(array), raise ValueError(message)."""
    a = np.asarray(a, np.float64)
    if a.ndim > 1 or (ok is not None and not np.all(ok(a))):
        raise ValueError(message)
    return np.ascontiguousarray(a.reshape(-1)), a.ndim == 0


def _hpd_levels(level):
    return _flat_argument(level, 'level lies in (0, 1] (a scalar or a sequence)', lambda v: (v > 0) & (v <= 1))


def _quantile_levels(q):
    return _flat_argument(q, 'quantiles lie in [0, 1] (a scalar or a sequence)', lambda v: (v >= 0) & (v <= 1))


def _philox_key(seed):
    """The Philox key of a device draw: `seed`, or one number from torch's global generator as PriorLockStep takes it (pyprob.seed /
    torch.manual_seed reproduce a run)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def _resample_meta(length, num_samples, ess_before, scheme):
    return dict(op='resample', length=length, num_samples=int(num_samples), ess_before=ess_before, **_scheme_meta(scheme))


# ---- the particles of M groups in order (csrc/is_sort.hip): one Empirical (M = 1) and the *_batch functions alike ----------------
def _sorted_groups(lw, column, n_per, stats):
    """(values, log-weights, index int32, counted int32 [M, 2], cumulative weights float64) of the M groups of n_per particles in
    stable ascending order of value: pp_is_sort_groups, then pp_is_cdf_groups over the sorted log-weights."""
    from .ops import ops
    value, lw_sorted, index, counted = ops.is_sort_groups(lw, column, n_per, stats)
    return value, lw_sorted, index, counted, ops.is_cdf_groups(lw_sorted, n_per, stats)


def _lw_sorted_groups(lw, n_per, stats):
    """(log-weights, index int32, counted int32 [M, 2]) of the M groups in stable ascending order of their LOG-WEIGHT
    (pp_is_sort_groups keyed on the log-weights themselves; the non-finite ones last)."""
    from .ops import ops
    return ops.is_sort_groups(lw, lw, n_per, stats)[1:]


def _device_quantiles(groups, n_per, qs):
    """float64 numpy [M, Q] of pp_is_quantile_groups over _sorted_groups' result: one launch, one copy."""
    from .ops import ops
    value, _, _, counted, cdf = groups
    return ops.is_quantile_groups(value, cdf, counted, n_per, torch.from_numpy(qs).to(value.device)).cpu().numpy()


def _device_hpd(groups, n_per, levels):
    """float64 numpy [M, L, 2] of pp_is_hpd_groups over _sorted_groups' result."""
    from .ops import ops
    value, _, _, counted, cdf = groups
    return ops.is_hpd_groups(value, cdf, counted, n_per, torch.from_numpy(levels).to(value.device))[0].cpu().numpy()


def _device_ecdf(groups, n_per, pts, strict):
    """float64 numpy [M, Q] of pp_is_ecdf_groups over _sorted_groups' result, pts [M, Q]: every group with its own points."""
    from .ops import ops
    value, _, _, counted, cdf = groups
    return ops.is_ecdf_groups(value, cdf, counted, n_per, torch.from_numpy(pts).to(value.device), bool(strict))[0].cpu().numpy()


def _device_psis(groups, n_per, stats, tail, want_weights):
    """(the smoothed log-weights on the device or None, float64 numpy [M, PP_IS_PSIS_WIDTH]) of pp_is_psis_groups over
    _lw_sorted_groups' result."""
    from .ops import ops
    lw_out, out = ops.is_psis_groups(*groups, n_per, stats, tail, want_weights)
    return lw_out, out.cpu().numpy()


# What an Empirical computes once on the device and keeps in its __dict__ (_device_cdf, _device_extent, _device_sorted,
# _device_lw_sorted, combine_duplicates' masses, resample_joint's cdf over all particles) or is handed by its batched call (model.py:
# _batch, _batch_log; resample_batch: _batch_cdf). All of it describes the particles as they are: add() drops every name listed
# here, so a new cache is registered by adding its name.
_DEVICE_CACHES = ('_dev_cdf', '_dev_extent', '_dev_sorted', '_dev_lw_sorted', '_fixed_mass', '_all_cdf', '_batch', '_batch_cdf',
                  '_batch_log')


class Empirical:
    """Weighted samples: the result type of Model.prior / posterior (pyprob/distributions/empirical.py). Memory-backed;
    values are floats / tensors / arbitrary objects (or ONE device tensor for lock-step runs), weights are log-weights.
    The reductions (finalize :298-309, expectation :451-466, moments :668-690, effective_sample_size :758-766) are
    vectorised over the weight array instead of looping over the values; the transformation methods (map, condition,
    resample, thin, unweighted, slicing, concatenation :568-664, :768-773) return new Empiricals like the reference."""

    def __init__(self, values=None, log_weights=None, weights=None, concat_empiricals=None, name='Empirical'):
        self.name = name
        self._metadata = {}
        self._finalized = False
        self.length = 0
        if concat_empiricals is not None:        # ParallelModel's merge (model.py:395-404)
            parts = list(concat_empiricals)
            self._values = [v for e in parts for v in e.get_values()]
            self._log_weights = np.concatenate([e.log_weights_numpy() for e in parts]) if parts else []
            self.finalize()
            return
        if weights is not None:
            if log_weights is not None:
                raise ValueError('Expecting log_weights or weights, not both.')
            with np.errstate(divide='ignore'):
                log_weights = np.log(np.asarray(weights, np.float64))
        self._values = [] if values is None else values
        if log_weights is None:
            log_weights = [] if values is None else np.zeros(len(values))
        self._log_weights = log_weights
        if values is not None and len(values) > 0:
            self.finalize()

    @classmethod
    def from_device(cls, values, log_weights, device_stats, name='Empirical'):
        """The result of a lock-step run: ONE device tensor of values, one of log-weights and the importance statistics
        the device reduced in float64 (pp_is_stats / pp_is_fused). mean / variance / effective_sample_size answer from
        those; the host copies behind everything else (weights, sampling, slicing ...) are made on first use - a
        posterior call of 10^6 particles does not pay a 4 MB read-back and a host-side exp per call."""
        out = cls(name=name)
        out._values, out._log_weights = values, log_weights
        out.length = int(log_weights.numel())
        out.device_stats = device_stats
        out._finalized = True
        for k in ('_lw', '_w', '_uniform', '_cum'):      # (set by finalize(); absent = not materialised yet)
            out.__dict__.pop(k, None)
        return out

    def __getattr__(self, name):
        if name in ('_lw', '_w', '_uniform', '_cum') and '_log_weights' in self.__dict__ and self.__dict__.get('_finalized'):
            self.finalize()          # host-side weights of a device-backed Empirical, on first use
            if name in self.__dict__:
                return self.__dict__[name]
        if name in ('addresses', 'statement_rows'):      # (the properties below raised AttributeError: say why)
            raise AttributeError(_STALE_STATEMENT_LOG if self.__dict__.get('_log_stale') else _NO_STATEMENT_LOG)
        raise AttributeError(name)

    def _host_weights_ready(self):
        return '_w' in self.__dict__

    # ---- construction ------------------------------------------------------------------------------------
    def add(self, value, log_weight=None, weight=None):
        if weight is not None:
            log_weight = math.log(weight) if weight > 0 else float('-inf')
        if not isinstance(self._values, list) or not isinstance(self._log_weights, list):
            lw = self._lw if self._finalized else self._log_weights
            lw = lw.cpu().numpy() if torch.is_tensor(lw) else lw
            self._values = list(self.get_values()) if self._finalized else list(self._values)
            self._log_weights = [float(x) for x in np.asarray(lw, np.float64)]
        self._values.append(value)
        self._log_weights.append(0.0 if log_weight is None else float(log_weight))
        self._finalized = False
        for k in _DEVICE_CACHES:
            self.__dict__.pop(k, None)
        # the statement log describes the particles of the lock-step call, not this grown set: marginal / joint must not answer
        # for the old one (statement_log itself stays readable, as before; _latent_table refuses through _log_stale)
        for k in ('_latents', '_statement_rows', '_statement_rows_raw'):
            self.__dict__.pop(k, None)
        if 'statement_log' in self.__dict__:
            self.__dict__['_log_stale'] = True

    def add_sequence(self, values, log_weights=None, weights=None):
        for i, v in enumerate(values):
            self.add(v, None if log_weights is None else log_weights[i], None if weights is None else weights[i])

    def finalize(self):
        fixed = self.__dict__.get('_fixed_mass')
        if fixed is not None:
            # the result of combine_duplicates on the device: the host-side weights come from the integer masses themselves, in
            # float64 (the float32 log-weights on the device carry them to 2^-24 only)
            mass, shift, top = fixed
            m = mass.cpu().numpy().astype(np.float64)
            with np.errstate(divide='ignore'):
                self._lw = np.log(m) - shift * math.log(2.0) + top
            self.length = len(m)
            self._w = m / m.sum()
            self._uniform = bool(self.length) and bool(np.all(m == m[0]))
            self._cum = None
            self._finalized = True
            return self
        lw = np.asarray(self._log_weights.cpu() if torch.is_tensor(self._log_weights) else self._log_weights, np.float64)
        self._lw = lw
        self.length = len(lw)
        m = np.max(lw) if self.length else 0.0
        w = np.exp(lw - m)
        self._w = w / w.sum() if self.length else w
        self._uniform = bool(self.length) and bool(np.all(lw == lw[0]))
        self._cum = None
        self._finalized = True
        return self

    def _check_finalized(self):
        if not self._finalized:
            raise RuntimeError('Empirical not finalized. Call finalize first.')

    def __len__(self):
        return self.length

    def rename(self, name):
        self.name = name
        return self

    def add_metadata(self, **kwargs):
        self._metadata.update(kwargs)

    @property
    def metadata(self):
        return self._metadata

    def _like(self, values, log_weights, **meta):
        out = Empirical(name=self.name)
        out._values, out._log_weights = values, log_weights
        out.finalize()
        out._metadata = dict(self._metadata)
        out.add_metadata(**meta)
        return out

    # ---- access ---------------------------------------------------------------------------------------------
    @property
    def log_weights(self):
        return self._lw

    @property
    def weights(self):
        return torch.from_numpy(self._w)

    @property
    def weighted(self):
        return not self._uniform

    def weights_numpy(self):
        return self._w

    def log_weights_numpy(self):
        return self._lw

    def get_values(self):
        self._check_finalized()
        v = self._values
        return list(v.detach().cpu().unbind(0)) if torch.is_tensor(v) else v

    def values_numpy(self):
        v = self._values
        if torch.is_tensor(v):
            return v.detach().cpu().double().numpy()
        return np.asarray([float(x) for x in v], np.float64)

    def _value(self, i):
        v = self._values
        return v[i].detach().cpu() if torch.is_tensor(v) else v[i]

    def __iter__(self):
        self._check_finalized()
        for i in range(self.length):
            yield self._value(i)

    def __getitem__(self, index):
        self._check_finalized()
        if isinstance(index, slice):
            return self._like(self.get_values()[index], self._lw[index], op='slice', index=str(index))
        if isinstance(index, (int, np.integer)):
            return self._value(int(index))
        raise RuntimeError('Cannot use the given value ({}) as index'.format(index))

    def _draw_indices(self, n, lo=None, hi=None, scheme='multinomial'):
        """n indices distributed like the (renormalised) weights of [lo, hi); randomness from torch's global generator
        (so pyprob.seed / torch.manual_seed make it reproducible). scheme 'stratified' / 'systematic': the positions
        min((j + u_j) / n, 1 - 2^-53) of pp_is_resample_scheme_groups, u_j one uniform per draw / one for all."""
        lo = 0 if lo is None else lo
        hi = self.length if hi is None else hi
        if hi <= lo:
            raise ValueError('empty index range')
        if _scheme_id(scheme) == 0:
            u = torch.rand(n, dtype=torch.float64).numpy()
        else:
            u = torch.rand(n if scheme == 'stratified' else 1, dtype=torch.float64).numpy()
            u = np.minimum((np.arange(n, dtype=np.float64) + u) / float(n), 1.0 - 2.0 ** -53)
        if self._uniform:
            return lo + np.minimum((u * (hi - lo)).astype(np.int64), hi - lo - 1)
        if self._cum is None:
            self._cum = np.cumsum(self._w)
        base = self._cum[lo - 1] if lo > 0 else 0.0
        total = self._cum[hi - 1] - base
        return np.minimum(np.searchsorted(self._cum, base + u * total, side='right'), hi - 1)

    # ---- device route of sample / resample (csrc/is_resample.hip) --------------------------------------------------
    def _device_backed(self):
        """Values and log-weights are ONE contiguous float32 device tensor each (the result of a lock-step posterior call):
        sample / resample then run on the device. PP_EMPIRICAL_DEVICE=0 keeps the host route for such objects too."""
        v, lw = self.__dict__.get('_values'), self.__dict__.get('_log_weights')
        return (self._finalized and torch.is_tensor(v) and torch.is_tensor(lw) and v.is_cuda and lw.is_cuda and
                v.dtype == torch.float32 and lw.dtype == torch.float32 and v.dim() == 1 and lw.dim() == 1 and
                v.numel() == lw.numel() and v.numel() > 0 and v.is_contiguous() and lw.is_contiguous() and
                os.environ.get('PP_EMPIRICAL_DEVICE', '1') != '0')

    def _device_cdf(self):
        """The running sum of exp(lw - max lw) in float64 on the device (pp_is_cdf_groups): computed once per object, 8 bytes per
        particle, dropped with the object. A group of a batched call hands the kernel the maximum its call already reduced."""
        cdf = self.__dict__.get('_dev_cdf')
        if cdf is None:
            from .ops import ops
            cdf = self.__dict__['_dev_cdf'] = ops.is_cdf_groups(self._log_weights, self.length, self._group_stats_row())
        return cdf

    def _index_range(self, min_index, max_index):
        lo = 0 if min_index is None else int(min_index)
        hi = self.length if max_index is None else int(max_index)
        if hi <= lo:
            raise ValueError('empty index range')
        if lo < 0 or hi > self.length:
            raise ValueError('index range [%d, %d) outside the %d values' % (lo, hi, self.length))
        return lo, hi

    def _device_draw(self, n, min_index, max_index, seed, offset, scheme='multinomial'):
        """n values drawn on the device according to the weights of [min_index, max_index): one launch, a device tensor."""
        from .ops import ops
        lo, hi = self._index_range(min_index, max_index)
        return _resample_op(self._device_cdf(), self._values, self.length, lo, hi, int(n), scheme, _philox_key(seed), int(offset),
                            False)[1]

    def _resampled(self, values, zeros, stats, num_samples, ess_before, scheme='multinomial'):
        out = Empirical.from_device(values, zeros, stats, name=self.name)
        out._metadata = dict(self._metadata)
        out.add_metadata(**_resample_meta(self.length, num_samples, ess_before, scheme))
        return out

    def sample(self, min_index=None, max_index=None):
        """One value drawn according to the weights (empirical.py:392-408; min_index inclusive, max_index exclusive). A
        device-backed Empirical draws on the device (see resample)."""
        self._check_finalized()
        if self._device_backed():
            return self._device_draw(1, min_index, max_index, None, 0)[0].cpu()
        return self._value(int(self._draw_indices(1, min_index, max_index)[0]))

    # ---- the other latents of a lock-step call (csrc/is_moments.hip) ------------------------------------------------
    def _latent_table(self):
        """{address: (values [n] of ALL particles of the call, rows that executed it or None)} in the order the statement log
        first meets each address - the statement log of a lock-step posterior call. Every other Empirical has none.

        The log is keyed by statement index first, and a branch that changes the number of statements before a common one puts
        the same address at different indices for different paths (`if a > 0: b = sample(...)` before `c = sample(...)`: 'c' is
        statement 2 of one path and statement 1 of the other). Such an address is ONE latent: its entries are merged into one
        column - each entry's rows copied in - under the union of their row lists, None where that is every particle."""
        log = self.__dict__.get('statement_log')
        if log is None:
            raise AttributeError(_NO_STATEMENT_LOG)
        if self.__dict__.get('_log_stale'):
            raise AttributeError(_STALE_STATEMENT_LOG)
        if os.environ.get('PP_EMPIRICAL_DEVICE', '1') == '0':
            raise ValueError('PP_EMPIRICAL_DEVICE=0 keeps every Empirical on the host route: the statement log is not served '
                             '(addresses / marginal / joint / resample_joint need the device route)')
        table = self.__dict__.get('_latents')
        if table is None:
            rows = self.statement_rows
            found = {}
            for j, entry in enumerate(log):
                for address, rec in entry.items():
                    if torch.is_tensor(rec[0]) and rec[0].dim() == 1:
                        found.setdefault(address, []).append((rec[0], rows[j].get(address) if j < len(rows) else None))
            table = {}
            for address, parts in found.items():
                whole = [p for p in parts if p[1] is None]
                if whole or len(parts) == 1:       # one entry, or an entry every particle wrote: the log's own tensor
                    table[address] = whole[0] if whole else parts[0]
                    continue
                column = parts[0][0].clone()
                for values, r in parts[1:]:
                    column.index_copy_(0, r, values.index_select(0, r))
                union = torch.unique(torch.cat([r for _, r in parts]))      # (sorted)
                table[address] = (column, None if union.numel() == column.numel() else union)
            self.__dict__['_latents'] = table
        return table

    @property
    def statement_rows(self):
        """Per statement index {address: the ascending int64 indices of the particles that executed it, or None = all of them}."""
        merged = self.__dict__.get('_statement_rows')
        if merged is None:
            raw = self.__dict__.get('_statement_rows_raw')
            if raw is None:
                raise AttributeError(_STALE_STATEMENT_LOG if self.__dict__.get('_log_stale') else _NO_STATEMENT_LOG)
            merged = [{a: (None if r is None else (r[0] if len(r) == 1 else torch.sort(torch.cat(r))[0])) for a, r in e.items()}
                      for e in raw]
            self.__dict__['_statement_rows'] = merged
        return merged

    @property
    def addresses(self):
        """The addresses of the statement log in statement order."""
        return list(self._latent_table())

    def _latent(self, address):
        table = self._latent_table()
        if address not in table:
            address = self.__dict__.get('statement_names', {}).get(address, address)
        if address not in table:       # the address= of a sample statement: the one full address it begins ('a' -> 'a__Normal__1')
            begun = [a for a in table if a.startswith(str(address) + '__')]
            address = begun[0] if len(begun) == 1 else address
        if address not in table:
            raise KeyError('unknown address {!r}: this posterior knows {} (names: {})'.format(
                address, list(table), list(self.__dict__.get('statement_names', {}))))
        return (address,) + table[address]

    def _all_lw(self):
        lw = self.__dict__.get('_all_log_weights')
        return lw if lw is not None else self._log_weights

    def marginal(self, address):
        """The posterior of ONE latent of a lock-step call as an Empirical of its own (pyprob: posterior.map(lambda t:
        t.named_variables[name].value)): the address's values of the statement log under the call's log-weights, its
        device_stats reduced on the device (pp_is_stats; the call's own for the latent forward() returned), so that mean /
        variance / resample / sample / median answer on the device as they do for the result column. `address` is an address of
        `addresses`, the name= of its sample statement, or the address= the statement was given where that begins one address
        only. Particles with a non-finite log-weight are dropped as the call dropped them. An address only some particles executed
        (a branch) gives the Empirical over THOSE particles, weights renormalised among them (pyprob: condition + map).

        The call's own statistics are reused only where the posterior's value column IS the log's tensor (the same memory): the
        inference-network route returning a latent as it drew it. Where the call copied the return value (the prior route) or
        forward() returned anything computed, the marginal takes pp_is_stats like every other address, and its mean may sit ~1e-9
        relative from `post.mean` (fp64 against fp32 exponent of the weights) - the same distribution either way."""
        address, values, rows = self._latent(address)
        lw = self._all_lw()
        own, own_stats = self.__dict__.get('_all_values'), self.__dict__.get('device_stats')
        if rows is None and own_stats is not None and torch.is_tensor(own) and own.data_ptr() == values.data_ptr() and \
                own.numel() == values.numel():
            # the latent forward() returned: this posterior's own column, under the statistics its call reduced - one source of
            # truth for the same numbers (the call's fused pass takes its weights from an fp32 exponent, pp_is_stats from an fp64
            # one: mean and variance of the same column differ by ~1e-9 relative between the two)
            values, lw, stats = self._values, self._log_weights, own_stats
        else:
            if rows is not None:
                values, lw = values.index_select(0, rows), lw.index_select(0, rows)
            stats = _device_stats(lw, values)
            if int(stats['count']) != lw.numel():
                ok = torch.isfinite(lw)
                values, lw = values[ok].contiguous(), lw[ok].contiguous()
                if lw.numel() == 0:
                    raise ValueError('no particle with a finite log-weight executed address {!r}'.format(address))
                stats = _device_stats(lw, values)
        out = Empirical.from_device(values, lw, stats, name=self.name)
        out._metadata = dict(self._metadata)
        out.add_metadata(op='marginal', address=address, length=self.length, length_after=out.length)
        return out

    def _joint_columns(self, addresses):
        table = self._latent_table()
        if addresses is None:
            chosen = [a for a, (_, rows) in table.items() if rows is None]
        else:
            chosen = []
            for a in addresses:
                a, _, rows = self._latent(a)
                if rows is not None:
                    raise ValueError('address {!r} was executed by {} of the particles only (a branch): joint() takes addresses '
                                     'that every particle executed - see marginal()'.format(a, int(rows.numel())))
                chosen.append(a)
        if not chosen:
            raise ValueError('no address that every particle executed')
        return chosen, [table[a][0] for a in chosen]

    def joint(self, addresses=None):
        """Means, covariances and correlations of several latents of a lock-step call over its weighted particles, as a
        JointMoments (addresses, mean [J], cov [J, J], corr [J, J], stddev [J] in float64 numpy, ess, count): one
        pp_is_moments_groups launch over the statement log's columns and one device-to-host copy. The covariance is the biased,
        weight-normalised form of Empirical.variance. addresses: addresses or statement names, default every address that ALL
        particles executed; an address of a branch raises ValueError. More than 16 addresses are served in blocks of 8 columns,
        one call per pair of blocks: the entries that cross two blocks come from separate calls (each over the same weights,
        each bit-reproducible). No particle with a finite log-weight: NaN arrays, count 0."""
        chosen, cols = self._joint_columns(addresses)
        lw = self._all_lw()
        return _joint_rows(chosen, _moment_rows(lw, cols, lw.numel(), self._group_stats_row()))[0]

    def resample_joint(self, num_samples, addresses=None, seed=None, offset=0, scheme='multinomial'):
        """num_samples JOINT draws of several latents: ONE index per sample from the weights (pp_is_resample_groups, the Philox
        contract of resample: draw k = key `seed`, counter offset + k), then row index[k] of every requested column. Returns
        {address: device tensor [num_samples]} plus 'index' (int64, into ALL particles of the call: the rows of the statement
        log's columns). With the same seed and offset the indices - and so the result column - are those resample() draws,
        PROVIDED the call dropped no particle. Where it dropped particles with a non-finite log-weight, the posterior's own
        particles are renumbered and resample() indexes those; here the cumulative weights run over all particles with weight 0
        for the dropped ones, so no draw lands on them, row k of every column is still one particle's, and the draws follow the
        same distribution - but they are another stream than resample()'s. scheme: as for resample."""
        from .ops import ops
        _scheme_id(scheme)
        if int(num_samples) < 1:
            raise ValueError('num_samples must be positive')
        chosen, cols = self._joint_columns(addresses)
        lw = self._all_lw()
        if lw is self._log_weights:
            cdf = self._device_cdf()
        else:       # (the call dropped particles: the cdf over ALL of them, weight 0 where the log-weight is not finite)
            cdf = self.__dict__.get('_all_cdf')
            if cdf is None:
                cdf = self.__dict__['_all_cdf'] = ops.is_cdf_groups(lw, lw.numel(), None)
        n = lw.numel()
        index = _resample_op(cdf, None, n, 0, n, int(num_samples), scheme, _philox_key(seed), int(offset), True)[0]
        out = {a: c.index_select(0, index) for a, c in zip(chosen, cols)}
        out['index'] = index
        return out

    # ---- histograms (csrc/is_hist.hip) ---------------------------------------------------------------------------------
    def _group_stats_row(self):
        """The [6] statistics row of this group of a batched call on the device (its maximum spares the kernels a launch)."""
        batch = self.__dict__.get('_batch')
        return batch[2][batch[3]] if (batch is not None and batch[2] is not None) else None

    def histogram(self, bins=50, range=None, edges=None):
        """The weighted histogram of the values as a Histogram (edges, mass, density, count, below, above, nan, particles; cdf,
        quantile, credible_interval, mode). bins: the number of equal bins over `range` = (lo, hi); range=None takes the finite
        extent of the values (of the particles with a finite log-weight; lo == hi is widened by 0.5 on either side as numpy does;
        an infinite value needs an explicit range) and the edges are numpy.linspace(lo, hi, bins + 1). edges: the bin edges
        themselves, strictly increasing and finite (log bins, for instance), instead of bins / range; at most 2048 bins. Bin b
        holds e_b <= x < e_{b+1}, the last bin also x == e_last (numpy.histogram's rule).

        A device-backed Empirical (the result of a lock-step posterior call, post.marginal(address), a device resample) is binned
        on the device: pp_is_extent_groups where the range is needed (four doubles come back), then pp_is_hist_groups - weights
        in fp64, summed in 64-bit fixed point, so the same call gives the same bits every time - and one copy of the row of
        bins. Every other Empirical, and all of them under PP_EMPIRICAL_DEVICE=0, computes the same Histogram in float64 numpy
        by the same bin rule (no fixed point: masses agree to rounding, counts exactly)."""
        self._check_finalized()
        if self.length == 0:
            raise ValueError('histogram of an empty Empirical')
        if self._device_backed():
            return _device_histograms(self._log_weights, self._values, self.length, bins, range, edges, self._group_stats_row())[0]
        lw = np.asarray(self._lw, np.float64)
        x = self.values_numpy()
        if x.shape != lw.shape:
            raise ValueError('histogram needs scalar values')
        e = _hist_edges_for(bins, range, edges, lambda: _host_extent(lw, x)[None])
        return _histogram_rows(e, _host_hist_row(lw, x, e[0])[None], exact=False)[0]

    def histogram2d(self, x, y, bins=(32, 32), range=None):
        """The weighted 2-D histogram of two latents of a lock-step call as a Histogram2D (x_edges, y_edges, mass [bx, by],
        density, count, outside, nan, particles): pp_is_hist_groups over the two columns of the statement log under the call's
        log-weights, one copy of the row. x / y: addresses or statement names as joint() takes them (an address only some particles
        executed raises joint()'s ValueError). bins: one number or (bins_x, bins_y), bins_x bins_y <= 2048; range: ((xlo, xhi),
        (ylo, yhi)), default the finite extent of each column (pp_is_extent_groups)."""
        chosen, cols = self._joint_columns([x, y])
        lw = self._all_lw()
        bx, by = (bins, bins) if np.ndim(bins) == 0 else bins
        _check_bins(bx)
        _check_bins(by)
        if int(bx) * int(by) > _HIST_MAX_BINS:
            raise ValueError('at most %d bins (bins_x * bins_y)' % _HIST_MAX_BINS)
        rx, ry = (None, None) if range is None else range
        from .ops import ops
        n = lw.numel()
        ex = _hist_edges_for(bx, rx, None, lambda: ops.is_extent_groups(lw, cols[0], n).cpu().numpy())[0]
        ey = _hist_edges_for(by, ry, None, lambda: ops.is_extent_groups(lw, cols[1], n).cpu().numpy())[0]
        row = ops.is_hist_groups(lw, cols[0], cols[1], n, torch.from_numpy(ex).to(lw.device), torch.from_numpy(ey).to(lw.device),
                                 self._group_stats_row()).cpu().numpy()[0]
        return _histogram2d_row(chosen, ex, ey, row)

    # ---- order statistics (csrc/is_sort.hip) ---------------------------------------------------------------------------
    def _device_sorted(self):
        """(values, log-weights, index int32, counted int32 [1, 2], cumulative weights float64) of the particles in stable ascending
        order of value on the device (pp_is_sort_groups, then pp_is_cdf_groups over the sorted log-weights): computed once per
        object and kept like the cdf of resample - 20 bytes per particle, dropped with the object."""
        s = self.__dict__.get('_dev_sorted')
        if s is None:
            s = self.__dict__['_dev_sorted'] = _sorted_groups(self._log_weights, self._values, self.length, self._group_stats_row())
        return s

    def _host_scalars(self):
        """(log-weights, values) in float64 numpy for the host route of the order statistics; values that are not scalars: None."""
        try:
            x = self.values_numpy()
        except (TypeError, ValueError, RuntimeError):
            return np.asarray(self._lw, np.float64), None
        lw = np.asarray(self._lw, np.float64)
        return lw, (x if x.shape == lw.shape else None)

    def _order_statistic(self, what, device, host):
        """The one body of quantile / hpd_interval / cdf after their argument is normalised: device(the sorted particles of
        _device_sorted) -> the numpy rows of the one group, or host(log-weights, values) in float64 numpy -> the row."""
        if self.length == 0:
            raise ValueError('%s of an empty Empirical' % what)
        if self._device_backed():
            return device(self._device_sorted())[0]
        lw, x = self._host_scalars()
        if x is None:
            raise ValueError('%s needs scalar values' % what)
        return host(lw, x)

    def quantile(self, q):
        """The exact weighted quantile of the values by the inverted cdf, for a scalar q (a float) or a sequence (float64 numpy
        [Q]), each in [0, 1]: with the counted particles (finite log-weight, value not NaN) in ascending order of value (ties in
        particle order, -0.0 == +0.0), W_k the cumulative sum of exp(lw - max lw) in that order and T its last value, the value of
        the first particle with W_k >= fl(q T) - for fl(q T) == 0 the first particle of positive cumulative weight. With uniform
        weights quantile(0.5) is the lower of the two middle values (what median returns for uniform tensor values). Nothing
        counted, or a total that is not positive and finite: NaN.

        A device-backed Empirical (the result of a lock-step posterior call, post.marginal(address), a device resample) is sorted
        once on the device (pp_is_sort_groups and the cumulative weights of the sorted particles, kept with the object); every
        call is then one launch of a binary search per q (pp_is_quantile_groups) and Q doubles travel back. Every other
        Empirical, and all of them under PP_EMPIRICAL_DEVICE=0, computes the same definition in float64 numpy (over float64
        values: the sums agree to rounding, the value returned is one of the particles' either way)."""
        self._check_finalized()
        qs, scalar = _quantile_levels(q)
        out = self._order_statistic('quantile', lambda s: _device_quantiles(s, self.length, qs),
                                    lambda lw, x: _host_quantiles(lw, x, qs))
        return float(out[0]) if scalar else out

    def credible_interval(self, level=0.9):
        """The equal-tailed interval (quantile((1 - level) / 2), quantile((1 + level) / 2)), both from one quantile call."""
        if not 0 < level <= 1:
            raise ValueError('level lies in (0, 1]')
        lo, hi = self.quantile([(1.0 - level) / 2.0, (1.0 + level) / 2.0])
        return float(lo), float(hi)

    def hpd_interval(self, level=0.9):
        """The highest-posterior-density interval: the SHORTEST interval [lo, hi] between two particles that holds the mass
        `level` - (lo, hi) floats for a scalar level in (0, 1], float64 numpy [L, 2] for a sequence. With the counted particles in
        ascending order of value, W_k their cumulative weights (quantile's) and T the last: among the particles i of positive
        weight with fl(W_{i-1} + fl(level T)) <= T, the one whose window up to the first particle j with W_j >= that target is
        narrowest, ties to the smallest i. On a skewed or one-sided posterior it differs from the equal-tailed credible_interval:
        an Exponential's 90 % interval starts at its minimum. A posterior of several modes gets ONE interval (regions of more
        than one interval are not built). Nothing counted, or a total that is not positive and finite: NaN.

        A device-backed Empirical is sorted once (as for quantile); every call is then one operator call (pp_is_hpd_groups: a
        thread per start, a binary search each) and one copy of 2 L doubles. Every other Empirical, and all of them under
        PP_EMPIRICAL_DEVICE=0, computes the same definition in float64 numpy."""
        self._check_finalized()
        levels, scalar = _hpd_levels(level)
        out = self._order_statistic('hpd_interval', lambda s: _device_hpd(s, self.length, levels),
                                    lambda lw, x: _host_hpd(lw, x, levels))
        return (float(out[0, 0]), float(out[0, 1])) if scalar else out

    def cdf(self, x, strict=False):
        """The posterior cdf P(X <= x) (strict: P(X < x)) at a scalar x (a float) or a sequence (float64 numpy of its shape [Q]): the
        cumulative weight of the counted particles (finite log-weight, value not NaN) whose value is <= x, over their total - the
        forward map of quantile(): cdf(quantile(q)) >= q up to two roundings. A NaN x, nothing counted or a total that is not
        positive and finite: NaN. Device-backed Empiricals answer from the sorted particles (as quantile) by one operator call
        (pp_is_ecdf_groups, a binary search per point) and one copy; every other Empirical, and all of them under
        PP_EMPIRICAL_DEVICE=0, in float64 numpy."""
        self._check_finalized()
        xs, scalar = _flat_argument(x, 'cdf takes a scalar or a sequence of points')
        out = self._order_statistic('cdf', lambda s: _device_ecdf(s, self.length, xs[None], strict),
                                    lambda lw, v: _host_ecdf(lw, v, xs, strict))
        return float(out[0]) if scalar else out

    # ---- Pareto-smoothed importance sampling (csrc/is_psis.hip) -----------------------------------------------------------
    def _device_lw_sorted(self):
        """(log-weights, index int32, counted int32 [1, 2]) of the call's particles in stable ascending order of their LOG-WEIGHT on
        the device (pp_is_sort_groups keyed on the log-weights themselves; the non-finite ones last): computed once per object and
        kept like _device_sorted - 8 bytes per particle, dropped with the object."""
        s = self.__dict__.get('_dev_lw_sorted')
        if s is None:
            lw = self._all_lw()
            s = self.__dict__['_dev_lw_sorted'] = _lw_sorted_groups(lw, lw.numel(), self._group_stats_row())
        return s

    def pareto_k(self, tail=None):
        """The shape k-hat of the generalised Pareto distribution fitted to the largest importance weights (PSIS: Vehtari, Simpson,
        Gelman, Yao, Gabry, JMLR 2024), a float: below 0.7 the importance-sampling estimates can be trusted, above it their
        variance is practically or literally infinite - what effective_sample_size does not show when the proposal misses a heavy
        tail. tail: the number of largest weights fitted, default ceil(min(c / 5, 3 sqrt(c))) of the c particles with a finite
        log-weight. +inf where no tail could be fitted (fewer than five distinct weights above the cutoff, all weights equal, a
        tail that underflows). The definition is pp_is_psis_groups' header comment.

        A device-backed Empirical is sorted by log-weight once (kept with the object); every call is then one operator call
        without the smoothing launch and one copy of 8 doubles. Every other Empirical, and all of them under
        PP_EMPIRICAL_DEVICE=0, computes the same definition in float64 numpy."""
        self._check_finalized()
        t = _psis_tail(tail)
        if self.length == 0:
            raise ValueError('pareto_k of an empty Empirical')
        if self._device_backed():
            groups = self._device_lw_sorted()
            row = _device_psis(groups, groups[0].numel(), self._group_stats_row(), t, False)[1][0]
        else:
            row = _host_psis(self._lw, t, False)[1]
        return float(row[0])

    def psis(self, tail=None):
        """A new Empirical with the same values and Pareto-smoothed log-weights: the `tail` largest weights (default as for pareto_k)
        are replaced by the order statistics of the generalised Pareto distribution fitted to them, capped at the largest weight,
        which stabilises every expectation taken afterwards; every other log-weight keeps its bits. `.fit` is a PsisFit (khat,
        sigma, tail, grid, log_cutoff, count, ess_before, ess_after); the metadata says op='psis'. A UserWarning names a k-hat
        above 0.7; where no tail could be fitted (k-hat = +inf) the weights are unchanged and the warning says so.

        A device-backed Empirical stays on the device (pp_is_psis_groups over the particles sorted by log-weight, the statistics
        reduced again by pp_is_stats). The posterior of a lock-step call is smoothed over ALL particles of the call and keeps its
        statement log: marginal / joint / resample_joint / histogram2d of the result answer under the smoothed weights. Every
        other Empirical, and all of them under PP_EMPIRICAL_DEVICE=0, computes the same definition in float64 numpy."""
        self._check_finalized()
        t = _psis_tail(tail)
        if self.length == 0:
            raise ValueError('psis of an empty Empirical')
        if self._device_backed():
            groups = self._device_lw_sorted()
            lw_out, rows = _device_psis(groups, groups[0].numel(), self._group_stats_row(), t, True)
            return self._psis_result(lw_out, rows[0])
        new, row = _host_psis(self._lw, t, True)
        ess = self.effective_sample_size
        out = self._like(self._values, new, op='psis', length=self.length, khat=float(row[0]))
        out.fit = _psis_fit(row, ess, out.effective_sample_size)
        return out

    def _psis_result(self, lw_out, row, stats=None):
        """The smoothed posterior of psis() from the log-weights the kernel wrote for the call's particles and its row of `out`;
        stats: pp_is_stats over the smoothed particles where the caller reduced them already (psis_batch: one copy for all)."""
        own = self.__dict__
        if '_all_log_weights' in own and own.get('_all_values') is not None:
            all_values = own['_all_values']
            if self._log_weights.numel() == lw_out.numel():      # (the call dropped no particle: the tensor the kernel wrote)
                values, lw = self._values, lw_out
            else:
                from .model import _drop_non_finite
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')              # (the call said so already)
                    values, lw = _drop_non_finite(all_values, lw_out)
        else:
            all_values, values, lw = None, self._values, lw_out
        out = Empirical.from_device(values, lw, _device_stats(lw, values) if stats is None else stats, name=self.name)
        if all_values is not None:
            out._all_values, out._all_log_weights = all_values, lw_out
            for k in ('statement_log', '_statement_rows_raw', 'statement_names', 'num_paths'):
                if k in own:
                    out.__dict__[k] = own[k]
        out._metadata = dict(self._metadata)
        out.add_metadata(op='psis', length=self.length, khat=float(row[0]))
        out.fit = _psis_fit(row, self.effective_sample_size, out.effective_sample_size)
        return out

    # ---- re-scoring under new observations (csrc/is_reobserve.hip) ------------------------------------------------------
    def _reobserve_weights(self, cols, M, likelihood_funcs, likelihood_importance):
        """([M, N] log-weights of ALL particles of the call under the M new observations, the re-scored names, the origin): ONE
        replay of the program over the statement log (state.ReobserveState), `old` by the accumulate route on a zeroed vector at
        the original scale, ONE pp_is_reobserve_groups call. cols: {name: float32 array [M, k]} (a name that only gets a new
        likelihood keeps its original value)."""
        from . import state
        from .is_engine import DistRunner, VecTerm
        from .ops import ops
        log = self.__dict__.get('statement_log')
        self._latent_table()          # (no statement log, a stale one, PP_EMPIRICAL_DEVICE=0: refused as marginal / joint refuse)
        origin = self.__dict__.get('_origin')
        if origin is None and self.__dict__.get('_origin_lost'):
            raise ValueError('reobserve: ' + self._origin_lost)
        if origin is None:
            raise AttributeError('this Empirical does not know the call that made it: reobserve serves the result of '
                                 'posterior_results(..., lock_step=True) and the members of posterior_results_batch')
        model, args, kwargs, observe0, scale0, engine = origin
        if self.__dict__.get('num_paths', 1) != 1:
            raise NotImplementedError('reobserve replays straight-line programs only: this posterior ran {} control-flow paths'
                                      .format(self.num_paths))
        if isinstance(observe0, tuple):      # a member of a batched call: row g of the call's observations
            obs, g = observe0
            observe0 = {k: v.as_subclass(torch.Tensor)[g].cpu() for k, v in obs.items()}
        observe0 = dict(observe0 or {})
        targets = list(dict.fromkeys(list(cols) + list(likelihood_funcs or {})))
        if not targets:
            raise ValueError('reobserve: name an observable in `observe` or `likelihood_funcs`')
        lw = self._all_lw()
        n, dev = int(lw.numel()), lw.device
        runner = _REOBSERVE_RUNNERS.get(dev)
        if runner is None:
            runner = _REOBSERVE_RUNNERS[dev] = DistRunner(dev)
        ls = state.ReobserveState(runner, n, log, targets, likelihood_funcs)
        with (torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext()):
            state._init_traces(func=model.forward, trace_mode=state.TraceMode.POSTERIOR,
                               inference_engine=state.InferenceEngine.IMPORTANCE_SAMPLING, observe=observe0,
                               likelihood_importance=scale0, lock_step=ls)
            runner.begin(n)
            try:
                state._begin_trace()
                model.forward(*args, **kwargs)
            finally:
                state._lock_step = None
                state._current_trace = None
                ls.memo = None
            seen = [r[0] for r in ls.records]
            unknown = [t for t in targets if t not in seen]
            if unknown:
                raise ValueError('reobserve: {} not among the named observes of the program: {}'.format(unknown, ls.observe_names))
            if len(ls.records) > 8:
                raise NotImplementedError('reobserve: at most 8 re-scored observe statements per call')
            scale1 = float(scale0 if likelihood_importance is None else likelihood_importance)
            old = torch.zeros(n, dtype=torch.float32, device=dev)
            kinds, ks, scales, params, xs = [], [], [], [], []
            for name, new, term0, v0, k in ls.records:
                runner.accumulate(old, term0, v0, float(scale0))
                if type(new) is VecTerm:
                    kind, ps = new.kind, new.params
                else:
                    wide = new.wide()
                    kind, ps = wide.kind, [p if p is None or p.numel() == 1 else p.reshape(n, 1) for p in wide.params]
                if name in cols:
                    c = np.ascontiguousarray(cols[name], np.float32).reshape(M, -1)
                    if c.shape[1] != k:
                        raise ValueError('reobserve: observable {!r} has {} values, the new observation {}'.format(name, k, c.shape[1]))
                    x = torch.from_numpy(c).to(dev)
                else:
                    x = v0.reshape(1, k)
                kinds.append(int(kind)); ks.append(k); scales.append(scale1); params += list(ps); xs.append(x)
            out = ops.reobserve_groups(lw, old, kinds, ks, scales, params, xs, int(M))
        # the scale a later reobserve takes the old terms out at: one number only where every weighted term carries it
        scale = scale1 if (len(seen) == ls.n_weighted or scale1 == float(scale0)) else None
        return out, seen, (model, args, kwargs, observe0, scale, engine)

    def _reobserve_stats(self, origin, out):
        """The [M, 6] statistics of out [M, N] over the call's values, on the device, and the values expanded to [M N]: ONE grouped
        pass (pp_is_fused_groups without a draw or a term) where the model has an inference network on this device, else one
        pp_is_stats launch per group. A group's row does not depend on M."""
        all_values = self.__dict__.get('_all_values')
        all_values = self._values if all_values is None else all_values
        M, N = int(out.shape[0]), int(out.shape[1])
        values = all_values if M == 1 else all_values.reshape(1, N).expand(M, N).reshape(-1)
        runner = getattr(getattr(origin[0], '_inference_network', None), '_is', None)
        if out.is_cuda and runner is not None and runner.dev == out.device and hasattr(runner, 'fused_groups'):
            return runner.fused_groups(None, N, None, [], values, out.reshape(-1), False, stats=True), values, runner
        return torch.stack([_device_stats_row(out[g], all_values)[:6] for g in range(M)]).contiguous(), values, None

    def _reobserve_result(self, lw_new, stats, origin, observe, names):
        """The Empirical of the call's particles under the new log-weights lw_new [N] (all particles): non-finite ones are
        dropped as the call dropped them, the full vectors, the statement log and the origin (new values merged) stay."""
        own = self.__dict__
        all_values = own.get('_all_values')
        all_values = self._values if all_values is None else all_values
        values, lw = all_values, lw_new
        if int(stats['count']) != lw_new.numel():
            from .model import _drop_non_finite
            values, lw = _drop_non_finite(all_values, lw_new)
            if lw.numel() == 0:
                raise ValueError('reobserve: no particle has a finite log-weight under the new observation')
            stats = _device_stats(lw, values)
        out = Empirical.from_device(values, lw, stats, name=self.name)
        out._all_values, out._all_log_weights = all_values, lw_new
        for k in ('statement_log', '_statement_rows_raw', 'statement_names', 'num_paths'):
            if k in own:
                out.__dict__[k] = own[k]
        model, args, kwargs, observe0, scale, engine = origin
        if scale is not None:
            out._origin = (model, args, kwargs, dict(observe0, **observe), scale, engine)
        else:       # the origin holds ONE likelihood_importance: the scale a later call takes the old terms out at
            out._origin_lost = ('this posterior was re-observed for SOME of its observes at another likelihood_importance than the '
                                'rest carry, so its terms no longer share one scale and it cannot be re-observed again - re-observe '
                                'the original posterior, naming every observe, instead')
        out._metadata = dict(self._metadata)
        out.add_metadata(op='reobserve', length=self.length, length_after=out.length, observables=list(names),
                         effective_sample_size=out.effective_sample_size)
        return out

    def reobserve(self, observe=None, likelihood_funcs=None, likelihood_importance=None):
        """The posterior of the SAME particles under new observed values and / or new likelihoods, without running the inference
        network or drawing anything again (pyprob/distributions/empirical.py:469-544): every name in `observe` or
        `likelihood_funcs` is an observe statement of the program whose term leaves the log-weights (at the original call's
        likelihood_importance) and enters again for the new value under `likelihood_funcs[name](v, trace)` - called ONCE: v has
        name, address, distribution (the program's object, parameters per particle), value (the original one), observed; trace is
        None, so `lambda v, trace: Normal(v.distribution.mean, 0.5)` works as in the reference - or, without a function, under
        the program's own distribution. likelihood_importance scales the new terms (None: the original call's).

        Returns a new device-backed Empirical over the same values tensor: log-weights for ALL particles of the call (one
        pp_is_reobserve_groups call, include/pyprob_amd.h states its formula), particles whose new weight is not finite dropped
        as the call drops them with the full vectors attached. It keeps the statement log - marginal / joint / resample_joint /
        histogram2d / psis answer under the new weights - and its origin with the new values merged, so it can be re-observed
        again. `pareto_k()` of the result says whether the reused particles still cover the new posterior.

        Differences from the reference: it serves Empiricals of Trace objects only, this serves the device-backed result of a
        lock-step posterior_results call (straight-line programs, scalar families; Categorical, Mixture and torch-route
        likelihoods, and branching programs raise NotImplementedError). There a new value without a likelihood function keeps
        the OLD log-prob (:515-527); here every name given is re-scored. As there: if any part of the program is conditional on
        the observed value, the result is not the posterior of the new observation - the replay shows the program the ORIGINAL
        values and nothing is drawn again."""
        self._check_finalized()
        observe = dict(observe or {})
        cols = {k: np.asarray(torch.as_tensor(v, dtype=torch.float32).cpu().numpy(), np.float32).reshape(1, -1)
                for k, v in observe.items()}
        out, names, origin = self._reobserve_weights(cols, 1, likelihood_funcs, likelihood_importance)
        from .is_engine import DistRunner
        stats = DistRunner._stats_dict(self._reobserve_stats(origin, out)[0].cpu().numpy()[0])
        return self._reobserve_result(out[0], stats, origin, observe, names)

    def reweight(self, func, min_index=None, max_index=None):
        """A new Empirical of the values [min_index, max_index) whose log-weights are func(value), one call per value
        (pyprob/distributions/empirical.py:546-566). Host-backed."""
        if self.length == 0:
            return self
        self._check_finalized()
        lo = 0 if min_index is None else int(min_index)
        hi = self.length if max_index is None else int(max_index)
        values = [self._value(i) for i in range(lo, hi)]
        return self._like(values, np.array([float(func(v)) for v in values], np.float64), op='reweight', length=self.length)

    def argsort(self):
        """The indices of the counted particles (finite log-weight, value not NaN) in stable ascending order of value: a device
        int64 tensor for a device-backed Empirical - to gather the other latents of the statement log in value order - and an
        int64 numpy array for every other."""
        self._check_finalized()
        if self.length and self._device_backed():
            _, _, index, counted, _ = self._device_sorted()
            return index[:int(counted[0, 0])].long()
        lw, x = self._host_scalars()
        if x is None:
            raise ValueError('argsort needs scalar values')
        return _host_order(lw, x)

    def combine_duplicates(self):
        """A new Empirical of the DISTINCT values, each under the summed weight of its particles (combine_duplicates,
        empirical.py:809-834), metadata op='combine_duplicates'. The values ASCEND (the reference keeps the order of first
        occurrence); particles without a finite log-weight or with a NaN value are left out; -0.0 and +0.0 are one value.

        A device-backed Empirical gives a device-backed result: the runs of equal values of the sorted particles are reduced on
        the device (pp_is_unique_groups: the histogram's 64-bit fixed point, so the same call gives the same bits) and
        log_weight = log(mass) - S ln 2 + max lw with S = pp_is_hist_shift(length); a value whose whole mass rounds to 0 (below
        2^-S of the heaviest particle) keeps log_weight -inf. Host-backed Empiricals with scalar values do the same in float64
        numpy; values that are not scalars raise the reference's RuntimeError for values that are not hashable."""
        self._check_finalized()
        if self.length and self._device_backed():
            from . import lib as L
            from .ops import ops
            value, lw, _, counted, _ = self._device_sorted()
            uv, mass, _, runs = ops.is_unique_groups(value, lw, counted, self.length, self._group_stats_row())
            r = int(runs[0])
            st = self.__dict__.get('device_stats')
            top = float(st['max_lw']) if st is not None else float(torch.where(torch.isfinite(lw), lw, lw.new_tensor(-math.inf)).max())
            shift = L.load().pp_is_hist_shift(self.length)
            values = uv[0, :r].contiguous()
            new_lw = (torch.log(mass[0, :r].double()) - shift * math.log(2.0) + top).float().contiguous()
            if r == 0:
                out = Empirical(name=self.name)
            else:
                out = Empirical.from_device(values, new_lw, _device_stats(new_lw, values), name=self.name)
                out.__dict__['_fixed_mass'] = (mass[0, :r].contiguous(), shift, top)
            out._metadata = dict(self._metadata)
            out.add_metadata(op='combine_duplicates', length=self.length, length_after=r)
            return out
        vals = self.get_values() if self.length else []
        if not all(isinstance(v, (int, float, np.integer, np.floating)) or (torch.is_tensor(v) and v.numel() == 1) or
                   (isinstance(v, np.ndarray) and v.size == 1) for v in vals):
            raise RuntimeError('The values in this Empirical as not hashable. Combining of duplicates not currently supported.')
        lw = np.asarray(self._lw, np.float64)
        x = np.asarray([float(v) for v in vals], np.float64)
        order = _host_order(lw, x)
        xs, ls = x[order], lw[order]
        heads = np.nonzero(np.concatenate([[True], xs[1:] != xs[:-1]]))[0] if len(order) else np.zeros(0, np.int64)
        top = ls.max() if len(order) else 0.0
        with np.errstate(divide='ignore'):
            new_lw = np.log(np.add.reduceat(np.exp(ls - top), heads)) + top if len(order) else np.zeros(0)
        return self._like([float(v) for v in xs[heads]], new_lw, op='combine_duplicates', length=self.length,
                          length_after=len(heads))

    # ---- density estimate (csrc/is_gmm.hip) ----------------------------------------------------------------------------
    def _skipping_variance(self):
        """The weighted variance over the particles with a finite log-weight only (`variance` on the host multiplies the value of a
        particle without weight by 0: NaN where that value is NaN): the device statistics of a device-backed Empirical - the
        object's own, else reduced here -, float64 numpy for every other."""
        if self._device_backed():
            st = self._device_moments() or _device_stats(self._log_weights, self._values)
            return float(max(st['var'], 0.0))
        lw, x = self._host_scalars()
        keep = np.isfinite(lw)
        if x is None or not keep.any():
            return float('nan')
        w = np.exp(lw[keep] - lw[keep].max())
        mean = np.sum(w * x[keep]) / w.sum()
        return float(np.sum(w * (x[keep] - mean) ** 2) / w.sum())

    def density_estimate(self, num_mixture_components=1, num_samples=None, tol=1e-3, max_iter=100, reg_covar=1e-6,
                         weights_init=None, means_init=None, stddevs_init=None):
        """A Mixture of num_mixture_components (K <= 16) Normals fitted to the weighted values by expectation-maximisation
        (density_estimate, empirical.py:795-807: scikit-learn's GaussianMixture(covariance_type='diag') in one dimension). The
        reference resamples 1000 values and drops the weights; here num_samples=None fits ALL particles under their own weights,
        in float64, by the definition of pp_is_gmm_groups (include/pyprob_amd.h): at most max_iter iterations, converged when the
        weighted mean log-likelihood changes by less than tol; reg_covar is added to every variance. An integer num_samples first
        resamples, as the reference does, on the route resample() takes for this object, and fits the draws.

        The start needs no random numbers: weights 1 / K, means the exact weighted quantiles (k + 1/2) / K (quantile(): the sort is
        kept with the object), variances variance / K^2 + reg_covar. weights_init / means_init / stddevs_init (K numbers each)
        replace each of these; weights_init is taken as given (positive numbers that sum to one).

        The returned Mixture carries `.fit` (MixtureFit): weights, means, stddevs in float64 numpy - the Normals themselves hold
        float32 -, lower_bound, n_iter, converged, count and metadata (op='density_estimate'). A fit that did not converge warns.
        A device-backed Empirical (the result of a lock-step posterior call, post.marginal(address), a device resample, a device
        combine_duplicates) is fitted on the device and 3 K + 6 doubles travel back; every other Empirical, and all of them
        under PP_EMPIRICAL_DEVICE=0, runs the same definition in float64 numpy."""
        self._check_finalized()
        K = _gmm_arguments(num_mixture_components, tol, max_iter, reg_covar)
        if self.length == 0:
            raise ValueError('density_estimate of an empty Empirical')
        if num_samples is not None:
            return self.resample(int(num_samples)).density_estimate(K, None, tol, max_iter, reg_covar, weights_init, means_init,
                                                                    stddevs_init)
        levels = (np.arange(K) + 0.5) / K
        device = self._device_backed()
        if not device:
            lw, x = self._host_scalars()
            if x is None:
                raise ValueError('density_estimate needs scalar values')
        init = _gmm_init_rows(K, reg_covar, weights_init, means_init, stddevs_init,
                              lambda: np.asarray(self.quantile(levels), np.float64)[None], lambda: [self._skipping_variance()])
        if device:
            from .ops import ops
            rows = ops.is_gmm_groups(self._log_weights, self._values, K, self.length, self._group_stats_row(),
                                     torch.from_numpy(init).to(self._log_weights.device), int(max_iter), float(tol),
                                     float(reg_covar)).cpu().numpy()
        else:
            rows = _host_gmm(lw, x, init[0], int(max_iter), float(tol), float(reg_covar))[None]
        return _mixtures_from_rows(rows, K, dict(self._metadata), self.length, tol, max_iter, reg_covar)[0]

    # ---- transformations (each returns a new Empirical) ------------------------------------------------------
    def map(self, func, min_index=None, max_index=None):
        self._check_finalized()
        if self.length == 0:
            return self
        sl = slice(min_index or 0, self.length if max_index is None else max_index)
        return self._like([func(v) for v in self.get_values()[sl]], self._lw[sl], op='map', length=self.length)

    def condition(self, criterion, min_index=None, max_index=None):
        self._check_finalized()
        if self.length == 0:
            return self
        lo, hi = min_index or 0, self.length if max_index is None else max_index
        vals = self.get_values()
        keep = [i for i in range(lo, hi) if criterion(vals[i])]
        return self._like([vals[i] for i in keep], self._lw[keep], op='condition', length=self.length, length_after=len(keep))

    def filter(self, *args, **kwargs):
        warnings.warn('Empirical.filter will be deprecated in future releases. Use Empirical.condition instead.')
        return self.condition(*args, **kwargs)

    def resample(self, num_samples, map_func=None, min_index=None, max_index=None, seed=None, offset=0, scheme='multinomial'):
        """num_samples unweighted draws (empirical.py:617-637).

        A device-backed Empirical (the result of a lock-step posterior call) is resampled on the device: its cumulative weights
        are computed once (pp_is_cdf_groups) and the draws are one launch (pp_is_resample_groups); the result is device-backed
        again, with the statistics of the drawn values reduced on the device, and no list of the particles is built. With
        map_func only the num_samples drawn values travel to the host and the result is host-backed. Draw j uses the Philox
        block of key `seed` and counter `offset + j`; seed=None takes the key from torch's global generator, so pyprob.seed /
        torch.manual_seed reproduce a run. These draws are a DIFFERENT STREAM of the same distribution as the host route's, which
        draws from torch's generator directly, ignores seed / offset, and serves every other Empirical (and all of them under
        PP_EMPIRICAL_DEVICE=0).

        scheme: 'multinomial' (independent draws, the reference's), 'stratified' (draw j at position (j + u_j) / num_samples of
        the mass, one uniform per draw) or 'systematic' ((j + u) / num_samples, ONE uniform for all draws: counter `offset`,
        stream 0x53) - pp_is_resample_scheme_groups, the same single launch. The two low-variance schemes return the particles in
        index order and every particle floor(n w) or ceil(n w) times (systematic; stratified within 2); the metadata names a
        scheme other than the default."""
        self._check_finalized()
        _scheme_id(scheme)
        if self._device_backed():
            if int(num_samples) < 1:
                raise ValueError('num_samples must be positive')
            ess = self.effective_sample_size
            drawn = self._device_draw(num_samples, min_index, max_index, seed, offset, scheme)
            if map_func is not None:
                out = [map_func(v) for v in drawn.cpu().unbind(0)]
                return self._like(out, np.zeros(len(out)), **_resample_meta(self.length, num_samples, ess, scheme))
            zeros = torch.zeros_like(drawn)
            return self._resampled(drawn, zeros, _device_stats(zeros, drawn), num_samples, ess, scheme)
        ess = self.effective_sample_size
        idx = self._draw_indices(int(num_samples), min_index, max_index, scheme)
        vals = self.get_values()
        out = [vals[i] if map_func is None else map_func(vals[i]) for i in idx]
        return self._like(out, np.zeros(len(out)), **_resample_meta(self.length, num_samples, ess, scheme))

    def thin(self, num_samples, map_func=None, min_index=None, max_index=None):
        self._check_finalized()
        lo, hi = min_index or 0, self.length if max_index is None else max_index
        step = max(1, math.floor((hi - lo) / num_samples))
        idx = list(range(lo, hi, step))
        vals = self.get_values()
        out = [vals[i] if map_func is None else map_func(vals[i]) for i in idx]
        return self._like(out, self._lw[idx], op='thin', length=self.length, num_samples=int(num_samples), step=int(step))

    def unweighted(self):
        return self._like(list(self.get_values()), np.zeros(self.length), op='discard_weights')

    # ---- reductions ------------------------------------------------------------------------------------------
    def expectation(self, func):
        """sum_i w_i func(x_i) (empirical.py:451-466). func is tried on the whole value array (numpy, then a torch tensor
        for functions like torch.sin) before falling back to one call per value."""
        self._check_finalized()
        v = self.values_numpy()
        for conv in ((lambda a: a), torch.from_numpy):
            try:
                fv = func(conv(v))
                fv = np.asarray(fv.detach().cpu() if torch.is_tensor(fv) else fv, np.float64)
                if fv.shape == v.shape:
                    return float(np.sum(self._w * fv))
            except Exception:   # noqa: BLE001 - func works on one value at a time, or on the other array type
                pass
        return float(np.sum(self._w * np.asarray([float(func(x)) for x in self.get_values()])))

    def _device_moments(self):
        st = self.__dict__.get('device_stats')
        # ONE source of truth per object: while the values live on the device the float64 device statistics answer mean /
        # variance / ESS - also after something (weights_numpy, sampling, slicing) materialised the host-side weights, so the
        # same property returns the same number whatever was called before
        return st if (st is not None and torch.is_tensor(self._values)) else None

    @property
    def mean(self):
        st = self._device_moments()
        if st is not None:
            return float(st['mean'])
        return float(np.sum(self._w * self.values_numpy()))

    @property
    def variance(self):
        st = self._device_moments()
        if st is not None:
            return float(max(st['var'], 0.0))
        v = self.values_numpy()
        return float(np.sum(self._w * (v - self.mean) ** 2))

    @property
    def stddev(self):
        return math.sqrt(self.variance)

    @property
    def skewness(self):
        v = self.values_numpy()
        return float(np.sum(self._w * ((v - self.mean) / self.stddev) ** 3))

    @property
    def kurtosis(self):
        v = self.values_numpy()
        return float(np.sum(self._w * ((v - self.mean) / self.stddev) ** 4))

    @property
    def effective_sample_size(self):
        st = self._device_moments()
        if st is not None:
            return float(st['ess'])
        return float(1.0 / np.sum(self._w ** 2))

    @property
    def mode(self):
        """Highest-weight value; with uniform weights the most frequent (hashable) value (empirical.py:693-712)."""
        self._check_finalized()
        if self._uniform:
            counts = {}
            for v in self.get_values():
                k = float(v) if torch.is_tensor(v) and v.numel() == 1 else v
                counts[k] = counts.get(k, 0) + 1
            return max(counts.items(), key=lambda kv: kv[1])[0]
        return self._value(int(np.argmax(self._lw)))

    @property
    def median(self):
        self._check_finalized()
        if self._uniform:
            v = self._values
            if torch.is_tensor(v) or (len(v) and torch.is_tensor(v[0])):
                # tensor values: torch.median, the LOWER of the two middle values of an even count (empirical.py:719-721)
                return float(np.sort(self.values_numpy())[(self.length - 1) // 2])
            return float(np.median(self.values_numpy()))       # :723-724
        return self.resample(1000).median           # empirical.py:727

    def _device_extent(self):
        """(min, max, counted, NaN values) of a device-backed Empirical from pp_is_extent_groups (computed once per object: four
        doubles travel, not the particles), or None where the kernel did not look at every particle (it skips those without a
        finite log-weight, numpy.min over the values does not)."""
        ext = self.__dict__.get('_dev_extent')
        if ext is None:
            from .ops import ops
            ext = self.__dict__['_dev_extent'] = ops.is_extent_groups(self._log_weights, self._values, self.length).cpu().numpy()[0]
        return ext if int(ext[2]) + int(ext[3]) == self.length else None

    @property
    def min(self):
        ext = self._device_extent() if self._device_backed() else None
        if ext is not None:
            return float('nan') if ext[3] else float(ext[0])
        return float(np.min(self.values_numpy()))

    @property
    def max(self):
        ext = self._device_extent() if self._device_backed() else None
        if ext is not None:
            return float('nan') if ext[3] else float(ext[1])
        return float(np.max(self.values_numpy()))

    def arg_max(self, map_func):
        vals = self.get_values()
        return vals[int(np.argmax([float(map_func(v)) for v in vals]))]

    def arg_min(self, map_func):
        vals = self.get_values()
        return vals[int(np.argmin([float(map_func(v)) for v in vals]))]

    def __repr__(self):
        try:
            return 'Empirical(items:{}, weighted:{}, mean:{}, stddev:{})'.format(self.length, self.weighted, self.mean, self.stddev)
        except Exception:   # noqa: BLE001 - values that are not scalars
            return 'Empirical(items:{})'.format(self.length)


_STATS_SCRATCH = {}
_REOBSERVE_RUNNERS = {}      # device -> the DistRunner of Empirical.reobserve's replays


def _device_stats_row(lw, x):
    """pp_is_stats over (lw, x): the row of doubles on the device (the scratch is kept per device)."""
    from . import lib as L
    from .ops import ops
    scratch = _STATS_SCRATCH.get(lw.device)
    if scratch is None:
        scratch = _STATS_SCRATCH[lw.device] = torch.zeros(L.PP_IS_STATS_SCRATCH, dtype=torch.float64, device=lw.device)
    return ops.is_stats(lw, x, scratch)


def _device_stats(lw, x):
    """pp_is_stats over (lw, x) as the dict Empirical.from_device takes (one small device-to-host copy)."""
    from .is_engine import DistRunner
    return DistRunner._stats_dict(_device_stats_row(lw, x))


class JointMoments:
    """First and second moments of J latents over one weighted particle set (Empirical.joint): addresses, mean [J], cov [J, J],
    corr [J, J], stddev [J] (float64 numpy), ess = (sum w)^2 / sum w^2 and count = the particles with a finite log-weight."""

    def __init__(self, addresses, mean, cov, corr, stddev, ess, count):
        self.addresses = list(addresses)
        self.mean, self.cov, self.corr, self.stddev = mean, cov, corr, stddev
        self.ess, self.count = float(ess), int(count)

    def __repr__(self):
        return 'JointMoments(addresses:{}, count:{}, ess:{:.2f}, mean:{})'.format(self.addresses, self.count, self.ess,
                                                                                  self.mean.tolist())


def _joint_rows(addresses, rows):
    """The M output rows of pp_is_moments_groups (max lw, W, sum w^2, count | c_j | S_j | Q_jk for j <= k) as M JointMoments, all
    groups in one pass of array arithmetic (the same operations per element whatever M is: a group's numbers do not depend on the
    groups next to it): mean_j = c_j + S_j / W, cov_jk = Q_jk / W - (S_j / W)(S_k / W) with the diagonal clamped at 0 like
    Empirical.variance, stddev = sqrt(diagonal), corr = cov / sqrt(var_j var_k). A group without a weight: NaN arrays, ess 0."""
    J = len(addresses)
    rows = np.asarray(rows, np.float64).reshape(-1, 4 + 2 * J + J * (J + 1) // 2)
    W, W2, count = rows[:, 1], rows[:, 2], rows[:, 3]
    ok = (count > 0) & (W > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        Wd = np.where(ok, W, np.nan)[:, None]
        s = rows[:, 4 + J:4 + 2 * J] / Wd
        mean = rows[:, 4:4 + J] + s
        iu, ku = np.triu_indices(J)
        cov = np.empty((rows.shape[0], J, J))
        cov[:, iu, ku] = rows[:, 4 + 2 * J:] / Wd
        cov[:, ku, iu] = cov[:, iu, ku]
        cov -= s[:, :, None] * s[:, None, :]
        d = np.arange(J)
        var = cov[:, d, d]
        var = np.where(var < 0, 0.0, var)       # (NaN stays NaN)
        cov[:, d, d] = var
        stddev = np.sqrt(var)
        corr = cov / np.sqrt(var[:, :, None] * var[:, None, :])
        ess = np.where(ok, W * W / np.where(ok, W2, 1.0), 0.0)
    return [JointMoments(addresses, mean[g], cov[g], corr[g], stddev[g], ess[g], count[g]) for g in range(rows.shape[0])]


def joint_from_moments(addresses, row):
    """One output row of pp_is_moments_groups as a JointMoments (see _joint_rows)."""
    return _joint_rows(addresses, np.asarray(row, np.float64)[None])[0]


def _moment_rows(lw, cols, n_per, stats):
    """numpy [M, PP_IS_MOMENTS_WIDTH(J)] of pp_is_moments_groups over the J columns: one launch and one copy up to 16 columns;
    beyond that blocks of 8 columns, one call per pair of blocks, the rows assembled on the host."""
    from . import lib as L
    from .ops import ops
    J = len(cols)
    if J <= L.PP_IS_MOMENTS_MAX_COLS:
        return ops.is_moments_groups(lw, list(cols), int(n_per), stats).cpu().numpy()
    half = L.PP_IS_MOMENTS_MAX_COLS // 2
    blocks = [list(range(b, min(J, b + half))) for b in range(0, J, half)]
    pairs = [(a, b) for a in range(len(blocks)) for b in range(a + 1, len(blocks))]
    parts = torch.cat([ops.is_moments_groups(lw, [cols[j] for j in blocks[a] + blocks[b]], int(n_per), stats)
                       for a, b in pairs], 1).cpu().numpy()
    M = parts.shape[0]
    out = np.zeros((M, L.PP_IS_MOMENTS_WIDTH(J)))
    where = {}
    e = 4 + 2 * J
    for j in range(J):
        for k in range(j, J):
            where[(j, k)] = e
            e += 1
    at = 0
    for a, b in pairs:
        idx = blocks[a] + blocks[b]
        n = len(idx)
        part = parts[:, at:at + L.PP_IS_MOMENTS_WIDTH(n)]
        at += L.PP_IS_MOMENTS_WIDTH(n)
        out[:, :4] = part[:, :4]
        q = 4 + 2 * n
        for u in range(n):
            out[:, 4 + idx[u]], out[:, 4 + J + idx[u]] = part[:, 4 + u], part[:, 4 + n + u]
            for v in range(u, n):
                out[:, where[(idx[u], idx[v])]] = part[:, q]
                q += 1
    return out


_HIST_MAX_BINS = 2048      # PP_IS_HIST_MAX_BINS (include/pyprob_amd.h)


class Histogram:
    """A weighted 1-D histogram of one weighted particle set (Empirical.histogram), float64 numpy: edges [bins + 1], mass [bins]
    (the posterior weight of every bin: mass.sum() + below + above + nan == 1), density = mass / bin width, count [bins] (int64:
    the particles per bin), below / above (the weight left and right of the edges; -inf and +inf values sit there), nan (the
    weight of the particles whose value is NaN) and particles (those with a finite log-weight, binned or not). A group without
    weight: NaN arrays and particles == 0."""

    def __init__(self, edges, mass, count, below, above, nan, particles):
        self.edges, self.mass, self.count = edges, mass, count
        self.below, self.above, self.nan, self.particles = float(below), float(above), float(nan), int(particles)
        self.density = mass / np.diff(edges)

    def cdf(self):
        """The cumulative posterior mass AT every edge [bins + 1]: cdf()[0] == below, cdf()[-1] == 1 - above - nan."""
        return self.below + np.concatenate([[0.0], np.cumsum(self.mass)])

    def quantile(self, q):
        """The value below which a fraction q of the posterior mass lies, for a scalar or an array q in [0, 1]: the cumulative
        mass interpolated linearly INSIDE the bin it crosses q in (the leftmost such point where bins are empty). Its resolution
        is the bin width: the histogram does not know where in a bin its particles sit. Mass below or above the edges is not
        resolved at all: a quantile that falls there is edges[0] / edges[-1], with a RuntimeWarning (so is one beyond 1 - nan)."""
        qs = np.asarray(q, np.float64)
        if np.any((qs < 0) | (qs > 1)):
            raise ValueError('quantiles lie in [0, 1]')
        if self.particles == 0:
            return float('nan') if qs.ndim == 0 else np.full(qs.shape, np.nan)
        c = self.cdf()
        k = np.searchsorted(c, qs, side='left')      # the first edge whose cumulative mass reaches q
        outside = (qs < c[0]) | (qs > c[-1] + 1e-12)      # (1e-12: the cumulative sum of all the mass is 1 to rounding only)
        if np.any(outside):
            warnings.warn('quantile outside the histogram\'s edges (mass below {:.3g}, above {:.3g}, NaN {:.3g}): the edge is '
                          'returned'.format(self.below, self.above, self.nan), RuntimeWarning, stacklevel=2)
        kk = np.clip(k, 1, len(c) - 1)
        step = c[kk] - c[kk - 1]
        with np.errstate(divide='ignore', invalid='ignore'):
            frac = np.where(step > 0, (qs - c[kk - 1]) / np.where(step > 0, step, 1.0), 0.0)
        out = self.edges[kk - 1] + np.clip(frac, 0.0, 1.0) * (self.edges[kk] - self.edges[kk - 1])
        out = np.where(k == 0, self.edges[0], np.where(k > len(c) - 1, self.edges[-1], out))
        return float(out) if qs.ndim == 0 else out

    def credible_interval(self, level=0.9):
        """The equal-tailed interval (quantile((1 - level) / 2), quantile((1 + level) / 2))."""
        if not 0 < level < 1:
            raise ValueError('level lies in (0, 1)')
        return self.quantile((1.0 - level) / 2.0), self.quantile((1.0 + level) / 2.0)

    @property
    def mode(self):
        """The centre of the bin of highest density (the first of equals)."""
        if self.particles == 0 or not np.isfinite(self.density).any():
            return float('nan')
        b = int(np.nanargmax(self.density))
        return float(0.5 * (self.edges[b] + self.edges[b + 1]))

    def __repr__(self):
        return 'Histogram(bins:{}, range:[{}, {}], particles:{}, below:{:.3g}, above:{:.3g}, nan:{:.3g})'.format(
            len(self.mass), self.edges[0], self.edges[-1], self.particles, self.below, self.above, self.nan)


class Histogram2D:
    """A weighted 2-D histogram of two latents of one weighted particle set (Empirical.histogram2d), float64 numpy: addresses,
    x_edges [bx + 1], y_edges [by + 1], mass [bx, by] (mass.sum() + outside + nan == 1), density = mass / bin area, count [bx, by]
    (int64), outside (the weight with either coordinate out of its range), nan (either coordinate NaN) and particles."""

    def __init__(self, addresses, x_edges, y_edges, mass, count, outside, nan, particles):
        self.addresses = list(addresses)
        self.x_edges, self.y_edges, self.mass, self.count = x_edges, y_edges, mass, count
        self.outside, self.nan, self.particles = float(outside), float(nan), int(particles)
        self.density = mass / (np.diff(x_edges)[:, None] * np.diff(y_edges)[None, :])

    def __repr__(self):
        return 'Histogram2D(addresses:{}, bins:{}x{}, particles:{}, outside:{:.3g}, nan:{:.3g})'.format(
            self.addresses, self.mass.shape[0], self.mass.shape[1], self.particles, self.outside, self.nan)


def _check_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= _HIST_MAX_BINS:
        raise ValueError('bins must be an integer in 1 .. %d, not %r' % (_HIST_MAX_BINS, bins))


def _check_edges(e):
    """edges [.., bins + 1] in float64: finite and strictly increasing along the last axis, at most 2048 bins."""
    if e.shape[-1] < 2 or e.shape[-1] - 1 > _HIST_MAX_BINS:
        raise ValueError('edges must hold 2 .. %d values (at most %d bins)' % (_HIST_MAX_BINS + 1, _HIST_MAX_BINS))
    if not np.isfinite(e).all() or not (np.diff(e, axis=-1) > 0).all():
        raise ValueError('edges must be finite and strictly increasing (a range too narrow for its number of bins in float64 is not)')
    return e


def _auto_range(ext):
    """(lo [M], hi [M]) from rows of (min, max, counted, NaN values): the finite extent; nothing counted: (0, 1) as numpy takes for
    no data; lo == hi: widened by 0.5 on either side as numpy does."""
    ext = np.asarray(ext, np.float64).reshape(-1, 4)
    none = ext[:, 2] == 0
    lo, hi = np.where(none, 0.0, ext[:, 0]), np.where(none, 1.0, ext[:, 1])
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError('the extent of the values is not finite (an infinite value under a finite weight): pass range=(lo, hi)')
    same = lo == hi
    return np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)


def _linspace_rows(lo, hi, bins):
    """numpy.linspace(lo[g], hi[g], bins + 1) for every g as [M, bins + 1]: one vectorised call where that is the same arithmetic
    (numpy switches formula for ALL rows when any step is zero)."""
    if np.all((hi - lo) / bins != 0):
        return np.ascontiguousarray(np.linspace(lo, hi, bins + 1, axis=-1))
    return np.stack([np.linspace(a, b, bins + 1) for a, b in zip(lo, hi)])


def _hist_edges_for(bins, range, edges, extent):
    """The edges [M, bins + 1] (M = 1 unless `extent` returns more rows) of histogram(bins, range, edges); extent() is called only
    where the range has to be found."""
    if edges is not None:
        e = np.array(edges, np.float64)
        if e.ndim != 1:
            raise ValueError('edges must be one-dimensional')
        return _check_edges(e)[None]
    _check_bins(bins)
    if range is None:
        lo, hi = _auto_range(extent())
    else:
        lo, hi = (float(v) for v in range)
        if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
            raise ValueError('range must be finite with lo <= hi, not %r' % (range,))
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        lo, hi = np.asarray([lo]), np.asarray([hi])
    return _check_edges(_linspace_rows(lo, hi, int(bins)))


def _histogram_rows(edges, rows, exact=True):
    """M Histograms from edges [1 or M, bins + 1] and rows [M, 2, bins + 3] (masses | counts over bins, below, above, NaN): the
    rows of pp_is_hist_groups (exact: fixed point - a slot's mass is slot / total, total = the exact integer sum of the row) or
    float64 sums of the host route. The same elementwise arithmetic whatever M is."""
    rows = np.asarray(rows)
    M, bins = rows.shape[0], rows.shape[2] - 3
    fixed = rows[:, 0, :]
    total = fixed.sum(1)        # (int64 for the device rows: at most 2^62, exact)
    ok = total > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        mass = np.where(ok[:, None], fixed.astype(np.float64) / np.where(ok, total, 1).astype(np.float64)[:, None], np.nan)
    count = rows[:, 1, :].astype(np.int64)
    particles = np.where(ok, count.sum(1), 0)
    return [Histogram(edges[g if edges.shape[0] > 1 else 0], mass[g, :bins], count[g, :bins], mass[g, bins], mass[g, bins + 1],
                      mass[g, bins + 2], particles[g]) for g in np.arange(M)]


def _histogram2d_row(addresses, ex, ey, row):
    bx, by = len(ex) - 1, len(ey) - 1
    fixed, count = row[0], row[1].astype(np.int64)
    total = int(fixed.sum())
    mass = fixed.astype(np.float64) / float(total) if total > 0 else np.full(fixed.shape, np.nan)
    return Histogram2D(addresses, ex, ey, mass[:bx * by].reshape(bx, by), count[:bx * by].reshape(bx, by), mass[bx * by],
                       mass[bx * by + 1], int(count.sum()) if total > 0 else 0)


def _device_histograms(lw, x, n_per, bins, range, edges, stats):
    """The Histograms of the M groups of n_per particles of (lw, x) on the device: pp_is_extent_groups and a copy of [M, 4] where
    the range has to be found, pp_is_hist_groups (edges shared by the groups, or one row per group from its own extent) and a copy
    of the rows."""
    from .ops import ops
    e = _hist_edges_for(bins, range, edges, lambda: ops.is_extent_groups(lw, x, int(n_per)).cpu().numpy())
    dev = torch.from_numpy(e if e.shape[0] > 1 else e[0]).to(lw.device)
    return _histogram_rows(e, ops.is_hist_groups(lw, x, None, int(n_per), dev, None, stats).cpu().numpy())


class PsisFit:
    """What Empirical.psis fitted: khat (the shape of the generalised Pareto tail with the paper's weak prior; +inf: no fit), sigma
    (its scale, in units of the largest weight), tail (the particles above the cutoff, ties with it excluded), grid (the points of
    the profile), log_cutoff (the log-weight of the cutoff particle), count (the particles with a finite log-weight), ess_before
    and ess_after."""

    def __init__(self, khat, sigma, tail, grid, log_cutoff, count, ess_before, ess_after):
        self.khat, self.sigma, self.tail, self.grid = float(khat), float(sigma), int(tail), int(grid)
        self.log_cutoff, self.count = float(log_cutoff), int(count)
        self.ess_before, self.ess_after = float(ess_before), float(ess_after)

    def __repr__(self):
        return 'PsisFit(khat:{}, sigma:{}, tail:{}, ess_before:{}, ess_after:{})'.format(self.khat, self.sigma, self.tail,
                                                                                         self.ess_before, self.ess_after)


PSIS_KHAT_THRESHOLD = 0.7


def _psis_fit(row, ess_before, ess_after):
    """The PsisFit of a row of pp_is_psis_groups' out, with psis()'s warning."""
    fit = PsisFit(row[0], row[1], row[2], row[3], row[5], row[6], ess_before, ess_after)
    if fit.khat == float('inf'):
        warnings.warn('Pareto smoothing: no tail could be fitted to the {} particles with a finite log-weight (k-hat = inf): the '
                      'weights are unchanged'.format(fit.count), UserWarning)
    elif not fit.khat <= PSIS_KHAT_THRESHOLD:
        warnings.warn('Pareto smoothing: k-hat = {:.3f} is above {}: the importance-sampling estimates of this posterior are '
                      'unreliable (their variance is practically or literally infinite)'.format(fit.khat, PSIS_KHAT_THRESHOLD),
                      UserWarning)
    return fit


def _psis_tail(tail):
    """The `tail` argument of pp_is_psis_groups: 0 (the rule) for None, else a positive integer."""
    if tail is None:
        return 0
    if isinstance(tail, bool) or not isinstance(tail, (int, np.integer)) or not 1 <= int(tail) <= 2 ** 31 - 1:
        raise ValueError('tail must be a positive integer or None (the rule min(c / 5, 3 sqrt(c))), not %r' % (tail,))
    return int(tail)


_GMM_MAX_K = 16      # PP_IS_GMM_MAX_K (include/pyprob_amd.h)


class MixtureFit:
    """What Empirical.density_estimate fitted, in float64 numpy: weights [K], means [K], stddevs [K]; lower_bound (the weighted mean
    log-likelihood of the last E-step), n_iter, converged, count (the particles with a finite log-weight) and metadata."""

    def __init__(self, weights, means, stddevs, lower_bound, n_iter, converged, count, metadata):
        self.weights, self.means, self.stddevs = weights, means, stddevs
        self.lower_bound, self.n_iter, self.converged, self.count = float(lower_bound), int(n_iter), bool(converged), int(count)
        self.metadata = metadata

    def __repr__(self):
        return 'MixtureFit(components:{}, n_iter:{}, converged:{}, lower_bound:{})'.format(len(self.weights), self.n_iter,
                                                                                           self.converged, self.lower_bound)


def _gmm_arguments(num_mixture_components, tol, max_iter, reg_covar):
    K = num_mixture_components
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= _GMM_MAX_K:
        raise ValueError('num_mixture_components must be an integer in 1 .. %d, not %r' % (_GMM_MAX_K, K))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
        raise ValueError('max_iter must be a positive integer, not %r' % (max_iter,))
    if not float(tol) >= 0 or not float(reg_covar) >= 0:
        raise ValueError('tol and reg_covar must not be negative')
    return int(K)


def _gmm_init_rows(K, reg_covar, weights_init, means_init, stddevs_init, quantiles, variances):
    """The initial parameters [M, 3 K] (weights | means | variances, float64) of density_estimate: the overrides where given (one
    row of K numbers, shared by the groups), else 1 / K, quantiles() = [M, K] and variances() = [M] / K^2 + reg_covar - each
    called only where its default is needed."""
    def override(a, name):
        a = np.asarray(a, np.float64).reshape(-1)
        if a.shape != (K,) or not np.isfinite(a).all():
            raise ValueError('%s must hold %d finite numbers' % (name, K))
        return a[None]
    mu = override(means_init, 'means_init') if means_init is not None else np.asarray(quantiles(), np.float64).reshape(-1, K)
    if stddevs_init is not None:
        v = override(stddevs_init, 'stddevs_init') ** 2
    else:
        v = np.asarray(variances(), np.float64).reshape(-1, 1) / float(K * K) + float(reg_covar) + np.zeros((1, K))
    pi = override(weights_init, 'weights_init') if weights_init is not None else np.full((1, K), 1.0 / K)
    if not (pi > 0).all():
        raise ValueError('weights_init must be positive')
    M = max(mu.shape[0], v.shape[0])
    if not (v[np.isfinite(v)] > 0).all():
        raise ValueError('the initial variances must be positive (constant values need reg_covar > 0 or stddevs_init)')
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(a, (M, K)) for a in (pi, mu, v)], 1))


def _mixtures_from_rows(rows, K, metadata, length, tol, max_iter, reg_covar):
    """The output rows [M, 3 K + 6] of pp_is_gmm_groups as M Mixtures of Normals, each with its MixtureFit as `.fit`. metadata: one
    dict, or one per row. The float32 parameters of all M K Normals are converted in one pass (a batched call builds hundreds)."""
    from .distributions import Mixture, Normal      # (the families' module re-exports this one: not at import time)
    rows = np.asarray(rows, np.float64).reshape(-1, 3 * K + 6)
    M = rows.shape[0]
    pi, mu, sd = rows[:, :K].copy(), rows[:, K:2 * K].copy(), np.sqrt(rows[:, 2 * K:3 * K])
    if not (rows[:, 3 * K + 4] > 0).all():
        raise ValueError('density_estimate: no particle with a finite log-weight')
    if not (np.isfinite(pi).all() and np.isfinite(mu).all() and np.isfinite(sd).all()):
        raise ValueError('density_estimate: the fit is not finite (a value that is not finite under a finite log-weight?)')
    for row in rows[rows[:, 3 * K + 2] == 0]:
        warnings.warn('density_estimate did not converge in {} iterations (last lower bound {}): raise max_iter or tol, or '
                      'check the initial parameters'.format(int(row[3 * K + 1]), row[3 * K]), RuntimeWarning, stacklevel=3)
    loc = torch.from_numpy(mu.astype(np.float32)).reshape(-1).unbind(0)
    scale = torch.from_numpy(sd.astype(np.float32)).reshape(-1).unbind(0)
    probs = torch.from_numpy(pi.astype(np.float32)).unbind(0)
    out = []
    for g in range(M):
        meta = dict(metadata if isinstance(metadata, dict) else metadata[g])
        meta.update(op='density_estimate', length=int(length), num_mixture_components=K, tol=float(tol), max_iter=int(max_iter),
                    reg_covar=float(reg_covar))
        mix = Mixture([Normal(loc[g * K + k], scale[g * K + k]) for k in range(K)], probs[g])
        mix.fit = MixtureFit(pi[g], mu[g], sd[g], rows[g, 3 * K], rows[g, 3 * K + 1], rows[g, 3 * K + 2], rows[g, 3 * K + 4], meta)
        out.append(mix)
    return out
