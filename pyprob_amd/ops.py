"""PyTorch-ROCm custom operators over the C ABI (SURVEY.md §8b seam B3): `torch.ops.pyprob_hip.*`.

Each operator is a thin wrapper over ONE `extern "C"` entry point of libpyprob_amd.so (include/pyprob_amd.h): it checks
shapes / dtypes / contiguity / device, passes the tensors' device pointers and torch's current HIP stream, and turns a
non-zero return code into a RuntimeError. All buffers are PyTorch-owned tensors (caching allocator); the kernels never
allocate. Only the device ("CUDA" dispatch key = HIP on ROCm) implementation exists in the product: calling an operator
with CPU tensors fails in the dispatcher - there is no CPU fallback. (The CPU test-suite registers oracle-backed "CPU"
kernels for these operators from tests/, to execute the host logic above them without a GPU.)

    ic_loss      InferenceNetworkLSTM._loss (+ backward)            pyprob/nn/inference_network_lstm.py:136-220
    adam_step    optim.Adam.step over the flat buffer                pyprob/nn/inference_network.py:348,496
    sgd_step     optim.SGD(momentum, nesterov).step                  pyprob/nn/inference_network.py:350
    larc_scale   the LARC wrapper's gradient rescaling               pyprob/nn/optimizer_larc.py:72-107
    is_init      InferenceNetwork._infer_init                        pyprob/nn/inference_network.py:141-148
    is_step      _infer_step + proposal.sample() + log_prob          pyprob/nn/inference_network_lstm.py:82-134,
    is_step_rows   (the same for the rows of a diverged path, state in place)
                                                                     pyprob/state.py:207-212
    log_prob     prior / likelihood log_prob terms of the log-weight pyprob/state.py:211, 147-149
    dist_logweight  the log-weight terms of every distribution family   pyprob/state.py:113-115, 147-149, 211
    dist_draw       draws of every distribution family (Philox)       pyprob/state.py:191-201, 218-221
    mix_logweight   Mixture.log_prob as a log-weight term               pyprob/distributions/mixture.py:38-45
    obs_draw        the synthetic observation block of n prior traces   pyprob/nn/dataset.py:50-62, state.py observe branch
    obs_logweight   the summed log-density of a vector-valued observe    pyprob/state.py:118-155, trace.py:123-125
    obs_logweight_groups  the same for the M N rows of a batched call, operands per particle or per group
    mix_draw        Mixture.sample (component selection + draw, Philox) pyprob/distributions/mixture.py:47-63
    is_cdf_groups       Empirical.finalize's weights as a running sum per group  pyprob/distributions/empirical.py:298-309
    is_resample_groups  Empirical.sample / resample: multinomial draws (Philox)   pyprob/distributions/empirical.py:392-408, 617-637
    is_resample_scheme_groups  the same with stratified / systematic positions (one launch)   pyprob/distributions/empirical.py:617-637
    is_moments_groups   weighted first and second moments of several latents per group   pyprob/distributions/empirical.py:298-309, 451-466, 668-690
    is_hist_groups      weighted 1-D / 2-D histogram of a latent (pair) per group, fixed point   pyprob/distributions/empirical.py:298-309, 889-914
    is_extent_groups    minimum, maximum and NaN count of a latent per group             pyprob/distributions/empirical.py:770-794
    is_sort_groups      the particles of every group in order of value (stable radix sort)   pyprob/distributions/empirical.py:714-728, 809-834
    is_quantile_groups  exact weighted quantiles over the sorted particles (inverted cdf)     pyprob/distributions/empirical.py:714-728
    is_unique_groups    distinct values with fixed-point masses and counts (combine_duplicates)   pyprob/distributions/empirical.py:809-834
    is_hpd_groups       highest-posterior-density interval over the sorted particles (the reference has none)   pyprob/distributions/empirical.py:668-728
    is_ecdf_groups      the posterior cdf at points given per group (the reference has none)      pyprob/distributions/empirical.py:668-728
    is_psis_groups      Pareto-smoothed importance weights and k-hat per group (the reference has none)   pyprob/distributions/empirical.py:758-766
    is_gmm_groups       weighted Gaussian-mixture EM of a latent per group (density_estimate)     pyprob/distributions/empirical.py:795-807
    reobserve_groups    the particles of one call re-scored under M new observations (reobserve)  pyprob/distributions/empirical.py:469-544

Non-tensor state travels as follows: the network description (`pp_net`, host struct with offsets into the flat
parameter buffer) is registered once per layer set with `register_net` and referenced by an integer handle; the
host-side arrays of a packed minibatch (`pp_batch.n_active / row_off / grp_off / nxt_off`) travel as one small CPU int32
tensor next to the device buffer (`PackedBatch.op_tensors`).
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L

NAMESPACE = 'pyprob_hip'

_lib = torch.library.Library(NAMESPACE, 'DEF')
_lib.define('ic_loss(Tensor params, Tensor(a!) grads, Tensor(b!) workspace, Tensor batch_dev, Tensor batch_host, int net, '
            'int flags) -> (Tensor, Tensor, Tensor)')
_lib.define('adam_step(Tensor(a!) params, Tensor(b!) grads, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, Tensor chunk_tensor, '
            'Tensor active, Tensor(e!) tensor_step, Tensor(f!) scratch, float lr, float beta1, float beta2, float eps, '
            'float weight_decay, float grad_scale, int flags, Tensor? skip) -> ()')
_lib.define('sgd_step(Tensor(a!) params, Tensor(b!) grads, Tensor(c!) momentum_buf, Tensor chunk_tensor, Tensor active, float lr, '
            'float momentum, bool nesterov, float weight_decay, float grad_scale, int flags, Tensor? skip) -> ()')
_lib.define('larc_scale(Tensor params, Tensor(a!) grads, Tensor chunk_tensor, Tensor active, float lr, float weight_decay, '
            'float grad_scale, float trust_coefficient, float eps, float epsilon, bool clip, Tensor(b!) scratch, Tensor? skip) -> ()')
_lib.define('is_init(Tensor params, Tensor(a!) workspace, int net, Tensor obs) -> Tensor')
_lib.define('is_step(Tensor params, Tensor(a!) workspace, int net, int addr_id, int prev_addr_id, int n, Tensor e_obs, '
            'Tensor? prev_value, Tensor? prior, Tensor(b!) h, Tensor(c!) c, int state_rows, Tensor? value_in, int seed, '
            'int offset) -> (Tensor, Tensor)')
_lib.define('is_step_rows(Tensor params, Tensor(a!) workspace, int net, int addr_id, int prev_addr_id, int n, Tensor e_obs, '
            'Tensor prev_value, Tensor? prior, Tensor(b!) h, Tensor(c!) c, int state_rows, Tensor rows, Tensor? value_in, int seed, '
            'int offset) -> (Tensor, Tensor)')
_lib.define('is_statement_rows(Tensor params, Tensor(a!) workspace, int net, int addr_id, int prev_addr_id, int n, Tensor e_obs, '
            'Tensor prev_value_full, Tensor prior, Tensor(b!) h, Tensor(c!) c, int state_rows, Tensor? rows, Tensor(d!) value_full, '
            'Tensor(e!) lw_full, int prior_kind, int seed, int offset) -> ()')
_lib.define('is_step_net(Tensor params, Tensor(a!) workspace, int net, int addr_id, int prev_addr_id, int n, Tensor e_obs, '
            'Tensor? prev_value, Tensor(b!) h, Tensor(c!) c, int state_rows) -> ()')
_lib.define('is_fused(Tensor(a!) workspace, int net, int addr_id, Tensor? prior, int[] kinds, Tensor?[] p0, int[] p0_strides, '
            'Tensor?[] p1, int[] p1_strides, Tensor?[] x, float[] scales, int[] flags, Tensor(b!) value, Tensor(c!) lw, '
            'bool overwrite, int seed, int offset, Tensor(d!)? stats_scratch) -> Tensor')
_lib.define('prior_draw(int kind, Tensor p0, Tensor p1, int n, int seed, int offset, int stream_id) -> Tensor')
_lib.define('obs_draw(int kind, Tensor p0, Tensor p1, int n, int k, int seed, int offset, int stream_id) -> Tensor')
_lib.define('obs_logweight(Tensor(a!)? lw, int kind, Tensor?[] params, Tensor x, int k, float scale, Tensor? rows, '
            'Tensor(b!)? lp_out, int n) -> ()')
_lib.define('obs_logweight_groups(Tensor(a!)? lw, int kind, Tensor?[] params, Tensor x, int per_group, int k, float scale, '
            'Tensor(b!)? lp_out, int n_groups, int n_per) -> ()')
_lib.define('log_prob(int kind, Tensor p0, int p0_stride, Tensor? p1, int p1_stride, Tensor x, int n) -> Tensor')
_lib.define('logweight_terms(Tensor(a!) lw, int[] kinds, Tensor?[] p0, int[] p0_strides, Tensor?[] p1, int[] p1_strides, '
            'Tensor[] x, float[] scales, bool overwrite) -> ()')
_lib.define('is_stats(Tensor lw, Tensor? x, Tensor(a!) scratch) -> Tensor')
_lib.define('is_cdf_groups(Tensor lw, int n_per, Tensor? stats) -> Tensor')
_lib.define('is_resample_groups(Tensor cdf, Tensor? values, int n_per, int lo, int hi, int n_out, int seed, int offset, '
            'bool want_index) -> (Tensor, Tensor)')
_lib.define('is_resample_scheme_groups(Tensor cdf, Tensor? values, int n_per, int lo, int hi, int n_out, int scheme, int seed, '
            'int offset, bool want_index) -> (Tensor, Tensor)')
_lib.define('is_moments_groups(Tensor lw, Tensor[] cols, int n_per, Tensor? stats) -> Tensor')
_lib.define('is_hist_groups(Tensor lw, Tensor x, Tensor? y, int n_per, Tensor edges_x, Tensor? edges_y, Tensor? stats) -> Tensor')
_lib.define('is_extent_groups(Tensor lw, Tensor x, int n_per) -> Tensor')
_lib.define('is_sort_groups(Tensor lw, Tensor x, int n_per, Tensor? stats) -> (Tensor, Tensor, Tensor, Tensor)')
_lib.define('is_quantile_groups(Tensor value_sorted, Tensor cdf_sorted, Tensor counted, int n_per, Tensor q) -> Tensor')
_lib.define('is_unique_groups(Tensor value_sorted, Tensor lw_sorted, Tensor counted, int n_per, Tensor? stats) -> '
            '(Tensor, Tensor, Tensor, Tensor)')
_lib.define('is_hpd_groups(Tensor value_sorted, Tensor cdf_sorted, Tensor counted, int n_per, Tensor level) -> (Tensor, Tensor)')
_lib.define('is_ecdf_groups(Tensor value_sorted, Tensor cdf_sorted, Tensor counted, int n_per, Tensor x, bool strict) -> '
            '(Tensor, Tensor)')
_lib.define('is_psis_groups(Tensor lw_sorted, Tensor index_sorted, Tensor counted, int n_per, Tensor? stats, int tail, '
            'bool want_weights) -> (Tensor?, Tensor)')
_lib.define('is_gmm_groups(Tensor lw, Tensor x, int n_components, int n_per, Tensor? stats, Tensor params_init, int max_iter, '
            'float tol, float reg_covar) -> Tensor')
_lib.define('reobserve_groups(Tensor lw, Tensor? old, int[] kinds, int[] ks, float[] scales, Tensor?[] params, Tensor[] xs, '
            'int n_groups) -> Tensor')
_lib.define('dist_logweight(Tensor(a!)? lw, int[] kinds, Tensor?[] params, int[] strides, Tensor[] x, float[] scales, Tensor? rows, '
            'Tensor(b!)? lp_out, int n) -> ()')
_lib.define('dist_draw(int kind, Tensor?[] params, int[] strides, Tensor? rows, Tensor(a!) out, int seed, int offset, '
            'int stream_id) -> ()')
_lib.define('mix_logweight(Tensor(a!)? lw, int[] kinds, Tensor?[] params, int[] strides, Tensor probs, Tensor x, float scale, '
            'Tensor? rows, Tensor(b!)? lp_out, int n) -> ()')
_lib.define('mix_draw(int[] kinds, Tensor?[] params, int[] strides, Tensor probs, Tensor? rows, Tensor(a!) out, int seed, int offset, '
            'int stream_id) -> ()')

# ---- network registry -------------------------------------------------------------------------------------------
_NETS = {}
_next_handle = [1]


def register_net(net_struct, spec):
    """Make a pp_net (ctypes struct built by NetSpec.c_struct) addressable from operator calls. Returns the handle."""
    h = _next_handle[0]
    _next_handle[0] += 1
    _NETS[h] = (net_struct, spec)
    return h


def unregister_net(handle):
    _NETS.pop(handle, None)


def net_struct(handle):
    return _NETS[handle][0]


def net_spec(handle):
    return _NETS[handle][1]


# ---- packed batch <-> (device buffer, host int32 descriptor) --------------------------------------------------------
BH_FIXED = 16
_BH_COLS = ('obs', 'value', 'prior', 'addr', 'prev_row', 'grp_rows', 'trace', 'row_off_dev', 'nxt_rows')


def batch_descriptor(n_traces, n_rows, t_max, obs_width, n_addr, offsets, n_active, row_off, grp_off, nxt_off):
    """CPU int32 tensor: [B, R, T, obs_width, n_addr, 9 word offsets into the device buffer (pp_batch device columns in
    _BH_COLS order), pad to 16 | n_active [T] | row_off [T+1] | grp_off [n_addr+1] | nxt_off [n_addr+1]]."""
    head = np.zeros(BH_FIXED, np.int32)
    head[:5] = (n_traces, n_rows, t_max, obs_width, n_addr)
    head[5:5 + len(_BH_COLS)] = [offsets[k] for k in _BH_COLS]
    arr = np.concatenate([head, np.asarray(n_active, np.int32), np.asarray(row_off, np.int32),
                          np.asarray(grp_off, np.int32), np.asarray(nxt_off, np.int32)])
    return torch.from_numpy(arr)


def _batch_struct(batch_dev, batch_host):
    bh = batch_host.numpy()
    B, R, T, W, A = (int(v) for v in bh[:5])
    if bh.size != BH_FIXED + T + (T + 1) + 2 * (A + 1):
        raise RuntimeError('pyprob_hip: malformed batch descriptor')
    c = L.pp_batch()
    c.n_traces, c.n_rows, c.t_max, c.obs_width = B, R, T, W
    base = batch_dev.data_ptr()
    for i, k in enumerate(_BH_COLS):
        setattr(c, k, base + 4 * int(bh[5 + i]))
    ip = C.POINTER(C.c_int32)
    o = BH_FIXED
    host = np.ascontiguousarray(bh[o:], np.int32)          # kept alive by the caller until the C call returns
    p = host.ctypes.data
    c.n_active = C.cast(p, ip)
    c.row_off = C.cast(p + 4 * T, ip)
    c.grp_off = C.cast(p + 4 * (2 * T + 1), ip)
    c.nxt_off = C.cast(p + 4 * (2 * T + 1 + A + 1), ip)
    return c, host, (B, R, T, W, A)


def _f32(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError('pyprob_hip: %s must be a contiguous float32 tensor' % name)
    return t


def _same_device(ref, *tensors):
    for t in tensors:
        if t is not None and t.device != ref.device:
            raise RuntimeError('pyprob_hip: tensors on different devices (%s, %s)' % (ref.device, t.device))


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


# ---- device implementations ("CUDA" dispatch key = HIP) ---------------------------------------------------------------
def _ic_loss_hip(params, grads, workspace, batch_dev, batch_host, net, flags):
    lib = L.load()
    netc = net_struct(net)
    _f32(params, 'params')
    _same_device(params, grads, workspace, batch_dev)
    if params.numel() < netc.n_params:
        raise RuntimeError('pyprob_hip::ic_loss: parameter buffer smaller than the network (%d < %d)'
                           % (params.numel(), netc.n_params))
    bwd = bool(flags & L.PP_LOSS_BACKWARD)
    if bwd and (_f32(grads, 'grads').numel() < netc.n_params):
        raise RuntimeError('pyprob_hip::ic_loss: gradient buffer smaller than the network')
    c, keep, (B, R, T, W, A) = _batch_struct(batch_dev, batch_host)
    need = lib.pp_ic_workspace_bytes(C.byref(netc), B, R)
    ws_bytes = workspace.numel() * workspace.element_size()
    if need == 0 or ws_bytes < need:
        raise RuntimeError('pyprob_hip::ic_loss: workspace too small (%d < %d bytes)' % (ws_bytes, need))
    loss = torch.empty(1, dtype=torch.float32, device=params.device)
    status = torch.zeros(1, dtype=torch.int32, device=params.device)
    lp = torch.empty(R if (flags & L.PP_LOSS_KEEP_LP) else 0, dtype=torch.float32, device=params.device)
    with torch.cuda.device(params.device):
        rc = lib.pp_ic_loss(C.byref(netc), C.byref(c), params.data_ptr(), grads.data_ptr() if bwd else None,
                            workspace.data_ptr(), ws_bytes, loss.data_ptr(), status.data_ptr(),
                            lp.data_ptr() if lp.numel() else None, int(flags), _stream(params))
    L.check(rc, 'pp_ic_loss')
    del keep
    return loss, status, lp


def _adam_step_hip(params, grads, exp_avg, exp_avg_sq, chunk_tensor, active, tensor_step, scratch, lr, beta1, beta2, eps,
                   weight_decay, grad_scale, flags, skip):
    lib = L.load()
    n = params.numel()
    for t, name in ((params, 'params'), (grads, 'grads'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq'), (active, 'active')):
        _f32(t, name)
    _same_device(params, grads, exp_avg, exp_avg_sq, chunk_tensor, active, tensor_step, scratch, skip)
    if min(grads.numel(), exp_avg.numel(), exp_avg_sq.numel()) < n or chunk_tensor.numel() * 1024 != n:
        raise RuntimeError('pyprob_hip::adam_step: buffer sizes do not match the parameter buffer')
    n_tensors = tensor_step.numel()
    if active.numel() < n_tensors or scratch.numel() < L.PP_ADAM_SCRATCH * n_tensors:
        raise RuntimeError('pyprob_hip::adam_step: per-tensor arrays too small')
    with torch.cuda.device(params.device):
        rc = lib.pp_adam_step(params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
                              chunk_tensor.data_ptr(), active.data_ptr(), tensor_step.data_ptr(), scratch.data_ptr(),
                              n_tensors, lr, beta1, beta2, eps, weight_decay, grad_scale, int(flags), L.ptr(skip),
                              _stream(params))
    L.check(rc, 'pp_adam_step')


def _sgd_step_hip(params, grads, momentum_buf, chunk_tensor, active, lr, momentum, nesterov, weight_decay, grad_scale, flags, skip):
    lib = L.load()
    n = params.numel()
    for t, name in ((params, 'params'), (grads, 'grads'), (momentum_buf, 'momentum_buf'), (active, 'active')):
        _f32(t, name)
    _same_device(params, grads, momentum_buf, chunk_tensor, active, skip)
    if min(grads.numel(), momentum_buf.numel()) < n or chunk_tensor.numel() * 1024 != n:
        raise RuntimeError('pyprob_hip::sgd_step: buffer sizes do not match the parameter buffer')
    with torch.cuda.device(params.device):
        rc = lib.pp_sgd_step(params.data_ptr(), grads.data_ptr(), momentum_buf.data_ptr(), n, chunk_tensor.data_ptr(),
                             active.data_ptr(), active.numel(), lr, momentum, int(bool(nesterov)), weight_decay, grad_scale,
                             int(flags), L.ptr(skip), _stream(params))
    L.check(rc, 'pp_sgd_step')


def _larc_scale_hip(params, grads, chunk_tensor, active, lr, weight_decay, grad_scale, trust_coefficient, eps, epsilon, clip,
                    scratch, skip):
    lib = L.load()
    n = params.numel()
    for t, name in ((params, 'params'), (grads, 'grads'), (active, 'active'), (scratch, 'scratch')):
        _f32(t, name)
    _same_device(params, grads, chunk_tensor, active, scratch, skip)
    if grads.numel() < n or chunk_tensor.numel() * 1024 != n:
        raise RuntimeError('pyprob_hip::larc_scale: buffer sizes do not match the parameter buffer')
    if scratch.numel() < L.larc_scratch_floats(n, active.numel()):
        raise RuntimeError('pyprob_hip::larc_scale: scratch too small')
    with torch.cuda.device(params.device):
        rc = lib.pp_larc_scale(params.data_ptr(), grads.data_ptr(), n, chunk_tensor.data_ptr(), active.data_ptr(),
                               active.numel(), lr, weight_decay, grad_scale, trust_coefficient, eps, epsilon, int(bool(clip)),
                               scratch.data_ptr(), L.ptr(skip), _stream(params))
    L.check(rc, 'pp_larc_scale')


def _is_ws(lib, netc, workspace, n):
    need = lib.pp_is_workspace_bytes(C.byref(netc), n)
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise RuntimeError('pyprob_hip: importance-sampling workspace too small (%d < %d bytes)' % (have, need))
    return have


def _is_init_hip(params, workspace, net, obs):
    lib = L.load()
    netc = net_struct(net)
    _same_device(params, workspace, obs)
    ws_bytes = _is_ws(lib, netc, workspace, 1)
    if _f32(obs, 'obs').numel() != sum(netc.obs_in[o] for o in range(netc.n_obs)):
        raise RuntimeError('pyprob_hip::is_init: observe has %d values, the network expects %d'
                           % (obs.numel(), sum(netc.obs_in[o] for o in range(netc.n_obs))))
    e = torch.zeros(netc.e_obs + 8, dtype=torch.float32, device=params.device)
    with torch.cuda.device(params.device):
        rc = lib.pp_is_init(C.byref(netc), params.data_ptr(), obs.data_ptr(), e.data_ptr(), workspace.data_ptr(), ws_bytes,
                            _stream(params))
    L.check(rc, 'pp_is_init')
    return e


def _is_step_hip(params, workspace, net, addr_id, prev_addr_id, n, e_obs, prev_value, prior, h, c, state_rows, value_in, seed,
                 offset, rows=None):
    lib = L.load()
    netc = net_struct(net)
    _same_device(params, workspace, e_obs, prev_value, prior, h, c, value_in)
    ws_bytes = _is_ws(lib, netc, workspace, n)
    if not (0 <= addr_id < netc.n_addr) or prev_addr_id >= netc.n_addr:
        raise RuntimeError('pyprob_hip::is_step: address id out of range')
    H = netc.lstm_dim
    depth = max(1, int(netc.lstm_depth))
    if rows is not None:
        if rows.dtype != torch.int64 or not rows.is_contiguous() or rows.numel() < n or rows.device != params.device:
            raise RuntimeError('pyprob_hip::is_step_rows: rows must be a contiguous int64 device tensor with n entries')
        if not lib.pp_is_step_fused_supported(C.byref(netc), int(addr_id), 1 << 30) or prev_addr_id < 0:
            raise RuntimeError('pyprob_hip::is_step_rows: no fused statement kernel for this network / statement')
    elif H > 0 and (h.numel() < depth * n * H or c.numel() < depth * n * H):
        raise RuntimeError('pyprob_hip::is_step: LSTM state smaller than [depth, n, H]')
    stride = 0
    if prior is not None:
        _f32(prior, 'prior')
        stride = 0 if prior.numel() == 2 else 1
        if stride and prior.numel() < 2 * n:
            raise RuntimeError('pyprob_hip::is_step: prior must be [1, 2] or [n, 2]')
    for t, name in ((prev_value, 'prev_value'), (value_in, 'value_in')):
        if t is not None and _f32(t, name).numel() < n:
            raise RuntimeError('pyprob_hip::is_step: %s shorter than n' % name)
    value = torch.empty(n, dtype=torch.float32, device=params.device)
    logq = torch.empty(n, dtype=torch.float32, device=params.device)
    with torch.cuda.device(params.device):
        if rows is None:
            rc = lib.pp_is_step(C.byref(netc), params.data_ptr(), int(addr_id), int(prev_addr_id), int(n), e_obs.data_ptr(),
                                L.ptr(prev_value), L.ptr(prior), stride, L.ptr(h), L.ptr(c), int(state_rows), L.ptr(value_in),
                                value.data_ptr(), logq.data_ptr(), int(seed), int(offset), workspace.data_ptr(), ws_bytes,
                                _stream(params))
        else:
            rc = lib.pp_is_step_rows(C.byref(netc), params.data_ptr(), int(addr_id), int(prev_addr_id), int(n), e_obs.data_ptr(),
                                     L.ptr(prev_value), L.ptr(prior), stride, L.ptr(h), L.ptr(c), int(state_rows),
                                     rows.data_ptr(), L.ptr(value_in), value.data_ptr(), logq.data_ptr(), int(seed), int(offset),
                                     workspace.data_ptr(), ws_bytes, _stream(params))
    L.check(rc, 'pp_is_step')
    return value, logq


def _is_step_rows_hip(params, workspace, net, addr_id, prev_addr_id, n, e_obs, prev_value, prior, h, c, state_rows, rows, value_in,
                      seed, offset):
    return _is_step_hip(params, workspace, net, addr_id, prev_addr_id, n, e_obs, prev_value, prior, h, c, state_rows, value_in,
                        seed, offset, rows=rows)


def _is_statement_rows_hip(params, workspace, net, addr_id, prev_addr_id, n, e_obs, prev_value_full, prior, h, c, state_rows, rows,
                           value_full, lw_full, prior_kind, seed, offset):
    """pp_is_statement_rows: the whole statement (previous values by row, draw, value scatter, log-weight update) in one launch."""
    lib = L.load()
    netc = net_struct(net)
    _same_device(params, workspace, e_obs, prev_value_full, prior, h, c, rows, value_full, lw_full)
    ws_bytes = _is_ws(lib, netc, workspace, n)
    if not (0 <= addr_id < netc.n_addr) or not (0 <= prev_addr_id < netc.n_addr):
        raise RuntimeError('pyprob_hip::is_statement_rows: address id out of range')
    if rows is not None and (rows.dtype != torch.int64 or not rows.is_contiguous() or rows.numel() < n):
        raise RuntimeError('pyprob_hip::is_statement_rows: rows must be a contiguous int64 tensor with n entries')
    for t, name in ((prev_value_full, 'prev_value_full'), (value_full, 'value_full'), (lw_full, 'lw_full')):
        if _f32(t, name).numel() < n:
            raise RuntimeError('pyprob_hip::is_statement_rows: %s shorter than n' % name)
    stride = 0 if _f32(prior, 'prior').numel() == 2 else 1
    if stride and prior.numel() < 2 * n:
        raise RuntimeError('pyprob_hip::is_statement_rows: prior must be [1, 2] or [n, 2]')
    with torch.cuda.device(params.device):
        rc = lib.pp_is_statement_rows(C.byref(netc), params.data_ptr(), int(addr_id), int(prev_addr_id), int(n), e_obs.data_ptr(),
                                      prev_value_full.data_ptr(), prior.data_ptr(), stride, h.data_ptr(), c.data_ptr(), int(state_rows),
                                      L.ptr(rows), value_full.data_ptr(), lw_full.data_ptr(), int(prior_kind), int(seed), int(offset),
                                      workspace.data_ptr(), ws_bytes, _stream(params))
    L.check(rc, 'pp_is_statement_rows')


def _is_step_net_hip(params, workspace, net, addr_id, prev_addr_id, n, e_obs, prev_value, h, c, state_rows):
    lib = L.load()
    netc = net_struct(net)
    _same_device(params, workspace, e_obs, prev_value, h, c)
    ws_bytes = _is_ws(lib, netc, workspace, n)
    if not (0 <= addr_id < netc.n_addr) or prev_addr_id >= netc.n_addr:
        raise RuntimeError('pyprob_hip::is_step_net: address id out of range')
    with torch.cuda.device(params.device):
        rc = lib.pp_is_step_net(C.byref(netc), params.data_ptr(), int(addr_id), int(prev_addr_id), int(n), e_obs.data_ptr(),
                                L.ptr(prev_value), L.ptr(h), L.ptr(c), int(state_rows), workspace.data_ptr(), ws_bytes,
                                _stream(params))
    L.check(rc, 'pp_is_step_net')


def _is_fused_hip(workspace, net, addr_id, prior, kinds, p0, p0_strides, p1, p1_strides, x, scales, flags, value, lw, overwrite,
                  seed, offset, stats_scratch):
    lib = L.load()
    netc = net_struct(net)
    count = len(kinds)
    n = value.numel()
    _same_device(value, lw, workspace, prior, stats_scratch)
    if _f32(lw, 'lw').numel() != n or not value.is_contiguous() or not lw.is_contiguous():
        raise RuntimeError('pyprob_hip::is_fused: value and lw must be contiguous float32 vectors of one length')
    arr = (L.pp_lw_term * max(count, 1))()
    fl = (C.c_int32 * max(count, 1))()
    for q in range(count):
        _same_device(value, p0[q], p1[q], x[q])
        for t, what in ((p0[q], 'p0'), (p1[q], 'p1'), (x[q], 'x')):
            # a term tensor is one shared value or one value per particle (Categorical: one probability row or n rows); a
            # k-element tensor with k != n (a vector-valued observation) would be read at the particle index
            if t is not None and int(kinds[q]) != 5 and t.numel() not in (1, n):
                raise RuntimeError('pyprob_hip::is_fused: term %d: %s has %d elements (1 or n = %d)' % (q, what, t.numel(), n))
        arr[q].kind = int(kinds[q])
        arr[q].p0, arr[q].p1, arr[q].x = L.ptr(p0[q]), L.ptr(p1[q]), L.ptr(x[q])
        arr[q].p0_stride, arr[q].p1_stride = int(p0_strides[q]), int(p1_strides[q])
        arr[q].x_stride = 0 if (x[q] is None or x[q].numel() == 1) else 1
        arr[q].scale = float(scales[q])
        fl[q] = int(flags[q])
    out = torch.empty(8, dtype=torch.float64, device=value.device)      # (the combine kernel writes the six statistics)
    if stats_scratch is not None and (stats_scratch.dtype != torch.float64 or stats_scratch.numel() < L.PP_IS_STATS_SCRATCH):
        raise RuntimeError('pyprob_hip::is_fused: scratch must hold PP_IS_STATS_SCRATCH doubles')
    with torch.cuda.device(value.device):
        rc = lib.pp_is_fused(C.byref(netc), int(addr_id), n, L.ptr(prior), arr, fl, count, value.data_ptr(), lw.data_ptr(),
                             1 if overwrite else 0, int(seed), int(offset), out.data_ptr() if stats_scratch is not None else None,
                             L.ptr(stats_scratch), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                             _stream(value))
    L.check(rc, 'pp_is_fused')
    return out


def _prior_draw_hip(kind, p0, p1, n, seed, offset, stream_id):
    lib = L.load()
    _same_device(p0, p1)
    out = torch.empty(n, dtype=torch.float32, device=p0.device)
    for t, name in ((p0, 'p0'), (p1, 'p1')):
        if _f32(t, name).numel() not in (1, n):
            raise RuntimeError('pyprob_hip::prior_draw: %s must have 1 or n elements' % name)
    with torch.cuda.device(p0.device):
        rc = lib.pp_prior_draw(int(kind), p0.data_ptr(), 0 if p0.numel() == 1 else 1, p1.data_ptr(), 0 if p1.numel() == 1 else 1,
                               int(n), int(seed), int(offset), int(stream_id) & 0xFFFFFFFF, out.data_ptr(), _stream(p0))
    L.check(rc, 'pp_prior_draw')
    return out


def obs_draw_strides(t, n, k, name='p', what='obs_draw'):
    """(row stride, element stride) with which pp_obs_draw / pp_obs_logweight read an operand of n rows of k values: a scalar (one
    element) -> (0, 0); [k] or [1, k] - one row shared by all rows -> (0, 1); [n] or [n, 1] - one value per row -> (1, 0);
    [n, k] -> (k, 1). A 1-D tensor of k elements is the shared row also when n == k (callers pass per-row values as [n, 1]).
    For `obs_logweight` only (obs_draw's accepted shapes are what they were): a contiguous [n, *event] whose trailing dimensions
    flatten to k (an image per row: [n, C, H, W]) -> (k, 1), and a 2-D [n, k] view with unit element stride and a row stride
    above k (a padded block) -> (that row stride, 1). Every other tensor has to be contiguous."""
    shape = tuple(t.shape)
    wide = what == 'obs_logweight'
    if wide and shape == (n, k) and not t.is_contiguous() and t.stride(1) == 1 and t.stride(0) >= k:
        return t.stride(0), 1
    if wide and not t.is_contiguous():
        raise RuntimeError('pyprob_hip::%s: %s must be contiguous (or a [n, k] view with padded rows)' % (what, name))
    if t.numel() == 1:
        return 0, 0
    if shape in ((k,), (1, k)):
        return 0, 1
    if shape in ((n,), (n, 1)):
        return 1, 0
    if shape == (n, k) or (wide and len(shape) > 2 and shape[0] == n and t.numel() == n * k):
        return k, 1
    raise RuntimeError('pyprob_hip::%s: %s must be a scalar, [k], [n], [n, 1] or [n, k] (n = %d, k = %d), got %s'
                       % (what, name, n, k, list(shape)))


def _obs_draw_hip(kind, p0, p1, n, k, seed, offset, stream_id):
    lib = L.load()
    _same_device(p0, p1)
    n, k = int(n), int(k)
    if n < 0 or k < 1:
        raise RuntimeError('pyprob_hip::obs_draw: n >= 0 rows of k >= 1 values, got n = %d, k = %d' % (n, k))
    (r0, e0), (r1, e1) = obs_draw_strides(_f32(p0, 'p0'), n, k, 'p0'), obs_draw_strides(_f32(p1, 'p1'), n, k, 'p1')
    out = torch.empty((n, k), dtype=torch.float32, device=p0.device)
    with torch.cuda.device(p0.device):
        rc = lib.pp_obs_draw(int(kind), p0.data_ptr(), r0, e0, p1.data_ptr(), r1, e1, n, k, int(seed), int(offset),
                             int(stream_id) & 0xFFFFFFFF, out.data_ptr(), _stream(p0))
    L.check(rc, 'pp_obs_draw')
    return out


def _obs_logweight_hip(lw, kind, params, x, k, scale, rows, lp_out, n):
    lib = L.load()
    n, k = int(n), int(k)
    if len(params) != 4:
        raise RuntimeError('pyprob_hip::obs_logweight: 4 parameter slots')
    ref = lw if lw is not None else lp_out
    if ref is None:
        raise RuntimeError('pyprob_hip::obs_logweight: lw or lp_out is needed')
    for t, name in ((lw, 'lw'), (lp_out, 'lp_out')):
        if t is not None and (_f32(t, name).numel() != n):
            raise RuntimeError('pyprob_hip::obs_logweight: %s must have n = %d elements' % (name, n))
    _same_device(ref, lw, lp_out, rows, x, *params)
    if n < 0 or k < 1:
        raise RuntimeError('pyprob_hip::obs_logweight: n >= 0 rows of k >= 1 values, got n = %d, k = %d' % (n, k))

    def operand(o, t, name):
        if t.dtype != torch.float32:
            raise RuntimeError('pyprob_hip: %s must be a float32 tensor' % name)
        rs, es = obs_draw_strides(t, n, k, name, 'obs_logweight')
        o.p, o.row_stride, o.elem_stride = t.data_ptr(), int(rs), int(es)
    arr = (L.pp_obs_operand * 4)()
    for q in range(4):
        if params[q] is not None:
            operand(arr[q], params[q], 'p%d' % q)
    xo = L.pp_obs_operand()
    operand(xo, x, 'x')
    rp, m = _rows_arg(rows, n, 'obs_logweight')
    with torch.cuda.device(ref.device):
        rc = lib.pp_obs_logweight(int(kind), arr, xo, k, float(scale), L.ptr(lw), L.ptr(lp_out), rp, int(m), n, _stream(ref))
    L.check(rc, 'pp_obs_logweight')


def obs_group_operands(params, x, per_group, n_groups, n_per, k):
    """The five operands (params[0..3], x) of pp_obs_logweight_groups as (tensor, row stride, element stride) or None: an operand
    whose bit is set in per_group (bit q < 4: params[q], bit 4: x) holds one row per GROUP and is classified by obs_draw_strides with
    n = n_groups rows ([M, k], [M, *event], a padded [M, k] view, [M, 1], or a shape shared by all rows); every other one with
    n = n_groups * n_per rows."""
    out = []
    for q, t in enumerate(list(params) + [x]):
        if t is None:
            out.append(None)
            continue
        name = 'x' if q == 4 else 'p%d' % q
        if t.dtype != torch.float32:
            raise RuntimeError('pyprob_hip: %s must be a float32 tensor' % name)
        rows = n_groups if (per_group >> q) & 1 else n_groups * n_per
        rs, es = obs_draw_strides(t, rows, k, name, 'obs_logweight')
        out.append((t, int(rs), int(es)))
    return out


def _obs_logweight_groups_hip(lw, kind, params, x, per_group, k, scale, lp_out, n_groups, n_per):
    lib = L.load()
    n_groups, n_per, k, per_group = int(n_groups), int(n_per), int(k), int(per_group)
    if len(params) != 4:
        raise RuntimeError('pyprob_hip::obs_logweight_groups: 4 parameter slots')
    ref = lw if lw is not None else lp_out
    if ref is None:
        raise RuntimeError('pyprob_hip::obs_logweight_groups: lw or lp_out is needed')
    if n_groups < 0 or n_per < 1 or k < 1 or not 0 <= per_group <= 31:
        raise RuntimeError('pyprob_hip::obs_logweight_groups: n_groups >= 0 groups of n_per >= 1 rows of k >= 1 values and a mask '
                           'of bits 0-4, got n_groups = %d, n_per = %d, k = %d, per_group = %d' % (n_groups, n_per, k, per_group))
    n = n_groups * n_per
    for t, name in ((lw, 'lw'), (lp_out, 'lp_out')):
        if t is not None and (_f32(t, name).numel() != n):
            raise RuntimeError('pyprob_hip::obs_logweight_groups: %s must have n_groups n_per = %d elements' % (name, n))
    _same_device(ref, lw, lp_out, x, *params)
    operands = obs_group_operands(params, x, per_group, n_groups, n_per, k)
    arr = (L.pp_obs_operand * 4)()
    xo = L.pp_obs_operand()
    for q, o in enumerate(operands):
        if o is not None:
            dst = xo if q == 4 else arr[q]
            dst.p, dst.row_stride, dst.elem_stride = o[0].data_ptr(), o[1], o[2]
    with torch.cuda.device(ref.device):
        rc = lib.pp_obs_logweight_groups(int(kind), arr, xo, per_group, k, float(scale), L.ptr(lw), L.ptr(lp_out), n_groups, n_per,
                                         _stream(ref))
    L.check(rc, 'pp_obs_logweight_groups')


def _reobserve_groups_hip(lw, old, kinds, ks, scales, params, xs, n_groups):
    """out [n_groups, N] of pp_is_reobserve_groups: term t has kind kinds[t], ks[t] values per observe, the parameter slots
    params[4 t .. 4 t + 3] with rows by particle (a scalar, [k], [N] / [N, 1] or [N, k]: obs_draw_strides over N rows) and the new
    values xs[t] with rows by group ([n_groups, k], or one element / [1, k]: the same for every group)."""
    lib = L.load()
    n_groups, T = int(n_groups), len(kinds)
    N = int(_f32(lw, 'lw').numel())
    if not 1 <= T <= L.PP_REOBS_MAX_TERMS or len(ks) != T or len(scales) != T or len(xs) != T or len(params) != 4 * T:
        raise RuntimeError('pyprob_hip::reobserve_groups: 1..%d terms with a kind, k, scale, x and 4 parameter slots each'
                           % L.PP_REOBS_MAX_TERMS)
    if n_groups < 0 or N < 1 or lw.dim() != 1 or not lw.is_contiguous():
        raise RuntimeError('pyprob_hip::reobserve_groups: n_groups >= 0 and a contiguous lw [N], N >= 1')
    if old is not None and (_f32(old, 'old').numel() != N or not old.is_contiguous()):
        raise RuntimeError('pyprob_hip::reobserve_groups: old must be a contiguous [N] like lw')
    _same_device(lw, old, *params, *xs)
    arr = (L.pp_reobs_term * T)()

    def operand(o, t, rows, k, name):
        if t.dtype != torch.float32:
            raise RuntimeError('pyprob_hip: %s must be a float32 tensor' % name)
        rs, es = obs_draw_strides(t, rows, k, name, 'obs_logweight')
        o.p, o.row_stride, o.elem_stride = t.data_ptr(), int(rs), int(es)
    for t in range(T):
        k = int(ks[t])
        if k < 1:
            raise RuntimeError('pyprob_hip::reobserve_groups: k >= 1 values per observe, got %d' % k)
        arr[t].kind, arr[t].k, arr[t].scale = int(kinds[t]), k, float(scales[t])
        for q in range(4):
            if params[4 * t + q] is not None:
                operand(arr[t].params[q], params[4 * t + q], N, k, 'term %d p%d' % (t, q))
        x = xs[t]
        if x.dim() != 2 or x.shape[1] != k or x.shape[0] not in (1, n_groups):
            raise RuntimeError('pyprob_hip::reobserve_groups: x of term %d must be [n_groups, k] or [1, k] (n_groups = %d, k = %d), '
                               'got %s' % (t, n_groups, k, list(x.shape)))
        operand(arr[t].x, x, int(x.shape[0]), k, 'term %d x' % t)
        if x.shape[0] == 1:
            arr[t].x.row_stride = 0
    out = torch.empty((n_groups, N), dtype=torch.float32, device=lw.device)
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_reobserve_groups(arr, T, lw.data_ptr(), L.ptr(old), out.data_ptr(), n_groups, N, _stream(lw))
    L.check(rc, 'pp_is_reobserve_groups')
    return out


def _log_prob_hip(kind, p0, p0_stride, p1, p1_stride, x, n):
    lib = L.load()
    _same_device(x, p0, p1)
    lp = torch.empty(n, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.pp_logweight_accumulate(int(kind), _f32(p0, 'p0').data_ptr(), int(p0_stride), L.ptr(p1), int(p1_stride),
                                         _f32(x, 'x').data_ptr(), 0 if x.numel() == 1 else 1, 1.0, None, lp.data_ptr(), int(n),
                                         _stream(x))
    L.check(rc, 'pp_logweight_accumulate')
    return lp


def _logweight_terms_hip(lw, kinds, p0, p0_strides, p1, p1_strides, x, scales, overwrite):
    lib = L.load()
    count = len(kinds)
    arr = (L.pp_lw_term * count)()
    for q in range(count):
        _same_device(lw, p0[q], p1[q], x[q])
        arr[q].kind = int(kinds[q])
        arr[q].p0, arr[q].p1, arr[q].x = L.ptr(p0[q]), L.ptr(p1[q]), x[q].data_ptr()
        arr[q].p0_stride, arr[q].p1_stride = int(p0_strides[q]), int(p1_strides[q])
        arr[q].x_stride = 0 if x[q].numel() == 1 else 1
        arr[q].scale = float(scales[q])
    with torch.cuda.device(lw.device):
        rc = lib.pp_logweight_terms(arr, count, _f32(lw, 'lw').data_ptr(), lw.numel(), 1 if overwrite else 0, _stream(lw))
    L.check(rc, 'pp_logweight_terms')


def _dist_fill(d, kind, params, strides, q, n, what):
    """pp_dist `d` from the 4 parameters / strides of term q (include/pyprob_amd.h: pointer + stride 0 shared / 1 per particle;
    Categorical: p0 = probability row(s) with the row stride in strides[0] and C in strides[1])."""
    d.kind = int(kind)
    for k in range(4):
        t, st = params[4 * q + k], int(strides[4 * q + k])
        if t is not None:
            _f32(t, '%s p%d' % (what, k))
            need = 1 if st == 0 else (n * st if kind == 5 else n)
            if kind == 5 and k == 0:
                need = int(strides[4 * q + 1]) if st == 0 else n * st
            if t.numel() < need:
                raise RuntimeError('pyprob_hip::%s: term %d parameter %d has %d elements, %d needed' % (what, q, k, t.numel(), need))
        d.p[k] = L.ptr(t)
        d.p_stride[k] = st


def _rows_arg(rows, n, what):
    if rows is None:
        return None, n
    if rows.dtype != torch.int64 or not rows.is_contiguous() or rows.dim() != 1:
        raise RuntimeError('pyprob_hip::%s: rows must be a contiguous int64 vector' % what)
    return rows.data_ptr(), rows.numel()


def _dist_logweight_hip(lw, kinds, params, strides, x, scales, rows, lp_out, n):
    lib = L.load()
    count = len(kinds)
    if not 1 <= count <= L.PP_DIST_MAX_TERMS or len(params) != 4 * count or len(strides) != 4 * count or len(x) != count \
            or len(scales) != count:
        raise RuntimeError('pyprob_hip::dist_logweight: 1..%d terms, 4 parameters and strides per term' % L.PP_DIST_MAX_TERMS)
    ref = lw if lw is not None else lp_out
    if ref is None:
        raise RuntimeError('pyprob_hip::dist_logweight: lw or lp_out is needed')
    for t, name in ((lw, 'lw'), (lp_out, 'lp_out')):
        if t is not None and (_f32(t, name).numel() != n):
            raise RuntimeError('pyprob_hip::dist_logweight: %s must have n = %d elements' % (name, n))
    _same_device(ref, lw, lp_out, rows, *params, *x)
    arr = (L.pp_dist_term * count)()
    for q in range(count):
        _dist_fill(arr[q].d, kinds[q], params, strides, q, n, 'dist_logweight')
        if _f32(x[q], 'x').numel() not in (1, n):
            raise RuntimeError('pyprob_hip::dist_logweight: x of term %d must have 1 or n elements' % q)
        arr[q].x = x[q].data_ptr()
        arr[q].x_stride = 0 if x[q].numel() == 1 else 1
        arr[q].scale = float(scales[q])
    rp, m = _rows_arg(rows, n, 'dist_logweight')
    with torch.cuda.device(ref.device):
        rc = lib.pp_dist_logweight(arr, count, L.ptr(lw), L.ptr(lp_out), rp, int(m), int(n), _stream(ref))
    L.check(rc, 'pp_dist_logweight')


def _dist_draw_hip(kind, params, strides, rows, out, seed, offset, stream_id):
    lib = L.load()
    if len(params) != 4 or len(strides) != 4:
        raise RuntimeError('pyprob_hip::dist_draw: 4 parameters and 4 strides')
    n = _f32(out, 'out').numel()
    _same_device(out, rows, *params)
    d = L.pp_dist()
    _dist_fill(d, kind, params, strides, 0, n, 'dist_draw')
    rp, m = _rows_arg(rows, n, 'dist_draw')
    with torch.cuda.device(out.device):
        rc = lib.pp_dist_draw(C.byref(d), rp, int(m), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), int(stream_id) & 0xFFFFFFFF,
                              out.data_ptr(), _stream(out))
    L.check(rc, 'pp_dist_draw')


def _mix_fill(kinds, params, strides, probs, n, what):
    """pp_mixture from the K components' kinds, 4 K parameters / strides and the weights (K: one shared row, n K: one per particle)."""
    K = len(kinds)
    if not 1 <= K <= L.PP_MIX_MAX_COMPONENTS or len(params) != 4 * K or len(strides) != 4 * K:
        raise RuntimeError('pyprob_hip::%s: 1..%d components, 4 parameters and strides per component' % (what, L.PP_MIX_MAX_COMPONENTS))
    if _f32(probs, 'probs').numel() not in (K, n * K):
        raise RuntimeError('pyprob_hip::%s: probs must have K = %d or n K = %d elements' % (what, K, n * K))
    mx = L.pp_mixture()
    mx.count = K
    mx.probs_stride = 0 if probs.numel() == K else K      # (n = 1: either reading is the same row)
    mx.probs = probs.data_ptr()
    for k in range(K):
        if int(kinds[k]) in (2, 5):
            raise RuntimeError('pyprob_hip::%s: component %d: Factor and Categorical are not mixture components' % (what, k))
        for q in range(4):
            if params[4 * k + q] is not None and int(strides[4 * k + q]) not in (0, 1):
                raise RuntimeError('pyprob_hip::%s: component %d: a parameter stride is 0 or 1' % (what, k))
        _dist_fill(mx.comp[k], int(kinds[k]), params, strides, k, n, what)
    return mx


def _mix_logweight_hip(lw, kinds, params, strides, probs, x, scale, rows, lp_out, n):
    lib = L.load()
    ref = lw if lw is not None else lp_out
    if ref is None:
        raise RuntimeError('pyprob_hip::mix_logweight: lw or lp_out is needed')
    for t, name in ((lw, 'lw'), (lp_out, 'lp_out')):
        if t is not None and (_f32(t, name).numel() != n):
            raise RuntimeError('pyprob_hip::mix_logweight: %s must have n = %d elements' % (name, n))
    _same_device(ref, lw, lp_out, rows, probs, x, *params)
    mx = _mix_fill(kinds, params, strides, probs, n, 'mix_logweight')
    if _f32(x, 'x').numel() not in (1, n):
        raise RuntimeError('pyprob_hip::mix_logweight: x must have 1 or n elements')
    rp, m = _rows_arg(rows, n, 'mix_logweight')
    with torch.cuda.device(ref.device):
        rc = lib.pp_mix_logweight(C.byref(mx), x.data_ptr(), 0 if x.numel() == 1 else 1, float(scale), L.ptr(lw), L.ptr(lp_out), rp,
                                  int(m), int(n), _stream(ref))
    L.check(rc, 'pp_mix_logweight')


def _mix_draw_hip(kinds, params, strides, probs, rows, out, seed, offset, stream_id):
    lib = L.load()
    n = _f32(out, 'out').numel()
    _same_device(out, rows, probs, *params)
    mx = _mix_fill(kinds, params, strides, probs, n, 'mix_draw')
    if int(stream_id) & ~0x7FFFFFFF:
        raise RuntimeError('pyprob_hip::mix_draw: stream_id must leave the top bit clear (it marks the selection stream)')
    rp, m = _rows_arg(rows, n, 'mix_draw')
    with torch.cuda.device(out.device):
        rc = lib.pp_mix_draw(C.byref(mx), rp, int(m), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), int(stream_id),
                             out.data_ptr(), _stream(out))
    L.check(rc, 'pp_mix_draw')


def _is_stats_hip(lw, x, scratch):
    lib = L.load()
    _same_device(lw, x, scratch)
    if scratch.dtype != torch.float64 or scratch.numel() < L.PP_IS_STATS_SCRATCH:
        raise RuntimeError('pyprob_hip::is_stats: scratch must hold PP_IS_STATS_SCRATCH doubles')
    out = torch.zeros(8, dtype=torch.float64, device=lw.device)
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_stats(_f32(lw, 'lw').data_ptr(), L.ptr(x), lw.numel(), out.data_ptr(), scratch.data_ptr(), _stream(lw))
    L.check(rc, 'pp_is_stats')
    return out


def _groups_of(t, n_per, what):
    n_per = int(n_per)
    if t.dim() != 1 or not t.is_contiguous() or n_per < 1 or t.numel() % n_per:
        raise RuntimeError('pyprob_hip::%s: a contiguous 1-D tensor of M * n_per elements (n_per >= 1)' % what)
    return t.numel() // n_per


def _particles_like(t, lw, name, what, of="the log-weights'"):
    if _f32(t, name).dim() != 1 or t.numel() != lw.numel():
        raise RuntimeError('pyprob_hip::%s: %s must be a contiguous 1-D tensor of %s M * n_per elements' % (what, name, of))


def _group_stats_ok(stats, M, what):
    if stats is not None and (stats.dtype != torch.float64 or not stats.is_contiguous() or stats.numel() < 6 * M):
        raise RuntimeError('pyprob_hip::%s: stats must be a contiguous float64 tensor of [M, 6]' % what)


def _workspace(sizer, device, *shape):
    """(uint8 tensor, its size): the workspace a pp_*_workspace_bytes function asks for at this shape."""
    need = sizer(*shape)
    return torch.empty(need, dtype=torch.uint8, device=device), need


def _is_cdf_groups_hip(lw, n_per, stats):
    """cdf [M n_per] (float64) of the M groups of n_per log-weights; stats: the [M, 6] (or, M = 1, the 6+) doubles pp_is_stats /
    pp_is_fused_groups reduced over the same log-weights - their maxima are taken instead of being searched."""
    lib = L.load()
    _same_device(lw, stats)
    M = _groups_of(_f32(lw, 'lw'), n_per, 'is_cdf_groups')
    _group_stats_ok(stats, M, 'is_cdf_groups')
    out = torch.empty(M * int(n_per), dtype=torch.float64, device=lw.device)
    ws, need = _workspace(lib.pp_is_cdf_workspace_bytes, lw.device, M, int(n_per))
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_cdf_groups(lw.data_ptr(), M, int(n_per), L.ptr(stats), out.data_ptr(), ws.data_ptr(), need, _stream(lw))
    L.check(rc, 'pp_is_cdf_groups')
    return out


def _is_resample_groups_hip(cdf, values, n_per, lo, hi, n_out, seed, offset, want_index):
    """(index int64 [M n_out] or empty, value float32 [M n_out] or empty): n_out draws from every group's cdf in [lo, hi)."""
    lib = L.load()
    _same_device(cdf, values)
    if cdf.dtype != torch.float64:
        raise RuntimeError('pyprob_hip::is_resample_groups: cdf must be float64 (is_cdf_groups)')
    M = _groups_of(cdf, n_per, 'is_resample_groups')
    if values is not None and _f32(values, 'values').numel() != cdf.numel():
        raise RuntimeError('pyprob_hip::is_resample_groups: values must have the cdf\'s M * n_per elements')
    n_out = int(n_out)
    index = torch.empty(M * max(n_out, 0) if want_index else 0, dtype=torch.int64, device=cdf.device)
    value = torch.empty(M * max(n_out, 0) if values is not None else 0, dtype=torch.float32, device=cdf.device)
    with torch.cuda.device(cdf.device):
        rc = lib.pp_is_resample_groups(cdf.data_ptr(), L.ptr(values), M, int(n_per), int(lo), int(hi), n_out,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                       index.data_ptr() if want_index else None, value.data_ptr() if values is not None else None,
                                       _stream(cdf))
    L.check(rc, 'pp_is_resample_groups')
    return index, value


def _is_resample_scheme_groups_hip(cdf, values, n_per, lo, hi, n_out, scheme, seed, offset, want_index):
    """is_resample_groups with a scheme (lib.PP_RESAMPLE_MULTINOMIAL / _STRATIFIED / _SYSTEMATIC): pp_is_resample_scheme_groups."""
    lib = L.load()
    _same_device(cdf, values)
    if cdf.dtype != torch.float64:
        raise RuntimeError('pyprob_hip::is_resample_scheme_groups: cdf must be float64 (is_cdf_groups)')
    M = _groups_of(cdf, n_per, 'is_resample_scheme_groups')
    if values is not None and _f32(values, 'values').numel() != cdf.numel():
        raise RuntimeError('pyprob_hip::is_resample_scheme_groups: values must have the cdf\'s M * n_per elements')
    n_out = int(n_out)
    index = torch.empty(M * max(n_out, 0) if want_index else 0, dtype=torch.int64, device=cdf.device)
    value = torch.empty(M * max(n_out, 0) if values is not None else 0, dtype=torch.float32, device=cdf.device)
    with torch.cuda.device(cdf.device):
        rc = lib.pp_is_resample_scheme_groups(cdf.data_ptr(), L.ptr(values), M, int(n_per), int(lo), int(hi), n_out, int(scheme),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                              index.data_ptr() if want_index else None,
                                              value.data_ptr() if values is not None else None, _stream(cdf))
    L.check(rc, 'pp_is_resample_scheme_groups')
    return index, value


def _is_moments_groups_hip(lw, cols, n_per, stats):
    """[M, PP_IS_MOMENTS_WIDTH(J)] (float64): the weight sums, pivots, first and second moments about the pivots of the J columns
    over each of the M groups of n_per particles (pp_is_moments_groups). stats: as for is_cdf_groups."""
    lib = L.load()
    cols = list(cols)
    _same_device(lw, stats, *cols)
    M = _groups_of(_f32(lw, 'lw'), n_per, 'is_moments_groups')
    J = len(cols)
    if not 1 <= J <= L.PP_IS_MOMENTS_MAX_COLS:
        raise RuntimeError('pyprob_hip::is_moments_groups: 1 .. %d columns per call' % L.PP_IS_MOMENTS_MAX_COLS)
    for c in cols:
        _particles_like(c, lw, 'every column', 'is_moments_groups')
    _group_stats_ok(stats, M, 'is_moments_groups')
    out = torch.empty((M, L.PP_IS_MOMENTS_WIDTH(J)), dtype=torch.float64, device=lw.device)
    ws, need = _workspace(lib.pp_is_moments_workspace_bytes, lw.device, M, int(n_per), J)
    ptrs = (C.c_void_p * J)(*[c.data_ptr() for c in cols])
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_moments_groups(lw.data_ptr(), C.cast(ptrs, C.c_void_p), J, M, int(n_per), L.ptr(stats), out.data_ptr(),
                                      ws.data_ptr(), need, _stream(lw))
    L.check(rc, 'pp_is_moments_groups')
    return out


def _hist_edges(e, M, what):
    """(bins, stride) of an edge tensor: [bins + 1] shared by the groups (stride 0) or [M, bins + 1], one row per group."""
    if e.dtype != torch.float64 or not e.is_contiguous() or e.dim() not in (1, 2) or e.shape[-1] < 2 or (e.dim() == 2 and e.shape[0] != M):
        raise RuntimeError('pyprob_hip::is_hist_groups: %s must be a contiguous float64 tensor of [bins + 1] or [M, bins + 1]' % what)
    return int(e.shape[-1]) - 1, (0 if e.dim() == 1 else int(e.shape[-1]))


def _is_hist_groups_hip(lw, x, y, n_per, edges_x, edges_y, stats):
    """[M, 2, slots] (int64): the fixed-point masses and the particle counts of the slots of each of the M groups of n_per particles
    (pp_is_hist_groups); slots = bins + 3 (1-D) or bins_x bins_y + 2 (2-D: y and edges_y given). Edges of dim 1 are shared by the
    groups, [M, bins + 1] is one row per group. stats: as for is_cdf_groups."""
    lib = L.load()
    _same_device(lw, x, y, edges_x, edges_y, stats)
    M = _groups_of(_f32(lw, 'lw'), n_per, 'is_hist_groups')
    _particles_like(x, lw, 'x', 'is_hist_groups')
    if (y is None) != (edges_y is None):
        raise RuntimeError('pyprob_hip::is_hist_groups: y and edges_y are given together (2-D) or not at all (1-D)')
    if y is not None:
        _particles_like(y, lw, 'y', 'is_hist_groups')
    bx, sx = _hist_edges(edges_x, M, 'edges_x')
    by, sy = _hist_edges(edges_y, M, 'edges_y') if edges_y is not None else (1, 0)
    if bx * by > L.PP_IS_HIST_MAX_BINS:
        raise RuntimeError('pyprob_hip::is_hist_groups: at most %d bins per call' % L.PP_IS_HIST_MAX_BINS)
    _group_stats_ok(stats, M, 'is_hist_groups')
    slots = bx + 3 if y is None else bx * by + 2
    out = torch.empty((M, 2, slots), dtype=torch.int64, device=lw.device)
    ws, need = _workspace(lib.pp_is_hist_workspace_bytes, lw.device, M, int(n_per), bx, by)
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_hist_groups(lw.data_ptr(), x.data_ptr(), L.ptr(y), M, int(n_per), edges_x.data_ptr(), bx, sx, L.ptr(edges_y),
                                   by, sy, L.ptr(stats), out.data_ptr(), ws.data_ptr(), need, _stream(lw))
    L.check(rc, 'pp_is_hist_groups')
    return out


def _is_extent_groups_hip(lw, x, n_per):
    """[M, 4] (float64): min x, max x, particles counted, particles whose x is NaN, per group of n_per particles
    (pp_is_extent_groups)."""
    lib = L.load()
    _same_device(lw, x)
    M = _groups_of(_f32(lw, 'lw'), n_per, 'is_extent_groups')
    _particles_like(x, lw, 'x', 'is_extent_groups')
    out = torch.empty((M, 4), dtype=torch.float64, device=lw.device)
    ws, need = _workspace(lib.pp_is_extent_workspace_bytes, lw.device, M, int(n_per))
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_extent_groups(lw.data_ptr(), x.data_ptr(), M, int(n_per), out.data_ptr(), ws.data_ptr(), need, _stream(lw))
    L.check(rc, 'pp_is_extent_groups')
    return out


def _counted_ok(counted, M, what):
    if counted.dtype != torch.int32 or not counted.is_contiguous() or counted.numel() != 2 * M:
        raise RuntimeError('pyprob_hip::%s: counted must be the contiguous int32 [M, 2] tensor of is_sort_groups' % what)


def _is_sort_groups_hip(lw, x, n_per, stats):
    """(value float32 [M n_per], lw float32 [M n_per], index int32 [M n_per], counted int32 [M, 2]): the particles of each of the M
    groups in stable ascending order of the key of x (pp_is_sort_groups); counted[g] = {particles with a real key, particles with a
    finite log-weight whose x is NaN}. stats: as for is_cdf_groups (the outputs do not depend on it)."""
    lib = L.load()
    _same_device(lw, x, stats)
    M = _groups_of(_f32(lw, 'lw'), n_per, 'is_sort_groups')
    _particles_like(x, lw, 'x', 'is_sort_groups')
    _group_stats_ok(stats, M, 'is_sort_groups')
    value, lw_out = torch.empty_like(x), torch.empty_like(lw)
    index = torch.empty(lw.numel(), dtype=torch.int32, device=lw.device)
    counted = torch.empty((M, 2), dtype=torch.int32, device=lw.device)
    ws, need = _workspace(lib.pp_is_sort_workspace_bytes, lw.device, M, int(n_per))
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_sort_groups(lw.data_ptr(), x.data_ptr(), M, int(n_per), L.ptr(stats), value.data_ptr(), lw_out.data_ptr(),
                                   index.data_ptr(), counted.data_ptr(), ws.data_ptr(), need, _stream(lw))
    L.check(rc, 'pp_is_sort_groups')
    return value, lw_out, index, counted


def _is_quantile_groups_hip(value_sorted, cdf_sorted, counted, n_per, q):
    """[M, Q] (float64): the inverted-cdf quantiles q (float64 [Q] in [0, 1], shared by the groups) of each of the M groups of n_per
    sorted particles (pp_is_quantile_groups); cdf_sorted = is_cdf_groups over the sorted log-weights."""
    lib = L.load()
    _same_device(value_sorted, cdf_sorted, counted, q)
    M = _groups_of(_f32(value_sorted, 'value_sorted'), n_per, 'is_quantile_groups')
    if cdf_sorted.dtype != torch.float64 or cdf_sorted.dim() != 1 or cdf_sorted.numel() != value_sorted.numel() or \
            not cdf_sorted.is_contiguous():
        raise RuntimeError('pyprob_hip::is_quantile_groups: cdf_sorted must be a contiguous float64 tensor of the values\' '
                           'M * n_per elements (is_cdf_groups)')
    _counted_ok(counted, M, 'is_quantile_groups')
    if q.dtype != torch.float64 or q.dim() != 1 or not q.is_contiguous():
        raise RuntimeError('pyprob_hip::is_quantile_groups: q must be a contiguous 1-D float64 tensor')
    Q = int(q.numel())
    out = torch.empty((M, Q), dtype=torch.float64, device=value_sorted.device)
    with torch.cuda.device(value_sorted.device):
        rc = lib.pp_is_quantile_groups(value_sorted.data_ptr(), cdf_sorted.data_ptr(), counted.data_ptr(), M, int(n_per),
                                       q.data_ptr(), Q, out.data_ptr(), _stream(value_sorted))
    L.check(rc, 'pp_is_quantile_groups')
    return out


def _sorted_ok(value_sorted, cdf_sorted, counted, n_per, what):
    M = _groups_of(_f32(value_sorted, 'value_sorted'), n_per, what)
    if cdf_sorted.dtype != torch.float64 or cdf_sorted.dim() != 1 or cdf_sorted.numel() != value_sorted.numel() or \
            not cdf_sorted.is_contiguous():
        raise RuntimeError('pyprob_hip::%s: cdf_sorted must be a contiguous float64 tensor of the values\' M * n_per elements '
                           '(is_cdf_groups)' % what)
    _counted_ok(counted, M, what)
    return M


def _is_hpd_groups_hip(value_sorted, cdf_sorted, counted, n_per, level):
    """(interval float64 [M, L, 2], index int32 [M, L, 2]): the highest-posterior-density interval of every level (float64 [L],
    shared by the groups) of each of the M groups of n_per sorted particles and its two positions in sorted order
    (pp_is_hpd_groups); cdf_sorted = is_cdf_groups over the sorted log-weights."""
    lib = L.load()
    _same_device(value_sorted, cdf_sorted, counted, level)
    M = _sorted_ok(value_sorted, cdf_sorted, counted, n_per, 'is_hpd_groups')
    if level.dtype != torch.float64 or level.dim() != 1 or not level.is_contiguous():
        raise RuntimeError('pyprob_hip::is_hpd_groups: level must be a contiguous 1-D float64 tensor')
    nl = int(level.numel())
    dev = value_sorted.device
    out = torch.empty((M, nl, 2), dtype=torch.float64, device=dev)
    index = torch.empty((M, nl, 2), dtype=torch.int32, device=dev)
    ws, need = _workspace(lib.pp_is_hpd_workspace_bytes, dev, M, int(n_per), nl)
    with torch.cuda.device(dev):
        rc = lib.pp_is_hpd_groups(value_sorted.data_ptr(), cdf_sorted.data_ptr(), counted.data_ptr(), M, int(n_per), level.data_ptr(),
                                  nl, out.data_ptr(), index.data_ptr(), ws.data_ptr(), need, _stream(value_sorted))
    L.check(rc, 'pp_is_hpd_groups')
    return out, index


def _is_ecdf_groups_hip(value_sorted, cdf_sorted, counted, n_per, x, strict):
    """(cdf float64 [M, Q], rank int32 [M, Q]): P(X <= x) (strict: <) at the Q points x[g] (float64 [M, Q]: per group) of each of
    the M groups of n_per sorted particles, and the number of counted particles at or below (below) the point
    (pp_is_ecdf_groups)."""
    lib = L.load()
    _same_device(value_sorted, cdf_sorted, counted, x)
    M = _sorted_ok(value_sorted, cdf_sorted, counted, n_per, 'is_ecdf_groups')
    if x.dtype != torch.float64 or x.dim() != 2 or x.shape[0] != M or not x.is_contiguous():
        raise RuntimeError('pyprob_hip::is_ecdf_groups: x must be a contiguous float64 tensor of [M, Q]')
    Q = int(x.shape[1])
    dev = value_sorted.device
    out = torch.empty((M, Q), dtype=torch.float64, device=dev)
    rank = torch.empty((M, Q), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pp_is_ecdf_groups(value_sorted.data_ptr(), cdf_sorted.data_ptr(), counted.data_ptr(), M, int(n_per), x.data_ptr(), Q,
                                   1 if strict else 0, out.data_ptr(), rank.data_ptr(), _stream(value_sorted))
    L.check(rc, 'pp_is_ecdf_groups')
    return out, rank


def _is_psis_groups_hip(lw_sorted, index_sorted, counted, n_per, stats, tail, want_weights):
    """(lw_out float32 [M n_per] in particle order or None, out float64 [M, PP_IS_PSIS_WIDTH]): the Pareto-smoothed log-weights and
    the fit (k-hat, sigma, n, m, f, cutoff log-weight, c, maximum) of each of the M groups of n_per particles sorted by their
    log-weight - is_sort_groups(lw, lw, ...) - (pp_is_psis_groups); tail: the tail length, 0 = min(c / 5, 3 sqrt(c)).
    want_weights=False: the diagnostic alone, without the smoothing launch."""
    lib = L.load()
    _same_device(lw_sorted, index_sorted, counted, stats)
    M = _groups_of(_f32(lw_sorted, 'lw_sorted'), n_per, 'is_psis_groups')
    if index_sorted.dtype != torch.int32 or index_sorted.dim() != 1 or index_sorted.numel() != lw_sorted.numel() or \
            not index_sorted.is_contiguous():
        raise RuntimeError('pyprob_hip::is_psis_groups: index_sorted must be the contiguous int32 tensor of is_sort_groups '
                           "(the log-weights' M * n_per elements)")
    _counted_ok(counted, M, 'is_psis_groups')
    _group_stats_ok(stats, M, 'is_psis_groups')
    if int(tail) < 0:
        raise RuntimeError('pyprob_hip::is_psis_groups: tail >= 0 (0: the rule)')
    dev = lw_sorted.device
    lw_out = torch.empty_like(lw_sorted) if want_weights else None
    out = torch.empty((M, L.PP_IS_PSIS_WIDTH), dtype=torch.float64, device=dev)
    ws, need = _workspace(lib.pp_is_psis_workspace_bytes, dev, M, int(n_per), int(tail))
    with torch.cuda.device(dev):
        rc = lib.pp_is_psis_groups(lw_sorted.data_ptr(), index_sorted.data_ptr(), counted.data_ptr(), M, int(n_per), L.ptr(stats),
                                   int(tail), L.ptr(lw_out), out.data_ptr(), ws.data_ptr(), need, _stream(lw_sorted))
    L.check(rc, 'pp_is_psis_groups')
    return lw_out, out


def _is_unique_groups_hip(value_sorted, lw_sorted, counted, n_per, stats):
    """(value float32 [M, n_per], mass int64 [M, n_per], count int32 [M, n_per], runs int32 [M]): the runs of equal keys among the
    counted sorted particles of each group (pp_is_unique_groups); entries at or beyond runs[g] are not written."""
    lib = L.load()
    _same_device(value_sorted, lw_sorted, counted, stats)
    M = _groups_of(_f32(value_sorted, 'value_sorted'), n_per, 'is_unique_groups')
    _particles_like(lw_sorted, value_sorted, 'lw_sorted', 'is_unique_groups', of="the values'")
    _counted_ok(counted, M, 'is_unique_groups')
    _group_stats_ok(stats, M, 'is_unique_groups')
    dev = value_sorted.device
    value = torch.empty((M, int(n_per)), dtype=torch.float32, device=dev)
    mass = torch.empty((M, int(n_per)), dtype=torch.int64, device=dev)
    count = torch.empty((M, int(n_per)), dtype=torch.int32, device=dev)
    runs = torch.empty(M, dtype=torch.int32, device=dev)
    ws, need = _workspace(lib.pp_is_unique_workspace_bytes, dev, M, int(n_per))
    with torch.cuda.device(dev):
        rc = lib.pp_is_unique_groups(value_sorted.data_ptr(), lw_sorted.data_ptr(), counted.data_ptr(), M, int(n_per), L.ptr(stats),
                                     value.data_ptr(), mass.data_ptr(), count.data_ptr(), runs.data_ptr(), ws.data_ptr(), need,
                                     _stream(value_sorted))
    L.check(rc, 'pp_is_unique_groups')
    return value, mass, count, runs


def gmm_check_every():
    """After how many EM iterations pp_is_gmm_groups asks whether every group converged: PP_GMM_CHECK, default 8. The result of
    a fit does not depend on it (a converged group is frozen on the device either way); it trades launches of frozen groups
    against host synchronisations."""
    import os
    try:
        n = int(os.environ.get('PP_GMM_CHECK', '8'))
    except ValueError:
        n = 8
    return n if n >= 1 else 8


def _is_gmm_groups_hip(lw, x, n_components, n_per, stats, params_init, max_iter, tol, reg_covar):
    """[M, PP_IS_GMM_WIDTH(K)] (float64): weights, means, variances | last lower bound, n_iter, converged, W, count, max lw of the
    weighted K-component Gaussian-mixture EM over x in each of the M groups of n_per particles (pp_is_gmm_groups), started from
    params_init (float64 [M, 3 K]: weights | means | variances). stats: as for is_cdf_groups."""
    lib = L.load()
    _same_device(lw, x, stats, params_init)
    M = _groups_of(_f32(lw, 'lw'), n_per, 'is_gmm_groups')
    _particles_like(x, lw, 'x', 'is_gmm_groups')
    K = int(n_components)
    if not 1 <= K <= L.PP_IS_GMM_MAX_K:
        raise RuntimeError('pyprob_hip::is_gmm_groups: 1 .. %d mixture components' % L.PP_IS_GMM_MAX_K)
    _group_stats_ok(stats, M, 'is_gmm_groups')
    if params_init.dtype != torch.float64 or not params_init.is_contiguous() or params_init.numel() != M * 3 * K:
        raise RuntimeError('pyprob_hip::is_gmm_groups: params_init must be a contiguous float64 tensor of [M, 3 K]')
    out = torch.empty((M, L.PP_IS_GMM_WIDTH(K)), dtype=torch.float64, device=lw.device)
    ws, need = _workspace(lib.pp_is_gmm_workspace_bytes, lw.device, M, int(n_per), K)
    with torch.cuda.device(lw.device):
        rc = lib.pp_is_gmm_groups(lw.data_ptr(), x.data_ptr(), K, M, int(n_per), L.ptr(stats), params_init.data_ptr(), int(max_iter),
                                  float(tol), float(reg_covar), gmm_check_every(), out.data_ptr(), ws.data_ptr(), need, _stream(lw))
    L.check(rc, 'pp_is_gmm_groups')
    return out


_lib.impl('ic_loss', _ic_loss_hip, 'CUDA')
_lib.impl('adam_step', _adam_step_hip, 'CUDA')
_lib.impl('sgd_step', _sgd_step_hip, 'CUDA')
_lib.impl('larc_scale', _larc_scale_hip, 'CUDA')
_lib.impl('is_init', _is_init_hip, 'CUDA')
_lib.impl('is_step', _is_step_hip, 'CUDA')
_lib.impl('is_step_rows', _is_step_rows_hip, 'CUDA')
_lib.impl('is_statement_rows', _is_statement_rows_hip, 'CUDA')
_lib.impl('is_step_net', _is_step_net_hip, 'CUDA')
_lib.impl('is_fused', _is_fused_hip, 'CUDA')
_lib.impl('prior_draw', _prior_draw_hip, 'CUDA')
_lib.impl('obs_draw', _obs_draw_hip, 'CUDA')
_lib.impl('obs_logweight', _obs_logweight_hip, 'CUDA')
_lib.impl('obs_logweight_groups', _obs_logweight_groups_hip, 'CUDA')
_lib.impl('reobserve_groups', _reobserve_groups_hip, 'CUDA')
_lib.impl('log_prob', _log_prob_hip, 'CUDA')
_lib.impl('logweight_terms', _logweight_terms_hip, 'CUDA')
_lib.impl('is_stats', _is_stats_hip, 'CUDA')
_lib.impl('is_cdf_groups', _is_cdf_groups_hip, 'CUDA')
_lib.impl('is_resample_groups', _is_resample_groups_hip, 'CUDA')
_lib.impl('is_resample_scheme_groups', _is_resample_scheme_groups_hip, 'CUDA')
_lib.impl('is_moments_groups', _is_moments_groups_hip, 'CUDA')
_lib.impl('is_hist_groups', _is_hist_groups_hip, 'CUDA')
_lib.impl('is_extent_groups', _is_extent_groups_hip, 'CUDA')
_lib.impl('is_sort_groups', _is_sort_groups_hip, 'CUDA')
_lib.impl('is_quantile_groups', _is_quantile_groups_hip, 'CUDA')
_lib.impl('is_unique_groups', _is_unique_groups_hip, 'CUDA')
_lib.impl('is_hpd_groups', _is_hpd_groups_hip, 'CUDA')
_lib.impl('is_ecdf_groups', _is_ecdf_groups_hip, 'CUDA')
_lib.impl('is_psis_groups', _is_psis_groups_hip, 'CUDA')
_lib.impl('is_gmm_groups', _is_gmm_groups_hip, 'CUDA')
_lib.impl('dist_logweight', _dist_logweight_hip, 'CUDA')
_lib.impl('dist_draw', _dist_draw_hip, 'CUDA')
_lib.impl('mix_logweight', _mix_logweight_hip, 'CUDA')
_lib.impl('mix_draw', _mix_draw_hip, 'CUDA')

ops = getattr(torch.ops, NAMESPACE)
