// The likelihood of a VECTOR-valued observe of a lock-step importance-sampling run (state.observe pyprob/state.py:118-155 with
// trace.py:123-125, which sums an observed variable's log_prob over its elements): one row of k values per particle - an image,
// a k-vector - scored in one launch. pp_dist_logweight (dist_kernels.hip) is the scalar form; this kernel is its k-wide form
// and for k = 1 gives the same bits. The per-element formula is dist_math.hpp's scalar_log_prob_at, nothing else.
// pp_obs_logweight_groups is the same kernel for the M n_per rows of a batched posterior call (is_batch.hip), where an operand may
// hold one row per GROUP (the observed image of each group): a template flag that resolves row pointers, one copy of everything else.
#include "common.hpp"
#include "dist_math.hpp"
#include "obs_row.hpp"

#include <math.h>

#include <algorithm>

namespace pp {

// GROUPS: m = n_groups * n_per rows without a row list, row j of group j / n_per (a workgroup, and for k <= 128 a wave, may
// straddle groups: the lanes of a row are still the G lanes they are in the plain kernel).
template <int KIND, bool GROUPS>
__global__ __launch_bounds__(256) void obs_logweight_kernel(ObsArgs A, int fast, int k, int G, float scale, float* __restrict__ lw,
                                                            float* __restrict__ lp_out, const int64_t* __restrict__ rows,
                                                            int64_t m, int n_per) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & (G - 1);          // the lane holds slots 4l .. 4l + 3
    const int rpw = 64 / G;                // rows per wave
    const int ng = (int)(((int64_t)k + 3) >> 2), nfull = k >> 2;
    const int64_t step = (int64_t)gridDim.x * 4 * rpw;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * rpw; base < m; base += step) {      // (wave-uniform)
        const int64_t j = base + lane / G;
        const bool live = j < m;
        const int64_t r = live ? (!GROUPS && rows ? rows[j] : j) : 0;
        const int64_t gr = GROUPS ? r / n_per : 0;
        float s0 = -0.0f, s1 = -0.0f, s2 = -0.0f, s3 = -0.0f;      // the lane's four slots
        if (live) {
            if (ng > G)      // (a function of k alone, like G)
                obs_row<KIND, 4, GROUPS>(A, fast != 0, r, gr, l, G, nfull, ng, k, s0, s1, s2, s3);
            else
                obs_row<KIND, 1, GROUPS>(A, fast != 0, r, gr, l, G, nfull, ng, k, s0, s1, s2, s3);
        }
        float acc = (s0 + s1) + (s2 + s3);
        for (int d = 1; d < G; d <<= 1) acc += __shfl_xor(acc, d);      // (G is wave-uniform: every lane takes every stage)
        if (live && l == 0) {
            if (lp_out) lp_out[r] = acc;
            if (lw) lw[r] = scaled_add(lw[r], scale, acc);
        }
    }
}

// The checks and the launch behind both entry points. groups: m = n_groups * n_per rows, no row list, per_group marks.
static int obs_logweight_launch(const char* who, int32_t kind, const pp_obs_operand params[4], pp_obs_operand x, int32_t k,
                                float scale, float* lw, float* lp_out, const int64_t* rows, int64_t m, bool groups, int n_per,
                                int per_group, void* stream) {
    if (kind < 0 || kind > PP_DIST_MAX_KIND || kind == 2 || kind == 5) {
        set_error("%s: kind %d is not a scalar family (0, 1, 3, 4, 6-13)", who, (int)kind);
        return PP_EINVAL;
    }
    if (!lw && !lp_out) {
        set_error("%s: lw or lp_out is needed", who);
        return PP_EINVAL;
    }
    const int np = obs_kind_params(kind);
    ObsArgs A{};
    for (int q = 0; q < np; ++q) {
        if (!params || !params[q].p || params[q].row_stride < 0 || params[q].elem_stride < 0) {
            set_error("%s: kind %d needs parameter %d (a pointer and strides >= 0)", who, (int)kind, q);
            return PP_EINVAL;
        }
        A.q[q] = ObsOperand{params[q].p, params[q].row_stride, params[q].elem_stride};
    }
    if (!x.p || x.row_stride < 0 || x.elem_stride < 0) {
        set_error("%s: no value block (a pointer and strides >= 0)", who);
        return PP_EINVAL;
    }
    A.x = ObsOperand{x.p, x.row_stride, x.elem_stride};
    A.per_group = groups ? per_group : 0;
    if (m == 0) return 0;
    const bool fast = obs_fast_path(A, np, k);
    const int G = obs_group(k);
    const int64_t rpb = 4 * (64 / G);      // rows per workgroup
    const dim3 grid((unsigned)std::min<int64_t>(65536, (m + rpb - 1) / rpb)), block(256);
    hipStream_t st = as_stream(stream);
#define PP_OBS_LW(K)                                                                                                                  \
    case K:                                                                                                                           \
        if (groups)                                                                                                                   \
            hipLaunchKernelGGL((obs_logweight_kernel<K, true>), grid, block, 0, st, A, fast ? 1 : 0, k, G, scale, lw, lp_out, rows, m, \
                               n_per);                                                                                                \
        else                                                                                                                          \
            hipLaunchKernelGGL((obs_logweight_kernel<K, false>), grid, block, 0, st, A, fast ? 1 : 0, k, G, scale, lw, lp_out, rows, m, \
                               n_per);                                                                                                \
        break
    switch (kind) {
        PP_OBS_LW(0); PP_OBS_LW(1); PP_OBS_LW(3); PP_OBS_LW(4); PP_OBS_LW(6); PP_OBS_LW(7); PP_OBS_LW(8); PP_OBS_LW(9);
        PP_OBS_LW(10); PP_OBS_LW(11); PP_OBS_LW(12); PP_OBS_LW(13);
        default: break;
    }
#undef PP_OBS_LW
    PP_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace pp

extern "C" {

int pp_obs_logweight(int32_t kind, const pp_obs_operand params[4], pp_obs_operand x, int32_t k, float scale, float* lw,
                     float* lp_out, const int64_t* rows, int32_t m, int32_t n, void* stream) {
    if (k < 1 || n < 0 || m < 0 || (!rows && m != n) || m > n) {
        pp::set_error("pp_obs_logweight: k >= 1 values per row, 0 <= m <= n rows, m = n without a row list (k %d, m %d, n %d)", (int)k,
                      (int)m, (int)n);
        return PP_EINVAL;
    }
    return pp::obs_logweight_launch("pp_obs_logweight", kind, params, x, k, scale, lw, lp_out, rows, m, false, 1, 0, stream);
}

int pp_obs_logweight_groups(int32_t kind, const pp_obs_operand params[4], pp_obs_operand x, int32_t per_group, int32_t k, float scale,
                            float* lw, float* lp_out, int32_t n_groups, int32_t n_per, void* stream) {
    if (k < 1 || n_groups < 0 || n_per < 1 || per_group < 0 || per_group > 31) {
        pp::set_error("pp_obs_logweight_groups: k >= 1 values per row, n_groups >= 0 groups of n_per >= 1 rows, per_group a mask of "
                      "bits 0-4 (k %d, n_groups %d, n_per %d, per_group %d)", (int)k, (int)n_groups, (int)n_per, (int)per_group);
        return PP_EINVAL;
    }
    return pp::obs_logweight_launch("pp_obs_logweight_groups", kind, params, x, k, scale, lw, lp_out, nullptr,
                                    (int64_t)n_groups * n_per, true, n_per, per_group, stream);
}

}  // extern "C"
