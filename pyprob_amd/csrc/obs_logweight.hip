// The likelihood of a VECTOR-valued observe of a lock-step importance-sampling run (state.observe pyprob/state.py:118-155 with
// trace.py:123-125, which sums an observed variable's log_prob over its elements): one row of k values per particle - an image,
// a k-vector - scored in one launch. pp_dist_logweight (dist_kernels.hip) is the scalar form; this kernel is its k-wide form
// and for k = 1 gives the same bits. The per-element formula is dist_math.hpp's scalar_log_prob_at, nothing else.
// pp_obs_logweight_groups is the same kernel for the M n_per rows of a batched posterior call (is_batch.hip), where an operand may
// hold one row per GROUP (the observed image of each group): a template flag that resolves row pointers, one copy of everything else.
#include "common.hpp"
#include "dist_math.hpp"

#include <math.h>

#include <algorithm>

namespace pp {

struct ObsOperand {
    const float* p;
    int64_t rs;      // row stride (elements)
    int es;          // element stride
};
struct ObsArgs {
    ObsOperand q[4];
    ObsOperand x;
    int per_group;      // pp_obs_logweight_groups: bit q < 4 - q[q], bit 4 - x is addressed with the row's GROUP index
};

// SUMMATION ORDER (include/pyprob_amd.h states it as part of the ABI). A row has 256 slots; element e belongs to slot e & 255.
// A slot starts at -0 (the additive identity: -0 + v == v for every v, so an empty slot changes no bit) and adds its elements'
// log-densities in ascending e. Then the four slots 4l .. 4l + 3 of lane l become t[l] = (s[4l] + s[4l+1]) + (s[4l+2] + s[4l+3]),
// and the 64 values t are combined by a butterfly: in stage d = 1, 2, 4, 8, 16, 32 every t[l] becomes t[l] + t[l ^ d] (fp32
// addition commutes, so both partners hold the same bits afterwards).
// G = the lanes that work on one row = the smallest power of two >= ceil(k / 4), at most 64 - a function of k alone. Lane l of
// the row's group holds the slots 4l .. 4l + 3 (one 16-byte load); for G < 64 the slots from 4G on are empty and the stages
// d >= G would add -0: they are skipped. 64 / G rows share a wave.
static inline int obs_group(int k) {
    const int64_t ng = ((int64_t)k + 3) / 4;
    int g = 1;
    while (g < 64 && g < ng) g <<= 1;
    return g;
}

// lw + scale * lp with pp_dist_logweight's two roundings - the product, then the sum (its term loop rounds scale * lp into an
// accumulator before it touches lw): never one fused multiply-add.
__device__ __forceinline__ float scaled_add(float lw, float scale, float lp) {
#pragma clang fp contract(off)
    const float t = scale * lp;
    return lw + t;
}

template <int KIND>
__device__ __forceinline__ constexpr int obs_n_params() {
    return (KIND == 3 || KIND == 4 || KIND == 6) ? 1 : ((KIND == 8 || KIND == 13) ? 4 : 2);
}

// One row for the lane that holds slots 4l .. 4l + 3, U groups of four per trip (U = 4 when a lane has more than one group, else
// 1: a function of k alone). The operands reach registers in one of two ways - `fast`: p1..p3 are constant along a row, p0 and x
// are each constant along a row or a run whose every row starts 16-byte aligned (one 16-byte load per group, all of a trip's
// issued before anything waits; a group index past the last full group reads group 0 again - a valid address - and a cut group is
// then read again by elements); otherwise 4-byte loads through the stride pairs (an element index past the row's end reads the
// row's last element again). Both ways fill the SAME registers and fall into the SAME instructions that evaluate and add the
// log-densities: there is one compiled copy of the arithmetic per family, so how the values were delivered cannot change a bit.
// GROUPS (pp_obs_logweight_groups): an operand marked in A.per_group starts its row at group index gr instead of r. The group
// index picks row POINTERS and nothing else: from the loads on, the code is the code of GROUPS = false.
template <int KIND, int U, bool GROUPS>
__device__ __forceinline__ void obs_row(const ObsArgs& A, bool fast, int64_t r, int64_t gr, int l, int G, int nfull, int ng, int k,
                                        float& s0, float& s1, float& s2, float& s3) {
    constexpr int NP = obs_n_params<KIND>();
    const auto row = [&](int q) -> int64_t { return GROUPS && ((A.per_group >> q) & 1) ? gr : r; };
    const float* ar = A.q[0].p + row(0) * A.q[0].rs;
    const float* xr = A.x.p + row(4) * A.x.rs;
    const float* br = NP >= 2 ? A.q[1].p + row(1) * A.q[1].rs : ar;
    const float* cr = NP >= 4 ? A.q[2].p + row(2) * A.q[2].rs : ar;
    const float* dr = NP >= 4 ? A.q[3].p + row(3) * A.q[3].rs : ar;
    const int64_t ea = A.q[0].es, eb = NP >= 2 ? A.q[1].es : 0, ec = NP >= 4 ? A.q[2].es : 0, ed = NP >= 4 ? A.q[3].es : 0,
                  ex = A.x.es;
    for (int i0 = l; i0 < ng; i0 += U * G) {
        float a[U][4], b[U][4], c[U][4], d[U][4], x[U][4];
        if (fast) {      // (nfull >= 1: the host asks for k >= 4)
            const bool a_run = ea != 0, x_run = ex != 0;
            const float4* av = reinterpret_cast<const float4*>(a_run ? ar : xr);      // (one of the two is a run)
            const float4* xv = reinterpret_cast<const float4*>(x_run ? xr : ar);
            float4 a4[U], x4[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int g = i0 + u * G, idx = g < nfull ? g : 0;
                a4[u] = av[idx];
                x4[u] = xv[idx];
            }
            const float a0 = ar[0], x0 = xr[0], b0 = br[0], c0 = cr[0], d0 = dr[0];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float af[4] = {a4[u].x, a4[u].y, a4[u].z, a4[u].w}, xf[4] = {x4[u].x, x4[u].y, x4[u].z, x4[u].w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    a[u][t] = a_run ? af[t] : a0;
                    x[u][t] = x_run ? xf[t] : x0;
                    b[u][t] = b0;
                    c[u][t] = c0;
                    d[u][t] = d0;
                }
                if (i0 + u * G == nfull && ng > nfull) {      // the row's cut group: by elements
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int e4 = 4 * nfull + t, e = e4 < k ? e4 : k - 1;
                        a[u][t] = a_run ? ar[e] : a0;
                        x[u][t] = x_run ? xr[e] : x0;
                    }
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int64_t e4 = 4 * ((int64_t)i0 + (int64_t)u * G) + t, e = e4 < k ? e4 : (int64_t)k - 1;
                    a[u][t] = ar[e * ea];
                    x[u][t] = xr[e * ex];
                    b[u][t] = NP >= 2 ? br[e * eb] : 0.0f;
                    c[u][t] = NP >= 4 ? cr[e * ec] : 0.0f;
                    d[u][t] = NP >= 4 ? dr[e * ed] : 0.0f;
                }
        }
        // the one copy of the arithmetic
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e0 = 4 * ((int64_t)i0 + (int64_t)u * G);
            const float l0 = scalar_log_prob_at(KIND, a[u][0], b[u][0], c[u][0], d[u][0], x[u][0]);
            const float l1 = scalar_log_prob_at(KIND, a[u][1], b[u][1], c[u][1], d[u][1], x[u][1]);
            const float l2 = scalar_log_prob_at(KIND, a[u][2], b[u][2], c[u][2], d[u][2], x[u][2]);
            const float l3 = scalar_log_prob_at(KIND, a[u][3], b[u][3], c[u][3], d[u][3], x[u][3]);
            if (e0 < k) s0 += l0;
            if (e0 + 1 < k) s1 += l1;
            if (e0 + 2 < k) s2 += l2;
            if (e0 + 3 < k) s3 += l3;
        }
    }
}

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

static inline int obs_kind_params(int kind) { return (kind == 3 || kind == 4 || kind == 6) ? 1 : ((kind == 8 || kind == 13) ? 4 : 2); }

static inline bool obs_aligned_run(const ObsOperand& o) {
    return o.es == 1 && (reinterpret_cast<uintptr_t>(o.p) & 15u) == 0 && (o.rs & 3) == 0;
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
    bool fast = k >= 4;
    for (int q = 1; q < np; ++q) fast = fast && A.q[q].es == 0;
    fast = fast && (A.q[0].es == 0 || obs_aligned_run(A.q[0])) && (A.x.es == 0 || obs_aligned_run(A.x)) &&
           (A.q[0].es == 1 || A.x.es == 1);
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
