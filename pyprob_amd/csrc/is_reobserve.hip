// Empirical.reobserve: the particles of ONE lock-step posterior call re-scored under M new observations (the reference's
// Empirical.reobserve, pyprob/distributions/empirical.py:469-544, walks the traces one by one). The N particles' old log-weights,
// the old likelihood terms and the program's per-particle likelihood parameters are read once; out is [M, N]:
//     out[g N + j] = lw[j] + (sum_t scale_t lp_t(g, j) - old[j])
// lp_t(g, j) is obs_row's sum (obs_row.hpp: the arithmetic of pp_obs_logweight, not a second copy of it) of the k_t values of
// group g under particle j's parameters. include/pyprob_amd.h states the roundings.
#include "common.hpp"
#include "dist_math.hpp"
#include "obs_row.hpp"

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>

namespace pp {

struct ReobsTerm {
    ObsArgs a;      // (per_group = bit 4: x is addressed with the group, the parameters with the particle)
    int kind, k, fast;
    float scale;
};
struct ReobsTerms {
    ReobsTerm t[PP_REOBS_MAX_TERMS];
    int count;
};

// lw + (s - old): the difference is rounded, then the sum.
__device__ __forceinline__ float reobs_combine(float lw, float s, float old) {
#pragma clang fp contract(off)
    const float d = s - old;
    return lw + d;
}

// The lane's share of term T for particle j and group g: its four slots, added as obs_logweight_kernel adds them. G is the
// kernel's lanes per row (>= the term's own: a lane past the term's last group of four keeps its slots at -0).
template <int KIND>
__device__ __forceinline__ float reobs_lane(const ReobsTerm& T, int64_t j, int64_t g, int l, int G) {
    const int k = T.k, ng = (int)(((int64_t)k + 3) >> 2), nfull = k >> 2;
    float s0 = -0.0f, s1 = -0.0f, s2 = -0.0f, s3 = -0.0f;
    if (ng > G)
        obs_row<KIND, 4, true>(T.a, T.fast != 0, j, g, l, G, nfull, ng, k, s0, s1, s2, s3);
    else
        obs_row<KIND, 1, true>(T.a, T.fast != 0, j, g, l, G, nfull, ng, k, s0, s1, s2, s3);
    return (s0 + s1) + (s2 + s3);
}

// (T.kind comes from the kernel argument block: every lane of a wave takes the same case)
__device__ __forceinline__ float reobs_term(const ReobsTerm& T, int64_t j, int64_t g, int l, int G) {
    switch (T.kind) {
#define PP_REOBS(K) case K: return reobs_lane<K>(T, j, g, l, G)
        PP_REOBS(0); PP_REOBS(1); PP_REOBS(3); PP_REOBS(4); PP_REOBS(6); PP_REOBS(7); PP_REOBS(8); PP_REOBS(9);
        PP_REOBS(10); PP_REOBS(11); PP_REOBS(12);
        default: return reobs_lane<13>(T, j, g, l, G);
#undef PP_REOBS
    }
}

// blockIdx.x walks tiles of 4 * 64 / G particles (grid-stride), blockIdx.y owns the groups [y * chunk, (y + 1) * chunk). A row's
// G lanes keep the particle's lw and old in registers for the whole chunk; the group index is uniform over the workgroup, so a
// group's values arrive by uniform addresses and its row of `out` is written by consecutive particles. (g, j) is computed from its
// own operands only: the grid, the chunk and the other groups cannot change a bit.
// KIND >= 0: every term is of this family (the usual call: one observe, or several of one family) - the kernel then holds that
// family's arithmetic alone and its registers are that family's, not the largest family's. KIND = -1: the families differ.
template <int KIND>
__global__ __launch_bounds__(256) void is_reobserve_kernel(ReobsTerms A, int G, const float* __restrict__ lw,
                                                           const float* __restrict__ old, float* __restrict__ out, int n_groups,
                                                           int n_per, int chunk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & (G - 1);
    const int rpw = 64 / G;
    const int g0 = blockIdx.y * chunk, g1 = min(n_groups, g0 + chunk);
    const int64_t step = (int64_t)gridDim.x * 4 * rpw;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * rpw; base < n_per; base += step) {      // (wave-uniform)
        const int64_t j = base + lane / G;
        const bool live = j < n_per;
        const float lwj = live ? lw[j] : 0.0f;
        const float oldj = live && old ? old[j] : 0.0f;
        const bool kept = fabsf(lwj) <= FLT_MAX;      // (false for NaN and the infinities: the call dropped this particle)
        for (int g = g0; g < g1; ++g) {
            float s = 0.0f;
            for (int t = 0; t < A.count; ++t) {
                float acc = -0.0f;
                if (live) acc = KIND >= 0 ? reobs_lane<(KIND >= 0 ? KIND : 0)>(A.t[t], j, g, l, G) : reobs_term(A.t[t], j, g, l, G);
                for (int d = 1; d < G; d <<= 1) acc += __shfl_xor(acc, d);      // (G is wave-uniform)
                s = scaled_add(s, A.t[t].scale, acc);
            }
            if (live && l == 0) out[(int64_t)g * n_per + j] = kept ? reobs_combine(lwj, s, oldj) : lwj;
        }
    }
}

// Every term has k = 1 and the same family (the scalar observes of a program): one lane per particle, 256 particles per workgroup.
// The particle's parameters of every term are read ONCE and stay in registers for the whole chunk of groups, next to lw[j] and
// old[j]; per group a lane reads each term's value by a uniform address and evaluates ONE log-density per term. A k = 1 row of
// obs_row is slot 0 alone: (-0 + lp + -0) + (-0 + -0) has lp's bits, so the bits are those of the general kernel (and of
// pp_dist_logweight); PP_REOBS_PLAIN=1 sends such calls through the general kernel (A/B runs, tests).
template <int KIND>
__global__ __launch_bounds__(256) void is_reobserve_k1_kernel(ReobsTerms A, const float* __restrict__ lw, const float* __restrict__ old,
                                                              float* __restrict__ out, int n_groups, int n_per, int chunk) {
    constexpr int NP = obs_n_params<KIND>();
    const int g0 = blockIdx.y * chunk, g1 = min(n_groups, g0 + chunk);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_per; j += (int64_t)gridDim.x * 256) {
        const float lwj = lw[j], oldj = old ? old[j] : 0.0f;
        const bool kept = fabsf(lwj) <= FLT_MAX;
        float p[PP_REOBS_MAX_TERMS][4];
#pragma unroll
        for (int t = 0; t < PP_REOBS_MAX_TERMS; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) p[t][q] = (t < A.count && q < NP) ? A.t[t].a.q[q].p[j * A.t[t].a.q[q].rs] : 0.0f;
        for (int g = g0; g < g1; ++g) {
            float s = 0.0f;
#pragma unroll
            for (int t = 0; t < PP_REOBS_MAX_TERMS; ++t)
                if (t < A.count) {
                    const float x = A.t[t].a.x.p[(int64_t)g * A.t[t].a.x.rs];
                    s = scaled_add(s, A.t[t].scale, scalar_log_prob_at(KIND, p[t][0], p[t][1], p[t][2], p[t][3], x));
                }
            out[(int64_t)g * n_per + j] = kept ? reobs_combine(lwj, s, oldj) : lwj;
        }
    }
}

}  // namespace pp

extern "C" {

int pp_is_reobserve_groups(const pp_reobs_term* terms, int32_t count, const float* lw, const float* old, float* out,
                           int32_t n_groups, int32_t n_per, void* stream) {
    const char* who = "pp_is_reobserve_groups";
    if (!terms || count < 1 || count > PP_REOBS_MAX_TERMS || n_groups < 0 || n_per < 1 || !lw || !out) {
        pp::set_error("%s: 1..%d terms, n_groups >= 0 groups of n_per >= 1 particles, lw and out (count %d, n_groups %d, n_per %d)",
                      who, PP_REOBS_MAX_TERMS, (int)count, (int)n_groups, (int)n_per);
        return PP_EINVAL;
    }
    pp::ReobsTerms A{};
    A.count = count;
    int G = 1;
    for (int t = 0; t < count; ++t) {
        const pp_reobs_term& s = terms[t];
        if (s.kind < 0 || s.kind > PP_DIST_MAX_KIND || s.kind == 2 || s.kind == 5) {
            pp::set_error("%s: term %d: kind %d is not a scalar family (0, 1, 3, 4, 6-13)", who, t, (int)s.kind);
            return PP_EINVAL;
        }
        if (s.k < 1) {
            pp::set_error("%s: term %d: k >= 1 values per observe (k %d)", who, t, (int)s.k);
            return PP_EINVAL;
        }
        const int np = pp::obs_kind_params(s.kind);
        pp::ReobsTerm& d = A.t[t];
        for (int q = 0; q < np; ++q) {
            if (!s.params[q].p || s.params[q].row_stride < 0 || s.params[q].elem_stride < 0) {
                pp::set_error("%s: term %d: kind %d needs parameter %d (a pointer and strides >= 0)", who, t, (int)s.kind, q);
                return PP_EINVAL;
            }
            d.a.q[q] = pp::ObsOperand{s.params[q].p, s.params[q].row_stride, s.params[q].elem_stride};
        }
        if (!s.x.p || s.x.row_stride < 0 || s.x.elem_stride < 0) {
            pp::set_error("%s: term %d: no value block (a pointer and strides >= 0)", who, t);
            return PP_EINVAL;
        }
        d.a.x = pp::ObsOperand{s.x.p, s.x.row_stride, s.x.elem_stride};
        d.a.per_group = PP_OBS_PER_GROUP_X;
        d.kind = s.kind;
        d.k = s.k;
        d.scale = s.scale;
        d.fast = pp::obs_fast_path(d.a, np, s.k) ? 1 : 0;
        G = std::max(G, pp::obs_group(s.k));
    }
    if (n_groups == 0) return 0;
    // tiles x chunks: enough workgroups for every CU also where N is small and M large, whole chunks of groups per workgroup
    // (lw and old are read once per chunk) where N alone fills the device
    const int64_t rpb = 4 * (64 / G);
    const int64_t tiles = (n_per + rpb - 1) / rpb;
    const int64_t nx = std::min<int64_t>(tiles, 65536);
    int64_t ny = std::min<int64_t>(std::min<int64_t>(n_groups, 65535), std::max<int64_t>(1, (4096 + nx - 1) / nx));
    const int chunk = (int)((n_groups + ny - 1) / ny);
    ny = (n_groups + chunk - 1) / chunk;
    int kind = A.t[0].kind;
    for (int t = 1; t < count; ++t)
        if (A.t[t].kind != kind) kind = -1;
    const dim3 grid((unsigned)nx, (unsigned)ny), block(256);
    hipStream_t st = pp::as_stream(stream);
    bool k1 = kind >= 0;
    for (int t = 0; t < count; ++t) k1 = k1 && A.t[t].k == 1;
    const char* plain = getenv("PP_REOBS_PLAIN");
    if (k1 && !(plain && plain[0] == '1')) {      // (G == 1: a tile is 256 particles here as there)
#define PP_REOBS_K1(K)                                                                                                           \
    case K:                                                                                                                      \
        hipLaunchKernelGGL((pp::is_reobserve_k1_kernel<K>), grid, block, 0, st, A, lw, old, out, n_groups, n_per, chunk);          \
        break
        switch (kind) {
            PP_REOBS_K1(0); PP_REOBS_K1(1); PP_REOBS_K1(3); PP_REOBS_K1(4); PP_REOBS_K1(6); PP_REOBS_K1(7);
            PP_REOBS_K1(8); PP_REOBS_K1(9); PP_REOBS_K1(10); PP_REOBS_K1(11); PP_REOBS_K1(12); PP_REOBS_K1(13);
            default: break;
        }
#undef PP_REOBS_K1
        PP_LAUNCH_CHECK(who);
        return 0;
    }
#define PP_REOBS_LAUNCH(K)                                                                                                       \
    case K:                                                                                                                      \
        hipLaunchKernelGGL((pp::is_reobserve_kernel<K>), grid, block, 0, st, A, G, lw, old, out, n_groups, n_per, chunk);          \
        break
    switch (kind) {
        PP_REOBS_LAUNCH(0); PP_REOBS_LAUNCH(1); PP_REOBS_LAUNCH(3); PP_REOBS_LAUNCH(4); PP_REOBS_LAUNCH(6); PP_REOBS_LAUNCH(7);
        PP_REOBS_LAUNCH(8); PP_REOBS_LAUNCH(9); PP_REOBS_LAUNCH(10); PP_REOBS_LAUNCH(11); PP_REOBS_LAUNCH(12); PP_REOBS_LAUNCH(13);
        default: hipLaunchKernelGGL((pp::is_reobserve_kernel<-1>), grid, block, 0, st, A, G, lw, old, out, n_groups, n_per, chunk);
    }
#undef PP_REOBS_LAUNCH
    PP_LAUNCH_CHECK(who);
    return 0;
}

}  // extern "C"
