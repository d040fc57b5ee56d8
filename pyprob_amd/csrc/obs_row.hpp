// One row of a vector-valued likelihood: the operand addressing, the 256-slot summation and the per-element arithmetic shared by
// pp_obs_logweight / pp_obs_logweight_groups (obs_logweight.hip) and pp_is_reobserve_groups (is_reobserve.hip). There is ONE
// copy of this text; a row's bits cannot depend on which of the kernels evaluated it.
#pragma once
#include "common.hpp"
#include "dist_math.hpp"

#include <math.h>

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

static inline int obs_kind_params(int kind) { return (kind == 3 || kind == 4 || kind == 6) ? 1 : ((kind == 8 || kind == 13) ? 4 : 2); }

static inline bool obs_aligned_run(const ObsOperand& o) {
    return o.es == 1 && (reinterpret_cast<uintptr_t>(o.p) & 15u) == 0 && (o.rs & 3) == 0;
}

// The 16-byte load path of obs_row may be taken: k >= 4, p1..p3 constant along a row, p0 and x each constant along a row or an
// aligned run, one of the two a run.
static inline bool obs_fast_path(const ObsArgs& A, int np, int k) {
    bool fast = k >= 4;
    for (int q = 1; q < np; ++q) fast = fast && A.q[q].es == 0;
    return fast && (A.q[0].es == 0 || obs_aligned_run(A.q[0])) && (A.x.es == 0 || obs_aligned_run(A.x)) &&
           (A.q[0].es == 1 || A.x.es == 1);
}

}  // namespace pp
