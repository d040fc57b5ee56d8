// Device log-weight terms and draws for every pyprob distribution family (include/pyprob_amd.h, ABI 15): the prior-proposal
// engine in lock step (state.sample's prior branch pyprob/state.py:191-201), uncontrolled draws of an IC run (:218-221),
// the likelihoods of state.observe (:118-155) and pyprob.factor (:113-115). The families' formulas are in dist_math.hpp.
#include "common.hpp"
#include "dist_math.hpp"

#include <math.h>

#include <algorithm>

namespace pp {

struct DistTerm {
    int kind, s[4], sx;
    const float* p[4];
    const float* x;
    float scale;
};
struct DistTerms {
    DistTerm t[PP_DIST_MAX_TERMS];
    int count;
};

// log p(x) of one term at particle r. `kind` comes from the kernel argument block: every lane of a wave takes the same branch.
__device__ __forceinline__ float dist_log_prob(const DistTerm& d, int64_t r) {
    const float x = d.x[r * d.sx];
    if (d.kind == 2) return x;
    if (d.kind == 5) {       // Categorical: row r * s[0] of C = s[1] probabilities; a fractional index is outside the support
        const float* p = d.p[0] + r * d.s[0];
        const int C = d.s[1], k = (int)x;
        float sum = 0.0f;
        for (int c = 0; c < C; ++c) sum += p[c];
        return (!(x >= 0.0f) || k >= C || (float)k != x) ? -INFINITY : categorical_lp(p, sum, k);
    }
    return scalar_log_prob(d.kind, d.p, d.s, r, x);
}

// lw[r] += sum_t scale_t log p_t(x_t[r]); r = rows[j] (rows != NULL) or j; lp_out[r] = the single term's log p
__global__ __launch_bounds__(256) void dist_logweight_kernel(DistTerms T, float* __restrict__ lw, float* __restrict__ lp_out,
                                                             const int64_t* __restrict__ rows, int m) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const int64_t r = rows ? rows[j] : (int64_t)j;
        float acc = 0.0f;
        for (int q = 0; q < T.count; ++q) {
            const float lp = dist_log_prob(T.t[q], r);
            if (lp_out) lp_out[r] = lp;
            acc += T.t[q].scale * lp;
        }
        if (lw) lw[r] += acc;
    }
}

// out[r] ~ family(params_r). Philox key = seed, counter = offset + r, stream id per statement (prior_draw_kernel's scheme);
// kinds 0 / 1 call prior_draw_kernel's normal_draw / uniform_draw on the same first block: pp_prior_draw's values, bit for bit.
// One instance per kind: the rejection samplers' registers do not weigh on the transform samplers' occupancy.
template <int KIND>
__global__ __launch_bounds__(256) void dist_draw_kernel(DistTerm d, const int64_t* __restrict__ rows, int m, uint64_t seed,
                                                        uint64_t offset, uint32_t stream_id, float* __restrict__ out) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const int64_t r = rows ? rows[j] : (int64_t)j;
        Philox rng(seed, offset + (uint64_t)r, stream_id);
        float v;
        if (KIND == 5) {          // Categorical: row r * s[0] of C = s[1] probabilities
            const float* p = d.p[0] + r * d.s[0];
            const int C = d.s[1];
            uint32_t w[4];
            rng.next(w);
            float sum = 0.0f;
            for (int c = 0; c < C; ++c) sum += p[c];
            int k;
            categorical_pick(p, C, u01(w[0]) * sum, k);
            v = (float)k;
        } else {
            const float a = d.p[0][r * d.s[0]];
            const float b = KIND == 3 || KIND == 4 || KIND == 6 ? 0.0f : d.p[1][r * d.s[1]];
            const bool four = KIND == 8 || KIND == 13;
            v = draw_one<KIND>(a, b, four ? d.p[2][r * d.s[2]] : 0.0f, four ? d.p[3][r * d.s[3]] : 0.0f, rng);
        }
        out[r] = v;
    }
}

// parameters each kind reads (Categorical: p0 only, C in p_stride[1]; Factor: none)
static inline int dist_n_params(int kind) {
    if (kind == 2) return 0;
    if (kind == 3 || kind == 4 || kind == 5 || kind == 6) return 1;
    if (kind == 8 || kind == 13) return 4;
    return 2;
}

static bool dist_ok(const pp_dist& d, const char* what) {
    if (d.kind < 0 || d.kind > PP_DIST_MAX_KIND) {
        set_error("%s: unknown distribution kind %d", what, d.kind);
        return false;
    }
    const int np = dist_n_params(d.kind);
    for (int q = 0; q < np; ++q)
        if (!d.p[q] || d.p_stride[q] < 0) {
            set_error("%s: kind %d needs parameter %d", what, d.kind, q);
            return false;
        }
    if (d.kind == 5 && d.p_stride[1] < 1) {
        set_error("%s: Categorical needs the number of categories in p_stride[1]", what);
        return false;
    }
    return true;
}

static DistTerm dist_term(const pp_dist& d, const float* x, int sx, float scale) {
    DistTerm t{};
    t.kind = d.kind;
    for (int q = 0; q < 4; ++q) {
        t.s[q] = d.p_stride[q];
        t.p[q] = d.p[q];
    }
    t.x = x;
    t.sx = sx;
    t.scale = scale;
    return t;
}

// ---- Mixture (pyprob/distributions/mixture.py): K scalar components of any kinds, K weights per particle or shared -------------
struct MixComp {
    int kind, s[4];
    const float* p[4];
};
struct MixArgs {
    int count, sp;              // K; row stride of probs (0: one shared row)
    const float* probs;
    MixComp c[PP_MIX_MAX_COMPONENTS];
};

// lp[r] = logsumexp_k( log clamp(w[r,k] / sum_k w[r,k]) + log p_k(x[r]) ) (mixture.py:15-16, 38-45; util.clamp_probs); lw[r] += scale lp,
// lp_out[r] = lp. The component loop runs on the argument block (k is wave-uniform); the log-sum-exp keeps a running maximum, so
// no per-component array exists: -inf when every component gives -inf, NaN as soon as one term is NaN.
__global__ __launch_bounds__(256) void mix_logweight_kernel(MixArgs M, const float* __restrict__ xs, int sx, float scale,
                                                            float* __restrict__ lw, float* __restrict__ lp_out,
                                                            const int64_t* __restrict__ rows, int m) {
    const int K = M.count;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const int64_t r = rows ? rows[j] : (int64_t)j;
        const float x = xs[r * sx];
        const float* w = M.probs + r * M.sp;
        float sum = 0.0f;
        for (int k = 0; k < K; ++k) sum += w[k];
        float mx = -INFINITY, acc = 0.0f;
        bool nan = false;
        for (int k = 0; k < K; ++k) {
            const float q = w[k] / sum;
            const float lq = q == q ? log_clamped(q) : NAN;
            const float t = lq + scalar_log_prob(M.c[k].kind, M.c[k].p, M.c[k].s, r, x);
            if (t != t) {
                nan = true;
            } else if (t > mx) {
                acc = acc * expf(mx - t) + 1.0f;
                mx = t;
            } else if (t > -INFINITY) {
                acc += t == mx ? 1.0f : expf(t - mx);
            }
        }
        const float lp = nan ? NAN : (mx > -INFINITY ? mx + logf(acc) : -INFINITY);
        if (lp_out) lp_out[r] = lp;
        if (lw) lw[r] += scale * lp;
    }
}

// out[r] ~ Mixture for the lanes whose selected component has kind KIND (the host launches one instance per distinct kind of
// the mixture). Selection: first word of Philox(seed, offset + r, stream_id | 0x80000000), dist_draw_kernel<5>'s categorical_pick on the
// unclamped weights (Categorical(probs).sample(), mixture.py:47-50). Draw: Philox(seed, offset + r, stream_id) - dist_draw_kernel's
// stream, so K = 1 or K identical components give pp_dist_draw's values. The selected component's parameters are picked in a
// wave-uniform loop over the argument block under the lane mask (no per-lane index into it).
template <int KIND>
__global__ __launch_bounds__(256) void mix_draw_kernel(MixArgs M, const int64_t* __restrict__ rows, int m, uint64_t seed,
                                                       uint64_t offset, uint32_t stream_id, float* __restrict__ out) {
    const int K = M.count;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const int64_t r = rows ? rows[j] : (int64_t)j;
        Philox pick(seed, offset + (uint64_t)r, stream_id | 0x80000000u);
        uint32_t w[4];
        pick.next(w);
        const float* p = M.probs + r * M.sp;
        float sum = 0.0f;
        for (int k = 0; k < K; ++k) sum += p[k];
        int sel;
        categorical_pick(p, K, u01(w[0]) * sum, sel);
        float a = 0.0f, b = 0.0f, c = 0.0f, d = 0.0f;
        bool mine = false;
        for (int k = 0; k < K; ++k) {
            if (M.c[k].kind != KIND) continue;       // wave-uniform
            if (k == sel) {
                mine = true;
                a = M.c[k].p[0][r * M.c[k].s[0]];
                if (!(KIND == 3 || KIND == 4 || KIND == 6)) b = M.c[k].p[1][r * M.c[k].s[1]];
                if (KIND == 8 || KIND == 13) {
                    c = M.c[k].p[2][r * M.c[k].s[2]];
                    d = M.c[k].p[3][r * M.c[k].s[3]];
                }
            }
        }
        if (mine) {
            Philox rng(seed, offset + (uint64_t)r, stream_id);
            out[r] = draw_one<KIND>(a, b, c, d, rng);
        }
    }
}

static bool mix_ok(const pp_mixture* mx, const char* what) {
    if (!mx || mx->count < 1 || mx->count > PP_MIX_MAX_COMPONENTS) {
        set_error("%s: a mixture has 1..%d components", what, PP_MIX_MAX_COMPONENTS);
        return false;
    }
    if (!mx->probs || (mx->probs_stride != 0 && mx->probs_stride != mx->count)) {
        set_error("%s: probs is one shared row (probs_stride 0) or one row of K per particle (probs_stride K)", what);
        return false;
    }
    for (int k = 0; k < mx->count; ++k) {
        const pp_dist& d = mx->comp[k];
        if (d.kind == 2 || d.kind == 5) {
            set_error("%s: component %d: Factor and Categorical are not mixture components", what, k);
            return false;
        }
        if (!dist_ok(d, what)) return false;
    }
    return true;
}

static MixArgs mix_args(const pp_mixture& mx) {
    MixArgs M{};
    M.count = mx.count;
    M.sp = mx.probs_stride;
    M.probs = mx.probs;
    for (int k = 0; k < mx.count; ++k) {
        M.c[k].kind = mx.comp[k].kind;
        for (int q = 0; q < 4; ++q) {
            M.c[k].s[q] = mx.comp[k].p_stride[q];
            M.c[k].p[q] = mx.comp[k].p[q];
        }
    }
    return M;
}

}  // namespace pp

int pp_dist_logweight(const pp_dist_term* terms, int32_t count, float* lw, float* lp_out, const int64_t* rows, int32_t m, int32_t n,
                      void* stream) {
    if (count < 1 || count > PP_DIST_MAX_TERMS || !terms || (lp_out && count != 1) || (!lw && !lp_out) || n < 0 || m < 0 ||
        (!rows && m != n) || m > n) {
        pp::set_error("pp_dist_logweight: bad argument (1..%d terms, lp_out with one term, m = n without a row list)",
                      PP_DIST_MAX_TERMS);
        return PP_EINVAL;
    }
    pp::DistTerms T{};
    T.count = count;
    for (int q = 0; q < count; ++q) {
        const pp_dist_term& s = terms[q];
        if (!pp::dist_ok(s.d, "pp_dist_logweight")) return PP_EINVAL;
        if (!s.x || s.x_stride < 0) {
            pp::set_error("pp_dist_logweight: term %d has no value", q);
            return PP_EINVAL;
        }
        T.t[q] = pp::dist_term(s.d, s.x, s.x_stride, s.scale);
    }
    if (m == 0) return 0;
    hipLaunchKernelGGL(pp::dist_logweight_kernel, dim3(std::min(2048, pp::cdiv(m, 256))), dim3(256), 0, pp::as_stream(stream), T, lw,
                       lp_out, rows, m);
    PP_LAUNCH_CHECK("pp_dist_logweight");
    return 0;
}

int pp_dist_draw(const pp_dist* d, const int64_t* rows, int32_t m, int32_t n, uint64_t seed, uint64_t offset, uint32_t stream_id,
                 float* out, void* stream) {
    if (!d || !out || n < 0 || m < 0 || (!rows && m != n) || m > n) {
        pp::set_error("pp_dist_draw: bad argument (m = n without a row list)");
        return PP_EINVAL;
    }
    if (!pp::dist_ok(*d, "pp_dist_draw")) return PP_EINVAL;
    if (d->kind == 2) {
        pp::set_error("pp_dist_draw: a Factor has no draw");
        return PP_EINVAL;
    }
    if (m == 0) return 0;
    const dim3 grid(std::min(2048, pp::cdiv(m, 256))), block(256);
    hipStream_t st = pp::as_stream(stream);
    const pp::DistTerm t = pp::dist_term(*d, nullptr, 0, 1.0f);
#define PP_DIST_DRAW(K) \
    case K: hipLaunchKernelGGL(pp::dist_draw_kernel<K>, grid, block, 0, st, t, rows, m, seed, offset, stream_id, out); break
    switch (d->kind) {
        PP_DIST_DRAW(0); PP_DIST_DRAW(1); PP_DIST_DRAW(3); PP_DIST_DRAW(4); PP_DIST_DRAW(5); PP_DIST_DRAW(6); PP_DIST_DRAW(7);
        PP_DIST_DRAW(8); PP_DIST_DRAW(9); PP_DIST_DRAW(10); PP_DIST_DRAW(11); PP_DIST_DRAW(12); PP_DIST_DRAW(13);
        default: break;
    }
#undef PP_DIST_DRAW
    PP_LAUNCH_CHECK("pp_dist_draw");
    return 0;
}

int pp_mix_logweight(const pp_mixture* mx, const float* x, int32_t x_stride, float scale, float* lw, float* lp_out,
                     const int64_t* rows, int32_t m, int32_t n, void* stream) {
    if (!x || x_stride < 0 || (!lw && !lp_out) || n < 0 || m < 0 || (!rows && m != n) || m > n) {
        pp::set_error("pp_mix_logweight: bad argument (a value, lw or lp_out, m = n without a row list)");
        return PP_EINVAL;
    }
    if (!pp::mix_ok(mx, "pp_mix_logweight")) return PP_EINVAL;
    if (m == 0) return 0;
    hipLaunchKernelGGL(pp::mix_logweight_kernel, dim3(std::min(2048, pp::cdiv(m, 256))), dim3(256), 0, pp::as_stream(stream),
                       pp::mix_args(*mx), x, x_stride, scale, lw, lp_out, rows, m);
    PP_LAUNCH_CHECK("pp_mix_logweight");
    return 0;
}

int pp_mix_draw(const pp_mixture* mx, const int64_t* rows, int32_t m, int32_t n, uint64_t seed, uint64_t offset,
                uint32_t stream_id, float* out, void* stream) {
    if (!out || n < 0 || m < 0 || (!rows && m != n) || m > n) {
        pp::set_error("pp_mix_draw: bad argument (m = n without a row list)");
        return PP_EINVAL;
    }
    if (stream_id & 0x80000000u) {
        pp::set_error("pp_mix_draw: the top bit of stream_id belongs to the component selection");
        return PP_EINVAL;
    }
    if (!pp::mix_ok(mx, "pp_mix_draw")) return PP_EINVAL;
    if (m == 0) return 0;
    const dim3 grid(std::min(2048, pp::cdiv(m, 256))), block(256);
    hipStream_t st = pp::as_stream(stream);
    const pp::MixArgs M = pp::mix_args(*mx);
    uint32_t kinds = 0;          // one launch per distinct kind of the mixture
    for (int k = 0; k < mx->count; ++k) kinds |= 1u << mx->comp[k].kind;
#define PP_MIX_DRAW(K) \
    if (kinds & (1u << K)) hipLaunchKernelGGL(pp::mix_draw_kernel<K>, grid, block, 0, st, M, rows, m, seed, offset, stream_id, out)
    PP_MIX_DRAW(0); PP_MIX_DRAW(1); PP_MIX_DRAW(3); PP_MIX_DRAW(4); PP_MIX_DRAW(6); PP_MIX_DRAW(7); PP_MIX_DRAW(8);
    PP_MIX_DRAW(9); PP_MIX_DRAW(10); PP_MIX_DRAW(11); PP_MIX_DRAW(12); PP_MIX_DRAW(13);
#undef PP_MIX_DRAW
    PP_LAUNCH_CHECK("pp_mix_draw");
    return 0;
}
