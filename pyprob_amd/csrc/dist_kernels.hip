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
    if (d.kind == 5) {       // Categorical: row r * s[0] of C = s[1] probabilities (is_kernels.hip's term_log_prob)
        const float* p = d.p[0] + r * d.s[0];
        const int C = d.s[1];
        float sum = 0.0f;
        for (int c = 0; c < C; ++c) sum += p[c];
        const int k = (int)x;
        if (!(x >= 0.0f) || k >= C || (float)k != x) return -INFINITY;
        return logf(fminf(fmaxf(p[k] / sum, kFp32Eps), 1.0f - kFp32Eps));
    }
    const float a = d.p[0][r * d.s[0]];
    switch (d.kind) {
        case 0: return lp_normal(a, d.p[1][r * d.s[1]], x);
        case 1: {
            const float b = d.p[1][r * d.s[1]];
            return (x >= a && x < b) ? -logf(b - a) : -INFINITY;
        }
        case 3: return (x >= 0.0f && x == floorf(x)) ? (x == 0.0f ? 0.0f : x * logf(a)) - a - lgammaf(x + 1.0f) : -INFINITY;
        case 4: {
            if (!(x == 0.0f || x == 1.0f)) return -INFINITY;
            const float q = fminf(fmaxf(a, kFp32Eps), 1.0f - kFp32Eps);
            return x * logf(q) + (1.0f - x) * log1pf(-q);
        }
        case 6: return lp_exponential(a, x);
        case 7: return lp_gamma(a, d.p[1][r * d.s[1]], x);
        case 8: return lp_beta(a, d.p[1][r * d.s[1]], d.p[2][r * d.s[2]], d.p[3][r * d.s[3]], x);
        case 9: return lp_lognormal(a, d.p[1][r * d.s[1]], x);
        case 10: return lp_weibull(a, d.p[1][r * d.s[1]], x);
        case 11: return lp_binomial(a, d.p[1][r * d.s[1]], x);
        case 12: return lp_vonmises(a, d.p[1][r * d.s[1]], x);
        default: return lp_truncnormal(a, d.p[1][r * d.s[1]], d.p[2][r * d.s[2]], d.p[3][r * d.s[3]], x);
    }
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
// kinds 0 / 1 are prior_draw_kernel's arithmetic on the same first block, so the values are bit-identical to pp_prior_draw.
// One instance per kind: the rejection samplers' registers do not weigh on the transform samplers' occupancy.
template <int KIND>
__global__ __launch_bounds__(256) void dist_draw_kernel(DistTerm d, const int64_t* __restrict__ rows, int m, uint64_t seed,
                                                        uint64_t offset, uint32_t stream_id, float* __restrict__ out) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        const int64_t r = rows ? rows[j] : (int64_t)j;
        Philox rng(seed, offset + (uint64_t)r, stream_id);
        float v;
        if (KIND == 5) {          // Categorical: the first c whose cumulative probability exceeds u * sum
            const float* p = d.p[0] + r * d.s[0];
            const int C = d.s[1];
            uint32_t w[4];
            rng.next(w);
            float sum = 0.0f;
            for (int c = 0; c < C; ++c) sum += p[c];
            const float target = u01(w[0]) * sum;
            float cum = 0.0f;
            int k = C - 1;
            for (int c = 0; c < C; ++c) {
                cum += p[c];
                if (target < cum) { k = c; break; }
            }
            v = (float)k;
        } else {
            const float a = d.p[0][r * d.s[0]];
            const float b = KIND == 3 || KIND == 4 || KIND == 6 ? 0.0f : d.p[1][r * d.s[1]];
            uint32_t w[4];
            switch (KIND) {
                case 0:
                    rng.next(w);
                    v = a + b * sqrtf(-2.0f * logf(u01(w[0]))) * cosf(kTwoPi * u01(w[1]));
                    break;
                case 1:
                    rng.next(w);
                    v = a + (b - a) * (((float)(w[0] >> 8)) * (1.0f / 16777216.0f));
                    v = v < b ? v : a;
                    break;
                case 3: v = poisson_draw(a, rng); break;
                case 4:
                    rng.next(w);
                    v = u01(w[0]) < a ? 1.0f : 0.0f;
                    break;
                case 6:
                    rng.next(w);
                    v = -logf(u01(w[0])) / a;
                    break;
                case 7: v = (a > 0.0f && b > 0.0f) ? expf(log_gamma_draw(a, rng) - logf(b)) : NAN; break;
                case 8: {
                    float y = NAN;
                    if (a > 0.0f && b > 0.0f) {
                        const float g1 = log_gamma_draw(a, rng), g0 = log_gamma_draw(b, rng);
                        // G1 / (G1 + G0) from the logs: the smaller share s = e / (1 + e), e = exp(-|g1 - g0|), stays > 0 down
                        // to the denormals, and y = 1 - s near 1 is rounded once
                        const float e = expf(-fabsf(g1 - g0)), s = e / (1.0f + e);
                        y = g1 >= g0 ? 1.0f - s : s;
                    }
                    const float lo = d.p[2][r * d.s[2]], hi = d.p[3][r * d.s[3]];
                    v = lo + y * (hi - lo);
                    break;
                }
                case 9:
                    rng.next(w);
                    v = expf(a + b * normal_from(w[0], w[1]));
                    break;
                case 10:
                    rng.next(w);
                    v = a * powf(-logf(u01(w[0])), 1.0f / b);
                    break;
                case 11: v = binomial_draw(a, b, rng); break;
                case 12: v = vonmises_draw(a, b, rng); break;
                default: v = truncnormal_draw(a, b, d.p[2][r * d.s[2]], d.p[3][r * d.s[3]], rng); break;
            }
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
