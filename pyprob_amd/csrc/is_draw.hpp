// Device-side proposal draws shared by the importance-sampling kernels (is_kernels.hip, is_step_fused.hip):
// Philox4x32-10 counters, the mixture draw + log q of one particle (Mixture.sample / Mixture.log_prob,
// pyprob/distributions/mixture.py:38-63; TruncatedNormal, distributions/truncated_normal.py:25-30, 94-112; proposal
// heads proposal_normal_normal_mixture.py:20-35, proposal_uniform_truncated_normal_mixture.py:24-35,
// proposal_poisson_truncated_normal_mixture.py).
#pragma once
#include "common.hpp"
#include "head_math.hpp"

#include <math.h>

namespace pp {

// ---- Philox4x32-10 (Salmon et al. 2011), counter = particle index, key = seed ----------------------------
struct Philox {
    uint32_t c[4], k[2];
    __device__ __forceinline__ Philox(uint64_t seed, uint64_t ctr, uint32_t stream) {
        c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = stream; c[3] = 0;
        k[0] = (uint32_t)seed; k[1] = (uint32_t)(seed >> 32);
    }
    __device__ __forceinline__ void next(uint32_t out[4]) {
        uint32_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
            const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1;
            const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
            x0 = y0; x1 = y1; x2 = y2; x3 = y3;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
        c[3]++;  // next block of four for this particle
    }
};
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// ---- the five network families (kinds 0, 1, 3, 4, 5 of include/pyprob_amd.h): ONE definition per formula, as torch evaluates
// them in fp32. Every log-weight and draw kernel of is_kernels.hip, dist_kernels.hip (through dist_math.hpp) and obs_draw.hip
// calls these, so the values of the entry points agree bit for bit by construction.
// SUPPORT GUARDS are not part of the Poisson, Bernoulli and Categorical forms: they stay at the call sites and differ.
// term_log_prob (pp_logweight_*, pp_is_fused) scores Poisson and Bernoulli unguarded and truncates the Categorical index;
// scalar_log_prob / dist_log_prob (pp_dist_logweight, pp_mix_logweight) give -inf for a negative or fractional Poisson value, a
// Bernoulli value outside {0, 1} and a fractional Categorical index.

// torch.distributions.Normal.log_prob
__device__ __forceinline__ float normal_lp(float loc, float scale, float x) {
    const float t = x - loc;
    return -(t * t) / (2.0f * scale * scale) - logf(scale) - kHalfLog2Pi;
}
// Uniform(low, high), support [low, high)
__device__ __forceinline__ float uniform_lp(float low, float high, float x) {
    return (x >= low && x < high) ? -logf(high - low) : -INFINITY;
}
// Poisson(rate) at a count v: xlogy(v, rate) - rate - lgamma(v + 1)
__device__ __forceinline__ float poisson_lp(float rate, float v) {
    return (v == 0.0f ? 0.0f : v * logf(rate)) - rate - lgammaf(v + 1.0f);
}
// Bernoulli(probs) at v in {0, 1}: probs clamped to [eps, 1 - eps] (probs_to_logits), v log p + (1 - v) log(1 - p)
__device__ __forceinline__ float bernoulli_lp(float probs, float v) {
    const float q = fminf(fmaxf(probs, kFp32Eps), 1.0f - kFp32Eps);
    return v * logf(q) + (1.0f - v) * log1pf(-q);
}
// Categorical over unnormalised weights p[0..C) whose sum the caller has taken (the plain loop stays at the call sites:
// as a function of its own it compiled to another loop form in the log-weight kernels): entry k scores
// log(clamp(p[k] / sum, eps, 1 - eps)) ...
__device__ __forceinline__ float categorical_lp(const float* p, float sum, int k) { return log_clamped(p[k] / sum); }
// ... and the draw for target = u * sum is k = the first c whose cumulative weight exceeds it (the last entry if rounding leaves
// none). (k by reference, not returned: the form that leaves every draw kernel's instructions as they were.)
__device__ __forceinline__ void categorical_pick(const float* p, int C, float target, int& k) {
    float cum = 0.0f;
    k = C - 1;
    for (int c = 0; c < C; ++c) {
        cum += p[c];
        if (target < cum) { k = c; break; }
    }
}
// Normal(a, b) from two Philox words (Box-Muller, the cos branch); Uniform[a, b) from one (torch.distributions.Uniform's support)
__device__ __forceinline__ float normal_draw(float a, float b, uint32_t w0, uint32_t w1) {
    return a + b * sqrtf(-2.0f * logf(u01(w0))) * cosf(kTwoPi * u01(w1));
}
__device__ __forceinline__ float uniform_draw(float a, float b, uint32_t w0) {
    const float v = a + (b - a) * (((float)(w0 >> 8)) * (1.0f / 16777216.0f));
    return v < b ? v : a;
}

// log_prob of the prior / likelihood families state.sample and state.observe score (state.py:211, 147-149), by the formulas
// above (pp_logweight_*, pp_is_fused, pp_is_fused_groups):
//   0 Normal(mean a, stddev b)   1 Uniform(low a, high b)   3 Poisson(rate a)   4 Bernoulli(probs a)
//   5 Categorical(probs row p0[i * s0 .. + C), C = s1)
__device__ __forceinline__ float term_log_prob(int kind, const float* __restrict__ p0, int s0, const float* __restrict__ p1,
                                               int s1, float v, int64_t i) {
    if (kind == 5) {         // (the index is the truncated value)
        const float* p = p0 + i * s0;
        const int C = s1, k = (int)v;
        float sum = 0.0f;
        for (int c = 0; c < C; ++c) sum += p[c];
        if (k < 0 || k >= C) return -INFINITY;
        return categorical_lp(p, sum, k);
    }
    const float a = p0[i * s0];
    if (kind == 3) return poisson_lp(a, v);          // (no support test on the value here, nor for Bernoulli: is_draw.hpp)
    if (kind == 4) return bernoulli_lp(a, v);
    const float b = p1[i * s1];
    return kind == 0 ? normal_lp(a, b, v) : uniform_lp(a, b, v);
}

// Standard normal deviate of the SHARED-proposal kernels (the first statement of a lock-step run: is_mixture_shared_kernel and
// is_fused_kernel, one draw per particle, 10^6 particles per call): sqrt(-2 ln u1) cos(2 pi u2) on the hardware log2 / cos /
// sqrt (v_log_f32, v_cos_f32 takes its argument in revolutions, v_sqrt_f32: ~1e-6 absolute on a deviate of unit scale, ~60
// issue slots fewer than the library forms). It shapes only WHICH value is drawn; log q, log p and the likelihood terms are
// evaluated at the value that was drawn, with the accurate forms. Both kernels share this function, so the same Philox block
// gives bit-identical values on the fused and on the per-term path (tests/test_gpu_is_fused.py).
__device__ __forceinline__ float box_muller_fast(float u1, float u2) {
    return __builtin_amdgcn_sqrtf(-2.0f * __logf(u1)) * __builtin_amdgcn_cosf(u2);
}

// One particle of a mixture head (KIND 0 / 1 / 2: head_math.hpp). y = the 3K head outputs of the particle (means | scales | logits). Draws v (Philox counter `ctr`,
// stream 0x1C) unless has_value, returns log q(v) in lp.
template <int KIND>
__device__ __forceinline__ void mixture_particle(const float* __restrict__ y, const float pa, const float pb, const int K,
                                                 const bool has_value, const float v_in, const uint64_t seed,
                                                 const uint64_t ctr, float& v_out, float& lp_out) {
    float mu[MAXK], sd[MAXK], p[MAXK];
    float zmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) zmax = fmaxf(zmax, y[2 * K + k]);
    float zs = 0.0f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) {
            p[k] = expf(y[2 * K + k] - zmax);
            zs += p[k];
        }
    float ps = 0.0f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) {
            p[k] = p[k] / zs;
            ps += p[k];
        }
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) {
            p[k] = p[k] / ps;
            const HeadComp c = head_component<KIND>(y[k], y[K + k], pa, pb);
            mu[k] = c.mu;
            sd[k] = c.sd;
        }
    float v;
    if (has_value) {
        v = v_in;
    } else {
        Philox rng(seed, ctr, 0x1C);
        v = NAN;
        for (int attempt = 0; attempt < 64; ++attempt) {
            uint32_t r[4];
            rng.next(r);
            const float u0 = u01(r[0]), u1 = u01(r[1]), u2 = u01(r[2]);
            // component index ~ Categorical(p)   (Mixture.sample, distributions/mixture.py:47-63)
            float cum = 0.0f, mk = mu[0], sk = sd[0];
            bool found = false;
#pragma unroll
            for (int k = 0; k < MAXK; ++k)
                if (k < K) {
                    cum += p[k];
                    if (!found) {
                        mk = mu[k];
                        sk = sd[k];
                        if (u0 < cum) found = true;
                    }
                }
            if (KIND == 0) {
                v = mk + sk * sqrtf(-2.0f * logf(u1)) * cosf(kTwoPi * u2);   // Box-Muller
                break;
            } else {
                // inverse-CDF draw inside [low, high) with rejection (distributions/truncated_normal.py:94-112)
                const float ca = std_cdf((pa - mk) / sk), cb = std_cdf((pb - mk) / sk);
                const float uu = ca + u1 * (cb - ca);
                v = mk + sk * kSqrt2 * erfinvf(2.0f * uu - 1.0f);
                if (isfinite(v) && v >= pa && v < pb) break;
                v = NAN;
            }
        }
    }
    // log q(v)   (Mixture.log_prob, distributions/mixture.py:42-44)
    float a[MAXK], amax = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) {
            float t, alpha, beta, Z;
            a[k] = log_clamped(p[k]) + component_logpdf<KIND>(v, mu[k], sd[k], pa, pb, t, alpha, beta, Z);
            amax = fmaxf(amax, a[k]);
        }
    float lp = amax;
    if (amax > -INFINITY) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) s += expf(a[k] - amax);
        lp = amax + logf(s);
    }
    v_out = v;
    lp_out = lp;
}

}  // namespace pp
