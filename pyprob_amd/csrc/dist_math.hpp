// Log-densities and samplers of every pyprob distribution family (pyprob/distributions/*.py, v1.5.0), one particle per lane:
// the device half of pp_dist_logweight / pp_dist_draw (dist_kernels.hip). The log-densities restate, operation for operation
// in fp32, what the torch.distributions classes behind pyprob's wrappers compute - except where that arithmetic itself fails
// (TruncatedNormal intervals inside one tail: kTruncTailFrom; lgamma differences at large counts: kLgammaFp64From; DESIGN.md
// "Where the log-densities leave the reference's fp32 arithmetic") -; the samplers draw from a particle's own
// Philox stream (counter = offset + particle, is_draw.hpp) and take a fresh block of four words per rejection round.
#pragma once
#include "common.hpp"
#include "head_math.hpp"
#include "is_draw.hpp"

#include <math.h>

namespace pp {

constexpr int kDistMaxRounds = 64;      // PP_DIST_MAX_ROUNDS
constexpr float kLog2Pi = 1.83787706640934548356f;
constexpr float kPi = 3.14159265358979323846f;
// lgammaf carries half an ulp of its own value: 6e-5 at lgamma(256) = 1161, 4e-3 at lgamma(1e4), 6e-2 at lgamma(1e5). Poisson,
// Binomial and Beta subtract such values from each other and from products of the same size, and what is left is a log-density of
// a few units. From this count / concentration on, those terms are taken in fp64 and the result is rounded once (per lane; below
// it every family keeps the reference's fp32 operations).
constexpr float kLgammaFp64From = 256.0f;
constexpr float kTruncTailFrom = 3.0f;      // lp_truncnormal: one-tail intervals from here on leave the reference's fp32 formula

// torch.xlogy(a, x): 0 where a == 0 (x not NaN), a * log(x) otherwise
__device__ __forceinline__ float xlogyf(float a, float x) { return (a == 0.0f && x == x) ? 0.0f : a * logf(x); }

// ---- log-densities (kinds 6-13; the formulas of kinds 0-5 are is_draw.hpp's, shared with term_log_prob) ------

// 6 Exponential(rate): log(rate) - rate x, support [0, inf)
// (the fused multiply-add is written out: it is what the compiler's contraction gives where one lane scores one value, and a
// kernel that scores several values per lane - pp_obs_logweight, whose products the compiler packs in pairs - must not differ)
__device__ __forceinline__ float lp_exponential(float rate, float x) {
    return x >= 0.0f ? fmaf(-rate, x, logf(rate)) : -INFINITY;
}

// 7 Gamma(concentration a, rate b): xlogy(a, b) + xlogy(a - 1, x) - b x - lgamma(a), support [0, inf)
__device__ __forceinline__ float lp_gamma(float a, float b, float x) {
    if (!(x >= 0.0f)) return -INFINITY;
    return xlogyf(a, b) + xlogyf(a - 1.0f, x) - b * x - lgammaf(a);
}

// 8 Beta(c1, c0, low, high) as pyprob's beta.py:38-40 scores it: torch Beta.log_prob (Dirichlet of (y, 1 - y)) at
// y = (x - low) / (high - low), with no -log(high - low) Jacobian. Support y in [0, 1].
__device__ __forceinline__ float lbeta_large(float c1, float c0) {
#pragma clang fp contract(off)
    return (float)(lgamma((double)c1 + (double)c0) - (lgamma((double)c1) + lgamma((double)c0)));
}
__device__ __forceinline__ float lp_beta(float c1, float c0, float low, float high, float x) {
    const float y = (x - low) / (high - low);
    if (!(y >= 0.0f && y <= 1.0f)) return -INFINITY;
    if (c1 + c0 >= kLgammaFp64From) return (xlogyf(c1 - 1.0f, y) + xlogyf(c0 - 1.0f, 1.0f - y)) + lbeta_large(c1, c0);
    return (xlogyf(c1 - 1.0f, y) + xlogyf(c0 - 1.0f, 1.0f - y)) + lgammaf(c1 + c0) - (lgammaf(c1) + lgammaf(c0));
}

// 9 LogNormal(loc, scale): Normal.log_prob(log x) - log x (ExpTransform's Jacobian), support (0, inf)
__device__ __forceinline__ float lp_lognormal(float loc, float scale, float x) {
    if (!(x > 0.0f)) return -INFINITY;
    const float y = logf(x);
    return normal_lp(loc, scale, y) - y;
}

// 10 Weibull(scale l, concentration k) = Exponential(1) pushed through x -> x^(1/k) -> l x (torch's TransformedDistribution):
// log k - log l + (k - 1) log(x / l) - (x / l)^k, support (0, inf)
__device__ __forceinline__ float lp_weibull(float l, float k, float x) {
    if (!(x > 0.0f)) return -INFINITY;
    const float z = x / l;
    const float lz = logf(z);
    return logf(k) - logf(l) + (k - 1.0f) * lz - expf(k * lz);
}

// 11 Binomial(total_count n, logits t): k t - lgamma(k + 1) - lgamma(n - k + 1) - (n max(t, 0) + n log1p(exp(-|t|)) -
// lgamma(n + 1)), support the integers 0..n
__device__ __forceinline__ float lp_binomial_large(float n, float t, float k) {
#pragma clang fp contract(off)
    const double dn = n, dt = t, dk = k;
    const double norm = dn * fmax(dt, 0.0) + dn * log1p(exp(-fabs(dt))) - lgamma(dn + 1.0);
    return (float)(dk * dt - lgamma(dk + 1.0) - lgamma(dn - dk + 1.0) - norm);
}
__device__ __forceinline__ float lp_binomial(float n, float t, float k) {
    if (!(k >= 0.0f && k <= n && k == floorf(k))) return -INFINITY;
    if (n >= kLgammaFp64From) return lp_binomial_large(n, t, k);
    const float clamp0 = (fmaxf(t, 0.0f) + t - fminf(t, 0.0f)) * 0.5f;      // torch's _clamp_by_zero
    const float norm = n * clamp0 + n * log1pf(expf(-fabsf(t))) - lgammaf(n + 1.0f);
    return k * t - lgammaf(k + 1.0f) - lgammaf(n - k + 1.0f) - norm;
}

// torch.distributions.von_mises._log_modified_bessel_fn(x, order=0): Abramowitz-Stegun polynomials
__device__ __forceinline__ float log_i0(float x) {
    if (x < 3.75f) {
        float y = x / 3.75f;
        y = y * y;
        const float p = 1.0f + y * (3.5156229f + y * (3.0899424f + y * (1.2067492f + y * (0.2659732f + y * (0.0360768f +
                                                                                                         y * 0.0045813f)))));
        return logf(p);
    }
    const float y = 3.75f / x;
    const float p = 0.39894228f + y * (0.01328592f + y * (0.00225319f + y * (-0.00157565f + y * (0.00916281f + y * (-0.02057706f +
                    y * (0.02635537f + y * (-0.01647633f + y * 0.00392377f)))))));
    return x - 0.5f * logf(x) + logf(p);
}

// 12 VonMises(loc, concentration k): k cos(x - loc) - log(2 pi) - log I0(k), support the real line
__device__ __forceinline__ float lp_vonmises(float loc, float k, float x) {
    if (!isfinite(x)) return -INFINITY;
    return k * cosf(x - loc) - kLog2Pi - log_i0(k);
}

// An interval [ta, tb] inside one tail, 3 <= ta < tb in that tail's own coordinates, scored at zt in the same coordinates:
// log phi(zt) - log Z with Z = Q(ta) - Q(tb), Q(t) = erfcx(t / sqrt 2) exp(-t^2 / 2) / 2. The exp(-ta^2 / 2) of Q(ta) is taken
// out of Z and joined with phi's exponent, -(zt - ta)(zt + ta) / 2, so nothing underflows at any ta:
//   log Z + ta^2 / 2 = log(erfcx(ta / sqrt 2) / 2) + log1p(-exp(-(tb - ta)(tb + ta) / 2) erfcx(tb / sqrt 2) / erfcx(ta / sqrt 2))
// No contraction: the three log-weight kernels must give the same bits.
__device__ __forceinline__ float truncnormal_tail_lp(float zt, float ta, float tb, float sd) {
#pragma clang fp contract(off)
    const float ea = erfcxf(ta * kInvSqrt2), eb = erfcxf(tb * kInvSqrt2);
    const float ratio = expf(-0.5f * ((tb - ta) * (tb + ta))) * (eb / ea);
    return -0.5f * ((zt - ta) * (zt + ta)) - kHalfLog2Pi - logf(sd) - logf(0.5f * ea) - log1pf(-ratio);
}

// 13 TruncatedNormal(mean, stddev, low, high) as truncated_normal.py:40-45 scores it: log(1[low <= x <= high]) +
// N(0, 1).log_prob((x - mean) / stddev) - log(stddev Z), Z = Phi(beta) - Phi(alpha) - except where the whole interval lies
// beyond 3 standard deviations on one side (alpha >= 3 or beta <= -3). There Z <= 1.35e-3, the fp32 difference of two
// 0.5 (1 + erf) carries ~1e-7 absolute - 7e-5 of Z at 3 sigma, 4e-2 at 5, all of it from 5.5 on (Z = 0, log-density +inf) -
// and the log-density is taken in the tail's own coordinates instead (truncnormal_tail_lp). The branch is per lane.
__device__ __forceinline__ float lp_truncnormal(float mu, float sd, float low, float high, float x) {
    if (!(x >= low && x <= high)) return -INFINITY;
    const float z = (x - mu) / sd;
    const float alpha = (low - mu) / sd, beta = (high - mu) / sd;
    if (alpha >= kTruncTailFrom) return truncnormal_tail_lp(z, alpha, beta, sd);
    if (beta <= -kTruncTailFrom) return truncnormal_tail_lp(-z, -beta, -alpha, sd);
    const float Z = std_cdf(beta) - std_cdf(alpha);
    return -(z * z) / 2.0f - kHalfLog2Pi - logf(sd * Z);
}

// 3 Poisson(rate) at a count from kLgammaFp64From on (below it: poisson_lp of is_draw.hpp)
__device__ __forceinline__ float lp_poisson_large(float rate, float v) {
#pragma clang fp contract(off)
    return (float)((double)v * log((double)rate) - (double)rate - lgamma((double)v + 1.0));
}

// log p(x) of a scalar family (kinds 0, 1, 3, 4, 6-13) from the parameter VALUES a..d = p0..p3 (the kinds with fewer parameters
// ignore the rest): the one per-element definition behind pp_dist_logweight, pp_mix_logweight and pp_obs_logweight. `kind` comes
// from a kernel argument block or a template argument, so every lane of a wave takes the same branch.
__device__ __forceinline__ float scalar_log_prob_at(int kind, float a, float b, float c, float d, float x) {
    switch (kind) {
        case 0: return normal_lp(a, b, x);
        case 1: return uniform_lp(a, b, x);
        case 3:      // (guarded here: is_draw.hpp)
            if (!(x >= 0.0f && x == floorf(x))) return -INFINITY;
            return x >= kLgammaFp64From ? lp_poisson_large(a, x) : poisson_lp(a, x);
        case 4: return (x == 0.0f || x == 1.0f) ? bernoulli_lp(a, x) : -INFINITY;
        case 6: return lp_exponential(a, x);
        case 7: return lp_gamma(a, b, x);
        case 8: return lp_beta(a, b, c, d, x);
        case 9: return lp_lognormal(a, b, x);
        case 10: return lp_weibull(a, b, x);
        case 11: return lp_binomial(a, b, x);
        case 12: return lp_vonmises(a, b, x);
        default: return lp_truncnormal(a, b, c, d, x);
    }
}

// The same at particle r: parameter q is p[q][r * s[q]] (only the parameters the kind has are read); shared by
// dist_logweight_kernel and mix_logweight_kernel.
__device__ __forceinline__ float scalar_log_prob(int kind, const float* const* p, const int* s, int64_t r, float x) {
    const bool one = kind == 3 || kind == 4 || kind == 6, four = kind == 8 || kind == 13;
    const float a = p[0][r * s[0]];
    const float b = one ? 0.0f : p[1][r * s[1]];
    const float c = four ? p[2][r * s[2]] : 0.0f;
    const float d = four ? p[3][r * s[3]] : 0.0f;
    return scalar_log_prob_at(kind, a, b, c, d, x);
}

// ---- samplers --------------------------------------------------------------------------------------------------------
// A lane's stream: the first block is drawn by the caller's Philox; every further round calls rng.next() again.

__device__ __forceinline__ float normal_from(uint32_t a, uint32_t b) {
    return sqrtf(-2.0f * logf(u01(a))) * cosf(kTwoPi * u01(b));
}

// log of a Gamma(a, 1) deviate (Marsaglia-Tsang 2000). a < 1: G(a) = G(a + 1) U^(1/a), added in log space so that
// a = 0.05 does not underflow to 0. NaN after kDistMaxRounds rejected rounds.
__device__ __forceinline__ float log_gamma_draw(float a, Philox& rng) {
    uint32_t r[4];
    float boost = 0.0f;
    if (a < 1.0f) {
        rng.next(r);
        boost = logf(u01(r[0])) / a;
        a += 1.0f;
    }
    const float d = a - 1.0f / 3.0f, c = 1.0f / sqrtf(9.0f * d);
    for (int round = 0; round < kDistMaxRounds; ++round) {
        rng.next(r);
        const float z = normal_from(r[0], r[1]);
        const float t = 1.0f + c * z;
        if (t <= 0.0f) continue;
        const float v = t * t * t;
        const float u = u01(r[2]);
        if (u < 1.0f - 0.0331f * (z * z) * (z * z) || logf(u) < 0.5f * z * z + d * (1.0f - v + logf(v)))
            return logf(d) + logf(v) + boost;
    }
    return NAN;
}

// Poisson(lam): multiplication for lam < 10, PTRS (Hoermann 1993) above; the acceptance test in fp64 (k log lam -
// lgamma(k + 1) loses the test's precision in fp32 at large rates)
__device__ __forceinline__ float poisson_draw(float lam, Philox& rng) {
    uint32_t r[4];
    if (!(lam >= 0.0f) || !isfinite(lam)) return NAN;
    if (lam == 0.0f) return 0.0f;
    if (lam < 10.0f) {
        const float L = expf(-lam);
        float p = 1.0f;
        int k = 0;
        for (int round = 0; round < kDistMaxRounds; ++round) {
            rng.next(r);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                p *= u01(r[q]);
                if (p <= L) return (float)k;
                ++k;
            }
        }
        return NAN;
    }
    const double dl = lam, slam = sqrt(dl), loglam = log(dl);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int round = 0; round < kDistMaxRounds; ++round) {
        rng.next(r);
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
            const double U = (double)u01(r[q]) - 0.5, V = (double)u01(r[q + 1]);
            const double us = 0.5 - fabs(U);
            const double k = floor((2.0 * a / us + b) * U + dl + 0.43);
            if (us >= 0.07 && V <= vr) return (float)k;
            if (k < 0.0 || (us < 0.013 && V > us)) continue;
            if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -dl + k * loglam - lgamma(k + 1.0)) return (float)k;
        }
    }
    return NAN;
}

// Binomial(n, logits t): with q = min(p, 1 - p), inversion for n q < 10, BTRS (Hoermann 1993) otherwise; k -> n - k when
// p > 1/2
__device__ __forceinline__ float binomial_draw(float nf, float t, Philox& rng) {
    uint32_t r[4];
    if (!(nf >= 0.0f) || nf != floorf(nf) || t != t) return NAN;
    const double n = nf;
    const double p = 1.0 / (1.0 + exp(-(double)t));
    const bool flip = p > 0.5;
    const double q = flip ? 1.0 - p : p;
    if (n == 0.0 || q == 0.0) return flip ? nf : 0.0f;
    double k = -1.0;
    if (n * q < 10.0) {
        const double s = q / (1.0 - q), g = s * (n + 1.0), q0 = exp(n * log1p(-q));
        const int cap = (int)fmin(n, 110.0);      // n q < 10: P(k > 110) is far below fp32 resolution
        for (int round = 0; round < kDistMaxRounds && k < 0.0; ++round) {
            rng.next(r);
            double U = (double)u01(r[0]) + (double)(r[1] >> 8) * (1.0 / 16777216.0) * (1.0 / 16777216.0);   // 48-bit uniform
            double px = q0;
            int j = 0;
            while (U > px && j < cap) {
                U -= px;
                ++j;
                px *= g / j - s;
            }
            if (U <= px) k = j;
        }
    } else {
        const double spq = sqrt(n * q * (1.0 - q));
        const double b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * q, c = n * q + 0.5;
        const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq, lpq = log(q / (1.0 - q));
        const double m = floor((n + 1.0) * q), h = lgamma(m + 1.0) + lgamma(n - m + 1.0);
        for (int round = 0; round < kDistMaxRounds && k < 0.0; ++round) {
            rng.next(r);
#pragma unroll
            for (int w = 0; w < 4; w += 2) {
                if (k >= 0.0) break;
                const double U = (double)u01(r[w]) - 0.5, V = (double)u01(r[w + 1]);
                const double us = 0.5 - fabs(U);
                const double kk = floor((2.0 * a / us + b) * U + c);
                if (kk < 0.0 || kk > n) continue;
                if (us >= 0.07 && V <= vr) { k = kk; break; }
                const double lv = log(V * alpha / (a / (us * us) + b));
                if (lv <= h - lgamma(kk + 1.0) - lgamma(n - kk + 1.0) + (kk - m) * lpq) k = kk;
            }
        }
    }
    if (k < 0.0) return NAN;
    return (float)(flip ? n - k : k);
}

// VonMises(loc, k): Best-Fisher, as torch's _rejection_sample in fp64 (fp32 loses the proposal for small k); the result
// wrapped into [-pi, pi). k below 1e-5 takes torch's Taylor form of the proposal parameter.
__device__ __forceinline__ float vonmises_draw(float loc, float kf, Philox& rng) {
    uint32_t r[4];
    if (!(kf > 0.0f) || !isfinite(kf)) return NAN;
    const double k = kf;
    double pr;
    if (k < 1e-5) {
        pr = 1.0 / k + k;
    } else {
        const double tau = 1.0 + sqrt(1.0 + 4.0 * k * k), rho = (tau - sqrt(2.0 * tau)) / (2.0 * k);
        pr = (1.0 + rho * rho) / (2.0 * rho);
    }
    for (int round = 0; round < kDistMaxRounds; ++round) {
        rng.next(r);
        const double u1 = u01(r[0]), u2 = u01(r[1]), u3 = u01(r[2]);
        const double z = cos(M_PI * u1);
        const double f = (1.0 + pr * z) / (pr + z);
        const double c = k * (pr - f);
        if ((c * (2.0 - c) - u2) > 0.0 || (log(c / u2) + 1.0 - c >= 0.0)) {
            const double th = (u3 < 0.5 ? -1.0 : 1.0) * acos(fmin(fmax(f, -1.0), 1.0));
            double x = fmod(th + (double)loc + M_PI, 2.0 * M_PI);
            if (x < 0.0) x += 2.0 * M_PI;
            return (float)(x - M_PI);
        }
    }
    return NAN;
}

// TruncatedNormal(mu, sd, low, high): the inverse CDF between Phi(alpha) and Phi(beta) (truncated_normal.py:94-112), a new
// round while the fp32 value lands outside [low, high]. An interval inside one tail is inverted in that tail's own
// coordinates (Phi(x) = erfc(-x / sqrt 2) / 2 below 0, 1 - Phi(x) = erfc(x / sqrt 2) / 2 above): 1 + erf(x / sqrt 2) keeps
// ~3 digits at x = -4 in fp32, and the draws of TruncatedNormal(3, 0.5, -1, 1) came out on a coarse grid.
// Beyond 4 standard deviations (the whole interval in one far tail, where erfc underflows fp32 from ~13 sigma on) the draw
// is Robert's (1995) rejection sampler on the standardised interval [ta, tb] of the tail, mirrored for the lower tail: an
// exponential proposal ta + E / lambda, lambda = (ta + sqrt(ta^2 + 4)) / 2, accepted with probability exp(-(z - lambda)^2 / 2),
// or for an interval narrower than 1 / lambda a uniform proposal accepted with probability exp(-(z^2 - ta^2) / 2). Both
// accept at least ~1/e of the proposals for any interval.
__device__ __forceinline__ float truncnormal_tail_draw(float mu, float sd, float low, float high, float ta, float tb, float sign,
                                                       Philox& rng) {
    uint32_t r[4];
    const float lam = 0.5f * (ta + sqrtf(ta * ta + 4.0f));
    const bool uniform = lam * (tb - ta) < 1.0f;
    for (int round = 0; round < kDistMaxRounds; ++round) {
        rng.next(r);
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
            const float u = u01(r[q]), w = u01(r[q + 1]);
            float z, acc;
            if (uniform) {
                z = ta + (tb - ta) * u;
                acc = expf(-0.5f * (z - ta) * (z + ta));
            } else {
                z = ta - logf(u) / lam;
                acc = z <= tb ? expf(-0.5f * (z - lam) * (z - lam)) : 0.0f;
            }
            if (w < acc) {
                const float v = mu + sign * z * sd;
                if (v >= low && v <= high) return v;
            }
        }
    }
    return NAN;
}

__device__ __forceinline__ float truncnormal_draw(float mu, float sd, float low, float high, Philox& rng) {
    uint32_t r[4];
    if (!(sd > 0.0f) || !(low < high)) return NAN;
    const float a = (low - mu) / sd, b = (high - mu) / sd;
    if (a >= 4.0f) return truncnormal_tail_draw(mu, sd, low, high, a, b, 1.0f, rng);
    if (b <= -4.0f) return truncnormal_tail_draw(mu, sd, low, high, -b, -a, -1.0f, rng);
    const int side = b <= 0.0f ? -1 : (a >= 0.0f ? 1 : 0);
    float ca, cb;
    if (side < 0) {
        ca = 0.5f * erfcf(-a * kInvSqrt2);
        cb = 0.5f * erfcf(-b * kInvSqrt2);
    } else if (side > 0) {
        ca = 0.5f * erfcf(a * kInvSqrt2);       // upper-tail masses: ca >= cb
        cb = 0.5f * erfcf(b * kInvSqrt2);
    } else {
        ca = std_cdf(a);
        cb = std_cdf(b);
    }
    for (int round = 0; round < kDistMaxRounds; ++round) {
        rng.next(r);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p = ca + u01(r[q]) * (cb - ca);
            const float z = side < 0 ? -kSqrt2 * erfcinvf(2.0f * p) : (side > 0 ? kSqrt2 * erfcinvf(2.0f * p) : kSqrt2 * erfinvf(2.0f * p - 1.0f));
            const float v = z * sd + mu;
            if (v >= low && v <= high) return v;
        }
    }
    return NAN;
}

// One draw of scalar family KIND from the lane's stream (parameters a..d = p0..p3 of include/pyprob_amd.h; the kinds with
// fewer parameters ignore the rest): the body of dist_draw_kernel<KIND>, shared with mix_draw_kernel<KIND>.
template <int KIND>
__device__ __forceinline__ float draw_one(float a, float b, float c, float d, Philox& rng) {
    uint32_t w[4];
    float v;
    switch (KIND) {
        case 0:
            rng.next(w);
            v = normal_draw(a, b, w[0], w[1]);
            break;
        case 1:
            rng.next(w);
            v = uniform_draw(a, b, w[0]);
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
            v = c + y * (d - c);
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
        default: v = truncnormal_draw(a, b, c, d, rng); break;
    }
    return v;
}

}  // namespace pp
