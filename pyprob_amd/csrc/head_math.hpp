// Proposal-head math shared by the training heads (kernels.hip, panel.hip, panel16.hip) and the importance-sampling
// draws (is_draw.hpp, is_kernels.hip, is_step_fused.hip): constants, the map from a head's raw outputs to one mixture
// component, its log-density and its gradient, and the one-lane-per-component loss and backward of the training heads.
// Every helper computes term for term what its callers wrote out before: the A/B tests compare paths bit for bit.
//
// KIND 0: Normal components around a Normal prior (pa, pb) = (mean, stddev); KIND 1: TruncatedNormal components inside
// a Uniform prior [pa, pb] (stddev = range/1000 + sigmoid(y) 10 range); KIND 2: the Poisson head - TruncatedNormal
// components on the fixed interval [pa, pb] = [0, 40] with stddev = exp(y) (proposal_normal_normal_mixture.py:20-35,
// proposal_uniform_truncated_normal_mixture.py:24-35, proposal_poisson_truncated_normal_mixture.py:19-37).
#pragma once
#include "common.hpp"

#include <math.h>

namespace pp {

constexpr int MAXK = 16;
constexpr float kFp32Eps = 1.1920928955078125e-07f;   // torch.finfo(float32).eps (util.clamp_probs)
constexpr float kHalfLog2Pi = 0.91893853320467274178f;
constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;
constexpr float kLogEps = -18.420680743952367f;        // log(1e-8), pyprob/util.py:35
constexpr float kSqrt2 = 1.41421356237309504880f;
constexpr float kTwoPi = 6.28318530717958647692f;

__device__ __forceinline__ float std_cdf(float x) { return 0.5f * (1.0f + erff(x * kInvSqrt2)); }
__device__ __forceinline__ float std_pdf(float x) { return kInvSqrt2Pi * expf(-0.5f * x * x); }

// sigmoid / tanh on the hardware exp2 and reciprocal (v_exp_f32, v_rcp_f32: ~1 ulp each; absolute error of the results
// ~1e-7, asserted by tests/test_gpu_is_step_fused.py against the float64 oracle)
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// log of a mixture weight clamped to [eps, 1 - eps] (util.clamp_probs). A NaN weight stays NaN, as torch's clamp keeps it:
// fmaxf / fminf alone would turn it into eps and a NaN logit into a finite log_prob.
__device__ __forceinline__ float log_clamped(float p) {
    return p == p ? logf(fminf(fmaxf(p, kFp32Eps), 1.0f - kFp32Eps)) : p;
}

// One component from the head outputs (ymu, ysd) of its mean and scale; sm, ss = sigmoid(ymu), sigmoid(ysd) are what the
// backward of KIND 1 / 2 needs (0 for KIND 0).
struct HeadComp {
    float mu, sd, sm, ss;
};

template <int KIND>
__device__ __forceinline__ HeadComp head_component(float ymu, float ysd, float pa, float pb) {
    HeadComp c{0.0f, 0.0f, 0.0f, 0.0f};
    if (KIND == 0) {
        c.mu = pa + ymu * pb;
        c.sd = expf(ysd) * pb;
    } else {
        const float rng = pb - pa;
        c.sm = sigmoidf_(ymu);
        c.ss = sigmoidf_(ysd);
        c.mu = pa + c.sm * rng;
        c.sd = KIND == 2 ? expf(ysd) : rng / 1000.0f + c.ss * rng * 10.0f;
    }
    return c;
}

// log f(v) of one component with the TruncatedNormal normaliser Z = Phi(beta) - Phi(alpha) given (KIND 1 / 2; unused for
// KIND 0); tt = (v - mu) / sd. Outside [pa, pb] a TruncatedNormal density is -inf.
template <int KIND>
__device__ __forceinline__ float component_logpdf(float v, float mu, float sd, float pa, float pb, float Z, float& tt) {
    tt = (v - mu) / sd;
    if (KIND == 0) return -0.5f * tt * tt - logf(sd) - kHalfLog2Pi;
    const bool inside = v >= pa && v <= pb;
    return (inside ? 0.0f : -INFINITY) + (-0.5f * tt * tt - kHalfLog2Pi) - logf(sd * Z);
}

// the same, computing alpha = (pa - mu) / sd, beta = (pb - mu) / sd and Z (KIND 1 / 2; left untouched for KIND 0)
template <int KIND>
__device__ __forceinline__ float component_logpdf(float v, float mu, float sd, float pa, float pb, float& tt, float& alpha,
                                                  float& beta, float& Z) {
    tt = (v - mu) / sd;
    if (KIND == 0) return -0.5f * tt * tt - logf(sd) - kHalfLog2Pi;
    alpha = (pa - mu) / sd;
    beta = (pb - mu) / sd;
    Z = std_cdf(beta) - std_cdf(alpha);
    const bool inside = v >= pa && v <= pb;
    return (inside ? 0.0f : -INFINITY) + (-0.5f * tt * tt - kHalfLog2Pi) - logf(sd * Z);
}

// d lp / d mu and d lp / d sd of a TruncatedNormal component with responsibility resp
__device__ __forceinline__ void truncated_grad(float resp, float tt, float sd, float alpha, float beta, float Z, float& dmu,
                                               float& dsd) {
    const float fa = std_pdf(alpha), fb = std_pdf(beta);
    dmu = resp * (tt / sd - (fa - fb) / (sd * Z));
    dsd = resp * ((tt * tt - 1.0f) / sd - (alpha * fa - beta * fb) / (sd * Z));
}

// grad_scale d lp / d (ymu, ysd) of one component with responsibility resp (the training heads' lane form)
template <int KIND>
__device__ __forceinline__ void component_grad(float resp, float grad_scale, const HeadComp& c, float tt, float alpha,
                                               float beta, float Z, float pa, float pb, float& d0, float& d1) {
    if (KIND == 0) {
        d0 = grad_scale * resp * tt / c.sd * pb;
        d1 = grad_scale * resp * (tt * tt - 1.0f);
    } else {
        const float rng = pb - pa;
        float dmu, dsd;
        truncated_grad(resp, tt, c.sd, alpha, beta, Z, dmu, dsd);
        d0 = grad_scale * dmu * rng * c.sm * (1.0f - c.sm);
        d1 = grad_scale * dsd * (KIND == 2 ? c.sd : rng * 10.0f * c.ss * (1.0f - c.ss));
    }
}

// ---- one mixture component per lane: the loss and backward of the training heads (head_tail_kernel, the 8- and 16-row
// panels). Lanes with comp = false (k >= K) take part in the row reductions with neutral values; sum / max reduce over
// the lanes of one row. lane_mixture_logprob returns log q(v) (NaN if any component is NaN, like the reference's
// logsumexp); lane_mixture_grad then gives grad_scale d lp / d (ymu, ysd, yz) of the lane's component, zero unless live.
struct LaneMixture {
    HeadComp c;
    float pi, ps, p;             // softmax weight, sum of the weights, renormalised weight
    float tt, alpha, beta, Z;    // alpha, beta, Z: KIND 1 / 2
    float a;                     // log p + log f(v)
};

template <int KIND, class Sum, class Max>
__device__ __forceinline__ float lane_mixture_logprob(bool comp, float ymu, float ysd, float yz, float v, float pa, float pb,
                                                      Sum sum, Max max, LaneMixture& m) {
    const float zmax = max(yz);
    const float e = comp ? expf(yz - zmax) : 0.0f;
    const float pi = e / sum(e);
    const float ps = sum(pi);
    const float p = pi / ps;
    const HeadComp c = head_component<KIND>(ymu, ysd, pa, pb);
    float tt, alpha = 0.0f, beta = 0.0f, Z = 1.0f;
    const float cl = component_logpdf<KIND>(v, c.mu, c.sd, pa, pb, tt, alpha, beta, Z);
    const float a = comp ? log_clamped(p) + cl : -INFINITY;
    const float amax = max(a);
    float lp = amax;
    if (amax > -INFINITY) lp = amax + logf(sum(comp ? expf(a - amax) : 0.0f));
    if (sum((comp && a != a) ? 1.0f : 0.0f) > 0.0f) lp = NAN;   // NaN in a component poisons the logsumexp
    m = LaneMixture{c, pi, ps, p, tt, alpha, beta, Z, a};
    return lp;
}

// responsibilities and the softmax / normalisation chain (see oracle/ic_oracle.py head_*_mixture)
template <int KIND, class Sum>
__device__ __forceinline__ void lane_mixture_grad(const LaneMixture& m, bool comp, bool live, float lp, float pa, float pb,
                                                  float grad_scale, Sum sum, float& d0, float& d1, float& d2) {
    d0 = 0.f, d1 = 0.f, d2 = 0.f;
    const float resp = (comp && live) ? expf(m.a - lp) : 0.0f;
    const bool in = (m.p >= kFp32Eps) && (m.p <= 1.0f - kFp32Eps);
    float dp = (comp && in) ? resp / m.p : 0.0f;
    const float dpp = sum(dp * m.p);
    dp = comp ? (dp - dpp) / m.ps : 0.0f;
    const float dpipi = sum(dp * m.pi);
    if (comp && live) {
        component_grad<KIND>(resp, grad_scale, m.c, m.tt, m.alpha, m.beta, m.Z, pa, pb, d0, d1);
        d2 = grad_scale * m.pi * (dp - dpipi);
    }
}

}  // namespace pp
