// What the joint-mixture kernels (is_gmm_joint.hip: the EM; is_proposal.hip: draws and densities of a fitted mixture) share: the packed
// layouts of a component of K full-covariance Gaussians over J coordinates, the Cholesky factorisation of its covariance and the
// log-density of a point from the component's constants. Everything has internal linkage: each translation unit compiles its own copy.
#pragma once
#include "common.hpp"

#include <math.h>

namespace pp {
namespace {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;

__host__ __device__ constexpr int tri_of(int J) { return J * (J + 1) / 2; }
// Parameters of one component: pi | mu [J] | Sigma, upper triangle row-major. The sums of one component have the same shape.
__host__ __device__ constexpr int params_of(int J) { return 1 + J + tri_of(J); }
// Constants of one component: mu [J] | L^-1, lower triangle row-major | c
__host__ __device__ constexpr int consts_of(int J) { return J + tri_of(J) + 1; }
// (j, m), j <= m, of an upper triangle stored row by row; (j, m), m <= j, of a lower triangle stored row by row
__host__ __device__ constexpr int upper_at(int J, int j, int m) { return j * J - j * (j - 1) / 2 + (m - j); }
__host__ __device__ constexpr int lower_at(int j, int m) { return j * (j + 1) / 2 + m; }

// Thread k of a workgroup: the Cholesky factor of the J x J matrix whose upper triangle is `cov` into lf, the factor's inverse into
// li (both lower triangles, row by row, in LDS: the indices are run-time values) and sum_j log L_jj. False where a pivot is not
// positive (a NaN included): lf and li are then incomplete.
__device__ bool factorise(const double* cov, int J, double* lf, double* li, double* logdet) {
    double ld = 0.0;
    for (int j = 0; j < J; ++j) {
        for (int m = 0; m <= j; ++m) {
            double s = cov[upper_at(J, m, j)];
            for (int q = 0; q < m; ++q) s -= lf[lower_at(j, q)] * lf[lower_at(m, q)];
            if (m < j) {
                lf[lower_at(j, m)] = s / lf[lower_at(m, m)];
            } else {
                if (!(s > 0.0)) return false;
                lf[lower_at(j, j)] = sqrt(s);
                ld += log(lf[lower_at(j, j)]);
            }
        }
    }
    for (int j = 0; j < J; ++j) {
        const double inv = 1.0 / lf[lower_at(j, j)];
        li[lower_at(j, j)] = inv;
        for (int m = 0; m < j; ++m) {
            double s = 0.0;
            for (int q = m; q < j; ++q) s += lf[lower_at(j, q)] * li[lower_at(q, m)];
            li[lower_at(j, m)] = -s * inv;
        }
    }
    *logdet = ld;
    return true;
}

// l_ik = c_k - 1/2 |L_k^-1 (x - mu_k)|^2 with the constants of component k at ck (LDS); d <- x - mu_k.
template <int J>
__device__ __forceinline__ double log_density(const float (&x)[J], const double* ck, double (&d)[J]) {
#pragma unroll
    for (int j = 0; j < J; ++j) d[j] = (double)x[j] - ck[j];
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double z = ck[J + lower_at(j, 0)] * d[0];
#pragma unroll
        for (int m = 1; m <= j; ++m) z += ck[J + lower_at(j, m)] * d[m];
        q += z * z;
    }
    return ck[J + tri_of(J)] - 0.5 * q;
}

}  // namespace
}  // namespace pp
