// The per-particle images of the pair operators (is_pairs.hip, is_kde_joint.hip) and the pass that writes them.
//   Gaussian image, feature-major [K][n_pad], K = J + 2 rounded up to even:  (fp32(alpha z_1) .. fp32(alpha z_J), 0.., q, 1)
//       alpha = sqrt(log2 e) / h,  q = fp32(log2(e) (lw - max) - alpha^2 |z|^2 / 2)  (fp64 arithmetic on the fp32 z, ONE rounding)
//   distance image (DIST only), particle-major [n_pad][DS], DS = J + 1 rounded up to 4:   (z_1 .. z_J, fp32(w))
// with z_j = fp32(((double)x_j - c_j) inv_s_j), the subtraction in fp64. The inner product of the image of i, read as a ROW (.., q, 1),
// and the image of another point read as a COLUMN (.., 1, q') is the base-2 exponent of w_i w' k(z_i, z'). A particle that does not
// count (is_pairs.hip states the rule), and the padding behind n_per, has zero coordinates, q = -inf and w = 0.
//
// Everything here has internal linkage: each translation unit that includes the header compiles its own copy.
#pragma once
#include "is_groups.hpp"

namespace pp {
namespace {

constexpr int OP_TILE = 2048, THREADS = 256, PER_THREAD = 8;
constexpr int CHUNK = 256, MAXJ = PP_IS_PAIRS_MAX_COLS;
constexpr double LOG2E = 1.4426950408889634;
static_assert(OP_TILE == THREADS * PER_THREAD && OP_TILE % CHUNK == 0, "tiling");

__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ constexpr int image_k(int J) { return (J + 3) & ~1; }
__host__ __device__ constexpr int dist_stride(int J) { return (J + 4) & ~3; }
__host__ __device__ constexpr int64_t pad_of(int n) { return (int64_t)ceil_div(n, CHUNK) * CHUNK; }

struct PairCols {
    const float* p[MAXJ];
};

// The workgroup's total of v in a fixed order: lanes by DPP, then the four waves in wave order. sh: 4 doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum_dpp(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Workgroup (tile blockIdx.x, group g0 + blockIdx.y) of one side: particles tile 2048 + tid + 256 k. Per tile (sum w, sum w^2, count)
// in fp64 to wsum[(g T + tile) 3].
template <int J, bool DIST>
__global__ __launch_bounds__(THREADS) void pairs_operand_kernel(const float* __restrict__ lw, PairCols cols, int n_per, int T, int g0,
                                                                const double* __restrict__ center, const double* __restrict__ inv_scale,
                                                                const double* __restrict__ h, int64_t sh_, const double* __restrict__ stats,
                                                                const float* __restrict__ tmax, float* __restrict__ img,
                                                                float* __restrict__ dimg, double* __restrict__ wsum) {
    constexpr int K = image_k(J), DS = dist_stride(J);
    __shared__ float shmax[THREADS / 64];
    __shared__ double shsum[THREADS / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y, base = g * n_per, pad = pad_of(n_per);
    const int64_t first = (int64_t)tile * OP_TILE + tid;
    float a[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + THREADS * k;
        a[k] = i < n_per ? lw[base + i] : -INFINITY;
    }
    const double M = group_max<THREADS>(stats, tmax, g, T, a, shmax);
    const bool any = group_any(M);
    const double hg = h[g * sh_];
    const double alpha = sqrt(LOG2E) / hg, half_alpha2 = 0.5 * LOG2E / (hg * hg);
    double c[J], is[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        c[j] = center[g * J + j];
        is[j] = inv_scale[g * J + j];
    }
    float* gi = img + g * K * pad;
    float* di = DIST ? dimg + g * DS * pad : nullptr;
    double W = 0.0, W2 = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + THREADS * k;
        if (i >= pad) continue;
        float z[J];
        bool ok = particle_counted(a[k], any);
        double r2 = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            z[j] = i < n_per ? (float)(((double)cols.p[j][base + i] - c[j]) * is[j]) : 0.0f;
            ok = ok && fabs(alpha * (double)z[j]) < 0x1p30;      // (false for NaN and inf; beyond it fp32 exponents overflow)
            r2 += (double)z[j] * (double)z[j];
        }
        const double w = ok ? particle_weight(a[k], M, any) : 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            gi[j * pad + i] = ok ? (float)(alpha * (double)z[j]) : 0.0f;
            if (DIST) di[i * DS + j] = ok ? z[j] : 0.0f;
        }
#pragma unroll
        for (int f = J; f < K - 2; ++f) gi[f * pad + i] = 0.0f;
        gi[(K - 2) * pad + i] = ok ? (float)(LOG2E * ((double)a[k] - M) - half_alpha2 * r2) : -INFINITY;
        gi[(K - 1) * pad + i] = 1.0f;
        if (DIST) {
            di[i * DS + J] = (float)w;
#pragma unroll
            for (int f = J + 1; f < DS; ++f) di[i * DS + f] = 0.0f;
        }
        W += w;
        W2 += w * w;
        cnt += ok ? 1.0 : 0.0;
    }
    W = block_sum(W, shsum);
    W2 = block_sum(W2, shsum);
    cnt = block_sum(cnt, shsum);
    if (tid == 0) {
        double* o = wsum + (g * T + tile) * 3;
        o[0] = W;
        o[1] = W2;
        o[2] = cnt;
    }
}

}  // namespace
}  // namespace pp
