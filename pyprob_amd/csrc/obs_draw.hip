// Synthetic observation BLOCKS of vectorised prior-trace generation (pyprob/nn/dataset.py:50-62 run n times; the observe branch of
// pyprob/state.py draws distribution.sample() for every observe of a PRIOR_FOR_INFERENCE_NETWORK trace): one row of k values per
// trace - an image for the CNN2D5C embedding, a k-vector for FEEDFORWARD. The scalar columns stay with prior_draw_kernel
// (is_kernels.hip); this kernel is its k-wide form and for k = 1 gives the same bits.
#include "common.hpp"
#include "is_draw.hpp"

#include <math.h>

#include <algorithm>

namespace pp {

// out[r * k + e] ~ Normal(p0, p1) (kind 0) | Uniform[p0, p1) (kind 1); p0 read at p0[r * r0 + e * e0], p1 likewise (element
// strides: 0 / 0 a scalar, 0 / 1 one shared row, 1 / 0 one value per trace, k / 1 a full [n, k] block - no parameter is ever
// materialised to [n, k]).
// Counters: element group q = e >> 2 of row r takes the Philox block (key seed; counter words lo, hi of offset + r, stream_id, q).
// Uniform element e uses word e & 3; Normal elements 4q, 4q + 1 are the cos and sin branches of Box-Muller on words (0, 1),
// 4q + 2, 4q + 3 those on words (2, 3) - so element 0 is prior_draw_kernel's value of the row, and a row depends on
// (seed, offset + r, stream_id) only.
// Work: one lane = one group = one Philox block and one 16-byte store (scalar stores where the group is cut by the row's end or
// its address is not 16-byte aligned: odd k, or an `out` that is only 4-byte aligned); consecutive lanes take consecutive groups
// of a row, so a wave writes 1 KiB contiguously. The group index is 64-bit: n * ceil(k / 4) may pass 2^31.
__global__ __launch_bounds__(256) void obs_draw_kernel(int kind, const float* __restrict__ p0, int64_t r0, int e0,
                                                       const float* __restrict__ p1, int64_t r1, int e1, int n, int k, uint64_t seed,
                                                       uint64_t offset, uint32_t stream_id, float* __restrict__ out) {
    const uint32_t gpr = ((uint32_t)k + 3u) >> 2;      // groups per row
    const uint64_t total = (uint64_t)n * gpr;
    const bool narrow = total <= 0xFFFFFFFFull;        // (uniform: the 32-bit division is a fraction of the 64-bit one)
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        const uint64_t r = narrow ? (uint64_t)((uint32_t)g / gpr) : g / gpr;
        const uint32_t q = (uint32_t)(g - r * gpr);
        const int e = (int)(q << 2);
        const int m = min(4, k - e);                   // elements of this group inside the row
        Philox rng(seed, offset + r, stream_id);
        rng.c[3] = q;
        uint32_t w[4];
        rng.next(w);
        const float* a_row = p0 + (int64_t)r * r0;
        const float* b_row = p1 + (int64_t)r * r1;
        float v[4];
        if (kind == 0) {
            const float rad0 = sqrtf(-2.0f * logf(u01(w[0]))), ang0 = kTwoPi * u01(w[1]);
            const float rad1 = sqrtf(-2.0f * logf(u01(w[2]))), ang1 = kTwoPi * u01(w[3]);
            const float z[4] = {cosf(ang0), sinf(ang0), cosf(ang1), sinf(ang1)};
            const float rad[4] = {rad0, rad0, rad1, rad1};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < m) {
                    const float a = a_row[(int64_t)(e + t) * e0], b = b_row[(int64_t)(e + t) * e1];
                    v[t] = a + b * rad[t] * z[t];
                } else {
                    v[t] = 0.0f;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < m) {
                    const float a = a_row[(int64_t)(e + t) * e0], b = b_row[(int64_t)(e + t) * e1];
                    v[t] = uniform_draw(a, b, w[t]);
                } else {
                    v[t] = 0.0f;
                }
            }
        }
        float* dst = out + (int64_t)r * k + e;
        if (m == 4 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < m) dst[t] = v[t];
        }
    }
}

}  // namespace pp

extern "C" {

int pp_obs_draw(int32_t kind, const float* p0, int64_t p0_row_stride, int32_t p0_elem_stride, const float* p1, int64_t p1_row_stride,
                int32_t p1_elem_stride, int32_t n, int32_t k, uint64_t seed, uint64_t offset, uint32_t stream_id, float* out,
                void* stream) {
    if ((kind != 0 && kind != 1) || k < 1 || n < 0) {
        pp::set_error("pp_obs_draw: Normal (0) or Uniform (1), k >= 1 values per row, n >= 0 rows (kind %d, k %d, n %d)", (int)kind,
                      (int)k, (int)n);
        return PP_EINVAL;
    }
    if (n == 0) return 0;
    if (!(p0 && p1 && out)) {
        pp::set_error("pp_obs_draw: two parameter arrays and an output block");
        return PP_EINVAL;
    }
    const int64_t groups = (int64_t)n * (((int64_t)k + 3) / 4);
    hipLaunchKernelGGL(pp::obs_draw_kernel, dim3((unsigned)std::min<int64_t>(2048, (groups + 255) / 256)), dim3(256), 0,
                       pp::as_stream(stream), kind, p0, p0_row_stride, p0_elem_stride, p1, p1_row_stride, p1_elem_stride, n, k, seed,
                       offset, stream_id, out);
    PP_LAUNCH_CHECK("pp_obs_draw");
    return 0;
}

}  // extern "C"
