// What the statistics of a lock-step posterior (is_resample.hip, is_moments.hip, is_hist.hip, is_sort.hip) agree on: which
// particles of a group count, what a particle weighs, and the host plumbing of a call over M groups of n_per particles.
//
// THE WEIGHT AND THE SKIP RULE. The maximum M_g of a group is the largest FINITE log-weight of its n_per particles: the caller's
// stats[6 g] (what pp_is_stats / pp_is_fused_groups reduced) or, without statistics, found here (group_max). A particle counts
// where M_g is finite and its own log-weight is finite (particle_counted); it weighs w = exp((double)lw - M_g) in fp64
// (particle_weight), every other particle weighs 0 and is SKIPPED: its values - uninitialised rows of a diverged path - may be
// loaded but select nothing and enter no sum. The integer statistics (histogram, distinct values) clamp w at 1
// (particle_weight_clamped: a caller's maximum below the true one must not overflow the fixed-point sum) and add
// llrint(w 2^S), S = hist_shift(n_per) (fixed_mass); the fp64 ones (cdf, moments) do not clamp. A maximum does not depend on
// the order it is taken in, so with and without `stats` a kernel sees the same M_g and gives the same bits.
//
// Everything here has internal linkage: each translation unit that includes the header compiles its own copy.
#pragma once
#include "common.hpp"

#include <math.h>

#include <algorithm>

namespace pp {
namespace {

// ---- host: shapes, launch chunks, workspace ------------------------------------------------------------------------------
inline int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }
inline int tiles_of(int n_per, int tile) { return cdiv(n_per, tile); }

// A call indexes its particles (and its draws or results: `n` per group) with 32 bits.
inline bool groups_count_ok(int M, int n) { return (int64_t)M * n <= 0x7fffffff; }
inline bool groups_shape_ok(int M, int n_per) { return M >= 0 && n_per >= 1 && groups_count_ok(M, n_per); }
#define PP_CHECK_GROUPS(name, M, n_per)                                                                            \
    do {                                                                                                           \
        PP_CHECK_ARG((n_per) >= 1 && (M) >= 0, name ": n_per >= 1 and n_groups >= 0");                             \
        PP_CHECK_ARG(pp::groups_count_ok(M, n_per), name ": more than 2^31 - 1 particles per call: shard the groups"); \
    } while (0)

// The groups of a call ride on grid dimension y or z, which is 16 bits wide: fn(g0, groups) per launch chunk, in order.
constexpr int GROUP_CHUNK = 65535;
template <class F>
inline void for_each_group_chunk(int M, F&& fn) {
    for (int g0 = 0; g0 < M; g0 += GROUP_CHUNK) fn(g0, std::min(GROUP_CHUNK, M - g0));
}

// Cuts a workspace into arrays that start on 256-byte boundaries, in the order taken. A null base only measures: every array
// is then null. bytes() asks for 256 more than the arrays (the caller's pointer need not be aligned further than malloc's).
struct Carver {
    char* base;
    int64_t offset = 0;
    explicit Carver(void* p) : base(static_cast<char*>(p)) {}
    template <class T>
    T* take(int64_t bytes) {
        T* r = base ? reinterpret_cast<T*>(base + offset) : nullptr;
        offset += align256(bytes);
        return r;
    }
    size_t bytes() const { return (size_t)(256 + offset); }
};
#define PP_CHECK_WORKSPACE(name, have, need)                                                                      \
    do {                                                                                                          \
        if ((need) > (have)) {                                                                                    \
            pp::set_error(name ": workspace too small (%zu < %zu bytes)", (size_t)(have), (size_t)(need));        \
            return PP_ENOSPACE;                                                                                   \
        }                                                                                                         \
    } while (0)

// Fixed-point masses: a weight is at most 1, so n_per of them times 2^S stay below 2^62 with S = 62 - ceil(log2 n_per).
inline int hist_shift(int n_per) {
    if (n_per < 1) return -1;
    int c = 0;
    while ((int64_t(1) << c) < n_per) ++c;
    return 62 - c;
}
inline double hist_scale(int n_per) { return ldexp(1.0, hist_shift(n_per)); }

// ---- device: the group's maximum -----------------------------------------------------------------------------------------
// The maximum of m over a workgroup of THREADS threads. shmax: THREADS / 64 floats of LDS (synchronised here, once).
template <int THREADS>
__device__ __forceinline__ float block_max(float m, float* shmax) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) shmax[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = shmax[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) r = fmaxf(r, shmax[w]);
    return r;
}

template <int N>
__device__ __forceinline__ float finite_max(const float (&a)[N]) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (isfinite(a[k])) m = fmaxf(m, a[k]);
    return m;
}

// This thread's share of the maximum of the T tile maxima of group g.
template <int THREADS>
__device__ __forceinline__ float tiles_max(const float* __restrict__ tmax, int64_t g, int T) {
    float m = -INFINITY;
    for (int t = threadIdx.x; t < T; t += THREADS) m = fmaxf(m, tmax[g * T + t]);
    return m;
}

// Groups of more than one tile, no statistics given: the maximum of the finite log-weights of the `tile` particles of tile
// blockIdx.x of group g0 + blockIdx.y, to tmax[g T + tile]. 256 threads.
__global__ __launch_bounds__(256) void group_tile_max_kernel(const float* __restrict__ lw, int n_per, int tile, int T, int g0,
                                                             float* __restrict__ tmax) {
    __shared__ float shmax[4];
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const float* l = lw + g * n_per;
    const int64_t lo = (int64_t)blockIdx.x * tile, hi = min((int64_t)n_per, lo + tile);
    float m = -INFINITY;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const float a = l[j];
        if (isfinite(a)) m = fmaxf(m, a);
    }
    m = block_max<256>(m, shmax);
    if (threadIdx.x == 0) tmax[g * T + blockIdx.x] = m;
}

// The maximum of group g in a tile kernel of THREADS threads and T tiles per group: the caller's statistics, else (one tile)
// the maximum over the workgroup's own particles `own`, else the maximum of the tile maxima group_tile_max_kernel left.
template <int THREADS, int N>
__device__ __forceinline__ double group_max(const double* __restrict__ stats, const float* __restrict__ tmax, int64_t g, int T,
                                            const float (&own)[N], float* shmax) {
    if (stats) return stats[6 * g];
    return (double)block_max<THREADS>(T == 1 ? finite_max(own) : tiles_max<THREADS>(tmax, g, T), shmax);
}
// (no finite log-weight in the group: every particle is skipped)
__device__ __forceinline__ bool group_any(double M) { return M > -INFINITY && M < INFINITY; }

// ---- device: a particle's weight -----------------------------------------------------------------------------------------
__device__ __forceinline__ bool particle_counted(float a, bool any) { return any && isfinite(a); }
__device__ __forceinline__ double particle_weight(float a, double M, bool any) {
    return particle_counted(a, any) ? exp((double)a - M) : 0.0;
}
__device__ __forceinline__ double particle_weight_clamped(float a, double M, bool any) { return fmin(particle_weight(a, M, any), 1.0); }
__device__ __forceinline__ unsigned long long fixed_mass(double w, double scale) { return (unsigned long long)llrint(w * scale); }

// ---- device: partial rows ------------------------------------------------------------------------------------------------
// acc + p[first stride] + ... + p[(rows - 1) stride], added in that order with 32 loads in flight.
template <class V>
__device__ __forceinline__ V add_rows(V acc, const V* __restrict__ p, int64_t stride, int first, int rows) {
    int t = first;
    for (; t + 32 <= rows; t += 32) {
        V u[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) u[q] = p[(t + q) * stride];
#pragma unroll
        for (int q = 0; q < 32; ++q) acc += u[q];
    }
    for (; t + 4 <= rows; t += 4) {
        V u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = p[(t + q) * stride];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += u[q];
    }
    for (; t < rows; ++t) acc += p[t * stride];
    return acc;
}

}  // namespace
}  // namespace pp
