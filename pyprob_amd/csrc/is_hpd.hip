// The highest-posterior-density interval and the cdf at a point of a device-backed posterior: two searches over the particles in
// value order with their cumulative weights (pp_is_sort_groups, then pp_is_cdf_groups over the sorted log-weights - what
// pp_is_quantile_groups takes).
//
// The reference has neither: its Empirical answers mean / variance / mode / min / max and a median of 1000 resampled values
// (pyprob/distributions/empirical.py:668-728) and no interval or cdf at all. Here
//   pp_is_hpd_groups    finds, for every group and level L, the shortest window [v_i, v_j] of sorted particles that holds the mass
//                       L T: one thread per start i, the end j_i by binary search for prev_i + fl(L T), the shortest window by a
//                       lexicographic minimum of (width, i) - and
//   pp_is_ecdf_groups   answers P(X <= x) (or <) at points given PER GROUP, one thread per point, by binary search over the values.
//
// WHY THE MINIMUM IS EXACT. A window is a pair of positions; its width is one fp64 subtraction of two fp32 values (exact), NaN
// (inf - inf) made +inf. The minimum of (width, i) under the lexicographic order is associative and commutative, so its value does
// not depend on the shape of the reduction (lanes, waves, tiles): two calls give the same bits, and group g of an M-group call
// equals the one-group call on its slice. An invalid start carries (+inf, INT_MAX): every valid start beats it, and a live group
// has at least one valid start (its first particle of positive weight, since fl(L T) <= T).
//
// WHY THE SEARCH MAY START AT i. j_i = max(i, #{k < c : cdf[k] < t_i}) with t_i = fl(prev_i + m) >= prev_i >= cdf[k] for k < i: every
// k < i is either counted or equal to t_i, and in the second case t_i == prev_i < cdf[i] makes the count over k >= i zero - either way
// i + #{i <= k < c : cdf[k] < t_i} is j_i. t_i <= T = cdf[c - 1] keeps j_i <= c - 1.
//
// No workgroup waits for another and nothing is accumulated with atomics: a group of more than one tile stores one record per
// (level, tile) and a second, dependent launch reduces them.
#include "is_groups.hpp"

#include <limits.h>

namespace pp {
namespace {

constexpr int TILE = PP_IS_HPD_TILE;      // starts per workgroup: 256 threads x PER_THREAD starts, strided by 256
constexpr int PER_THREAD = 8;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight starts");
constexpr int LEVEL_CHUNK = 65535;        // levels ride on grid dimension y

// What a start, a wave, a workgroup or a tile knows: the shortest window so far. In registers a window is three scalars (a struct
// selected by ?: goes through the stack); the struct is the record in memory.
struct Window {
    double width;
    int i, j;
};
__device__ __forceinline__ bool better(double w, int i, double bw, int bi) { return w < bw || (w == bw && i < bi); }
__device__ __forceinline__ void take(double& bw, int& bi, int& bj, double w, int i, int j) {
    const bool t = better(w, i, bw, bi);
    bw = t ? w : bw;
    bi = t ? i : bi;
    bj = t ? j : bj;
}

// The workgroup's best window, valid in thread 0. LDS: 4 widths, 4 starts, 4 ends.
__device__ __forceinline__ void block_best(double& bw, int& bi, int& bj, double* shw, int* shi, int* shj) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(bw, o, 64);
        const int i = __shfl_xor(bi, o, 64);
        const int j = __shfl_xor(bj, o, 64);
        take(bw, bi, bj, w, i, j);
    }
    if ((threadIdx.x & 63) == 0) {
        shw[threadIdx.x >> 6] = bw;
        shi[threadIdx.x >> 6] = bi;
        shj[threadIdx.x >> 6] = bj;
    }
    __syncthreads();
    bw = shw[0];
    bi = shi[0];
    bj = shj[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) take(bw, bi, bj, shw[q], shi[q], shj[q]);
}

__device__ __forceinline__ void write_interval(int bi, int bj, const float* __restrict__ v, double* __restrict__ out,
                                               int* __restrict__ index_out, int64_t slot) {
    const bool live = bi != INT_MAX;
    out[2 * slot] = live ? (double)v[bi] : NAN;
    out[2 * slot + 1] = live ? (double)v[bj] : NAN;
    if (index_out) {
        index_out[2 * slot] = live ? bi : -1;
        index_out[2 * slot + 1] = live ? bj : -1;
    }
}

// Workgroup (tile blockIdx.x, level l0 + blockIdx.y, group g0 + blockIdx.z): the shortest window among the starts of its tile.
// T == 1: the group's answer, written to out / index_out. T > 1: one record to rec[(g n_l + level) T + tile].
__global__ __launch_bounds__(256) void hpd_tile_kernel(const float* __restrict__ value, const double* __restrict__ cdf,
                                                       const int* __restrict__ counted, int n_per, int T, int n_l, int l0, int g0,
                                                       const double* __restrict__ level, double* __restrict__ out,
                                                       int* __restrict__ index_out, Window* __restrict__ rec) {
    __shared__ double shw[4];
    __shared__ int shi[4], shj[4];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.z;
    const int lv = l0 + (int)blockIdx.y;
    const float* v = value + g * n_per;
    const double* cd = cdf + g * n_per;
    const int c = max(0, min(counted[2 * g], n_per));
    const double L = level[lv];
    const double total = c > 0 ? cd[c - 1] : 0.0;
    const bool live = c > 0 && total > 0.0 && total < INFINITY && L > 0.0 && L <= 1.0;      // (a NaN level fails both)
    double bw = INFINITY;
    int bi = INT_MAX, bj = INT_MAX;
    const int64_t first = (int64_t)blockIdx.x * TILE + tid;      // (start k of this thread: first + 256 k)
    if (live && (int64_t)blockIdx.x * TILE < c) {      // (uniform in the workgroup)
        const double m = __dmul_rn(L, total);
        int a[PER_THREAD], b[PER_THREAD];
        double t[PER_THREAD];
        bool ok[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const bool in = first + k * 256 < c;
            const int i = (int)(first + k * 256);
            const double cur = in ? cd[i] : 0.0;
            const double prev = (in && i > 0) ? cd[i - 1] : 0.0;
            t[k] = __dadd_rn(prev, m);
            ok[k] = in && cur > prev && t[k] <= total;
            a[k] = ok[k] ? i : 0;      // the first position in [i, c] with cdf >= t (c: none - excluded by t <= total)
            b[k] = ok[k] ? c : 0;
        }
        // eight independent searches per thread, their loads issued together; every search of the workgroup ends within
        // bit_length(c) rounds
        bool any = true;
        while (any) {
            double x[PER_THREAD];
            int mid[PER_THREAD];
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                mid[k] = a[k] + ((b[k] - a[k]) >> 1);
                x[k] = a[k] < b[k] ? cd[mid[k]] : 0.0;
            }
            any = false;
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                if (a[k] < b[k]) {
                    if (x[k] < t[k]) a[k] = mid[k] + 1;
                    else b[k] = mid[k];
                }
                any = any || a[k] < b[k];
            }
        }
        float vi[PER_THREAD], vj[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            a[k] = min(a[k], c - 1);
            vi[k] = ok[k] ? v[first + k * 256] : 0.0f;
            vj[k] = ok[k] ? v[a[k]] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {      // (ascending i: a tie keeps the earlier start)
            double w = (double)vj[k] - (double)vi[k];
            w = w != w ? INFINITY : w;
            if (ok[k]) take(bw, bi, bj, w, (int)(first + k * 256), a[k]);
        }
    }
    block_best(bw, bi, bj, shw, shi, shj);
    if (tid == 0) {
        const int64_t slot = g * n_l + lv;
        if (T == 1) {
            write_interval(bi, bj, v, out, index_out, slot);
        } else {
            Window* r = rec + slot * T + blockIdx.x;
            r->width = bw;
            r->i = bi;
            r->j = bj;
        }
    }
}

// Groups of more than one tile: workgroup (level l0 + blockIdx.x, group g0 + blockIdx.y) reduces the T records of its slot, each
// thread taking records tid, tid + 256, ... in tile order.
__global__ __launch_bounds__(256) void hpd_reduce_kernel(const float* __restrict__ value, int n_per, int T, int n_l, int l0, int g0,
                                                         const Window* __restrict__ rec, double* __restrict__ out,
                                                         int* __restrict__ index_out) {
    __shared__ double shw[4];
    __shared__ int shi[4], shj[4];
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t slot = g * n_l + l0 + (int)blockIdx.x;
    const Window* r = rec + slot * T;
    double bw = INFINITY;
    int bi = INT_MAX, bj = INT_MAX;
    for (int t = threadIdx.x; t < T; t += 256) take(bw, bi, bj, r[t].width, r[t].i, r[t].j);
    block_best(bw, bi, bj, shw, shi, shj);
    if (threadIdx.x == 0) write_interval(bi, bj, value + g * n_per, out, index_out, slot);
}

// One thread per (group, point).
__global__ __launch_bounds__(256) void ecdf_kernel(const float* __restrict__ value, const double* __restrict__ cdf,
                                                   const int* __restrict__ counted, int n_per, int n_x, int64_t outputs,
                                                   const double* __restrict__ x, int strict, double* __restrict__ out,
                                                   int* __restrict__ rank_out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= outputs) return;
    const int64_t g = o / n_x;
    const int c = max(0, min(counted[2 * g], n_per));
    const double at = x[o];
    double r = NAN;
    int rank = -1;
    if (c > 0 && at == at) {
        const double* cd = cdf + g * n_per;
        const float* v = value + g * n_per;
        const double total = cd[c - 1];
        if (total > 0.0 && total < INFINITY) {
            int a = 0, e = c;      // the first i in [0, c] whose value is > at (strict: >= at); c: none
            while (a < e) {
                const int mid = a + ((e - a) >> 1);
                const double y = (double)v[mid];
                if (strict ? y < at : y <= at) a = mid + 1;
                else e = mid;
            }
            rank = a;
            r = a == 0 ? 0.0 : __ddiv_rn(cd[a - 1], total);
        }
    }
    out[o] = r;
    if (rank_out) rank_out[o] = rank;
}

struct HpdWorkspace {
    Window* rec;
    size_t bytes;
};
void hpd_carve(int M, int n_per, int n_l, void* p, HpdWorkspace& w) {
    Carver c(p);
    const int T = tiles_of(std::max(n_per, 1), TILE);
    const int64_t slots = T > 1 ? (int64_t)std::max(M, 0) * std::max(n_l, 0) * T : 0;
    w.rec = c.take<Window>(slots * (int64_t)sizeof(Window));
    w.bytes = c.bytes();
}
inline bool hpd_shape_ok(int M, int n_per, int n_l) {
    return groups_shape_ok(M, n_per) && n_l >= 0 && (int64_t)M * n_l * 2 <= 0x7fffffff;
}

}  // namespace

int is_hpd_groups(const float* value, const double* cdf, const int* counted, int M, int n_per, const double* level, int n_l,
                  double* out, int* index_out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(value && cdf && counted && level && out && ws,
                 "pp_is_hpd_groups: null pointer (the sorted values, their cdf, the counts, level, out and the workspace are required)");
    PP_CHECK_ARG(n_per >= 1 && M >= 0 && n_l >= 0, "pp_is_hpd_groups: n_per >= 1, n_groups >= 0 and n_l >= 0");
    PP_CHECK_ARG(hpd_shape_ok(M, n_per, n_l), "pp_is_hpd_groups: more than 2^31 - 1 particles or results per call: shard the groups");
    HpdWorkspace w;
    hpd_carve(M, n_per, n_l, ws, w);
    PP_CHECK_WORKSPACE("pp_is_hpd_groups", ws_bytes, w.bytes);
    if (M == 0 || n_l == 0) return 0;
    const int T = tiles_of(n_per, TILE);
    for_each_group_chunk(M, [&](int g0, int groups) {
        for (int l0 = 0; l0 < n_l; l0 += LEVEL_CHUNK) {
            const int levels = std::min(LEVEL_CHUNK, n_l - l0);
            hipLaunchKernelGGL(hpd_tile_kernel, dim3(T, levels, groups), dim3(256), 0, st, value, cdf, counted, n_per, T, n_l, l0, g0,
                               level, out, index_out, w.rec);
            if (T > 1)
                hipLaunchKernelGGL(hpd_reduce_kernel, dim3(levels, groups), dim3(256), 0, st, value, n_per, T, n_l, l0, g0,
                                   (const Window*)w.rec, out, index_out);
        }
    });
    PP_LAUNCH_CHECK("pp_is_hpd_groups");
    return 0;
}

int is_ecdf_groups(const float* value, const double* cdf, const int* counted, int M, int n_per, const double* x, int n_x, int strict,
                   double* out, int* rank_out, hipStream_t st) {
    PP_CHECK_ARG(value && cdf && counted && x && out,
                 "pp_is_ecdf_groups: null pointer (the sorted values, their cdf, the counts, x and out are required)");
    PP_CHECK_ARG(n_per >= 1 && M >= 0 && n_x >= 0, "pp_is_ecdf_groups: n_per >= 1, n_groups >= 0 and n_x >= 0");
    PP_CHECK_ARG(groups_count_ok(M, n_per) && groups_count_ok(M, n_x),
                 "pp_is_ecdf_groups: more than 2^31 - 1 particles or results per call: shard the groups");
    const int64_t outputs = (int64_t)M * n_x;
    if (outputs == 0) return 0;
    hipLaunchKernelGGL(ecdf_kernel, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, st, value, cdf, counted, n_per, n_x, outputs,
                       x, strict, out, rank_out);
    PP_LAUNCH_CHECK("pp_is_ecdf_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_hpd_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_l) {
    if (!pp::hpd_shape_ok(n_groups, n_per, n_l)) return 0;
    pp::HpdWorkspace w;
    pp::hpd_carve(n_groups, n_per, n_l, nullptr, w);
    return w.bytes;
}

int pp_is_hpd_groups(const float* value_sorted, const double* cdf_sorted, const int32_t* counted, int32_t n_groups, int32_t n_per,
                     const double* level, int32_t n_l, double* out, int32_t* index_out, void* workspace, size_t workspace_bytes,
                     void* stream) {
    return pp::is_hpd_groups(value_sorted, cdf_sorted, counted, n_groups, n_per, level, n_l, out, index_out, workspace,
                             workspace_bytes, pp::as_stream(stream));
}

int pp_is_ecdf_groups(const float* value_sorted, const double* cdf_sorted, const int32_t* counted, int32_t n_groups, int32_t n_per,
                      const double* x, int32_t n_x, int32_t strict, double* out, int32_t* rank_out, void* stream) {
    return pp::is_ecdf_groups(value_sorted, cdf_sorted, counted, n_groups, n_per, x, n_x, strict, out, rank_out,
                              pp::as_stream(stream));
}

}  // extern "C"
