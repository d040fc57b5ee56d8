// Weighted Gaussian kernel density of the latents of a (batched) lock-step posterior call on the device: the smooth density at given
// points (1-D) and on a rectangular grid of two latents (2-D). The reference has no counterpart: its Empirical offers plot_histogram
// (pyprob/distributions/empirical.py:889-914) and the 1000-sample density_estimate (:795-807).
//   pp_is_kde_groups    density[g, q] = sum_i wbar_i N(p[g, q]; x_i, h_g^2) over the particles of group g that count (finite log-weight,
//       x not NaN: what pp_is_sort_groups counts), wbar their weights w_i = exp(lw_i - max_g) (is_groups.hpp) over their sum.
//   pp_is_kde2d_groups  density[g, a, b] = sum_i wbar_i N(px[g, a]; x_i, hx_g^2) N(py[g, b]; y_i, hy_g^2): a product kernel on the grid
//       px x py (a particle counts where neither coordinate is NaN).
// Both write log(density) next to it (-inf where the density is 0). The normaliser sum w is taken HERE, over the particles that
// count and from the very fp32 weights the sums use - the statistics row's sum also counts the particles whose value is NaN.
//
// SHAPE OF THE WORK. One workgroup of 256 threads per (group, tile of 2048 particles, chunk of points / quad of grid blocks). It stages
// its tile ONCE into LDS as (x_i, w_i) pairs (2-D: (x_i, y_i, w_i, 0)), w_i rounded to fp32; a skipped particle is staged as value 0,
// weight 0, so that no NaN reaches a sum. It keeps fp64 sums in registers and STORES one partial row per tile; kde_combine_kernel
// adds the rows of a group in tile order, applies 1 / (h sqrt(2 pi) sum w) and writes density and log density. A group of one tile
// is finished by the tile kernel itself (one launch). No atomics, no workgroup waits for another, and a result depends on
// (n_per, Q) and the group's own data only: every sum has a fixed order.
//
// 1-D, ON THE VALU. Lane t of chunk c keeps the P points c 256 P + 256 j + t (j < P) in registers, each as an fp32 pair hi + lo of
// the fp64 point, and walks the tile by LDS broadcast reads: one ds_read_b64 (x_i, w_i) feeds P times
//       d = (hi - x_i) + lo;  t = d s;  k = v_exp_f32(-(t t));  acc = fma(w_i, k, acc)        s = fp32(1 / (h sqrt(2 ln 2)))
// so that exp(-z^2 / 2) = 2^(-(z / sqrt(2 ln 2))^2) costs one transcendental and five plain operations. The exponent comes from
// the DIFFERENCE: hi - x_i is exact for neighbours (Sterbenz) and otherwise rounds relative to itself, so a posterior of width 1e-2
// at 1000 keeps every digit fp32 particles have. (The matrix pipe would need the expanded square (x^2, x, 1) . (1, -2 p, p^2), which
// cancels catastrophically in fp32 once range / h reaches 10^3 - DESIGN.md 4.3.) acc is fp32 over a sub-tile of 256 particles in
// index order and is then added to the lane's fp64 sum. P = 1, 2 or 4: the smallest that covers Q with one chunk, else 4 - the
// point loop is unrolled, P independent chains hide the latency of v_exp_f32; the bits do not depend on P.
//
// 2-D, ON THE MATRIX PIPE. D[a, b] = sum_i (w_i kx(px_a - x_i)) ky(py_b - y_i) is a product with K = the particles whose operands
// are computed, not loaded. A wave owns a 32 x 32 block of the grid (a workgroup four of them); per K-step of
// v_mfma_f32_32x32x2_f32 lane l evaluates ITS element of either fragment - A[row l % 32][k l / 32] = w_i kx, B[k l / 32][column
// l % 32] = ky, i = 2 step + l / 32 - straight into the operand registers: two v_exp_f32 per lane buy 2048 kernel evaluations.
// The particle comes from one ds_read_b128 (two addresses per wave). All operands are >= 0: nothing cancels. The 16 fp32
// accumulators are flushed to fp64 once per tile. Grid sides that are no multiple of 32 are padded with the side's last point; a
// padded row or column is never stored.
//
// ERROR (the bound tests/test_gpu_kde.py holds every case to; u = 2^-24). With a_i = -z_i^2 / 2 the exponent of term i:
//   * d carries two roundings (hi - x_i, + lo), s one, t = d s one, t t one: the argument of v_exp_f32 is off by at most
//     (2 (1 + 1 + 1 + 1) + 1) u = 9 u relative, the term by 9 |a_i| u; lo itself is the fp32 rounding of p - hi, an absolute 2^-48 |p|
//     on d: sqrt(2 |a_i|) (|p| / h) 2^-48 on the term;
//   * v_exp_f32 is good to 1 ulp (2 u), the weight is rounded to fp32 once (u), and the fp32 sum of a sub-tile rounds once per fma
//     (256 u): c2 = 259. 2-D: the same per axis plus the product w kx (u), the product and the accumulation inside the MFMA over
//     the 2048 particles of a tile, taken at 2 u each since the ISA promises no rounding mode there (u + 4096 u): c2 = 4103;
//   * the fp64 flushes, the rows added in tile order, sum w and the scale: (4 n_per + 16) 2^-53;
//   * v_exp_f32 returns 0 below 2^-126 and a weight, a product or a sum below that may be flushed: (4 + 4 n_per) 2^-126 / (h sqrt(2 pi))
//     absolute (2-D: / (2 pi hx hy)).
// Every term is >= 0, so |density - exact| <= sum_i wbar_i k_i expm1((9 |a_i| + c2) u + ...) / (h sqrt(2 pi)) + the last two.
#include "is_groups.hpp"

namespace pp {
namespace {

constexpr int TILE = 2048, THREADS = 256, PER_THREAD = 8, SUB = 256;
constexpr double SQRT_2PI = 2.5066282746310002, TWO_PI = 6.283185307179586;
constexpr double INV_SQRT_2LN2 = 0.8493218002880191;      // exp(-z^2 / 2) = 2^(-(z / sqrt(2 ln 2))^2)
__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Workspace: per (group, tile) one partial row [width] of doubles and the tile's weight sum where a group has more than one tile,
// and one float (the tile's maximum) where the caller gives no statistics.
struct KdeWorkspace {
    double* partial;
    double* wsum;
    float* tmax;
    size_t bytes;
};
void kde_carve(int M, int n_per, int64_t width, void* p, KdeWorkspace& w) {
    Carver c(p);
    const int T = tiles_of(std::max(n_per, 1), TILE);
    const int64_t tiles = (int64_t)std::max(M, 0) * T;
    w.partial = c.take<double>(T > 1 ? tiles * width * 8 : 0);
    w.wsum = c.take<double>(T > 1 ? tiles * 8 : 0);
    w.tmax = c.take<float>(tiles * 4);
    w.bytes = c.bytes();
}
bool kde_shape_ok(int M, int n_per, int64_t width, int64_t max_width) {
    return groups_shape_ok(M, n_per) && width >= 1 && width <= max_width && (int64_t)M * width <= 0x7fffffff;
}

// Stages tile `tile` of group g into LDS - all TILE entries, weight 0 behind the group's end - and returns the sum of the staged
// fp32 weights in fp64, in a fixed order (lane l adds entries l, l + 64, ...; then the wave's fixed tree): every wave computes it.
template <bool TWO_D>
__device__ __forceinline__ double stage_tile(const float* __restrict__ lw, const float* __restrict__ x, const float* __restrict__ y,
                                             int n_per, int T, int64_t g, int tile, const double* __restrict__ stats,
                                             const float* __restrict__ tmax, float* sh, float* shmax) {
    constexpr int W = TWO_D ? 4 : 2;      // floats per staged particle; the weight is the last but one (2-D) / the last (1-D)
    const int tid = threadIdx.x;
    const int64_t base = g * n_per;
    const int64_t first = (int64_t)tile * TILE + tid;
    float a[PER_THREAD], xv[PER_THREAD], yv[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + THREADS * k;
        const bool in = i < n_per;
        a[k] = in ? lw[base + i] : -INFINITY;
        xv[k] = in ? x[base + i] : 0.0f;
        yv[k] = (TWO_D && in) ? y[base + i] : 0.0f;
    }
    const double M = group_max<THREADS>(stats, tmax, g, T, a, shmax);
    const bool any = group_any(M);
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const bool ok = particle_counted(a[k], any) && xv[k] == xv[k] && yv[k] == yv[k];
        float* e = sh + (tid + THREADS * k) * W;
        e[0] = ok ? xv[k] : 0.0f;
        if (TWO_D) {
            e[1] = ok ? yv[k] : 0.0f;
            e[3] = 0.0f;
        }
        e[W == 4 ? 2 : 1] = ok ? (float)particle_weight(a[k], M, any) : 0.0f;
    }
    __syncthreads();
    const int lane = tid & 63;
    double s = 0.0;
#pragma unroll 8
    for (int j = 0; j < TILE / 64; ++j) s += (double)sh[(lane + 64 * j) * W + (W == 4 ? 2 : 1)];
    return wave_sum_dpp(s);
}

__device__ __forceinline__ void split_point(double p, float& hi, float& lo) {
    hi = (float)p;
    lo = (float)(p - (double)hi);
}
// exp(-z^2 / 2) of z = (p - v) / h from the difference: p = hi + lo, s = fp32(1 / (h sqrt(2 ln 2))).
__device__ __forceinline__ float gauss(float hi, float lo, float v, float s) {
    const float t = ((hi - v) + lo) * s;
    return __builtin_amdgcn_exp2f(-(t * t));
}
__device__ __forceinline__ void store_density(double sum, double coef_w, double* __restrict__ dens, double* __restrict__ logd, int64_t at) {
    const double d = sum * (1.0 / coef_w);
    dens[at] = d;
    logd[at] = log(d);
}

// 1-D. Workgroup (tile blockIdx.x, chunk blockIdx.y of 256 P points, group g0 + blockIdx.z).
template <int P>
__global__ __launch_bounds__(THREADS) void kde_tile_kernel(const float* __restrict__ lw, const float* __restrict__ x, int n_per, int T,
                                                           int g0, const double* __restrict__ pts, int64_t sp, int Q,
                                                           const double* __restrict__ h, int64_t sh_, const double* __restrict__ stats,
                                                           const float* __restrict__ tmax, double* __restrict__ partial,
                                                           double* __restrict__ wsum, double* __restrict__ dens,
                                                           double* __restrict__ logd) {
    __shared__ float sh[TILE * 2];
    __shared__ float shmax[THREADS / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.z;
    const double W = stage_tile<false>(lw, x, nullptr, n_per, T, g, tile, stats, tmax, sh, shmax);
    const double hg = h[g * sh_];
    const float s = (float)(INV_SQRT_2LN2 / hg);
    const int q0 = blockIdx.y * THREADS * P + tid;
    float hi[P], lo[P];
    double sum[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int q = q0 + THREADS * j;
        split_point(q < Q ? pts[g * sp + q] : 0.0, hi[j], lo[j]);
        sum[j] = 0.0;
    }
    if (q0 - (tid & 63) < Q) {      // (a wave without a point has nothing to add)
        const int subs = ceil_div(min(TILE, n_per - tile * TILE), SUB);
        const float2* e = reinterpret_cast<const float2*>(sh);
        for (int u = 0; u < subs; ++u) {
            float acc[P];
#pragma unroll
            for (int j = 0; j < P; ++j) acc[j] = 0.0f;
#pragma unroll 8
            for (int i = 0; i < SUB; ++i) {
                const float2 p = e[u * SUB + i];
#pragma unroll
                for (int j = 0; j < P; ++j) acc[j] = __builtin_fmaf(p.y, gauss(hi[j], lo[j], p.x, s), acc[j]);
            }
#pragma unroll
            for (int j = 0; j < P; ++j) sum[j] += (double)acc[j];
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int q = q0 + THREADS * j;
        if (q >= Q) continue;
        if (T == 1)
            store_density(sum[j], SQRT_2PI * hg * W, dens, logd, g * Q + q);
        else
            partial[(g * T + tile) * Q + q] = sum[j];
    }
    if (T > 1 && blockIdx.y == 0 && tid == 0) wsum[g * T + tile] = W;
}

// 2-D. Workgroup (tile blockIdx.x, grid blocks 4 blockIdx.y + wave, group g0 + blockIdx.z); block b covers rows [32 (b / nby), + 32)
// of px and columns [32 (b % nby), + 32) of py.
__global__ __launch_bounds__(THREADS) void kde2d_tile_kernel(const float* __restrict__ lw, const float* __restrict__ x,
                                                             const float* __restrict__ y, int n_per, int T, int g0,
                                                             const double* __restrict__ px, int64_t spx, int Qx,
                                                             const double* __restrict__ py, int64_t spy, int Qy,
                                                             const double* __restrict__ hx, int64_t shx, const double* __restrict__ hy,
                                                             int64_t shy, const double* __restrict__ stats, const float* __restrict__ tmax,
                                                             double* __restrict__ partial, double* __restrict__ wsum,
                                                             double* __restrict__ dens, double* __restrict__ logd) {
    __shared__ float sh[TILE * 4];
    __shared__ float shmax[THREADS / 64];
    const int tid = threadIdx.x, tile = blockIdx.x, lane = tid & 63, c31 = lane & 31, hh = lane >> 5;
    const int64_t g = (int64_t)g0 + blockIdx.z;
    const double W = stage_tile<true>(lw, x, y, n_per, T, g, tile, stats, tmax, sh, shmax);
    const int nby = ceil_div(Qy, 32), blk = blockIdx.y * 4 + (tid >> 6);
    if (blk < ceil_div(Qx, 32) * nby) {
        const int row0 = (blk / nby) * 32, col0 = (blk % nby) * 32;
        const double hxg = hx[g * shx], hyg = hy[g * shy];
        const float sx = (float)(INV_SQRT_2LN2 / hxg), sy = (float)(INV_SQRT_2LN2 / hyg);
        float ahi, alo, bhi, blo;      // (a side that ends inside the block repeats its last point: those rows are not stored)
        split_point(px[g * spx + min(row0 + c31, Qx - 1)], ahi, alo);
        split_point(py[g * spy + min(col0 + c31, Qy - 1)], bhi, blo);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const int steps = ceil_div(min(TILE, n_per - tile * TILE), 2);
        const f32x4* e = reinterpret_cast<const f32x4*>(sh) + hh;
        for (int k = 0; k < steps; ++k) {
            const f32x4 p = e[2 * k];      // (x_i, y_i, w_i, 0) of particle 2 k + lane / 32
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p[2] * gauss(ahi, alo, p[0], sx), gauss(bhi, blo, p[1], sy), acc, 0, 0, 0);
        }
        const int64_t width = (int64_t)Qx * Qy;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = row0 + (r & 3) + 8 * (r >> 2) + 4 * hh, b = col0 + c31;
            if (a >= Qx || b >= Qy) continue;
            if (T == 1)
                store_density((double)acc[r], TWO_PI * hxg * hyg * W, dens, logd, g * width + (int64_t)a * Qy + b);
            else
                partial[(g * T + tile) * width + (int64_t)a * Qy + b] = (double)acc[r];
        }
    }
    if (T > 1 && blockIdx.y == 0 && tid == 0) wsum[g * T + tile] = W;
}

// Groups of more than one tile: thread (blockIdx.x, threadIdx.x) adds entry e of the T partial rows of group g0 + blockIdx.y in tile
// order, and the T weight sums, and scales.
__global__ __launch_bounds__(256) void kde_combine_kernel(const double* __restrict__ partial, const double* __restrict__ wsum, int T,
                                                          int64_t width, int g0, const double* __restrict__ hx, int64_t shx,
                                                          const double* __restrict__ hy, int64_t shy, double* __restrict__ dens,
                                                          double* __restrict__ logd) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= width) return;
    const double sum = add_rows(0.0, partial + g * T * width + e, width, 0, T);
    const double W = add_rows(0.0, wsum + g * T, (int64_t)1, 0, T);
    const double coef = hy ? TWO_PI * hx[g * shx] * hy[g * shy] : SQRT_2PI * hx[g * shx];
    store_density(sum, coef * W, dens, logd, g * width + e);
}

template <int P>
void launch_kde(dim3 grid, hipStream_t st, const float* lw, const float* x, int n_per, int T, int g0, const double* pts, int64_t sp, int Q,
                const double* h, int64_t sh, const double* stats, const KdeWorkspace& w, double* dens, double* logd) {
    hipLaunchKernelGGL(kde_tile_kernel<P>, grid, dim3(THREADS), 0, st, lw, x, n_per, T, g0, pts, sp, Q, h, sh, stats, (const float*)w.tmax,
                       w.partial, w.wsum, dens, logd);
}

}  // namespace

int is_kde_groups(const float* lw, const float* x, int M, int n_per, const double* pts, int Q, int64_t sp, const double* h, int64_t sh,
                  const double* stats, double* dens, double* logd, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && x && pts && h && dens && logd && ws, "pp_is_kde_groups: null pointer (only stats may be null)");
    PP_CHECK_GROUPS("pp_is_kde_groups", M, n_per);
    PP_CHECK_ARG(Q >= 1 && Q <= PP_IS_KDE_MAX_POINTS, "pp_is_kde_groups: 1 <= n_x <= %d", PP_IS_KDE_MAX_POINTS);
    PP_CHECK_ARG((int64_t)M * Q <= 0x7fffffff, "pp_is_kde_groups: more than 2^31 - 1 results per call: shard the groups");
    PP_CHECK_ARG(sp == 0 || sp >= Q, "pp_is_kde_groups: x_stride is 0 (shared) or at least n_x");
    PP_CHECK_ARG(sh == 0 || sh == 1, "pp_is_kde_groups: bandwidth_stride is 0 (shared) or 1");
    KdeWorkspace w;
    kde_carve(M, n_per, Q, ws, w);
    PP_CHECK_WORKSPACE("pp_is_kde_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(n_per, TILE);
    const int P = Q <= THREADS ? 1 : Q <= 2 * THREADS ? 2 : 4;
    for_each_group_chunk(M, [&](int g0, int groups) {
        if (T > 1 && !stats) hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, TILE, T, g0, w.tmax);
        const dim3 grid(T, cdiv(Q, THREADS * P), groups);
        if (P == 1)
            launch_kde<1>(grid, st, lw, x, n_per, T, g0, pts, sp, Q, h, sh, stats, w, dens, logd);
        else if (P == 2)
            launch_kde<2>(grid, st, lw, x, n_per, T, g0, pts, sp, Q, h, sh, stats, w, dens, logd);
        else
            launch_kde<4>(grid, st, lw, x, n_per, T, g0, pts, sp, Q, h, sh, stats, w, dens, logd);
        if (T > 1)
            hipLaunchKernelGGL(kde_combine_kernel, dim3(cdiv(Q, 256), groups), dim3(256), 0, st, (const double*)w.partial,
                               (const double*)w.wsum, T, (int64_t)Q, g0, h, sh, (const double*)nullptr, (int64_t)0, dens, logd);
    });
    PP_LAUNCH_CHECK("pp_is_kde_groups");
    return 0;
}

int is_kde2d_groups(const float* lw, const float* x, const float* y, int M, int n_per, const double* px, int Qx, int64_t spx,
                    const double* py, int Qy, int64_t spy, const double* hx, int64_t shx, const double* hy, int64_t shy,
                    const double* stats, double* dens, double* logd, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && x && y && px && py && hx && hy && dens && logd && ws, "pp_is_kde2d_groups: null pointer (only stats may be null)");
    PP_CHECK_GROUPS("pp_is_kde2d_groups", M, n_per);
    PP_CHECK_ARG(Qx >= 1 && Qx <= PP_IS_KDE2D_MAX_SIDE && Qy >= 1 && Qy <= PP_IS_KDE2D_MAX_SIDE,
                 "pp_is_kde2d_groups: 1 <= n_x, n_y <= %d", PP_IS_KDE2D_MAX_SIDE);
    const int64_t width = (int64_t)Qx * Qy;
    PP_CHECK_ARG((int64_t)M * width <= 0x7fffffff, "pp_is_kde2d_groups: more than 2^31 - 1 results per call: shard the groups");
    PP_CHECK_ARG((spx == 0 || spx >= Qx) && (spy == 0 || spy >= Qy), "pp_is_kde2d_groups: a point stride is 0 (shared) or at least its side");
    PP_CHECK_ARG((shx == 0 || shx == 1) && (shy == 0 || shy == 1), "pp_is_kde2d_groups: a bandwidth stride is 0 (shared) or 1");
    KdeWorkspace w;
    kde_carve(M, n_per, width, ws, w);
    PP_CHECK_WORKSPACE("pp_is_kde2d_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(n_per, TILE);
    const int quads = cdiv(cdiv(Qx, 32) * cdiv(Qy, 32), 4);
    for_each_group_chunk(M, [&](int g0, int groups) {
        if (T > 1 && !stats) hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, TILE, T, g0, w.tmax);
        hipLaunchKernelGGL(kde2d_tile_kernel, dim3(T, quads, groups), dim3(THREADS), 0, st, lw, x, y, n_per, T, g0, px, spx, Qx, py, spy, Qy,
                           hx, shx, hy, shy, stats, (const float*)w.tmax, w.partial, w.wsum, dens, logd);
        if (T > 1)
            hipLaunchKernelGGL(kde_combine_kernel, dim3(cdiv(width, 256), groups), dim3(256), 0, st, (const double*)w.partial,
                               (const double*)w.wsum, T, width, g0, hx, shx, hy, shy, dens, logd);
    });
    PP_LAUNCH_CHECK("pp_is_kde2d_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_kde_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_x) {
    if (!pp::kde_shape_ok(n_groups, n_per, n_x, PP_IS_KDE_MAX_POINTS)) return 0;
    pp::KdeWorkspace w;
    pp::kde_carve(n_groups, n_per, n_x, nullptr, w);
    return w.bytes;
}

int pp_is_kde_groups(const float* lw, const float* x, int32_t n_groups, int32_t n_per, const double* points, int32_t n_x, int64_t x_stride,
                     const double* bandwidth, int64_t bandwidth_stride, const double* stats, double* density, double* log_density,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_kde_groups(lw, x, n_groups, n_per, points, n_x, x_stride, bandwidth, bandwidth_stride, stats, density, log_density,
                             workspace, workspace_bytes, pp::as_stream(stream));
}

size_t pp_is_kde2d_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_x, int32_t n_y) {
    if (n_x < 1 || n_y < 1 || n_x > PP_IS_KDE2D_MAX_SIDE || n_y > PP_IS_KDE2D_MAX_SIDE) return 0;
    if (!pp::kde_shape_ok(n_groups, n_per, (int64_t)n_x * n_y, (int64_t)PP_IS_KDE2D_MAX_SIDE * PP_IS_KDE2D_MAX_SIDE)) return 0;
    pp::KdeWorkspace w;
    pp::kde_carve(n_groups, n_per, (int64_t)n_x * n_y, nullptr, w);
    return w.bytes;
}

int pp_is_kde2d_groups(const float* lw, const float* x, const float* y, int32_t n_groups, int32_t n_per, const double* points_x, int32_t n_x,
                       int64_t x_stride, const double* points_y, int32_t n_y, int64_t y_stride, const double* bandwidth_x,
                       int64_t bandwidth_x_stride, const double* bandwidth_y, int64_t bandwidth_y_stride, const double* stats,
                       double* density, double* log_density, void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_kde2d_groups(lw, x, y, n_groups, n_per, points_x, n_x, x_stride, points_y, n_y, y_stride, bandwidth_x, bandwidth_x_stride,
                               bandwidth_y, bandwidth_y_stride, stats, density, log_density, workspace, workspace_bytes,
                               pp::as_stream(stream));
}

}  // extern "C"
