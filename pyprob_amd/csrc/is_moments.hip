// Joint weighted moments of up to 16 latent columns of a (batched) lock-step posterior call on the device.
//
// The reference answers every question about a weighted particle set on the host: finalize normalises the weights
// (pyprob/distributions/empirical.py:298-309), expectation sums w f(x) over the values (:451-466) and mean / variance are
// expectations (:668-690); the posterior of another latent of the same particles is posterior.map(...) followed by those. Here
//   pp_is_moments_groups  writes, per group g of n_per particles, the row
//       max lw, W = sum w, sum w^2, count of finite lw | c_j | S_j = sum w (x_j - c_j) | Q_jk = sum w (x_j - c_j)(x_k - c_k), j <= k
//   with the particle's weight w (is_groups.hpp: which particles count and what they weigh) and the pivot c_j = x_j[g, 0] (0 where that is not finite). The host forms
//   mean_j = c_j + S_j / W and cov_jk = Q_jk / W - (S_j / W)(S_k / W): sums about a pivot keep a narrow posterior far from zero
//   accurate where raw second moments cancel.
//
// SHAPE OF THE WORK. The columns are cut into blocks of four; a workgroup takes one tile of TILE particles of one group and one
// PAIR of column blocks (bi <= bj): 16 products, and on a diagonal pair the four S_j and the three weight sums (the combine reads
// the latter from pair 0) - 23 fp64 accumulators per lane; an off-diagonal pair sums and reduces its 16 products alone and stores
// zeros in the other seven slots (all 136 pairs of 16 columns would be 272 VGPRs). The grid runs over (tile, block pair, group); every
// workgroup STORES its partial row in the workspace, and one workgroup per group adds the partial rows in tile order. No atomics,
// no workgroup waits for another: the launches are dependent launches on the caller's stream.
//
// ORDER OF THE SUMS. A lane adds its eight particles (tile offset + 256 k + thread) in the order of k, the 64 lanes of a wave
// meet by lane exchanges of doubles in a fixed pattern (wave_sum_dpp, common.hpp), the four waves in LDS as ((0 + 1) + 2) + 3, the tiles in
// index order. The order is a function of n_per and n_cols alone: group g of an M-group call carries the bits of the one-group
// call on the same particles, and a call repeated gives the same bits. The column values of a skipped particle are read but enter
// no product.
#include "is_groups.hpp"

namespace pp {
namespace {

constexpr int TILE = 2048;                // particles per workgroup: 256 threads x PER_THREAD particles, 256 apart
constexpr int PER_THREAD = 8;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight particles");
constexpr int BLK = 4;                    // columns per block
// A partial row: Q[a][b] at 4 a + b | S[a] at 16 + a | W, sum w^2, count at 20, 21, 22 | the group's maximum at 23 |
// the pivots c[a] of block bi at 24 + a
constexpr int SLOT_S = 16, SLOT_W = 20, SLOT_MAX = 23, SLOT_C = 24, SLOTS = 28, SUMS = 23;

struct MomentCols {
    const float* p[PP_IS_MOMENTS_MAX_COLS];
};

__host__ __device__ inline int blocks_of(int J) { return (J + BLK - 1) / BLK; }
inline int pairs_of(int J) { return blocks_of(J) * (blocks_of(J) + 1) / 2; }
// block pairs (bi <= bj) in row-major order of the upper triangle
__device__ __forceinline__ int pair_index(int B, int bi, int bj) { return bi * B - bi * (bi - 1) / 2 + (bj - bi); }

// Workspace: one partial row per (group, tile, block pair) and one float (tile maximum) per tile.
struct MomentsWorkspace {
    double* partial;
    float* tmax;
    size_t bytes;
};
void moments_carve(int M, int n_per, int J, void* p, MomentsWorkspace& w) {
    Carver c(p);
    const int64_t slots = (int64_t)std::max(M, 0) * tiles_of(std::max(n_per, 1), TILE);
    w.partial = c.take<double>(slots * pairs_of(J) * SLOTS * 8);
    w.tmax = c.take<float>(slots * 4);
    w.bytes = c.bytes();
}

// Step 0 (groups of more than one tile, no statistics given): group_tile_max_kernel.
// Step 1: workgroup (tile blockIdx.x, block pair blockIdx.y, group g0 + blockIdx.z) stores its partial row.
__global__ __launch_bounds__(256) void moments_tile_kernel(const float* __restrict__ lw, MomentCols cols, int J, int n_per, int T,
                                                           int g0, const double* __restrict__ stats,
                                                           const float* __restrict__ tmax, double* __restrict__ partial) {
    __shared__ float shmax[4];
    __shared__ double sh[4][SUMS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.z;
    const int B = blocks_of(J);
    int bi = 0, rem = blockIdx.y;
    while (rem >= B - bi) {
        rem -= B - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int64_t base = g * n_per;
    const float* l = lw + base;
    const int64_t first = (int64_t)blockIdx.x * TILE + tid;
    float a[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) a[k] = first + 256 * k < n_per ? l[first + 256 * k] : -INFINITY;
    const double M = group_max<256>(stats, tmax, g, T, a, shmax);
    const bool any = group_any(M);
    // the columns of the two blocks and their pivots: the group's first value where that is finite, else 0
    const float* pa[BLK];
    const float* pb[BLK];
    double ca[BLK], cb[BLK];
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
        const int ja = BLK * bi + q, jb = BLK * bj + q;
        pa[q] = ja < J ? cols.p[ja] + base : nullptr;
        pb[q] = jb < J ? cols.p[jb] + base : nullptr;
        const float xa = pa[q] ? pa[q][0] : 0.0f, xb = pb[q] ? pb[q][0] : 0.0f;
        ca[q] = isfinite(xa) ? (double)xa : 0.0;
        cb[q] = isfinite(xb) ? (double)xb : 0.0;
    }
    double Q[BLK][BLK], S[BLK], W = 0.0, W2 = 0.0, count = 0.0;
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
        S[q] = 0.0;
#pragma unroll
        for (int r = 0; r < BLK; ++r) Q[q][r] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + 256 * k;
        const bool in = i < n_per;
        float xa[BLK], xb[BLK];
#pragma unroll
        for (int q = 0; q < BLK; ++q) {
            xa[q] = (in && pa[q]) ? pa[q][i] : 0.0f;
            xb[q] = (in && pb[q] && !diag) ? pb[q][i] : 0.0f;
        }
        if (particle_counted(a[k], any)) {      // (a skipped particle's values enter no product: 0 * NaN never reaches a sum)
            const double w = particle_weight(a[k], M, any);
            if (diag) {      // (W, W2, count and S are read from diagonal pairs only: an off-diagonal pair sums its Q alone)
                W += w;
                W2 += w * w;
                count += 1.0;
            }
            double da[BLK], db[BLK];
#pragma unroll
            for (int q = 0; q < BLK; ++q) da[q] = pa[q] ? (double)xa[q] - ca[q] : 0.0;
#pragma unroll
            for (int q = 0; q < BLK; ++q) db[q] = diag ? da[q] : (pb[q] ? (double)xb[q] - cb[q] : 0.0);
#pragma unroll
            for (int q = 0; q < BLK; ++q) {
                const double wd = w * da[q];
                if (diag) S[q] += wd;
#pragma unroll
                for (int r = 0; r < BLK; ++r) Q[q][r] += wd * db[r];
            }
        }
    }
    // the 64 lanes of a wave, then the four waves in order
    double v[SUMS];
#pragma unroll
    for (int q = 0; q < BLK; ++q) {
#pragma unroll
        for (int r = 0; r < BLK; ++r) v[BLK * q + r] = Q[q][r];
        v[SLOT_S + q] = S[q];
    }
    v[SLOT_W] = W;
    v[SLOT_W + 1] = W2;
    v[SLOT_W + 2] = count;
#pragma unroll
    for (int e = 0; e < SUMS; ++e) {
        if (e >= SLOT_S && !diag) {      // (zeros, uniform over the workgroup: nothing to reduce, the row stays defined)
            if (lane == 0) sh[wave][e] = 0.0;
            continue;
        }
        const double s = wave_sum_dpp(v[e]);
        if (lane == 0) sh[wave][e] = s;
    }
    __syncthreads();
    double* row = partial + ((g * T + blockIdx.x) * gridDim.y + blockIdx.y) * SLOTS;
    if (tid < SUMS) row[tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    else if (tid == SLOT_MAX) row[tid] = any ? M : (double)-INFINITY;
    else if (tid < SLOTS) row[tid] = tid == SLOT_C ? ca[0] : tid == SLOT_C + 1 ? ca[1] : tid == SLOT_C + 2 ? ca[2] : ca[3];
}

// Step 2: one workgroup per group; thread e forms entry e of the group's output row from the partial rows, in tile order.
__global__ __launch_bounds__(256) void moments_combine_kernel(const double* __restrict__ partial, int J, int T, int P, int g0,
                                                              double* __restrict__ out) {
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const int width = PP_IS_MOMENTS_WIDTH(J);
    const int B = blocks_of(J);
    const double* rows = partial + g * T * P * SLOTS;
    const int64_t stride = (int64_t)P * SLOTS;
    for (int e = threadIdx.x; e < width; e += 256) {
        int pair = 0, slot;
        bool summed = true;
        if (e == 0) {
            slot = SLOT_MAX;
            summed = false;
        } else if (e < 4) {
            slot = SLOT_W + e - 1;
        } else if (e < 4 + J) {
            const int j = e - 4;
            pair = pair_index(B, j / BLK, j / BLK);
            slot = SLOT_C + j % BLK;
            summed = false;
        } else if (e < 4 + 2 * J) {
            const int j = e - 4 - J;
            pair = pair_index(B, j / BLK, j / BLK);
            slot = SLOT_S + j % BLK;
        } else {
            int j = 0, r = e - 4 - 2 * J;
            while (r >= J - j) {
                r -= J - j;
                ++j;
            }
            const int k = j + r;
            pair = pair_index(B, j / BLK, k / BLK);
            slot = BLK * (j % BLK) + k % BLK;
        }
        const double* p = rows + (int64_t)pair * SLOTS + slot;
        out[g * width + e] = summed ? add_rows(p[0], p, stride, 1, T) : p[0];      // (in tile order)
    }
}

}  // namespace

int is_moments_groups(const float* lw, const float* const* cols, int J, int M, int n_per, const double* stats, double* out, void* ws,
                      size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && cols && out && ws, "pp_is_moments_groups: null pointer (lw, cols, out and the workspace are required)");
    PP_CHECK_ARG(J >= 1 && J <= PP_IS_MOMENTS_MAX_COLS, "pp_is_moments_groups: n_cols in 1 .. %d", PP_IS_MOMENTS_MAX_COLS);
    PP_CHECK_GROUPS("pp_is_moments_groups", M, n_per);
    MomentCols c;
    for (int j = 0; j < PP_IS_MOMENTS_MAX_COLS; ++j) {
        c.p[j] = j < J ? cols[j] : nullptr;
        PP_CHECK_ARG(j >= J || c.p[j], "pp_is_moments_groups: null column pointer %d", j);
    }
    MomentsWorkspace w;
    moments_carve(M, n_per, J, ws, w);
    PP_CHECK_WORKSPACE("pp_is_moments_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(n_per, TILE), P = pairs_of(J);
    for_each_group_chunk(M, [&](int g0, int groups) {
        if (T > 1 && !stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, TILE, T, g0, w.tmax);
        hipLaunchKernelGGL(moments_tile_kernel, dim3(T, P, groups), dim3(256), 0, st, lw, c, J, n_per, T, g0, stats,
                           (const float*)w.tmax, w.partial);
        hipLaunchKernelGGL(moments_combine_kernel, dim3(groups), dim3(256), 0, st, (const double*)w.partial, J, T, P, g0, out);
    });
    PP_LAUNCH_CHECK("pp_is_moments_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_moments_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_cols) {
    if (n_groups < 0 || n_per < 1 || n_cols < 1 || n_cols > PP_IS_MOMENTS_MAX_COLS) return 0;
    pp::MomentsWorkspace w;
    pp::moments_carve(n_groups, n_per, n_cols, nullptr, w);
    return w.bytes;
}

int pp_is_moments_groups(const float* lw, const float* const* cols, int32_t n_cols, int32_t n_groups, int32_t n_per,
                         const double* stats, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_moments_groups(lw, cols, n_cols, n_groups, n_per, stats, out, workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
