// Pair sums between the JOINT particles of two lock-step posteriors on the device: what the Gaussian-kernel MMD^2 and the
// multivariate energy distance are made of (Empirical.compare_joint). The reference has no distance between two Empiricals.
//   pp_is_pairs_groups  per group g, with z = (x - center_g) inv_scale_g the standardised coordinates of the counted particles of
//       side a (weights w, normalised) and side b (weights v), k(z, z') = exp(-|z - z'|^2 / (2 h_g^2)):
//       out[g] = { k_aa = sum_ij w_i w_j k, k_bb, k_ab = sum_ij w_i v_j k, d_aa = sum_ij w_i w_j |z_i - z_j|, d_bb, d_ab,
//                  sum w^2, sum v^2, count_a, count_b }.
// A particle counts where its log-weight is finite (is_groups.hpp) and its J standardised coordinates are finite with |z_j| alpha <
// 2^30 (a NaN coordinate drops it: kde2d's rule; beyond that limit fp32 exponents would overflow to inf - inf). The weights are
// exp(lw - max) in fp64; the normalisers W = sum w are taken HERE, over the counted particles, and divide the sums at the very end.
//
// THREE PASSES, dependent launches on the caller's stream, no atomics, no workgroup waits for another.
// 1. OPERANDS (pairs_operand_kernel, one launch per side, a workgroup per 2048 particles). Per particle, z_j = fp32(((double)x_j -
//    c_j) inv_s_j) - the subtraction in fp64, so a posterior of width 1e-2 at 1000 keeps its digits - and two images in the workspace:
//      Gaussian image, feature-major [K][n_pad], K = J + 2 rounded up to even:  (fp32(alpha z_1) .. fp32(alpha z_J), 0.., q, 1)
//          alpha = sqrt(log2 e) / h,  q = fp32(log2(e) (lw - max) - alpha^2 |z|^2 / 2)  (fp64 arithmetic on the fp32 z, ONE rounding)
//      distance image, particle-major [n_pad][DS], DS = J + 1 rounded up to 4:   (z_1 .. z_J, fp32(w))
//    and per tile sum w, sum w^2 and the count, in fp64. The inner product of the image of i, read as a ROW (.., q, 1), and the image
//    of j, read as a COLUMN (.., 1, q: the last two features swap on load), is log2 of w_i w_j k(z_i, z_j): nothing is left to
//    multiply. A particle that does not count, and the padding behind n_per, has zero coordinates, q = -inf and w = 0: its terms
//    are exactly 0 (2^-inf; the padding features are 0 on BOTH sides, so no 0 inf occurs).
// 2. PAIR SUMS, two kernels over one tiling. A workgroup of four waves owns 128 rows of one of the three products of a group (aa, bb,
//    ab) and one strip of columns: the column chunks (256 columns) of a product are cut into at most 16 strips of equal length.
//    aa and bb visit only what lies on or above the diagonal and count what lies above it twice.
//      pairs_gauss_kernel<K / 2>, ON THE MATRIX PIPE. A wave owns 32 rows: its K / 2 A-fragments of v_mfma_f32_32x32x2_f32 stay in
//        registers for the whole strip. A chunk of the column image (256 x K floats, <= 10 KB) goes global -> registers (issued one
//        chunk ahead) -> LDS; per 32 x 32 block of exponents a wave issues K / 2 ds_read_b32 + K / 2 MFMAs, 16 v_exp_f32 and a tree of
//        15 additions, doubles the block's sum above the diagonal (exact) and adds it to an fp32 chunk sum, which is flushed to the
//        lane's fp64 sum every chunk: an fp32 sum never holds more than 16 x 8 = 128 terms.
//      pairs_dist_kernel<J>, ON THE VALU. Thread t owns ROW t % 128 (its z and w in registers) and walks the half t / 128 of every
//        chunk; the column (z', v) is wave-uniform, so it is read from the distance image by scalar loads into SGPRs - no LDS, no
//        staging. d = v_sqrt_f32(sum_j (z_j - z'_j)^2) from the DIFFERENCE (the expanded square is wrong at coincident pairs), acc =
//        fma(v_j, d, acc) in fp32 over the 128 columns of a half chunk, then sum += (double)acc in fp64; the row weight is applied
//        once, in fp64, at the end. A half chunk that sits on the diagonal counts the pairs with column > row (d = 0 on the diagonal).
//    Every workgroup adds its lanes by DPP, its waves in wave order and STORES one double per (kind, product, row block, strip).
// 3. COMBINE (pairs_combine_kernel, one workgroup per group): thread t adds the partials t, t + 256, .. of a sum in that order, then
//    lanes and waves as above; the tile sums of the weights likewise; ten doubles are written.
// The order of every sum is a function of (n_per_a, n_per_b, J) alone: two calls give the same bits, and group g of an M-group call
// gives the bits of the one-group call on its slices.
//
// RESOURCES (gfx950, hipcc -O3; the build fails if a pair kernel or the operand kernel uses scratch): pairs_gauss_kernel<5> (J = 7, 8)
// 40 VGPRs + 16 AGPRs, 10.3 KB LDS; pairs_dist_kernel<8> 37 VGPRs, 32 B LDS; pairs_operand_kernel<8> 92 VGPRs; no scratch anywhere.
//
// ERROR (what tests/test_gpu_pairs.py holds every sum to; u = 2^-24, all terms are >= 0 so the bounds add up term by term).
// Gaussian sums. With P = alpha^2 sum_j |z_j z'_j|, N = alpha^2 |z|^2, N' = alpha^2 |z'|^2, L = log2(e) |lw - max| (L' likewise) and
// S = P + N + N' + L + L' the base-2 exponent E of a pair is off by
//   * the fp32 rounding of z and z' (the restatement keeps them in fp64): dE = alpha^2 (z - z').dz, at most (N + N' + 2 P) u;
//   * fp32(alpha z), one rounding per operand: 2 P u; q and q', one rounding each: (N / 2 + L + N' / 2 + L') u;
//   * the K products and K additions inside the MFMA, taken at 2 u each on partial sums of at most S since the ISA promises no
//     rounding mode there: (2 + 2 K) S u;
//   in all at most (2 K + 9) S u, so the term is off by expm1(ln 2 (2 K + 9) S u) relative; then
//   * v_exp_f32, 1 ulp: 2 u; the fp32 sums of at most 128 terms (tree, doubling, chunk sum): 128 u: c2 = 130;
//   * the fp64 sums (lanes, waves, partials, normalisers): (n_a + n_b + 64) 2^-53 relative;
//   * v_exp_f32 returns 0 below 2^-126: n_r n_c 2^-126 / (W_r W_c) absolute.
// Distance sums. The fp32 rounding of z and z' moves d by at most u (|z| + |z'|) ABSOLUTE (triangle inequality); from the fp32 z
// on, each difference and each square rounds once (3 u on a term of d^2), the J - 1 additions once each, the square root halves
// that and v_sqrt_f32 adds 1 ulp: (J / 2 + 3) u relative; fp32(v_j) and fp32(w_i): 2 u; the fp32 sum of 128 fma: 128 u:
//   |d_sum - exact| <= sum_ij w_i v_j (d_ij (J / 2 + 133) u + (|z_i| + |z'_j|) u) + (n_a + n_b + 64) 2^-53 d_sum
// (v_sqrt_f32 flushes an argument below 2^-126: 2^-63 absolute on d, far below the second term).
#include "is_pair_image.hpp"      // (pass 1, the images and their constants: shared with is_kde_joint.hip)

namespace pp {
namespace {

constexpr int ROWS = 128, HALF = 128, MAX_STRIPS = 16;
constexpr int GROUPS_PER_LAUNCH = 65535 / 3;       // (three products per group ride on grid dimension z)
static_assert(HALF == ROWS && 2 * HALF == CHUNK, "tiling");

// The three products of a group: 0 = aa, 1 = bb, 2 = ab. Rows, columns, row blocks, column chunks, chunks per strip, strips.
struct Shape {
    int n_r, n_c, RB, chunks, per_strip, S;
};
__host__ __device__ inline Shape shape_of(int prod, int na, int nb) {
    Shape s;
    s.n_r = prod == 1 ? nb : na;
    s.n_c = prod == 0 ? na : nb;
    s.RB = ceil_div(s.n_r, ROWS);
    s.chunks = ceil_div(s.n_c, CHUNK);
    s.per_strip = ceil_div(s.chunks, MAX_STRIPS);
    s.S = ceil_div(s.chunks, s.per_strip);
    return s;
}
// partial[(((g 2 + kind) 3 + prod) RBmax + rb) MAX_STRIPS + strip], kind 0 = Gaussian, 1 = distance
__host__ __device__ inline int64_t partial_at(int64_t g, int kind, int prod, int RBmax, int rb, int strip) {
    return ((((g * 2 + kind) * 3 + prod) * RBmax + rb) * MAX_STRIPS) + strip;
}

// Workspace, per side: the two images, per operand tile (sum w, sum w^2, count) and one float (the tile's maximum, read where the
// caller gives no statistics); then the partial sums.
struct PairsWorkspace {
    float* img[2];
    float* dimg[2];
    double* wsum[2];
    float* tmax[2];
    double* partial;
    size_t bytes;
};
void pairs_carve(int M, int na, int nb, int J, void* p, PairsWorkspace& w) {
    Carver c(p);
    const int64_t m = std::max(M, 0);
    const int n[2] = {std::max(na, 1), std::max(nb, 1)};
    for (int s = 0; s < 2; ++s) {
        const int64_t tiles = m * tiles_of(n[s], OP_TILE);
        w.img[s] = c.take<float>(m * image_k(J) * pad_of(n[s]) * 4);
        w.dimg[s] = c.take<float>(m * dist_stride(J) * pad_of(n[s]) * 4);
        w.wsum[s] = c.take<double>(tiles * 3 * 8);
        w.tmax[s] = c.take<float>(tiles * 4);
    }
    w.partial = c.take<double>(m * 6 * ceil_div(std::max(n[0], n[1]), ROWS) * MAX_STRIPS * 8);
    w.bytes = c.bytes();
}
bool pairs_shape_ok(int M, int na, int nb, int J) {
    return J >= 1 && J <= MAXJ && groups_shape_ok(M, na) && groups_shape_ok(M, nb);
}

// ---- 2. pair sums ---------------------------------------------------------------------------------------------------------------
// What a pair workgroup (row block blockIdx.x, strip blockIdx.y, product blockIdx.z % 3 of group g0 + blockIdx.z / 3) works on.
struct PairJob {
    int prod, rb, c_lo, c_hi;      // column chunks [c_lo, c_hi); empty where the strip lies below the diagonal
    int64_t g, pad_r, pad_c;
    bool sym, live;
};
__device__ __forceinline__ PairJob pair_job(int na, int nb, int g0) {
    PairJob j;
    j.prod = blockIdx.z % 3;
    j.g = (int64_t)g0 + blockIdx.z / 3;
    const Shape s = shape_of(j.prod, na, nb);
    j.rb = blockIdx.x;
    j.live = j.rb < s.RB && (int)blockIdx.y < s.S;
    j.sym = j.prod != 2;
    j.c_lo = blockIdx.y * s.per_strip;
    j.c_hi = min(s.chunks, j.c_lo + s.per_strip);
    if (j.sym) j.c_lo = max(j.c_lo, j.rb * ROWS / CHUNK);      // (the chunks before this one lie below the diagonal)
    j.pad_r = pad_of(s.n_r);
    j.pad_c = pad_of(s.n_c);
    return j;
}

template <int K2>
__global__ __launch_bounds__(THREADS) void pairs_gauss_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b, int na,
                                                              int nb, int g0, int RBmax, double* __restrict__ partial) {
    constexpr int K = 2 * K2;
    __shared__ float sh[K * CHUNK];
    __shared__ double shsum[THREADS / 64];
    const PairJob job = pair_job(na, nb, g0);
    if (!job.live) return;
    const int tid = threadIdx.x, lane = tid & 63, c31 = lane & 31, hh = lane >> 5;
    const float* R = (job.prod == 1 ? img_b : img_a) + job.g * K * job.pad_r;
    const float* C = (job.prod == 0 ? img_a : img_b) + job.g * K * job.pad_c;
    const int rt = job.rb * (ROWS / 32) + (tid >> 6);      // this wave's rows [32 rt, + 32)
    float ar[K2];
#pragma unroll
    for (int s = 0; s < K2; ++s) ar[s] = R[(2 * s + hh) * job.pad_r + 32 * rt + c31];
    // thread t stages column t of a chunk, as a COLUMN image: the features K - 2 (q) and K - 1 (1) change places
    float nx[K];
    auto load = [&](int c) {
#pragma unroll
        for (int f = 0; f < K; ++f) nx[f] = C[(f == K - 2 ? K - 1 : f == K - 1 ? K - 2 : f) * job.pad_c + (int64_t)c * CHUNK + tid];
    };
    double sum = 0.0;
    if (job.c_lo < job.c_hi) load(job.c_lo);
    for (int c = job.c_lo; c < job.c_hi; ++c) {
        __syncthreads();
#pragma unroll
        for (int f = 0; f < K; ++f) sh[f * CHUNK + tid] = nx[f];
        __syncthreads();
        if (c + 1 < job.c_hi) load(c + 1);
        float sub = 0.0f;
        for (int ti = 0; ti < CHUNK / 32; ++ti) {
            const int ct = c * (CHUNK / 32) + ti;
            if (job.sym && ct < rt) continue;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < K2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[s], sh[(2 * s + hh) * CHUNK + 32 * ti + c31], acc, 0, 0, 0);
            float e[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_exp2f(acc[r]);
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int r = 0; r < w; ++r) e[r] += e[r + w];
            sub += (job.sym && ct > rt) ? 2.0f * e[0] : e[0];
        }
        sum += (double)sub;
    }
    sum = block_sum(sum, shsum);
    if (tid == 0) partial[partial_at(job.g, 0, job.prod, RBmax, job.rb, blockIdx.y)] = sum;
}

// acc over the HALF columns from col0 on; ABOVE: only the pairs with column > row count.
template <int J, bool ABOVE>
__device__ __forceinline__ float dist_half_chunk(const float* __restrict__ C, int col0, int row, const float (&z)[J]) {
    constexpr int DS = dist_stride(J);
    float acc = 0.0f;
#pragma unroll 4
    for (int i = 0; i < HALF; ++i) {
        const float* p = C + (int64_t)(col0 + i) * DS;      // (wave-uniform: scalar loads)
        float d2 = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float t = z[j] - p[j];
            d2 = __builtin_fmaf(t, t, d2);
        }
        float d = __builtin_amdgcn_sqrtf(d2);
        if (ABOVE) d = col0 + i > row ? d : 0.0f;
        acc = __builtin_fmaf(p[J], d, acc);
    }
    return acc;
}

template <int J>
__global__ __launch_bounds__(THREADS) void pairs_dist_kernel(const float* __restrict__ dimg_a, const float* __restrict__ dimg_b, int na,
                                                             int nb, int g0, int RBmax, double* __restrict__ partial) {
    constexpr int DS = dist_stride(J);
    __shared__ double shsum[THREADS / 64];
    const PairJob job = pair_job(na, nb, g0);
    if (!job.live) return;
    const int tid = threadIdx.x, row = job.rb * ROWS + (tid & (ROWS - 1));
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);
    const float* R = (job.prod == 1 ? dimg_b : dimg_a) + job.g * DS * job.pad_r + (int64_t)row * DS;
    const float* C = (job.prod == 0 ? dimg_a : dimg_b) + job.g * DS * job.pad_c;
    float z[J];
#pragma unroll
    for (int j = 0; j < J; ++j) z[j] = R[j];
    const float w = R[J];
    double sum = 0.0;
    for (int c = job.c_lo; c < job.c_hi; ++c) {
        const int col0 = c * CHUNK + HALF * half;      // (a half chunk and a row block are both 128 wide and aligned)
        if (!job.sym)
            sum += (double)dist_half_chunk<J, false>(C, col0, row, z);
        else if (col0 > job.rb * ROWS)
            sum += 2.0 * (double)dist_half_chunk<J, false>(C, col0, row, z);
        else if (col0 == job.rb * ROWS)
            sum += 2.0 * (double)dist_half_chunk<J, true>(C, col0, row, z);
    }
    sum = block_sum(sum * (double)w, shsum);
    if (tid == 0) partial[partial_at(job.g, 1, job.prod, RBmax, job.rb, blockIdx.y)] = sum;
}

// ---- 3. combine -----------------------------------------------------------------------------------------------------------------
// One workgroup per group g0 + blockIdx.x.
__global__ __launch_bounds__(THREADS) void pairs_combine_kernel(const double* __restrict__ partial, const double* __restrict__ wsum_a,
                                                                const double* __restrict__ wsum_b, int na, int nb, int g0, int RBmax,
                                                                double* __restrict__ out) {
    __shared__ double shsum[THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    double side[2][3];      // W, sum w^2, count
    for (int s = 0; s < 2; ++s) {
        const int T = ceil_div(s ? nb : na, OP_TILE);
        const double* p = (s ? wsum_b : wsum_a) + g * T * 3;
        for (int q = 0; q < 3; ++q) {
            double v = 0.0;
            for (int t = tid; t < T; t += THREADS) v += p[t * 3 + q];
            side[s][q] = block_sum(v, shsum);
        }
    }
    double sums[2][3];
    for (int kind = 0; kind < 2; ++kind)
        for (int prod = 0; prod < 3; ++prod) {
            const Shape s = shape_of(prod, na, nb);
            const double* p = partial + partial_at(g, kind, prod, RBmax, 0, 0);
            double v = 0.0;
            for (int e = tid; e < s.RB * s.S; e += THREADS) v += p[(int64_t)(e / s.S) * MAX_STRIPS + e % s.S];
            sums[kind][prod] = block_sum(v, shsum);
        }
    if (tid != 0) return;
    const double Wa = side[0][0], Wb = side[1][0];
    double* o = out + g * PP_IS_PAIRS_WIDTH;
    for (int kind = 0; kind < 2; ++kind) {
        o[3 * kind + 0] = sums[kind][0] / (Wa * Wa);
        o[3 * kind + 1] = sums[kind][1] / (Wb * Wb);
        o[3 * kind + 2] = sums[kind][2] / (Wa * Wb);
    }
    o[6] = side[0][1] / (Wa * Wa);
    o[7] = side[1][1] / (Wb * Wb);
    o[8] = side[0][2];
    o[9] = side[1][2];
}

struct PairSide {
    const float* lw;
    PairCols cols;
    const double* stats;
    int n_per;
};

template <int J>
void launch_pairs(hipStream_t st, const PairSide (&side)[2], int g0, int groups, const double* center, const double* inv_scale,
                  const double* h, int64_t sh, const PairsWorkspace& w, double* out) {
    const int na = side[0].n_per, nb = side[1].n_per, RBmax = ceil_div(std::max(na, nb), ROWS);
    for (int s = 0; s < 2; ++s) {
        const int T = tiles_of(side[s].n_per, OP_TILE);
        if (T > 1 && !side[s].stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, side[s].lw, side[s].n_per, OP_TILE, T, g0, w.tmax[s]);
        hipLaunchKernelGGL((pairs_operand_kernel<J, true>), dim3(T, groups), dim3(THREADS), 0, st, side[s].lw, side[s].cols, side[s].n_per, T, g0,
                           center, inv_scale, h, sh, side[s].stats, (const float*)w.tmax[s], w.img[s], w.dimg[s], w.wsum[s]);
    }
    int S = 0;
    for (int prod = 0; prod < 3; ++prod) S = std::max(S, shape_of(prod, na, nb).S);
    const dim3 grid(RBmax, S, 3 * groups);
    hipLaunchKernelGGL(pairs_gauss_kernel<image_k(J) / 2>, grid, dim3(THREADS), 0, st, (const float*)w.img[0], (const float*)w.img[1], na, nb,
                       g0, RBmax, w.partial);
    hipLaunchKernelGGL(pairs_dist_kernel<J>, grid, dim3(THREADS), 0, st, (const float*)w.dimg[0], (const float*)w.dimg[1], na, nb, g0, RBmax,
                       w.partial);
    hipLaunchKernelGGL(pairs_combine_kernel, dim3(groups), dim3(THREADS), 0, st, (const double*)w.partial, (const double*)w.wsum[0],
                       (const double*)w.wsum[1], na, nb, g0, RBmax, out);
}

}  // namespace

int is_pairs_groups(const float* lw_a, const float* const* cols_a, const double* stats_a, int na, const float* lw_b,
                    const float* const* cols_b, const double* stats_b, int nb, int J, int M, const double* center, const double* inv_scale,
                    const double* h, int64_t sh, double* out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw_a && cols_a && lw_b && cols_b && center && inv_scale && h && out && ws,
                 "pp_is_pairs_groups: null pointer (only stats_a and stats_b may be null)");
    PP_CHECK_ARG(J >= 1 && J <= MAXJ, "pp_is_pairs_groups: n_cols in 1 .. %d", MAXJ);
    PP_CHECK_GROUPS("pp_is_pairs_groups", M, na);
    PP_CHECK_GROUPS("pp_is_pairs_groups", M, nb);
    PP_CHECK_ARG(sh == 0 || sh == 1, "pp_is_pairs_groups: bandwidth_stride is 0 (shared) or 1");
    PairSide side[2] = {{lw_a, {}, stats_a, na}, {lw_b, {}, stats_b, nb}};
    for (int j = 0; j < MAXJ; ++j) {
        side[0].cols.p[j] = j < J ? cols_a[j] : nullptr;
        side[1].cols.p[j] = j < J ? cols_b[j] : nullptr;
        PP_CHECK_ARG(j >= J || (cols_a[j] && cols_b[j]), "pp_is_pairs_groups: null column pointer %d", j);
    }
    PairsWorkspace w;
    pairs_carve(M, na, nb, J, ws, w);
    PP_CHECK_WORKSPACE("pp_is_pairs_groups", ws_bytes, w.bytes);
    for (int g0 = 0; g0 < M; g0 += GROUPS_PER_LAUNCH) {
        const int groups = std::min(GROUPS_PER_LAUNCH, M - g0);
        switch (J) {
            case 1: launch_pairs<1>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            case 2: launch_pairs<2>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            case 3: launch_pairs<3>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            case 4: launch_pairs<4>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            case 5: launch_pairs<5>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            case 6: launch_pairs<6>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            case 7: launch_pairs<7>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
            default: launch_pairs<8>(st, side, g0, groups, center, inv_scale, h, sh, w, out); break;
        }
    }
    PP_LAUNCH_CHECK("pp_is_pairs_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_pairs_workspace_bytes(int32_t n_groups, int32_t n_per_a, int32_t n_per_b, int32_t n_cols) {
    if (!pp::pairs_shape_ok(n_groups, n_per_a, n_per_b, n_cols)) return 0;
    pp::PairsWorkspace w;
    pp::pairs_carve(n_groups, n_per_a, n_per_b, n_cols, nullptr, w);
    return w.bytes;
}

int pp_is_pairs_groups(const float* lw_a, const float* const* cols_a, const double* stats_a, int32_t n_per_a, const float* lw_b,
                       const float* const* cols_b, const double* stats_b, int32_t n_per_b, int32_t n_cols, int32_t n_groups,
                       const double* center, const double* inv_scale, const double* bandwidth, int64_t bandwidth_stride, double* out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_pairs_groups(lw_a, cols_a, stats_a, n_per_a, lw_b, cols_b, stats_b, n_per_b, n_cols, n_groups, center, inv_scale,
                               bandwidth, bandwidth_stride, out, workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
