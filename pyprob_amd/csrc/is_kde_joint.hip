// The product-Gaussian kernel density of the JOINT particles of a lock-step posterior at query points, and the mean-shift map that
// climbs it (Empirical.kde_joint, Empirical.modes). The reference has neither.
//   pp_is_kde_joint_groups   per group g and query q, z = (x - center_g) inv_scale_g standardised, w the normalised weights of the
//       counted particles (the rule of is_pairs.hip), h = h_g:
//         log_density[g, q] = log sum_i w_i N_J(z_q; z_i, h^2 I)
//         mean[g, q, :]     = sum_i w_i k_qi z_i / sum_i w_i k_qi,   k_qi = exp(-|z_q - z_i|^2 / (2 h^2))      (where asked for)
//   pp_is_meanshift_groups   x <- mean(x) from seeds in standardised coordinates until every seed's step is below tol h.
// Both are a softmax over the particles of E_qi = log2(w_i k_qi): the normaliser is the density, the weighted mean of the particles
// the mean-shift step - two chained matrix products with an exp2 between them and a running maximum.
//
// PASSES, dependent launches on the caller's stream, no atomics, no workgroup waits for another.
// 1. OPERANDS (is_pair_image.hpp, the pass of is_pairs.hip without its distance image): per particle (alpha z, 0.., q, 1), feature-major
//    [K][n_pad], alpha = sqrt(log2 e) / h, and per 2048 particles sum w and the count in fp64.
// 2. MAIN (kdej_main_kernel<K / 2, MEAN>). A workgroup of four waves owns QTILE = 128 queries (a wave 32: its K / 2 B-fragments of the
//    query image (alpha z_q, 0.., 1, q_q), q_q = -alpha^2 |z_q|^2 / 2, stay in registers) and ONE strip of the particles, staged through
//    LDS in chunks of 256 (global -> registers one chunk ahead -> LDS, row stride 260 floats). Per 32-particle block a wave
//      a. takes the 32 x 32 exponents from K / 2 v_mfma_f32_32x32x2_f32, particles as ROWS and queries as COLUMNS: a lane holds the
//         16 particles 8 (r / 4) + 4 (lane / 32) + r % 4 of ONE query, lane % 32;
//      b. raises the running reference m of its query: the per-lane maximum of the 16, one exchange with the partner half-wave, and m =
//         max(m, ceil(.)). m is an INTEGER, so rescaling what was summed under the old m is v_ldexp_f32 - exact - and happens only in
//         the blocks where some lane's m rose (a wave-uniform branch; the bits do not depend on it: 2^0 = 1);
//      c. p_r = v_exp_f32(E_r - m) in (0, 1], a tree of 15 additions into the lane's fp32 sum;
//      d. MEAN: mean-sum += P Z on the matrix pipe with the p_r as B operands STRAIGHT FROM THE ACCUMULATOR REGISTERS: in the MFMA of
//         register r the k index is the pair of particles that the two half-waves hold in p_r, the A operand row j is alpha z_j of
//         those two particles, read from the staged chunk (one ds_read_b128 per four r). 16 MFMAs per block; rows 0 .. J - 1 of the
//         result are the sums (lane: features 4 (lane / 32) + r, r < 4, of query lane % 32), the other 24 rows are not used.
//    Every chunk the fp32 sums (at most 128 terms in a lane's density sum, 256 products in a mean sum) are flushed to fp64 under the same
//    integer reference. The strip stores (m, sum, mean-sum[J]) per query: partial[g][strip][slot][Q_pad].
//    The number of strips is a function of (n_per, Q) alone (kdej_split): about 1024 workgroups per group where the particles allow it,
//    at most 128 strips, so a mean-shift call with a few hundred seeds still fills the chip.
// 3. COMBINE (kdej_combine_kernel, a thread per query): the strips in strip order under the largest m - ldexp again, exact - then
//    log_density = ln 2 m + log(sum) - log(W) - J log(h sqrt(2 pi)) and mean = mean-sum / (alpha sum). Mean shift instead moves the
//    open seeds in place (kdej_shift_kernel), freezes those whose step fell below tol h, and every check_every iterations one
//    workgroup folds the seeds' states into the word the host reads (pp_is_gmm_groups' scheme: a frozen seed never moves again, so the
//    result does not depend on check_every); one MAIN pass without the second product then gives the final points' log-densities.
// The order of every sum is a function of (n_per, Q, J) alone: two calls give the same bits, and group g of an M-group call gives
// the bits of the one-group call on its slices.
//
// FAR QUERIES. m follows the largest exponent wherever it lies, so a query whose every k_qi underflows fp32 (40 h away: 2^-1154) still
// has its largest term in (1/2, 1] and a finite log-density and mean. This holds while the products of the exponent stay in fp32
// range (|alpha z| < 2^30 by the counting rule; a query with |alpha z_q| beyond about 2^60 / max |alpha z_i|, or a non-finite
// coordinate): beyond it the exponent is -inf or NaN, log_density is -inf or NaN and the mean NaN. A group without a counted particle
// gives NaN rows and count 0.
//
// WHICH PIPE BOUNDS IT. Per 32 x 32 block a wave issues K / 2 + 16 MFMAs of 16 passes (64 cycles each: 1344 cycles at J = 8) against
// 17 v_exp_f32 (quarter rate, 16 cycles each: 272 cycles) and about 70 other VALU operations: with the mean the kernel is bound by the
// matrix pipe, by the second product, three quarters of whose rows are padding. v_mfma_f32_16x16x4_f32 would halve that waste (16 rows)
// but its accumulator holds 4 particles of a query over 4 lanes: the maximum then costs two exchanges and a v_exp_f32 of the
// rescale per 4 exponents instead of per 16. The VALU (16 x J fma per lane and block with the coordinates broadcast from LDS) costs
// 512 cycles at J = 8 plus 32 broadcast ds_read_b128, on the pipe that already carries the exponentials. Without the mean (kde_joint)
// K / 2 MFMAs (320 cycles) stand against the same VALU work: v_exp_f32 and its companions bound it.
//
// RESOURCES (gfx950, hipcc -O3; the build fails if the main kernel uses scratch): recorded in DESIGN.md section 4.3.
//
// ERROR (what tests/test_gpu_kde_joint.py holds every query to; u = 2^-24). With N = alpha^2 |z_i|^2, N' = alpha^2 |z_q|^2, P <= sqrt(N N'),
// L = log2(e) |lw_i - max| and S = P + N + N' + L the exponent of a pair is off, as in is_pairs.hip, by at most (2 K + 9) S u (the
// fp32 roundings of z, of alpha z, of q and q_q, K products and K additions inside the MFMA at 2 u each), and E - m (|m| <= S + 1)
// rounds once more: delta = (2 K + 12) S u. Every term is >= 0, so with R the largest |z_i| of the group and L_max its largest L
//   eps(q) = expm1(ln 2 (2 K + 12) (alpha^2 (R^2 + |z_q|^2 + R |z_q|) + L_max) u)        the expanded square; grows as h shrinks
//          + 650 u                                                                         v_exp_f32 (2 u), the fp32 sums, fp32(alpha z)
//          + (n + 64) 2^-52 + n 2^-124                                                     fp64 sums, normaliser; terms below 2^-126
//   |log_density - exact| <= -log1p(-eps),    |mean_j - exact| <= 2 eps R / (1 - eps)      (|z_ij| <= R; numerator and denominator)
// (mean sums: a term alpha z_ij p carries the term's error, 2 u of the two roundings of alpha z and 512 u of the 256 products and
// additions of a chunk in the MFMA: below 650 u). The expanded square is NOT re-centred per query tile: the queries of a tile are
// arbitrary points (mean-shift seeds are draws from the whole posterior), so a tile centre does not shrink |z|; the standardisation
// already centres the cloud. At Scott's bandwidth and |z| <= 5 the bound stays below 1e-3 relative at J = 8; at a fifth of it, it
// allows a few per cent, which is what a density estimate that under-smoothed is worth; the observed errors are far below either.
#include "is_pair_image.hpp"

namespace pp {
namespace {

constexpr int QBLOCK = PP_IS_KDEJ_QUERY_BLOCK, QTILE = PP_IS_KDEJ_QUERY_TILE, PBLOCK = PP_IS_KDEJ_PARTICLE_BLOCK;
constexpr int MAX_STRIPS = PP_IS_KDEJ_MAX_STRIPS, TARGET_WG = PP_IS_KDEJ_TARGET_WORKGROUPS, MAXQ = PP_IS_KDEJ_MAX_Q;
constexpr int STRIDE = CHUNK + 4;          // LDS row stride: the 16-byte reads of the J feature rows fall into distinct banks
constexpr int SLOTS = 2 + MAXJ;            // m, sum, mean-sum[8] per (strip, query)
constexpr float M_NONE = -3.0e38f;         // the reference before the first finite exponent
static_assert(QBLOCK == 32 && PBLOCK == 32 && QTILE == QBLOCK * (THREADS / 64) && CHUNK == PP_IS_KDEJ_CHUNK && CHUNK % PBLOCK == 0 &&
                  MAXJ == PP_IS_KDEJ_MAX_J,
              "tiling");

struct Split {
    int QT, chunks, per_strip, S;
    int64_t q_pad;
};
__host__ __device__ inline Split kdej_split(int n_per, int Q) {
    Split s;
    s.QT = ceil_div(Q, QTILE);
    s.q_pad = (int64_t)s.QT * QTILE;
    s.chunks = ceil_div(n_per, CHUNK);
    const int want = min(MAX_STRIPS, max(1, ceil_div(TARGET_WG, s.QT)));
    s.per_strip = ceil_div(s.chunks, want);
    s.S = ceil_div(s.chunks, s.per_strip);
    return s;
}

// Workspace: the image, per operand tile (sum w, sum w^2, count) and the tile maxima, the strips' partials; mean shift adds the seeds'
// states and the word the host reads.
struct KdejWorkspace {
    float* img;
    double* wsum;
    float* tmax;
    double* partial;
    int32_t* state;
    int32_t* all_done;
    size_t bytes;
};
void kdej_carve(int M, int n_per, int J, int Q, bool shift, void* p, KdejWorkspace& w) {
    Carver c(p);
    const int64_t m = std::max(M, 0);
    const int n = std::max(n_per, 1);
    const Split s = kdej_split(n, std::max(Q, 1));
    const int64_t tiles = m * tiles_of(n, OP_TILE);
    w.img = c.take<float>(m * image_k(J) * pad_of(n) * 4);
    w.wsum = c.take<double>(tiles * 3 * 8);
    w.tmax = c.take<float>(tiles * 4);
    w.partial = c.take<double>(m * s.S * SLOTS * s.q_pad * 8);
    w.state = c.take<int32_t>(shift ? m * Q * 4 : 0);
    w.all_done = c.take<int32_t>(shift ? 4 : 0);
    w.bytes = c.bytes();
}
bool kdej_shape_ok(int M, int n_per, int J, int Q) {
    return J >= 1 && J <= MAXJ && Q >= 1 && Q <= MAXQ && groups_shape_ok(M, n_per) && groups_count_ok(M, Q);
}

// ---- 2. main ----------------------------------------------------------------------------------------------------------------------
// Workgroup (query tile blockIdx.x, strip blockIdx.y, group g0 + blockIdx.z). points: [M, Q, J] doubles, in the original coordinates
// (center, inv_scale given) or standardised already (center == nullptr: mean shift's seeds).
template <int K2, bool MEAN>
__global__ __launch_bounds__(THREADS) void kdej_main_kernel(const float* __restrict__ img, const double* __restrict__ points,
                                                            const double* __restrict__ center, const double* __restrict__ inv_scale,
                                                            const double* __restrict__ h, int64_t sh_, int n_per, int Q, int J, int g0,
                                                            double* __restrict__ partial) {
    constexpr int K = 2 * K2;
    __shared__ __attribute__((aligned(16))) float sh[K * STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, c31 = lane & 31, hh = lane >> 5;
    const int64_t g = (int64_t)g0 + blockIdx.z;
    const Split sp = kdej_split(n_per, Q);
    const int64_t pad = pad_of(n_per);
    const float* I = img + g * K * pad;
    const int c_lo = blockIdx.y * sp.per_strip, c_hi = min(sp.chunks, c_lo + sp.per_strip);
    const int q = blockIdx.x * QTILE + (tid >> 6) * QBLOCK + c31;

    // the query's image as a COLUMN: (alpha z_q, 0.., 1, q_q); this lane keeps the features 2 s + hh
    float bq[K2];
    {
        const double hg = h[g * sh_];
        const double alpha = sqrt(LOG2E) / hg, half_alpha2 = 0.5 * LOG2E / (hg * hg);
        const double* x = points + (g * Q + min(q, Q - 1)) * J;      // (a lane behind Q repeats the last query and stores nothing)
        double r2 = 0.0;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const float z = j < J ? (center ? (float)((x[j] - center[g * J + j]) * inv_scale[g * J + j]) : (float)x[j]) : 0.0f;
            r2 += (double)z * (double)z;
        }
#pragma unroll
        for (int s = 0; s < K2; ++s) {
            const int f = 2 * s + hh;      // (below J: a coordinate, read once more rather than kept in an indexed array)
            const int j = min(f, J - 1);
            const float z = center ? (float)((x[j] - center[g * J + j]) * inv_scale[g * J + j]) : (float)x[j];
            bq[s] = f < J ? (float)(alpha * (double)z) : f == K - 2 ? 1.0f : f == K - 1 ? (float)(-half_alpha2 * r2) : 0.0f;
        }
    }
    const int jj = min(c31, J - 1);      // (the rows J .. 31 of the second product repeat row J - 1 and are never read)

    float nx[K];
    auto load = [&](int c) {
#pragma unroll
        for (int f = 0; f < K; ++f) nx[f] = I[f * pad + (int64_t)c * CHUNK + tid];
    };
    float m = M_NONE, m64 = M_NONE, s32 = 0.0f;
    double S64 = 0.0, A64[4] = {0.0, 0.0, 0.0, 0.0};
    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = 0.0f;
    load(c_lo);
    for (int c = c_lo; c < c_hi; ++c) {
        __syncthreads();
#pragma unroll
        for (int f = 0; f < K; ++f) sh[f * STRIDE + tid] = nx[f];
        __syncthreads();
        if (c + 1 < c_hi) load(c + 1);
        for (int b = 0; b < CHUNK / PBLOCK; ++b) {
            f32x16 e;
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < K2; ++s)
                e = __builtin_amdgcn_mfma_f32_32x32x2f32(sh[(2 * s + hh) * STRIDE + PBLOCK * b + c31], bq[s], e, 0, 0, 0);
            float t[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = e[r];
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int r = 0; r < w; ++r) t[r] = fmaxf(t[r], t[r + w]);
            const float bm = fmaxf(t[0], __shfl_xor(t[0], 32, 64));
            const float mn = fmaxf(m, ceilf(bm));
            if (__any(mn > m)) {
                const int d = (int)fmaxf(m - mn, -2000.0f);
                s32 = ldexpf(s32, d);
                if (MEAN) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc2[r] = ldexpf(acc2[r], d);
                }
                m = mn;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_exp2f(e[r] - m);
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = e[r];
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int r = 0; r < w; ++r) t[r] += t[r + w];
            s32 += t[0];
            if (MEAN) {
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 zv = *reinterpret_cast<const f32x4*>(&sh[jj * STRIDE + PBLOCK * b + 8 * r4 + 4 * hh]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(zv[r], e[4 * r4 + r], acc2, 0, 0, 0);
                }
            }
        }
        // the chunk's fp32 sums to fp64, under the same integer reference
        const int d = (int)fmaxf(m64 - m, -2000.0f);
        S64 = ldexp(S64, d) + (double)s32;
        s32 = 0.0f;
        if (MEAN) {
#pragma unroll
            for (int r = 0; r < 4; ++r) A64[r] = ldexp(A64[r], d) + (double)acc2[r];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[r] = 0.0f;
        }
        m64 = m;
    }
    const double S_all = S64 + __shfl_xor(S64, 32, 64);      // (the two halves hold the two halves of every block's particles)
    if (q >= Q) return;
    double* o = partial + ((g * sp.S + blockIdx.y) * SLOTS) * sp.q_pad + q;
    if (hh == 0) {
        o[0] = (double)m;
        o[sp.q_pad] = S_all;
    }
    if (MEAN) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * hh + r < J) o[(2 + 4 * hh + r) * sp.q_pad] = A64[r];
    }
}

// ---- 3. combine -----------------------------------------------------------------------------------------------------------------
// What the strips of query q of group g add up to: log-density (standardised coordinates) and, MEAN, the mean; W and the count of the
// group from the operand tiles. Every thread of the workgroup calls it (block_sum).
struct KdejPoint {
    double log_density, mean[MAXJ], count;
};
__device__ __forceinline__ KdejPoint kdej_point(const double* __restrict__ partial, const double* __restrict__ wsum,
                                                const double* __restrict__ h, int64_t sh_, int n_per, int Q, int J, int64_t g, int q,
                                                bool mean, double* shsum) {
    const Split sp = kdej_split(n_per, Q);
    const int T = ceil_div(n_per, OP_TILE);
    double W = 0.0, cnt = 0.0;
    for (int t = threadIdx.x; t < T; t += THREADS) {
        W += wsum[(g * T + t) * 3];
        cnt += wsum[(g * T + t) * 3 + 2];
    }
    W = block_sum(W, shsum);
    cnt = block_sum(cnt, shsum);
    KdejPoint r;
    r.count = cnt;
    r.log_density = NAN;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) r.mean[j] = NAN;
    if (q >= Q || !(cnt > 0.0)) return r;
    const double* p = partial + g * sp.S * SLOTS * sp.q_pad + q;
    const int64_t strip = SLOTS * sp.q_pad;
    double m = (double)M_NONE;
    for (int s = 0; s < sp.S; ++s) m = fmax(m, p[s * strip]);
    double S = 0.0, A[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) A[j] = 0.0;
    for (int s = 0; s < sp.S; ++s) {
        const int d = (int)fmax(p[s * strip] - m, -2000.0);
        S += ldexp(p[s * strip + sp.q_pad], d);
        if (mean) {
#pragma unroll
            for (int j = 0; j < MAXJ; ++j)
                if (j < J) A[j] += ldexp(p[s * strip + (2 + j) * sp.q_pad], d);
        }
    }
    const double hg = h[g * sh_];
    r.log_density = (0.6931471805599453 * m + log(S)) - log(W) - J * (log(hg) + 0.9189385332046727);
    const double inv = hg / (sqrt(LOG2E) * S);
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (mean && j < J) r.mean[j] = A[j] * inv;
    return r;
}

// Workgroup (256 queries blockIdx.x, group g0 + blockIdx.y).
__global__ __launch_bounds__(THREADS) void kdej_combine_kernel(const double* __restrict__ partial, const double* __restrict__ wsum,
                                                               const double* __restrict__ h, int64_t sh_, int n_per, int Q, int J, int g0,
                                                               double* __restrict__ log_density, double* __restrict__ mean,
                                                               double* __restrict__ count) {
    __shared__ double shsum[THREADS / 64];
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int q = blockIdx.x * THREADS + threadIdx.x;
    const KdejPoint r = kdej_point(partial, wsum, h, sh_, n_per, Q, J, g, q, mean != nullptr, shsum);
    if (q == 0 && count) count[g] = r.count;
    if (q >= Q) return;
    log_density[g * Q + q] = r.log_density;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (mean && j < J) mean[(g * Q + q) * J + j] = r.mean[j];
}

// Mean shift's combine: an open seed moves to its mean IN PLACE (x: [M, Q, J], read by the main launch before, written by this thread
// alone) and is frozen where the step fell below tol h (state 1) or the mean is not a number (state 2: nothing to climb).
__global__ __launch_bounds__(THREADS) void kdej_shift_kernel(const double* __restrict__ partial, const double* __restrict__ wsum,
                                                             const double* __restrict__ h, int64_t sh_, int n_per, int Q, int J, int g0,
                                                             int iter, double tol, double* __restrict__ x, int32_t* __restrict__ state,
                                                             int32_t* __restrict__ n_iter) {
    __shared__ double shsum[THREADS / 64];
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int q = blockIdx.x * THREADS + threadIdx.x;
    const KdejPoint r = kdej_point(partial, wsum, h, sh_, n_per, Q, J, g, q, true, shsum);
    if (q >= Q || state[g * Q + q] != 0) return;
    double step2 = 0.0;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (j < J) {
            const double d = r.mean[j] - x[(g * Q + q) * J + j];
            step2 += d * d;
            x[(g * Q + q) * J + j] = r.mean[j];
        }
    n_iter[g * Q + q] = iter;
    const double lim = tol * h[g * sh_];
    if (!(step2 == step2))
        state[g * Q + q] = 2;
    else if (step2 < lim * lim)
        state[g * Q + q] = 1;
}

__global__ __launch_bounds__(256) void kdej_seed_kernel(const double* __restrict__ seeds, int64_t points, int J, double* __restrict__ x,
                                                        int32_t* __restrict__ state, int32_t* __restrict__ n_iter) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= points) return;
    for (int j = 0; j < J; ++j) x[i * J + j] = seeds[i * J + j];
    state[i] = 0;
    n_iter[i] = 0;
}

// One workgroup: *all_done = no seed is open; FINISH: converged[i] = the seed froze on its step.
template <bool FINISH>
__global__ __launch_bounds__(256) void kdej_fold_kernel(const int32_t* __restrict__ state, int64_t points, int32_t* __restrict__ out) {
    if (FINISH) {
        const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (i < points) out[i] = state[i] == 1;
        return;
    }
    __shared__ int open[4];
    int mine = 0;
    for (int64_t i = threadIdx.x; i < points; i += 256) mine |= state[i] == 0;
    const int w = __any(mine);
    if ((threadIdx.x & 63) == 0) open[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) *out = !(open[0] | open[1] | open[2] | open[3]);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct KdejCall {
    const float* lw;
    PairCols cols;
    const double* stats;
    int n_per, J, M;
    const double *center, *inv_scale, *h;
    int64_t sh;
    hipStream_t st;
};

template <int J>
void launch_operands(const KdejCall& a, const KdejWorkspace& w) {
    const int T = tiles_of(a.n_per, OP_TILE);
    for_each_group_chunk(a.M, [&](int g0, int groups) {
        if (T > 1 && !a.stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, a.st, a.lw, a.n_per, OP_TILE, T, g0, w.tmax);
        hipLaunchKernelGGL((pairs_operand_kernel<J, false>), dim3(T, groups), dim3(THREADS), 0, a.st, a.lw, a.cols, a.n_per, T, g0, a.center,
                           a.inv_scale, a.h, a.sh, a.stats, (const float*)w.tmax, w.img, (float*)nullptr, w.wsum);
    });
}
void kdej_operands(const KdejCall& a, const KdejWorkspace& w) {
    switch (a.J) {
        case 1: launch_operands<1>(a, w); break;
        case 2: launch_operands<2>(a, w); break;
        case 3: launch_operands<3>(a, w); break;
        case 4: launch_operands<4>(a, w); break;
        case 5: launch_operands<5>(a, w); break;
        case 6: launch_operands<6>(a, w); break;
        case 7: launch_operands<7>(a, w); break;
        default: launch_operands<8>(a, w); break;
    }
}

template <int K2, bool MEAN>
void launch_main(const KdejCall& a, const KdejWorkspace& w, const double* points, bool standardised, int Q, int g0, int groups) {
    const Split sp = kdej_split(a.n_per, Q);
    hipLaunchKernelGGL((kdej_main_kernel<K2, MEAN>), dim3(sp.QT, sp.S, groups), dim3(THREADS), 0, a.st, (const float*)w.img, points,
                       standardised ? nullptr : a.center, a.inv_scale, a.h, a.sh, a.n_per, Q, a.J, g0, w.partial);
}
void kdej_main(const KdejCall& a, const KdejWorkspace& w, const double* points, bool standardised, int Q, bool mean, int g0, int groups) {
    switch (image_k(a.J) / 2 * 2 + (mean ? 1 : 0)) {
        case 4: launch_main<2, false>(a, w, points, standardised, Q, g0, groups); break;
        case 5: launch_main<2, true>(a, w, points, standardised, Q, g0, groups); break;
        case 6: launch_main<3, false>(a, w, points, standardised, Q, g0, groups); break;
        case 7: launch_main<3, true>(a, w, points, standardised, Q, g0, groups); break;
        case 8: launch_main<4, false>(a, w, points, standardised, Q, g0, groups); break;
        case 9: launch_main<4, true>(a, w, points, standardised, Q, g0, groups); break;
        case 10: launch_main<5, false>(a, w, points, standardised, Q, g0, groups); break;
        default: launch_main<5, true>(a, w, points, standardised, Q, g0, groups); break;
    }
}
void kdej_evaluate(const KdejCall& a, const KdejWorkspace& w, const double* points, bool standardised, int Q, double* log_density,
                   double* mean, double* count) {
    for_each_group_chunk(a.M, [&](int g0, int groups) {
        kdej_main(a, w, points, standardised, Q, mean != nullptr, g0, groups);
        hipLaunchKernelGGL(kdej_combine_kernel, dim3(cdiv(Q, THREADS), groups), dim3(THREADS), 0, a.st, (const double*)w.partial,
                           (const double*)w.wsum, a.h, a.sh, a.n_per, Q, a.J, g0, log_density, mean, count);
    });
}

// The checks and the call description the two entry points share.
int kdej_call(const char* name, const float* lw, const float* const* cols, const double* stats, int n_per, int J, int M,
              const double* center, const double* inv_scale, const double* h, int64_t sh, int Q, hipStream_t st, KdejCall& a) {
    PP_CHECK_ARG(lw && cols && center && inv_scale && h, "%s: null pointer (only stats and optional outputs may be null)", name);
    PP_CHECK_ARG(J >= 1 && J <= MAXJ, "%s: n_cols in 1 .. %d", name, MAXJ);
    PP_CHECK_ARG(n_per >= 1 && M >= 0, "%s: n_per >= 1 and n_groups >= 0", name);
    PP_CHECK_ARG(groups_count_ok(M, n_per), "%s: more than 2^31 - 1 particles per call: shard the groups", name);
    PP_CHECK_ARG(Q >= 1 && Q <= MAXQ && groups_count_ok(M, Q), "%s: 1 .. %d points per group, at most 2^31 - 1 per call", name, MAXQ);
    PP_CHECK_ARG(sh == 0 || sh == 1, "%s: bandwidth_stride is 0 (shared) or 1", name);
    a = KdejCall{lw, {}, stats, n_per, J, M, center, inv_scale, h, sh, st};
    for (int j = 0; j < MAXJ; ++j) {
        a.cols.p[j] = j < J ? cols[j] : nullptr;
        PP_CHECK_ARG(j >= J || cols[j], "%s: null column pointer %d", name, j);
    }
    return 0;
}

}  // namespace

int is_kde_joint_groups(const float* lw, const float* const* cols, const double* stats, int n_per, int J, int M, const double* center,
                        const double* inv_scale, const double* h, int64_t sh, const double* points, int Q, double* log_density,
                        double* mean, double* count, void* ws, size_t ws_bytes, hipStream_t st) {
    KdejCall a;
    PP_TRY(kdej_call("pp_is_kde_joint_groups", lw, cols, stats, n_per, J, M, center, inv_scale, h, sh, Q, st, a));
    PP_CHECK_ARG(points && log_density && ws, "pp_is_kde_joint_groups: null pointer (points, log_density and the workspace are required)");
    KdejWorkspace w;
    kdej_carve(M, n_per, J, Q, false, ws, w);
    PP_CHECK_WORKSPACE("pp_is_kde_joint_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    kdej_operands(a, w);
    kdej_evaluate(a, w, points, false, Q, log_density, mean, count);
    PP_LAUNCH_CHECK("pp_is_kde_joint_groups");
    return 0;
}

int is_meanshift_groups(const float* lw, const float* const* cols, const double* stats, int n_per, int J, int M, const double* center,
                        const double* inv_scale, const double* h, int64_t sh, const double* seeds, int Q, double tol, int max_iter,
                        int check_every, double* x, double* log_density, int32_t* n_iter, int32_t* converged, double* count, void* ws,
                        size_t ws_bytes, hipStream_t st) {
    const char* name = "pp_is_meanshift_groups";
    KdejCall a;
    PP_TRY(kdej_call(name, lw, cols, stats, n_per, J, M, center, inv_scale, h, sh, Q, st, a));
    PP_CHECK_ARG(seeds && x && log_density && n_iter && converged && ws, "%s: null pointer (only stats and count may be null)", name);
    PP_CHECK_ARG(max_iter >= 1 && tol >= 0.0, "%s: max_iter >= 1 and tol >= 0", name);
    KdejWorkspace w;
    kdej_carve(M, n_per, J, Q, true, ws, w);
    PP_CHECK_WORKSPACE("pp_is_meanshift_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    if (check_every < 1) check_every = 8;
    const int64_t points = (int64_t)M * Q;
    kdej_operands(a, w);
    hipLaunchKernelGGL(kdej_seed_kernel, dim3(cdiv(points, 256)), dim3(256), 0, st, seeds, points, J, x, w.state, n_iter);
    for (int iter = 1; iter <= max_iter; ++iter) {
        for_each_group_chunk(M, [&](int g0, int groups) {
            kdej_main(a, w, x, true, Q, true, g0, groups);
            hipLaunchKernelGGL(kdej_shift_kernel, dim3(cdiv(Q, THREADS), groups), dim3(THREADS), 0, st, (const double*)w.partial,
                               (const double*)w.wsum, h, sh, n_per, Q, J, g0, iter, tol, x, w.state, n_iter);
        });
        if (iter % check_every == 0 && iter < max_iter) {
            int done = 0;
            hipLaunchKernelGGL(kdej_fold_kernel<false>, dim3(1), dim3(256), 0, st, (const int32_t*)w.state, points, w.all_done);
            PP_LAUNCH_CHECK(name);
            hipError_t e = hipMemcpyAsync(&done, w.all_done, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                set_error("%s: reading the converged word failed: %s", name, hipGetErrorString(e));
                return (int)e;
            }
            if (done) break;
        }
    }
    kdej_evaluate(a, w, x, true, Q, log_density, nullptr, count);
    hipLaunchKernelGGL(kdej_fold_kernel<true>, dim3(cdiv(points, 256)), dim3(256), 0, st, (const int32_t*)w.state, points, converged);
    PP_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_kde_joint_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_cols, int32_t n_points, int32_t meanshift) {
    if (!pp::kdej_shape_ok(n_groups, n_per, n_cols, n_points)) return 0;
    pp::KdejWorkspace w;
    pp::kdej_carve(n_groups, n_per, n_cols, n_points, meanshift != 0, nullptr, w);
    return w.bytes;
}

int32_t pp_is_kde_joint_strips(int32_t n_per, int32_t n_points) {
    if (n_per < 1 || n_points < 1 || n_points > PP_IS_KDEJ_MAX_Q) return 0;
    return pp::kdej_split(n_per, n_points).S;
}

int pp_is_kde_joint_groups(const float* lw, const float* const* cols, const double* stats, int32_t n_per, int32_t n_cols, int32_t n_groups,
                           const double* center, const double* inv_scale, const double* bandwidth, int64_t bandwidth_stride,
                           const double* points, int32_t n_points, double* log_density, double* mean, double* count, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return pp::is_kde_joint_groups(lw, cols, stats, n_per, n_cols, n_groups, center, inv_scale, bandwidth, bandwidth_stride, points,
                                   n_points, log_density, mean, count, workspace, workspace_bytes, pp::as_stream(stream));
}

int pp_is_meanshift_groups(const float* lw, const float* const* cols, const double* stats, int32_t n_per, int32_t n_cols, int32_t n_groups,
                           const double* center, const double* inv_scale, const double* bandwidth, int64_t bandwidth_stride,
                           const double* seeds, int32_t n_seeds, double tol, int32_t max_iter, int32_t check_every, double* points,
                           double* log_density, int32_t* n_iter, int32_t* converged, double* count, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return pp::is_meanshift_groups(lw, cols, stats, n_per, n_cols, n_groups, center, inv_scale, bandwidth, bandwidth_stride, seeds, n_seeds,
                                   tol, max_iter, check_every, points, log_density, n_iter, converged, count, workspace, workspace_bytes,
                                   pp::as_stream(stream));
}

}  // extern "C"
