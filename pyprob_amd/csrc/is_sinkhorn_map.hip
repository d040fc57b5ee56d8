// The barycentric projection of an entropic transport plan between the JOINT particles of two lock-step posteriors, in both directions
// (Empirical.sinkhorn(transport=True)). The reference has no distance between two Empiricals, let alone a map. include/pyprob_amd.h
// states the definition: given the potentials f, g of problem (a, b) - plain inputs, converged or not - per particle i of side a
//     map_ab[i]     = center + scale sum_j P_ij z'_j / sum_j P_ij,      P_ij = a_i b_j exp((f_i + g_j - C_ij) / eps)
//     log_mass_a[i] = log(sum_j P_ij / a_i) = f_i / eps + log sum_j b_j exp((g_j - C_ij) / eps)        (0 where the marginal holds)
// and the mirror per particle of side b. The query's own potential and weight cancel in the map: per query it is a softmax over the
// particles of the other ("summed") side of E = log2(e) (lw - max + pot / eps) - alpha^2 |z - z'|^2 / 2, alpha^2 = log2(e) / eps - the
// exponents of a Sinkhorn half-step - whose normaliser is the row mass and whose weighted mean of the summed side's coordinates is the
// map. Nothing of size n_a x n_b is stored. This file shares is_pair_image.hpp and common.hpp with the other pair operators and
// nothing else; the tiling constants are pp_is_sinkhorn_groups' (PP_IS_SINKHORN_*), so a map costs about what a half-step's strips do.
//
// LAUNCHES, dependent on the caller's stream, no atomics, no workgroup waits for another.
// 1. OPERANDS (map_operand_kernel<J>, once per side): pairs_operand_kernel's particles, rule and arithmetic with alpha from eps; the
//    image of is_pair_image.hpp, feature-major [K][n_pad] = (alpha z, 0.., q, 1) with the side's potential IN q: q = fp32(base + log2(e)
//    pot / eps), base = log2(e) (lw - max) - alpha^2 |z|^2 / 2, formed in fp64, ONE rounding (-inf where the particle does not count,
//    whatever its potential is); the query column nq = fp32(-alpha^2 |z|^2 / 2); in fp64 pot / eps (NaN where the particle does not
//    count: the combine's flag) and per 2048 particles (sum w, count).
// 2. MAIN (map_main_kernel<K / 2>, ONE launch: the directions that were asked for, of all groups, ride on grid dimension z). A
//    workgroup of four waves owns QTILE = 128 queries - any number of tiles on grid dimension x - and ONE strip of the summed side,
//    staged through LDS in chunks of 256 (global -> registers one chunk ahead -> LDS, row stride 260 floats; the row of ones is written
//    once). The query fragment (alpha z_q, 0.., 1, nq_q) is built in registers from the rows of the query side's OWN image. Per
//    32-particle block a wave
//      a. takes the 32 x 32 exponents from K / 2 v_mfma_f32_32x32x2_f32, particles as rows and queries as columns: a lane holds the 16
//         particles 8 (r / 4) + 4 (lane / 32) + r % 4 of ONE query, lane % 32;
//      b. raises the INTEGER running maximum m of its query (per-lane maximum of the 16, one exchange with the partner half-wave, ceil);
//         what was summed under the old m is rescaled by v_ldexp_f32 - exact - in the blocks where some lane's m rose (a wave-uniform
//         branch; the bits do not depend on it: 2^0 = 1);
//      c. p_r = v_exp_f32(E_r - m) in (0, 1];
//      d. SECOND PRODUCT on the matrix pipe with the p_r as B operands STRAIGHT FROM THE ACCUMULATOR REGISTERS: in the MFMA of register
//         r the k index is the pair of particles the two half-waves hold in p_r; A row j < J is alpha z'_j of those two particles, and
//         every A row from J on is the staged ROW OF ONES (one ds_read_b128 per four r, a broadcast for the lanes >= J). 16 MFMAs per
//         block; result rows 0 .. J - 1 are the mean-sums and row 8 - register 4 of the lower half-wave, a row of ones at every J <=
//         8 - is sum p, the normaliser: it comes off the matrix pipe, in rows that were padding, and the tree of 15 additions and the
//         exchange of the two half-sums that a half-step pays on the VALU are not there.
//    Every chunk the five fp32 sums of a lane (at most 256 products each) are flushed to fp64 under the same integer reference. The
//    strip stores (m, sum, mean-sum[J]) per query: partial[group][direction][strip][slot][q_pad]. The strips are a function of
//    (n_summed, n_query) alone (map_split: pp_is_sinkhorn_strips' rule).
// 3. COMBINE (map_combine_kernel, a thread per query, both directions on grid dimension y): the strips in strip order under the
//    largest m (ldexp, exact), then log_mass = pot_q / eps + ln 2 m + log(sum) - log W and map_j = center_j + (mean-sum_j / (alpha
//    sum)) / inv_scale_j; NaN rows for a query that does not count and for a group whose summed side has no counted particle.
// The order of every sum is a function of (n_a, n_b, J) alone: two calls give the same bits, and group g of an M-group call gives the
// bits of its own one-group call.
//
// WHICH PIPE BOUNDS THE PASS - a DERIVATION until profiles/sinkhorn_map_bench.json says otherwise. Per 32 x 32 block a wave issues K / 2 +
// 16 MFMAs of 16 passes (64 cycles each: 1344 cycles at J = 7, 8, 1152 at J <= 2) against 16 v_exp_f32 (quarter rate, 16 cycles each:
// 256 cycles) and about 55 full-rate VALU operations (16 subtractions, the tree of 15 maxima, the copies out of the accumulator, the
// exchange and the ceil: some 220 cycles) and 4 + K / 2 LDS reads. The matrix pipe carries 1344 cycles, the VALU about 480: the second
// product bounds the pass at every J, and of its 32 result rows J + 1 are used. The row of ones makes that padding pay for the
// normaliser (the VALU sheds 60 cycles it could not hide behind anything at J <= 2) but does not shorten the matrix pipe's share;
// v_mfma_f32_16x16x4_f32 would halve the second product's passes, at the price is_kde_joint.hip states - a query's exponents over
// four lanes, two exchanges and a rescale per 4 exponents - and was not chosen here. The bench file's first
// record agrees with the count: at 10^5 against 10^5 particles and J = 8 the pass runs at 0.69 of the fp32 MFMA peak with the padding
// rows counted and at 0.13 of the v_exp_f32 rate; at 10^4 against 10^4 (0.29 of the peak) its six short launches weigh as much.
//
// RESOURCES (gfx950, hipcc -O3; the build fails if the main or the combine kernel uses scratch): recorded in DESIGN.md section 4.3.
//
// ERROR (what tests/test_gpu_sinkhorn_map.py holds every element to; u = 2^-24). Per direction, with N = alpha^2 |z'_j|^2, N' = alpha^2
// |z_q|^2, P <= sqrt(N N'), L = log2(e) |lw_j - max|, F = log2(e) |pot_j| / eps of the SUMMED particle and S = P + N + N' + L + F, the
// exponent of a pair is off, as in is_sinkhorn.hip, by at most (2 K + 9) S u (the fp32 roundings of z, alpha z, q and nq; K products
// and K additions inside the MFMA at 2 u each), and E - m (|m| <= S + 1) rounds once more: (2 K + 12) S u. With R_s, R_q the largest |z|
// of the summed and the query side, L_max and F_max the largest L and F of the summed side:
//   e = expm1(ln 2 (2 K + 12) (alpha^2 (R_s^2 + R_q^2 + R_s R_q) + L_max + F_max) u)     the expanded square and the potential in q
//     + 650 u                                                                            v_exp_f32 (2 u), the fp32 sums, fp32(alpha z)
//     + (n + 64) 2^-52 + n 2^-124                                                        fp64 sums, log W; terms below 2^-126
// (the normaliser's fp32 sum is now 256 additions of exact products p x 1 per chunk inside the MFMA, 256 u, where the half-step had a
// tree and 128 terms; a mean-sum's term alpha z'_j p carries 2 u of the roundings of alpha z' and 512 u of the 256 products and
// additions of a chunk: both below 650 u with v_exp_f32's 2 u.) Numerator and denominator of the mean are each within a factor 1 +- e
// of exact sums of terms bounded by R_s times the denominator's, so, is_kde_joint.hip's formula,
//   |mean_j - exact| <= 2 e R_s / (1 - e)     in standardised units,
//   |map_j - exact|  <= scale_j 2 e R_s / (1 - e) + 2^-50 (|center_j| + scale_j R_s)     (inv_scale = fl(1 / scale), the fp64 epilogue)
//   |log_mass - exact| <= -log1p(-e) + 2^-50 (log2(e) |pot_q| / eps + alpha^2 (R_s^2 + R_q^2 + R_s R_q) + L_max + F_max)
// the last term the fp64 additions of pot_q / eps, ln 2 m, log(sum) and log W, each at most that large. A query 40 units from every
// summed particle has exponents near -alpha^2 800: m follows the largest wherever it lies, its term is in (1/2, 1], and the map comes
// out finite at (about) the nearest particle - while alpha |z| < 2^30, the counting rule.
#include "is_pair_image.hpp"

namespace pp {
namespace {

constexpr int QBLOCK = PP_IS_SINKHORN_QUERY_BLOCK, QTILE = PP_IS_SINKHORN_QUERY_TILE, PBLOCK = PP_IS_SINKHORN_PARTICLE_BLOCK;
constexpr int MAX_STRIPS = PP_IS_SINKHORN_MAX_STRIPS, TARGET_WG = PP_IS_SINKHORN_TARGET_WORKGROUPS;
constexpr int STRIDE = CHUNK + 4;          // LDS row stride: the 16-byte reads of the J feature rows fall into distinct banks
constexpr int SUM_REG = 4;                 // accumulator register of result row 8 (lower half-wave): the row of ones' product, sum p
constexpr float M_NONE = -3.0e38f;         // the reference before the first finite exponent
static_assert(QBLOCK == 32 && PBLOCK == 32 && QTILE == QBLOCK * (THREADS / 64) && CHUNK == PP_IS_SINKHORN_CHUNK && CHUNK % PBLOCK == 0 &&
                  MAXJ == PP_IS_SINKHORN_MAX_J && MAXJ <= 8 && 2 * PP_IS_SINKHORN_MAX_GROUPS <= 65535,
              "tiling");

struct Split {
    int QT, chunks, per_strip, S;
    int64_t q_pad;
};
__host__ __device__ inline Split map_split(int n_sum, int n_query) {
    Split s;
    s.QT = ceil_div(n_query, QTILE);
    s.q_pad = (int64_t)s.QT * QTILE;
    s.chunks = ceil_div(n_sum, CHUNK);
    const int want = min(MAX_STRIPS, max(1, ceil_div(TARGET_WG, s.QT)));
    s.per_strip = ceil_div(s.chunks, want);
    s.S = ceil_div(s.chunks, s.per_strip);
    return s;
}

// Direction 0: the queries are side a, side b is summed (map_ab, log_mass_a); direction 1 the mirror.
struct Dir {
    int n_s, n_q;
};
__host__ __device__ inline Dir dir_of(int d, int na, int nb) { return d ? Dir{na, nb} : Dir{nb, na}; }
// Doubles of one (group, direction) region of the partials: the larger S (2 + J) q_pad of the two directions.
inline int64_t partial_region(int na, int nb, int J) {
    int64_t r = 0;
    for (int d = 0; d < 2; ++d) {
        const Split s = map_split(dir_of(d, na, nb).n_s, dir_of(d, na, nb).n_q);
        r = std::max(r, (int64_t)s.S * (2 + J) * s.q_pad);
    }
    return r;
}

// What the kernels read and write, per side (0: a, 1: b): see the head comment. first, dirs: the directions of this call.
struct MapDev {
    float *img0, *img1, *nq0, *nq1;
    double *potq0, *potq1, *wsum0, *wsum1, *partial;
    const double *eps, *center, *inv_scale;
    int na, nb, J, first, dirs;
    int64_t region;
};
struct MapWorkspace {
    MapDev d;
    float* tmax[2];
    size_t bytes;
};
void map_carve(int M, int na, int nb, int J, void* p, MapWorkspace& w) {
    Carver c(p);
    const int64_t m = std::max(M, 0);
    na = std::max(na, 1);
    nb = std::max(nb, 1);
    const int64_t pa = m * pad_of(na), pb = m * pad_of(nb);
    MapDev& d = w.d;
    d.img0 = c.take<float>(pa * image_k(J) * 4);
    d.img1 = c.take<float>(pb * image_k(J) * 4);
    d.nq0 = c.take<float>(pa * 4);
    d.nq1 = c.take<float>(pb * 4);
    d.potq0 = c.take<double>(pa * 8);
    d.potq1 = c.take<double>(pb * 8);
    d.wsum0 = c.take<double>(m * tiles_of(na, OP_TILE) * 2 * 8);
    d.wsum1 = c.take<double>(m * tiles_of(nb, OP_TILE) * 2 * 8);
    w.tmax[0] = c.take<float>(m * tiles_of(na, OP_TILE) * 4);
    w.tmax[1] = c.take<float>(m * tiles_of(nb, OP_TILE) * 4);
    d.na = na;
    d.nb = nb;
    d.J = J;
    d.first = 0;
    d.dirs = 2;
    d.region = partial_region(na, nb, J);
    d.partial = c.take<double>(m * 2 * d.region * 8);
    d.eps = d.center = d.inv_scale = nullptr;
    w.bytes = c.bytes();
}
bool map_shape_ok(int M, int na, int nb, int J) {
    return J >= 1 && J <= MAXJ && M <= PP_IS_SINKHORN_MAX_GROUPS && groups_shape_ok(M, na) && groups_shape_ok(M, nb);
}

// ---- 1. operands ------------------------------------------------------------------------------------------------------------------
// Workgroup (tile blockIdx.x, group blockIdx.y) of one side: particles tile 2048 + tid + 256 k. pot: the side's potential [M, n_per].
template <int J>
__global__ __launch_bounds__(THREADS) void map_operand_kernel(const float* __restrict__ lw, PairCols cols, int n_per, int T,
                                                              const double* __restrict__ center, const double* __restrict__ inv_scale,
                                                              const double* __restrict__ eps, const double* __restrict__ pot,
                                                              const double* __restrict__ stats, const float* __restrict__ tmax,
                                                              float* __restrict__ img, float* __restrict__ nq, double* __restrict__ potq,
                                                              double* __restrict__ wsum) {
    constexpr int K = image_k(J);
    __shared__ float shmax[THREADS / 64];
    __shared__ double shsum[THREADS / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int64_t g = blockIdx.y, base = g * n_per, pad = pad_of(n_per);
    const int64_t first = (int64_t)tile * OP_TILE + tid;
    float a[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + THREADS * k;
        a[k] = i < n_per ? lw[base + i] : -INFINITY;
    }
    const double M = group_max<THREADS>(stats, tmax, g, T, a, shmax);
    const bool any = group_any(M);
    const double e = eps[g];
    const double alpha = sqrt(LOG2E / e), half_alpha2 = 0.5 * LOG2E / e;
    double c[J], is[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        c[j] = center[g * J + j];
        is[j] = inv_scale[g * J + j];
    }
    float* gi = img + g * K * pad;
    double W = 0.0, cnt = 0.0;
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
        const double p = ok ? pot[base + i] : NAN;          // (ok implies i < n_per)
#pragma unroll
        for (int j = 0; j < J; ++j) gi[j * pad + i] = ok ? (float)(alpha * (double)z[j]) : 0.0f;
#pragma unroll
        for (int f = J; f < K - 2; ++f) gi[f * pad + i] = 0.0f;
        gi[(K - 2) * pad + i] = ok ? (float)((LOG2E * ((double)a[k] - M) - half_alpha2 * r2) + LOG2E * p / e) : -INFINITY;
        gi[(K - 1) * pad + i] = 1.0f;
        nq[g * pad + i] = ok ? (float)(-half_alpha2 * r2) : 0.0f;
        potq[g * pad + i] = p / e;
        W += w;
        cnt += ok ? 1.0 : 0.0;
    }
    W = block_sum(W, shsum);
    cnt = block_sum(cnt, shsum);
    if (tid == 0) {
        double* o = wsum + (g * T + tile) * 2;
        o[0] = W;
        o[1] = cnt;
    }
}

// ---- 2. main ----------------------------------------------------------------------------------------------------------------------
// Workgroup (query tile blockIdx.x, strip blockIdx.y, group and direction on blockIdx.z). A workgroup beyond its direction's tiles or
// strips returns.
template <int K2>
__global__ __launch_bounds__(THREADS) void map_main_kernel(MapDev d) {
    constexpr int K = 2 * K2;
    __shared__ __attribute__((aligned(16))) float sh[K * STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, c31 = lane & 31, hh = lane >> 5;
    const int slot = blockIdx.z % d.dirs, dir = d.first + slot, J = d.J;
    const int64_t g = blockIdx.z / d.dirs;
    const Dir job = dir_of(dir, d.na, d.nb);
    const Split sp = map_split(job.n_s, job.n_q);
    if ((int)blockIdx.x >= sp.QT || (int)blockIdx.y >= sp.S) return;
    const int64_t pad_s = pad_of(job.n_s), pad_q = pad_of(job.n_q);
    const float* I = (dir ? d.img0 : d.img1) + g * K * pad_s;
    const float* Q = (dir ? d.img1 : d.img0) + g * K * pad_q;
    const float* NQ = (dir ? d.nq1 : d.nq0) + g * pad_q;
    const int c_lo = blockIdx.y * sp.per_strip, c_hi = min(sp.chunks, c_lo + sp.per_strip);
    const int q = blockIdx.x * QTILE + (tid >> 6) * QBLOCK + c31;      // (< q_pad <= pad_q: the padding's image is zeros)

    // the query's image as a COLUMN, from the rows of its own side's image: (alpha z_q, 0.., 1, nq_q); this lane keeps features 2 s + hh
    float bq[K2];
#pragma unroll
    for (int s = 0; s < K2 - 1; ++s) bq[s] = Q[(2 * s + hh) * pad_q + q];
    bq[K2 - 1] = hh ? NQ[q] : 1.0f;
    const int jj = c31 < J ? c31 : K - 1;      // the second product's A row of this lane: a coordinate row, or the row of ones

    float nx[K - 1];
    auto load = [&](int c) {
#pragma unroll
        for (int f = 0; f < K - 1; ++f) nx[f] = I[f * pad_s + (int64_t)c * CHUNK + tid];
    };
    sh[(K - 1) * STRIDE + tid] = 1.0f;      // (the row of ones: written once, the staging below leaves it alone)
    float m = M_NONE, m64 = M_NONE;
    double A64[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = 0.0f;
    load(c_lo);
    for (int c = c_lo; c < c_hi; ++c) {
        __syncthreads();
#pragma unroll
        for (int f = 0; f < K - 1; ++f) sh[f * STRIDE + tid] = nx[f];
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
                const int dm = (int)fmaxf(m - mn, -2000.0f);
#pragma unroll
                for (int r = 0; r <= SUM_REG; ++r) acc2[r] = ldexpf(acc2[r], dm);
                m = mn;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_exp2f(e[r] - m);
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 zv = *reinterpret_cast<const f32x4*>(&sh[jj * STRIDE + PBLOCK * b + 8 * r4 + 4 * hh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(zv[r], e[4 * r4 + r], acc2, 0, 0, 0);
            }
        }
        // the chunk's fp32 sums to fp64, under the same integer reference
        const int dm = (int)fmaxf(m64 - m, -2000.0f);
#pragma unroll
        for (int r = 0; r <= SUM_REG; ++r) A64[r] = ldexp(A64[r], dm) + (double)acc2[r];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[r] = 0.0f;
        m64 = m;
    }
    if (q >= job.n_q) return;
    double* o = d.partial + (g * 2 + slot) * d.region + (int64_t)blockIdx.y * (2 + J) * sp.q_pad + q;
    if (hh == 0) {
        o[0] = (double)m;
        o[sp.q_pad] = A64[SUM_REG];      // (result row 8: both half-waves' particles are in it, the MFMA summed over k)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (4 * hh + r < J) o[(2 + 4 * hh + r) * sp.q_pad] = A64[r];
}

// ---- 3. combine -----------------------------------------------------------------------------------------------------------------
// Workgroup (256 queries blockIdx.x, direction slot blockIdx.y, group blockIdx.z). out_map: [M, n_q, J], out_mass: [M, n_q], per
// direction; either may be null.
__global__ __launch_bounds__(THREADS) void map_combine_kernel(MapDev d, double* __restrict__ map0, double* __restrict__ map1,
                                                              double* __restrict__ mass0, double* __restrict__ mass1) {
    __shared__ double shsum[THREADS / 64];
    const int slot = blockIdx.y, dir = d.first + slot, J = d.J;
    const int64_t g = blockIdx.z;
    const Dir job = dir_of(dir, d.na, d.nb);
    if ((int)blockIdx.x * THREADS >= job.n_q) return;
    const Split sp = map_split(job.n_s, job.n_q);
    const int T = ceil_div(job.n_s, OP_TILE);
    const double* wsum = dir ? d.wsum0 : d.wsum1;
    double W = 0.0, cnt = 0.0;
    for (int t = threadIdx.x; t < T; t += THREADS) {
        W += wsum[(g * T + t) * 2];
        cnt += wsum[(g * T + t) * 2 + 1];
    }
    W = block_sum(W, shsum);
    cnt = block_sum(cnt, shsum);
    const int q = blockIdx.x * THREADS + threadIdx.x;
    if (q >= job.n_q) return;
    const double pe = (dir ? d.potq1 : d.potq0)[g * pad_of(job.n_q) + q];
    double lm = NAN, mean[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) mean[j] = NAN;
    if (cnt > 0.0 && pe == pe) {
        const double* p = d.partial + (g * 2 + slot) * d.region + q;
        const int64_t strip = (2 + J) * sp.q_pad;
        double m = (double)M_NONE;
        for (int s = 0; s < sp.S; ++s) m = fmax(m, p[s * strip]);
        double S = 0.0, A[MAXJ];
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) A[j] = 0.0;
        for (int s = 0; s < sp.S; ++s) {
            const int dm = (int)fmax(p[s * strip] - m, -2000.0);
            S += ldexp(p[s * strip + sp.q_pad], dm);
#pragma unroll
            for (int j = 0; j < MAXJ; ++j)
                if (j < J) A[j] += ldexp(p[s * strip + (2 + j) * sp.q_pad], dm);
        }
        lm = pe + ((0.6931471805599453 * m + log(S)) - log(W));
        const double inv = 1.0 / (sqrt(LOG2E / d.eps[g]) * S);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < J) mean[j] = d.center[g * J + j] + (A[j] * inv) / d.inv_scale[g * J + j];
    }
    double* om = dir ? map1 : map0;
    double* ol = dir ? mass1 : mass0;
    if (ol) ol[g * job.n_q + q] = lm;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (om && j < J) om[(g * job.n_q + q) * J + j] = mean[j];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct MapSide {
    const float* lw;
    PairCols cols;
    const double *stats, *pot;
    int n_per;
};

template <int J>
void launch_operands(hipStream_t st, const MapSide (&side)[2], int M, const MapWorkspace& w) {
    const MapDev& d = w.d;
    for (int s = 0; s < 2; ++s) {
        const int T = tiles_of(side[s].n_per, OP_TILE);
        if (T > 1 && !side[s].stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, M), dim3(256), 0, st, side[s].lw, side[s].n_per, OP_TILE, T, 0, w.tmax[s]);
        hipLaunchKernelGGL(map_operand_kernel<J>, dim3(T, M), dim3(THREADS), 0, st, side[s].lw, side[s].cols, side[s].n_per, T, d.center,
                           d.inv_scale, d.eps, side[s].pot, side[s].stats, (const float*)w.tmax[s], s ? d.img1 : d.img0,
                           s ? d.nq1 : d.nq0, s ? d.potq1 : d.potq0, s ? d.wsum1 : d.wsum0);
    }
}

template <int K2>
void launch_main(hipStream_t st, const MapDev& d, int M) {
    int QT = 0, S = 0;
    for (int k = d.first; k < d.first + d.dirs; ++k) {
        const Split sp = map_split(dir_of(k, d.na, d.nb).n_s, dir_of(k, d.na, d.nb).n_q);
        QT = std::max(QT, sp.QT);
        S = std::max(S, sp.S);
    }
    hipLaunchKernelGGL(map_main_kernel<K2>, dim3(QT, S, d.dirs * M), dim3(THREADS), 0, st, d);
}

}  // namespace

int is_sinkhorn_map_groups(const float* lw_a, const float* const* cols_a, const double* stats_a, int na, const float* lw_b,
                           const float* const* cols_b, const double* stats_b, int nb, int J, int M, const double* center,
                           const double* inv_scale, const double* eps, const double* f, const double* g, double* map_ab, double* map_ba,
                           double* log_mass_a, double* log_mass_b, void* ws, size_t ws_bytes, hipStream_t st) {
    const char* name = "pp_is_sinkhorn_map_groups";
    PP_CHECK_ARG(lw_a && cols_a && lw_b && cols_b && center && inv_scale && eps && f && g && ws,
                 "%s: null pointer (only stats_a, stats_b and the outputs may be null)", name);
    PP_CHECK_ARG(J >= 1 && J <= MAXJ, "%s: n_cols in 1 .. %d", name, MAXJ);
    PP_CHECK_ARG(na >= 1 && nb >= 1 && M >= 0 && M <= PP_IS_SINKHORN_MAX_GROUPS, "%s: n_per_a, n_per_b >= 1 and n_groups in 0 .. %d", name,
                 PP_IS_SINKHORN_MAX_GROUPS);
    PP_CHECK_ARG(groups_count_ok(M, na) && groups_count_ok(M, nb), "%s: more than 2^31 - 1 particles per call: shard the groups", name);
    MapSide side[2] = {{lw_a, {}, stats_a, f, na}, {lw_b, {}, stats_b, g, nb}};
    for (int j = 0; j < MAXJ; ++j) {
        side[0].cols.p[j] = j < J ? cols_a[j] : nullptr;
        side[1].cols.p[j] = j < J ? cols_b[j] : nullptr;
        PP_CHECK_ARG(j >= J || (cols_a[j] && cols_b[j]), "%s: null column pointer %d", name, j);
    }
    MapWorkspace w;
    map_carve(M, na, nb, J, ws, w);
    PP_CHECK_WORKSPACE("pp_is_sinkhorn_map_groups", ws_bytes, w.bytes);
    const bool want[2] = {map_ab || log_mass_a, map_ba || log_mass_b};
    if (M == 0 || !(want[0] || want[1])) return 0;
    MapDev& d = w.d;
    d.eps = eps;
    d.center = center;
    d.inv_scale = inv_scale;
    d.first = want[0] ? 0 : 1;
    d.dirs = (want[0] ? 1 : 0) + (want[1] ? 1 : 0);
    switch (J) {
        case 1: launch_operands<1>(st, side, M, w); break;
        case 2: launch_operands<2>(st, side, M, w); break;
        case 3: launch_operands<3>(st, side, M, w); break;
        case 4: launch_operands<4>(st, side, M, w); break;
        case 5: launch_operands<5>(st, side, M, w); break;
        case 6: launch_operands<6>(st, side, M, w); break;
        case 7: launch_operands<7>(st, side, M, w); break;
        default: launch_operands<8>(st, side, M, w); break;
    }
    switch (image_k(J) / 2) {
        case 2: launch_main<2>(st, d, M); break;
        case 3: launch_main<3>(st, d, M); break;
        case 4: launch_main<4>(st, d, M); break;
        default: launch_main<5>(st, d, M); break;
    }
    const int nq = d.dirs == 2 ? std::max(na, nb) : (d.first ? nb : na);
    hipLaunchKernelGGL(map_combine_kernel, dim3(ceil_div(nq, THREADS), d.dirs, M), dim3(THREADS), 0, st, d, map_ab, map_ba, log_mass_a,
                       log_mass_b);
    PP_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_sinkhorn_map_workspace_bytes(int32_t n_groups, int32_t n_per_a, int32_t n_per_b, int32_t n_cols) {
    if (!pp::map_shape_ok(n_groups, n_per_a, n_per_b, n_cols)) return 0;
    pp::MapWorkspace w;
    pp::map_carve(n_groups, n_per_a, n_per_b, n_cols, nullptr, w);
    return w.bytes;
}

int pp_is_sinkhorn_map_groups(const float* lw_a, const float* const* cols_a, const double* stats_a, int32_t n_per_a, const float* lw_b,
                              const float* const* cols_b, const double* stats_b, int32_t n_per_b, int32_t n_cols, int32_t n_groups,
                              const double* center, const double* inv_scale, const double* epsilon, const double* f, const double* g,
                              double* map_ab, double* map_ba, double* log_mass_a, double* log_mass_b, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return pp::is_sinkhorn_map_groups(lw_a, cols_a, stats_a, n_per_a, lw_b, cols_b, stats_b, n_per_b, n_cols, n_groups, center, inv_scale,
                                      epsilon, f, g, map_ab, map_ba, log_mass_a, log_mass_b, workspace, workspace_bytes,
                                      pp::as_stream(stream));
}

}  // extern "C"
