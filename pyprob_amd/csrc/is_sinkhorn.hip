// The entropic optimal-transport cost between the JOINT particles of two lock-step posteriors and its debiased form, the Sinkhorn
// divergence (Empirical.sinkhorn). The reference has no distance between two Empiricals. include/pyprob_amd.h states the definition:
// three problems per pair of particle sets - (a, b) with the potentials f, g and the symmetric (a, a), (b, b) with one potential p each
// - iterated in the log domain. One half-step is, per particle j of one side ("query"), a log-sum-exp over the particles i of the
// other ("summed") side:
//     new_j = -eps (log sum_i exp2(E_ij) - log W),   E_ij = log2(e) (lw_i - max + pot_i / eps) - alpha^2 |z_i - z'_j|^2 / 2
// with alpha^2 = log2(e) / eps: the shape is_kde_joint.hip evaluates with eps = h^2, plus the potential. Nothing of size n_a x n_b is
// stored: a half-step keeps (m, sum) per (strip, query), the potentials are O(n_a + n_b).
//
// WHAT IS STORED (workspace, per side s and group): the image of is_pair_image.hpp, feature-major [K][n_pad] = (alpha z, 0.., q, 1), whose
// q row belongs to the potential of problem (a, b) on that side (f on a, g on b); a second q column for the side's symmetric problem;
// the query column nq = fp32(-alpha^2 |z|^2 / 2); in fp64 base = log2(e) (lw - max) - alpha^2 |z|^2 / 2 (-inf where the particle does
// not count), the weight exp(lw - max) and the four potentials f, g, p_a, p_b. A q column is fp32(base + log2(e) pot / eps): formed in
// fp64, ONE rounding. The coordinates are written once; a new potential rewrites its q column and nothing else.
//
// LAUNCHES, dependent on the caller's stream, no atomics, no workgroup waits for another.
// 1. OPERANDS (sink_operand_kernel<J>, once per side): the rule and the arithmetic of pairs_operand_kernel with alpha from eps, the
//    columns above at potential 0, and per 2048 particles (sum w, sum w^2, count) in fp64.
// 2. Per iteration two HALF-STEPS. The first carries three jobs per group on grid dimension z - the g update (summed a under f, queries
//    b), the (a, a) and the (b, b) update - the second the f update (summed b under the new g, queries a).
//    MAIN (sink_main_kernel<K / 2>): a workgroup of four waves owns QTILE = 128 queries - any number of tiles on grid dimension x - and
//    ONE strip of the summed side, staged through LDS in chunks of 256 (global -> registers one chunk ahead -> LDS). The SAME image
//    serves as rows here and as columns in the next half-step: the query fragment (alpha z_q, 0.., 1, nq_q) is built in registers from
//    the coordinate rows and nq - the (.., q, 1) / (.., 1, q') swap costs nothing - and the staged rows are (alpha z_i, 0.., q_i, 1)
//    with the ones written to LDS once. Per 32-particle block a wave takes the 32 x 32 exponents from K / 2 v_mfma_f32_32x32x2_f32
//    (particles as rows, queries as columns: a lane holds 16 particles of ONE query), raises the INTEGER running maximum m of its
//    query (per-lane maximum of the 16, one exchange with the partner half-wave, ceil; what was summed under the old m is rescaled by
//    v_ldexp_f32 - exact - in the blocks where some lane's m rose), takes p = v_exp_f32(E - m) in (0, 1] and adds a tree of 15
//    additions to the lane's fp32 sum; every chunk (128 terms per lane) the fp32 sum is flushed to fp64 under the same m. The strip
//    stores (m, sum) per query. The strips of a job are a function of (n_summed, n_query) alone (sink_split: about 1024 workgroups per
//    job, at most 16 strips).
//    UPDATE (sink_update_kernel, a thread per query): the strips in strip order under the largest m (ldexp, exact), T = -eps (ln 2 m +
//    log sum - log W), the new potential (T, or (old + T) / 2 for a symmetric problem), its q column, and the workgroup's maximum of
//    |new - old| (one double per workgroup).
// 3. FOLD (sink_fold_kernel, a workgroup per problem): residual = the maximum over the update workgroups / eps, the iteration count, and
//    the problem is FROZEN where residual < tol: the main and update workgroups of a frozen problem return at once, so its potentials
//    never move again and nothing depends on check_every, the interval at which one more workgroup folds the flags into the word the
//    host reads (pp_is_gmm_groups' scheme).
// 4. FINISH (a workgroup per group): the costs as fp64 sums in a fixed order (a thread's particles in index order, block_sum), the row
//    of 12 and the copies of the potentials.
// The order of every sum is a function of (n_a, n_b, J) alone: two calls give the same bits, and group g of an M-group call gives the
// bits of its own one-group call.
//
// WHICH PIPE BOUNDS A HALF-STEP. Per 32 x 32 block a wave issues K / 2 MFMAs of 16 passes (64 cycles each: 320 cycles at J = 8, 128 at
// J <= 2) against 16 v_exp_f32 (quarter rate, 16 cycles each: 256 cycles) and about 70 full-rate VALU operations (16 subtractions, the
// two trees of 15, the copies out of the accumulator, the exchange: some 280 cycles): the VALU carries 540 cycles per block at every J,
// the matrix pipe at most 320, so v_exp_f32 and its companions bound the half-step and the matrix pipe idles 40 % (J = 8) to 75 %
// (J <= 2) of the time. There is no second product here, unlike mean shift. At small n the iteration is five dependent launches of
// a few microseconds each and launch latency dominates. The measured fractions are in profiles/sinkhorn_bench.json where recorded.
//
// RESOURCES (gfx950, hipcc -O3; the build fails if the main kernel uses scratch): recorded in DESIGN.md section 4.3.
//
// ERROR (what tests/test_gpu_sinkhorn.py holds every potential and cost to; u = 2^-24). ONE EVALUATION. With N = alpha^2 |z_i|^2, N' =
// alpha^2 |z_q|^2, P <= sqrt(N N'), L = log2(e) |lw_i - max|, F = log2(e) |pot_i| / eps and S = P + N + N' + L + F the exponent of a
// pair is off, as in is_kde_joint.hip, by at most (2 K + 9) S u (the fp32 roundings of z, alpha z, q and nq; K products and K additions
// inside the MFMA at 2 u each), and E - m (|m| <= S + 1) rounds once more: (2 K + 12) S u. With R_s, R_q the largest |z| of the summed
// and the query side, L_max the largest L and F_max the largest F of the summed side:
//   e = expm1(ln 2 (2 K + 12) (alpha^2 (R_s^2 + R_q^2 + R_s R_q) + L_max + F_max) u)     the expanded square and the potential in q
//     + 650 u                                                                            v_exp_f32 (2 u), the fp32 sums
//     + (n + 64) 2^-52 + n 2^-124                                                        fp64 sums, log W; terms below 2^-126
//   |log sum - exact| <= d = -log1p(-e), so T is off by at most eps d GIVEN the potential it read.
// ITERATION. The soft minimum pot -> T(pot) is 1-Lipschitz in the sup norm, so an error delta of the potential read comes out as at most
// delta: a half-step adds eps d, and after t half-steps of problem (a, b) |f - exact|, |g - exact| <= t eps d (t = 2 iterations at
// the end of an iteration for f, one less for g). The averaged update gives (delta + delta + eps d) / 2 = delta + eps d / 2 per
// iteration: |p - exact| <= iterations eps d / 2. d is taken at the largest F_max over the iterations. The costs are convex
// combinations (sum a = sum b = 1; the weights are fp64 on both routes, their relative error c = (n + 64) 2^-52):
//   |ot_ab - exact| <= err(f) + err(g) + c (max |f| + max |g|),   |ot_aa - exact| <= 2 err(p) + 2 c max |p|.
// The residual of an iteration inherits 2 t d from its two potentials: n_iter may differ from the float64 route's by the iterations
// whose residual lies that close to tol; the test compares at tol = 0.
#include "is_pair_image.hpp"

namespace pp {
namespace {

constexpr int QBLOCK = PP_IS_SINKHORN_QUERY_BLOCK, QTILE = PP_IS_SINKHORN_QUERY_TILE, PBLOCK = PP_IS_SINKHORN_PARTICLE_BLOCK;
constexpr int MAX_STRIPS = PP_IS_SINKHORN_MAX_STRIPS, TARGET_WG = PP_IS_SINKHORN_TARGET_WORKGROUPS, WIDTH = PP_IS_SINKHORN_WIDTH;
constexpr int STRIDE = CHUNK + 32;         // LDS row stride: the two half-waves of a fragment read fall into different banks
constexpr float M_NONE = -3.0e38f;         // the reference before the first finite exponent
constexpr int JOBS = 4, PROBLEMS = 3;      // jobs: 0 g update, 1 (a, a), 2 (b, b), 3 f update; problems: 0 ab, 1 aa, 2 bb
static_assert(QBLOCK == 32 && PBLOCK == 32 && QTILE == QBLOCK * (THREADS / 64) && CHUNK == PP_IS_SINKHORN_CHUNK && CHUNK % PBLOCK == 0 &&
                  CHUNK % QTILE == 0 && MAXJ == PP_IS_SINKHORN_MAX_J && 3 * PP_IS_SINKHORN_MAX_GROUPS <= 65535,
              "tiling");

struct Split {
    int QT, chunks, per_strip, S;
    int64_t q_pad;
};
__host__ __device__ inline Split sink_split(int n_sum, int n_query) {
    Split s;
    s.QT = ceil_div(n_query, QTILE);
    s.q_pad = (int64_t)s.QT * QTILE;
    s.chunks = ceil_div(n_sum, CHUNK);
    const int want = min(MAX_STRIPS, max(1, ceil_div(TARGET_WG, s.QT)));
    s.per_strip = ceil_div(s.chunks, want);
    s.S = ceil_div(s.chunks, s.per_strip);
    return s;
}

// A half-step job: which side is summed, which side's particles are the queries, whose problem it is.
struct Job {
    int sum_side, q_side, prob, n_s, n_q;
};
__host__ __device__ inline Job job_of(int j, int na, int nb) {
    Job r;
    r.sum_side = (j == 2 || j == 3) ? 1 : 0;
    r.q_side = (j == 0 || j == 2) ? 1 : 0;
    r.prob = j == 3 ? 0 : j;
    r.n_s = r.sum_side ? nb : na;
    r.n_q = r.q_side ? nb : na;
    return r;
}
// Doubles of one (group, job slot) region of the partials: the largest S 2 q_pad of the four jobs.
inline int64_t partial_region(int na, int nb) {
    int64_t r = 0;
    for (int j = 0; j < JOBS; ++j) {
        const Job job = job_of(j, na, nb);
        const Split s = sink_split(job.n_s, job.n_q);
        r = std::max(r, (int64_t)s.S * 2 * s.q_pad);
    }
    return r;
}

// What the kernels read and write, per side [2]: see the head comment. pot: f, g, p_a, p_b, [M][n_pad of its side].
struct SinkDev {
    float *img0, *img1, *qself0, *qself1, *nq0, *nq1;
    double *base0, *base1, *wgt0, *wgt1, *pot0, *pot1, *pot2, *pot3, *wsum0, *wsum1;
    double *partial, *wgmax, *resid;
    int32_t *state, *n_iter, *all_done;
    const double* eps;
    int na, nb, J, NB;
    int64_t region;
};
struct SinkWorkspace {
    SinkDev d;
    float* tmax[2];
    size_t bytes;
};
void sink_carve(int M, int na, int nb, int J, void* p, SinkWorkspace& w) {
    Carver c(p);
    const int64_t m = std::max(M, 0);
    na = std::max(na, 1);
    nb = std::max(nb, 1);
    const int64_t pa = m * pad_of(na), pb = m * pad_of(nb);
    SinkDev& d = w.d;
    d.img0 = c.take<float>(pa * image_k(J) * 4);
    d.img1 = c.take<float>(pb * image_k(J) * 4);
    d.qself0 = c.take<float>(pa * 4);
    d.qself1 = c.take<float>(pb * 4);
    d.nq0 = c.take<float>(pa * 4);
    d.nq1 = c.take<float>(pb * 4);
    d.base0 = c.take<double>(pa * 8);
    d.base1 = c.take<double>(pb * 8);
    d.wgt0 = c.take<double>(pa * 8);
    d.wgt1 = c.take<double>(pb * 8);
    d.pot0 = c.take<double>(pa * 8);
    d.pot1 = c.take<double>(pb * 8);
    d.pot2 = c.take<double>(pa * 8);
    d.pot3 = c.take<double>(pb * 8);
    d.wsum0 = c.take<double>(m * tiles_of(na, OP_TILE) * 3 * 8);
    d.wsum1 = c.take<double>(m * tiles_of(nb, OP_TILE) * 3 * 8);
    w.tmax[0] = c.take<float>(m * tiles_of(na, OP_TILE) * 4);
    w.tmax[1] = c.take<float>(m * tiles_of(nb, OP_TILE) * 4);
    d.na = na;
    d.nb = nb;
    d.J = J;
    d.NB = ceil_div(std::max(na, nb), THREADS);
    d.region = partial_region(na, nb);
    d.partial = c.take<double>(m * PROBLEMS * d.region * 8);
    d.wgmax = c.take<double>(m * JOBS * d.NB * 8);
    d.resid = c.take<double>(m * PROBLEMS * 8);
    d.state = c.take<int32_t>(m * PROBLEMS * 4);
    d.n_iter = c.take<int32_t>(m * PROBLEMS * 4);
    d.all_done = c.take<int32_t>(4);
    d.eps = nullptr;
    w.bytes = c.bytes();
}
bool sink_shape_ok(int M, int na, int nb, int J) {
    return J >= 1 && J <= MAXJ && M <= PP_IS_SINKHORN_MAX_GROUPS && groups_shape_ok(M, na) && groups_shape_ok(M, nb);
}

// ---- 1. operands ------------------------------------------------------------------------------------------------------------------
// Workgroup (tile blockIdx.x, group blockIdx.y) of one side: pairs_operand_kernel's particles, rule and arithmetic with alpha^2 =
// log2(e) / eps; the q columns at potential 0, nq, base, the weight and the side's two potentials (0, NaN where not counted).
template <int J>
__global__ __launch_bounds__(THREADS) void sink_operand_kernel(const float* __restrict__ lw, PairCols cols, int n_per, int T,
                                                               const double* __restrict__ center, const double* __restrict__ inv_scale,
                                                               const double* __restrict__ eps, const double* __restrict__ stats,
                                                               const float* __restrict__ tmax, float* __restrict__ img,
                                                               float* __restrict__ qself, float* __restrict__ nq, double* __restrict__ base_,
                                                               double* __restrict__ wgt, double* __restrict__ pot_ab,
                                                               double* __restrict__ pot_self, double* __restrict__ wsum) {
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
        for (int j = 0; j < J; ++j) gi[j * pad + i] = ok ? (float)(alpha * (double)z[j]) : 0.0f;
#pragma unroll
        for (int f = J; f < K - 2; ++f) gi[f * pad + i] = 0.0f;
        const double b = ok ? LOG2E * ((double)a[k] - M) - half_alpha2 * r2 : -INFINITY;
        gi[(K - 2) * pad + i] = (float)b;
        gi[(K - 1) * pad + i] = 1.0f;
        qself[g * pad + i] = (float)b;
        nq[g * pad + i] = ok ? (float)(-half_alpha2 * r2) : 0.0f;
        base_[g * pad + i] = b;
        wgt[g * pad + i] = w;
        pot_ab[g * pad + i] = ok ? 0.0 : NAN;
        pot_self[g * pad + i] = ok ? 0.0 : NAN;
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

// One thread: every problem open, nothing counted yet.
__global__ __launch_bounds__(256) void sink_reset_kernel(int64_t problems, int32_t* __restrict__ state, int32_t* __restrict__ n_iter,
                                                         double* __restrict__ resid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= problems) return;
    state[i] = 0;
    n_iter[i] = 0;
    resid[i] = NAN;
}

// ---- 2. half-step: main -----------------------------------------------------------------------------------------------------------
// Workgroup (query tile blockIdx.x, strip blockIdx.y, job and group on blockIdx.z: phase 0 carries the jobs 0 .. 2 of a group, phase 1
// job 3). A workgroup beyond its job's tiles or strips, or of a frozen problem, returns.
template <int K2>
__global__ __launch_bounds__(THREADS) void sink_main_kernel(SinkDev d, int phase) {
    constexpr int K = 2 * K2;
    __shared__ __attribute__((aligned(16))) float sh[K * STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, c31 = lane & 31, hh = lane >> 5;
    const int nj = phase ? 1 : 3;
    const int j = phase ? 3 : (int)(blockIdx.z % 3);
    const int64_t g = blockIdx.z / nj;
    const Job job = job_of(j, d.na, d.nb);
    if (d.state[g * PROBLEMS + job.prob] != 0) return;
    const Split sp = sink_split(job.n_s, job.n_q);
    if ((int)blockIdx.x >= sp.QT || (int)blockIdx.y >= sp.S) return;
    const int64_t pad_s = pad_of(job.n_s), pad_q = pad_of(job.n_q);
    const float* I = (job.sum_side ? d.img1 : d.img0) + g * K * pad_s;
    const float* qc = (j == 1 || j == 2) ? (job.sum_side ? d.qself1 : d.qself0) + g * pad_s : I + (K - 2) * pad_s;
    const float* Q = (job.q_side ? d.img1 : d.img0) + g * K * pad_q;
    const float* NQ = (job.q_side ? d.nq1 : d.nq0) + g * pad_q;
    const int c_lo = blockIdx.y * sp.per_strip, c_hi = min(sp.chunks, c_lo + sp.per_strip);
    const int q = blockIdx.x * QTILE + (tid >> 6) * QBLOCK + c31;      // (< q_pad <= pad_q: the padding's image is zeros)

    // the query's image as a COLUMN, from the rows of the same image: (alpha z_q, 0.., 1, nq_q); this lane keeps the features 2 s + hh
    float bq[K2];
#pragma unroll
    for (int s = 0; s < K2 - 1; ++s) bq[s] = Q[(2 * s + hh) * pad_q + q];
    bq[K2 - 1] = hh ? NQ[q] : 1.0f;

    float nx[K - 1];
    auto load = [&](int c) {
#pragma unroll
        for (int f = 0; f < K - 2; ++f) nx[f] = I[f * pad_s + (int64_t)c * CHUNK + tid];
        nx[K - 2] = qc[(int64_t)c * CHUNK + tid];
    };
    sh[(K - 1) * STRIDE + tid] = 1.0f;      // (the row of ones: written once, the staging below leaves it alone)
    float m = M_NONE, m64 = M_NONE, s32 = 0.0f;
    double S64 = 0.0;
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
                s32 = ldexpf(s32, (int)fmaxf(m - mn, -2000.0f));
                m = mn;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = __builtin_amdgcn_exp2f(e[r] - m);
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int r = 0; r < w; ++r) t[r] += t[r + w];
            s32 += t[0];
        }
        // the chunk's fp32 sum to fp64, under the same integer reference
        S64 = ldexp(S64, (int)fmaxf(m64 - m, -2000.0f)) + (double)s32;
        s32 = 0.0f;
        m64 = m;
    }
    const double S_all = S64 + __shfl_xor(S64, 32, 64);      // (the two halves hold the two halves of every block's particles)
    if (q >= job.n_q || hh) return;
    double* o = d.partial + (g * PROBLEMS + job.prob) * d.region + (int64_t)blockIdx.y * 2 * sp.q_pad + q;
    o[0] = (double)m;
    o[sp.q_pad] = S_all;
}

// The workgroup's maximum of v (a maximum does not depend on its order). sh: 4 doubles.
__device__ __forceinline__ double block_max_f64(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// ---- 2. half-step: update ---------------------------------------------------------------------------------------------------------
// Workgroup (256 queries blockIdx.x, job blockIdx.y of the phase, group blockIdx.z): the new potential of its queries, their q column
// and wgmax[(g JOBS + job) NB + blockIdx.x] = the largest |new - old| (+inf where a new potential is not a number).
__global__ __launch_bounds__(THREADS) void sink_update_kernel(SinkDev d, int phase) {
    __shared__ double shsum[THREADS / 64];
    const int j = phase ? 3 : (int)blockIdx.y;
    const int64_t g = blockIdx.z;
    const Job job = job_of(j, d.na, d.nb);
    if (d.state[g * PROBLEMS + job.prob] != 0) return;
    const int q = blockIdx.x * THREADS + threadIdx.x;
    if ((int)blockIdx.x * THREADS >= job.n_q) return;
    const Split sp = sink_split(job.n_s, job.n_q);
    const int T = ceil_div(job.n_s, OP_TILE);
    const double* wsum = job.sum_side ? d.wsum1 : d.wsum0;
    double W = 0.0, cnt = 0.0;
    for (int t = threadIdx.x; t < T; t += THREADS) {
        W += wsum[(g * T + t) * 3];
        cnt += wsum[(g * T + t) * 3 + 2];
    }
    W = block_sum(W, shsum);
    cnt = block_sum(cnt, shsum);
    double diff = 0.0;
    if (q < job.n_q) {
        const int64_t pad_q = pad_of(job.n_q), at = g * pad_q + q;
        const double b = (job.q_side ? d.base1 : d.base0)[at];
        if (b > -INFINITY) {
            const double* p = d.partial + (g * PROBLEMS + job.prob) * d.region + q;
            const int64_t strip = 2 * sp.q_pad;
            double m = (double)M_NONE;
            for (int s = 0; s < sp.S; ++s) m = fmax(m, p[s * strip]);
            double S = 0.0;
            for (int s = 0; s < sp.S; ++s) S += ldexp(p[s * strip + sp.q_pad], (int)fmax(p[s * strip] - m, -2000.0));
            const double e = d.eps[g];
            const double t = -e * ((0.6931471805599453 * m + log(S)) - log(W));
            double* pot = j == 0 ? d.pot1 : j == 1 ? d.pot2 : j == 2 ? d.pot3 : d.pot0;
            float* qcol = j == 0   ? d.img1 + (g * image_k(d.J) + image_k(d.J) - 2) * pad_q
                          : j == 3 ? d.img0 + (g * image_k(d.J) + image_k(d.J) - 2) * pad_q
                          : j == 1 ? d.qself0 + g * pad_q
                                   : d.qself1 + g * pad_q;
            const double old = pot[at];
            double nw = (j == 1 || j == 2) ? 0.5 * (old + t) : t;
            if (!(cnt > 0.0)) nw = NAN;
            pot[at] = nw;
            qcol[q] = (float)(b + LOG2E * nw / e);
            diff = nw == nw ? fabs(nw - old) : INFINITY;
        }
    }
    diff = block_max_f64(diff, shsum);
    if (threadIdx.x == 0) d.wgmax[(g * JOBS + j) * d.NB + blockIdx.x] = diff;
}

// ---- 3. fold ----------------------------------------------------------------------------------------------------------------------
// Workgroup (problem blockIdx.x, group blockIdx.y): the residual of the iteration, and the problem freezes where it is below tol
// (state 1) or not finite (state 2: a side without a counted particle).
__global__ __launch_bounds__(THREADS) void sink_fold_kernel(SinkDev d, int iter, double tol) {
    __shared__ double shsum[THREADS / 64];
    const int prob = blockIdx.x;
    const int64_t g = blockIdx.y, at = g * PROBLEMS + prob;
    if (d.state[at] != 0) return;
    double v = 0.0;
    for (int j = 0; j < JOBS; ++j) {
        const Job job = job_of(j, d.na, d.nb);
        if (job.prob != prob) continue;
        const int nblk = ceil_div(job.n_q, THREADS);
        for (int t = threadIdx.x; t < nblk; t += THREADS) v = fmax(v, d.wgmax[(g * JOBS + j) * d.NB + t]);
    }
    v = block_max_f64(v, shsum);
    if (threadIdx.x != 0) return;
    const double r = v / d.eps[g];
    d.resid[at] = r;
    d.n_iter[at] = iter;
    if (!(r < INFINITY))
        d.state[at] = 2;
    else if (r < tol)
        d.state[at] = 1;
}

// One workgroup: *all_done = no problem is open.
__global__ __launch_bounds__(256) void sink_done_kernel(const int32_t* __restrict__ state, int64_t problems, int32_t* __restrict__ out) {
    __shared__ int open[4];
    int mine = 0;
    for (int64_t i = threadIdx.x; i < problems; i += 256) mine |= state[i] == 0;
    const int w = __any(mine);
    if ((threadIdx.x & 63) == 0) open[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) *out = !(open[0] | open[1] | open[2] | open[3]);
}

// ---- 4. finish --------------------------------------------------------------------------------------------------------------------
// sum_i w_i pot_i over the counted particles of a side in a fixed order (a thread's particles in index order, then block_sum).
__device__ __forceinline__ double weighted_sum(const double* __restrict__ wgt, const double* __restrict__ pot, int n, double* sh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const double p = pot[i];
        if (p == p) s += wgt[i] * p;
    }
    return block_sum(s, sh);
}
__device__ __forceinline__ double tiles_sum(const double* __restrict__ wsum, int64_t g, int n, int slot, double* sh) {
    const int T = ceil_div(n, OP_TILE);
    double s = 0.0;
    for (int t = threadIdx.x; t < T; t += THREADS) s += wsum[(g * T + t) * 3 + slot];
    return block_sum(s, sh);
}
// Workgroup per group: the row of 12 and the copies of the potentials that were asked for.
__global__ __launch_bounds__(THREADS) void sink_finish_kernel(SinkDev d, double* __restrict__ out, double* __restrict__ f,
                                                              double* __restrict__ gg, double* __restrict__ p_a,
                                                              double* __restrict__ p_b) {
    __shared__ double shsum[THREADS / 64];
    const int64_t g = blockIdx.x, pa = pad_of(d.na), pb = pad_of(d.nb);
    const double Wa = tiles_sum(d.wsum0, g, d.na, 0, shsum), Wb = tiles_sum(d.wsum1, g, d.nb, 0, shsum);
    const double ca = tiles_sum(d.wsum0, g, d.na, 2, shsum), cb = tiles_sum(d.wsum1, g, d.nb, 2, shsum);
    const double sf = weighted_sum(d.wgt0 + g * pa, d.pot0 + g * pa, d.na, shsum);
    const double sg = weighted_sum(d.wgt1 + g * pb, d.pot1 + g * pb, d.nb, shsum);
    const double sa = weighted_sum(d.wgt0 + g * pa, d.pot2 + g * pa, d.na, shsum);
    const double sb = weighted_sum(d.wgt1 + g * pb, d.pot3 + g * pb, d.nb, shsum);
    if (f)
        for (int i = threadIdx.x; i < d.na; i += THREADS) f[g * d.na + i] = d.pot0[g * pa + i];
    if (gg)
        for (int i = threadIdx.x; i < d.nb; i += THREADS) gg[g * d.nb + i] = d.pot1[g * pb + i];
    if (p_a)
        for (int i = threadIdx.x; i < d.na; i += THREADS) p_a[g * d.na + i] = d.pot2[g * pa + i];
    if (p_b)
        for (int i = threadIdx.x; i < d.nb; i += THREADS) p_b[g * d.nb + i] = d.pot3[g * pb + i];
    if (threadIdx.x != 0) return;
    const bool empty = !(ca > 0.0 && cb > 0.0);
    double* o = out + g * WIDTH;
    o[0] = empty ? NAN : sf / Wa + sg / Wb;
    o[1] = empty ? NAN : 2.0 * (sa / Wa);
    o[2] = empty ? NAN : 2.0 * (sb / Wb);
    int status = empty ? 8 : 0;
    for (int p = 0; p < PROBLEMS; ++p) {
        o[3 + p] = (double)d.n_iter[g * PROBLEMS + p];
        o[6 + p] = empty ? NAN : d.resid[g * PROBLEMS + p];
        if (d.state[g * PROBLEMS + p] == 0) status |= 1 << p;
    }
    o[9] = ca;
    o[10] = cb;
    o[11] = (double)status;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct SinkSide {
    const float* lw;
    PairCols cols;
    const double* stats;
    int n_per;
};

template <int J>
void launch_operands(hipStream_t st, const SinkSide (&side)[2], int M, const double* center, const double* inv_scale, const double* eps,
                     const SinkWorkspace& w) {
    const SinkDev& d = w.d;
    for (int s = 0; s < 2; ++s) {
        const int T = tiles_of(side[s].n_per, OP_TILE);
        if (T > 1 && !side[s].stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, M), dim3(256), 0, st, side[s].lw, side[s].n_per, OP_TILE, T, 0, w.tmax[s]);
        hipLaunchKernelGGL(sink_operand_kernel<J>, dim3(T, M), dim3(THREADS), 0, st, side[s].lw, side[s].cols, side[s].n_per, T, center,
                           inv_scale, eps, side[s].stats, (const float*)w.tmax[s], s ? d.img1 : d.img0, s ? d.qself1 : d.qself0,
                           s ? d.nq1 : d.nq0, s ? d.base1 : d.base0, s ? d.wgt1 : d.wgt0, s ? d.pot1 : d.pot0, s ? d.pot3 : d.pot2,
                           s ? d.wsum1 : d.wsum0);
    }
}

template <int K2>
void launch_main(hipStream_t st, const SinkDev& d, int M, int phase) {
    int QT = 0, S = 0;
    for (int j = phase ? 3 : 0; j < (phase ? 4 : 3); ++j) {
        const Job job = job_of(j, d.na, d.nb);
        const Split sp = sink_split(job.n_s, job.n_q);
        QT = std::max(QT, sp.QT);
        S = std::max(S, sp.S);
    }
    hipLaunchKernelGGL(sink_main_kernel<K2>, dim3(QT, S, (phase ? 1 : 3) * M), dim3(THREADS), 0, st, d, phase);
}
void sink_half_step(hipStream_t st, const SinkDev& d, int M, int phase) {
    switch (image_k(d.J) / 2) {
        case 2: launch_main<2>(st, d, M, phase); break;
        case 3: launch_main<3>(st, d, M, phase); break;
        case 4: launch_main<4>(st, d, M, phase); break;
        default: launch_main<5>(st, d, M, phase); break;
    }
    const int nq = phase ? d.na : std::max(d.na, d.nb);
    hipLaunchKernelGGL(sink_update_kernel, dim3(ceil_div(nq, THREADS), phase ? 1 : 3, M), dim3(THREADS), 0, st, d, phase);
}

}  // namespace

int is_sinkhorn_groups(const float* lw_a, const float* const* cols_a, const double* stats_a, int na, const float* lw_b,
                       const float* const* cols_b, const double* stats_b, int nb, int J, int M, const double* center,
                       const double* inv_scale, const double* eps, double tol, int max_iter, int check_every, double* out, double* f,
                       double* g, double* p_a, double* p_b, void* ws, size_t ws_bytes, hipStream_t st) {
    const char* name = "pp_is_sinkhorn_groups";
    PP_CHECK_ARG(lw_a && cols_a && lw_b && cols_b && center && inv_scale && eps && out && ws,
                 "%s: null pointer (only stats_a, stats_b and the potentials' outputs may be null)", name);
    PP_CHECK_ARG(J >= 1 && J <= MAXJ, "%s: n_cols in 1 .. %d", name, MAXJ);
    PP_CHECK_ARG(na >= 1 && nb >= 1 && M >= 0 && M <= PP_IS_SINKHORN_MAX_GROUPS, "%s: n_per_a, n_per_b >= 1 and n_groups in 0 .. %d", name,
                 PP_IS_SINKHORN_MAX_GROUPS);
    PP_CHECK_ARG(groups_count_ok(M, na) && groups_count_ok(M, nb), "%s: more than 2^31 - 1 particles per call: shard the groups", name);
    PP_CHECK_ARG(max_iter >= 1 && tol >= 0.0, "%s: max_iter >= 1 and tol >= 0", name);
    SinkSide side[2] = {{lw_a, {}, stats_a, na}, {lw_b, {}, stats_b, nb}};
    for (int j = 0; j < MAXJ; ++j) {
        side[0].cols.p[j] = j < J ? cols_a[j] : nullptr;
        side[1].cols.p[j] = j < J ? cols_b[j] : nullptr;
        PP_CHECK_ARG(j >= J || (cols_a[j] && cols_b[j]), "%s: null column pointer %d", name, j);
    }
    SinkWorkspace w;
    sink_carve(M, na, nb, J, ws, w);
    PP_CHECK_WORKSPACE("pp_is_sinkhorn_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    if (check_every < 1) check_every = 8;
    w.d.eps = eps;
    const SinkDev& d = w.d;
    const int64_t problems = (int64_t)M * PROBLEMS;
    switch (J) {
        case 1: launch_operands<1>(st, side, M, center, inv_scale, eps, w); break;
        case 2: launch_operands<2>(st, side, M, center, inv_scale, eps, w); break;
        case 3: launch_operands<3>(st, side, M, center, inv_scale, eps, w); break;
        case 4: launch_operands<4>(st, side, M, center, inv_scale, eps, w); break;
        case 5: launch_operands<5>(st, side, M, center, inv_scale, eps, w); break;
        case 6: launch_operands<6>(st, side, M, center, inv_scale, eps, w); break;
        case 7: launch_operands<7>(st, side, M, center, inv_scale, eps, w); break;
        default: launch_operands<8>(st, side, M, center, inv_scale, eps, w); break;
    }
    hipLaunchKernelGGL(sink_reset_kernel, dim3(cdiv(problems, 256)), dim3(256), 0, st, problems, d.state, d.n_iter, d.resid);
    for (int iter = 1; iter <= max_iter; ++iter) {
        sink_half_step(st, d, M, 0);
        sink_half_step(st, d, M, 1);
        hipLaunchKernelGGL(sink_fold_kernel, dim3(PROBLEMS, M), dim3(THREADS), 0, st, d, iter, tol);
        if (iter % check_every == 0 && iter < max_iter) {
            int done = 0;
            hipLaunchKernelGGL(sink_done_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)d.state, problems, d.all_done);
            PP_LAUNCH_CHECK(name);
            hipError_t e = hipMemcpyAsync(&done, d.all_done, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                set_error("%s: reading the converged word failed: %s", name, hipGetErrorString(e));
                return (int)e;
            }
            if (done) break;
        }
    }
    hipLaunchKernelGGL(sink_finish_kernel, dim3(M), dim3(THREADS), 0, st, d, out, f, g, p_a, p_b);
    PP_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_sinkhorn_workspace_bytes(int32_t n_groups, int32_t n_per_a, int32_t n_per_b, int32_t n_cols) {
    if (!pp::sink_shape_ok(n_groups, n_per_a, n_per_b, n_cols)) return 0;
    pp::SinkWorkspace w;
    pp::sink_carve(n_groups, n_per_a, n_per_b, n_cols, nullptr, w);
    return w.bytes;
}

int32_t pp_is_sinkhorn_strips(int32_t n_sum, int32_t n_query) {
    if (n_sum < 1 || n_query < 1) return 0;
    return pp::sink_split(n_sum, n_query).S;
}

int pp_is_sinkhorn_groups(const float* lw_a, const float* const* cols_a, const double* stats_a, int32_t n_per_a, const float* lw_b,
                          const float* const* cols_b, const double* stats_b, int32_t n_per_b, int32_t n_cols, int32_t n_groups,
                          const double* center, const double* inv_scale, const double* epsilon, double tol, int32_t max_iter,
                          int32_t check_every, double* out, double* f, double* g, double* p_a, double* p_b, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return pp::is_sinkhorn_groups(lw_a, cols_a, stats_a, n_per_a, lw_b, cols_b, stats_b, n_per_b, n_cols, n_groups, center, inv_scale,
                                  epsilon, tol, max_iter, check_every, out, f, g, p_a, p_b, workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
