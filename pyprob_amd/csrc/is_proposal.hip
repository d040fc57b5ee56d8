// Draws from, and the density of, a fitted mixture of K full-covariance Gaussians over J latents (the rows pp_is_gmm_joint_groups
// writes) on the device: the proposal of the NEXT importance-sampling call. The reference has no counterpart.
//   pp_is_proposal_groups  mode 0 (draw): J columns of fp32 draws x_i ~ q_g = sum_k pi_k N(mu_k, Sigma_k) and -log q_g(x_i) for the n_per
//   particles of each of M groups; mode 1 (score): -log q_g at the caller's columns. 1 <= J <= 8, 1 <= K <= 16.
//
// SHAPE OF THE WORK: two dependent launches on the caller's stream.
//   prepare kernel   One workgroup of 64 threads per group, thread k: component k. The weights are normalised (added in the order of
//                    k by one thread), Sigma_k = L_k L_k^T is factorised in fp64 (gmm_factor.hpp: the factorisation of the EM, its
//                    run-time indices in LDS - nothing in scratch) and the group's BLOCK goes to the workspace: per component
//                    mu_k [J] | L_k^-1 packed | c_k = log pi_k - sum_j log L_k,jj - J/2 log 2 pi | L_k packed, then the K cumulative
//                    weights and a word that says the group is bad. K (J + J (J + 1) + 1) + K + 1 doubles: 10504 bytes at J = 8,
//                    K = 16. A weight that is not positive and finite, or a pivot that is not positive (a NaN included), makes the
//                    group bad: status[g] = 1 + the first such component, else 0.
//   particle kernel  Compiled per J. A workgroup of 256 threads takes one tile of 2048 particles of one group and copies the block to
//                    LDS once. A thread holds its eight particles (256 apart: the columns are read and written coalesced), J floats
//                    each, in registers.
//                    DRAW. Philox4x32-10 with key = seed, counter = offset + g n_per + i and stream id PROPOSAL_STREAM gives the
//                    particle 1 + 2 ceil(J / 2) words: word 0 picks the component - the first k whose cumulative weight exceeds
//                    the uniform -, each following pair gives two standard normals (Box-Muller, both branches). x = mu_k + L_k z is
//                    a packed triangular product in fp64 whose operands the lane reads from LDS at ITS component; the result is
//                    ROUNDED TO fp32 - the value the program sees and the statement log keeps.
//                    DENSITY, both modes, at that fp32 value: components outermost (every lane reads the same LDS address: a
//                    broadcast), y = L_c^-1 (x - mu_c) as J (J + 1) / 2 FMAs, a running logsumexp of c_c - |y|^2 / 2 with ONE exp per
//                    (particle, component), one log at the end, ONE rounding to fp32.
//                    The difference form x - mu_c keeps a narrow component far from the origin (|x|^2 - 2 x mu + mu^2 would cancel
//                    at 1e6 / sigma^2), so this is fp64 VALU work: the fp64 matrix instructions would need the expanded square.
// No atomics, no workgroup waits for another, no dynamically indexed private array (the build fails on scratch memory).
// A particle's outputs are a function of (seed, offset + g n_per + i, the group's row) alone: not of M, of the tile, or of how a call
// is split. A bad group's outputs are NaN; no NaN reaches another group.
#include "gmm_factor.hpp"
#include "is_draw.hpp"
#include "is_groups.hpp"

#include <float.h>

namespace pp {
namespace {

constexpr int TILE = 2048;                // particles per workgroup: 256 threads x PER_THREAD particles, 256 apart
constexpr int PER_THREAD = 8;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight particles");
constexpr int MAXCOMP = PP_IS_GMM_MAX_K;
constexpr int MAXJ = PP_IS_GMM_JOINT_MAX_J;
constexpr int MAXTRI = tri_of(MAXJ);
// The Philox stream id of the proposal's draws. Taken elsewhere: the statement indices j, 0x1C, 0x52, 0x53, 0x4000 + i,
// 0x10000 + j and everything with the top bit.
constexpr uint32_t PROPOSAL_STREAM = PP_IS_PROPOSAL_STREAM;

// One component of a block: the constants of gmm_factor.hpp's log_density (mu | L^-1 | c), then L, lower triangle row by row.
__host__ __device__ constexpr int comp_of(int J) { return consts_of(J) + tri_of(J); }
// A group's block: K components | K cumulative weights | bad (0 / 1)
__host__ __device__ constexpr int block_of(int J, int K) { return K * comp_of(J) + K + 1; }

struct ProposalCols {
    float* p[MAXJ];
};

// Launch 1: the block of group g0 + blockIdx.x from its row of the fit; 64 threads.
__global__ __launch_bounds__(64) void proposal_prepare_kernel(const double* __restrict__ fit, int64_t ld_fit, int J, int K, int g0,
                                                              double* __restrict__ blocks, int* __restrict__ status) {
    __shared__ double lf[MAXCOMP * MAXTRI], li[MAXCOMP * MAXTRI], ld[MAXCOMP], pi[MAXCOMP];
    __shared__ int bad[MAXCOMP];
    __shared__ int first_bad;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const int tid = threadIdx.x, tri = tri_of(J), CP = comp_of(J);
    const double* row = fit + g * ld_fit;
    double* blk = blocks + g * block_of(J, K);
    if (tid < K) {
        const double w = row[tid];
        const bool ok = w > 0.0 && w < (double)INFINITY &&
                        factorise(row + K + K * J + tid * tri, J, lf + tid * MAXTRI, li + tid * MAXTRI, ld + tid);
        bad[tid] = ok ? 0 : 1;
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int k = K - 1; k >= 0; --k) b = bad[k] ? k + 1 : b;
        first_bad = b;
        status[g] = b;
        blk[K * CP + K] = b ? 1.0 : 0.0;
        if (!b) {
            double total = 0.0;
            for (int k = 0; k < K; ++k) total += row[k];
            double cum = 0.0;
            for (int k = 0; k < K; ++k) {
                pi[k] = row[k] / total;
                cum += pi[k];
                blk[K * CP + k] = cum;
            }
        }
    }
    __syncthreads();
    if (first_bad) return;
    const int C = consts_of(J);
    for (int s = tid; s < K * CP; s += 64) {
        const int k = s / CP, e = s - k * CP;
        blk[s] = e < J            ? row[K + k * J + e]
                 : e < J + tri    ? li[k * MAXTRI + e - J]
                 : e == J + tri   ? log(pi[k]) - ld[k] - 0.5 * J * LOG_2PI
                                  : lf[k * MAXTRI + e - C];
    }
}

// Two standard normals from two Philox words: Box-Muller, both branches, on the hardware log2 / sqrt / sin / cos (the last two take
// revolutions). It shapes only WHICH value is drawn: the density is evaluated at the value, in fp64.
__device__ __forceinline__ void normal_pair(uint32_t w0, uint32_t w1, double& z0, double& z1) {
    const float r = __builtin_amdgcn_sqrtf(-2.0f * __logf(u01(w0))), u = u01(w1);
    z0 = (double)(r * __builtin_amdgcn_cosf(u));
    z1 = (double)(r * __builtin_amdgcn_sinf(u));
}

// x ~ q of the block `blk` (LDS) for Philox counter `ctr`, rounded to fp32.
template <int J>
__device__ __forceinline__ void draw_particle(const double* blk, int K, uint64_t seed, uint64_t ctr, float (&x)[J]) {
    constexpr int PAIRS = (J + 1) / 2, WORDS = 1 + 2 * PAIRS, CALLS = (WORDS + 3) / 4, CP = comp_of(J), C = consts_of(J);
    Philox rng(seed, ctr, PROPOSAL_STREAM);
    uint32_t w[4 * CALLS];
#pragma unroll
    for (int c = 0; c < CALLS; ++c) {
        uint32_t r[4];
        rng.next(r);
#pragma unroll
        for (int q = 0; q < 4; ++q) w[4 * c + q] = r[q];
    }
    const double u = (double)u01(w[0]);
    const double* cum = blk + K * CP;
    int k = K - 1;
    for (int c = K - 2; c >= 0; --c) k = u < cum[c] ? c : k;      // (the first c with u < cum[c]; the last where rounding leaves none)
    double z[2 * PAIRS];
#pragma unroll
    for (int p = 0; p < PAIRS; ++p) normal_pair(w[1 + 2 * p], w[2 + 2 * p], z[2 * p], z[2 * p + 1]);
    const double* ck = blk + k * CP;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double s = ck[j];
#pragma unroll
        for (int m = 0; m <= j; ++m) s += ck[C + lower_at(j, m)] * z[m];
        x[j] = (float)s;
    }
}

// Launch 2: workgroup (tile blockIdx.x, group g0 + blockIdx.y).
template <int J>
__global__ __launch_bounds__(256) void proposal_particle_kernel(ProposalCols cols, int K, int64_t n_per, int g0, int mode, uint64_t seed,
                                                                uint64_t offset, const double* __restrict__ blocks,
                                                                float* __restrict__ neg_log_q) {
    constexpr int CP = comp_of(J);
    __shared__ double sh[MAXCOMP * CP + MAXCOMP + 1];
    const int tid = threadIdx.x, B = block_of(J, K);
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const double* blk = blocks + g * B;
    for (int s = tid; s < B; s += 256) sh[s] = blk[s];
    __syncthreads();
    const int64_t base = g * n_per, first = (int64_t)blockIdx.x * TILE + tid;
    const bool bad = sh[K * CP + K] != 0.0;      // (uniform over the workgroup)
    float xv[PER_THREAD][J];
    if (mode == 0) {
#pragma unroll
        for (int p = 0; p < PER_THREAD; ++p) {
            const int64_t i = first + 256 * p;
            if (bad) {
#pragma unroll
                for (int j = 0; j < J; ++j) xv[p][j] = NAN;
            } else {
                draw_particle<J>(sh, K, seed, offset + (uint64_t)(base + i), xv[p]);
            }
            if (i < n_per) {
#pragma unroll
                for (int j = 0; j < J; ++j) cols.p[j][base + i] = xv[p][j];
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < PER_THREAD; ++p) {
            const int64_t i = first + 256 * p;
#pragma unroll
            for (int j = 0; j < J; ++j) xv[p][j] = i < n_per ? cols.p[j][base + i] : 0.0f;
        }
    }
    // logsumexp_c l_c by a running maximum: s holds sum exp(l - top), one exp per (particle, component)
    double top[PER_THREAD], s[PER_THREAD];
#pragma unroll
    for (int p = 0; p < PER_THREAD; ++p) {
        top[p] = -DBL_MAX;
        s[p] = 0.0;
    }
    for (int c = 0; c < K; ++c) {
        const double* ck = sh + c * CP;
#pragma unroll
        for (int p = 0; p < PER_THREAD; ++p) {
            double d[J];
            const double e = log_density<J>(xv[p], ck, d);
            const double t = exp(-fabs(e - top[p]));
            const bool up = e > top[p];
            s[p] = up ? s[p] * t + 1.0 : s[p] + t;
            top[p] = up ? e : top[p];
        }
    }
#pragma unroll
    for (int p = 0; p < PER_THREAD; ++p) {
        const int64_t i = first + 256 * p;
        if (i < n_per) neg_log_q[base + i] = bad ? NAN : (float)-(top[p] + log(s[p]));
    }
}

template <int J>
void launch_particles(dim3 grid, hipStream_t st, const ProposalCols& cols, int K, int64_t n_per, int g0, int mode, uint64_t seed,
                      uint64_t offset, const double* blocks, float* neg_log_q) {
    hipLaunchKernelGGL(proposal_particle_kernel<J>, grid, dim3(256), 0, st, cols, K, n_per, g0, mode, seed, offset, blocks, neg_log_q);
}
using ParticleLauncher = void (*)(dim3, hipStream_t, const ProposalCols&, int, int64_t, int, int, uint64_t, uint64_t, const double*,
                                  float*);
const ParticleLauncher PARTICLE_LAUNCHERS[MAXJ] = {launch_particles<1>, launch_particles<2>, launch_particles<3>, launch_particles<4>,
                                                   launch_particles<5>, launch_particles<6>, launch_particles<7>, launch_particles<8>};

bool proposal_shape_ok(int M, int J, int K) { return M >= 0 && J >= 1 && J <= MAXJ && K >= 1 && K <= MAXCOMP; }
size_t proposal_bytes(int M, int J, int K) { return (size_t)256 + (size_t)align256((int64_t)M * block_of(J, K) * 8); }

}  // namespace

int is_proposal_groups(const double* fit, int64_t ld_fit, int M, int J, int K, int64_t n_per, int mode, uint64_t seed, uint64_t offset,
                       float* const* cols, float* neg_log_q, int* status, void* ws, size_t ws_bytes, hipStream_t st) {
    const char* name = "pp_is_proposal_groups";
    PP_CHECK_ARG(J >= 1 && J <= MAXJ, "%s: n_cols in 1 .. %d", name, MAXJ);
    PP_CHECK_ARG(K >= 1 && K <= MAXCOMP, "%s: n_components in 1 .. %d", name, MAXCOMP);
    PP_CHECK_ARG(fit && cols && neg_log_q && status && ws,
                 "%s: null pointer (fit_rows, cols, neg_log_q, status and the workspace are required)", name);
    ProposalCols c;
    for (int j = 0; j < MAXJ; ++j) {
        c.p[j] = j < J ? cols[j] : nullptr;
        PP_CHECK_ARG(j >= J || c.p[j], "%s: column %d is a null pointer", name, j);
    }
    PP_CHECK_ARG(mode == 0 || mode == 1, "%s: mode 0 (draw) or 1 (score)", name);
    PP_CHECK_ARG(M >= 0 && n_per >= 0, "%s: n_groups >= 0 and n_per >= 0", name);
    PP_CHECK_ARG(n_per <= (int64_t)0x7fffffff * TILE, "%s: more than 2^31 - 1 tiles of %d particles per group", name, TILE);
    PP_CHECK_ARG(ld_fit >= (int64_t)K * params_of(J), "%s: ld_fit below the K (1 + J + J (J + 1) / 2) doubles of a row", name);
    PP_CHECK_ARG(ws_bytes >= proposal_bytes(M, J, K), "%s: workspace too small (%zu < %zu bytes)", name, ws_bytes,
                 proposal_bytes(M, J, K));
    if (M == 0 || n_per == 0) return 0;
    double* blocks = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
    const unsigned T = (unsigned)((n_per + TILE - 1) / TILE);
    for_each_group_chunk(M, [&](int g0, int groups) {
        hipLaunchKernelGGL(proposal_prepare_kernel, dim3(groups), dim3(64), 0, st, fit, ld_fit, J, K, g0, blocks, status);
        PARTICLE_LAUNCHERS[J - 1](dim3(T, groups), st, c, K, n_per, g0, mode, seed, offset, (const double*)blocks, neg_log_q);
    });
    PP_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_proposal_workspace_bytes(int32_t n_groups, int32_t n_cols, int32_t n_components) {
    return pp::proposal_shape_ok(n_groups, n_cols, n_components) ? pp::proposal_bytes(n_groups, n_cols, n_components) : 0;
}

int pp_is_proposal_groups(const double* fit_rows, int64_t ld_fit, int32_t n_groups, int32_t n_cols, int32_t n_components, int64_t n_per,
                          int32_t mode, uint64_t seed, uint64_t offset, float* const* cols, float* neg_log_q, int32_t* status,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_proposal_groups(fit_rows, ld_fit, n_groups, n_cols, n_components, n_per, mode, seed, offset, cols, neg_log_q, status,
                                  workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
