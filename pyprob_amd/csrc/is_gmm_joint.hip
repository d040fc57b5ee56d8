// Weighted EM for a mixture of K full-covariance Gaussians over J latents of a (batched) lock-step posterior call on the device.
//
// is_gmm.hip fits one latent with one variance per component; the dependence BETWEEN latents - ridges, two joint modes that look
// unimodal in every marginal - needs the joint density. Here
//   pp_is_gmm_joint_groups  runs the EM of include/pyprob_amd.h in fp64 over the n_per particles of each of M groups: J columns of
//   the statement log (1 <= J <= 8), K components (1 <= K <= 16) with means mu_k [J] and covariances Sigma_k = L_k L_k^T [J, J].
//   A particle counts where is_groups.hpp counts it AND all its J coordinates are finite; it weighs w = exp((double)lw - max_g).
//
// SHAPE OF THE WORK, as in is_gmm.hip: the row of `out` of a group is its state; per iteration two dependent launches.
//   tile kernel     A workgroup of 256 threads takes one tile of 2048 particles of one group: a thread holds its eight particles
//                   (J floats each) in registers. The group's constants - per component mu_k, the packed lower-triangular INVERSE
//                   factor L_k^-1 and c_k = log pi_k - sum_j log L_k,jj - J/2 log 2 pi, J + J (J + 1) / 2 + 1 doubles - were formed
//                   ONCE per iteration by the combine kernel and lie in the workspace; the workgroup copies them to LDS, where every
//                   lane reads the same address (a broadcast). l_ik = c_k - 1/2 |L_k^-1 (x_i - mu_k)|^2 is a triangular product of
//                   J (J + 1) / 2 FMAs, compiled per J.
//                   K (1 + J + J (J + 1) / 2) + 3 sums (723 at J = 8, K = 16) cannot live in registers at once, so the tile is swept
//                   twice. SWEEP 1, components outermost: a running logsumexp per particle (top, s: ONE exp per (i, k)) leaves L_i.
//                   SWEEP 2, components outermost again: the 1 + J + J (J + 1) / 2 accumulators of ONE component (45 at J = 8) in
//                   registers; l_ik is recomputed - 44 FMAs against 90 registers times sixteen -, r_ik = w_i exp(l_ik - L_i) enters
//                   R, r d_j and r d_j d_m (j <= m); the accumulators are reduced and parked in LDS, and the next component starts.
//   combine kernel  One workgroup per group adds the tile rows in tile order, forms pi', mu', Sigma' (thread k: component k),
//                   factorises the K matrices in LDS (Cholesky, then the inverse of the factor by forward substitution) and writes
//                   the state, the flags and the constants of the next iteration. A pivot that is not positive: nothing of the
//                   state's parameters is written, degenerate = 1, and the group is frozen like a converged one.
// No atomics, no workgroup waits for another, no dynamically indexed private array (nothing in scratch memory).
//
// ORDER OF THE SUMS, as in is_gmm.hip: a lane adds its eight particles (tile offset + 256 p + thread) in the order of p, the 64 lanes
// of a wave meet by lane exchanges in a fixed pattern (wave_sum_dpp), the four waves in LDS as ((0 + 1) + 2) + 3, the tiles in index
// order, the components in the order of k. The order is a function of (n_per, J, K) alone: group g of an M-group call carries the bits
// of the one-group call on the same particles, whatever the other groups do and whatever check_every is.
#include "gmm_factor.hpp"
#include "is_groups.hpp"

#include <float.h>

namespace pp {
namespace {

constexpr int TILE = 2048;                // particles per workgroup: 256 threads x PER_THREAD particles, 256 apart
constexpr int PER_THREAD = 8;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight particles");
constexpr int MAXK = PP_IS_GMM_MAX_K;
constexpr int MAXJ = PP_IS_GMM_JOINT_MAX_J;

// A partial row: component k's sums R | S [J] | Q [tri] at k params_of(J) | sum w L, W, count, the group's maximum
__host__ __device__ constexpr int slots_of(int J, int K) { return K * params_of(J) + 4; }
// A row of `out`: pi [K] | mu [K, J] | Sigma [K, tri] | lower bound, n_iter, converged, degenerate, W, count, the group's maximum
__host__ __device__ constexpr int width_of(int J, int K) { return PP_IS_GMM_JOINT_WIDTH(J, K); }
constexpr int MAXTRI = tri_of(MAXJ), MAXP = params_of(MAXJ);

struct JointCols {
    const float* p[MAXJ];
};

// Workspace: one partial row per (group, tile), one float (tile maximum) per tile, the constants of every group, the "all groups
// closed" word.
struct JointWorkspace {
    double* partial;
    float* tmax;
    double* cons;
    int* all_done;
    size_t bytes;
};
void joint_carve(int M, int n_per, int J, int K, void* p, JointWorkspace& w) {
    Carver c(p);
    const int64_t groups = std::max(M, 0);
    const int64_t tiles = groups * tiles_of(std::max(n_per, 1), TILE);
    w.partial = c.take<double>(tiles * slots_of(J, K) * 8);
    w.tmax = c.take<float>(tiles * 4);
    w.cons = c.take<double>(groups * K * consts_of(J) * 8);
    w.all_done = c.take<int>(4);
    w.bytes = c.bytes();
}

// The constants of a group from its parameters `par` (pi | mu | Sigma, any address space), the inverse factors and log-determinants:
// entry e of component k at cons[k consts_of(J) + e]; all threads of the workgroup.
__device__ void publish_constants(const double* par, const double* li, const double* ld, int J, int K, int threads,
                                  double* __restrict__ cons) {
    const int C = consts_of(J), tri = tri_of(J);
    for (int s = threadIdx.x; s < K * C; s += threads) {
        const int k = s / C, e = s - k * C;
        cons[s] = e < J ? par[K + k * J + e] : e < J + tri ? li[k * MAXTRI + e - J] : log(par[k]) - ld[k] - 0.5 * J * LOG_2PI;
    }
}

// Step 0: the state and the constants of group blockIdx.x from the caller's parameters; 64 threads.
__global__ __launch_bounds__(64) void joint_init_kernel(const double* __restrict__ init, int J, int K, int g0, double* __restrict__ out,
                                                        double* __restrict__ cons) {
    __shared__ double lf[MAXK * MAXTRI], li[MAXK * MAXTRI], ld[MAXK];
    __shared__ int bad;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const int tid = threadIdx.x, P = params_of(J), off = K * P;
    const double* par = init + g * off;
    double* state = out + g * width_of(J, K);
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid < K && !factorise(par + K + K * J + tid * tri_of(J), J, lf + tid * MAXTRI, li + tid * MAXTRI, ld + tid)) bad = 1;
    __syncthreads();
    const bool degenerate = bad != 0;
    for (int s = tid; s < off; s += 64) state[s] = par[s];
    if (tid < 7) state[off + tid] = (tid == 0 || tid == 6) ? (double)-INFINITY : (tid == 3 && degenerate) ? 1.0 : 0.0;
    if (!degenerate) publish_constants(par, li, ld, J, K, 64, cons + g * K * consts_of(J));
}

// Step 1 of an iteration: workgroup (tile blockIdx.x, group g0 + blockIdx.y) stores its partial row.
template <int J>
__global__ __launch_bounds__(256) void joint_tile_kernel(const float* __restrict__ lw, JointCols cols, int K, int n_per, int T, int g0,
                                                         const double* __restrict__ stats, const float* __restrict__ tmax,
                                                         const double* __restrict__ out, const double* __restrict__ cons,
                                                         double* __restrict__ partial) {
    constexpr int TRI = tri_of(J), P = params_of(J), C = consts_of(J);
    __shared__ float shmax[4];
    __shared__ double sh_c[MAXK * C];
    __shared__ double sh[4][MAXK * P + 3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const double* flags = out + g * width_of(J, K) + K * P;
    if (flags[2] != 0.0 || flags[3] != 0.0) return;      // (converged or degenerate: frozen - uniform over the workgroup)
    const int64_t base = g * n_per;
    const float* l = lw + base;
    const int64_t first = (int64_t)blockIdx.x * TILE + tid;
    float a[PER_THREAD], xv[PER_THREAD][J];
#pragma unroll
    for (int p = 0; p < PER_THREAD; ++p) {
        const bool in = first + 256 * p < n_per;
        a[p] = in ? l[first + 256 * p] : -INFINITY;
#pragma unroll
        for (int j = 0; j < J; ++j) xv[p][j] = in ? cols.p[j][base + first + 256 * p] : 0.0f;
    }
    for (int s = tid; s < K * C; s += 256) sh_c[s] = cons[g * K * C + s];
    const double M = group_max<256>(stats, tmax, g, T, a, shmax);      // (its barrier also publishes the constants)
    if (stats) __syncthreads();
    const bool any = group_any(M);
    // A skipped particle - no finite log-weight, or a coordinate that is not finite - gets weight 0 and the coordinates 0: every
    // product it enters is +0, and a sum that gains +0 keeps its bits.
    double w[PER_THREAD], count = 0.0;
#pragma unroll
    for (int p = 0; p < PER_THREAD; ++p) {
        bool ok = particle_counted(a[p], any);
#pragma unroll
        for (int j = 0; j < J; ++j) ok = ok && isfinite(xv[p][j]);
        w[p] = ok ? particle_weight(a[p], M, any) : 0.0;
        count += ok ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) xv[p][j] = ok ? xv[p][j] : 0.0f;
    }
    // sweep 1: L_i = logsumexp_k l_ik by a running maximum - s holds sum exp(l - top)
    double L[PER_THREAD], s[PER_THREAD];
#pragma unroll
    for (int p = 0; p < PER_THREAD; ++p) {
        L[p] = -DBL_MAX;
        s[p] = 0.0;
    }
    for (int k = 0; k < K; ++k) {
        const double* ck = sh_c + k * C;
#pragma unroll
        for (int p = 0; p < PER_THREAD; ++p) {
            double d[J];
            const double e = log_density<J>(xv[p], ck, d);
            const double t = exp(-fabs(e - L[p]));
            const bool up = e > L[p];
            s[p] = up ? s[p] * t + 1.0 : s[p] + t;
            L[p] = up ? e : L[p];
        }
    }
    double WL = 0.0, W = 0.0;
#pragma unroll
    for (int p = 0; p < PER_THREAD; ++p) {
        L[p] += log(s[p]);
        W += w[p];
        WL += w[p] * L[p];
    }
    // sweep 2: the sums of one component at a time
    for (int k = 0; k < K; ++k) {
        const double* ck = sh_c + k * C;
        double acc[P];
#pragma unroll
        for (int q = 0; q < P; ++q) acc[q] = 0.0;
#pragma unroll
        for (int p = 0; p < PER_THREAD; ++p) {
            double d[J];
            const double e = log_density<J>(xv[p], ck, d);
            const double r = w[p] * exp(e - L[p]);
            acc[0] += r;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double rd = r * d[j];
                acc[1 + j] += rd;
#pragma unroll
                for (int m = j; m < J; ++m) acc[1 + J + upper_at(J, j, m)] += rd * d[m];
            }
        }
        // the 64 lanes of a wave; the four waves meet below
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const double v = wave_sum_dpp(acc[q]);
            if (lane == 0) sh[wave][k * P + q] = v;
        }
    }
    {
        const double wl = wave_sum_dpp(WL), ws = wave_sum_dpp(W), n = wave_sum_dpp(count);
        if (lane == 0) {
            sh[wave][K * P] = wl;
            sh[wave][K * P + 1] = ws;
            sh[wave][K * P + 2] = n;
        }
    }
    __syncthreads();
    double* row = partial + (g * T + blockIdx.x) * slots_of(J, K);
    for (int q = tid; q < K * P + 3; q += 256) row[q] = ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
    if (tid == 0) row[K * P + 3] = any ? M : (double)-INFINITY;
    (void)TRI;
}

// Step 2 of iteration `iter`: one workgroup of 256 threads per group adds the partial rows in tile order and forms the new state.
__global__ __launch_bounds__(256) void joint_combine_kernel(const double* __restrict__ partial, int J, int K, int T, int g0, int iter,
                                                            double tol, double reg_covar, double* __restrict__ out,
                                                            double* __restrict__ cons) {
    __shared__ double sum[MAXK * MAXP + 4], fresh[MAXK * MAXP];
    __shared__ double lf[MAXK * MAXTRI], li[MAXK * MAXTRI], ld[MAXK];
    __shared__ int bad;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const int tid = threadIdx.x, tri = tri_of(J), P = params_of(J), off = K * P, slots = slots_of(J, K);
    double* state = out + g * width_of(J, K);
    if (state[off + 2] != 0.0 || state[off + 3] != 0.0) return;      // (converged or degenerate: frozen)
    const double* rows = partial + g * T * slots;
    for (int s = tid; s < slots; s += 256)
        sum[s] = s < slots - 1 ? add_rows(rows[s], rows + s, (int64_t)slots, 1, T) : rows[s];      // (in tile order; the maximum: every tile's)
    if (tid == 0) bad = 0;
    __syncthreads();
    const double W = sum[off + 1], count = sum[off + 2];
    const bool none = !(count > 0.0);
    if (tid < K && !none) {
        const int k = tid;
        double total = 0.0;
        for (int c = 0; c < K; ++c) total += sum[c * P] + 10.0 * DBL_EPSILON;
        const double N = sum[k * P] + 10.0 * DBL_EPSILON;
        const double* S = sum + k * P + 1;
        fresh[k] = N / total;
        for (int j = 0; j < J; ++j) fresh[K + k * J + j] = state[K + k * J + j] + S[j] / N;
        double* cov = fresh + K + K * J + k * tri;
        for (int j = 0; j < J; ++j)
            for (int m = j; m < J; ++m)
                cov[upper_at(J, j, m)] = S[J + upper_at(J, j, m)] / N - (S[j] / N) * (S[m] / N) + (j == m ? reg_covar : 0.0);
        if (!factorise(cov, J, lf + k * MAXTRI, li + k * MAXTRI, ld + k)) bad = 1;
    }
    __syncthreads();
    const bool degenerate = !none && bad != 0;
    if (none) {
        for (int s = tid; s < off; s += 256) state[s] = NAN;
    } else if (!degenerate) {
        for (int s = tid; s < off; s += 256) state[s] = fresh[s];
        publish_constants(fresh, li, ld, J, K, 256, cons + g * K * consts_of(J));
    }
    if (tid == 0) {
        const double lb = sum[off] / W, before = state[off];
        const bool converged = fabs(lb - before) < tol;
        state[off] = none ? NAN : lb;
        state[off + 1] = none ? 0.0 : (double)iter;
        state[off + 2] = none ? 1.0 : (converged && !degenerate) ? 1.0 : 0.0;
        state[off + 3] = degenerate ? 1.0 : 0.0;
        state[off + 4] = none ? 0.0 : W;
        state[off + 5] = none ? 0.0 : count;
        state[off + 6] = sum[off + 3];
    }
}

// Every check_every iterations: one workgroup folds the M flags into the word the host reads.
__global__ __launch_bounds__(256) void joint_all_done_kernel(const double* __restrict__ out, int J, int K, int M, int* __restrict__ all_done) {
    __shared__ int open[4];
    int mine = 0;
    for (int64_t g = threadIdx.x; g < M; g += 256) {
        const double* flags = out + g * width_of(J, K) + K * params_of(J);
        mine |= flags[2] == 0.0 && flags[3] == 0.0;
    }
    const int w = __any(mine);
    if ((threadIdx.x & 63) == 0) open[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) *all_done = !(open[0] | open[1] | open[2] | open[3]);
}

template <int J>
void launch_tile(dim3 grid, hipStream_t st, const float* lw, const JointCols& cols, int K, int n_per, int T, int g0, const double* stats,
                 const float* tmax, const double* out, const double* cons, double* partial) {
    hipLaunchKernelGGL(joint_tile_kernel<J>, grid, dim3(256), 0, st, lw, cols, K, n_per, T, g0, stats, tmax, out, cons, partial);
}
using TileLauncher = void (*)(dim3, hipStream_t, const float*, const JointCols&, int, int, int, int, const double*, const float*,
                              const double*, const double*, double*);
const TileLauncher TILE_LAUNCHERS[MAXJ] = {launch_tile<1>, launch_tile<2>, launch_tile<3>, launch_tile<4>,
                                           launch_tile<5>, launch_tile<6>, launch_tile<7>, launch_tile<8>};

}  // namespace

int is_gmm_joint_groups(const float* lw, const float* const* cols, int J, int K, int M, int n_per, const double* stats,
                        const double* init, int max_iter, double tol, double reg_covar, int check_every, double* out, void* ws,
                        size_t ws_bytes, hipStream_t st) {
    const char* name = "pp_is_gmm_joint_groups";
    PP_CHECK_ARG(lw && cols && init && out && ws, "%s: null pointer (lw, cols, params_init, out and the workspace are required)", name);
    PP_CHECK_ARG(J >= 1 && J <= MAXJ, "%s: n_cols in 1 .. %d", name, MAXJ);
    PP_CHECK_ARG(K >= 1 && K <= MAXK, "%s: n_components in 1 .. %d", name, MAXK);
    JointCols c;
    for (int j = 0; j < MAXJ; ++j) {
        c.p[j] = j < J ? cols[j] : nullptr;
        PP_CHECK_ARG(j >= J || c.p[j], "%s: column %d is a null pointer", name, j);
    }
    PP_CHECK_GROUPS("pp_is_gmm_joint_groups", M, n_per);
    PP_CHECK_ARG(max_iter >= 1, "%s: max_iter >= 1", name);
    PP_CHECK_ARG(tol >= 0.0 && reg_covar >= 0.0, "%s: tol >= 0 and reg_covar >= 0", name);
    JointWorkspace w;
    joint_carve(M, n_per, J, K, ws, w);
    PP_CHECK_WORKSPACE("pp_is_gmm_joint_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    if (check_every < 1) check_every = 8;
    const int T = tiles_of(n_per, TILE);
    for_each_group_chunk(M, [&](int g0, int groups) {
        hipLaunchKernelGGL(joint_init_kernel, dim3(groups), dim3(64), 0, st, init, J, K, g0, out, w.cons);
        if (T > 1 && !stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, TILE, T, g0, w.tmax);
    });
    for (int iter = 1; iter <= max_iter; ++iter) {
        for_each_group_chunk(M, [&](int g0, int groups) {
            TILE_LAUNCHERS[J - 1](dim3(T, groups), st, lw, c, K, n_per, T, g0, stats, (const float*)w.tmax, (const double*)out,
                                  (const double*)w.cons, w.partial);
            hipLaunchKernelGGL(joint_combine_kernel, dim3(groups), dim3(256), 0, st, (const double*)w.partial, J, K, T, g0, iter, tol,
                               reg_covar, out, w.cons);
        });
        if (iter % check_every == 0 && iter < max_iter) {
            int done = 0;
            hipLaunchKernelGGL(joint_all_done_kernel, dim3(1), dim3(256), 0, st, (const double*)out, J, K, M, w.all_done);
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
    PP_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_gmm_joint_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_cols, int32_t n_components) {
    if (!pp::groups_shape_ok(n_groups, n_per) || n_cols < 1 || n_cols > PP_IS_GMM_JOINT_MAX_J || n_components < 1 ||
        n_components > PP_IS_GMM_MAX_K)
        return 0;
    pp::JointWorkspace w;
    pp::joint_carve(n_groups, n_per, n_cols, n_components, nullptr, w);
    return w.bytes;
}

int pp_is_gmm_joint_groups(const float* lw, const float* const* cols, int32_t n_cols, int32_t n_components, int32_t n_groups,
                           int32_t n_per, const double* stats, const double* params_init, int32_t max_iter, double tol,
                           double reg_covar, int32_t check_every, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_gmm_joint_groups(lw, cols, n_cols, n_components, n_groups, n_per, stats, params_init, max_iter, tol, reg_covar,
                                   check_every, out, workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
