// Weighted Gaussian-mixture EM over one latent of a (batched) lock-step posterior call on the device.
//
// The reference's Empirical.density_estimate (pyprob/distributions/empirical.py:795-807) resamples 1000 values on the host, throws
// the weights away and fits scikit-learn's GaussianMixture(covariance_type='diag') to them. Here
//   pp_is_gmm_groups  runs that EM, in one dimension and in fp64, over ALL n_per particles of each of M groups under their own
//   weights w_i (is_groups.hpp: which particles count and what they weigh; W = sum w_i) from the caller's initial parameters:
//   iteration t = 1 .. max_iter of a group, with pi_k, mu_k, v_k its current weights, means and variances,
//     E-step   l_ik = log pi_k - 1/2 log(2 pi v_k) - (x_i - mu_k)^2 / (2 v_k),  L_i = logsumexp_k l_ik,
//              r_ik = w_i exp(l_ik - L_i),  lb_t = sum_i w_i L_i / W
//     M-step   N_k = sum_i r_ik + 10 DBL_EPSILON,  d_k = sum_i r_ik (x_i - mu_k) / N_k,  mu'_k = mu_k + d_k,
//              v'_k = max(sum_i r_ik (x_i - mu_k)^2 / N_k - d_k^2, 0) + reg_covar,  pi'_k = N_k / sum_k N_k
//     stop     |lb_t - lb_{t-1}| < tol (lb_0 = -inf): converged, n_iter = t, the parameters are those AFTER this M-step (as in
//              scikit-learn); tol = 0 runs exactly max_iter iterations.
//   The sums of the M-step are taken about the current mean: a narrow posterior far from zero keeps its variance (the concern of
//   pp_is_moments_groups' pivots).
//
// SHAPE OF THE WORK. The row of `out` of a group IS its state: the current parameters, the last lower bound, n_iter and the
// converged flag. Per iteration two dependent launches on the caller's stream: a workgroup of 256 threads takes one tile of TILE
// particles of one group, holds the group's constants (mu_k, log pi_k - 1/2 log(2 pi v_k), 1 / (2 v_k)) in LDS - every lane reads
// the same address, a broadcast - sums r_k, r_k (x - mu_k), r_k (x - mu_k)^2 per component plus w L, w and the count in fp64
// registers (3 K + 3, the kernel is compiled per K), and STORES its partial row; then one workgroup per group adds the partial rows
// in tile order and forms the new parameters, the lower bound and the flag. No atomics, no workgroup waits for another. A
// converged group is frozen: both kernels return at entry on its flag. Every `check_every` iterations a one-workgroup launch folds
// the flags into one word, which the host reads to stop enqueuing; what a group computes does not depend on it.
//
// ORDER OF THE SUMS. As in is_moments.hip: a lane adds its eight particles (tile offset + 256 k + thread) in the order of k, the 64
// lanes of a wave meet by lane exchanges in a fixed pattern (wave_sum_dpp), the four waves in LDS as ((0 + 1) + 2) + 3, the tiles in
// index order, the components of sum_k N_k in the order of k. The order is a function of n_per and K alone: group g of an M-group
// call carries the bits of the one-group call on the same particles, whatever the other groups do and whatever check_every is.
#include "is_groups.hpp"

#include <float.h>

namespace pp {
namespace {

constexpr int TILE = 2048;                // particles per workgroup: 256 threads x PER_THREAD particles, 256 apart
constexpr int PER_THREAD = 8;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight particles");
constexpr int MAXK = PP_IS_GMM_MAX_K;
// A partial row of K components: sum r_k at k | sum r_k d at K + k | sum r_k d^2 at 2 K + k | sum w L, W, count, the group's maximum
__host__ __device__ constexpr int slots_of(int K) { return 3 * K + 4; }
// A row of `out`: pi at k | mu at K + k | v at 2 K + k | lower bound, n_iter, converged, W, count, the group's maximum
__host__ __device__ constexpr int width_of(int K) { return PP_IS_GMM_WIDTH(K); }

// Workspace: one partial row per (group, tile), one float (tile maximum) per tile, the "all groups converged" word.
struct GmmWorkspace {
    double* partial;
    float* tmax;
    int* all_done;
    size_t bytes;
};
void gmm_carve(int M, int n_per, int K, void* p, GmmWorkspace& w) {
    Carver c(p);
    const int64_t tiles = (int64_t)std::max(M, 0) * tiles_of(std::max(n_per, 1), TILE);
    w.partial = c.take<double>(tiles * slots_of(K) * 8);
    w.tmax = c.take<float>(tiles * 4);
    w.all_done = c.take<int>(4);
    w.bytes = c.bytes();
}

// Step 0: the state of every group from the caller's parameters; one thread per entry of `out`.
__global__ __launch_bounds__(256) void gmm_init_kernel(const double* __restrict__ init, int K, int64_t total, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int width = width_of(K);
    const int64_t g = i / width;
    const int e = (int)(i - g * width);
    out[i] = e < 3 * K ? init[g * 3 * K + e] : e == 3 * K ? (double)-INFINITY : e == 3 * K + 5 ? (double)-INFINITY : 0.0;
}

// Step 1 of an iteration: workgroup (tile blockIdx.x, group g0 + blockIdx.y) stores its partial row.
template <int K>
__global__ __launch_bounds__(256) void gmm_tile_kernel(const float* __restrict__ lw, const float* __restrict__ x, int n_per, int T,
                                                       int g0, const double* __restrict__ stats, const float* __restrict__ tmax,
                                                       const double* __restrict__ out, double* __restrict__ partial) {
    constexpr int SUMS = 3 * K + 3;
    __shared__ float shmax[4];
    __shared__ double sh[4][SUMS];
    __shared__ double sh_mu[K], sh_c[K], sh_h[K];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const double* state = out + g * width_of(K);
    if (state[3 * K + 2] != 0.0) return;      // (converged: frozen - uniform over the workgroup)
    const int64_t base = g * n_per;
    const float* l = lw + base;
    const float* xs = x + base;
    const int64_t first = (int64_t)blockIdx.x * TILE + tid;
    float a[PER_THREAD], xv[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const bool in = first + 256 * k < n_per;
        a[k] = in ? l[first + 256 * k] : -INFINITY;
        xv[k] = in ? xs[first + 256 * k] : 0.0f;
    }
    if (tid < K) {
        const double pi = state[tid], v = state[2 * K + tid];
        sh_mu[tid] = state[K + tid];
        sh_c[tid] = log(pi) - 0.5 * log(6.283185307179586476925286766559 * v);
        sh_h[tid] = 1.0 / (2.0 * v);
    }
    const double M = group_max<256>(stats, tmax, g, T, a, shmax);      // (its barrier also publishes the constants)
    if (stats) __syncthreads();
    const bool any = group_any(M);
    double R[K], S[K], Q[K], WL = 0.0, W = 0.0, count = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) R[c] = S[c] = Q[c] = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        if (particle_counted(a[k], any)) {      // (a skipped particle's value enters nothing)
            const double w = particle_weight(a[k], M, any);
            const double xd = (double)xv[k];
            double d[K], e[K], top = -INFINITY;
#pragma unroll
            for (int c = 0; c < K; ++c) {
                d[c] = xd - sh_mu[c];
                e[c] = sh_c[c] - d[c] * d[c] * sh_h[c];
                top = fmax(top, e[c]);
            }
            double s = 0.0;      // (fmax drops a NaN, e[c] - top keeps it: a NaN value under a weight reaches every sum)
#pragma unroll
            for (int c = 0; c < K; ++c) {
                e[c] = exp(e[c] - top);
                s += e[c];
            }
            const double L = top + log(s);
            const double ws = w / s;
            W += w;
            WL += w * L;
            count += 1.0;
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const double r = ws * e[c];
                const double rd = r * d[c];
                R[c] += r;
                S[c] += rd;
                Q[c] += rd * d[c];
            }
        }
    }
    // the 64 lanes of a wave, then the four waves in order
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const double r = wave_sum_dpp(R[c]), s = wave_sum_dpp(S[c]), q = wave_sum_dpp(Q[c]);
        if (lane == 0) {
            sh[wave][c] = r;
            sh[wave][K + c] = s;
            sh[wave][2 * K + c] = q;
        }
    }
    {
        const double wl = wave_sum_dpp(WL), w = wave_sum_dpp(W), n = wave_sum_dpp(count);
        if (lane == 0) {
            sh[wave][3 * K] = wl;
            sh[wave][3 * K + 1] = w;
            sh[wave][3 * K + 2] = n;
        }
    }
    __syncthreads();
    double* row = partial + (g * T + blockIdx.x) * slots_of(K);
    if (tid < SUMS) row[tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    else if (tid == SUMS) row[tid] = any ? M : (double)-INFINITY;
}

// Step 2 of iteration `iter`: one workgroup of 64 threads per group adds the partial rows in tile order and forms the new state.
__global__ __launch_bounds__(64) void gmm_combine_kernel(const double* __restrict__ partial, int K, int T, int g0, int iter, double tol,
                                                         double reg_covar, double* __restrict__ out) {
    __shared__ double sum[3 * MAXK + 4];
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const int slots = slots_of(K), tid = threadIdx.x;
    double* state = out + g * width_of(K);
    if (state[3 * K + 2] != 0.0) return;      // (converged: frozen)
    const double* rows = partial + g * T * slots;
    if (tid < slots - 1) sum[tid] = add_rows(rows[tid], rows + tid, (int64_t)slots, 1, T);      // (in tile order)
    else if (tid == slots - 1) sum[tid] = rows[tid];                                              // (the maximum: every tile's)
    __syncthreads();
    const double W = sum[3 * K + 1], count = sum[3 * K + 2];
    const bool none = !(count > 0.0);
    if (tid < K) {
        double total = 0.0;
        for (int c = 0; c < K; ++c) total += sum[c] + 10.0 * DBL_EPSILON;
        const double N = sum[tid] + 10.0 * DBL_EPSILON;
        const double d = sum[K + tid] / N;
        const double v = fmax(sum[2 * K + tid] / N - d * d, 0.0) + reg_covar;
        state[tid] = none ? NAN : N / total;
        state[K + tid] = none ? NAN : state[K + tid] + d;
        // (fmax drops a NaN: a NaN value under a weight gives NaN parameters, not a variance of reg_covar)
        state[2 * K + tid] = (none || d != d) ? NAN : v;
    } else if (tid == K) {
        const double lb = sum[3 * K] / W, before = state[3 * K];
        const bool converged = fabs(lb - before) < tol;
        state[3 * K] = none ? NAN : lb;
        state[3 * K + 1] = none ? 0.0 : (double)iter;
        state[3 * K + 2] = (none || converged) ? 1.0 : 0.0;
        state[3 * K + 3] = none ? 0.0 : W;
        state[3 * K + 4] = none ? 0.0 : count;
        state[3 * K + 5] = sum[3 * K + 3];
    }
}

// Every check_every iterations: one workgroup folds the M flags into the word the host reads.
__global__ __launch_bounds__(256) void gmm_all_done_kernel(const double* __restrict__ out, int K, int M, int* __restrict__ all_done) {
    __shared__ int open[4];
    int mine = 0;
    for (int64_t g = threadIdx.x; g < M; g += 256) mine |= out[g * width_of(K) + 3 * K + 2] == 0.0;
    const int w = __any(mine);
    if ((threadIdx.x & 63) == 0) open[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) *all_done = !(open[0] | open[1] | open[2] | open[3]);
}

template <int K>
void launch_tile(dim3 grid, hipStream_t st, const float* lw, const float* x, int n_per, int T, int g0, const double* stats,
                 const float* tmax, const double* out, double* partial) {
    hipLaunchKernelGGL(gmm_tile_kernel<K>, grid, dim3(256), 0, st, lw, x, n_per, T, g0, stats, tmax, out, partial);
}
using TileLauncher = void (*)(dim3, hipStream_t, const float*, const float*, int, int, int, const double*, const float*, const double*,
                              double*);
const TileLauncher TILE_LAUNCHERS[MAXK] = {launch_tile<1>,  launch_tile<2>,  launch_tile<3>,  launch_tile<4>,
                                           launch_tile<5>,  launch_tile<6>,  launch_tile<7>,  launch_tile<8>,
                                           launch_tile<9>,  launch_tile<10>, launch_tile<11>, launch_tile<12>,
                                           launch_tile<13>, launch_tile<14>, launch_tile<15>, launch_tile<16>};

}  // namespace

int is_gmm_groups(const float* lw, const float* x, int K, int M, int n_per, const double* stats, const double* init, int max_iter,
                  double tol, double reg_covar, int check_every, double* out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && x && init && out && ws, "pp_is_gmm_groups: null pointer (lw, x, params_init, out and the workspace are required)");
    PP_CHECK_ARG(K >= 1 && K <= MAXK, "pp_is_gmm_groups: n_components in 1 .. %d", MAXK);
    PP_CHECK_GROUPS("pp_is_gmm_groups", M, n_per);
    PP_CHECK_ARG(max_iter >= 1, "pp_is_gmm_groups: max_iter >= 1");
    PP_CHECK_ARG(tol >= 0.0 && reg_covar >= 0.0, "pp_is_gmm_groups: tol >= 0 and reg_covar >= 0");
    GmmWorkspace w;
    gmm_carve(M, n_per, K, ws, w);
    PP_CHECK_WORKSPACE("pp_is_gmm_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    if (check_every < 1) check_every = 8;
    const int T = tiles_of(n_per, TILE);
    const int64_t total = (int64_t)M * width_of(K);
    hipLaunchKernelGGL(gmm_init_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, init, K, total, out);
    if (T > 1 && !stats)
        for_each_group_chunk(M, [&](int g0, int groups) {
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, TILE, T, g0, w.tmax);
        });
    for (int iter = 1; iter <= max_iter; ++iter) {
        for_each_group_chunk(M, [&](int g0, int groups) {
            TILE_LAUNCHERS[K - 1](dim3(T, groups), st, lw, x, n_per, T, g0, stats, (const float*)w.tmax, (const double*)out, w.partial);
            hipLaunchKernelGGL(gmm_combine_kernel, dim3(groups), dim3(64), 0, st, (const double*)w.partial, K, T, g0, iter, tol,
                               reg_covar, out);
        });
        if (iter % check_every == 0 && iter < max_iter) {
            int done = 0;
            hipLaunchKernelGGL(gmm_all_done_kernel, dim3(1), dim3(256), 0, st, (const double*)out, K, M, w.all_done);
            PP_LAUNCH_CHECK("pp_is_gmm_groups");
            hipError_t e = hipMemcpyAsync(&done, w.all_done, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                set_error("pp_is_gmm_groups: reading the converged word failed: %s", hipGetErrorString(e));
                return (int)e;
            }
            if (done) break;
        }
    }
    PP_LAUNCH_CHECK("pp_is_gmm_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_gmm_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_components) {
    if (!pp::groups_shape_ok(n_groups, n_per) || n_components < 1 || n_components > PP_IS_GMM_MAX_K) return 0;
    pp::GmmWorkspace w;
    pp::gmm_carve(n_groups, n_per, n_components, nullptr, w);
    return w.bytes;
}

int pp_is_gmm_groups(const float* lw, const float* x, int32_t n_components, int32_t n_groups, int32_t n_per, const double* stats,
                     const double* params_init, int32_t max_iter, double tol, double reg_covar, int32_t check_every, double* out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_gmm_groups(lw, x, n_components, n_groups, n_per, stats, params_init, max_iter, tol, reg_covar, check_every, out,
                             workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
