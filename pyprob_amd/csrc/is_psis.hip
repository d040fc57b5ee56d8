// Pareto-smoothed importance weights and the k-hat diagnostic of a device-backed posterior (PSIS: Vehtari, Simpson, Gelman, Yao,
// Gabry, JMLR 2024): a generalised Pareto distribution fitted to the largest weights of every group by the Zhang-Stephens
// profile estimate, its shape k-hat, and the tail weights replaced by the fitted distribution's order statistics.
//
// The reference has no counterpart: the only reliability figure of its Empirical is effective_sample_size
// (pyprob/distributions/empirical.py:758-766). The definition is the header comment of pp_is_psis_groups (include/pyprob_amd.h).
//
// Four dependent launches over the particles sorted by log-weight (pp_is_sort_groups keyed on the log-weight itself):
//   (a) psis_tail_kernel     one thread per tail rank: the exceedance y_r (one fp64 exp) to the workspace; the first thread of a
//                            group writes the group's row of `out` with k-hat = +inf, sigma = NaN ("no fit") and u, q, y_{n-1}.
//   (b) psis_profile_kernel  one WAVE per (group, grid point j): lane l adds log1p(-theta_j y_r) over r = l, l + 64, ... in index
//                            order with a compensated sum, the 64 lane sums are added by a fixed butterfly: kappa_j, L_j.
//   (c) psis_fit_kernel      one workgroup per group: omega_j = 1 / sum_l exp(L_l - L_j) (thread t takes j = t, t + 256, ..., each
//                            sum over l in index order), theta-hat, one pass over y for kappa, then sigma and k-hat to `out`.
//   (d) psis_smooth_kernel   one thread per sorted position: the smoothed or the copied log-weight through index_sorted.
// No atomics, no workgroup waits for another. Every sum's order is a function of n and m alone: two calls give the same bits,
// and group g of an M-group call equals the one-group call on its slice.
#include "is_groups.hpp"

namespace pp {
namespace {

constexpr int WIDTH = PP_IS_PSIS_WIDTH;
constexpr int HDR = 4;           // per group in the workspace: u, q, y_{n-1}, (unused)
constexpr int WAVES = 4;         // grid points per workgroup of launch (b)

// The tail length the rule gives c counted particles, and the largest tail and grid any group of n_per particles can have.
__host__ __device__ inline int64_t tail_rule(int c, int tail) {
    return tail > 0 ? (int64_t)tail : (int64_t)ceil(fmin(c / 5.0, 3.0 * sqrt((double)c)));
}
inline int psis_ycap(int n_per, int tail) { return (int)std::max<int64_t>(1, std::min<int64_t>(tail_rule(n_per, tail), n_per)); }
inline int psis_mcap(int ycap) { return 30 + (int)floor(sqrt((double)ycap)); }

// acc += x, compensated (Kahan): the lane's sum does not lose the low bits of a long tail.
__device__ __forceinline__ void kahan_add(double& s, double& comp, double x) {
    const double y = x - comp;
    const double t = s + y;
    comp = (t - s) - y;
    s = t;
}

// The sum over a workgroup of 256 threads in a fixed order: the butterfly of every wave, then wave 0 + 1 + 2 + 3. sh: 4 doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ void write_row(double* __restrict__ row, double n, double m, double f, double sb, double c, double Mg) {
    row[0] = INFINITY;
    row[1] = NAN;
    row[2] = n;
    row[3] = m;
    row[4] = f;
    row[5] = sb;
    row[6] = c;
    row[7] = Mg;
}

// (a) workgroup (tile blockIdx.x of the tail, group g0 + blockIdx.y)
__global__ __launch_bounds__(256) void psis_tail_kernel(const float* __restrict__ lw_sorted, const int* __restrict__ counted, int n_per,
                                                        int tail, int ycap, int g0, double* __restrict__ y, double* __restrict__ hdr,
                                                        double* __restrict__ out) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const float* s = lw_sorted + g * n_per;
    const int c = max(0, min(counted[2 * g], n_per));
    const bool head = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t nt = tail_rule(c, tail);
    const int64_t b64 = (int64_t)c - nt - 1;
    if (c == 0 || b64 < 0) {      // (no-fit condition A)
        if (head) write_row(out + g * WIDTH, 0.0, 0.0, 0.0, NAN, (double)c, c > 0 ? (double)s[c - 1] : NAN);
        return;
    }
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((int64_t)blockIdx.x * 256 >= nt) return;      // (n <= n_t: a tile past this group's tail, never tile 0 as n_t >= 1)
    const int b = (int)b64;
    const float cut = s[b];
    int lo = b + 1, hi = c;      // f: the first position in [b + 1, c] whose log-weight is above the cutoff's
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= cut) lo = mid + 1;
        else hi = mid;
    }
    const int f = lo, n = c - f;
    if (r >= n && !head) return;      // (ties with the cutoff shortened the tail: no exp for a rank it does not have)
    const double Mg = (double)s[c - 1], sb = (double)cut;
    const double u = exp(sb - Mg);
    if (r < n && r < ycap) y[g * ycap + r] = exp((double)s[f + r] - Mg) - u;
    if (head) {
        bool fit = n > 4 && n <= ycap;
        if (fit) fit = (exp((double)s[f] - Mg) - u) > 0.0;      // (no-fit condition B; y_0 as launch (b) reads it)
        double* h = hdr + g * HDR;
        h[0] = u;
        h[1] = fit ? exp((double)s[f + (int)(n / 4.0 + 0.5) - 1] - Mg) - u : NAN;
        h[2] = fit ? exp((double)s[c - 1] - Mg) - u : NAN;
        h[3] = 0.0;
        write_row(out + g * WIDTH, (double)n, fit ? (double)(30 + (int)floor(sqrt((double)n))) : 0.0, (double)f, sb, (double)c, Mg);
    }
}

// (b) wave w of workgroup (block blockIdx.x of grid points, group g0 + blockIdx.y): grid point j = 4 blockIdx.x + w + 1.
__global__ __launch_bounds__(256) void psis_profile_kernel(const double* __restrict__ y, const double* __restrict__ hdr,
                                                           const double* __restrict__ out, int ycap, int mcap, int g0,
                                                           double* __restrict__ theta, double* __restrict__ prof) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const double* row = out + g * WIDTH;
    const int m = (int)row[3], n = (int)row[2];
    const int j0 = (int)blockIdx.x * WAVES + (int)(threadIdx.x >> 6);
    if (j0 >= m || j0 >= mcap || n > ycap) return;      // (whole waves leave; nothing below synchronises the workgroup)
    const int lane = threadIdx.x & 63;
    const double q = hdr[g * HDR + 1], ymax = hdr[g * HDR + 2];
    const double th = 1.0 / ymax + (1.0 - sqrt((double)m / ((double)(j0 + 1) - 0.5))) / (3.0 * q);
    const double* yy = y + g * ycap;
    double sum = 0.0, comp = 0.0;
    for (int r = lane; r < n; r += 64) kahan_add(sum, comp, log1p(-th * yy[r]));
    const double kappa = wave_sum(sum - comp) / (double)n;
    if (lane == 0) {
        theta[g * mcap + j0] = th;
        prof[g * mcap + j0] = (double)n * (log(-th / kappa) - kappa - 1.0);
    }
}

// (c) one workgroup per group g0 + blockIdx.x
__global__ __launch_bounds__(256) void psis_fit_kernel(const double* __restrict__ y, const double* __restrict__ theta,
                                                       const double* __restrict__ prof, int ycap, int mcap, int g0,
                                                       double* __restrict__ out) {
    __shared__ double sh_a[4], sh_b[4];
    const int64_t g = (int64_t)g0 + blockIdx.x;
    double* row = out + g * WIDTH;
    const int m = (int)row[3], n = (int)row[2];
    if (m <= 0 || m > mcap || n > ycap) return;      // (no fit; uniform in the workgroup)
    const double* L = prof + g * mcap;
    const double* th = theta + g * mcap;
    double acc = 0.0;
    for (int j = threadIdx.x; j < m; j += 256) {
        const double Lj = L[j];
        double sum = 0.0;
        for (int l = 0; l < m; ++l) sum += exp(L[l] - Lj);
        acc += (1.0 / sum) * th[j];      // (an overflowing sum: omega_j = 0)
    }
    const double that = block_sum(acc, sh_a);
    const double* yy = y + g * ycap;
    double sum = 0.0, comp = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) kahan_add(sum, comp, log1p(-that * yy[r]));
    const double kappa = block_sum(sum - comp, sh_b) / (double)n;
    if (threadIdx.x == 0) {
        row[0] = ((double)n * kappa + 5.0) / ((double)n + 10.0);
        row[1] = -kappa / that;
    }
}

// (d) one thread per sorted position of group g0 + blockIdx.y
__global__ __launch_bounds__(256) void psis_smooth_kernel(const float* __restrict__ lw_sorted, const int* __restrict__ index_sorted,
                                                          const double* __restrict__ out, int n_per, int g0,
                                                          float* __restrict__ lw_out) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_per) return;
    const double* row = out + g * WIDTH;
    const double k = row[0];
    const int n = (int)row[2], f = (int)row[4], c = (int)row[6];
    float v = lw_sorted[g * n_per + p];
    unsigned bits = __float_as_uint(v);
    if (k > -INFINITY && k < INFINITY && n > 0 && p >= f && p < c) {
        const double sigma = row[1], Mg = row[7];
        const double u = exp(row[5] - Mg);
        const double lp = log1p(-((double)(p - f) + 0.5) / (double)n);
        const double w = k == 0.0 ? u - sigma * lp : u + sigma * expm1(-k * lp) / k;
        bits = __float_as_uint((float)(fmin(log(w), 0.0) + Mg));
    }
    const int idx = index_sorted[g * n_per + p];
    if ((unsigned)idx < (unsigned)n_per) reinterpret_cast<unsigned*>(lw_out)[g * n_per + idx] = bits;
}

struct PsisWorkspace {
    double *y, *hdr, *theta, *prof;
    int ycap, mcap;
    size_t bytes;
};
void psis_carve(int M, int n_per, int tail, void* p, PsisWorkspace& w) {
    Carver c(p);
    const int64_t groups = std::max(M, 0);
    w.ycap = psis_ycap(std::max(n_per, 1), tail);
    w.mcap = psis_mcap(w.ycap);
    w.y = c.take<double>(groups * w.ycap * (int64_t)sizeof(double));
    w.hdr = c.take<double>(groups * HDR * (int64_t)sizeof(double));
    w.theta = c.take<double>(groups * w.mcap * (int64_t)sizeof(double));
    w.prof = c.take<double>(groups * w.mcap * (int64_t)sizeof(double));
    w.bytes = c.bytes();
}
inline bool psis_shape_ok(int M, int n_per, int tail) { return groups_shape_ok(M, n_per) && tail >= 0; }

}  // namespace

int is_psis_groups(const float* lw_sorted, const int* index_sorted, const int* counted, int M, int n_per, const double* stats,
                   int tail, float* lw_out, double* out, void* ws, size_t ws_bytes, hipStream_t st) {
    (void)stats;      // (the maximum is the last counted sorted log-weight: the same bits)
    PP_CHECK_ARG(lw_sorted && index_sorted && counted && out && ws,
                 "pp_is_psis_groups: null pointer (the sorted log-weights, their indices, the counts, out and the workspace are required)");
    PP_CHECK_GROUPS("pp_is_psis_groups", M, n_per);
    PP_CHECK_ARG(tail >= 0, "pp_is_psis_groups: tail >= 0 (0: the rule min(c / 5, 3 sqrt(c)))");
    PsisWorkspace w;
    psis_carve(M, n_per, tail, ws, w);
    PP_CHECK_WORKSPACE("pp_is_psis_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    for_each_group_chunk(M, [&](int g0, int groups) {
        hipLaunchKernelGGL(psis_tail_kernel, dim3(cdiv(w.ycap, 256), groups), dim3(256), 0, st, lw_sorted, counted, n_per, tail, w.ycap,
                           g0, w.y, w.hdr, out);
        hipLaunchKernelGGL(psis_profile_kernel, dim3(cdiv(w.mcap, WAVES), groups), dim3(256), 0, st, (const double*)w.y,
                           (const double*)w.hdr, (const double*)out, w.ycap, w.mcap, g0, w.theta, w.prof);
        hipLaunchKernelGGL(psis_fit_kernel, dim3(groups), dim3(256), 0, st, (const double*)w.y, (const double*)w.theta,
                           (const double*)w.prof, w.ycap, w.mcap, g0, out);
        if (lw_out)
            hipLaunchKernelGGL(psis_smooth_kernel, dim3(cdiv(n_per, 256), groups), dim3(256), 0, st, lw_sorted, index_sorted,
                               (const double*)out, n_per, g0, lw_out);
    });
    PP_LAUNCH_CHECK("pp_is_psis_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_psis_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t tail) {
    if (!pp::psis_shape_ok(n_groups, n_per, tail)) return 0;
    pp::PsisWorkspace w;
    pp::psis_carve(n_groups, n_per, tail, nullptr, w);
    return w.bytes;
}

int pp_is_psis_groups(const float* lw_sorted, const int32_t* index_sorted, const int32_t* counted, int32_t n_groups, int32_t n_per,
                      const double* stats, int32_t tail, float* lw_out, double* out, void* workspace, size_t workspace_bytes,
                      void* stream) {
    return pp::is_psis_groups(lw_sorted, index_sorted, counted, n_groups, n_per, stats, tail, lw_out, out, workspace, workspace_bytes,
                              pp::as_stream(stream));
}

}  // extern "C"
