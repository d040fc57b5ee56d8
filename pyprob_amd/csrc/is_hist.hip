// Weighted 1-D and 2-D histograms of the latents of a (batched) lock-step posterior call on the device, and a latent's extent.
//
// The reference normalises the weights of an Empirical on the host (pyprob/distributions/empirical.py:298-309) and draws its
// histogram from all values and weights on the host (plot_histogram, :889-914). Here
//   pp_is_hist_groups    writes, per group g of n_per particles, the row [2][slots] of 64-bit integers: the fixed-point mass
//       sum_i llrint(w_i 2^S) and the particle count of every slot (is_groups.hpp: which particles count, the clamped weight w
//       and the shift S). Slots, 1-D: [bins ..., below, above, x is NaN]; 2-D: [ix bins_y + iy ...,
//       outside, either coordinate NaN]. Bin b holds e_b <= x < e_{b+1}, the last bin also x == e_last (numpy.histogram's rule),
//       found by binary search over the edges staged in LDS: non-uniform edges cost the same as uniform ones, and the bin is a
//       function of the very array the host shows the user.
//   pp_is_extent_groups  writes, per group, min x, max x, the particles counted and the particles whose x is NaN.
//
// SHAPE OF THE WORK. A workgroup takes one tile of one group, eight particles per thread (256 threads and 2048 particles up to 256
// bins, 1024 threads and 8192 particles above), bins them into an LDS histogram with
// integer LDS adds (ds_add_u64 for the mass, ds_add_u32 for the count) and STORES its partial row in the workspace with plain
// stores; a second launch adds the partial rows of every group, one thread per slot. A group of one tile stores its row in `out`
// directly. No global atomics, no workgroup waits for another: the launches are dependent launches on the caller's stream.
// LDS per workgroup: 12 bytes per slot and 8 per edge, sized at launch - 41 KB at 2048 bins, 1 KB at 50.
//
// ORDER. Integer sums, minima and maxima do not depend on the order they are taken in: a call repeated gives the same bits, group g
// of an M-group call carries the bits of the one-group call on its slice, and the tile size is free to change. (fp64 accumulators
// would need a fixed order for that, and float atomics have none.) The x / y of a skipped particle are loaded, but whatever they
// hold selects no slot and enters no count.
#include "is_groups.hpp"

namespace pp {
namespace {

// Particles per workgroup: eight per thread, one workgroup width apart. A partial row is 16 bytes per slot, so the tile grows with the
// histogram: 256 threads (2048 particles, 16 KB read) up to 256 bins (a row of 4 KB at most), 1024 threads (8192 particles) above,
// where a row reaches 32 KB. The wide workgroup, not more particles per thread: a thread's eight fp64 exponentials and LDS adds are
// one dependent chain, and it is the number of waves on a SIMD that hides it (four rounds of 256 threads ran 44 us at 10^6
// particles where one round of 1024 threads runs the same tiles). Integer sums: the tiling changes no bit.
constexpr int PER_THREAD = 8;
constexpr int SMALL_BINS = 256, SMALL_THREADS = 256, LARGE_THREADS = 1024;
constexpr int EXTENT_TILE = 256 * PER_THREAD;

inline int tile_for(int bins) { return (bins <= SMALL_BINS ? SMALL_THREADS : LARGE_THREADS) * PER_THREAD; }
inline int slots_of(int bx, int by, bool two_d) { return two_d ? bx * by + 2 : bx + 3; }

// Workspace: one partial row (2 slots int64) per (group, tile) where a group has more than one tile, one float (the tile's maximum)
// per (group, tile).
struct HistWorkspace {
    int64_t* partial;
    float* tmax;
    size_t bytes;
};
void hist_carve(int M, int n_per, int bins, void* p, HistWorkspace& w) {      // (bins + 3 slots cover the 1-D and the 2-D row)
    Carver c(p);
    const int slots = bins + 3;
    const int T = tiles_of(std::max(n_per, 1), tile_for(bins));
    const int64_t tiles = (int64_t)std::max(M, 0) * T;
    w.partial = c.take<int64_t>(T > 1 ? tiles * 2 * slots * 8 : 0);
    w.tmax = c.take<float>(tiles * 4);
    w.bytes = c.bytes();
}

struct ExtentPartial {
    float lo, hi;
    uint32_t counted, nans;
};
size_t extent_bytes(int M, int n_per) {
    const int T = tiles_of(std::max(n_per, 1), EXTENT_TILE);
    return (size_t)(256 + align256(T > 1 ? (int64_t)std::max(M, 0) * T * (int64_t)sizeof(ExtentPartial) : 0));
}

// The bins of the eight values v[k] in the n = nb + 1 strictly increasing edges e (LDS): pos = the number of edges <= v, found by
// a branchless binary search whose trip count depends on n alone - the eight searches advance together, so eight LDS reads are in
// flight per step where one search after the other would wait for each of its own. Returns in b[k]: -1 below e[0], nb above e[nb],
// else the bin with e[b] <= v < e[b + 1], the last bin closed on the right. A NaN compares false everywhere (pos 0): the caller
// gives NaN its own slot.
__device__ __forceinline__ void bins_of(const double* e, int nb, const float (&v)[PER_THREAD], int (&b)[PER_THREAD]) {
    const int n = nb + 1;
    int pos[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) pos[k] = 0;
    for (int step = 1 << (31 - __clz(n)); step > 0; step >>= 1) {
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int at = pos[k] + step;
            const double edge = e[min(at, n) - 1];
            pos[k] = (at <= n && edge <= (double)v[k]) ? at : pos[k];
        }
    }
    const double last = e[nb];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) b[k] = pos[k] == n ? ((double)v[k] == last ? nb - 1 : nb) : pos[k] - 1;
}

// Workgroup (tile blockIdx.x, group g0 + blockIdx.y) stores its row [2][slots] at dst + (g T + tile) 2 slots.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void hist_tile_kernel(const float* __restrict__ lw, const float* __restrict__ x,
                                                        const float* __restrict__ y, int n_per, int T, int g0,
                                                        const double* __restrict__ ex, int bx, int64_t sx,
                                                        const double* __restrict__ ey, int by, int64_t sy,
                                                        const double* __restrict__ stats, const float* __restrict__ tmax, double scale,
                                                        int64_t* __restrict__ dst) {
    extern __shared__ unsigned long long dyn[];
    __shared__ float shmax[THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const bool two_d = y != nullptr;
    const int slots = two_d ? bx * by + 2 : bx + 3;
    const int ne = bx + 1 + (two_d ? by + 1 : 0);
    unsigned long long* mass = dyn;                                      // [slots]
    double* edge_x = reinterpret_cast<double*>(dyn + slots);             // [bx + 1]
    double* edge_y = edge_x + bx + 1;                                    // [by + 1] (2-D)
    unsigned int* count = reinterpret_cast<unsigned int*>(dyn + slots + ne);      // [slots]
    for (int s = tid; s < slots; s += THREADS) {
        mass[s] = 0;
        count[s] = 0;
    }
    for (int i = tid; i <= bx; i += THREADS) edge_x[i] = ex[g * sx + i];
    if (two_d)
        for (int i = tid; i <= by; i += THREADS) edge_y[i] = ey[g * sy + i];
    const int64_t base = g * n_per;
    const float* l = lw + base;
    const int64_t first = (int64_t)blockIdx.x * (THREADS * PER_THREAD) + tid;
    float a[PER_THREAD], xv[PER_THREAD], yv[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) a[k] = first + THREADS * k < n_per ? l[first + THREADS * k] : -INFINITY;
    const double M = group_max<THREADS>(stats, tmax, g, T, a, shmax);      // (one tile: the workgroup's own particles are the group)
    const bool any = group_any(M);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + THREADS * k;
        const bool in = i < n_per;
        xv[k] = in ? x[base + i] : 0.0f;
        yv[k] = (in && two_d) ? y[base + i] : 0.0f;
    }
    // (the bins of all eight, skipped particles included: their values select nothing below)
    int ix[PER_THREAD], iy[PER_THREAD];
    bins_of(edge_x, bx, xv, ix);
    if (two_d) bins_of(edge_y, by, yv, iy);
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        if (!particle_counted(a[k], any)) continue;      // (a skipped particle is in no slot and no count)
        const unsigned long long q = fixed_mass(particle_weight_clamped(a[k], M, any), scale);
        int slot;
        if (!two_d) {
            slot = xv[k] != xv[k] ? bx + 2 : ix[k] < 0 ? bx : ix[k] == bx ? bx + 1 : ix[k];
        } else {
            const bool nan = xv[k] != xv[k] || yv[k] != yv[k];
            const bool outside = ix[k] < 0 || ix[k] == bx || iy[k] < 0 || iy[k] == by;
            slot = nan ? bx * by + 1 : outside ? bx * by : ix[k] * by + iy[k];
        }
        atomicAdd(&mass[slot], q);
        atomicAdd(&count[slot], 1u);
    }
    __syncthreads();
    int64_t* row = dst + (g * T + blockIdx.x) * 2 * slots;
    for (int s = tid; s < slots; s += THREADS) {
        row[s] = (int64_t)mass[s];
        row[slots + s] = (int64_t)count[s];
    }
}

// Groups of more than one tile: thread (blockIdx.x, threadIdx.x) adds entry e of the T partial rows of group g0 + blockIdx.y.
__global__ __launch_bounds__(256) void hist_combine_kernel(const int64_t* __restrict__ partial, int width, int T, int g0,
                                                           int64_t* __restrict__ out) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= width) return;
    out[g * width + e] = add_rows(int64_t(0), partial + g * T * width + e, (int64_t)width, 0, T);
}

// min / max of x and the two counts over tile blockIdx.x of group g0 + blockIdx.y; a group of one tile writes its output row.
__global__ __launch_bounds__(256) void extent_tile_kernel(const float* __restrict__ lw, const float* __restrict__ x, int n_per, int T,
                                                          int g0, ExtentPartial* __restrict__ partial, double* __restrict__ out) {
    __shared__ float shlo[4], shhi[4];
    __shared__ unsigned int shcnt[2];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t base = g * n_per;
    const int64_t first = (int64_t)blockIdx.x * EXTENT_TILE + tid;
    if (tid < 2) shcnt[tid] = 0;
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    unsigned int counted = 0, nans = 0;
    float a[PER_THREAD], xv[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + 256 * k;
        const bool in = i < n_per;
        a[k] = in ? lw[base + i] : -INFINITY;
        xv[k] = in ? x[base + i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        if (!isfinite(a[k])) continue;
        if (xv[k] != xv[k]) {
            ++nans;
        } else {
            ++counted;
            lo = fminf(lo, xv[k]);
            hi = fmaxf(hi, xv[k]);
        }
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((tid & 63) == 0) {
        shlo[tid >> 6] = lo;
        shhi[tid >> 6] = hi;
    }
    atomicAdd(&shcnt[0], counted);
    atomicAdd(&shcnt[1], nans);
    __syncthreads();
    if (tid == 0) {
        lo = fminf(fminf(shlo[0], shlo[1]), fminf(shlo[2], shlo[3]));
        hi = fmaxf(fmaxf(shhi[0], shhi[1]), fmaxf(shhi[2], shhi[3]));
        if (T == 1) {
            double* o = out + 4 * g;
            o[0] = (double)lo;
            o[1] = (double)hi;
            o[2] = (double)shcnt[0];
            o[3] = (double)shcnt[1];
        } else {
            ExtentPartial r;
            r.lo = lo;
            r.hi = hi;
            r.counted = shcnt[0];
            r.nans = shcnt[1];
            partial[g * T + blockIdx.x] = r;
        }
    }
}

// Groups of more than one tile: one workgroup per group meets the T tile results.
__global__ __launch_bounds__(256) void extent_combine_kernel(const ExtentPartial* __restrict__ partial, int T, int g0,
                                                             double* __restrict__ out) {
    __shared__ float shlo[4], shhi[4];
    __shared__ unsigned long long shcnt[2];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    if (tid < 2) shcnt[tid] = 0;
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    unsigned long long counted = 0, nans = 0;
    for (int t = tid; t < T; t += 256) {
        const ExtentPartial r = partial[g * T + t];
        lo = fminf(lo, r.lo);
        hi = fmaxf(hi, r.hi);
        counted += r.counted;
        nans += r.nans;
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((tid & 63) == 0) {
        shlo[tid >> 6] = lo;
        shhi[tid >> 6] = hi;
    }
    atomicAdd(&shcnt[0], counted);
    atomicAdd(&shcnt[1], nans);
    __syncthreads();
    if (tid == 0) {
        double* o = out + 4 * g;
        o[0] = (double)fminf(fminf(shlo[0], shlo[1]), fminf(shlo[2], shlo[3]));
        o[1] = (double)fmaxf(fmaxf(shhi[0], shhi[1]), fmaxf(shhi[2], shhi[3]));
        o[2] = (double)shcnt[0];
        o[3] = (double)shcnt[1];
    }
}

bool hist_shape_ok(int M, int n_per, int bx, int by) {
    return groups_shape_ok(M, n_per) && bx >= 1 && by >= 1 && (int64_t)bx * by <= PP_IS_HIST_MAX_BINS;
}

}  // namespace

int is_hist_groups(const float* lw, const float* x, const float* y, int M, int n_per, const double* ex, int bx, int64_t sx,
                   const double* ey, int by, int64_t sy, const double* stats, int64_t* out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && x && ex && out && ws, "pp_is_hist_groups: null pointer (lw, x, edges_x, out and the workspace are required)");
    PP_CHECK_GROUPS("pp_is_hist_groups", M, n_per);
    PP_CHECK_ARG(bx >= 1 && by >= 1 && (int64_t)bx * by <= PP_IS_HIST_MAX_BINS,
                 "pp_is_hist_groups: bins_x >= 1, bins_y >= 1 and bins_x * bins_y <= %d", PP_IS_HIST_MAX_BINS);
    PP_CHECK_ARG((y != nullptr) == (ey != nullptr), "pp_is_hist_groups: y and edges_y are given together (2-D) or not at all (1-D)");
    PP_CHECK_ARG(y || by == 1, "pp_is_hist_groups: bins_y must be 1 for a 1-D histogram");
    PP_CHECK_ARG(sx == 0 || sx >= bx + 1, "pp_is_hist_groups: edges_x_stride is 0 (shared) or at least bins_x + 1");
    PP_CHECK_ARG(!y || sy == 0 || sy >= by + 1, "pp_is_hist_groups: edges_y_stride is 0 (shared) or at least bins_y + 1");
    const bool two_d = y != nullptr;
    const int slots = slots_of(bx, by, two_d);
    HistWorkspace w;
    hist_carve(M, n_per, bx * by, ws, w);      // (one size for 1-D and 2-D: pp_is_hist_workspace_bytes does not know which)
    PP_CHECK_WORKSPACE("pp_is_hist_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int tile = tile_for(bx * by), T = tiles_of(n_per, tile), width = 2 * slots;
    const int ne = bx + 1 + (two_d ? by + 1 : 0);
    const size_t lds = (size_t)slots * 12 + (size_t)ne * 8;
    const double scale = hist_scale(n_per);
    for_each_group_chunk(M, [&](int g0, int groups) {
        if (T > 1 && !stats) hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, tile, T, g0, w.tmax);
        int64_t* dst = T > 1 ? w.partial : out;
        if (tile == SMALL_THREADS * PER_THREAD)
            hipLaunchKernelGGL(hist_tile_kernel<SMALL_THREADS>, dim3(T, groups), dim3(SMALL_THREADS), lds, st, lw, x, y, n_per, T, g0, ex, bx,
                               sx, ey, by, sy, stats, (const float*)w.tmax, scale, dst);
        else
            hipLaunchKernelGGL(hist_tile_kernel<LARGE_THREADS>, dim3(T, groups), dim3(LARGE_THREADS), lds, st, lw, x, y, n_per, T, g0, ex, bx,
                               sx, ey, by, sy, stats, (const float*)w.tmax, scale, dst);
        if (T > 1)
            hipLaunchKernelGGL(hist_combine_kernel, dim3(cdiv(width, 256), groups), dim3(256), 0, st, (const int64_t*)w.partial, width,
                               T, g0, out);
    });
    PP_LAUNCH_CHECK("pp_is_hist_groups");
    return 0;
}

int is_extent_groups(const float* lw, const float* x, int M, int n_per, double* out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && x && out && ws, "pp_is_extent_groups: null pointer (lw, x, out and the workspace are required)");
    PP_CHECK_GROUPS("pp_is_extent_groups", M, n_per);
    PP_CHECK_WORKSPACE("pp_is_extent_groups", ws_bytes, extent_bytes(M, n_per));
    if (M == 0) return 0;
    const int T = tiles_of(n_per, EXTENT_TILE);
    ExtentPartial* partial = static_cast<ExtentPartial*>(ws);
    for_each_group_chunk(M, [&](int g0, int groups) {
        hipLaunchKernelGGL(extent_tile_kernel, dim3(T, groups), dim3(256), 0, st, lw, x, n_per, T, g0, partial, out);
        if (T > 1)
            hipLaunchKernelGGL(extent_combine_kernel, dim3(groups), dim3(256), 0, st, (const ExtentPartial*)partial, T, g0, out);
    });
    PP_LAUNCH_CHECK("pp_is_extent_groups");
    return 0;
}

}  // namespace pp

extern "C" {

int32_t pp_is_hist_shift(int32_t n_per) { return pp::hist_shift(n_per); }

size_t pp_is_hist_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t bins_x, int32_t bins_y) {
    if (!pp::hist_shape_ok(n_groups, n_per, bins_x, bins_y)) return 0;
    pp::HistWorkspace w;
    pp::hist_carve(n_groups, n_per, bins_x * bins_y, nullptr, w);
    return w.bytes;
}

int pp_is_hist_groups(const float* lw, const float* x, const float* y, int32_t n_groups, int32_t n_per, const double* edges_x,
                      int32_t bins_x, int64_t edges_x_stride, const double* edges_y, int32_t bins_y, int64_t edges_y_stride,
                      const double* stats, int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_hist_groups(lw, x, y, n_groups, n_per, edges_x, bins_x, edges_x_stride, edges_y, bins_y, edges_y_stride, stats, out,
                              workspace, workspace_bytes, pp::as_stream(stream));
}

size_t pp_is_extent_workspace_bytes(int32_t n_groups, int32_t n_per) {
    if (!pp::groups_shape_ok(n_groups, n_per)) return 0;
    return pp::extent_bytes(n_groups, n_per);
}

int pp_is_extent_groups(const float* lw, const float* x, int32_t n_groups, int32_t n_per, double* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return pp::is_extent_groups(lw, x, n_groups, n_per, out, workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
