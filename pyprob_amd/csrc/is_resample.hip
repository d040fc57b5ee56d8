// Resampling a device-backed posterior on the device: the cumulative weights of every group of a (batched) lock-step call and
// multinomial draws from them.
//
// The reference keeps the normalised weights of an Empirical on the host (finalize, pyprob/distributions/empirical.py:298-309),
// draws ONE index per call from a Categorical over them (sample, :392-408) and resamples by calling sample() num_samples times
// (resample, :617-637). Here
//   pp_is_cdf_groups       writes cdf[g, i] = the sum of the weights of particles 0 .. i of group g in fp64 (is_groups.hpp: what
//                          a particle weighs and which particles weigh nothing), and
//   pp_is_resample_groups  draws n_out indices per group by inverting that cdf at Philox uniforms of 53 bits, one thread per draw;
//   pp_is_resample_scheme_groups  the same launch shape for stratified and systematic positions (resample_scheme_kernel).
//
// ORDER OF THE SUMS. cdf[g, i] is built as  tile offset + (wave offset + (lane offset + running sum of the thread's own eight)),
// and every offset is carried FORWARD: the offset of lane l + 1 is (offset of lane l) + (total of lane l), rounded once - the
// value lane l stored for its last particle. Likewise for the four waves of a tile and for the tiles of a group. Two things
// follow that a tree-shaped scan does not give in floating point: the cdf never decreases, and it is flat exactly across a
// particle of weight 0 (also where a thread, wave or tile ends) - so the binary search of the draw kernel and numpy.searchsorted
// agree on it and a particle of weight 0 is not selected. The order is a function of n_per alone: group g of an M-group call
// carries the bits of the one-group call on the same particles, and a call repeated gives the same bits. No workgroup waits for
// another inside a kernel and nothing is accumulated with atomics: the three steps are dependent launches on the caller's stream.
#include "is_draw.hpp"
#include "is_groups.hpp"

namespace pp {
namespace {

constexpr int TILE = PP_IS_CDF_TILE;      // particles per workgroup: 256 threads x PER_THREAD consecutive particles
constexpr int PER_THREAD = 8;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight particles");
constexpr int RESAMPLE_BLOCKS = 2048;     // workgroups of the draw kernel at most (8 per CU)


// Workspace of pp_is_cdf_groups: one double (tile total, then tile offset) and one float (tile maximum) per tile of every group
// with more than one tile; a one-tile group needs neither.
struct CdfWorkspace {
    double* total;
    float* tmax;
    size_t bytes;
};
void cdf_carve(int M, int n_per, void* p, CdfWorkspace& w) {
    Carver c(p);
    const int T = tiles_of(std::max(n_per, 1), TILE);
    const int64_t slots = T > 1 ? (int64_t)std::max(M, 0) * T : 0;
    w.total = c.take<double>(slots * 8);
    w.tmax = c.take<float>(slots * 4);
    w.bytes = c.bytes();
}

// Step 0 (groups of more than one tile, no statistics given): group_tile_max_kernel.
// Step 1: workgroup (tile t, group g0 + blockIdx.y) writes the tile-local inclusive sums of its particles to cdf and (T > 1) the
// tile's total to total[g T + t]. Thread `tid` owns particles [t TILE + 8 tid, + 8).
__global__ __launch_bounds__(256) void cdf_scan_kernel(const float* __restrict__ lw, int n_per, int T, int g0,
                                                       const double* __restrict__ stats, const float* __restrict__ tmax,
                                                       double* __restrict__ cdf, double* __restrict__ total) {
    __shared__ float shmax[4];
    __shared__ double shtot[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const float* l = lw + g * n_per;
    double* out = cdf + g * n_per;
    const int64_t first = (int64_t)blockIdx.x * TILE + (int64_t)tid * PER_THREAD;
    float a[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) a[k] = first + k < n_per ? l[first + k] : -INFINITY;
    const double M = group_max<256>(stats, tmax, g, T, a, shmax);
    const bool any = group_any(M);
    // the thread's own running sums
    double s[PER_THREAD];
    double run = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        run += particle_weight(a[k], M, any);
        s[k] = run;
    }
    // lane offsets, carried forward through the wave: offset(l + 1) = offset(l) + total(l). Every lane follows the whole chain
    // (the totals arrive by __shfl from a constant lane, a register read) and keeps the value at its own position.
    double mine = 0.0, chain = 0.0;
#pragma unroll
    for (int q = 0; q < 64; ++q) {
        const double t = __shfl(run, q, 64);
        if (lane == q) mine = chain;
        chain += t;
    }
    if (lane == 0) shtot[wave] = chain;      // the wave's total = what its last lane stores for its last particle
    __syncthreads();
    // the four waves, in order
    double woff = 0.0;
    for (int q = 0; q < wave; ++q) woff += shtot[q];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k)
        if (first + k < n_per) out[first + k] = woff + (mine + s[k]);
    if (T > 1 && tid == 0) total[g * T + blockIdx.x] = ((shtot[0] + shtot[1]) + shtot[2]) + shtot[3];
}

// Step 2: one workgroup per group turns its tile totals into exclusive offsets in place, in index order (offset(t + 1) =
// offset(t) + total(t): the value tile t's last particle gets in step 3). The totals pass through LDS in chunks of 1024.
__global__ __launch_bounds__(256) void cdf_offsets_kernel(double* __restrict__ total, int T, int g0) {
    __shared__ double sh[1024];
    __shared__ double carry;
    const int tid = threadIdx.x;
    double* t = total + ((int64_t)g0 + blockIdx.x) * T;
    if (tid == 0) carry = 0.0;
    for (int base = 0; base < T; base += 1024) {
        const int cnt = min(1024, T - base);
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) sh[i] = t[base + i];
        __syncthreads();
        if (tid == 0) {
            double c = carry;
            for (int i = 0; i < cnt; ++i) {
                const double v = sh[i];
                sh[i] = c;
                c += v;
            }
            carry = c;
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) t[base + i] = sh[i];
    }
}

// Step 3: tiles 1 .. T - 1 of every group add their offset in place (tile 0's offset is 0).
__global__ __launch_bounds__(256) void cdf_add_kernel(double* __restrict__ cdf, int n_per, int T, int g0,
                                                      const double* __restrict__ offset) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int tile = (int)blockIdx.x + 1;
    double* out = cdf + g * n_per;
    const double off = offset[g * T + tile];
    const int64_t first = (int64_t)tile * TILE + (int64_t)threadIdx.x * PER_THREAD;
    double v[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) v[k] = first + k < n_per ? out[first + k] : 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k)
        if (first + k < n_per) out[first + k] = off + v[k];
}

// One thread per draw: output o = g n_out + j takes the Philox block of counter offset + o (stream 0x52), a uniform of 53 bits,
// target = base + u * total (two roundings) and index = lo + #{i in [lo, hi): cdf[g, i] <= target}, at most hi - 1.
__global__ __launch_bounds__(256) void resample_kernel(const double* __restrict__ cdf, const float* __restrict__ values, int n_per,
                                                       int lo, int hi, int n_out, int64_t outputs, uint64_t seed, uint64_t offset,
                                                       int64_t* __restrict__ index_out, float* __restrict__ value_out) {
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < outputs; o += (int64_t)gridDim.x * 256) {
        const int64_t g = o / n_out;
        const double* c = cdf + g * n_per;
        const double base = lo > 0 ? c[lo - 1] : 0.0;
        const double total = c[hi - 1] - base;
        int64_t idx = -1;
        float v = NAN;
        if (total > 0.0 && total < INFINITY) {
            Philox rng(seed, offset + (uint64_t)o, 0x52);
            uint32_t r[4];
            rng.next(r);
            const uint64_t bits = ((uint64_t)(r[0] >> 5) << 26) + (uint64_t)(r[1] >> 6);
            const double u = __dmul_rn(__dadd_rn((double)bits, 0.5), 0x1.0p-53);
            const double target = __dadd_rn(base, __dmul_rn(u, total));
            int a = lo, b = hi;      // the first i in [lo, hi] with cdf[i] > target (hi: none)
            while (a < b) {
                const int mid = a + ((b - a) >> 1);
                if (c[mid] <= target) a = mid + 1;
                else b = mid;
            }
            idx = min(a, hi - 1);
            if (value_out) v = values[g * n_per + idx];
        }
        if (index_out) index_out[o] = idx;
        if (value_out) value_out[o] = v;
    }
}

// The low-variance schemes, one thread per draw as above. Draw j of group g sits at position p = min((j + u) / n_out, 1 - 2^-53) of
// the group's mass (two roundings before the minimum) and takes target = base + p * total (two more) through the search of
// resample_kernel. STRATIFIED: u is the 53-bit uniform of the block at counter offset + g n_out + j, stream 0x52 - one per draw.
// SYSTEMATIC: ONE u per group, from the block at counter offset + g, stream 0x53 (every thread of the group regenerates it).
// p never decreases in j, so neither do the targets and the indices of a group.
__global__ __launch_bounds__(256) void resample_scheme_kernel(const double* __restrict__ cdf, const float* __restrict__ values,
                                                              int n_per, int lo, int hi, int n_out, int64_t outputs, int scheme,
                                                              uint64_t seed, uint64_t offset, int64_t* __restrict__ index_out,
                                                              float* __restrict__ value_out) {
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < outputs; o += (int64_t)gridDim.x * 256) {
        const int64_t g = o / n_out;
        const int64_t j = o - g * n_out;
        const double* c = cdf + g * n_per;
        const double base = lo > 0 ? c[lo - 1] : 0.0;
        const double total = c[hi - 1] - base;
        int64_t idx = -1;
        float v = NAN;
        if (total > 0.0 && total < INFINITY) {
            const bool systematic = scheme == PP_RESAMPLE_SYSTEMATIC;
            Philox rng(seed, offset + (uint64_t)(systematic ? g : o), systematic ? 0x53 : 0x52);
            uint32_t r[4];
            rng.next(r);
            const uint64_t bits = ((uint64_t)(r[0] >> 5) << 26) + (uint64_t)(r[1] >> 6);
            const double u = __dmul_rn(__dadd_rn((double)bits, 0.5), 0x1.0p-53);
            const double p = fmin(__ddiv_rn(__dadd_rn((double)j, u), (double)n_out), 1.0 - 0x1.0p-53);
            const double target = __dadd_rn(base, __dmul_rn(p, total));
            int a = lo, b = hi;      // the first i in [lo, hi] with cdf[i] > target (hi: none)
            while (a < b) {
                const int mid = a + ((b - a) >> 1);
                if (c[mid] <= target) a = mid + 1;
                else b = mid;
            }
            idx = min(a, hi - 1);
            if (value_out) v = values[g * n_per + idx];
        }
        if (index_out) index_out[o] = idx;
        if (value_out) value_out[o] = v;
    }
}

}  // namespace

int is_cdf_groups(const float* lw, int M, int n_per, const double* stats, double* cdf, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(lw && cdf && ws, "pp_is_cdf_groups: null pointer (lw, cdf_out and the workspace are required)");
    PP_CHECK_GROUPS("pp_is_cdf_groups", M, n_per);
    CdfWorkspace w;
    cdf_carve(M, n_per, ws, w);
    PP_CHECK_WORKSPACE("pp_is_cdf_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(n_per, TILE);
    for_each_group_chunk(M, [&](int g0, int groups) {
        if (T > 1 && !stats)
            hipLaunchKernelGGL(group_tile_max_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, TILE, T, g0, w.tmax);
        hipLaunchKernelGGL(cdf_scan_kernel, dim3(T, groups), dim3(256), 0, st, lw, n_per, T, g0, stats, (const float*)w.tmax, cdf, w.total);
        if (T > 1) {
            hipLaunchKernelGGL(cdf_offsets_kernel, dim3(groups), dim3(256), 0, st, w.total, T, g0);
            hipLaunchKernelGGL(cdf_add_kernel, dim3(T - 1, groups), dim3(256), 0, st, cdf, n_per, T, g0, (const double*)w.total);
        }
    });
    PP_LAUNCH_CHECK("pp_is_cdf_groups");
    return 0;
}

int is_resample_groups(const double* cdf, const float* values, int M, int n_per, int lo, int hi, int n_out, uint64_t seed,
                       uint64_t offset, int64_t* index_out, float* value_out, hipStream_t st) {
    PP_CHECK_ARG(cdf, "pp_is_resample_groups: null pointer (the cdf is required)");
    PP_CHECK_ARG(n_per >= 1 && M >= 0 && n_out >= 0, "pp_is_resample_groups: n_per >= 1, n_groups >= 0 and n_out >= 0");
    PP_CHECK_ARG(0 <= lo && lo < hi && hi <= n_per, "pp_is_resample_groups: an index range 0 <= lo < hi <= n_per");
    PP_CHECK_ARG(groups_count_ok(M, n_per) && groups_count_ok(M, n_out),
                 "pp_is_resample_groups: more than 2^31 - 1 particles or draws per call: shard the groups");
    PP_CHECK_ARG(index_out || value_out, "pp_is_resample_groups: index_out or value_out (or both)");
    PP_CHECK_ARG(!value_out || values, "pp_is_resample_groups: value_out needs the values");
    const int64_t outputs = (int64_t)M * n_out;
    if (outputs == 0) return 0;
    const int blocks = (int)std::min<int64_t>(RESAMPLE_BLOCKS, (outputs + 255) / 256);
    hipLaunchKernelGGL(resample_kernel, dim3(blocks), dim3(256), 0, st, cdf, values, n_per, lo, hi, n_out, outputs, seed, offset,
                       index_out, value_out);
    PP_LAUNCH_CHECK("pp_is_resample_groups");
    return 0;
}

int is_resample_scheme_groups(const double* cdf, const float* values, int M, int n_per, int lo, int hi, int n_out, int scheme,
                              uint64_t seed, uint64_t offset, int64_t* index_out, float* value_out, hipStream_t st) {
    PP_CHECK_ARG(scheme == PP_RESAMPLE_MULTINOMIAL || scheme == PP_RESAMPLE_STRATIFIED || scheme == PP_RESAMPLE_SYSTEMATIC,
                 "pp_is_resample_scheme_groups: scheme is PP_RESAMPLE_MULTINOMIAL, _STRATIFIED or _SYSTEMATIC");
    if (scheme == PP_RESAMPLE_MULTINOMIAL)
        return is_resample_groups(cdf, values, M, n_per, lo, hi, n_out, seed, offset, index_out, value_out, st);
    PP_CHECK_ARG(cdf, "pp_is_resample_scheme_groups: null pointer (the cdf is required)");
    PP_CHECK_ARG(n_per >= 1 && M >= 0 && n_out >= 0, "pp_is_resample_scheme_groups: n_per >= 1, n_groups >= 0 and n_out >= 0");
    PP_CHECK_ARG(0 <= lo && lo < hi && hi <= n_per, "pp_is_resample_scheme_groups: an index range 0 <= lo < hi <= n_per");
    PP_CHECK_ARG(groups_count_ok(M, n_per) && groups_count_ok(M, n_out),
                 "pp_is_resample_scheme_groups: more than 2^31 - 1 particles or draws per call: shard the groups");
    PP_CHECK_ARG(index_out || value_out, "pp_is_resample_scheme_groups: index_out or value_out (or both)");
    PP_CHECK_ARG(!value_out || values, "pp_is_resample_scheme_groups: value_out needs the values");
    const int64_t outputs = (int64_t)M * n_out;
    if (outputs == 0) return 0;
    const int blocks = (int)std::min<int64_t>(RESAMPLE_BLOCKS, (outputs + 255) / 256);
    hipLaunchKernelGGL(resample_scheme_kernel, dim3(blocks), dim3(256), 0, st, cdf, values, n_per, lo, hi, n_out, outputs, scheme, seed,
                       offset, index_out, value_out);
    PP_LAUNCH_CHECK("pp_is_resample_scheme_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_cdf_workspace_bytes(int32_t n_groups, int32_t n_per) {
    if (n_groups < 0 || n_per < 1) return 0;
    pp::CdfWorkspace w;
    pp::cdf_carve(n_groups, n_per, nullptr, w);
    return w.bytes;
}

int pp_is_cdf_groups(const float* lw, int32_t n_groups, int32_t n_per, const double* stats, double* cdf_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return pp::is_cdf_groups(lw, n_groups, n_per, stats, cdf_out, workspace, workspace_bytes, pp::as_stream(stream));
}

int pp_is_resample_groups(const double* cdf, const float* values, int32_t n_groups, int32_t n_per, int32_t lo, int32_t hi,
                          int32_t n_out, uint64_t seed, uint64_t offset, int64_t* index_out, float* value_out, void* stream) {
    return pp::is_resample_groups(cdf, values, n_groups, n_per, lo, hi, n_out, seed, offset, index_out, value_out,
                                  pp::as_stream(stream));
}

int pp_is_resample_scheme_groups(const double* cdf, const float* values, int32_t n_groups, int32_t n_per, int32_t lo, int32_t hi,
                                 int32_t n_out, int32_t scheme, uint64_t seed, uint64_t offset, int64_t* index_out, float* value_out,
                                 void* stream) {
    return pp::is_resample_scheme_groups(cdf, values, n_groups, n_per, lo, hi, n_out, scheme, seed, offset, index_out, value_out,
                                         pp::as_stream(stream));
}

}  // extern "C"
