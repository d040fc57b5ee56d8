// Two-sample distances between two device-backed posteriors: the Kolmogorov-Smirnov statistic and where it is attained, the
// Wasserstein-1 and Wasserstein-2 distances and the energy distance of two weighted samples of a scalar, from the particles of both
// sides in value order with their cumulative weights (pp_is_sort_groups, then pp_is_cdf_groups over the sorted log-weights - what
// pp_is_quantile_groups takes). The reference compares posteriors by Distribution.kl_divergence against an analytic one; it has no
// distance between two Empiricals.
//
// All four are sums or maxima over the MERGE of two sorted sequences: of the values (the VALUE walk: F - G is constant between two
// merged values, so ks, W1 = int |F - G| and the energy distance 2 int (F - G)^2 are sums over the merged elements) and of the
// normalised cumulative weights u (the QUANTILE walk: both quantile functions are constant between two merged u, so
// W2^2 = int (F^-1 - G^-1)^2 is a sum over them). The definitions are in include/pyprob_amd.h.
//
// THE WORK SPLIT is a merge path, the same for both walks (one kernel template over the key). A workgroup of 256 threads owns TILE =
// 2048 consecutive MERGED positions of one group. Lanes 0 and 1 find where the tile's first and last diagonal cross the two sequences
// by binary search in global memory: the tile merges A[iA0, iA1) with B[jB0, jB1), 2048 elements in all. Both ranges, one element
// before and one after each (the state at the tile's start and the look-ahead of its last element), are staged into LDS ONCE as fp32
// value and fp64 u = fl(W / T): 2052 x 12 bytes. Every thread then finds its own 8-position diagonal by binary search in LDS and
// merges its eight elements serially, heads in LDS, sums in fp64 registers, the (|D|, position) maximum under the lexicographic order.
// The workgroup reduces by wave shuffles, then LDS in wave order. A group that fits one tile is finished by that launch; a longer one
// stores one record of 32 bytes per tile and a second launch, one workgroup per group, adds the records in tile order.
//
// BITS. The split depends on the keys alone and the shape of every sum on (ca, cb) alone: a tile past ca + cb holds zeros, and adding
// +0.0 to a sum of non-negative terms changes nothing, so neither n_per nor the number of groups enters - two calls give the same
// bits, and group g of an M-group call equals the one-group call on its slices. The maximum is order-independent by construction.
// No atomics, no workgroup waits for another, no scratch (build.py checks the resource remarks).
#include "is_groups.hpp"

#include <limits.h>

namespace pp {
namespace {

constexpr int TILE = PP_IS_TWOSAMPLE_TILE;      // merged positions per workgroup: 256 threads x PER_THREAD consecutive positions
constexpr int PER_THREAD = 8;
constexpr int STAGE = TILE + 4;                 // both ranges, a look-behind and a look-ahead each
constexpr int WIDTH = PP_IS_TWOSAMPLE_WIDTH;
static_assert(TILE == 256 * PER_THREAD, "a tile is 256 threads of eight merged positions");

// One side of one group: its sorted values, their cumulative weights, the counted particles and the last cumulative weight.
struct Side {
    const float* v;
    const double* w;
    int c;
    double total;
};
__device__ __forceinline__ Side side_of(const float* __restrict__ value, const double* __restrict__ cdf,
                                        const int* __restrict__ counted, int n_per, int64_t g) {
    Side s;
    s.v = value + g * n_per;
    s.w = cdf + g * n_per;
    s.c = max(0, min(counted[2 * g], n_per));
    s.total = s.c > 0 ? s.w[s.c - 1] : 0.0;
    return s;
}
__device__ __forceinline__ bool side_live(const Side& s) { return s.c > 0 && s.total > 0.0 && s.total < INFINITY; }

// What a tile leaves for the second launch.
struct Record {
    double s0, s1, best;
    int pos;
    float z;
};
static_assert(sizeof(Record) == 32, "a record is 32 bytes");

// The first i in [max(0, d - cb), min(d, ca)] whose A[i] is NOT among the first d merged elements (A before B on ties): the number
// of A's among them. ka / kb: the keys of the two sequences by position.
template <class KA, class KB>
__device__ __forceinline__ int merge_path(int d, int ca, int cb, KA ka, KB kb) {
    int lo = max(0, d - cb), hi = min(d, ca);
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ka(mid) <= kb(d - 1 - mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void take(double& best, int& pos, float& z, double d, int p, float at) {
    const bool t = d > best || (d == best && p < pos);
    best = t ? d : best;
    pos = t ? p : pos;
    z = t ? at : z;
}

// The workgroup's sums and maximum, valid in thread 0. LDS: 4 of each.
__device__ __forceinline__ void block_reduce(double& s0, double& s1, double& best, int& pos, float& z, double* sh0, double* sh1,
                                             double* shb, int* shp, float* shz) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
        const double d = __shfl_xor(best, o, 64);
        const int p = __shfl_xor(pos, o, 64);
        const float at = __shfl_xor(z, o, 64);
        take(best, pos, z, d, p, at);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh0[wave] = s0;
        sh1[wave] = s1;
        shb[wave] = best;
        shp[wave] = pos;
        shz[wave] = z;
    }
    __syncthreads();
    s0 = sh0[0];
    s1 = sh1[0];
    best = shb[0];
    pos = shp[0];
    z = shz[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        s0 += sh0[q];
        s1 += sh1[q];
        take(best, pos, z, shb[q], shp[q], shz[q]);
    }
}

// The row of group g from the reduced sums: the value walk writes everything but wasserstein2, the quantile walk that.
template <bool QUANTILE>
__device__ __forceinline__ void write_row(double* __restrict__ out, int64_t g, bool live, int ca, int cb, double s0, double s1,
                                          double best, int pos, float z) {
    double* r = out + g * WIDTH;
    if (QUANTILE) {
        r[3] = live ? sqrt(s0) : NAN;
        return;
    }
    r[0] = live ? best : NAN;
    r[1] = live ? (double)z : NAN;
    r[2] = live ? s0 : NAN;
    r[4] = live ? 2.0 * s1 : NAN;
    r[5] = (double)ca;
    r[6] = (double)cb;
    r[7] = live ? (double)pos : NAN;
}

// Workgroup (tile blockIdx.x, group g0 + blockIdx.y). T == 1: the group's row (its part of it). T > 1: one record to rec[g T + tile].
template <bool QUANTILE>
__global__ __launch_bounds__(256) void twosample_tile_kernel(const float* __restrict__ value_a, const double* __restrict__ cdf_a,
                                                             const int* __restrict__ counted_a, int na,
                                                             const float* __restrict__ value_b, const double* __restrict__ cdf_b,
                                                             const int* __restrict__ counted_b, int nb, int T, int g0,
                                                             double* __restrict__ out, Record* __restrict__ rec) {
    __shared__ float shv[STAGE];
    __shared__ double shu[STAGE];
    __shared__ int split[2];
    __shared__ double sh0[4], sh1[4], shb[4];
    __shared__ int shp[4];
    __shared__ float shz[4];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const Side A = side_of(value_a, cdf_a, counted_a, na, g), B = side_of(value_b, cdf_b, counted_b, nb, g);
    const bool live = side_live(A) && side_live(B);
    const int total = live ? A.c + B.c : 0;      // (n_per_a + n_per_b fits 31 bits: checked on the host)
    const int d0 = (int)min((int64_t)blockIdx.x * TILE, (int64_t)total), d1 = d0 + min(TILE, total - d0);
    const bool active = d0 < total;              // (uniform in the workgroup)
    double s0 = 0.0, s1 = 0.0, best = -1.0;
    int pos = INT_MAX;
    float z = 0.0f;
    if (active) {
        if (tid < 2) {
            const auto ka = [&](int i) { return QUANTILE ? __ddiv_rn(A.w[i], A.total) : (double)A.v[i]; };
            const auto kb = [&](int j) { return QUANTILE ? __ddiv_rn(B.w[j], B.total) : (double)B.v[j]; };
            split[tid] = merge_path(tid ? d1 : d0, A.c, B.c, ka, kb);
        }
        __syncthreads();
        const int iA0 = split[0], iA1 = split[1], jB0 = d0 - iA0, jB1 = d1 - iA1;
        const int nA = iA1 - iA0, nB = jB1 - jB0, offB = nA + 2;      // nA + nB = d1 - d0 <= TILE
        // slot t < nA + 2 holds A[iA0 - 1 + t], slot offB + t holds B[jB0 - 1 + t]; a position outside [0, c) holds (0, 0)
        for (int t = tid; t < nA + nB + 4; t += 256) {
            const bool a = t < offB;
            const Side& s = a ? A : B;
            const int idx = a ? iA0 - 1 + t : jB0 - 1 + (t - offB);
            const bool in = idx >= 0 && idx < s.c;
            shv[t] = in ? s.v[idx] : 0.0f;
            shu[t] = in ? __ddiv_rn(s.w[idx], s.total) : 0.0;
        }
        __syncthreads();
        const int dl = tid * PER_THREAD, cnt = min(PER_THREAD, d1 - d0 - dl);
        if (cnt > 0) {
            const int la = 1 - iA0, lb = offB + 1 - jB0;      // slot of A[i]: la + i; of B[j]: lb + j
            const auto key = [&](int slot) { return QUANTILE ? shu[slot] : (double)shv[slot]; };
            const int il = merge_path(dl, nA, nB, [&](int x) { return key(1 + x); }, [&](int x) { return key(offB + 1 + x); });
            int i = iA0 + il, j = jB0 + (dl - il);
            // the state before this thread's first element: the cumulative weights consumed so far (0 at the start of a side)
            double fa = shu[la + i - 1], fb = shu[lb + j - 1];
            double prev = fmax(fa, fb);
            for (int s = 0; s < cnt; ++s) {
                const bool more_a = i < A.c, more_b = j < B.c;
                const bool from_a = more_a && (!more_b || key(la + i) <= key(lb + j));
                if (QUANTILE) {
                    const double u = from_a ? shu[la + i] : shu[lb + j];
                    const float x = shv[la + min(i, A.c - 1)], y = shv[lb + min(j, B.c - 1)];
                    if (u > prev) {
                        const double diff = x == y ? 0.0 : (double)x - (double)y;
                        s0 += (u - prev) * (diff * diff);
                    }
                    prev = u;
                    i += from_a ? 1 : 0;
                    j += from_a ? 0 : 1;
                } else {
                    const float at = from_a ? shv[la + i] : shv[lb + j];
                    fa = from_a ? shu[la + i] : fa;
                    fb = from_a ? fb : shu[lb + j];
                    i += from_a ? 1 : 0;
                    j += from_a ? 0 : 1;
                    const bool next_a = i < A.c, next_b = j < B.c;
                    const float ha = shv[la + i], hb = shv[lb + j];
                    const float next = next_a ? ((next_b && hb < ha) ? hb : ha) : hb;
                    const bool any = next_a || next_b, step = any && next > at;
                    const double D = fa - fb, absD = fabs(D);
                    if (!any || step) take(best, pos, z, absD, d0 + dl + s, at);
                    if (step && D != 0.0) {
                        const double gap = (double)next - (double)at;
                        s0 += absD * gap;
                        s1 += D * D * gap;
                    }
                }
            }
        }
    }
    block_reduce(s0, s1, best, pos, z, sh0, sh1, shb, shp, shz);
    if (tid == 0) {
        if (T == 1) {
            write_row<QUANTILE>(out, g, live, A.c, B.c, s0, s1, best, pos, z);
        } else {
            Record* r = rec + g * T + blockIdx.x;
            r->s0 = s0;
            r->s1 = s1;
            r->best = best;
            r->pos = pos;
            r->z = z;
        }
    }
}

// Groups of more than one tile: workgroup g0 + blockIdx.x adds the T records of its group, each thread taking records tid,
// tid + 256, ... in tile order.
template <bool QUANTILE>
__global__ __launch_bounds__(256) void twosample_reduce_kernel(const float* __restrict__ value_a, const double* __restrict__ cdf_a,
                                                               const int* __restrict__ counted_a, int na,
                                                               const float* __restrict__ value_b, const double* __restrict__ cdf_b,
                                                               const int* __restrict__ counted_b, int nb, int T, int g0,
                                                               const Record* __restrict__ rec, double* __restrict__ out) {
    __shared__ double sh0[4], sh1[4], shb[4];
    __shared__ int shp[4];
    __shared__ float shz[4];
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const Side A = side_of(value_a, cdf_a, counted_a, na, g), B = side_of(value_b, cdf_b, counted_b, nb, g);
    const Record* r = rec + g * T;
    double s0 = 0.0, s1 = 0.0, best = -1.0;
    int pos = INT_MAX;
    float z = 0.0f;
    for (int t = threadIdx.x; t < T; t += 256) {
        s0 += r[t].s0;
        s1 += r[t].s1;
        take(best, pos, z, r[t].best, r[t].pos, r[t].z);
    }
    block_reduce(s0, s1, best, pos, z, sh0, sh1, shb, shp, shz);
    if (threadIdx.x == 0) write_row<QUANTILE>(out, g, side_live(A) && side_live(B), A.c, B.c, s0, s1, best, pos, z);
}

inline bool twosample_shape_ok(int M, int na, int nb) {
    return groups_shape_ok(M, na) && groups_shape_ok(M, nb) && (int64_t)na + nb <= 0x7fffffff;
}
struct TwoSampleWorkspace {
    Record* rec;
    size_t bytes;
};
void twosample_carve(int M, int na, int nb, void* p, TwoSampleWorkspace& w) {
    Carver c(p);
    const int T = tiles_of(std::max(na, 1) + std::max(nb, 1), TILE);
    w.rec = c.take<Record>(T > 1 ? (int64_t)std::max(M, 0) * T * (int64_t)sizeof(Record) : 0);
    w.bytes = c.bytes();
}

template <bool QUANTILE>
void twosample_walk(const float* va, const double* wa, const int* ca, int na, const float* vb, const double* wb, const int* cb, int nb,
                    int M, int T, double* out, Record* rec, hipStream_t st) {
    for_each_group_chunk(M, [&](int g0, int groups) {
        hipLaunchKernelGGL(twosample_tile_kernel<QUANTILE>, dim3(T, groups), dim3(256), 0, st, va, wa, ca, na, vb, wb, cb, nb, T, g0,
                           out, rec);
        if (T > 1)
            hipLaunchKernelGGL(twosample_reduce_kernel<QUANTILE>, dim3(groups), dim3(256), 0, st, va, wa, ca, na, vb, wb, cb, nb, T, g0,
                               (const Record*)rec, out);
    });
}

}  // namespace

int is_twosample_groups(const float* va, const double* wa, const int* ca, int na, const float* vb, const double* wb, const int* cb,
                        int nb, int M, double* out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(va && wa && ca && vb && wb && cb && out && ws,
                 "pp_is_twosample_groups: null pointer (the sorted values, their cdf and the counts of both sides, out and the "
                 "workspace are required)");
    PP_CHECK_ARG(na >= 1 && nb >= 1 && M >= 0, "pp_is_twosample_groups: n_per_a >= 1, n_per_b >= 1 and n_groups >= 0");
    PP_CHECK_ARG(twosample_shape_ok(M, na, nb),
                 "pp_is_twosample_groups: more than 2^31 - 1 particles per call or per pair of groups: shard the groups");
    TwoSampleWorkspace w;
    twosample_carve(M, na, nb, ws, w);
    PP_CHECK_WORKSPACE("pp_is_twosample_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(na + nb, TILE);
    // (the quantile walk reuses the records of the value walk: the launches are dependent on the caller's stream)
    twosample_walk<false>(va, wa, ca, na, vb, wb, cb, nb, M, T, out, w.rec, st);
    twosample_walk<true>(va, wa, ca, na, vb, wb, cb, nb, M, T, out, w.rec, st);
    PP_LAUNCH_CHECK("pp_is_twosample_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_twosample_workspace_bytes(int32_t n_groups, int32_t n_per_a, int32_t n_per_b) {
    if (!pp::twosample_shape_ok(n_groups, n_per_a, n_per_b)) return 0;
    pp::TwoSampleWorkspace w;
    pp::twosample_carve(n_groups, n_per_a, n_per_b, nullptr, w);
    return w.bytes;
}

int pp_is_twosample_groups(const float* value_a, const double* cdf_a, const int32_t* counted_a, int32_t n_per_a, const float* value_b,
                           const double* cdf_b, const int32_t* counted_b, int32_t n_per_b, int32_t n_groups, double* out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_twosample_groups(value_a, cdf_a, counted_a, n_per_a, value_b, cdf_b, counted_b, n_per_b, n_groups, out, workspace,
                                   workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
