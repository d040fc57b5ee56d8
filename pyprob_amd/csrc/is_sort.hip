// Order statistics of a (batched) lock-step posterior call on the device: a segmented, stable key-value sort of every group's
// particles by value, the inverted-cdf quantile over the sorted particles, and the distinct values with their masses.
//
// The reference answers a weighted median by resampling 1000 values on the host (pyprob/distributions/empirical.py:714-728) and
// combines duplicates by one host pass over all values per distinct value (combine_duplicates, :809-834). Here
//   pp_is_sort_groups      writes, per group of n_per particles, the stable ascending order of the particles by a 32-bit key of
//       x (value_out, lw_out, index_out) and the two counts of counted_out;
//   pp_is_quantile_groups  searches the cumulative weights of the sorted particles (pp_is_cdf_groups over lw_out) for q T;
//   pp_is_unique_groups    reduces every run of equal keys to (value, fixed-point mass, particle count); the mass is the
//       histogram's (is_groups.hpp: which particles count, the clamped weight and the shift).
//
// SHAPE OF THE SORT. A least-significant-digit radix sort with 8-bit digits, four passes. A workgroup of 256 threads takes a tile of
// up to 2048 particles; wave w owns the consecutive positions [w seg, (w + 1) seg) of it and walks them 64 at a time, so "position
// order" is (wave, round, lane). In a round the lanes with the same digit find each other with eight ballots; a lane's rank among
// them is the population count of the lower peers, and the lowest peer advances the wave's running count of that digit in LDS. A
// particle's destination is (particles of lower digits) + (same digit in earlier tiles) + (same digit in earlier waves of the tile)
// + (same digit earlier in the wave): every term counts particles BEFORE it in position order, which is what makes a pass stable.
// A group of one tile runs the four passes in LDS in one launch. A longer group takes, per pass, three dependent launches on the
// caller's stream: per-tile digit counts (integer LDS adds), one workgroup per group that turns the (tile, digit) counts into
// exclusive offsets, and the scatter into the other of two buffers in the workspace. No global atomics, no workgroup waits for
// another inside a kernel. Every output is a function of the keys alone: two identical calls give the same bits and group g of an
// M-group call carries the bits of the one-group call on its slice.
#include "is_groups.hpp"

namespace pp {
namespace {

constexpr int THREADS = 256, PER_THREAD = 8, TILE = THREADS * PER_THREAD;      // 2048 particles per workgroup
static_assert(TILE == PP_IS_SORT_TILE, "a tile is 256 threads of eight particles");
constexpr int DIGITS = 256;
constexpr uint32_t EXCLUDED = 0xFFFFFFFFu;


// The key of a particle: EXCLUDED where the log-weight is not finite or x is NaN, else the order-preserving map of the bits of x
// (-0.0 first made +0.0). No value maps to EXCLUDED: that would take the bits of a NaN.
__device__ __forceinline__ uint32_t sort_key(float lw, float x) {
    if (!isfinite(lw) || x != x) return EXCLUDED;
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int wave_inclusive(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Exclusive sum of v over the 256 threads in thread order, and the total. shw: four ints of LDS (synchronised here).
__device__ __forceinline__ int block_exclusive(int v, int* shw, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_inclusive(v);
    __syncthreads();
    if (lane == 63) shw[wave] = inc;
    __syncthreads();
    int off = 0;
    for (int q = 0; q < wave; ++q) off += shw[q];
    total = shw[0] + shw[1] + shw[2] + shw[3];
    return off + inc - v;
}

// One round of one wave: every lane holds a digit; returns the number of particles with that digit earlier in the wave's
// segment (earlier rounds from the running count `cnt` of this wave, this round from the lower lanes) and advances the count.
__device__ __forceinline__ int wave_rank(int digit, int* cnt) {
    const int lane = threadIdx.x & 63;
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    const int lower = __popcll(peers & ((1ull << lane) - 1ull));
    const int old = cnt[digit];
    __builtin_amdgcn_wave_barrier();
    if (lower == 0) cnt[digit] = old + __popcll(peers);      // (one lane per digit, and the wave's own row: no atomic)
    __builtin_amdgcn_wave_barrier();
    return old + lower;
}

// ---- groups of one tile: the whole sort in LDS ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void sort_small_kernel(const float* __restrict__ lw, const float* __restrict__ x, int n_per,
                                                             int g0, float* __restrict__ value_out, float* __restrict__ lw_out,
                                                             int* __restrict__ index_out, int* __restrict__ counted_out) {
    __shared__ uint32_t skey[2][TILE];
    __shared__ uint16_t sidx[2][TILE];
    __shared__ int cnt[4][DIGITS];
    __shared__ int base[4][DIGITS];
    __shared__ int shw[4];
    __shared__ int shc[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    const int64_t b = g * n_per;
    const int R = (n_per + THREADS - 1) / THREADS;      // rounds: 1 .. 8
    const int seg = 64 * R, P = THREADS * R;            // (positions n_per .. P - 1 are padding: EXCLUDED, last in position order)
    if (tid < 2) shc[tid] = 0;
    __syncthreads();
    int real = 0, nanx = 0;
    for (int p = tid; p < P; p += THREADS) {
        uint32_t k = EXCLUDED;
        if (p < n_per) {
            const float a = lw[b + p], v = x[b + p];
            k = sort_key(a, v);
            real += k != EXCLUDED;
            nanx += isfinite(a) && v != v;
        }
        skey[0][p] = k;
        sidx[0][p] = (uint16_t)p;
    }
    if (real) atomicAdd(&shc[0], real);
    if (nanx) atomicAdd(&shc[1], nanx);
    int cur = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
#pragma unroll
        for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
        __syncthreads();
        uint32_t key[PER_THREAD];
        uint16_t id[PER_THREAD];
        int rank[PER_THREAD];
#pragma unroll
        for (int r = 0; r < PER_THREAD; ++r) {
            if (r < R) {
                const int p = wave * seg + r * 64 + lane;
                key[r] = skey[cur][p];
                id[r] = sidx[cur][p];
                rank[r] = wave_rank((int)((key[r] >> shift) & 255u), cnt[wave]);
            }
        }
        __syncthreads();
        {
            const int c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid], c3 = cnt[3][tid];
            int total;
            const int ex = block_exclusive(c0 + c1 + c2 + c3, shw, total);
            base[0][tid] = ex;
            base[1][tid] = ex + c0;
            base[2][tid] = ex + c0 + c1;
            base[3][tid] = ex + c0 + c1 + c2;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PER_THREAD; ++r) {
            if (r < R) {
                const int dest = base[wave][(key[r] >> shift) & 255u] + rank[r];
                if (dest < P) {      // (always: the destinations are a permutation of 0 .. P - 1)
                    skey[cur ^ 1][dest] = key[r];
                    sidx[cur ^ 1][dest] = id[r];
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int p = tid; p < n_per; p += THREADS) {
        const int i = min((int)sidx[cur][p], n_per - 1);      // (always below n_per: the padding sorts last)
        index_out[b + p] = i;
        value_out[b + p] = x[b + i];
        lw_out[b + p] = lw[b + i];
    }
    if (tid < 2) counted_out[2 * g + tid] = shc[tid];
}

// ---- longer groups: count, offsets, scatter per pass ------------------------------------------------------------------------
// Workgroup (tile blockIdx.x, group g0 + blockIdx.y) stores the number of its particles per digit at hist[(g T + tile) 256 + d];
// the first pass forms the keys from (lw, x) and stores the tile's two counts.
template <bool FIRST>
__global__ __launch_bounds__(THREADS) void sort_count_kernel(const float* __restrict__ lw, const float* __restrict__ x,
                                                             const uint32_t* __restrict__ keys, int n_per, int T, int g0, int shift,
                                                             int* __restrict__ hist, int* __restrict__ tilecnt) {
    __shared__ int h[DIGITS];
    __shared__ int shc[2];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t b = g * n_per;
    h[tid] = 0;
    if (tid < 2) shc[tid] = 0;
    __syncthreads();
    int real = 0, nanx = 0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = (int64_t)blockIdx.x * TILE + k * THREADS + tid;
        if (i < n_per) {
            uint32_t key;
            if (FIRST) {
                const float a = lw[b + i], v = x[b + i];
                key = sort_key(a, v);
                real += key != EXCLUDED;
                nanx += isfinite(a) && v != v;
            } else {
                key = keys[b + i];
            }
            atomicAdd(&h[(key >> shift) & 255u], 1);
        }
    }
    if (FIRST) {
        if (real) atomicAdd(&shc[0], real);
        if (nanx) atomicAdd(&shc[1], nanx);
    }
    __syncthreads();
    const int64_t t = g * T + blockIdx.x;
    hist[t * DIGITS + tid] = h[tid];
    if (FIRST && tid < 2) tilecnt[2 * t + tid] = shc[tid];
}

// One workgroup per group: hist[g, tile, d] becomes the number of particles of digit d in the tiles before `tile`, dbase[g, d] the
// number of particles of the group with a lower digit. Thread d walks its column in tile order. The first pass adds up counted_out.
__global__ __launch_bounds__(THREADS) void sort_scan_kernel(int* __restrict__ hist, int* __restrict__ dbase, int T, int g0,
                                                            const int* __restrict__ tilecnt, int* __restrict__ counted_out) {
    __shared__ int shw[4];
    __shared__ int shc[2];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    int* col = hist + g * T * DIGITS + tid;
    int run = 0;
    int t = 0;
    for (; t + 8 <= T; t += 8) {      // (eight loads in flight)
        int c[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) c[q] = col[(int64_t)(t + q) * DIGITS];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            col[(int64_t)(t + q) * DIGITS] = run;
            run += c[q];
        }
    }
    for (; t < T; ++t) {
        const int c = col[(int64_t)t * DIGITS];
        col[(int64_t)t * DIGITS] = run;
        run += c;
    }
    int total;
    dbase[g * DIGITS + tid] = block_exclusive(run, shw, total);
    if (tilecnt) {
        if (tid < 2) shc[tid] = 0;
        __syncthreads();
        int real = 0, nanx = 0;
        for (int q = tid; q < T; q += THREADS) {
            real += tilecnt[2 * (g * T + q)];
            nanx += tilecnt[2 * (g * T + q) + 1];
        }
        if (real) atomicAdd(&shc[0], real);
        if (nanx) atomicAdd(&shc[1], nanx);
        __syncthreads();
        if (tid < 2) counted_out[2 * g + tid] = shc[tid];
    }
}

// Workgroup (tile, group) moves its particles to their places of this pass. FIRST forms the keys and the indices, LAST writes the
// outputs instead of the buffers.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(THREADS) void sort_scatter_kernel(const float* __restrict__ lw, const float* __restrict__ x,
                                                               const uint32_t* __restrict__ keys_in, const int* __restrict__ idx_in,
                                                               int n_per, int T, int g0, int shift, const int* __restrict__ hist,
                                                               const int* __restrict__ dbase, uint32_t* __restrict__ keys_out,
                                                               int* __restrict__ idx_out, float* __restrict__ value_out,
                                                               float* __restrict__ lw_out, int* __restrict__ index_out) {
    __shared__ int cnt[4][DIGITS];
    __shared__ int base[4][DIGITS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t b = g * n_per;
#pragma unroll
    for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
    __syncthreads();
    uint32_t key[PER_THREAD];
    int id[PER_THREAD], rank[PER_THREAD];
    // (all loads first; a position at or beyond n_per is padding of the group's last tile: EXCLUDED, after every particle)
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        const int64_t i = (int64_t)blockIdx.x * TILE + wave * (64 * PER_THREAD) + r * 64 + lane;
        key[r] = EXCLUDED;
        id[r] = -1;
        if (i < n_per) {
            if (FIRST) {
                key[r] = sort_key(lw[b + i], x[b + i]);
                id[r] = (int)i;
            } else {
                key[r] = keys_in[b + i];
                id[r] = idx_in[b + i];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) rank[r] = wave_rank((int)((key[r] >> shift) & 255u), cnt[wave]);
    __syncthreads();
    {
        const int c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid];
        const int ex = dbase[g * DIGITS + tid] + hist[(g * T + blockIdx.x) * DIGITS + tid];
        base[0][tid] = ex;
        base[1][tid] = ex + c0;
        base[2][tid] = ex + c0 + c1;
        base[3][tid] = ex + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        if (id[r] < 0) continue;
        const int dest = base[wave][(key[r] >> shift) & 255u] + rank[r];
        if (dest >= n_per || id[r] >= n_per) continue;      // (never: the destinations of a group are a permutation of 0 .. n_per - 1)
        if (LAST) {
            index_out[b + dest] = id[r];
            value_out[b + dest] = x[b + id[r]];
            lw_out[b + dest] = lw[b + id[r]];
        } else {
            keys_out[b + dest] = key[r];
            idx_out[b + dest] = id[r];
        }
    }
}

// Workspace of the sort: nothing for groups of one tile; else two key and two index buffers of M n_per words, the (tile, digit)
// counts, the digit offsets of every group and the two counts of every tile.
struct SortWorkspace {
    uint32_t *keys_a, *keys_b;
    int *idx_a, *idx_b, *hist, *dbase, *tilecnt;
    size_t bytes;
};
void sort_carve(int M, int n_per, void* p, SortWorkspace& w) {
    Carver c(p);
    const int T = tiles_of(std::max(n_per, 1), TILE);
    const int64_t m = std::max(M, 0);
    const bool big = T > 1;
    const int64_t words = big ? m * n_per * 4 : 0;
    w.keys_a = c.take<uint32_t>(words);
    w.keys_b = c.take<uint32_t>(words);
    w.idx_a = c.take<int>(words);
    w.idx_b = c.take<int>(words);
    w.hist = c.take<int>(big ? m * T * DIGITS * 4 : 0);
    w.dbase = c.take<int>(big ? m * DIGITS * 4 : 0);
    w.tilecnt = c.take<int>(big ? m * T * 8 : 0);
    w.bytes = c.bytes();
}

// ---- quantile ------------------------------------------------------------------------------------------------------------------
// One thread per (group, q).
__global__ __launch_bounds__(256) void quantile_kernel(const float* __restrict__ value, const double* __restrict__ cdf,
                                                       const int* __restrict__ counted, int n_per, int n_q, int64_t outputs,
                                                       const double* __restrict__ q, double* __restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= outputs) return;
    const int64_t g = o / n_q;
    const int c = min(counted[2 * g], n_per);
    double r = NAN;
    if (c > 0) {
        const double* cd = cdf + g * n_per;
        const double total = cd[c - 1];
        if (total > 0.0 && total < INFINITY) {
            const double t = __dmul_rn(q[o - g * n_q], total);
            int a = 0, e = c;      // the first i in [0, c] with cdf[i] >= t (t > 0) or cdf[i] > 0 (else); c: none
            const bool strict = t > 0.0;
            while (a < e) {
                const int mid = a + ((e - a) >> 1);
                const double v = cd[mid];
                if (strict ? v < t : v <= 0.0) a = mid + 1;
                else e = mid;
            }
            r = (double)value[g * n_per + min(a, c - 1)];
        }
    }
    out[o] = r;
}

// ---- distinct values ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t value_key(float x) {
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return b;      // (equal keys <=> equal bits after -0.0 -> +0.0: the map of sort_key is one to one)
}

// Thread `tid` of tile blockIdx.x owns the eight consecutive particles from first = tile TILE + 8 tid. head[k]: the particle is
// among the first c counted ones and begins a run (its key differs from the one before it, or it is particle 0).
__device__ __forceinline__ int load_heads(const float* __restrict__ v, int64_t first, int c, float (&val)[PER_THREAD],
                                          bool (&head)[PER_THREAD]) {
    float prev = (first > 0 && first - 1 < c) ? v[first - 1] : 0.0f;
    int heads = 0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + k;
        val[k] = i < c ? v[i] : 0.0f;
        head[k] = i < c && (i == 0 || value_key(val[k]) != value_key(prev));
        heads += head[k];
        prev = val[k];
    }
    return heads;
}

// Step 1: the number of runs that begin in tile (blockIdx.x) of group g0 + blockIdx.y, and (no statistics given) the maximum of the
// tile's finite log-weights - over all n_per particles, as the histogram takes it.
__global__ __launch_bounds__(THREADS) void unique_count_kernel(const float* __restrict__ value, const float* __restrict__ lw,
                                                               const int* __restrict__ counted, int n_per, int T, int g0,
                                                               int* __restrict__ heads, float* __restrict__ tmax) {
    __shared__ int shw[4];
    __shared__ float shmax[4];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int c = min(counted[2 * g], n_per);
    const int64_t first = (int64_t)blockIdx.x * TILE + (int64_t)tid * PER_THREAD;
    float val[PER_THREAD];
    bool head[PER_THREAD];
    const int mine = load_heads(value + g * n_per, first, c, val, head);
    int total;
    block_exclusive(mine, shw, total);
    if (tid == 0) heads[g * T + blockIdx.x] = total;
    if (tmax) {
        float a[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) a[k] = first + k < n_per ? lw[g * n_per + first + k] : -INFINITY;
        const float m = block_max<THREADS>(finite_max(a), shmax);
        if (tid == 0) tmax[g * T + blockIdx.x] = m;
    }
}

// Step 2: one workgroup per group. first_run[g, t] = the number of runs that begin before tile t, runs_out[g] their number, and
// gmax[g] the maximum of the tile maxima.
__global__ __launch_bounds__(THREADS) void unique_offsets_kernel(const int* __restrict__ heads, int* __restrict__ first_run, int T,
                                                                 int g0, const float* __restrict__ tmax, double* __restrict__ gmax,
                                                                 int* __restrict__ runs_out) {
    __shared__ int shw[4];
    __shared__ float shmax[4];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.x;
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += THREADS) {
        const int t = t0 + tid;
        const int h = t < T ? heads[g * T + t] : 0;
        int total;
        const int ex = block_exclusive(h, shw, total);
        if (t < T) first_run[g * T + t] = carry + ex;
        carry += total;
    }
    if (tid == 0) runs_out[g] = carry;
    if (tmax) {
        float m = tiles_max<THREADS>(tmax, g, T);
        __syncthreads();
        m = block_max<THREADS>(m, shmax);
        if (tid == 0) gmax[g] = (double)m;
    }
}

// Step 3: the tile adds up its runs in LDS (integer adds: no order). Local run 0 is what lies before the tile's first head - the
// tail of a run that began in an earlier tile - and goes to lead[g, t]; local run r >= 1 is run first_run[g, t] + r - 1 of the group.
__global__ __launch_bounds__(THREADS) void unique_reduce_kernel(const float* __restrict__ value, const float* __restrict__ lw,
                                                                const int* __restrict__ counted, int n_per, int T, int g0,
                                                                const double* __restrict__ stats, const double* __restrict__ gmax,
                                                                double scale, const int* __restrict__ first_run,
                                                                float* __restrict__ value_out, int64_t* __restrict__ mass_out,
                                                                int* __restrict__ count_out, int64_t* __restrict__ lead_mass,
                                                                int* __restrict__ lead_count) {
    __shared__ unsigned long long smass[TILE + 1];
    __shared__ unsigned int scount[TILE + 1];
    __shared__ int shw[4];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int64_t b = g * n_per;
    const int c = min(counted[2 * g], n_per);
    const int64_t first = (int64_t)blockIdx.x * TILE + (int64_t)tid * PER_THREAD;
    for (int s = tid; s <= TILE; s += THREADS) {
        smass[s] = 0;
        scount[s] = 0;
    }
    float val[PER_THREAD];
    bool head[PER_THREAD];
    const int mine = load_heads(value + b, first, c, val, head);
    int total;
    int local = block_exclusive(mine, shw, total);      // (the syncs inside also publish the zeroed rows)
    const double M = stats ? stats[6 * g] : gmax[g];
    const bool any = group_any(M);
    const int run0 = first_run[g * T + blockIdx.x];
    unsigned long long acc = 0;
    unsigned int n = 0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int64_t i = first + k;
        if (i >= c) break;
        if (head[k]) {
            if (n) {
                atomicAdd(&smass[local], acc);
                atomicAdd(&scount[local], n);
            }
            acc = 0;
            n = 0;
            ++local;
            value_out[b + run0 + local - 1] = val[k];
        }
        acc += fixed_mass(particle_weight_clamped(lw[b + i], M, any), scale);
        ++n;
    }
    if (n) {
        atomicAdd(&smass[local], acc);
        atomicAdd(&scount[local], n);
    }
    __syncthreads();
    for (int s = tid + 1; s <= total; s += THREADS) {
        mass_out[b + run0 + s - 1] = (int64_t)smass[s];
        count_out[b + run0 + s - 1] = (int)scount[s];
    }
    if (tid == 0) {
        lead_mass[g * T + blockIdx.x] = (int64_t)smass[0];
        lead_count[g * T + blockIdx.x] = (int)scount[0];
    }
}

// Step 4 (groups of more than one tile): one thread per tile in which a run begins adds to the tile's LAST run what the following
// tiles hold of it - their leading parts, up to and including the first tile in which another run begins. Every run is completed
// by one thread.
__global__ __launch_bounds__(THREADS) void unique_stitch_kernel(const int* __restrict__ heads, const int* __restrict__ first_run,
                                                                const int64_t* __restrict__ lead_mass,
                                                                const int* __restrict__ lead_count, int n_per, int T, int g0,
                                                                int64_t* __restrict__ mass_out, int* __restrict__ count_out) {
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int h = heads[g * T + t];
    if (h == 0) return;
    int64_t mass = 0;
    int n = 0;
    for (int j = t + 1; j < T; ++j) {
        mass += lead_mass[g * T + j];
        n += lead_count[g * T + j];
        if (heads[g * T + j] > 0) break;
    }
    if (n) {
        const int64_t r = g * n_per + first_run[g * T + t] + h - 1;
        mass_out[r] += mass;
        count_out[r] += n;
    }
}

struct UniqueWorkspace {
    int *heads, *first_run, *lead_count;
    float* tmax;
    double* gmax;
    int64_t* lead_mass;
    size_t bytes;
};
void unique_carve(int M, int n_per, void* p, UniqueWorkspace& w) {
    Carver c(p);
    const int64_t tiles = (int64_t)std::max(M, 0) * tiles_of(std::max(n_per, 1), TILE);
    w.heads = c.take<int>(tiles * 4);
    w.first_run = c.take<int>(tiles * 4);
    w.lead_count = c.take<int>(tiles * 4);
    w.tmax = c.take<float>(tiles * 4);
    w.gmax = c.take<double>((int64_t)std::max(M, 0) * 8);
    w.lead_mass = c.take<int64_t>(tiles * 8);
    w.bytes = c.bytes();
}

}  // namespace

int is_sort_groups(const float* lw, const float* x, int M, int n_per, const double* stats, float* value_out, float* lw_out,
                   int* index_out, int* counted_out, void* ws, size_t ws_bytes, hipStream_t st) {
    (void)stats;      // (the keys do not depend on the weights' maximum: with and without it the same bits)
    PP_CHECK_ARG(lw && x && value_out && lw_out && index_out && counted_out && ws,
                 "pp_is_sort_groups: null pointer (lw, x, the four outputs and the workspace are required)");
    PP_CHECK_GROUPS("pp_is_sort_groups", M, n_per);
    SortWorkspace w;
    sort_carve(M, n_per, ws, w);
    PP_CHECK_WORKSPACE("pp_is_sort_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(n_per, TILE);
    for_each_group_chunk(M, [&](int g0, int groups) {
        if (T == 1) {
            hipLaunchKernelGGL(sort_small_kernel, dim3(groups), dim3(THREADS), 0, st, lw, x, n_per, g0, value_out, lw_out, index_out,
                               counted_out);
            return;
        }
        const dim3 tiles(T, groups);
        // pass 0: (lw, x) -> a; pass 1: a -> b; pass 2: b -> a; pass 3: a -> the outputs
        hipLaunchKernelGGL(sort_count_kernel<true>, tiles, dim3(THREADS), 0, st, lw, x, (const uint32_t*)nullptr, n_per, T, g0, 0, w.hist,
                           w.tilecnt);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(groups), dim3(THREADS), 0, st, w.hist, w.dbase, T, g0, (const int*)w.tilecnt,
                           counted_out);
        hipLaunchKernelGGL((sort_scatter_kernel<true, false>), tiles, dim3(THREADS), 0, st, lw, x, (const uint32_t*)nullptr,
                           (const int*)nullptr, n_per, T, g0, 0, (const int*)w.hist, (const int*)w.dbase, w.keys_a, w.idx_a,
                           (float*)nullptr, (float*)nullptr, (int*)nullptr);
        for (int pass = 1; pass < 4; ++pass) {
            const uint32_t* kin = pass == 2 ? w.keys_b : w.keys_a;
            const int* iin = pass == 2 ? w.idx_b : w.idx_a;
            uint32_t* kout = pass == 2 ? w.keys_a : w.keys_b;
            int* iout = pass == 2 ? w.idx_a : w.idx_b;
            hipLaunchKernelGGL(sort_count_kernel<false>, tiles, dim3(THREADS), 0, st, lw, x, kin, n_per, T, g0, 8 * pass, w.hist,
                               (int*)nullptr);
            hipLaunchKernelGGL(sort_scan_kernel, dim3(groups), dim3(THREADS), 0, st, w.hist, w.dbase, T, g0, (const int*)nullptr,
                               (int*)nullptr);
            if (pass < 3)
                hipLaunchKernelGGL((sort_scatter_kernel<false, false>), tiles, dim3(THREADS), 0, st, lw, x, kin, iin, n_per, T, g0,
                                   8 * pass, (const int*)w.hist, (const int*)w.dbase, kout, iout, (float*)nullptr, (float*)nullptr,
                                   (int*)nullptr);
            else
                hipLaunchKernelGGL((sort_scatter_kernel<false, true>), tiles, dim3(THREADS), 0, st, lw, x, kin, iin, n_per, T, g0,
                                   8 * pass, (const int*)w.hist, (const int*)w.dbase, (uint32_t*)nullptr, (int*)nullptr, value_out,
                                   lw_out, index_out);
        }
    });
    PP_LAUNCH_CHECK("pp_is_sort_groups");
    return 0;
}

int is_quantile_groups(const float* value, const double* cdf, const int* counted, int M, int n_per, const double* q, int n_q,
                       double* out, hipStream_t st) {
    PP_CHECK_ARG(value && cdf && counted && q && out,
                 "pp_is_quantile_groups: null pointer (the sorted values, their cdf, the counts, q and out are required)");
    PP_CHECK_ARG(n_per >= 1 && M >= 0 && n_q >= 0, "pp_is_quantile_groups: n_per >= 1, n_groups >= 0 and n_q >= 0");
    PP_CHECK_ARG(groups_count_ok(M, n_per) && groups_count_ok(M, n_q),
                 "pp_is_quantile_groups: more than 2^31 - 1 particles or results per call: shard the groups");
    const int64_t outputs = (int64_t)M * n_q;
    if (outputs == 0) return 0;
    hipLaunchKernelGGL(quantile_kernel, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, st, value, cdf, counted, n_per, n_q,
                       outputs, q, out);
    PP_LAUNCH_CHECK("pp_is_quantile_groups");
    return 0;
}

int is_unique_groups(const float* value, const float* lw, const int* counted, int M, int n_per, const double* stats,
                     float* value_out, int64_t* mass_out, int* count_out, int* runs_out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(value && lw && counted && value_out && mass_out && count_out && runs_out && ws,
                 "pp_is_unique_groups: null pointer (the sorted values and log-weights, the counts, the four outputs and the "
                 "workspace are required)");
    PP_CHECK_GROUPS("pp_is_unique_groups", M, n_per);
    UniqueWorkspace w;
    unique_carve(M, n_per, ws, w);
    PP_CHECK_WORKSPACE("pp_is_unique_groups", ws_bytes, w.bytes);
    if (M == 0) return 0;
    const int T = tiles_of(n_per, TILE);
    const double scale = hist_scale(n_per);
    float* tmax = stats ? nullptr : w.tmax;
    for_each_group_chunk(M, [&](int g0, int groups) {
        const dim3 tiles(T, groups);
        hipLaunchKernelGGL(unique_count_kernel, tiles, dim3(THREADS), 0, st, value, lw, counted, n_per, T, g0, w.heads, tmax);
        hipLaunchKernelGGL(unique_offsets_kernel, dim3(groups), dim3(THREADS), 0, st, (const int*)w.heads, w.first_run, T, g0,
                           (const float*)tmax, w.gmax, runs_out);
        hipLaunchKernelGGL(unique_reduce_kernel, tiles, dim3(THREADS), 0, st, value, lw, counted, n_per, T, g0, stats,
                           (const double*)w.gmax, scale, (const int*)w.first_run, value_out, mass_out, count_out, w.lead_mass,
                           w.lead_count);
        if (T > 1)
            hipLaunchKernelGGL(unique_stitch_kernel, dim3(cdiv(T, THREADS), groups), dim3(THREADS), 0, st, (const int*)w.heads,
                               (const int*)w.first_run, (const int64_t*)w.lead_mass, (const int*)w.lead_count, n_per, T, g0, mass_out,
                               count_out);
    });
    PP_LAUNCH_CHECK("pp_is_unique_groups");
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_is_sort_workspace_bytes(int32_t n_groups, int32_t n_per) {
    if (!pp::groups_shape_ok(n_groups, n_per)) return 0;
    pp::SortWorkspace w;
    pp::sort_carve(n_groups, n_per, nullptr, w);
    return w.bytes;
}

int pp_is_sort_groups(const float* lw, const float* x, int32_t n_groups, int32_t n_per, const double* stats, float* value_out,
                      float* lw_out, int32_t* index_out, int32_t* counted_out, void* workspace, size_t workspace_bytes,
                      void* stream) {
    return pp::is_sort_groups(lw, x, n_groups, n_per, stats, value_out, lw_out, index_out, counted_out, workspace, workspace_bytes,
                              pp::as_stream(stream));
}

int pp_is_quantile_groups(const float* value_sorted, const double* cdf_sorted, const int32_t* counted, int32_t n_groups,
                          int32_t n_per, const double* q, int32_t n_q, double* out, void* stream) {
    return pp::is_quantile_groups(value_sorted, cdf_sorted, counted, n_groups, n_per, q, n_q, out, pp::as_stream(stream));
}

size_t pp_is_unique_workspace_bytes(int32_t n_groups, int32_t n_per) {
    if (!pp::groups_shape_ok(n_groups, n_per)) return 0;
    pp::UniqueWorkspace w;
    pp::unique_carve(n_groups, n_per, nullptr, w);
    return w.bytes;
}

int pp_is_unique_groups(const float* value_sorted, const float* lw_sorted, const int32_t* counted, int32_t n_groups, int32_t n_per,
                        const double* stats, float* value_out, int64_t* mass_out, int32_t* count_out, int32_t* runs_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_unique_groups(value_sorted, lw_sorted, counted, n_groups, n_per, stats, value_out, mass_out, count_out, runs_out,
                                workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
