// Weight gradients of the backward pass in one launch:
//   dW_ih = dG^T X,  dW_hh = dG_t^T h_{t-1},  dW1 = dz1^T h,  dW2 = dy^T a1,  the observe-embedding's dWf1 = dE^T f1, dWf0 = dF1^T cat,
//   dW1_o = dCat_o^T h_o
// (inference_network_lstm.py:186-220 backward: torch.autograd's weight gradients of nn.LSTM / nn.Linear), every product
// with K = rows of the minibatch and both operands stored row = k by the kernels before it (the second one optionally
// through a row gather: h_{t-1} by prev_row, the rows of an address group).
//
// Why not the grouped tile kernels (gemm_f32.hip): those stage K slabs through an LDS ring, three slabs ahead - a workgroup
// streams ~45 GB/s, so 1 024 rows cost ~13 us per tile however small the problem (measured: the four one-tile embedding
// problems ALONE take the launch 13 us, profiles/r03g_wgrad_composition.txt). Here both operands are k-major, which is the
// MFMA operand layout of v_mfma_f32_32x32x2_f32 as it lies in memory (lane l supplies A[k0 + l / 32][m0 + l % 32]): the
// fragments are plain coalesced dword loads into a register ring, eight row pairs ahead of the MFMAs - no LDS, no barrier
// in the K loop. A workgroup (8 waves) owns a 64 x 64 output tile over one of S row ranges; every wave multiplies the whole
// tile over its own eighth of the rows; the waves meet in LDS, the S ranges in float atomics on dW.
// Single-statement batches (behind the panel kernel): 23.2 -> 15.2 us. Ragged batches (K up to 2 600 rows, 33 problems):
// one launch instead of two, step 0.555 -> 0.519 ms; what bounds it there: DESIGN.md 8.2 (the float atomics).
//
// Two K loops share the kernel, chosen per problem by the host (WgradT1Prob::wide, wgrad_t1_build): the WIDE loop - one float4
// per lane and operand on v_mfma_f32_16x16x4_f32, tile edges in units of 16, a ring of five quad-rows, the waves meeting in
// two rounds of b128 LDS operations whose layout hands every atomic instruction 64 consecutive floats of a row - for
// operands that are 16-byte aligned with pitches that are multiples of 4 (every problem of the training steps), and the
// dword loop described above for everything else (PP_WGRAD_WIDE=0: for every problem - the A/B arm).
//
// The reduction jobs of the backward pass (aux_jobs.hpp: column sums, table-column gradients, bias gradients, the loss) ride
// behind the tiles as before (in a launch of one round: the derived jobs first, wgrad_t1()).
#include "wgrad_t1.hpp"

#include <stdlib.h>

#include <algorithm>

namespace pp {

extern long long* g_wgtrace;   // gemm_f32.hip (pp_debug_wgtrace)
extern int g_wgtrace_cap, g_wgtrace_mode;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_RING = 8;    // row pairs in the ring: nine in flight (36 loads per wave) while one multiplies. The operands
                              // were written by the previous kernel on other XCDs - every load is a ~2 us trip to the
                              // Infinity Cache - and a CU needs ~100 KB in flight to stream at its L1 fill rate

// two rows (k + lane / 32) of the tile's 64 A columns and 64 B columns: the operands of four MFMAs
struct Pair {
    float a0, a1, b0, b1;
};

// K loop of one wave: the whole 64 x 64 tile over rows [kb, ke).
template <bool GATHER>
__device__ __forceinline__ void wgrad_kloop(f32x16 (&acc)[2][2], const float* __restrict__ A, const float* __restrict__ B,
                                            const int32_t* __restrict__ bidx, const int lda, const int ldb, const int M, const int N,
                                            const int m0, const int n0, const int kb, const int ke, const int lane,
                                            const bool hm, const bool hn) {
    const int l31 = lane & 31, h = lane >> 5;
    // columns beyond M / N are clamped: their products land in accumulator rows / columns the epilogue never stores.
    // Rows beyond the range are clamped too and enter as a * 0 (a multiply, not a select: a select lets the compiler
    // predicate the LOAD, one branch per load)
    const float* pa0 = A + min(m0 + l31, M - 1);
    const float* pa1 = A + min(m0 + 32 + l31, M - 1);
    const float* pb0 = B + min(n0 + l31, N - 1);
    const float* pb1 = B + min(n0 + 32 + l31, N - 1);
    // Row gather on the second operand: an index loaded next to its row would have to be WAITED for, and loads return in
    // order - s_waitcnt on the youngest load drains the whole ring, every pair (measured: the ragged step's launch ran its
    // MFMAs a third of the time). So a lane keeps the indices of 64 rows (one coalesced load per 32 pairs, issued a block
    // ahead: by the time it is read more than 63 younger loads have been issued) and a pair takes its two with v_readlane.
    int idxA = 0, idxB = 0;
    if (GATHER) idxA = bidx[min(kb + lane, ke - 1)];
    auto load = [&](int pidx, Pair& p) {      // row pair pidx of this wave: rows kb + 2 pidx + h
        const int k = kb + 2 * pidx + h;
        const int kc = min(k, ke - 1);
        const float keep = k < ke ? 1.0f : 0.0f;
        p.a0 = pa0[(int64_t)kc * lda] * keep;
        p.a1 = pa1[(int64_t)kc * lda] * keep;
        int kb2 = kc;
        if (GATHER) {
            if ((pidx & 31) == 0) {      // first pair of a 64-row block (wave-uniform): fetch the NEXT block's indices
                const int nb = (pidx >> 5) + 1;
                const int v = bidx[min(kb + 64 * nb + lane, ke - 1)];
                idxB = (nb & 1) ? v : idxB;
                idxA = (nb & 1) ? idxA : v;
            }
            const int v = ((pidx >> 5) & 1) ? idxB : idxA;
            const int sel = 2 * (pidx & 31);
            const int r0 = __builtin_amdgcn_readlane(v, sel), r1 = __builtin_amdgcn_readlane(v, sel + 1);
            kb2 = h ? r1 : r0;
        }
        p.b0 = pb0[(int64_t)kb2 * ldb];
        p.b1 = pb1[(int64_t)kb2 * ldb];
    };
    auto mma = [&](const Pair& p) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(p.a0, p.b0, acc[0][0], 0, 0, 0);
        if (hn) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(p.a0, p.b1, acc[0][1], 0, 0, 0);
        if (hm) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(p.a1, p.b0, acc[1][0], 0, 0, 0);
        if (hm && hn) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(p.a1, p.b1, acc[1][1], 0, 0, 0);
    };
    Pair f[WG_RING];
    const int nfr = (ke - kb + 1) >> 1;      // row pairs of this wave
    // (loads are unconditional so that the compiler counts them with s_waitcnt vmcnt(N) instead of draining the queue at
    // a branch)
#pragma unroll
    for (int i = 0; i < WG_RING - 1; ++i) load(i, f[i]);
    int i0 = 0;
    for (; i0 + WG_RING <= nfr; i0 += WG_RING) {
#pragma unroll
        for (int j = 0; j < WG_RING; ++j) {
            load(i0 + j + WG_RING - 1, f[(j + WG_RING - 1) % WG_RING]);
            mma(f[j]);
        }
    }
    const int nrem = nfr - i0;      // < WG_RING: already in the ring
#pragma unroll
    for (int j = 0; j < WG_RING - 1; ++j)
        if (j < nrem) mma(f[j]);
}

// ---- the wide loop: 16-byte operand loads on v_mfma_f32_16x16x4_f32 ----------------------------------------------------
// A k-major row is also the operand layout of the 16x16x4 MFMA (lane (q = l / 16, c = l % 16) supplies k = q, column c), and
// nothing says that column c of the MFMA has to be column c of the tile: lane (q, c) loads ONE float4 of row k0 + q at the
// tile's columns 4 c .. 4 c + 3 of A and of B, and MFMA (i, j) multiplies component i of the A vector by component j of the B
// vector - the output block {rows 4 x + i} x {columns 4 y + j} of the tile. Two 1 KB loads feed 16 MFMAs over four rows (the
// dword loop: four 256 B loads per four MFMAs over two rows), and lane (q, c) ends up with the 16 x 4 block at rows
// 16 q + 4 r + i (r = accumulator register), columns 4 c + j: for a fixed (i, r) its four j-accumulators are one float4 of a
// tile row, which is what the epilogue below moves through LDS.
// Tile edges come in units of 16: a tile is MB x NB blocks of 16 (MB, NB in {1, 2, 4}: vectors of 4, 2, 1 floats at column
// MB c, rows MB (4 q + r) + i) - M = 271 is four 64-row tiles and one of 16, where the 32-wide quadrants multiplied 320.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int WG_RINGW = 5;   // quad-rows in the ring, 4 .. 6 fit under 128 VGPRs: five in flight (10 KB per wave, 80 KB per
                              // workgroup) while one multiplies
constexpr int WG_RINGW_GATHER = 4;      // (the row gather keeps two index registers and the lane selects: five spill; and 4 divides an index block)

template <int MB, int NB>
struct Quad {      // four rows (k + lane / 16) of the tile's A and B columns: the operands of MB x NB MFMAs
    float a[MB], b[NB];
};

template <int W>
__device__ __forceinline__ void load_vec(float (&d)[W], const float* __restrict__ p) {
    if constexpr (W == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    } else if constexpr (W == 2) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(p);
        d[0] = v[0]; d[1] = v[1];
    } else {
        d[0] = *p;
    }
}

// K loop of one wave: the whole tile over rows [kb, ke), conventions as in wgrad_kloop (unconditional loads, rows past the
// range enter as a * 0, the row gather's indices in blocks of 64 rows = 16 quad-rows).
template <bool GATHER, int MB, int NB>
__device__ __forceinline__ void wgrad_kloop_wide(f32x4 (&acc)[4][4], const float* __restrict__ A, const float* __restrict__ B,
                                                 const int32_t* __restrict__ bidx, const int lda, const int ldb, const int M,
                                                 const int N, const int m0, const int n0, const int kb, const int ke,
                                                 const int lane) {
    const int c = lane & 15, q = lane >> 4;
    // single columns are clamped as in the dword loop; a float2 / float4 lies inside the row pitch (the host's rule) and
    // what it reads beyond M / N lands in accumulator rows / columns the epilogue never stores
    const float* pa = A + (MB == 1 ? min(m0 + c, M - 1) : m0 + MB * c);
    const float* pb = B + (NB == 1 ? min(n0 + c, N - 1) : n0 + NB * c);
    // Row gather: the block scheme of the dword loop (a lane keeps the indices of 64 rows = 16 quad-rows, a quad-row takes its
    // four with v_readlane), but WITHOUT a branch round the index load - the compiler drains the queue where such a branch
    // joins: the ring is four deep here, so every fourth load (a fixed place of the unrolled loop) is the possible first
    // quad-row of a block; there the next block's indices are loaded again, unconditionally (64 lanes x 4 bytes per 8 KB of
    // operands), after the register of the current block took the previous copy if a block begins.
    int cur = 0, nxt = 0;
    if (GATHER) {
        cur = bidx[min(kb + lane, ke - 1)];
        nxt = bidx[min(kb + 64 + lane, ke - 1)];
        asm volatile("" : "+v"(nxt));      // (lands with cur, which the first B load waits for anyway: sunk into the loop's
                                           // preheader, behind the ring's first loads, it costs the loop a wait on them)
    }
    const int q_odd = -(q & 1), q_hi = -(q >> 1);
    auto load = [&](int pidx, Quad<MB, NB>& p, bool site) {      // quad-row pidx of this wave: rows kb + 4 pidx + q
        const int k = kb + 4 * pidx + q;
        const int kc = min(k, ke - 1);
        load_vec<MB>(p.a, pa + (int64_t)kc * lda);
        int kb2 = kc;
        if (GATHER) {
            if (site) {      // (pidx % 4 == 0, known at compile time)
                cur = (pidx & 15) == 0 ? nxt : cur;
                nxt = bidx[min(kb + 64 * ((pidx >> 4) + 1) + lane, ke - 1)];
            }
            const int v = cur;
            const int sel = 4 * (pidx & 15);
            const int r0 = __builtin_amdgcn_readlane(v, sel), r1 = __builtin_amdgcn_readlane(v, sel + 1);
            const int r2 = __builtin_amdgcn_readlane(v, sel + 2), r3 = __builtin_amdgcn_readlane(v, sel + 3);
            // (bit selects: a ?: chain over q becomes a switch with a branch per load)
            const int t0 = r0 ^ ((r0 ^ r1) & q_odd), t1 = r2 ^ ((r2 ^ r3) & q_odd);
            kb2 = t0 ^ ((t0 ^ t1) & q_hi);
        }
        load_vec<NB>(p.b, pb + (int64_t)kb2 * ldb);
    };
    // (the * 0 of the rows past the range is applied here, not at the load: behind the load it is an s_waitcnt on the
    // youngest load of the ring)
    auto mma = [&](int pidx, const Quad<MB, NB>& p) {
        const float keep = kb + 4 * pidx + q < ke ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const float a = p.a[i] * keep;
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, p.b[j], acc[i][j], 0, 0, 0);
        }
    };
    constexpr int RING = GATHER ? WG_RINGW_GATHER : WG_RINGW;
    static_assert(WG_RINGW_GATHER == 4, "the index blocks' reload sits at every fourth quad-row");
    Quad<MB, NB> f[RING];
    const int nfr = (ke - kb + 3) >> 2;      // quad-rows of this wave
#pragma unroll
    for (int i = 0; i < RING - 1; ++i) load(i, f[i], false);
    int i0 = 0;
    for (; i0 + RING <= nfr; i0 += RING) {
#pragma unroll
        for (int j = 0; j < RING; ++j) {
            load(i0 + j + RING - 1, f[(j + RING - 1) % RING], ((j + RING - 1) & 3) == 0);
            __builtin_amdgcn_sched_barrier(0);      // (left alone the scheduler gathers an iteration's loads behind its MFMAs and
            mma(i0 + j, f[j]);                      // drains the queue - s_waitcnt vmcnt(0) - once per trip round the ring)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const int nrem = nfr - i0;      // < RING: already in the ring
#pragma unroll
    for (int j = 0; j < RING - 1; ++j)
        if (j < nrem) mma(i0 + j, f[j]);
}

template <int MB, int NB>
__device__ __forceinline__ void wgrad_kloop_wide_any(f32x4 (&acc)[4][4], const float* A, const float* B, const int32_t* bidx,
                                                     const int lda, const int ldb, const int M, const int N, const int m0,
                                                     const int n0, const int kb, const int ke, const int lane) {
    if (bidx) wgrad_kloop_wide<true, MB, NB>(acc, A, B, bidx, lda, ldb, M, N, m0, n0, kb, ke, lane);
    else wgrad_kloop_wide<false, MB, NB>(acc, A, B, bidx, lda, ldb, M, N, m0, n0, kb, ke, lane);
}

// One tile of a wide problem over the rows [k0, k1) of its split: the K loop, then the eight waves' partial tiles meet in LDS
// in TWO rounds of 64 KB (round h: the accumulators i = 2 h, 2 h + 1 = 32 of the tile's rows) and three barriers (the 32 x 32
// quadrants of the dword loop: seven, on 64 + 64 dword operations per thread). An accumulator (i, j) of lane (q, c) is a
// float4 over r: four rows of ONE column, 4 c + j. It goes as it is (ds_write_b128) to slot (i & 1, q) of the wave's 8 KB, to
// the float4 of its column - so that the thread that sums a slot over the eight waves reads the float4 of column `lane`
// (ds_read_b128) and a wave's atomic instruction covers 64 consecutive floats of one row of dW. The float4s of a slot are
// swizzled inside groups of four, (c, j) -> 4 c + (j ^ (c >> 1 & 3)): a store instruction (one j) would otherwise put its
// eight-lane groups on two of the eight 16-byte bank columns, four ways; reads stay inside their aligned groups of four.
__device__ __forceinline__ void wgrad_tile_wide(const WgradT1Args& g, const WgradT1Prob& p, const int m0, const int n0, const int k0,
                                                const int k1, float* lds) {
    const float* const A = p.A;
    const float* const B = p.B;
    float* const C = p.C;
    const int32_t* const bidx = p.bidx;
    const int lda = p.lda, ldb = p.ldb, ldc = p.ldc, M = p.M, N = p.N;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per = ((k1 - k0 + 31) >> 5) * 4;      // rows per wave: whole quad-rows
    const int kb = k0 + wave * per, ke = min(k1, kb + per);
    const int mb = M - m0 > 32 ? 4 : M - m0 > 16 ? 2 : 1, nb = N - n0 > 32 ? 4 : N - n0 > 16 ? 2 : 1;      // (wave-uniform)
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (kb < ke) {
#define PP_WIDE_CASE(MB, NB) \
    case MB * 8 + NB: wgrad_kloop_wide_any<MB, NB>(acc, A, B, bidx, lda, ldb, M, N, m0, n0, kb, ke, lane); break;
        switch (mb * 8 + nb) {
            PP_WIDE_CASE(4, 4) PP_WIDE_CASE(4, 2) PP_WIDE_CASE(4, 1)
            PP_WIDE_CASE(2, 4) PP_WIDE_CASE(2, 2) PP_WIDE_CASE(2, 1)
            PP_WIDE_CASE(1, 4) PP_WIDE_CASE(1, 2) PP_WIDE_CASE(1, 1)
        }
#undef PP_WIDE_CASE
    }
    if (g.trace && threadIdx.x == 0) g.trace[8 * blockIdx.x + 4] = wall_clock64();
    // the thread's slot of a round: rows mb (4 sq + r) + 2 h + si, r = 0 .. 3, of column (nb = 4: lane) nb (lane >> 2) + (lane & 3)
    const int si = wave >> 2, sq = wave & 3;
    const int oc = lane >> 2, oj = lane & 3;
    f32x4 out[2];
    auto add_out = [&](int h, const f32x4& v) {
        const int i = 2 * h + si, gn = n0 + nb * oc + oj;
        if (i >= mb || oj >= nb || gn >= N) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = m0 + mb * (4 * sq + r) + i;
            if (gm < M) atomicAdd(C + (int64_t)gm * ldc + gn, v[r]);
        }
    };
    const int wr = wave * 2048 + q * 256 + 16 * c, swz = (c >> 1) & 3;      // + si 1024 + 4 (j ^ swz)
    const int rd = wave * 256 + 4 * ((lane & ~3) | (oj ^ ((lane >> 3) & 3)));      // + source wave 2048
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (2 * h >= mb) break;      // (block-uniform: a tile of 16 or 32 rows has no accumulators i >= 2)
        if (h) __syncthreads();
#pragma unroll
        for (int il = 0; il < 2; ++il)
            if (2 * h + il < mb) {      // (the slots of rows the tile does not have are neither written nor read)
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(lds + wr + il * 1024 + 4 * (j ^ swz)) = acc[2 * h + il][j];
            }
        __syncthreads();
        f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (2 * h + si < mb) {
#pragma unroll
            for (int w = 0; w < 8; ++w) v += *reinterpret_cast<const f32x4*>(lds + w * 2048 + rd);
        }
        out[h] = v;
        if (!g.aux_first) add_out(h, v);      // one round of workgroups: the atomics of a round overlap the next round's LDS traffic
    }
    if (g.aux_first) {      // (several rounds of workgroups: the atomics after the last LDS round, as in the dword path)
        add_out(0, out[0]);
        if (mb > 2) add_out(1, out[1]);
    }
}

__global__ __launch_bounds__(512, 4) void wgrad_t1_kernel(const WgradT1Args g, const AuxJobs aux) {
    __shared__ __attribute__((aligned(16))) float lds[16384];      // wide tiles: [8 waves][8 slots][64 lanes] float4; dword tiles: [8 waves][16][64] partial quadrants (the first half); the reduction jobs use 2 048 floats
    const long long t_start = g.trace ? wall_clock64() : 0;
    // The reduction jobs ride in front of the tiles when the tiles need more than one round of the chip's workgroup slots
    // (ragged batches: they would otherwise start when the last tile has been dispatched and BE the tail of the launch,
    // ~15 us, tools/wg_trace_wgrad.py), else behind them (one round: the tiles are the long workgroups and start at once).
    const int aux_lo = g.aux_first ? 0 : g.n_blocks;
    const int bx = (int)blockIdx.x - (g.aux_first ? aux.n_blocks : 0);
    if ((int)blockIdx.x >= aux_lo && (int)blockIdx.x < aux_lo + aux.n_blocks) {
        // (behind the tiles the list is rotated: the jobs derived from the group sums first, the column sums last - wgrad_t1())
        int jb = (int)blockIdx.x - aux_lo + g.aux_rot;
        if (jb >= aux.n_blocks) jb -= aux.n_blocks;
        aux_job_run(aux, jb, lds);
        if (g.trace && threadIdx.x == 0) {
            long long* tr = g.trace + 8 * blockIdx.x;
            tr[0] = t_start; tr[1] = wall_clock64(); tr[2] = 100; tr[3] = 0;
        }
        return;
    }
    int pi = 0;
#pragma unroll
    for (int q = 1; q < WGRAD_T1_MAX; ++q)
        if (q < g.n_prob && bx >= g.p[q].first) pi = q;
    // (scalar loads with a run-time index: one trip to the kernel arguments)
    const float* const A = g.p[pi].A;
    const float* const B = g.p[pi].B;
    float* const C = g.p[pi].C;
    const int32_t* const bidx = g.p[pi].bidx;
    const int lda = g.p[pi].lda, ldb = g.p[pi].ldb, ldc = g.p[pi].ldc, M = g.p[pi].M, N = g.p[pi].N, nt = g.p[pi].nt;
    const int K = g.p[pi].K, ks = g.p[pi].ks;
    const int local = bx - g.p[pi].first;
    const int mtg = g.p[pi].mtg;
    int s, tm, tn;
    if (mtg > 0) {
        // XCD-aware order (workgroups go to the 8 XCDs round-robin by block index, each XCD has its own L2): block r (mod 8)
        // of the problem owns the row tiles tm = r (mod 8) - all their column tiles and row splits. An XCD then fetches ITS
        // M / 8 columns of A once and all of B; with the column tile fastest (below) every XCD owned one column tile of B and
        // streamed ALL of A - the larger operand (dG: 4H columns) - from the Infinity Cache: 8 x |A| + |B| instead of
        // |A| + 8 x |B| per launch. Row tiles past the end of a ragged last group are empty workgroups.
        const int r = local & 7, u = local >> 3;
        const int tmg = u % mtg, v = u / mtg;
        tn = v % nt;
        s = v / nt;
        tm = tmg * 8 + r;
        if (tm * 64 >= M) return;
    } else {
        const int tiles = ((M + 63) >> 6) * nt;
        s = local / tiles;
        const int t = local - s * tiles;
        tm = t / nt;
        tn = t - tm * nt;
    }
    if (g.p[pi].wide) {      // (per problem, from the host: alignment and pitches; PP_WGRAD_WIDE=0: none)
        wgrad_tile_wide(g, g.p[pi], tm * 64, tn * 64, s * ks, min(K, s * ks + ks), lds);
        if (g.trace && threadIdx.x == 0) {
            long long* tr = g.trace + 8 * blockIdx.x;
            tr[0] = t_start; tr[1] = wall_clock64(); tr[2] = pi; tr[3] = s;
        }
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = tm * 64, n0 = tn * 64;
    // Every wave multiplies the WHOLE 64 x 64 tile over its own eighth of the split's rows: each row of the operands enters
    // the CU once (quadrant-per-wave layouts fetch every line twice, and the L1 fill rate is what bounds the stream), and
    // the four accumulators are independent MFMA chains.
    const int k0 = s * ks, k1 = min(K, k0 + ks);
    const int per = ((k1 - k0 + 15) >> 4) * 2;
    const int kb = k0 + wave * per, ke = min(k1, kb + per);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const bool hm = m0 + 32 < M, hn = n0 + 32 < N;      // second half of the tile's rows / columns exists (wave-uniform)
    if (kb < ke) {
        if (bidx) wgrad_kloop<true>(acc, A, B, bidx, lda, ldb, M, N, m0, n0, kb, ke, lane, hm, hn);
        else wgrad_kloop<false>(acc, A, B, bidx, lda, ldb, M, N, m0, n0, kb, ke, lane, hm, hn);
    }
    if (g.trace && threadIdx.x == 0) g.trace[8 * blockIdx.x + 4] = wall_clock64();
    // the eight waves' partial tiles meet in LDS, one 32 x 32 quadrant at a time; the S row ranges meet in float atomics
    // D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    // (launches with several rounds of workgroups issue the atomics after the LAST LDS round: a barrier waits for the
    // workgroup's outstanding memory operations and the memory side is saturated with atomics there, tools/wg_trace_wgrad.py)
    float out[2][2][2];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            out[qi][qj][0] = out[qi][qj][1] = 0.0f;
            if ((qi && !hm) || (qj && !hn)) continue;      // (block-uniform)
            if (qi + qj > 0) __syncthreads();
            float* mine = lds + wave * 1024 + lane;
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[r * 64] = acc[qi][qj][r];
            __syncthreads();
            // 512 threads: element (r, lane) with r = 2 (tid >> 6) + {0, 1}
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int r = 2 * wave + e;
                float v = 0.0f;
#pragma unroll
                for (int w = 0; w < 8; ++w) v += lds[w * 1024 + r * 64 + lane];
                out[qi][qj][e] = v;
                if (!g.aux_first) {      // one round of workgroups: the atomics of a round overlap the next round's LDS traffic
                    const int gm = m0 + 32 * qi + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int gn = n0 + 32 * qj + l31;
                    if (gm < M && gn < N) atomicAdd(C + (int64_t)gm * ldc + gn, v);
                }
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
        for (int qj = 0; qj < 2; ++qj) {
            if (!g.aux_first || (qi && !hm) || (qj && !hn)) continue;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int r = 2 * wave + e;
                const int gm = m0 + 32 * qi + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int gn = n0 + 32 * qj + l31;
                if (gm < M && gn < N) atomicAdd(C + (int64_t)gm * ldc + gn, out[qi][qj][e]);
            }
        }
    if (g.trace && threadIdx.x == 0) {
        long long* tr = g.trace + 8 * blockIdx.x;
        tr[0] = t_start; tr[1] = wall_clock64(); tr[2] = pi; tr[3] = s;
    }
}

}  // namespace

bool wgrad_t1_build(const pp_gemm_args* q, const GemmHole* holes, int n, WgradT1Args& out) {
    static const int env = getenv("PP_WGRAD_T1") ? atoi(getenv("PP_WGRAD_T1")) : 1;
    static const int env_s = 0;
    static const int env_xmap = getenv("PP_WGRAD_XMAP") ? atoi(getenv("PP_WGRAD_XMAP")) : 1;      // A/B: 0 = column tiles fastest
    static const bool env_wgs_set = false;
    static const int env_wgs = 240;
    if (!env || deterministic_mode() || n <= 0) return false;
    // PP_WGRAD_WIDE=0: every problem takes the dword loop and its epilogue (read per call, for the A/B and the parity tests)
    const char* const env_wide = getenv("PP_WGRAD_WIDE");
    const bool wide_on = !(env_wide && atoi(env_wide) == 0);
    out = WgradT1Args{};
    int np = 0;
    // The 16-byte loop (wgrad_kloop_wide) takes a problem whose operand pointers are 16-byte aligned after the cut, whose
    // pitches are multiples of 4 floats, and whose last tile's float2 / float4 (16 vectors from the tile's first column; a
    // 16-wide edge loads single clamped floats) end inside the row pitch: M = 271 with lda = 272 does (256 + 16 x 1), an odd
    // pitch or a cut at an odd column does not.
    auto vec_ok = [](const float* ptr, int64_t ld, int lo, int ext) {
        if (((uintptr_t)ptr & 15) || (ld & 3)) return false;
        const int t0 = (ext - 1) / 64 * 64, rem = ext - t0;
        const int w = rem > 32 ? 4 : rem > 16 ? 2 : 1;
        return w == 1 || (int64_t)lo + t0 + 16 * w <= ld;
    };
    // a cut [m_lo, m_hi) x [n_lo, n_hi) of problem a whose first k_lo rows contribute nothing
    auto add = [&](const pp_gemm_args& a, int m_lo, int m_hi, int n_lo, int n_hi, int k_lo) -> bool {
        if (m_hi <= m_lo || n_hi <= n_lo || k_lo >= a.K) return true;
        if (np >= WGRAD_T1_MAX) return false;
        WgradT1Prob& p = out.p[np++];
        p.A = a.A + (int64_t)k_lo * a.lda + m_lo;
        p.bidx = a.b_idx ? a.b_idx + k_lo : nullptr;
        p.B = a.B + (a.b_idx ? 0 : (int64_t)k_lo * a.ldb) + n_lo;
        p.C = a.C + (int64_t)m_lo * a.ldc + n_lo;
        p.lda = (int)a.lda; p.ldb = (int)a.ldb; p.ldc = (int)a.ldc;
        p.M = m_hi - m_lo; p.N = n_hi - n_lo; p.nt = cdiv(p.N, 64);
        p.K = a.K - k_lo;
        p.wide = (wide_on && vec_ok(p.A, a.lda, m_lo, p.M) && vec_ok(p.B, a.ldb, n_lo, p.N)) ? 1 : 0;
        return true;
    };
    for (int i = 0; i < n; ++i) {
        const pp_gemm_args& a = q[i];
        if (!a.a_kmajor || !a.b_kmajor || a.a_idx || a.c_idx || a.bias || a.bias2 || a.mask || a.relu || a.colsum ||
            !a.accumulate || a.K <= 0 || a.M <= 0 || a.N <= 0 || a.lda >= (1 << 30) || a.ldb >= (1 << 30) || a.ldc >= (1 << 30))
            return false;
        // Zero blocks (GemmHole: the product is zero for m, n, k inside the block): only blocks that start at k = 0 are used
        // (a trace's first time step has no previous variable and a zero cell state). The tensor is cut along the blocks'
        // edges; a cell starts at the largest k1 of the blocks that cover it.
        int mc[6] = {0, (int)a.M, 0, 0, 0, 0}, nc[6] = {0, (int)a.N, 0, 0, 0, 0};
        int nm = 2, nn = 2;
        GemmBlock z[2];
        int nz = 0;
        if (holes) {
            for (int b = 0; b < 2; ++b) {
                GemmBlock h = holes[i].b[b];
                h.m0 = std::max(h.m0, 0); h.n0 = std::max(h.n0, 0);
                h.m1 = std::min(h.m1, (int)a.M); h.n1 = std::min(h.n1, (int)a.N); h.k1 = std::min(h.k1, (int)a.K);
                if (h.m1 <= h.m0 || h.n1 <= h.n0 || h.k1 <= h.k0 || h.k0 > 0) continue;      // (k0 > 0: not used, still correct)
                z[nz++] = h;
                mc[nm++] = h.m0; mc[nm++] = h.m1;
                nc[nn++] = h.n0; nc[nn++] = h.n1;
            }
        }
        std::sort(mc, mc + nm);
        std::sort(nc, nc + nn);
        nm = (int)(std::unique(mc, mc + nm) - mc);
        nn = (int)(std::unique(nc, nc + nn) - nc);
        for (int jn = 0; jn + 1 < nn; ++jn) {
            int run_lo = -1, run_hi = -1, run_k = 0;      // consecutive row intervals with the same first row merge
            for (int jm = 0; jm + 1 < nm; ++jm) {
                int k_lo = 0;
                for (int b = 0; b < nz; ++b)
                    if (z[b].m0 <= mc[jm] && z[b].m1 >= mc[jm + 1] && z[b].n0 <= nc[jn] && z[b].n1 >= nc[jn + 1])
                        k_lo = std::max(k_lo, z[b].k1);
                if (run_lo >= 0 && k_lo == run_k) {
                    run_hi = mc[jm + 1];
                } else {
                    if (run_lo >= 0 && !add(a, run_lo, run_hi, nc[jn], nc[jn + 1], run_k)) return false;
                    run_lo = mc[jm]; run_hi = mc[jm + 1]; run_k = k_lo;
                }
            }
            if (run_lo >= 0 && !add(a, run_lo, run_hi, nc[jn], nc[jn + 1], run_k)) return false;
        }
    }
    if (np == 0) return false;
    // row splits: ~240 workgroups in the launch when the work is small (one per CU: fewer, longer row ranges mean fewer
    // atomics), one workgroup per tile when there are more tiles than that; at least 64 rows per split
    int64_t tile_rows = 0;
    for (int i = 0; i < np; ++i) tile_rows += (int64_t)cdiv(out.p[i].M, 64) * out.p[i].nt * out.p[i].K;
    // (large launches - ragged batches: 10^6 tile rows - want ~600 rows per workgroup: balance over 2 x 256 slots matters more
    // than the atomics of the extra splits)
    const int64_t blocks = env_wgs_set ? env_wgs : std::min<int64_t>(1536, std::max<int64_t>(env_wgs, tile_rows / 600));
    const int target_rows = (int)std::max<int64_t>(64, cdiv(tile_rows, std::max<int64_t>(blocks, 1)));
    out.n_prob = np;
    // the longest row ranges first: their workgroups start first and the short ones fill the tail
    std::stable_sort(out.p, out.p + np, [](const WgradT1Prob& x, const WgradT1Prob& y) { return x.K > y.K; });
    int first = 0;
    for (int i = 0; i < np; ++i) {
        WgradT1Prob& p = out.p[i];
        int S = env_s > 0 ? env_s : (p.K + target_rows / 2) / target_rows;
        S = std::max(1, std::min(S, std::min(16, std::max(1, p.K / 64))));
        p.S = S;
        p.ks = ((cdiv(p.K, S) + 3) / 4) * 4;
        p.first = first;
        const int mt = cdiv(p.M, 64);
        p.mtg = (env_xmap && mt >= 8) ? cdiv(mt, 8) : 0;
        first += (p.mtg ? p.mtg * 8 : mt) * p.nt * S;
    }
    out.n_blocks = first;
    return true;
}

int wgrad_t1(const WgradT1Args& a, const AuxJobs* aux, hipStream_t st) {
    static const AuxJobs none{};
    const AuxJobs& j = aux ? *aux : none;
    const int blocks = a.n_blocks + (aux ? j.n_blocks : 0);
    WgradT1Args t = a;
    t.aux_first = (aux && a.n_blocks > 512) ? 1 : 0;      // 2 workgroups x 256 CUs = one round
    // A launch of one round, jobs included: in the per-workgroup timeline of the benchmark's step
    // (tools/wg_trace_wgrad_single.py) workgroup id >= 256 shares its CU with workgroup id - 256, and a table-gradient job next to a full tile costs both ~3 us - with
    // the list in its own order those pairs are the last workgroups of the launch. Rotated, the outer / table / bias jobs come
    // first and land on the CUs that get no second workgroup or next to the short tiles the launch starts with; the column
    // sums follow. A placement heuristic, not a guarantee: the pairing is the dispatcher's and was observed, and the gain was
    // measured on the benchmark's shapes (H = 512 and 1024, B = 1024; 219 tiles + 281 jobs at H = 512) only - other one-round launches
    // (small batches, PP_PANEL=0) run the same jobs in another order, checked for results, not for time.
    // PP_WGRAD_JOBROT=0: the list's own order (read per call, for the A/B and the parity test).
    const char* const env_rot = getenv("PP_WGRAD_JOBROT");
    if (aux && blocks <= 512 && !(env_rot && atoi(env_rot) == 0)) t.aux_rot = j.cs_first[j.n_colsum];
    if (g_wgtrace && g_wgtrace_mode == 1 && blocks <= g_wgtrace_cap) t.trace = g_wgtrace;
    hipLaunchKernelGGL(wgrad_t1_kernel, dim3(blocks), dim3(512), 0, st, t, j);
    PP_LAUNCH_CHECK("wgrad_t1");
    return 0;
}

}  // namespace pp

// Host-side plan of the weight-gradient launch for `count` queued products (no device work): which cuts of the tensors become
// problems, their row ranges and splits. For tests of the host logic (tests/test_host.py). zero_blocks: [count][2][6] =
// {m0, m1, n0, n1, k0, k1} per product or NULL; out: [cap][10] = {M, N, K, S, ks, gather, first, C offset, A offset, B offset}
// (offsets in floats from the product's own pointers). Returns the number of problems, 0 if the tile kernels take the flush.
extern "C" int pp_debug_wgrad_plan(const pp_gemm_args* q, const int32_t* zero_blocks, int32_t count, int64_t* out, int32_t cap,
                                   int32_t* n_blocks) {
    std::vector<pp::GemmHole> holes((size_t)std::max(count, 0));
    for (int i = 0; i < count && zero_blocks; ++i)
        for (int b = 0; b < 2; ++b) {
            const int32_t* z = zero_blocks + ((int64_t)i * 2 + b) * 6;
            holes[i].b[b] = pp::GemmBlock{z[0], z[1], z[2], z[3], z[4], z[5]};
        }
    pp::WgradT1Args a;
    if (!pp::wgrad_t1_build(q, zero_blocks ? holes.data() : nullptr, count, a)) return 0;
    if (n_blocks) *n_blocks = a.n_blocks;
    for (int i = 0; i < a.n_prob && i < cap; ++i) {
        const pp::WgradT1Prob& p = a.p[i];
        // which product does the problem belong to: the one whose C range contains its C
        int src = -1;
        for (int k = 0; k < count; ++k)
            if (p.C >= q[k].C && p.C < q[k].C + (int64_t)q[k].M * q[k].ldc) src = k;
        int64_t* o = out + (int64_t)i * 10;
        o[0] = p.M; o[1] = p.N; o[2] = p.K; o[3] = p.S; o[4] = p.ks; o[5] = p.bidx ? 1 : 0; o[6] = p.first;
        o[7] = src >= 0 ? p.C - q[src].C : -1;
        o[8] = src >= 0 ? p.A - q[src].A : -1;
        o[9] = src >= 0 ? (p.bidx ? p.bidx - q[src].b_idx : (p.B - q[src].B)) : -1;
    }
    return a.n_prob;
}

// Builds the same plan, reports per problem (in the plan's order) whether it takes the 16-byte loop (wide_out[i] = 1) or the
// dword loop, and with launch != 0 runs the launch on `stream` without reduction jobs: the kernel alone, for tests and
// timelines. Returns the number of problems; 0: refused (the tile kernels take these products), nothing is launched.
extern "C" int pp_debug_wgrad_run(const pp_gemm_args* q, const int32_t* zero_blocks, int32_t count, int32_t launch, void* stream,
                                  int32_t* wide_out, int32_t cap) {
    std::vector<pp::GemmHole> holes((size_t)std::max(count, 0));
    for (int i = 0; i < count && zero_blocks; ++i)
        for (int b = 0; b < 2; ++b) {
            const int32_t* z = zero_blocks + ((int64_t)i * 2 + b) * 6;
            holes[i].b[b] = pp::GemmBlock{z[0], z[1], z[2], z[3], z[4], z[5]};
        }
    pp::WgradT1Args a;
    if (!pp::wgrad_t1_build(q, zero_blocks ? holes.data() : nullptr, count, a)) return 0;
    for (int i = 0; i < a.n_prob && i < cap && wide_out; ++i) wide_out[i] = a.p[i].wide;
    if (launch && pp::wgrad_t1(a, nullptr, (hipStream_t)stream) != 0) return 0;
    return a.n_prob;
}
