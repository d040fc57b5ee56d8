// Batched posteriors: M observations ("groups") of n_per particles each in one lock-step importance-sampling call.
//
// The reference serves one observation per posterior call (pyprob/model.py:106-117: _infer_init embeds THE observation,
// pyprob/nn/inference_network.py:141-148; every trace's first _infer_step runs on that one embedding,
// pyprob/nn/inference_network_lstm.py:82-134), so posteriors for M observations are M calls. Here
//   pp_is_batch_first   evaluates embedding + first LSTM step + proposal layer for M observation rows at once (the launches of
//                       the training step's forward at T = 1: [the convolution stack of a CNN2D5C observable at B = M,] embedding
//                       GEMMs, input gather, gate GEMM, cell, head GEMMs), and
//   pp_is_fused_groups  is pp_is_fused's pass with the proposal of particle i read from row i / n_per of the head outputs and
//                       per-group operands, followed by the importance statistics of every group.
//   pp_is_batch_bias    writes, for a LATER statement (prev_addr_id >= 0), the bias row of every group: what is_prep_kernel computes
//                       for the one observation of a single call, on the M embedding rows pp_is_batch_first left in the workspace, and
//   pp_is_statement_groups  runs that statement for all M n_per particles as ONE launch of the GROUPED fused statement kernel
//                       (is_step_fused.hip, is_step_small.hip): particle i starts from bias row i / n_per.
// Draw and log-density arithmetic is is_draw.hpp's (mixture_particle, term_log_prob) and head_math.hpp's: nothing is restated.
#include "cnn2d.hpp"
#include "common.hpp"
#include "gather.hpp"
#include "is_draw.hpp"
#include "is_step_fused.hpp"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace pp {

int lstm_cell_fwd(float* G, const float* c_prev, float* c, float* h, int n, int H, hipStream_t st, int c_prev_shared = 0);

namespace {

inline int64_t r4(int64_t x) { return (x + 3) & ~int64_t(3); }

constexpr int GROUP_MAX_TERMS = 8;
constexpr int GROUP_BLOCKS = 2048;        // workgroups of the draw pass at most (8 per CU)
// statistics: a group is reduced by B(n_per) workgroups over contiguous slices - a function of n_per alone, so that group g of an
// M-group call and a one-group call on the same particles add in the same order
constexpr int STAT_SLICE = 65536;         // particles per workgroup up to STAT_MAX_SLICES slices
constexpr int STAT_MAX_SLICES = 256;
constexpr int STAT_MIN_SLOTS = 256;       // partial records in the workspace: max(M, STAT_MIN_SLOTS)

inline size_t stats_workspace_bytes(int M) { return (size_t)std::max(std::max(M, 1), STAT_MIN_SLOTS) * 6 * sizeof(double); }
inline int stat_slices(int n_per) { return std::min(STAT_MAX_SLICES, cdiv(n_per, STAT_SLICE)); }

struct GroupTerm {
    int kind, c0, c1, cx, flags, C;      // c*: operand stride code 0 shared / 1 per particle / 2 per group; C: categories (kind 5)
    const float *p0, *p1, *x;
    float scale;
};
struct GroupTerms {
    GroupTerm t[GROUP_MAX_TERMS];
    int count;
};

__device__ __forceinline__ int64_t operand_at(int code, int64_t i, int64_t g) { return code == 1 ? i : (code == 2 ? g : 0); }

// One pass over the M n_per particles: particle i belongs to group g = i / n_per, draws from the proposal of row g of y (Philox
// counter offset + i, stream 0x1C: mixture_particle, what pp_is_step's per-particle kernel runs), lw (+)= - log q + the terms.
// KIND -1: no draw, the values are read. 8 bytes per particle reach memory; a workgroup may straddle groups.
template <int KIND>
__global__ __launch_bounds__(256) void is_fused_groups_kernel(const float* __restrict__ y, int64_t ldy, const float* __restrict__ prior,
                                                              int64_t total, int n_per, int K, const GroupTerms terms,
                                                              float* __restrict__ value, float* __restrict__ lw, int overwrite,
                                                              uint64_t seed, uint64_t offset, int prior_per_particle) {
    float pa = 0.0f, pb = 1.0f;
    if constexpr (KIND >= 0) {
        pa = prior[0];
        pb = prior[1];
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t g = i / n_per;
        float acc = overwrite ? 0.0f : lw[i];
        float v;
        if constexpr (KIND < 0) {
            v = value[i];
        } else {
            float lq;
            if (prior_per_particle) {      // a later statement whose prior depends on an earlier draw: [M n_per, 2]
                pa = prior[2 * i];
                pb = prior[2 * i + 1];
            }
            mixture_particle<KIND>(y + g * ldy, pa, pb, K, false, 0.0f, seed, offset + (uint64_t)i, v, lq);
            acc -= lq;                 // - log q(v)   (state.py:212, 217)
            value[i] = v;
        }
        for (int t = 0; t < terms.count; ++t) {
            const GroupTerm& T = terms.t[t];
            const float x = (T.flags & 4) ? v : T.x[operand_at(T.cx, i, g)];
            float lp;
            if (T.kind == 2) {
                lp = x;
            } else if (T.kind == 0 || T.kind == 1) {      // two parameters, either may BE the particle's value
                const float a = (T.flags & 1) ? v : T.p0[operand_at(T.c0, i, g)];
                const float b = (T.flags & 2) ? v : T.p1[operand_at(T.c1, i, g)];
                lp = T.kind == 0 ? normal_lp(a, b, x) : uniform_lp(a, b, x);
            } else {                                      // Poisson, Bernoulli: one value; Categorical: one row of C weights
                lp = term_log_prob(T.kind, T.p0 + operand_at(T.c0, i, g) * (T.kind == 5 ? T.C : 1), 0, T.p1, T.C, x, 0);
            }
            acc += T.scale * lp;
        }
        lw[i] = acc;
    }
}

// The six numbers of pp_is_stats for one slice of one group: workgroup (slice b, group g0 + blockIdx.y) sweeps its particles
// twice - the maximum of the finite log-weights, then the float64 sums of w = exp(lw - max) (fp64 exp) - with every thread
// walking its particles in index order and the threads combined by a butterfly and a fixed four-wave sum: the same bits on
// every run. One slice per group: the record is the group's result (dst = out); otherwise a partial for group_combine_kernel.
__global__ __launch_bounds__(256) void group_stats_kernel(const float* __restrict__ lw, const float* __restrict__ x, int n_per,
                                                          int slice, int g0, double* __restrict__ dst) {
    __shared__ float shmax[4];
    __shared__ double sh[4][5];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = (int64_t)g0 + blockIdx.y;
    const int lo = (int)blockIdx.x * slice, hi = (int)min((int64_t)n_per, (int64_t)lo + slice);
    const float* l = lw + g * n_per;
    const float* xv = x + g * n_per;
    float m = -INFINITY;
    for (int j = lo + tid; j < hi; j += 256) {
        const float a = l[j];
        if (isfinite(a)) m = fmaxf(m, a);        // Model._traces drops non-finite weights (model.py:65-68)
    }
    m = wave_max(m);
    if (lane == 0) shmax[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(shmax[0], shmax[1]), fmaxf(shmax[2], shmax[3]));
    double S[5] = {0, 0, 0, 0, 0};
    if (m > -INFINITY) {
        const double M = (double)m;
        for (int j = lo + tid; j < hi; j += 256) {
            const float a = l[j];
            if (!isfinite(a)) continue;
            // fp64 exponent: Empirical / util.effective_sample_size normalise in float64 (empirical.py:300, util.py:398-399)
            const double e = exp((double)a - M), xd = (double)xv[j];
            S[0] += e; S[1] += e * e; S[2] += e * xd; S[3] += e * xd * xd; S[4] += 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double r = wave_sum(S[q]);
        if (lane == 0) sh[wave][q] = r;
    }
    __syncthreads();
    double* rec = dst + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 6;
    if (tid < 5) rec[1 + tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
    if (tid == 0) rec[0] = (double)m;
}

// One thread per group adds its B partial records in slice order, rescaled to the group's maximum.
__global__ __launch_bounds__(256) void group_combine_kernel(const double* __restrict__ partial, int B, int groups,
                                                            double* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const double* p = partial + (int64_t)g * B * 6;
    double gm = -INFINITY;
    for (int b = 0; b < B; ++b) gm = fmax(gm, p[b * 6]);
    double S[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
        const double mb = p[b * 6];
        if (!(mb > -INFINITY)) continue;
        const double r = exp(mb - gm);
        S[0] += p[b * 6 + 1] * r;
        S[1] += p[b * 6 + 2] * r * r;
        S[2] += p[b * 6 + 3] * r;
        S[3] += p[b * 6 + 4] * r;
        S[4] += p[b * 6 + 5];
    }
    double* o = out + (int64_t)g * 6;
    o[0] = gm;
    for (int q = 0; q < 5; ++q) o[1 + q] = S[q];
}

struct BatchWorkspace {
    double* partial;          // FIRST: pp_is_fused_groups needs nothing else
    float *oh0, *oh1, *cat, *f1, *E, *X, *G, *A1, *h, *c;
    int64_t e4, i4, hid4, out4, ohid4;
    float* cnn_feat[PP_MAX_OBS];      // a CNN2D5C observable's [M, round4(F)] features and the scratch of its convolution stack at B = M
    void* cnn_ws[PP_MAX_OBS];
    size_t cnn_ws_bytes[PP_MAX_OBS];
    IsFusedBuffers fz;        // LAST: the fragment images of pp_is_statement_groups (empty: no fused statement kernel for this network)
    size_t bytes;
};

void batch_carve(const pp_net* net, int M, void* p, BatchWorkspace& w) {
    char* base = static_cast<char*>(p);
    size_t off = 0;
    auto take = [&](int64_t bytes) {
        off = (off + 255) & ~size_t(255);
        char* q = base ? base + off : nullptr;
        off += (size_t)std::max<int64_t>(bytes, 4);
        return q;
    };
    auto takef = [&](int64_t count) { return reinterpret_cast<float*>(take(count * 4)); };
    M = std::max(M, 1);
    w.partial = reinterpret_cast<double*>(take((int64_t)stats_workspace_bytes(M)));      // at offset 0
    const int H = std::max(1, (int)net->lstm_dim);
    w.e4 = r4(net->e_obs);
    w.i4 = r4(net->lstm_in);
    int64_t hid = 1, out = 1;
    for (int a = 0; a < net->n_addr; ++a) {
        hid = std::max<int64_t>(hid, net->addrs[a].hid);
        out = std::max<int64_t>(out, net->addrs[a].n_out);
    }
    w.hid4 = r4(hid);
    w.out4 = r4(out);
    w.ohid4 = 4;
    for (int o = 0; o < net->n_obs; ++o) w.ohid4 = std::max<int64_t>(w.ohid4, r4(net->obs_hid[o]));
    w.oh0 = takef(M * w.ohid4);
    w.oh1 = takef(M * w.ohid4);
    w.cat = takef(M * w.e4);
    w.f1 = takef(M * w.e4);
    w.E = takef(M * w.e4);
    w.X = takef(M * w.i4);
    w.G = takef((int64_t)M * 4 * H);
    w.A1 = takef(M * w.hid4);
    w.h = takef((int64_t)M * H);
    w.c = takef((int64_t)M * H);
    // (after every block a network without an image observable has: such a network keeps its size and offsets byte for byte)
    for (int o = 0; o < PP_MAX_OBS; ++o) {
        w.cnn_feat[o] = nullptr; w.cnn_ws[o] = nullptr; w.cnn_ws_bytes[o] = 0;
        if (o < net->n_obs && net->obs_kind[o] == PP_OBS_CNN2D5C) {
            w.cnn_feat[o] = takef(M * r4(net->obs_feat[o]));
            w.cnn_ws_bytes[o] = cnn_workspace_bytes(net, o, M);
            w.cnn_ws[o] = take((int64_t)w.cnn_ws_bytes[o]);
        }
    }
    is_fused_carve_sizes(net, w.fz);
    w.fz.whh = takef(w.fz.n_whh);
    w.fz.w1 = takef(w.fz.n_w1);
    w.fz.w2 = takef(w.fz.n_w2);
    w.bytes = off + 256;
}

int lin(const float* x, int64_t ldx, const float* W, const float* b, const float* b2, float* y, int64_t ldy, int n, int in, int out,
        bool relu, hipStream_t st) {
    pp_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = x; g.lda = ldx;
    g.B = W; g.ldb = in;
    g.C = y; g.ldc = ldy;
    g.M = n; g.N = out; g.K = in;
    g.bias = b; g.bias2 = b2; g.relu = relu;
    return gemm_f32(&g, st);
}

bool batch_net_ok(const pp_net* net) {
    if (!net || net->n_obs < 1 || net->n_obs > PP_MAX_OBS) return false;
    for (int o = 0; o < net->n_obs; ++o) {
        CnnGeom g;
        if (net->obs_kind[o] != PP_OBS_FEEDFORWARD && !(net->obs_kind[o] == PP_OBS_CNN2D5C && cnn_geom(net, o, g))) return false;
    }
    return net->lstm_dim == 0 || std::max(1, (int)net->lstm_depth) == 1;
}

}  // namespace

int is_batch_first(const pp_net* net, const float* P, const float* obs, int addr_id, int M, float* y_out, int64_t ldy, float* h_out,
                   float* c_out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(net && P && obs && y_out && ws, "pp_is_batch_first: null pointer");
    PP_CHECK_ARG(batch_net_ok(net), "pp_is_batch_first: FEEDFORWARD or CNN2D5C observe embeddings and a FeedForward network or an LSTM of depth 1");
    PP_CHECK_ARG(addr_id >= 0 && addr_id < net->n_addr, "pp_is_batch_first: address id out of range");
    PP_CHECK_ARG(M >= 0, "pp_is_batch_first: negative group count");
    const pp_addr& ad = net->addrs[addr_id];
    PP_CHECK_ARG(ldy >= ad.n_out && (ldy % 4) == 0, "pp_is_batch_first: ldy must be a multiple of 4 and at least the head's %d outputs", ad.n_out);
    if (M == 0) return 0;
    BatchWorkspace w;
    batch_carve(net, M, ws, w);
    if (w.bytes > ws_bytes) {
        set_error("pp_is_batch_first: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return PP_ENOSPACE;
    }
    // _infer_init for M rows: EmbeddingFeedForward per observable (the hidden rows ping-pong between two buffers), concatenation,
    // the two final layers (inference_network.py:132-148). A CNN2D5C observable: its M images (columns [ci, ci + C H W) of the rows)
    // through the convolution stack at B = M, _lin1 / _lin2 read the [M, round4(F)] features - pp_is_init's route for one image
    // (an image's features do not depend on the batch it sits in, cnn2d.hip).
    int ci = 0, co = 0, width = 0;
    for (int o = 0; o < net->n_obs; ++o) width += net->obs_in[o];
    for (int o = 0; o < net->n_obs; ++o) {
        const int depth = net->obs_depth[o] ? net->obs_depth[o] : 2;
        const float* x = obs + ci;
        int64_t ldx = width;
        int in = net->obs_in[o];
        if (net->obs_kind[o] == PP_OBS_CNN2D5C) {
            const int64_t f4 = r4(net->obs_feat[o]);
            PP_TRY(cnn_forward(net, o, P, x, ldx, M, w.cnn_feat[o], f4, w.cnn_ws[o], w.cnn_ws_bytes[o], false, st));
            x = w.cnn_feat[o]; ldx = f4; in = net->obs_feat[o];
        }
        for (int l = 0; l < depth; ++l) {
            const bool last = l == depth - 1;
            const int out = last ? net->obs_out[o] : net->obs_hid[o];
            float* y = last ? w.cat + co : ((l & 1) ? w.oh1 : w.oh0);
            const int64_t wl = net->obs_depth[o] ? net->obs_w[o][l] : (l == 0 ? net->obs_w0[o] : net->obs_w1[o]);
            const int64_t bl = net->obs_depth[o] ? net->obs_b[o][l] : (l == 0 ? net->obs_b0[o] : net->obs_b1[o]);
            PP_TRY(lin(x, ldx, P + wl, P + bl, nullptr, y, last ? w.e4 : w.ohid4, M, in, out, true, st));
            x = y; ldx = last ? w.e4 : w.ohid4; in = out;
        }
        ci += net->obs_in[o];
        co += net->obs_out[o];
    }
    PP_TRY(lin(w.cat, w.e4, P + net->fin_w0, P + net->fin_b0, nullptr, w.f1, w.e4, M, net->e_obs, net->e_obs, true, st));
    PP_TRY(lin(w.f1, w.e4, P + net->fin_w1, P + net->fin_b1, nullptr, w.E, w.e4, M, net->e_obs, net->e_obs, true, st));
    // _infer_step(prev_variable = None): zero state and a zero previous-sample embedding for every row
    // (inference_network_lstm.py:82-134); FeedForward network: the proposal layer reads the embedding
    // (inference_network_feedforward.py:52-66)
    const float* top = w.E;
    int64_t ldtop = w.e4;
    int Hin = net->e_obs;
    if (net->lstm_dim > 0) {
        const int H = net->lstm_dim;
        float* h = h_out ? h_out : w.h;
        float* c = c_out ? c_out : w.c;
        PP_TRY(lstm_input_gather(net, P, w.E, w.e4, nullptr, nullptr, nullptr, nullptr, addr_id, -1, M, w.X, w.i4, st));
        PP_TRY(lin(w.X, w.i4, P + net->w_ih, P + net->b_ih, P + net->b_hh, w.G, 4 * (int64_t)H, M, net->lstm_in, 4 * H, false, st));
        PP_TRY(lstm_cell_fwd(w.G, nullptr, c, h, M, H, st));
        top = h; ldtop = H; Hin = H;
    }
    PP_TRY(lin(top, ldtop, P + ad.w1, P + ad.b1, nullptr, w.A1, w.hid4, M, Hin, ad.hid, true, st));
    PP_TRY(lin(w.A1, w.hid4, P + ad.w2, P + ad.b2, nullptr, y_out, ldy, M, ad.hid, ad.n_out, false, st));
    return 0;
}

int is_fused_groups(const pp_net* net, int addr_id, int M, int n_per, const float* y, int64_t ldy, const float* prior,
                    const pp_lw_term* terms, const int32_t* term_flags, int n_terms, float* value, float* lw, int overwrite,
                    uint64_t seed, uint64_t offset, double* stats_out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(net && value && lw && M >= 0 && n_per >= 1 && n_terms >= 0 && n_terms <= GROUP_MAX_TERMS && (!n_terms || terms),
                 "pp_is_fused_groups: bad argument (a network, value and lw, n_per >= 1, at most %d terms)", GROUP_MAX_TERMS);
    GroupTerms t;
    memset(&t, 0, sizeof(t));
    t.count = n_terms;
    for (int q = 0; q < n_terms; ++q) {
        const pp_lw_term& s = terms[q];
        const int fl = term_flags ? term_flags[q] : 0;
        const bool two = s.kind == 0 || s.kind == 1;
        const auto code_ok = [](int c) { return c >= 0 && c <= 2; };
        // (the stride fields carry the operand codes; Categorical keeps its category count in p1_stride as in pp_lw_term)
        PP_CHECK_ARG(s.kind >= 0 && s.kind <= 5 && !(!(fl & 4) && !s.x) && !(s.kind != 2 && !((fl & 1) || s.p0)) &&
                         !(two && !((fl & 2) || s.p1)) && !((fl & 3) && !two) && !(s.kind == 5 && s.p1_stride < 1) &&
                         code_ok(s.p0_stride) && code_ok(s.x_stride) && (s.kind == 5 || code_ok(s.p1_stride)),
                     "pp_is_fused_groups: bad term %d", q);
        t.t[q] = GroupTerm{s.kind, s.p0_stride, s.kind == 5 ? 0 : s.p1_stride, s.x_stride, fl, s.kind == 5 ? s.p1_stride : 1,
                           s.p0, s.p1, s.x, s.scale};
    }
    int kind = -1, K = 0;
    if (addr_id >= 0) {
        PP_CHECK_ARG(y && prior && addr_id < net->n_addr, "pp_is_fused_groups: a draw needs the head outputs, the prior parameters and a valid address");
        const pp_addr& ad = net->addrs[addr_id];
        PP_CHECK_ARG((ad.kind == PP_HEAD_NORMAL_MIXTURE || ad.kind == PP_HEAD_TRUNCNORMAL_MIXTURE || ad.kind == PP_HEAD_POISSON_TN_MIXTURE) &&
                         ad.n_out % 3 == 0 && ad.n_out / 3 <= MAXK,
                     "pp_is_fused_groups: mixture heads only");
        PP_CHECK_ARG(ldy >= ad.n_out, "pp_is_fused_groups: ldy is smaller than the head's %d outputs", ad.n_out);
        kind = ad.kind == PP_HEAD_NORMAL_MIXTURE ? 0 : (ad.kind == PP_HEAD_TRUNCNORMAL_MIXTURE ? 1 : 2);
        K = ad.n_out / 3;
    }
    double* partial = nullptr;      // the partial records: the FIRST block of the batch workspace (batch_carve), nothing else is used
    if (stats_out) {
        PP_CHECK_ARG(ws, "pp_is_fused_groups: the statistics need the workspace");
        const size_t need = stats_workspace_bytes(M);
        if (need > ws_bytes) {
            set_error("pp_is_fused_groups: workspace too small (%zu < %zu bytes)", ws_bytes, need);
            return PP_ENOSPACE;
        }
        partial = static_cast<double*>(ws);
    }
    if (M == 0) return 0;
    const int64_t total = (int64_t)M * n_per;
    const int prior_pp = (overwrite & PP_GROUPS_PRIOR_PER_PARTICLE) ? 1 : 0;
    overwrite &= 1;
    const int blocks = (int)std::min<int64_t>(GROUP_BLOCKS, (total + 255) / 256);
#define PP_GROUPS_LAUNCH(KIND)                                                                                              \
    hipLaunchKernelGGL(is_fused_groups_kernel<KIND>, dim3(blocks), dim3(256), 0, st, y, ldy, prior, total, n_per, K, t, value, lw, \
                       overwrite, seed, offset, prior_pp)
    if (kind < 0) PP_GROUPS_LAUNCH(-1);
    else if (kind == 0) PP_GROUPS_LAUNCH(0);
    else if (kind == 1) PP_GROUPS_LAUNCH(1);
    else PP_GROUPS_LAUNCH(2);
#undef PP_GROUPS_LAUNCH
    PP_LAUNCH_CHECK("pp_is_fused_groups");
    if (!stats_out) return 0;
    // the statistics as dependent launches on the same stream: the slices of every group, then (more than one slice) the combine
    const int B = stat_slices(n_per);
    const int slice = cdiv(n_per, B);
    const int slots = std::max(M, STAT_MIN_SLOTS);
    const int per_launch = B == 1 ? 65535 : std::min(65535, std::max(1, slots / B));
    for (int g0 = 0; g0 < M; g0 += per_launch) {
        const int groups = std::min(per_launch, M - g0);
        double* dst = B == 1 ? stats_out + (int64_t)g0 * 6 : partial;
        hipLaunchKernelGGL(group_stats_kernel, dim3(B, groups), dim3(256), 0, st, (const float*)lw, (const float*)value, n_per, slice, g0, dst);
        if (B > 1)
            hipLaunchKernelGGL(group_combine_kernel, dim3(cdiv(groups, 256)), dim3(256), 0, st, (const double*)partial, B, groups,
                               stats_out + (int64_t)g0 * 6);
    }
    PP_LAUNCH_CHECK("pp_is_fused_groups(statistics)");
    return 0;
}

// ---- later statements of a batched call ---------------------------------------------------------------------------------------
// The bias rows of statement (addr_id, prev_addr_id >= 0) for the groups: is_prep_kernel's bias code (is_step_fused.hip) on a grid
// of (gate columns, groups) - the same products in the same order as the single call's row, so a group's row does not depend on
// how many groups the call has. A workgroup serves four gate columns (one wave each) x BIAS_GROUPS groups: the weight rows are read
// once for all of them.
constexpr int BIAS_GROUPS = 4;

struct BiasArgs {
    const float* P;
    const int64_t* at;
    int64_t w_ih, w_hh, b_ih, b_hh;
    int H, I, M;
    GatherDims d;
    int addr_id, prev_addr;
    const float* E; int64_t lde;      // [M][lde] observe embeddings
    const float* h_prev;              // [M][H] or nullptr
    float* bias;                      // [M][4 H]
};

__global__ __launch_bounds__(256) void batch_bias_kernel(const BiasArgs a) {
    __shared__ float sx[BIAS_GROUPS][1024 + 1024];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = a.H;
    const int g0 = (int)blockIdx.y * BIAS_GROUPS, ng = min(BIAS_GROUPS, a.M - g0);
    const int n = (int)blockIdx.x * 4 + wave;      // gate column (4 H is a multiple of 4)
    const int c1 = a.d.e_obs, c2 = c1 + a.d.smp;
    const float* wi = a.P + a.w_ih + (int64_t)n * a.I;
    float acc[BIAS_GROUPS];
#pragma unroll
    for (int q = 0; q < BIAS_GROUPS; ++q) acc[q] = 0.0f;
    if (a.h_prev)
        for (int e = tid; e < ng * H; e += 256) sx[e / H][1024 + e % H] = a.h_prev[(int64_t)g0 * H + e];
    for (int base = 0; base < a.I; base += 1024) {
        const int cnt = min(1024, a.I - base);
        if (base) __syncthreads();      // the previous chunk has been consumed
        for (int kk = tid; kk < cnt; kk += 256) {
            const int k = base + kk;
            const bool obs = k < c1;
            const float shared = (obs || k < c2) ? 0.0f : gather_embedding_elem(a.d, a.P, a.at, k, a.prev_addr, 0.0f, a.addr_id);
            for (int q = 0; q < ng; ++q) sx[q][kk] = obs ? a.E[(int64_t)(g0 + q) * a.lde + k] : shared;
        }
        __syncthreads();
        for (int kk = lane; kk < cnt; kk += 64) {
            const float w = wi[base + kk];
#pragma unroll
            for (int q = 0; q < BIAS_GROUPS; ++q)
                if (q < ng) acc[q] += w * sx[q][kk];
        }
    }
    if (a.h_prev) {
        const float* wh = a.P + a.w_hh + (int64_t)n * H;
        for (int k = lane; k < H; k += 64) {
            const float w = wh[k];
#pragma unroll
            for (int q = 0; q < BIAS_GROUPS; ++q)
                if (q < ng) acc[q] += w * sx[q][1024 + k];
        }
    }
    const float b = a.P[a.b_ih + n] + a.P[a.b_hh + n];
#pragma unroll
    for (int q = 0; q < BIAS_GROUPS; ++q) {
        const float r = wave_sum(acc[q]);
        if (q < ng && lane == 0) a.bias[(int64_t)(g0 + q) * 4 * H + n] = r + b;
    }
}

int is_batch_bias(const pp_net* net, const float* P, int addr_id, int prev_addr_id, int M, int ws_groups, int first_group,
                  const float* h_prev, float* bias_out, void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(net && P && bias_out && ws, "pp_is_batch_bias: null pointer");
    PP_CHECK_ARG(batch_net_ok(net) && net->lstm_dim > 0 && net->lstm_dim <= 1024 && net->addr_table,
                 "pp_is_batch_bias: FEEDFORWARD or CNN2D5C observe embeddings and an LSTM of depth 1 with at most 1024 hidden units");
    PP_CHECK_ARG(addr_id >= 0 && addr_id < net->n_addr && prev_addr_id >= 0 && prev_addr_id < net->n_addr,
                 "pp_is_batch_bias: a statement after the first one (address ids in range, prev_addr_id >= 0)");
    PP_CHECK_ARG(M >= 0 && first_group >= 0 && (int64_t)first_group + M <= ws_groups,
                 "pp_is_batch_bias: groups [first_group, first_group + n_groups) of the ws_groups rows pp_is_batch_first embedded");
    {
        const int kind = net->addrs[addr_id].kind;
        PP_CHECK_ARG(kind == PP_HEAD_NORMAL_MIXTURE || kind == PP_HEAD_TRUNCNORMAL_MIXTURE,
                     "pp_is_batch_bias: Normal / Uniform statements (mixture heads) only: the rows are pp_is_statement_groups' operand");
    }
    if (M == 0) return 0;
    BatchWorkspace w;
    batch_carve(net, ws_groups, ws, w);      // (as the pp_is_batch_first call carved it: that is where its embedding rows are)
    if (w.bytes > ws_bytes) {
        set_error("pp_is_batch_bias: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return PP_ENOSPACE;
    }
    BiasArgs a{};
    a.P = P; a.at = net->addr_table;
    a.w_ih = net->w_ih; a.w_hh = net->w_hh; a.b_ih = net->b_ih; a.b_hh = net->b_hh;
    a.H = net->lstm_dim; a.I = net->lstm_in; a.M = M;
    a.d = GatherDims{net->e_obs, net->smp_dim, net->dtype_dim, net->addr_dim, net->lstm_in};
    a.addr_id = addr_id; a.prev_addr = prev_addr_id;
    a.E = w.E + (int64_t)first_group * w.e4; a.lde = w.e4;
    a.h_prev = h_prev; a.bias = bias_out;
    for (int g0 = 0; g0 < M; g0 += 65535 * BIAS_GROUPS) {
        const int groups = std::min(M - g0, 65535 * BIAS_GROUPS);
        BiasArgs q = a;
        q.M = groups;
        q.E = a.E + (int64_t)g0 * a.lde;
        q.h_prev = h_prev ? h_prev + (int64_t)g0 * a.H : nullptr;
        q.bias = bias_out + (int64_t)g0 * 4 * a.H;
        hipLaunchKernelGGL(batch_bias_kernel, dim3(a.H, cdiv(groups, BIAS_GROUPS)), dim3(256), 0, st, q);
    }
    PP_LAUNCH_CHECK("pp_is_batch_bias");
    return 0;
}

int is_batch_statement_groups(const pp_net* net, const float* P, int addr_id, int prev_addr_id, int M, int n_per, const float* bias,
                              const float* c0, const float* prev_value, const float* prior, int prior_stride, float* h, float* c,
                              float* value, float* lw, int prior_kind, uint64_t seed, uint64_t offset, float* y_out, int64_t ldy,
                              void* ws, size_t ws_bytes, hipStream_t st) {
    PP_CHECK_ARG(net && P && bias && prev_value && prior && h && c && value && lw && ws, "pp_is_statement_groups: null pointer");
    PP_CHECK_ARG(M >= 0 && n_per >= 1, "pp_is_statement_groups: n_groups >= 0 and n_per >= 1");
    PP_CHECK_ARG(addr_id >= 0 && addr_id < net->n_addr && prev_addr_id >= 0 && prev_addr_id < net->n_addr,
                 "pp_is_statement_groups: a statement after the first one (address ids in range, prev_addr_id >= 0)");
    PP_CHECK_ARG((prior_kind == 0 || prior_kind == 1) && (prior_stride == 0 || prior_stride == 1),
                 "pp_is_statement_groups: Normal (0) or Uniform (1) prior, one shared pair (stride 0) or one pair per particle (1)");
    const pp_addr& ad = net->addrs[addr_id];
    PP_CHECK_ARG((ad.kind == PP_HEAD_NORMAL_MIXTURE || ad.kind == PP_HEAD_TRUNCNORMAL_MIXTURE) && ad.n_out % 3 == 0 && ad.n_out / 3 <= MAXK,
                 "pp_is_statement_groups: Normal / Uniform statements (mixture heads) only");
    PP_CHECK_ARG(is_statement_groups_supported(net, addr_id),
                 "pp_is_statement_groups: no fused statement kernel for this network and address (one-layer LSTM of H = 32 .. 512, head of at "
                 "most 32 outputs)");
    PP_CHECK_ARG(!y_out || ldy >= ad.n_out, "pp_is_statement_groups: ldy is smaller than the head's %d outputs", ad.n_out);
    PP_CHECK_ARG((int64_t)M * n_per * net->lstm_dim < (int64_t(1) << 32) && (int64_t)M * n_per <= 0x7fffffff,
                 "pp_is_statement_groups: more than 2^32 state elements per call: shard the groups");
    if (M == 0) return 0;
    BatchWorkspace w;
    batch_carve(net, M, ws, w);
    if (w.bytes > ws_bytes) {
        set_error("pp_is_statement_groups: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return PP_ENOSPACE;
    }
    const IsStatementOut whole{value, lw, prior_kind};
    return is_statement_groups(net, P, addr_id, prev_addr_id, M, n_per, bias, c0, prev_value, prior, prior_stride, h, c, whole, seed,
                               offset, w.fz, y_out, ldy, st);
}

}  // namespace pp

extern "C" {

size_t pp_is_batch_workspace_bytes(const pp_net* net, int32_t n_groups) {
    if (!net || n_groups < 0) return 0;
    pp::BatchWorkspace w;
    pp::batch_carve(net, n_groups, nullptr, w);
    return w.bytes;
}

int pp_is_batch_first(const pp_net* net, const float* params, const float* obs, int32_t addr_id, int32_t n_groups, float* y_out,
                      int64_t ldy, float* h_out, float* c_out, void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_batch_first(net, params, obs, addr_id, n_groups, y_out, ldy, h_out, c_out, workspace, workspace_bytes,
                              pp::as_stream(stream));
}

int pp_is_fused_groups(const pp_net* net, int32_t addr_id, int32_t n_groups, int32_t n_per, const float* y, int64_t ldy,
                       const float* prior, const pp_lw_term* terms, const int32_t* term_flags, int32_t n_terms, float* value,
                       float* lw, int32_t overwrite, uint64_t seed, uint64_t offset, double* stats_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return pp::is_fused_groups(net, addr_id, n_groups, n_per, y, ldy, prior, terms, term_flags, n_terms, value, lw, overwrite, seed,
                               offset, stats_out, workspace, workspace_bytes, pp::as_stream(stream));
}

int pp_is_batch_bias(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n_groups,
                     int32_t ws_groups, int32_t first_group, const float* h_prev, float* bias_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return pp::is_batch_bias(net, params, addr_id, prev_addr_id, n_groups, ws_groups, first_group, h_prev, bias_out, workspace,
                             workspace_bytes, pp::as_stream(stream));
}

int pp_is_statement_groups(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n_groups,
                           int32_t n_per, const float* bias, const float* c0, const float* prev_value, const float* prior,
                           int32_t prior_stride, float* h, float* c, float* value, float* lw, int32_t prior_kind, uint64_t seed,
                           uint64_t offset, float* y_out, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream) {
    return pp::is_batch_statement_groups(net, params, addr_id, prev_addr_id, n_groups, n_per, bias, c0, prev_value, prior, prior_stride,
                                         h, c, value, lw, prior_kind, seed, offset, y_out, ldy, workspace, workspace_bytes,
                                         pp::as_stream(stream));
}

}  // extern "C"
