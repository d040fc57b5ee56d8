// Host-side orchestration behind the C ABI: InferenceNetworkLSTM._loss (+ backward) as a chain of HIP kernels over
// the step-major packed trace batch. No allocation, no host synchronisation: every launch goes to the caller's stream.
#include "common.hpp"
#include "gather.hpp"
#include "aux_jobs.hpp"
#include "panel.hpp"
#include "panel16.hpp"
#include "wgrad_t1.hpp"
#include "cnn2d.hpp"
#include "adam_live.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace pp {

// kernels.hip / gemm_f32.hip
const char* last_error();
int colsum_multi(const ColsumJob* jobs, int count, hipStream_t st, const float* fin_acc = nullptr,
                 const int32_t* fin_flag = nullptr, int fin_traces = 0, float* fin_loss = nullptr,
                 int32_t* fin_status = nullptr);
int colsum_f32(const float* X, int64_t ldx, const int32_t* idx, int n_rows, int n_cols, float* out, float* out2,
               hipStream_t st);
int embedding_rows(const float* E, int64_t lde, const int32_t* trace, int n_rows, int e_obs, float* Hs, int64_t ldh,
                   float* zero_small, int n_small, hipStream_t st);
int sample_embed_bwd(const pp_net* net, const float* params, const float* value, const int32_t* addr,
                     const int32_t* prev_row, int row_begin, int n_rows, const float* dX, int64_t ldx, float* grads,
                     hipStream_t st);
// lstm_tail.hip: the late time steps of a ragged batch in one launch per direction
bool dp_overlap_hull(int64_t* lo, int64_t* hi);          // dp.hip
int dp_bucket0_issue(float* grads_full, hipStream_t st);
int lstm_tail_plan(const int32_t* n_active, int T, int H, int* t0_out, int* teams_out);
void lstm_tail_exchange_bytes(int H, size_t* fwd, size_t* bwd);
int lstm_tail_fwd(float* G, float* C, float* Hs, const float* Whh, const int32_t* row_off_dev, int t0, int T, int H, int teams,
                  void* xch_f, void* xch_b, int32_t* flag, hipStream_t st);
int lstm_tail_bwd(float* G, const float* C, float* dH, float* dC, const float* Whh, const int32_t* row_off_dev, int t0, int T,
                  int H, int teams, void* xch_f, void* xch_b, int32_t* flag, float* db, float* db2, const LossFinalize& fin,
                  hipStream_t st);
int obs_grad(const float* dX, int64_t ldx, const int32_t* row_off_dev, int t_max, int n_traces, int e_obs,
             const float* E, int64_t lde, float* dE, int64_t ldde, hipStream_t st);
int lstm_cell_fwd(float* G, const float* c_prev, float* c, float* h, int n, int H, hipStream_t st, int c_prev_shared = 0);
int lstm_cell_bwd(float* G, const float* c_prev, const float* c, const float* dh, float* dc_carry, int n, int n_next,
                  int H, float* db, float* db2, hipStream_t st, const float* fin_acc = nullptr,
                  const int32_t* fin_flag = nullptr, int fin_traces = 0, float* fin_loss = nullptr,
                  int32_t* fin_status = nullptr, const float* dh_parts = nullptr, int n_parts = 0, int64_t part_stride = 0);
int head_logprob(int kind, const float* y, int64_t ldy, const int32_t* rows, const float* value, const float* prior,
                 int n, int n_out, float grad_scale, float* lp_out, float* dy, float* loss_acc, int32_t* nonfinite,
                 hipStream_t st);
bool head_tail_supported(int kind, int hid, int n_out);
struct TailJob {
    const float* A1; const float* W2; const float* b2; const int32_t* rows; float* DY; float* dZ1; int n;
};
int head_tail_multi(int kind, const TailJob* jobs, int count, int64_t lda1, int hid, int n_out, const float* value,
                    const float* prior, float grad_scale, float* lp_out, int64_t lddy, int64_t lddz, float* loss_acc,
                    int32_t* nonfinite, hipStream_t st);
int loss_finalize(const float* acc, const int32_t* flag, int n_traces, float* loss_out, int32_t* status_out,
                  hipStream_t st);
int loss_from_rows(const float* lp, int n_rows, int n_traces, const int32_t* flag, float* loss_out, int32_t* status_out,
                   hipStream_t st);
int sample_embed_bwd_det(const pp_net* net, const float* params, const float* value, const int32_t* prev_row,
                         const int32_t* nxt_rows, const int32_t* nxt_off, const float* dX, int64_t ldx, float* grads,
                         hipStream_t st);
int adam_step(float* params, float* grads, float* m, float* v, int64_t n_params, const int32_t* chunk_tensor,
              const float* active, int32_t* tensor_step, int32_t* arrived, int n_tensors, float lr, float beta1, float beta2,
              float eps, float wd, float gscale, int flags, const int32_t* skip, hipStream_t st);
int adam_step_live(float* params, float* grads, float* m, float* v, int64_t n_params, const int32_t* chunk_tensor,
                   const float* active, int32_t* tensor_step, int32_t* arrived, int n_tensors, float lr, float beta1, float beta2,
                   float eps, float wd, float gscale, int flags, const int32_t* skip, hipStream_t st);
int adam_live_bind(const float* grads, const float* m, const float* v, int64_t n_params, const int32_t* first, int n_tensors,
                   bool clean);
void adam_live_unbind(const float* grads);
bool adam_live_table(const float* grads, const float* m, const float* v, int64_t n_params, int n_tensors, bool wd_on,
                     AdamLiveTable& tab);
int adam_live_info(const float* grads, int64_t* out, uint8_t* touched_out);

extern long long* g_timeline;   // kernels.hip

// obs_embed.hip (obs_embed.hpp: obs_fused_supported, obs_fused_args)
int obs_embed_dgrad_fused(const pp_net* net, const float* P, int n_traces, float* const* obs_h, const float* cat,
                          const float* f1, const float* dX, int64_t ldx, const int32_t* row_off_dev, int t_max,
                          const float* E, float* dE, float* dF1, float* dCat, float* dHo0, int64_t dh_stride,
                          hipStream_t st, int n_split = 1, int64_t split_stride = 0);

static inline int64_t round4(int64_t x) { return (x + 3) & ~int64_t(3); }

// ---- in-stream kernel timing (bench.py roofline leg) ---------------------------------------------------
struct Prof {
    int which = -1;
    std::vector<hipEvent_t> ev0, ev1;
    std::vector<double> flops;
    int used = 0;
    int stride = 1, seen = 0;      // an event pair around every stride-th launch of the class (pp_prof_stride)
    bool cur = false;
};
static Prof g_prof;

void prof_begin(int which, hipStream_t st) {
    if (g_prof.which != which) return;
    g_prof.cur = (g_prof.seen++ % g_prof.stride) == 0 && g_prof.used < (int)g_prof.ev0.size();
    if (g_prof.cur) (void)hipEventRecord(g_prof.ev0[g_prof.used], st);
}
void prof_end(int which, double flops, hipStream_t st) {
    if (g_prof.which == which && g_prof.cur) {
        (void)hipEventRecord(g_prof.ev1[g_prof.used], st);
        g_prof.flops[g_prof.used] = flops;
        g_prof.used++;
        g_prof.cur = false;
    }
}

// ---- workspace carving ------------------------------------------------------------------------------
struct Carver {
    char* base;
    size_t off = 0, cap;
    Carver(void* p, size_t c) : base(static_cast<char*>(p)), cap(c) {}
    template <typename T>
    T* take(int64_t count) {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (size_t)std::max<int64_t>(count, 1) * sizeof(T);
        return p;
    }
};

struct Workspace {
    // forward activations
    float* obs_h[PP_MAX_OBS];  // [B, round4(obs_hid)] (first hidden layer; depth 2: the only one)
    float* obs_hl[PP_MAX_OBS][PP_MAX_OBS_DEPTH];   // hidden activations of layer l < depth - 1 (obs_hl[o][0] == obs_h[o])
    float* dObsH2;             // second [B, maxhid4] scratch of the generic-depth backward
    float* cat;                // [B, e4] concatenated per-observable embeddings
    float* f1;                 // [B, e4] hidden layer of the final observe embedding
    float* E;                  // [B, e4] observe embedding
    float* X;                  // [R, i4] LSTM input rows
    float* G;                  // [R, 4H] gate pre-activations -> gates -> dG   (layer 0; layer k: Gl[k] ...)
    float* C;                  // [R, H]
    float* Hs;                 // [R, H] hidden states of the TOP layer (what the proposal heads read)
    float* Gl[PP_MAX_LSTM_DEPTH];   // per layer of nn.LSTM(I, H, depth): Gl[0] == G, Hl[depth - 1] == Hs
    float* Cl[PP_MAX_LSTM_DEPTH];
    float* Hl[PP_MAX_LSTM_DEPTH];
    float* dH2;                // [R, H] gradient into the hidden states of the layer below (depth > 1)
    float* A1;                 // [R, hid4] head hidden activations, group-compact row order
    float* Y;                  // [R, out4] head outputs
    float* DY;                 // [R, out4]
    // backward
    float* dZ1;                // [R, hid4]
    float* dH;                 // [R, H]
    float* dC;                 // [B, H]
    float* dHp;                // [DH_SPLITS][B, H] partial tiles of the recurrent data-gradient product (see ic_loss)
    float* dX;                 // [R, i4]
    float* dE;                 // [B, e4]
    float* dF1;                // [B, e4]
    float* dCat;               // [B, e4]
    float* dObsH;              // n_obs x [B, maxhid4] (observable o at dObsH + o * B * maxhid4)
    float* loss_acc;           // [1]
    int32_t* flag;             // [1]
    void* xch_f;               // granule exchange areas of the LSTM tail kernels: at the START of the workspace (a fixed
    void* xch_b;               // place whatever the batch size), zero when the workspace was allocated (see the header)
    float* lp_rows;            // [R] per-row proposal log_prob (deterministic mode: the loss is reduced from it)
    float* AB;                 // [n_addr][2][4H] per-address bias vectors of the LSTM input (gather.hpp, AddrBias)
    float* gsum;               // [n_addr][2][4H] column sums of dG per address group (current | previous statement)
    float* WihT;               // [e_obs][4H] k-major copy of W_ih[:, :e_obs] (panel.hpp), rewritten every step
    float* W1T;                // [H][64 ceil(maxhid / 64)] k-major copy of the present address's first head layer
    unsigned long long* xz; unsigned long long* xd; int32_t* epoch;   // pair hand-off of the panel launch (panel.hpp)
    Panel16Images p16;         // fragment images of the 16-row panel kernel (panel16_images.hpp), rewritten every step
    bool compact;              // LSTM input rows are [E | s_prev] (i4 = round4(e_obs + smp_dim)), the table columns a bias
    int xc;                    // columns of an LSTM input row: e_obs + smp_dim (compact) or lstm_in
    int64_t e4, i4, hid4, out4, ohid4[PP_MAX_OBS], maxohid4;
    // CNN2D5C observables (cnn2d.hip): features [B, f4] in front of _lin1, their gradient, the convolution stack's workspace
    // (saved activations, gradient ping-pong, weight images, split-K partials)
    float* cnn_feat[PP_MAX_OBS]; float* cnn_dfeat[PP_MAX_OBS]; void* cnn_ws[PP_MAX_OBS]; size_t cnn_ws_bytes[PP_MAX_OBS];
    int64_t f4[PP_MAX_OBS];
    size_t bytes;
};

// Switches of the training step (A/B measurements, tests; all default 1), read together, once per process, as
// deterministic_mode() is: at the first workspace-size query or step, whichever comes first (carve needs PP_ADDR_BIAS)
struct StepEnv {
    int addr_bias, dx_partials, fuse_cell_bwd, fuse_cell, gemm_holes, cell_lean, fuse_cell_rec, dh_partials, aux_colsum;
    int first_early;   // PP_FIRST_EARLY: the first launch's embedding workgroups in their early order (obs_embed.hip); 0 = the order before
};
static int env_flag(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static const StepEnv& step_env() {
    static const StepEnv env{env_flag("PP_ADDR_BIAS", 1),     env_flag("PP_DX_PARTIALS", 1),   env_flag("PP_FUSE_CELL_BWD", 1),
                             env_flag("PP_FUSE_CELL", 1),     env_flag("PP_GEMM_HOLES", 1),    env_flag("PP_CELL_LEAN", 1),
                             env_flag("PP_FUSE_CELL_REC", 1), env_flag("PP_DH_PARTIALS", 1),   env_flag("PP_AUX_COLSUM", 1),
                             env_flag("PP_FIRST_EARLY", 1)};
    return env;
}

// The address terms of the LSTM input as a per-address bias (gather.hpp): the default for LSTM networks whose dimensions
// allow 16-byte pieces; PP_ADDR_BIAS=0 and the deterministic mode keep the full-width rows (A/B measurements, tests).
static bool compact_rows(const pp_net* net) {
    if (!step_env().addr_bias || deterministic_mode() || net->lstm_dim == 0) return false;
    const int c2 = net->e_obs + net->smp_dim, ne = net->dtype_dim + net->addr_dim;
    return net->lstm_in % 4 == 0 && c2 % 4 == 0 && net->lstm_dim % 16 == 0 && ne >= 2 && ne % 2 == 0 && ne <= 128 && net->n_addr >= 1 &&
           net->n_addr <= 1024 && net->addr_table != nullptr;
}
constexpr int DX_SPLITS = 16;
constexpr int DH_SPLITS = 8;

static void carve(const pp_net* net, int B, int R, void* p, size_t cap, Workspace& w) {
    Carver c(p, cap);
    const bool ff = net->lstm_dim == 0;   // FeedForward network: no LSTM buffers, the heads read rows of width e_obs
    const int H = ff ? net->e_obs : net->lstm_dim;
    {   // first, so that their place does not depend on (B, R): the tail kernels' tags outlive a call
        size_t fb = 0, bb = 0;
        if (!ff) lstm_tail_exchange_bytes(H, &fb, &bb);
        w.xch_f = c.take<char>((int64_t)fb);
        w.xch_b = c.take<char>((int64_t)bb);
        // epoch of the panel launch's pair hand-off: a fixed place too (it counts the steps of this workspace)
        w.epoch = c.take<int32_t>(16);
    }
    w.e4 = round4(net->e_obs);
    w.compact = compact_rows(net);
    w.xc = w.compact ? net->e_obs + net->smp_dim : net->lstm_in;
    w.i4 = round4(w.xc);
    int64_t hid = 1, out = 1;
    for (int a = 0; a < net->n_addr; ++a) {
        hid = std::max<int64_t>(hid, net->addrs[a].hid);
        out = std::max<int64_t>(out, net->addrs[a].n_out);
    }
    w.hid4 = round4(hid);
    w.out4 = round4(out);
    w.maxohid4 = 4;
    for (int o = 0; o < net->n_obs; ++o) {
        w.ohid4[o] = round4(net->obs_hid[o]);
        w.maxohid4 = std::max(w.maxohid4, w.ohid4[o]);
        w.obs_h[o] = c.take<float>((int64_t)B * w.ohid4[o]);
        const int depth = net->obs_depth[o] ? net->obs_depth[o] : 2;
        for (int l = 0; l < PP_MAX_OBS_DEPTH; ++l) w.obs_hl[o][l] = nullptr;
        w.obs_hl[o][0] = w.obs_h[o];
        for (int l = 1; l + 1 < depth; ++l) w.obs_hl[o][l] = c.take<float>((int64_t)B * w.ohid4[o]);
    }
    w.cat = c.take<float>((int64_t)B * w.e4);
    w.f1 = c.take<float>((int64_t)B * w.e4);
    w.E = c.take<float>((int64_t)B * w.e4);
    w.X = c.take<float>(ff ? 0 : (int64_t)R * w.i4);
    const int L = ff ? 1 : std::max(1, std::min((int)net->lstm_depth, PP_MAX_LSTM_DEPTH));
    for (int l = 0; l < PP_MAX_LSTM_DEPTH; ++l) w.Gl[l] = w.Cl[l] = w.Hl[l] = nullptr;
    for (int l = 0; l < L; ++l) {
        w.Gl[l] = c.take<float>(ff ? 0 : (int64_t)R * 4 * H);
        w.Cl[l] = c.take<float>(ff ? 0 : (int64_t)R * H);
        w.Hl[l] = c.take<float>((int64_t)R * H);
    }
    w.G = w.Gl[0];
    w.C = w.Cl[0];
    w.Hs = w.Hl[L - 1];
    w.dH2 = c.take<float>(L > 1 ? (int64_t)R * H : 0);
    w.A1 = c.take<float>((int64_t)R * w.hid4);
    w.Y = c.take<float>((int64_t)R * w.out4);
    w.DY = c.take<float>((int64_t)R * w.out4);
    w.dZ1 = c.take<float>((int64_t)R * w.hid4);
    w.dH = c.take<float>((int64_t)R * H);
    w.dC = c.take<float>(ff ? 0 : (int64_t)B * H);
    w.dHp = c.take<float>(ff ? 0 : (int64_t)B * H * DH_SPLITS);   // stored K-split partials of dh_{t-1} += dG_t W_hh
    // (compact rows: room for the partial tiles of up to DX_SPLITS K splits of dX, see ic_loss)
    w.dX = c.take<float>(ff ? 0 : (int64_t)R * w.i4 * (w.compact ? DX_SPLITS : 1));
    w.dE = c.take<float>((int64_t)B * w.e4);
    w.dF1 = c.take<float>((int64_t)B * w.e4);
    w.dCat = c.take<float>((int64_t)B * w.e4);
    w.dObsH = c.take<float>((int64_t)net->n_obs * B * w.maxohid4);
    w.dObsH2 = c.take<float>((int64_t)B * w.maxohid4);
    // 64 loss accumulator slots, one per 128-byte line (atomics to one line serialise in its L2 channel), then the
    // non-finite flag; cleared by the step's first kernel
    w.loss_acc = c.take<float>(PP_LOSS_SLOTS_FLOATS);
    w.flag = reinterpret_cast<int32_t*>(w.loss_acc ? w.loss_acc + 64 * 32 : nullptr);
    w.lp_rows = c.take<float>(deterministic_mode() ? R : 0);
    w.AB = c.take<float>(w.compact ? (int64_t)net->n_addr * 2 * 4 * H : 0);
    w.gsum = c.take<float>(w.compact ? (int64_t)net->n_addr * 2 * 4 * H : 0);
    const bool panel_shape = w.compact && (H == 512 || H == 1024);
    w.WihT = c.take<float>(panel_shape ? (int64_t)net->e_obs * (4 * H + 64) : 0);
    w.W1T = c.take<float>(panel_shape ? (int64_t)H * 64 * ((hid + 63) / 64) : 0);
    // pair hand-off of the split panel launch: partial sums [panels][2][8][hid4] and [panels][2][8][64], flags, epoch
    // (sized for whichever panel kernel takes the batch: two workgroups per 8-row panel / four per 16-row panel)
    const int64_t n_pan = (B + 7) / 8;
    w.xz = c.take<unsigned long long>(panel_shape ? std::max<int64_t>(n_pan * 2 * 8 * w.hid4, panel16_xz_granules(B, H)) : 0);
    w.xd = c.take<unsigned long long>(panel_shape ? std::max<int64_t>(n_pan * 2 * 8 * 64, panel16_xd_granules(B)) : 0);
    w.p16 = Panel16Images{};
    if (panel_shape && net->e_obs == 64) {
        panel16_image_sizes(H, hid, net->e_obs, w.p16.frags);
        for (int i = 0; i < 6; ++i) w.p16.img[i] = c.take<float>(w.p16.frags[i] * 256);
    }
    for (int o = 0; o < PP_MAX_OBS; ++o) {      // (last: a network without an image observable is carved as before)
        w.cnn_feat[o] = w.cnn_dfeat[o] = nullptr; w.cnn_ws[o] = nullptr; w.cnn_ws_bytes[o] = 0; w.f4[o] = 0;
        if (o < net->n_obs && net->obs_kind[o] == PP_OBS_CNN2D5C) {
            w.f4[o] = round4(net->obs_feat[o]);
            w.cnn_feat[o] = c.take<float>((int64_t)B * w.f4[o]);
            w.cnn_dfeat[o] = c.take<float>((int64_t)B * w.f4[o]);
            w.cnn_ws_bytes[o] = cnn_workspace_bytes(net, o, B);
            w.cnn_ws[o] = c.take<char>((int64_t)w.cnn_ws_bytes[o]);
        }
    }
    w.bytes = c.off + 256;
}

static int check_net(const pp_net* net) {
    PP_CHECK_ARG(net, "null pp_net");
    PP_CHECK_ARG(net->n_obs >= 1 && net->n_obs <= PP_MAX_OBS, "pp_net: n_obs=%d out of range", net->n_obs);
    PP_CHECK_ARG(net->lstm_dim >= 0 && net->e_obs > 0, "pp_net: bad dimensions");
    if (net->lstm_dim == 0) {   // InferenceNetworkFeedForward: no LSTM, no address / sample embeddings
        PP_CHECK_ARG(net->lstm_in == 0, "pp_net: a FeedForward network (lstm_dim 0) has lstm_in 0");
    } else {
        PP_CHECK_ARG(net->lstm_in > 0 && net->lstm_in == net->e_obs + net->smp_dim + 2 * (net->addr_dim + net->dtype_dim),
                     "pp_net: lstm_in != e_obs + smp_dim + 2*(addr_dim+dtype_dim)");
    }
    PP_CHECK_ARG(net->n_addr == 0 || net->addrs, "pp_net: addrs is null");
    PP_CHECK_ARG(net->lstm_depth >= 0 && net->lstm_depth <= PP_MAX_LSTM_DEPTH, "pp_net: lstm_depth %d out of range", net->lstm_depth);
    for (int o = 0; o < net->n_obs; ++o) {
        if (net->obs_kind[o] == PP_OBS_FEEDFORWARD) continue;
        CnnGeom g;
        PP_CHECK_ARG(net->obs_kind[o] == PP_OBS_CNN2D5C && cnn_geom(net, o, g) && g.F == net->obs_feat[o] &&
                         net->obs_in[o] == g.C * g.H * g.W && net->obs_depth[o] == 2,
                     "pp_net: observable %d: not a valid CNN2D5C description (kind %d, shape [%d, %d, %d], obs_feat %d, obs_in %d)", o,
                     net->obs_kind[o], net->obs_shape[o][0], net->obs_shape[o][1], net->obs_shape[o][2], net->obs_feat[o],
                     net->obs_in[o]);
    }
    return 0;
}

// y = act(x W^T + b): x [n, in] (ldx), W [out, in], y [n, out] (ldy)
static int linear_fwd(const float* x, int64_t ldx, const int32_t* x_idx, const float* W, const float* b, float* y,
                      int64_t ldy, int n, int in, int out, bool relu, const float* bias2, hipStream_t st,
                      const GemmHole* hole = nullptr) {
    pp_gemm_args g{};
    g.A = x; g.lda = ldx; g.a_idx = x_idx;
    g.B = W; g.ldb = in;
    g.C = y; g.ldc = ldy;
    g.M = n; g.N = out; g.K = in;
    g.bias = b; g.bias2 = bias2; g.relu = relu ? 1 : 0;
    return gemm_f32(&g, st, hole);
}

// the weight-gradient leaves of the backward pass, one grouped launch (timed as kernel class 1 when armed)
static int launch_wgrads(std::vector<pp_gemm_args>& wq, hipStream_t st, const std::vector<GemmHole>* holes = nullptr,
                         bool timed = true, const AuxJobs* aux = nullptr, bool t1 = false) {
    if (wq.empty()) return aux ? aux_jobs_launch(*aux, st) : 0;
    double flops = 0.0;
    for (const auto& g : wq) flops += 2.0 * (double)g.M * (double)g.N * (double)g.K;
    if (timed) prof_begin(1, st);
    WgradT1Args wa;
    // k-major operands stream straight into MFMA fragments (wgrad_t1.hip) unless a product needs what only the tile kernels do
    if (t1 && wgrad_t1_build(wq.data(), holes && holes->size() == wq.size() ? holes->data() : nullptr, (int)wq.size(), wa))
        PP_TRY(wgrad_t1(wa, aux, st));
    else
        PP_TRY(gemm_f32_grouped(wq.data(), (int)wq.size(), st, holes ? holes->data() : nullptr, nullptr, aux));
    if (timed) prof_end(1, flops, st);
    return 0;
}

// dW[out, in] += dz^T x  (dz [n, out] (lddz), x [n, in] (ldx, optional k-gather x_idx)): queued; all weight-gradient
// products of a backward pass are leaves of the dependency graph and run as one grouped launch (gemm_f32_grouped)
static void queue_wgrad(std::vector<pp_gemm_args>& q, const float* dz, int64_t lddz, const float* x, int64_t ldx,
                        const int32_t* x_idx, float* dW, int n, int in, int out, std::vector<GemmHole>* holes = nullptr,
                        GemmHole hole = GemmHole{}) {
    if (holes) {
        holes->resize(q.size(), GemmHole{});
        holes->push_back(hole);
    }
    pp_gemm_args g{};
    g.A = dz; g.lda = lddz; g.a_kmajor = 1;
    g.B = x; g.ldb = ldx; g.b_kmajor = 1; g.b_idx = x_idx;
    g.C = dW; g.ldc = in;
    g.M = out; g.N = in; g.K = n;
    g.accumulate = 1;
    g.split_k = 1;
    q.push_back(g);
}

static int linear_wgrad(const float* dz, int64_t lddz, const float* x, int64_t ldx, const int32_t* x_idx, float* dW,
                        float* db, float* db2, int n, int in, int out, hipStream_t st) {
    std::vector<pp_gemm_args> q;
    queue_wgrad(q, dz, lddz, x, ldx, x_idx, dW, n, in, out);
    PP_TRY(gemm_f32(&q[0], st));
    if (db) PP_TRY(colsum_f32(dz, lddz, nullptr, n, out, db, db2, st));
    return 0;
}

// dx[n, in] (lddx, optional scatter idx) = (dz W) (* relu mask); W [out, in]
static int linear_dgrad(const float* dz, int64_t lddz, const float* W, float* dx, int64_t lddx, const int32_t* dx_idx,
                        const float* mask, int64_t ldmask, int n, int in, int out, bool accumulate, hipStream_t st,
                        float* colsum = nullptr, const GemmHole* hole = nullptr) {
    pp_gemm_args g{};
    g.A = dz; g.lda = lddz;
    g.B = W; g.ldb = in; g.b_kmajor = 1;
    g.C = dx; g.ldc = lddx; g.c_idx = dx_idx;
    g.M = n; g.N = in; g.K = out;
    g.mask = mask; g.ldmask = ldmask;
    g.accumulate = accumulate ? 1 : 0;
    g.colsum = colsum;
    g.split_k = 1;
    return gemm_f32(&g, st, hole);
}

// Layer l of observable o's EmbeddingFeedForward(num_layers = depth), ReLU after every layer (embedding_feedforward.py:35-48):
// y[out] = relu(W[out, in] x + b), w / b offsets into the flat parameter (and gradient) buffer. A CNN2D5C observable's layers
// are _lin1 / _lin2 behind its convolution stack: layer 0 reads the stack's features
struct ObsLin { int in, out; int64_t w, b; };
static int obs_layers(const pp_net* net, int o) { return net->obs_depth[o] ? net->obs_depth[o] : 2; }
static ObsLin obs_lin(const pp_net* net, int o, int l) {
    const bool cnn = net->obs_kind[o] == PP_OBS_CNN2D5C, deep = net->obs_depth[o] != 0;
    ObsLin r;
    r.in = l == 0 ? (cnn ? net->obs_feat[o] : net->obs_in[o]) : net->obs_hid[o];
    r.out = l == obs_layers(net, o) - 1 ? net->obs_out[o] : net->obs_hid[o];
    r.w = deep ? net->obs_w[o][l] : (l == 0 ? net->obs_w0[o] : net->obs_w1[o]);
    r.b = deep ? net->obs_b[o][l] : (l == 0 ? net->obs_b0[o] : net->obs_b1[o]);
    return r;
}

// the observe embedding on its own: small embeddings (`fused`) in one launch (obs_embed.hip), else layer by layer
static int observe_embedding_fwd(const pp_net* net, const float* P, const float* obs, int64_t ldobs, int B, const Workspace& w,
                                 hipStream_t st, bool bwd, bool fused) {
    if (fused) return obs_embed_fwd_fused(net, P, obs, B, w.obs_h, w.cat, w.f1, w.E, st, nullptr, nullptr, nullptr, step_env().first_early);
    int ci = 0, co = 0;
    for (int o = 0; o < net->n_obs; ++o) {
        const int depth = obs_layers(net, o);
        const float* x = obs + ci;
        int64_t ldx = ldobs;
        if (net->obs_kind[o] == PP_OBS_CNN2D5C) {
            // EmbeddingCNN2D5C (embedding_cnn_2d_5c.py:32-44): the convolution stack, then _lin1 / _lin2 read its features
            PP_TRY(cnn_forward(net, o, P, x, ldx, B, w.cnn_feat[o], w.f4[o], w.cnn_ws[o], w.cnn_ws_bytes[o], bwd, st));
            x = w.cnn_feat[o]; ldx = w.f4[o];
        }
        for (int l = 0; l < depth; ++l) {
            const ObsLin ly = obs_lin(net, o, l);
            const bool last = l == depth - 1;
            float* y = last ? w.cat + co : w.obs_hl[o][l];
            const int64_t ldy = last ? w.e4 : w.ohid4[o];
            PP_TRY(linear_fwd(x, ldx, nullptr, P + ly.w, P + ly.b, y, ldy, B, ly.in, ly.out, true, nullptr, st));
            x = y; ldx = ldy;
        }
        ci += net->obs_in[o];
        co += net->obs_out[o];
    }
    PP_TRY(linear_fwd(w.cat, w.e4, nullptr, P + net->fin_w0, P + net->fin_b0, w.f1, w.e4, B, net->e_obs, net->e_obs, true,
                      nullptr, st));
    PP_TRY(linear_fwd(w.f1, w.e4, nullptr, P + net->fin_w1, P + net->fin_b1, w.E, w.e4, B, net->e_obs, net->e_obs, true,
                      nullptr, st));
    return 0;
}

// ---- the training step (ic_loss): switches, plan, phases ------------------------------------------------------------
// What ic_loss decides, all of it before the first launch (plan_step): the phases below only read it.
struct StepPlan {
    bool ff, det, bwd;             // FeedForward network (inference_network_feedforward.py:68-98); deterministic mode; backward pass
    int B, R, T, H, L, I;          // traces, rows, time steps, hidden width (FF: e_obs), LSTM layers (FF: 0), lstm_in
    // columns of an LSTM input row [E | s_prev | d_prev | a_prev | d_cur | a_cur] (gather.hpp): c1 = e_obs, the sample embedding
    // starts there, the table columns at c2, the current statement's at c4; ne = dtype_dim + addr_dim
    int c1, c2, c3, c4, c5, ne;
    // single-statement batches have no previous statement at all: the sample-embedding columns are zero in every row
    int nx;                        // columns of the compact input product: e_obs (T == 1) or c2
    uint32_t present[32];          // compact rows: bit a = address a occurs in the batch (current or previous statement)
    int n_present, only_addr;
    bool fused_obs;                // small embeddings: one fused launch per direction (obs_embed.hip)
    bool compact;                  // LSTM input rows are [E | s_prev], the table columns a per-address bias (gather.hpp)
    // Single-statement batch: dX = dG W_ih[:, :e_obs] has ONE consumer, the observe-embedding backward kernel; its K splits
    // store their partial tiles and that kernel adds them - no float atomics (6-8 us per 64 x 64 tile, tools/wg_trace.py)
    // and no cleared dX
    bool dx_partials;
    int dx_splits;                 // K splits of dX that the observe-embedding backward adds (1: complete rows)
    // (see GemmExt::lean) the cell backward of a single-statement, single-layer batch runs in the dH epilogue, and with the
    // zero blocks on neither dX nor dW_ih read the forget gate's columns of first-step rows
    // (H a multiple of 64: the zero blocks then cover the forget gate's tiles and slabs exactly; and dX as stored split
    // partials: that product then runs on the async tiles, which skip the forget gate's K range)
    bool lean_cell;
    // Single-statement batch, one LSTM layer: every row is a trace's only time step, so the cell backward needs nothing
    // but dh from the heads - it runs in the epilogue of the dH product (gemm_tile_direct), which also adds each tile's
    // column sums of dG to its address's group sums; the loss is finalised by the jobs behind the weight-gradient tiles.
    bool fused_bwd;
    // Row-panel kernel (panel.hip): a single-statement batch with ONE address keeps input product + cell, head layer 1, the
    // head tail, dz1, dH + cell backward and dX in one launch (rows of the one address group are the batch rows in order)
    bool panel;
    bool panel16_go;               // the 16-row kernel (panel16.hip) instead of the 8-row one (panel.hip)
    bool obs_tail;                 // training: the observe-embedding backward of the rows rides in the panel kernel's tail
    ObsFusedArgs obs_args;         // ... with these layer descriptions
    // ... and the FORWARD embedding in its staging phase (panel16.hip EMBED, PP_PANEL_EMBED): the first launch has no embedding
    // workgroups then. Set by ic_loss once the launch's arguments stand (panel16_embed_ok); every other path leaves it false
    bool panel_embed;
    // ragged batches: the time steps t >= tail_t0 (few rows each) of every LSTM layer run in one launch per direction
    int tail_t0, tail_teams;
    // FeedForward, single-statement batch: row r IS trace r, the heads read E in place and the embedding kernel clears the
    // loss slots - one launch less
    bool in_place;
    const float* heads_in;         // input rows of the proposal layers: LSTM outputs, or observe embeddings (FF)
    int64_t heads_ld;
    // deterministic mode: the heads write the per-row log_prob only; the loss is a fixed-order sum over the rows and the
    // kernels of the backward pass get no loss slots to fold
    float* lp_rows;
    float* loss_slots;
    const float* fin_acc;
    LossFinalize fin;              // folds the loss slots: carried by exactly one launch of a backward pass
};

static StepPlan plan_step(const pp_net* net, const pp_batch* bt, int flags, float* lp_out, float* loss_out, int32_t* status_out,
                          const Workspace& w) {
    const StepEnv& env = step_env();
    StepPlan p{};
    p.bwd = flags & PP_LOSS_BACKWARD;
    p.ff = net->lstm_dim == 0;
    p.det = deterministic_mode();
    p.B = bt->n_traces; p.R = bt->n_rows; p.T = bt->t_max; p.H = p.ff ? net->e_obs : net->lstm_dim; p.I = net->lstm_in;
    // nn.LSTM(I, H, depth), inference_network_lstm.py:31,186-188: layer k reads the hidden states of layer k - 1
    p.L = p.ff ? 0 : std::max(1, (int)net->lstm_depth);
    const int B = p.B, R = p.R, T = p.T, H = p.H;
    p.fused_obs = obs_fused_supported(net);
    p.tail_t0 = T;
    if (!p.ff) lstm_tail_plan(bt->n_active, T, H, &p.tail_t0, &p.tail_teams);
    p.compact = w.compact;
    p.c1 = net->e_obs; p.c2 = p.c1 + net->smp_dim; p.c3 = p.c2 + net->dtype_dim; p.c4 = p.c3 + net->addr_dim;
    p.c5 = p.c4 + net->dtype_dim; p.ne = net->dtype_dim + net->addr_dim;
    p.nx = (T == 1) ? net->e_obs : p.c2;
    p.dx_partials = p.compact && p.bwd && T == 1 && env.dx_partials && p.fused_obs;
    p.lean_cell = p.compact && p.bwd && T == 1 && p.L == 1 && H % 64 == 0 && env.fuse_cell_bwd && env.fuse_cell &&
                  env.gemm_holes == 1 && env.cell_lean && p.dx_partials;
    if (p.compact)
        for (int a = 0; a < net->n_addr; ++a)
            if (bt->grp_off[a + 1] > bt->grp_off[a] || bt->nxt_off[a + 1] > bt->nxt_off[a]) {
                p.present[a >> 5] |= 1u << (a & 31);
                ++p.n_present;
                p.only_addr = a;
            }
    if (p.lean_cell && p.n_present == 1 && p.fused_obs && bt->grp_off[p.only_addr] == 0 && bt->grp_off[p.only_addr + 1] == R) {
        const pp_addr& ad = net->addrs[p.only_addr];
        const bool shape_ok = head_tail_supported(ad.kind, ad.hid, ad.n_out) &&
                              w.hid4 <= ((ad.hid + 15) & ~15) && w.out4 <= 64 && (flags & PP_LOSS_KEEP_LP ? lp_out != nullptr : true);
        p.panel16_go = shape_ok && w.p16.img[0] && panel16_supported(ad.kind, H, ad.hid, ad.n_out, net->e_obs, R);
        if (p.panel16_go && p.bwd) p.panel16_go = obs_fused_args(net, w.obs_h, p.obs_args) && panel16_obs_ok(p.obs_args);
        p.panel = p.panel16_go || (shape_ok && panel_t1_supported(ad.kind, H, ad.hid, ad.n_out, net->e_obs) && panel_t1_split(R, H) == 2);
        if (p.panel)
            p.obs_tail = p.bwd && (p.panel16_go || panel_obs_tail_ok(net, H, ad.hid, ad.n_out, net->e_obs)) &&
                         obs_fused_args(net, w.obs_h, p.obs_args);
    }
    p.fused_bwd = p.compact && T == 1 && p.L == 1 && env.fuse_cell_bwd;
    // (panel: complete rows, written by the panel launch; else ~3 slabs per split - the K loop is short either way; more
    // splits = more workgroups streaming dG)
    p.dx_splits = (p.dx_partials && !p.panel) ? std::max(1, std::min(DX_SPLITS, (4 * H / 32) / 4)) : 1;
    p.in_place = p.ff && p.fused_obs && T == 1;
    p.heads_in = p.in_place ? w.E : w.Hs;
    p.heads_ld = p.in_place ? w.e4 : H;
    p.lp_rows = p.det ? (((flags & PP_LOSS_KEEP_LP) && lp_out) ? lp_out : w.lp_rows) : ((flags & PP_LOSS_KEEP_LP) ? lp_out : nullptr);
    p.loss_slots = p.det ? nullptr : w.loss_acc;
    p.fin_acc = p.det ? nullptr : w.loss_acc;
    p.fin = LossFinalize{p.fin_acc, w.flag, B > 0 ? 1.0f / (float)B : 0.0f, loss_out, status_out};
    return p;
}

// what every phase works on
struct Step {
    const pp_net* net; const pp_batch* bt; const float* P; float* grads;
    const Workspace& w; const StepPlan& p;
    hipStream_t st;
    float* lp_out; int flags;      // (loss_out / status_out: p.fin)
};
// Leaves of the backward pass, queued by its phases and launched once, at its end (reduce_and_flush): the weight-gradient
// products with their zero blocks (paired by index) and the column sums (bias / table gradients). Their ORDER is the order
// of the tiles and of the reduction jobs in that launch.
// (a second stream for these leaves with fork / join events was measured twice and lost both times - 0.157 -> 0.166 ms
// on config 2, 183 vs 170 us with two grouped launches: a cross-queue event wait costs ~5 us - and is gone)
struct GradQueue {
    std::vector<pp_gemm_args> wq;
    std::vector<GemmHole> holes;
    std::vector<ColsumJob> cs;
};
struct LstmLayer { int64_t w_ih, w_hh, b_ih, b_hh; };   // parameter offsets of layer l of nn.LSTM(I, H, depth)
static LstmLayer lstm_layer(const pp_net* net, int l) {
    if (l == 0) return LstmLayer{net->w_ih, net->w_hh, net->b_ih, net->b_hh};
    return LstmLayer{net->lstm_w_ih[l], net->lstm_w_hh[l], net->lstm_b_ih[l], net->lstm_b_hh[l]};
}

// compact rows: the step's first launch computes the per-address bias vectors of the LSTM input (reads W_ih[:, c2:I] per
// present address, writes 2 x 4H, clears the group sums)
static AddrBias addr_bias(const Step& s) {
    const pp_net* net = s.net; const Workspace& w = s.w; const StepPlan& p = s.p;
    AddrBias ab{};
    ab.AB = w.AB; ab.gsum = w.gsum; ab.step_epoch = w.epoch;
    ab.W = s.P + net->w_ih; ab.b_ih = s.P + net->b_ih; ab.b_hh = s.P + net->b_hh;
    ab.params = s.P; ab.at = net->addr_table; ab.ldw = p.I;
    ab.N = 4 * p.H; ab.c2 = p.c2; ab.c3 = p.c3; ab.c4 = p.c4; ab.c5 = p.c5; ab.I = p.I; ab.n_addr = net->n_addr;
    for (int q = 0; q < 32; ++q) ab.present[q] = p.present[q];
    // PP_ADDR_BIAS_DIRECT (default 1, read per call: the A/B arm): one present address - its embedding vectors' offsets from the
    // host's record, the table round trip leaves the bias workgroups' load chain (gather.hpp)
    const char* dv = getenv("PP_ADDR_BIAS_DIRECT");
    if (p.n_present == 1 && !(dv && atoi(dv) == 0)) {
        ab.direct_on = 1; ab.direct_addr = p.only_addr;
        ab.direct_dt = net->addrs[p.only_addr].dtype_emb; ab.direct_ad = net->addrs[p.only_addr].addr_emb;
    }
    return ab;
}
// ... and the jobs behind its weight-gradient tiles turn the group sums of dG into the table-column gradients
static void aux_derived(const Step& s, AuxJobs& aux) {
    const pp_net* net = s.net; const StepPlan& p = s.p;
    aux.gsum = s.w.gsum; aux.W = s.P + net->w_ih; aux.dW = s.grads + net->w_ih; aux.ldw = p.I;
    aux.params = s.P; aux.grads = s.grads; aux.at = net->addr_table;
    aux.N = 4 * p.H; aux.c2 = p.c2; aux.c4 = p.c4; aux.nd = net->dtype_dim; aux.ne = p.ne; aux.n_addr = net->n_addr;
    for (int q = 0; q < 32; ++q) aux.present[q] = p.present[q];
    aux.all_present = 0;
}

// the k-major weight copies (8-row kernel) or the six fragment images (16-row kernel) of the panel launch: extra workgroups
// of the first launch
static PanelTranspose panel_transpose_job(const Step& s) {
    const pp_net* net = s.net; const Workspace& w = s.w; const StepPlan& p = s.p;
    const pp_addr& ad = net->addrs[p.only_addr];
    const int H = p.H;
    PanelTranspose ptr{};
    ptr.Wih = s.P + net->w_ih; ptr.ldw = p.I; ptr.WihT = w.WihT;
    ptr.W1 = s.P + ad.w1; ptr.W1T = w.W1T; ptr.ld1T = 64 * ((ad.hid + 63) / 64);
    ptr.H = H; ptr.hid = ad.hid; ptr.e = net->e_obs;
    ptr.tiles_ih = 3 * H / 64;
    ptr.n_blocks = panel_transpose_blocks(H, ad.hid);
    if (p.panel16_go) {      // the job writes the six fragment images instead (one thread per fragment lane)
        ptr.mode16 = 1;
        ptr.wt = store_wt_mode();
        ptr.p16.W2 = s.P + ad.w2; ptr.p16.n_out = ad.n_out;
        ptr.p16.im = w.p16;
        panel16_image_sizes(H, ad.hid, net->e_obs, ptr.p16.im.frags);      // (this address's head; the buffers hold the widest)
        int nb = 0;
        for (int i = 0; i < 6; ++i) {
            ptr.p16.blocks_before[i] = nb;
            nb += cdiv(ptr.p16.im.frags[i] * 64, 256);
        }
        ptr.p16.blocks_before[6] = nb;
        ptr.n_blocks = nb;
    }
    return ptr;
}

// First launch: observe embedding; for small embeddings the same launch assembles the LSTM input rows of its traces
// and clears the loss slots and (backward) dX. Otherwise embedding GEMMs + the stand-alone gather kernel.
static int first_launch(const Step& s) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const float* P = s.P; hipStream_t st = s.st;
    const int B = p.B, R = p.R, T = p.T, H = p.H;
    const int n_clear = PP_LOSS_SLOTS_FLOATS;
    // kernel class 2 of the in-stream timing: observe embedding + LSTM input rows (the gather path). Algorithmic bytes:
    // observations and per-row (value, address, previous row) in; X rows, E / cat / f1 and the observables' hidden
    // activations out (4 I per trace-step written, 4 n_obs per trace read)
    double gather_bytes = 4.0 * B * bt->obs_width + 12.0 * R + 4.0 * (p.ff ? 0.0 : (double)R * w.xc) + 3.0 * 4.0 * B * net->e_obs;
    if (!p.ff && p.bwd) gather_bytes += 4.0 * R * w.xc;   // the same launch clears dX
    AddrBias abias{};
    if (p.compact) {
        abias = addr_bias(s);
        gather_bytes += (double)p.n_present * (4.0 * 4 * H * (2.0 * p.ne) + 4.0 * 4.0 * 4 * H);
    }
    for (int o = 0; o < net->n_obs; ++o) gather_bytes += 4.0 * B * net->obs_hid[o];
    if (p.panel_embed) {      // no embedding workgroups: the launch is its jobs (the panel launch reads the observations and writes the rows)
        gather_bytes = 0.0;
        if (p.compact) gather_bytes += (double)p.n_present * (4.0 * 4 * H * (2.0 * p.ne) + 4.0 * 4.0 * 4 * H);
    }
    prof_begin(2, st);
    if (p.ff) {
        // every time step's proposal layer reads the observe embedding of its trace (:72,85): Hs rows = E[trace]
        if (p.fused_obs) {
            RowBuild rb{};
            rb.zero_small = p.in_place ? w.loss_acc : nullptr;
            rb.n_small = n_clear;
            PP_TRY(obs_embed_fwd_fused(net, P, bt->obs, B, w.obs_h, w.cat, w.f1, w.E, st, &rb, nullptr, nullptr, step_env().first_early));
        } else {
            PP_TRY(observe_embedding_fwd(net, P, bt->obs, bt->obs_width, B, w, st, p.bwd, false));
        }
        if (!p.in_place) PP_TRY(embedding_rows(w.E, w.e4, bt->trace, R, net->e_obs, w.Hs, H, w.loss_acc, n_clear, st));
    } else if (p.fused_obs && T <= 2) {   // (long traces: a wave would write all rows of its trace serially - separate gather)
        RowBuild rb{};
        rb.d = GatherDims{net->e_obs, net->smp_dim, net->dtype_dim, net->addr_dim, net->lstm_in};
        rb.params = P; rb.at = net->addr_table; rb.row_off = bt->row_off_dev; rb.t_max = T;
        rb.value = bt->value; rb.addr = bt->addr; rb.prev_row = bt->prev_row;
        rb.X = w.X; rb.ldx = w.i4; rb.xcols = w.xc;
        rb.zero_like = (p.bwd && !p.dx_partials) ? w.dX : nullptr;
        rb.zero_small = w.loss_acc; rb.n_small = n_clear;
        PanelTranspose ptr{};
        if (p.panel) ptr = panel_transpose_job(s);
        // (panel_embed: the panel launch computes the embedding of its rows and writes E, cat, f1, the hidden rows and X)
        PP_TRY(obs_embed_fwd_fused(net, P, bt->obs, B, w.obs_h, w.cat, w.f1, w.E, st, &rb, p.compact ? &abias : nullptr,
                                   p.panel ? &ptr : nullptr, step_env().first_early, p.panel_embed));
    } else {
        PP_TRY(observe_embedding_fwd(net, P, bt->obs, bt->obs_width, B, w, st, p.bwd, p.fused_obs));
        // (also clears the loss slots and, for a backward pass, dX: see the kernel)
        PP_TRY(lstm_input_gather(net, P, w.E, w.e4, bt->trace, bt->value, bt->addr, bt->prev_row, -1, -1, R, w.X, w.i4, st,
                                 p.bwd ? w.dX : nullptr, w.loss_acc, n_clear, w.xc, p.compact ? &abias : nullptr));
    }
    prof_end(2, gather_bytes, st);
    return 0;
}

// Second launch of the panel step: everything between the LSTM input rows and dX (and, training, the observe-embedding
// backward in its tail)
// (the launch's arguments; also what ic_loss asks panel16_embed_ok about, in front of the first launch)
static void panel_args(const Step& s, PanelArgs& pa, PanelObs& po) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const float* P = s.P;
    const int B = p.B, R = p.R, H = p.H;
    const pp_addr& ad = net->addrs[p.only_addr];
    pa = PanelArgs{};
    pa.B = R; pa.H = H; pa.hid = ad.hid; pa.n_out = ad.n_out; pa.K = ad.n_out / 3; pa.e = net->e_obs;
    pa.ldx = (int)w.i4; pa.lda1 = (int)w.hid4; pa.lddy = (int)w.out4; pa.ldw = p.I;
    pa.X = w.X; pa.Wih = P + net->w_ih; pa.AB = w.AB + (int64_t)p.only_addr * 2 * 4 * H;
    pa.WihT = w.WihT; pa.W1T = w.W1T;
    pa.xz = w.xz; pa.xd = w.xd; pa.epoch = w.epoch;
    pa.W1 = P + ad.w1; pa.b1 = P + ad.b1; pa.W2 = P + ad.w2; pa.b2 = P + ad.b2;
    pa.value = bt->value; pa.prior = bt->prior;
    pa.Hs = w.Hl[0]; pa.G = w.Gl[0]; pa.A1 = w.A1; pa.DY = w.DY; pa.dZ1 = w.dZ1; pa.dX = w.dX;
    pa.gsum = w.gsum + (int64_t)p.only_addr * 2 * 4 * H;
    pa.lp_out = (s.flags & PP_LOSS_KEEP_LP) ? s.lp_out : nullptr;
    pa.loss_acc = w.loss_acc; pa.flag = w.flag; pa.grad_scale = -1.0f / (float)B;
    pa.dbg = g_timeline;
    po = PanelObs{};
    if (p.obs_tail) {
        po.a = p.obs_args;
        po.P = P; po.cat = w.cat; po.f1 = w.f1;
        po.dE = w.dE; po.dF1 = w.dF1; po.dCat = w.dCat; po.dHo0 = w.dObsH;
        po.dh_stride = (int64_t)B * w.maxohid4;
        po.embed = p.panel_embed ? 1 : 0; po.xcols = w.xc;
        po.obs = bt->obs; po.E = w.E; po.Xw = w.X; po.cat_w = w.cat; po.f1_w = w.f1;
    }
}

static int panel_launch(const Step& s) {
    const pp_net* net = s.net; const Workspace& w = s.w; const StepPlan& p = s.p;
    hipStream_t st = s.st;
    const int R = p.R, H = p.H;
    const pp_addr& ad = net->addrs[p.only_addr];
    PanelArgs pa;
    PanelObs po;
    panel_args(s, pa, po);
    prof_begin(0, st);
    if (p.panel16_go) {
        Panel16Args p16{};
        p16.a = pa;
        for (int i = 0; i < 6; ++i) p16.img[i] = w.p16.img[i];
        PP_TRY(panel16(ad.kind, p16, st, p.obs_tail ? &po : nullptr));
    } else {
        PP_TRY(panel_t1(ad.kind, pa, st, p.obs_tail ? &po : nullptr));
    }
    // executed data-path FLOPs of the launch: forward + backward products of the 8-row panels
    prof_end(0, 2.0 * R * (2.0 * 3.0 * H * net->e_obs + 2.0 * (double)H * ad.hid + 2.0 * (double)ad.hid * ad.n_out), st);
    return 0;
}

// Input product of layer 0 over compact rows: G = [E | s_prev] W_ih[:, :c2]^T + cur[addr] + prev[previous addr] (gather.hpp);
// first-step rows have no previous statement: their sample-embedding columns are zero too. *cell_done: the first time
// step's cell ran in the product's epilogue
static int lstm_input_compact(const Step& s, bool* cell_done) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const int B = p.B, R = p.R, T = p.T, H = p.H;
    pp_gemm_args g{};
    g.A = w.X; g.lda = w.i4;
    g.B = s.P + net->w_ih; g.ldb = p.I;
    g.C = w.Gl[0]; g.ldc = 4 * H;
    g.M = R; g.N = 4 * H; g.K = p.nx;
    GemmExt x{};
    x.rb = w.AB; x.rb_addr = bt->addr; x.rb_prev = T > 1 ? bt->prev_row : nullptr;
    if (T == 1 && p.n_present == 1) {   // one address in a single-statement batch: the bias is one vector
        x.rb = w.AB + (int64_t)p.only_addr * 2 * 4 * H;
        x.rb_addr = nullptr;
    }
    if (step_env().fuse_cell) {   // gate-interleaved tiles, LSTM cell of the first time step in the epilogue
        x.cell_H = H; x.cell_rows = B; x.cell_c = w.Cl[0]; x.cell_h = w.Hl[0];
        x.lean = p.lean_cell ? 1 : 0;
        *cell_done = true;
    }
    GemmHole zc{};
    zc.b[0] = GemmBlock{0, B, 0, 4 * H, net->e_obs, p.nx};
    if (lstm_input_fast_ok(g, x)) PP_TRY(lstm_input_fast(g, x, s.st));      // (lstm_input.hip; the zero block is zeros in X)
    else PP_TRY(gemm_f32(&g, s.st, &zc, &x));
    prof_end(0, 2.0 * R * (double)p.nx * 4.0 * H, s.st);
    return 0;
}

// the time steps of layer l behind its input product: G_t += h_{t-1} W_hh^T, then the cell
static int lstm_recurrence(const Step& s, int l, bool cell_done) {
    const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const int T = p.T, H = p.H;
    const float* Whh = s.P + lstm_layer(s.net, l).w_hh;
    const bool fuse_rec = step_env().fuse_cell_rec && !p.ff && !p.det;   // (float4 stores, and no fixed order is at stake)
    for (int t = 0; t < T; ++t) {
        if (p.tail_teams && t == p.tail_t0)   // all remaining time steps of this layer: one launch (lstm_tail.hip)
            return lstm_tail_fwd(w.Gl[l], w.Cl[l], w.Hl[l], Whh, bt->row_off_dev, p.tail_t0, T, H, p.tail_teams, w.xch_f, w.xch_b,
                                 w.flag, s.st);
        const int n = bt->n_active[t], r0 = bt->row_off[t];
        float* Gt = w.Gl[l] + (int64_t)r0 * 4 * H;
        const float* c_prev = nullptr;
        if (t > 0) {
            const int rp = bt->row_off[t - 1];
            pp_gemm_args g{};
            g.A = w.Hl[l] + (int64_t)rp * H; g.lda = H;
            g.B = Whh; g.ldb = H;
            g.C = Gt; g.ldc = 4 * H;
            g.M = n; g.N = 4 * H; g.K = H;
            c_prev = w.Cl[l] + (int64_t)rp * H;
            // Recurrent product with the cell in its epilogue (gate-interleaved tiles; one workgroup per tile walks all of
            // K = H, the pre-activations are read instead of accumulated into): no lstm_cell_fwd launch, no round trip of
            // G. Needs enough tiles to fill the chip without a K split: n >= 64 rows x 4H / 64 column tiles.
            if (fuse_rec && H % 16 == 0 && n >= 64) {
                GemmExt x{};
                x.cell_H = H; x.cell_rows = n; x.cell_c = w.Cl[l] + (int64_t)r0 * H; x.cell_h = w.Hl[l] + (int64_t)r0 * H;
                x.cell_cprev = c_prev;
                PP_TRY(gemm_f32(&g, s.st, nullptr, &x));
                continue;
            }
            g.accumulate = 1;
            g.split_k = 1;   // few rows late in a ragged batch: spread K over workgroups (accumulation into G)
            PP_TRY(gemm_f32(&g, s.st));
        }
        if (t == 0 && cell_done) continue;
        PP_TRY(lstm_cell_fwd(Gt, c_prev, w.Cl[l] + (int64_t)r0 * H, w.Hl[l] + (int64_t)r0 * H, n, H, s.st));
    }
    return 0;
}

static int lstm_forward(const Step& s) {
    const pp_net* net = s.net; const Workspace& w = s.w; const StepPlan& p = s.p;
    const int B = p.B, R = p.R, H = p.H;
    for (int l = 0; l < p.L; ++l) {
        bool cell_done = false;
        if (l == 0) prof_begin(0, s.st);
        if (l == 0 && p.compact) {
            PP_TRY(lstm_input_compact(s, &cell_done));
        } else {
            const LstmLayer ly = lstm_layer(net, l);
            const float* in = l == 0 ? w.X : w.Hl[l - 1];
            const int64_t in_ld = l == 0 ? w.i4 : H;
            const int in_w = l == 0 ? p.I : H;
            // a trace's first time step has no previous variable: columns [e_obs, c4) of its LSTM input row are zero
            // (inference_network_lstm.py:159-162) - rows [0, B) of the step-major layout, layer 0 -
            // ... and no previous cell state in any layer: its forget gate multiplies c_{-1} = 0, so columns [H, 2H) of its
            // pre-activations are never looked at (lstm_cell_fwd/bwd with c_prev == NULL) - not computed at all
            GemmHole zero{};
            zero.b[1] = GemmBlock{0, B, H, 2 * H, 0, in_w};
            if (l == 0) zero.b[0] = GemmBlock{0, B, 0, 4 * H, p.c1, p.c4};
            PP_TRY(linear_fwd(in, in_ld, nullptr, s.P + ly.w_ih, s.P + ly.b_ih, w.Gl[l], 4 * H, R, in_w, 4 * H, false, s.P + ly.b_hh,
                              s.st, &zero));
            if (l == 0) prof_end(0, 2.0 * R * (double)p.I * 4.0 * H, s.st);
        }
        PP_TRY(lstm_recurrence(s, l, cell_done));
    }
    return 0;
}

// bias gradients of one address group's proposal layers (rows [h0, h0 + m) of the group-compact buffers) by the
// low-contention column-sum jobs
static void queue_head_bias_sums(const Step& s, GradQueue& q, const pp_addr& ad, int h0, int m) {
    const Workspace& w = s.w;
    q.cs.push_back(ColsumJob{w.DY + (int64_t)h0 * w.out4, w.out4, nullptr, m, ad.n_out, s.grads + ad.b2, nullptr});
    q.cs.push_back(ColsumJob{w.dZ1 + (int64_t)h0 * w.hid4, w.hid4, nullptr, m, ad.hid, s.grads + ad.b1, nullptr});
}

// Heads: first FF layer of EVERY address group in one grouped launch (rows gathered by address: the dispatch gather),
// then the fused tails, grouped by (kind, shape)
static int heads_forward(const Step& s, GradQueue& q) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const float* P = s.P; hipStream_t st = s.st;
    const int H = p.H;
    const float gscale = -1.0f / (float)p.B;
    {
        std::vector<pp_gemm_args> hq;
        for (int a = 0; a < net->n_addr; ++a) {
            const int g0 = bt->grp_off[a], n = bt->grp_off[a + 1] - g0;
            if (n <= 0) continue;
            const pp_addr& ad = net->addrs[a];
            pp_gemm_args g{};
            g.A = p.heads_in; g.lda = p.heads_ld; g.a_idx = bt->grp_rows + g0;
            g.B = P + ad.w1; g.ldb = H;
            g.C = w.A1 + (int64_t)g0 * w.hid4; g.ldc = w.hid4;
            g.M = n; g.N = ad.hid; g.K = H;
            g.bias = P + ad.b1; g.relu = 1;
            hq.push_back(g);
        }
        PP_TRY(gemm_f32_grouped(hq.data(), (int)hq.size(), st));
    }
    std::vector<char> done(net->n_addr, 0);
    for (int a = 0; a < net->n_addr; ++a) {
        const int g0 = bt->grp_off[a], n = bt->grp_off[a + 1] - g0;
        if (n <= 0 || done[a]) continue;
        const pp_addr& ad = net->addrs[a];
        if (head_tail_supported(ad.kind, ad.hid, ad.n_out)) {
            // fused tail (layer 2 + log_prob + loss [+ dy, dz1]) for this and every later group of the same head shape
            std::vector<TailJob> tj;
            for (int b = a; b < net->n_addr; ++b) {
                const pp_addr& bd = net->addrs[b];
                const int h0 = bt->grp_off[b], m = bt->grp_off[b + 1] - h0;
                if (m <= 0 || done[b] || bd.kind != ad.kind || bd.hid != ad.hid || bd.n_out != ad.n_out) continue;
                done[b] = 1;
                tj.push_back(TailJob{w.A1 + (int64_t)h0 * w.hid4, P + bd.w2, P + bd.b2, bt->grp_rows + h0,
                                     p.bwd ? w.DY + (int64_t)h0 * w.out4 : nullptr, w.dZ1 + (int64_t)h0 * w.hid4, m});
                if (p.bwd) queue_head_bias_sums(s, q, bd, h0, m);
            }
            PP_TRY(head_tail_multi(ad.kind, tj.data(), (int)tj.size(), w.hid4, ad.hid, ad.n_out, bt->value, bt->prior, gscale,
                                   p.lp_rows, w.out4, w.hid4, p.loss_slots, w.flag, st));
            continue;
        }
        done[a] = 1;
        float* A1 = w.A1 + (int64_t)g0 * w.hid4;
        float* Y = w.Y + (int64_t)g0 * w.out4;
        PP_TRY(linear_fwd(A1, w.hid4, nullptr, P + ad.w2, P + ad.b2, Y, w.out4, n, ad.hid, ad.n_out, false, nullptr, st));
        PP_TRY(head_logprob(ad.kind, Y, w.out4, bt->grp_rows + g0, bt->value, bt->prior, n, ad.n_out, gscale, p.lp_rows,
                            p.bwd ? w.DY + (int64_t)g0 * w.out4 : nullptr, p.loss_slots, w.flag, st));
    }
    return 0;
}

// weight gradients of address a's two proposal layers
static void queue_head_wgrads(const Step& s, GradQueue& q, int a) {
    const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const pp_addr& ad = s.net->addrs[a];
    const int g0 = bt->grp_off[a], n = bt->grp_off[a + 1] - g0;
    queue_wgrad(q.wq, w.DY + (int64_t)g0 * w.out4, w.out4, w.A1 + (int64_t)g0 * w.hid4, w.hid4, nullptr, s.grads + ad.w2, n, ad.hid,
                ad.n_out);
    // (panel kernel: one group that covers all rows in order - no gather, the product can take the streaming kernel)
    queue_wgrad(q.wq, w.dZ1 + (int64_t)g0 * w.hid4, w.hid4, p.heads_in, p.heads_ld, p.panel ? nullptr : bt->grp_rows + g0,
                s.grads + ad.w1, n, p.H, ad.hid);
}

// Heads backward: what the fused tails left undone, then dH = dZ1 W1 of every address group in one grouped launch
static int heads_backward(const Step& s, GradQueue& q) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const float* P = s.P; float* grads = s.grads; hipStream_t st = s.st;
    const int H = p.H;
    std::vector<pp_gemm_args> dq;   // per-address data gradients into dH
    for (int a = 0; a < net->n_addr; ++a) {
        const int g0 = bt->grp_off[a], n = bt->grp_off[a + 1] - g0;
        if (n <= 0) continue;
        const pp_addr& ad = net->addrs[a];
        const float* A1 = w.A1 + (int64_t)g0 * w.hid4;
        const float* DY = w.DY + (int64_t)g0 * w.out4;
        float* dZ1 = w.dZ1 + (int64_t)g0 * w.hid4;
        queue_head_wgrads(s, q, a);
        if (!head_tail_supported(ad.kind, ad.hid, ad.n_out)) {   // (else dz1 was produced by the forward tail)
            grads_touch(grads + ad.b2);
            grads_touch(grads + ad.b1);
            PP_TRY(colsum_f32(DY, w.out4, nullptr, n, ad.n_out, grads + ad.b2, nullptr, st));
            PP_TRY(linear_dgrad(DY, w.out4, P + ad.w2, dZ1, w.hid4, nullptr, A1, w.hid4, n, ad.hid, ad.n_out, false, st,
                                p.det ? nullptr : grads + ad.b1));   // db1 = colsum(dZ1) fused into the epilogue
            if (p.det) q.cs.push_back(ColsumJob{dZ1, w.hid4, nullptr, n, ad.hid, grads + ad.b1, nullptr});
        }
        pp_gemm_args g{};   // dH[rows of this address] = dZ1 W1
        g.A = dZ1; g.lda = w.hid4;
        g.B = P + ad.w1; g.ldb = H; g.b_kmajor = 1;
        g.C = w.dH; g.ldc = H; g.c_idx = bt->grp_rows + g0;
        g.M = n; g.N = H; g.K = ad.hid;
        if (p.fused_bwd) g.colsum = w.gsum + (int64_t)a * 2 * 4 * H;   // group sums of dG (current-address slot)
        dq.push_back(g);
    }
    if (p.fused_bwd) {   // ... with the cell backward in its epilogue
        GemmExt x{};
        x.bw_G = w.Gl[0]; x.bw_C = w.Cl[0]; x.bw_H = H; x.lean = p.lean_cell ? 1 : 0;
        return gemm_f32_grouped(dq.data(), (int)dq.size(), st, nullptr, &x);
    }
    return gemm_f32_grouped(dq.data(), (int)dq.size(), st);
}

// Parameter gradients of LSTM layer l (leaves, grouped with every head's weight gradients). First-time-step rows give
// nothing to the forget-gate rows (dG[:, H:2H] = 0 where c_{t-1} = 0) and, in layer 0, nothing to the previous-variable
// columns of dW_ih (their inputs are zero there)
static void queue_lstm_wgrads(const Step& s, GradQueue& q, int l) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const int B = p.B, R = p.R, H = p.H;
    const LstmLayer ly = lstm_layer(net, l);
    GemmHole wh{};
    if (l == 0 && p.compact) {   // dW_ih[:, :c2] = dG^T [E | s_prev]; the table columns follow from the group sums (aux jobs)
        wh.b[1] = GemmBlock{H, 2 * H, 0, p.nx, 0, B};
        wh.b[0] = GemmBlock{0, 4 * H, p.c1, p.nx, 0, B};
        queue_wgrad(q.wq, w.Gl[0], 4 * H, w.X, w.i4, nullptr, s.grads + net->w_ih, R, p.nx, 4 * H, &q.holes, wh);
        q.wq.back().ldc = p.I;
    } else {
        const float* in = l == 0 ? w.X : w.Hl[l - 1];
        const int64_t in_ld = l == 0 ? w.i4 : H;
        const int in_w = l == 0 ? p.I : H;
        wh.b[1] = GemmBlock{H, 2 * H, 0, in_w, 0, B};
        if (l == 0) wh.b[0] = GemmBlock{0, 4 * H, p.c1, p.c4, 0, B};
        queue_wgrad(q.wq, w.Gl[l], 4 * H, in, in_ld, nullptr, s.grads + ly.w_ih, R, in_w, 4 * H, &q.holes, wh);
    }
    if (p.T > 1) {
        const int r1 = bt->row_off[1];
        queue_wgrad(q.wq, w.Gl[l] + (int64_t)r1 * 4 * H, 4 * H, w.Hl[l], H, bt->prev_row + r1, s.grads + ly.w_hh, R - r1, H, 4 * H);
    }
}

// the time steps of layer l, last to first: cell backward (bias gradients fused), dh_{t-1} += dG_t W_hh
static int lstm_backward_steps(const Step& s, int l, float* dH_cur) {
    const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const int B = p.B, T = p.T, H = p.H;
    const LstmLayer ly = lstm_layer(s.net, l);
    const float* Whh = s.P + ly.w_hh;
    float* db_ih = p.det ? nullptr : s.grads + ly.b_ih;
    float* db_hh = p.det ? nullptr : s.grads + ly.b_hh;
    if (db_ih) grads_touch(db_ih);
    if (db_hh) grads_touch(db_hh);
    // the top layer's first cell launch folds the loss slots (the tail launch when there is one)
    LossFinalize fin = p.fin;
    if (l != p.L - 1) fin.acc = nullptr;
    int dh_parts = 0;   // K splits of dG_{t+1} W_hh waiting in w.dHp for the cell backward of step t
    for (int t = T - 1; t >= 0; --t) {
        if (p.tail_teams && t >= p.tail_t0) {   // steps T-1 .. tail_t0 in one launch; it leaves dh / dc of step tail_t0 - 1
            PP_TRY(lstm_tail_bwd(w.Gl[l], w.Cl[l], dH_cur, w.dC, Whh, bt->row_off_dev, p.tail_t0, T, H, p.tail_teams, w.xch_f,
                                 w.xch_b, w.flag, db_ih, db_hh, fin, s.st));
            t = p.tail_t0;
            continue;
        }
        const int n = bt->n_active[t], r0 = bt->row_off[t];
        const int n_next = (t + 1 < T) ? bt->n_active[t + 1] : 0;
        float* Gt = w.Gl[l] + (int64_t)r0 * 4 * H;
        const float* c_prev = t > 0 ? w.Cl[l] + (int64_t)bt->row_off[t - 1] * H : nullptr;
        PP_TRY(lstm_cell_bwd(Gt, c_prev, w.Cl[l] + (int64_t)r0 * H, dH_cur + (int64_t)r0 * H, w.dC, n, n_next, H, db_ih, db_hh, s.st,
                             t == T - 1 ? fin.acc : nullptr, w.flag, B, fin.loss_out, fin.status_out, w.dHp, dh_parts,
                             (int64_t)B * H));   // + the stored partials of dG_{t+1} W_hh
        dh_parts = 0;
        if (t == 0) break;
        // dh_{t-1} += dG_t W_hh as K-split partial tiles that the NEXT cell-backward launch adds (rows [0, n) of step t - 1
        // are the same traces): no float atomics (6 us per 64 x 64 tile), no read-modify-write of dH
        const int tiles = cdiv(n, 64) * cdiv(H, 64), nslab = 4 * H / 32;
        const int splits = std::max(1, std::min({DH_SPLITS, cdiv(256, tiles), nslab / 2}));
        if (step_env().dh_partials && !p.det && splits > 1 && H % 4 == 0) {
            pp_gemm_args g{};
            g.A = Gt; g.lda = 4 * H;
            g.B = Whh; g.ldb = H; g.b_kmajor = 1;
            g.C = w.dHp; g.ldc = H;
            g.M = n; g.N = H; g.K = 4 * H;
            GemmExt x{};
            x.split_stride = (int64_t)B * H;
            x.force_splits = splits;
            PP_TRY(gemm_f32(&g, s.st, nullptr, &x));
            dh_parts = splits;
        } else {
            PP_TRY(linear_dgrad(Gt, 4 * H, Whh, dH_cur + (int64_t)bt->row_off[t - 1] * H, H, nullptr, nullptr, 0, n, H, 4 * H, true,
                                s.st));
        }
    }
    return 0;
}

static int lstm_backward(const Step& s, GradQueue& q) {
    const Workspace& w = s.w; const StepPlan& p = s.p;
    const int B = p.B, R = p.R, H = p.H;
    float* dH_cur = w.dH;          // gradient into the hidden states of the layer being processed (top: from the heads)
    float* dH_other = w.dH2;
    for (int l = p.L - 1; l >= 0; --l) {
        const LstmLayer ly = lstm_layer(s.net, l);
        if (!p.fused_bwd) PP_TRY(lstm_backward_steps(s, l, dH_cur));   // (else dG is already in place)
        if (p.det)   // bias gradients = column sums of the complete dG of this layer, by the single-writer kernel
            q.cs.push_back(ColsumJob{w.Gl[l], 4 * H, nullptr, R, 4 * H, s.grads + ly.b_ih, s.grads + ly.b_hh});
        queue_lstm_wgrads(s, q, l);
        if (l > 0) {   // gradient into the hidden states of the layer below: dH_{l-1} = dG_l W_ih_l (the forget-gate part of
            GemmHole dh{};                                         // the sum is zero for first-time-step rows)
            dh.b[0] = GemmBlock{0, B, 0, H, H, 2 * H};
            PP_TRY(linear_dgrad(w.Gl[l], 4 * H, s.P + ly.w_ih, dH_other, H, nullptr, nullptr, 0, R, H, 4 * H, false, s.st, nullptr,
                                &dh));
            std::swap(dH_cur, dH_other);
        }
    }
    return 0;
}

// Layer 0's data gradient dX = dG W_ih, then scatter into the embedding tables / sample embeddings (the observe embedding
// follows). Nobody reads the previous-variable columns of first-time-step rows (no previous variable, no parameter behind
// them). The forget-gate part of the summation over the gates is zero for those rows.
static int input_backward(const Step& s, GradQueue& q) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const float* P = s.P; float* grads = s.grads; hipStream_t st = s.st;
    const int B = p.B, R = p.R, T = p.T, H = p.H;
    if (p.compact) {
        // dX[:, :c2] = dG W_ih[:, :c2] (observe-embedding and sample-embedding columns; the table columns need no per-row
        // gradient: their parameter gradients follow from the column sums of dG per address group)
        const GemmHole dx_unused{{{0, B, p.c1, p.nx, 0, 4 * H}, {0, B, 0, p.nx, H, 2 * H}}};
        pp_gemm_args g{};
        g.A = w.G; g.lda = 4 * H;
        g.B = P + net->w_ih; g.ldb = p.I; g.b_kmajor = 1;
        g.C = w.dX; g.ldc = w.i4;
        g.M = R; g.N = p.nx; g.K = 4 * H;
        if (p.dx_partials) {
            GemmExt x{};
            x.split_stride = (int64_t)R * w.i4;
            x.force_splits = p.dx_splits;
            PP_TRY(gemm_f32(&g, st, &dx_unused, &x));
        } else {
            g.accumulate = 1;   // dX was cleared by the gather kernel
            g.split_k = 1;
            PP_TRY(gemm_f32(&g, st, &dx_unused));
        }
        if (!p.fused_bwd)   // group sums of dG by current / previous address (the fused dH epilogue produced the former)
            for (int a = 0; a < net->n_addr; ++a) {
                const int g0 = bt->grp_off[a], n = bt->grp_off[a + 1] - g0;
                if (n > 0) q.cs.push_back(ColsumJob{w.G, 4 * H, bt->grp_rows + g0, n, 4 * H, w.gsum + (int64_t)a * 2 * 4 * H, nullptr});
                const int q0 = bt->nxt_off[a], m = bt->nxt_off[a + 1] - q0;
                if (m > 0)
                    q.cs.push_back(ColsumJob{w.G, 4 * H, bt->nxt_rows + q0, m, 4 * H, w.gsum + ((int64_t)a * 2 + 1) * 4 * H, nullptr});
            }
    } else {
        const GemmHole dx_unused{{{0, B, p.c1, p.c4, 0, 4 * H}, {0, B, 0, p.I, H, 2 * H}}};
        PP_TRY(linear_dgrad(w.G, 4 * H, P + net->w_ih, w.dX, w.i4, nullptr, nullptr, 0, R, p.I, 4 * H, true, st, nullptr,
                            &dx_unused));   // dX was cleared by the gather kernel
        for (int a = 0; a < net->n_addr; ++a) {   // table columns of dX -> the embedding vectors
            const pp_addr& ad = net->addrs[a];
            const int g0 = bt->grp_off[a], n = bt->grp_off[a + 1] - g0;
            if (n > 0) {  // rows where `a` is the current address
                q.cs.push_back(ColsumJob{w.dX + p.c4, w.i4, bt->grp_rows + g0, n, net->dtype_dim, grads + ad.dtype_emb, nullptr});
                q.cs.push_back(ColsumJob{w.dX + p.c5, w.i4, bt->grp_rows + g0, n, net->addr_dim, grads + ad.addr_emb, nullptr});
            }
            const int q0 = bt->nxt_off[a], m = bt->nxt_off[a + 1] - q0;
            if (m > 0) {  // rows whose previous variable has address `a`
                q.cs.push_back(ColsumJob{w.dX + p.c2, w.i4, bt->nxt_rows + q0, m, net->dtype_dim, grads + ad.dtype_emb, nullptr});
                q.cs.push_back(ColsumJob{w.dX + p.c3, w.i4, bt->nxt_rows + q0, m, net->addr_dim, grads + ad.addr_emb, nullptr});
            }
        }
    }
    if (T > 1) grads_touch_all(grads);   // (the sample-embedding scatter writes the layers of every previous address)
    if (T > 1 && p.det)
        PP_TRY(sample_embed_bwd_det(net, P, bt->value, bt->prev_row, bt->nxt_rows, bt->nxt_off, w.dX, w.i4, grads, st));
    else if (T > 1)
        PP_TRY(sample_embed_bwd(net, P, bt->value, bt->addr, bt->prev_row, bt->row_off[1], R, w.dX, w.i4, grads, st));
    return 0;
}

// Launches the queued weight-gradient leaves as one grouped launch, `aux` behind its tiles.
static int flush_wgrads(const Step& s, GradQueue& q, const AuxJobs* aux = nullptr) {
    std::vector<pp_gemm_args>& wq = q.wq;
    std::vector<GemmHole>& wholes = q.holes;
    wholes.resize(wq.size(), GemmHole{});
    // data parallel with an overlap range (dp.hip): the products that complete the range - the LSTM layer's weight
    // gradients - and the reduction jobs go first; the range's all-reduce starts on the side stream behind them and the
    // remaining products (proposal layers, observe embedding) run under it
    int64_t lo = 0, hi = 0;
    if (dp_overlap_hull(&lo, &hi) && wq.size() > 1) {
        std::vector<pp_gemm_args> qa, qb;
        std::vector<GemmHole> ha, hb;
        for (size_t i = 0; i < wq.size(); ++i) {
            const bool in = wq[i].C >= s.grads + lo && wq[i].C < s.grads + hi;
            (in ? qa : qb).push_back(wq[i]);
            (in ? ha : hb).push_back(wholes[i]);
        }
        if (!qa.empty() && !qb.empty()) {
            PP_TRY(launch_wgrads(qa, s.st, &ha, true, aux, true));
            PP_TRY(dp_bucket0_issue(s.grads, s.st));
            PP_TRY(launch_wgrads(qb, s.st, &hb, false, nullptr, true));
            wq.clear();
            wholes.clear();
            return 0;
        }
    }
    PP_TRY(launch_wgrads(wq, s.st, &wholes, true, aux, true));
    wq.clear();
    wholes.clear();
    return 0;
}

// the live column-sum jobs as jobs behind the weight-gradient tiles; false (nothing copied): more than the job table holds
static bool colsums_ride(const std::vector<ColsumJob>& cs, AuxJobs& aux) {
    int n_live = 0;
    for (const auto& j : cs) n_live += (j.n_rows > 0 && j.n_cols > 0) ? 1 : 0;
    if (n_live > AUX_MAX_COLSUM) return false;
    for (const auto& j : cs)
        if (j.n_rows > 0 && j.n_cols > 0) aux.cs[aux.n_colsum++] = j;
    return true;
}

// Column sums + weight-gradient leaves. Compact rows: the jobs that turn the group sums of dG into the table-column
// gradients (and, after the fused cell backward, the LSTM bias gradients and the loss) ride behind the tiles of the
// grouped weight-gradient launch; for a single-statement batch so do the column sums themselves (nothing in the
// launch depends on anything else in it), which removes the separate column-sum launch.
static int reduce_and_flush(const Step& s, GradQueue& q) {
    const pp_net* net = s.net; const StepPlan& p = s.p;
    const bool ride = step_env().aux_colsum;
    AuxJobs aux{};
    // the tensors these leaves write may be non-zero from now on (adam_live.hpp; group sums into the workspace mark nothing)
    for (const auto& g : q.wq) grads_touch(g.C);
    for (const auto& j : q.cs) {
        grads_touch(j.out);
        if (j.out2) grads_touch(j.out2);
    }
    if (p.compact) {   // the jobs derived from the group sums: the table columns of dW_ih, every address's tables, the biases
        grads_touch(s.grads + net->w_ih);
        for (int a = 0; a < net->n_addr; ++a) {
            grads_touch(s.grads + net->addrs[a].addr_emb);
            grads_touch(s.grads + net->addrs[a].dtype_emb);
        }
        if (p.fused_bwd) {
            grads_touch(s.grads + net->b_ih);
            grads_touch(s.grads + net->b_hh);
        }
    }
    if (!p.compact) {
        // FeedForward network: no column sum depends on another launch's group sums, so they all ride behind the
        // weight-gradient tiles (and the loss is finalised there): one launch less per step
        if (p.ff && !p.det && ride && !q.wq.empty() && colsums_ride(q.cs, aux)) {
            aux.fin = p.fin;
            aux_layout(aux, false);
            return flush_wgrads(s, q, &aux);
        }
        if (p.ff)   // (LSTM: the first cell launch of the backward pass finalises the loss)
            PP_TRY(colsum_multi(q.cs.data(), (int)q.cs.size(), s.st, p.fin_acc, s.w.flag, p.B, p.fin.loss_out, p.fin.status_out));
        else
            PP_TRY(colsum_multi(q.cs.data(), (int)q.cs.size(), s.st));
        return flush_wgrads(s, q);
    }
    if (!(p.fused_bwd && ride && colsums_ride(q.cs, aux))) PP_TRY(colsum_multi(q.cs.data(), (int)q.cs.size(), s.st));
    aux_derived(s, aux);
    if (p.fused_bwd) {
        aux.db_ih = s.grads + net->b_ih; aux.db_hh = s.grads + net->b_hh;
        aux.fin = p.fin;
    }
    aux_layout(aux, true);
    return flush_wgrads(s, q, &aux);
}

// the gradient of the observe embedding is summed over the time steps from dX[:, :e_obs] (LSTM) / from dH (FF)
static const float* obs_grad_rows(const Step& s, int64_t* ld) {
    *ld = s.p.ff ? s.p.H : s.w.i4;
    return s.p.ff ? s.w.dH : s.w.dX;
}

// Fused observe-embedding backward: dE (sum over the trace's time steps of dX, masked by the last ReLU) and the data
// gradients of the whole stack in one launch ...
static int obs_dgrad_fused(const Step& s) {
    const Workspace& w = s.w; const StepPlan& p = s.p;
    int64_t ldxs;
    const float* dXs = obs_grad_rows(s, &ldxs);
    return obs_embed_dgrad_fused(s.net, s.P, p.B, w.obs_h, w.cat, w.f1, dXs, ldxs, s.bt->row_off_dev, p.T, w.E, w.dE, w.dF1, w.dCat,
                                 w.dObsH, (int64_t)p.B * w.maxohid4, s.st, p.dx_splits, (int64_t)p.R * w.i4);
}
// ... its weight gradients join the grouped MFMA launch; bias gradients are column sums of the same buffers
static void queue_obs_grads_fused(const Step& s, GradQueue& q) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w;
    float* grads = s.grads;
    const int B = s.p.B, e = net->e_obs;
    const int64_t dhs = (int64_t)B * w.maxohid4;
    queue_wgrad(q.wq, w.dE, w.e4, w.f1, w.e4, nullptr, grads + net->fin_w1, B, e, e);
    queue_wgrad(q.wq, w.dF1, w.e4, w.cat, w.e4, nullptr, grads + net->fin_w0, B, e, e);
    q.cs.push_back(ColsumJob{w.dE, w.e4, nullptr, B, e, grads + net->fin_b1, nullptr});
    q.cs.push_back(ColsumJob{w.dF1, w.e4, nullptr, B, e, grads + net->fin_b0, nullptr});
    int ci = 0, co = 0;
    for (int o = 0; o < net->n_obs; ++o) {
        const int in = net->obs_in[o], hid = net->obs_hid[o], out = net->obs_out[o];
        float* dHo = w.dObsH + (int64_t)o * dhs;
        queue_wgrad(q.wq, w.dCat + co, w.e4, w.obs_h[o], w.ohid4[o], nullptr, grads + net->obs_w1[o], B, hid, out);
        // dW0[:, k] = sum_b dh[b, :] obs[b, k]: a handful of input columns -> weighted column sums, not a GEMM
        for (int k = 0; k < in; ++k)
            q.cs.push_back(ColsumJob{dHo, w.ohid4[o], nullptr, B, hid, grads + net->obs_w0[o] + k, nullptr, bt->obs + ci + k,
                                     bt->obs_width, in});
        q.cs.push_back(ColsumJob{w.dCat + co, w.e4, nullptr, B, out, grads + net->obs_b1[o], nullptr});
        q.cs.push_back(ColsumJob{dHo, w.ohid4[o], nullptr, B, hid, grads + net->obs_b0[o], nullptr});
        ci += in;
        co += out;
    }
}

// Generic observe-embedding backward (any depth, CNN2D5C): behind the step's grouped launch, layer by layer
static int obs_backward_generic(const Step& s, GradQueue& q) {
    const pp_net* net = s.net; const pp_batch* bt = s.bt; const Workspace& w = s.w; const StepPlan& p = s.p;
    const float* P = s.P; float* grads = s.grads; hipStream_t st = s.st;
    const int B = p.B, e = net->e_obs;
    int64_t ldxs;
    const float* dXs = obs_grad_rows(s, &ldxs);
    grads_touch_all(grads);   // (layer by layer below, the convolution stack included: no leaf list to mark from)
    PP_TRY(obs_grad(dXs, ldxs, bt->row_off_dev, p.T, B, e, w.E, w.e4, w.dE, w.e4, st));   // dE, ReLU mask applied
    PP_TRY(reduce_and_flush(s, q));
    PP_TRY(linear_wgrad(w.dE, w.e4, w.f1, w.e4, nullptr, grads + net->fin_w1, grads + net->fin_b1, nullptr, B, e, e, st));
    PP_TRY(linear_dgrad(w.dE, w.e4, P + net->fin_w1, w.dF1, w.e4, nullptr, w.f1, w.e4, B, e, e, false, st,
                        p.det ? nullptr : grads + net->fin_b0));
    if (p.det) PP_TRY(colsum_f32(w.dF1, w.e4, nullptr, B, e, grads + net->fin_b0, nullptr, st));
    PP_TRY(linear_wgrad(w.dF1, w.e4, w.cat, w.e4, nullptr, grads + net->fin_w0, nullptr, nullptr, B, e, e, st));
    PP_TRY(linear_dgrad(w.dF1, w.e4, P + net->fin_w0, w.dCat, w.e4, nullptr, w.cat, w.e4, B, e, e, false, st));
    int ci = 0, co = 0;
    for (int o = 0; o < net->n_obs; ++o) {
        // backward through EmbeddingFeedForward(num_layers = depth): dz of layer l (ReLU mask already applied) gives
        // dW_l = dz^T x_l, db_l = colsum dz, and dz of layer l - 1 = (dz W_l) * [x_l > 0]
        const bool cnn = net->obs_kind[o] == PP_OBS_CNN2D5C;      // layer 0 (_lin1) reads the convolution stack's features
        const float* dz = w.dCat + co;
        int64_t lddz = w.e4;
        float* scratch[2] = {w.dObsH, w.dObsH2};
        for (int l = obs_layers(net, o) - 1; l >= 0; --l) {
            const ObsLin ly = obs_lin(net, o, l);
            const float* x = l == 0 ? (cnn ? w.cnn_feat[o] : bt->obs + ci) : w.obs_hl[o][l - 1];
            const int64_t ldx = l == 0 ? (cnn ? w.f4[o] : bt->obs_width) : w.ohid4[o];
            PP_TRY(linear_wgrad(dz, lddz, x, ldx, nullptr, grads + ly.w, grads + ly.b, nullptr, B, ly.in, ly.out, st));
            if (l > 0) {
                float* dprev = scratch[l & 1];
                PP_TRY(linear_dgrad(dz, lddz, P + ly.w, dprev, w.ohid4[o], nullptr, x, ldx, B, ly.in, ly.out, false, st));
                dz = dprev;
                lddz = w.ohid4[o];
            } else if (cnn) {
                // the image is data, its features are not: dFeatures = dz W_lin1 (no mask here: the pool backward applies
                // conv5's), then back through the stack
                PP_TRY(linear_dgrad(dz, lddz, P + ly.w, w.cnn_dfeat[o], w.f4[o], nullptr, nullptr, 0, B, ly.in, ly.out, false, st));
                PP_TRY(cnn_backward(net, o, w.cnn_dfeat[o], w.f4[o], B, grads, w.cnn_ws[o], w.cnn_ws_bytes[o], st));
            }
        }
        ci += net->obs_in[o];
        co += net->obs_out[o];
    }
    return 0;
}

int ic_loss(const pp_net* net, const pp_batch* bt, const float* P, float* grads, void* ws,
            size_t ws_bytes, float* loss_out, int32_t* status_out, float* lp_out, int flags, hipStream_t st) {
    PP_TRY(check_net(net));
    PP_CHECK_ARG(bt && P && ws && loss_out, "pp_ic_loss: null pointer");
    PP_CHECK_ARG(bt->n_traces > 0 && bt->n_rows >= bt->n_traces && bt->t_max >= 1, "pp_ic_loss: empty batch");
    PP_CHECK_ARG(bt->n_active && bt->row_off && bt->grp_off && bt->obs && bt->value && bt->prior && bt->addr &&
                     bt->prev_row && bt->grp_rows && bt->trace && bt->row_off_dev && bt->nxt_off && bt->nxt_rows,
                 "pp_ic_loss: incomplete pp_batch");
    {
        int obs_in = 0;
        for (int o = 0; o < net->n_obs; ++o) obs_in += net->obs_in[o];
        PP_CHECK_ARG(bt->obs_width == obs_in, "pp_ic_loss: batch obs_width %d != the network's observable width %d",
                     bt->obs_width, obs_in);
    }
    const bool bwd = flags & PP_LOSS_BACKWARD;
    PP_CHECK_ARG(!bwd || grads, "pp_ic_loss: PP_LOSS_BACKWARD needs a gradient buffer");
    Workspace w;
    carve(net, bt->n_traces, bt->n_rows, ws, ws_bytes, w);
    if (w.bytes > ws_bytes) {
        set_error("pp_ic_loss: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
        return PP_ENOSPACE;
    }
    if (bwd && (flags & PP_LOSS_ZERO_GRADS)) (void)hipMemsetAsync(grads, 0, (size_t)net->n_params * sizeof(float), st);
    StepPlan p = plan_step(net, bt, flags, lp_out, loss_out, status_out, w);
    const Step s{net, bt, P, grads, w, p, st, lp_out, flags};
    if (p.panel16_go && p.obs_tail && p.T == 1 && p.compact) {      // (both launches read the answer from the plan)
        PanelArgs pa;
        PanelObs po;
        panel_args(s, pa, po);
        p.panel_embed = bt->obs_width == p.obs_args.width && panel16_embed_ok(pa, po);
    }
    GradQueue q;
    PP_TRY(first_launch(s));
    if (p.panel) {
        // The headline step, four launches with Adam: the first one also wrote the panel kernel's weight images; the panel
        // launch left dG, the group sums, dz1, dy and dX (and, with obs_tail, the embedding's data gradients) - what
        // remains is to queue the leaves in the general path's order and to launch them.
        // (panel implies lean_cell, which implies bwd, compact rows, T == 1 and one LSTM layer: no forward-only call gets here)
        PP_TRY(panel_launch(s));
        const pp_addr& ad = net->addrs[p.only_addr];
        queue_head_bias_sums(s, q, ad, 0, p.R);
        queue_head_wgrads(s, q, p.only_addr);
        queue_lstm_wgrads(s, q, 0);
        if (!p.obs_tail) PP_TRY(obs_dgrad_fused(s));
        queue_obs_grads_fused(s, q);
        return reduce_and_flush(s, q);
    }
    PP_TRY(lstm_forward(s));
    PP_TRY(heads_forward(s, q));
    if (p.det) PP_TRY(loss_from_rows(p.lp_rows, p.R, p.B, w.flag, loss_out, status_out, st));
    if (!bwd) {
        if (!p.det) PP_TRY(loss_finalize(w.loss_acc, w.flag, p.B, loss_out, status_out, st));
        return 0;
    }
    // (with a backward pass the loss slots are folded by the first LSTM-cell launch, or behind the weight-gradient tiles)
    PP_TRY(heads_backward(s, q));
    PP_TRY(lstm_backward(s, q));
    if (!p.ff) PP_TRY(input_backward(s, q));
    if (!p.fused_obs) return obs_backward_generic(s, q);
    PP_TRY(obs_dgrad_fused(s));
    queue_obs_grads_fused(s, q);
    return reduce_and_flush(s, q);
}

}  // namespace pp

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
extern "C" {

int pp_abi_version(void) { return PP_ABI_VERSION; }
const char* pp_last_error(void) { return pp::last_error(); }

int pp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

size_t pp_ic_workspace_bytes(const pp_net* net, int32_t n_traces, int32_t n_rows) {
    if (!net || pp::check_net(net) != 0) return 0;
    pp::Workspace w;
    pp::carve(net, n_traces, n_rows, nullptr, 0, w);
    return w.bytes;
}

int pp_ic_loss(const pp_net* net, const pp_batch* batch, const float* params, float* grads, void* workspace,
               size_t workspace_bytes, float* loss_out, int32_t* status_out, float* lp_out, int32_t flags, void* stream) {
    return pp::ic_loss(net, batch, params, grads, workspace, workspace_bytes, loss_out, status_out, lp_out, flags,
                       pp::as_stream(stream));
}

int pp_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n_params,
                 const int32_t* chunk_tensor, const float* active, int32_t* tensor_step, int32_t* arrived, int32_t n_tensors,
                 float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, int32_t flags,
                 const int32_t* skip, void* stream) {
    // kernel class 3 of the in-stream timing: the optimizer pass over the flat buffers (HBM bound): reads of params, grads
    // and both moments, writes of params, both moments and the cleared gradients - 8 x 4 bytes per (padded) parameter
    // (the caller filled `grads` by means this library does not see, and the call moves the moments of whatever is non-zero:
    // for the live-chunk launch of the training paths every tensor of a bound buffer is touched from here on)
    pp::grads_touch_all(grads);
    pp::prof_begin(3, pp::as_stream(stream));
    const int rc = pp::adam_step(params, grads, exp_avg, exp_avg_sq, n_params, chunk_tensor, active, tensor_step, arrived,
                                 n_tensors, lr, beta1, beta2, eps, weight_decay, grad_scale, flags, skip, pp::as_stream(stream));
    pp::prof_end(3, ((flags & PP_ADAM_ZERO_GRADS) ? 32.0 : 28.0) * (double)n_params, pp::as_stream(stream));
    return rc;
}

int pp_adam_step_live(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n_params,
                      const int32_t* chunk_tensor, const float* active, int32_t* tensor_step, int32_t* arrived, int32_t n_tensors,
                      float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, int32_t flags,
                      const int32_t* skip, void* stream) {
    pp::prof_begin(3, pp::as_stream(stream));
    const int rc = pp::adam_step_live(params, grads, exp_avg, exp_avg_sq, n_params, chunk_tensor, active, tensor_step, arrived,
                                      n_tensors, lr, beta1, beta2, eps, weight_decay, grad_scale, flags, skip,
                                      pp::as_stream(stream));
    pp::prof_end(3, ((flags & PP_ADAM_ZERO_GRADS) ? 32.0 : 28.0) * (double)n_params, pp::as_stream(stream));
    return rc;
}

int pp_adam_live_bind(const float* grads, const float* exp_avg, const float* exp_avg_sq, int64_t n_params,
                      const int32_t* tensor_first, int32_t n_tensors, int32_t clean) {
    return pp::adam_live_bind(grads, exp_avg, exp_avg_sq, n_params, tensor_first, n_tensors, clean != 0);
}

int pp_adam_live_unbind(const float* grads) {
    pp::adam_live_unbind(grads);
    return 0;
}

int pp_adam_live_mark_touched(const void* buffer) {
    pp::grads_touch_all(buffer);
    return 0;
}

int pp_adam_live_mark_range(const float* grads, int64_t offset, int64_t count) {
    pp::grads_touch_range(grads, offset, count);
    return 0;
}

int pp_adam_live_info(const float* grads, int64_t* out, uint8_t* touched_out) {
    if (!out) return PP_EINVAL;
    return pp::adam_live_info(grads, out, touched_out);
}

static void adam_table_words(const pp::AdamLiveTable& tab, int32_t* out) {
    int k = 0;
    out[k++] = tab.n_runs; out[k++] = tab.live_blocks; out[k++] = tab.n_gaps;
    for (int r = 0; r < pp::ADAM_LIVE_MAX_RUNS; ++r) { out[k++] = tab.run_blk[r]; out[k++] = tab.run_chunk[r]; }
    for (int g = 0; g <= pp::ADAM_LIVE_MAX_RUNS; ++g) { out[k++] = tab.gap_t0[g]; out[k++] = tab.gap_t1[g]; }
}

int pp_adam_live_plan(const int32_t* tensor_first, int32_t n_tensors, const uint8_t* live, int32_t* out) {
    if (!(tensor_first && live && out) || n_tensors <= 0) return PP_EINVAL;
    pp::AdamLiveTable tab;
    if (!pp::adam_live_plan(tensor_first, n_tensors, live, tab)) return 1;
    adam_table_words(tab, out);
    return 0;
}

int pp_adam_live_table(const float* grads, const float* exp_avg, const float* exp_avg_sq, int64_t n_params, int32_t n_tensors,
                       float weight_decay, int32_t* out) {
    if (!out) return PP_EINVAL;
    pp::AdamLiveTable tab;
    if (!pp::adam_live_table(grads, exp_avg, exp_avg_sq, n_params, n_tensors, weight_decay != 0.0f, tab)) return 1;
    adam_table_words(tab, out);
    return 0;
}

int pp_colsum_f32(const float* X, int64_t ldx, const int32_t* row_idx, int32_t n_rows, int32_t n_cols, float* out,
                  float* out2, void* stream) {
    pp::grads_touch_all(out);
    pp::grads_touch_all(out2);
    return pp::colsum_f32(X, ldx, row_idx, n_rows, n_cols, out, out2, pp::as_stream(stream));
}

int pp_lstm_input_gather(const pp_net* net, const float* params, const float* E, const int32_t* trace_of_row,
                         const float* value, const int32_t* addr, const int32_t* prev_row, int32_t n_rows, float* X,
                         int64_t ldx, void* stream) {
    if (!net) return PP_EINVAL;
    return pp::lstm_input_gather(net, params, E, pp::round4(net->e_obs), trace_of_row, value, addr, prev_row, -1, -1, n_rows,
                                 X, ldx, pp::as_stream(stream));
}

int pp_lstm_cell_fwd(float* G, const float* c_prev, float* c, float* h, int32_t n, int32_t H, void* stream) {
    return pp::lstm_cell_fwd(G, c_prev, c, h, n, H, pp::as_stream(stream));
}

int pp_lstm_cell_bwd(float* G, const float* c_prev, const float* c, const float* dh, float* dc_carry, int32_t n,
                     int32_t n_next, int32_t H, void* stream) {
    return pp::lstm_cell_bwd(G, c_prev, c, dh, dc_carry, n, n_next, H, nullptr, nullptr, pp::as_stream(stream));
}

int pp_head_logprob(int32_t kind, const float* y, int64_t ldy, const int32_t* rows, const float* value, const float* prior,
                    int32_t n, int32_t n_out, float grad_scale, float* lp_out, float* dy, float* loss_acc,
                    int32_t* nonfinite, void* stream) {
    return pp::head_logprob(kind, y, ldy, rows, value, prior, n, n_out, grad_scale, lp_out, dy, loss_acc, nonfinite,
                            pp::as_stream(stream));
}

// Shader-clock probe: one wave spins for `iters` dependent FMAs and records s_memtime (shader cycles) and
// s_memrealtime (100 MHz wall clock) before and after. out[0] = shader cycles, out[1] = wall ticks (10 ns).
__global__ void clock_probe_kernel(int iters, long long* out, float* sink) {
    float x = (float)threadIdx.x;
    const long long c0 = clock64();
    const long long w0 = wall_clock64();
    for (int i = 0; i < iters; ++i) x = x * 1.0000001f + 0.5f;
    const long long c1 = clock64();
    const long long w1 = wall_clock64();
    if (threadIdx.x == 0) {
        out[0] = c1 - c0;
        out[1] = w1 - w0;
    }
    if (x == 123.456f) sink[0] = x;
}

int pp_debug_clock_probe(int32_t iters, long long* out /*dev [2]*/, float* sink /*dev [1]*/, void* stream) {
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, pp::as_stream(stream), iters, out, sink);
    PP_LAUNCH_CHECK("pp_debug_clock_probe");
    return 0;
}

int pp_debug_timeline(long long* buf /*dev [16] or NULL*/) {
    pp::g_timeline = buf;
    return 0;
}

int pp_prof_arm(int32_t which, int32_t max_samples) {
    for (auto e : pp::g_prof.ev0) (void)hipEventDestroy(e);
    for (auto e : pp::g_prof.ev1) (void)hipEventDestroy(e);
    pp::g_prof.ev0.clear();
    pp::g_prof.ev1.clear();
    pp::g_prof.flops.clear();
    pp::g_prof.used = 0;
    pp::g_prof.seen = 0;
    pp::g_prof.cur = false;
    pp::g_prof.which = -1;
    if (max_samples <= 0) return 0;
    pp::g_prof.ev0.resize(max_samples);
    pp::g_prof.ev1.resize(max_samples);
    pp::g_prof.flops.assign(max_samples, 0.0);
    for (int i = 0; i < max_samples; ++i) {
        if (hipEventCreate(&pp::g_prof.ev0[i]) != hipSuccess || hipEventCreate(&pp::g_prof.ev1[i]) != hipSuccess) {
            pp::set_error("pp_prof_arm: hipEventCreate failed");
            return PP_ENODEV;
        }
    }
    pp::g_prof.which = which;
    return 0;
}

int pp_prof_stride(int32_t stride) {
    pp::g_prof.stride = stride > 0 ? stride : 1;
    return 0;
}

int pp_prof_collect(float* ms_out, int32_t cap, int32_t* n_out, double* flops_out) {
    int n = std::min<int>(pp::g_prof.used, cap);
    for (int i = 0; i < n; ++i) {
        (void)hipEventSynchronize(pp::g_prof.ev1[i]);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, pp::g_prof.ev0[i], pp::g_prof.ev1[i]);
        ms_out[i] = ms;
        if (flops_out) flops_out[i] = pp::g_prof.flops[i];
    }
    if (n_out) *n_out = n;
    pp::g_prof.used = 0;
    return 0;
}

}  // extern "C"
