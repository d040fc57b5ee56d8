/*
 * pyprob_amd.h -- C ABI of libpyprob_amd.so: the MI355X (gfx950) inference-compilation engine for pyprob.
 *
 * This is the drop-in boundary (SURVEY.md §8b seam B3). pyprob itself is 100% Python and has no FFI for this
 * path, so every entry point below cites the reference *Python* code it replaces (paths relative to the pyprob
 * v1.5.0 tree). The reference-side binding a maintainer would add is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - plain C: pointers, sizes, POD structs; no torch/HIP types. `stream` is a hipStream_t passed as void*.
 *   - every pointer marked "dev" is device (HBM) memory owned by the caller (the host uses the PyTorch-ROCm
 *     caching allocator as plumbing); the library never allocates or frees device memory and never
 *     synchronises the stream unless the function says so.
 *   - all arithmetic is fp32 (reference: util._dtype = torch.float, pyprob/util.py:29). GEMMs use the exact
 *     fp32 MFMA (v_mfma_f32_32x32x2_f32), everything else fp32 VALU.
 *   - return value: 0 on success, a hipError_t (>0) from a failed launch, or a PP_E* code (<0). No C++
 *     exceptions cross this ABI. pp_last_error() returns a static, thread-local description.
 *   - threading: call from one host thread per stream (pyprob's trace runtime is single-threaded,
 *     pyprob/state.py:13-27).
 *
 * Packed trace batch ("step-major ragged"): the B traces of a minibatch are sorted by controlled length,
 * longest first; row r = row_off[t] + b holds time step t of trace b (b < n_active[t]). Sub-batches of the
 * reference (pyprob/nn/dataset.py:21-37: traces with an identical address sequence) are runs of traces in this
 * order; because nn.LSTM weights are shared and h0=c0=0 for every trace, running all sub-batches through one
 * step-major pass is arithmetically the per-sub-batch loop of InferenceNetworkLSTM._loss
 * (pyprob/nn/inference_network_lstm.py:138-219).
 */
#ifndef PYPROB_AMD_H
#define PYPROB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ABI_VERSION 15
#define PP_MAX_OBS 8
#define PP_MAX_LSTM_DEPTH 4
#define PP_MAX_OBS_DEPTH 4

/* error codes (negative; positive values are hipError_t) */
#define PP_EINVAL   (-1)   /* bad argument (shape, alignment, null pointer) */
#define PP_ENOSPACE (-2)   /* workspace too small */
#define PP_ENODEV   (-3)   /* no gfx950 device / kernels not loadable */
#define PP_EHIP     (-4)   /* a HIP runtime call failed (pp_last_error() has the text) */

/* proposal head kinds (pyprob/nn/inference_network_lstm.py:52-66) */
#define PP_HEAD_NORMAL_MIXTURE       0  /* ProposalNormalNormalMixture: prior Normal(mean, stddev) */
#define PP_HEAD_TRUNCNORMAL_MIXTURE  1  /* ProposalUniformTruncatedNormalMixture: prior Uniform(low, high) */
#define PP_HEAD_CATEGORICAL          2  /* ProposalCategoricalCategorical: prior Categorical(C) */
#define PP_HEAD_BERNOULLI            4  /* ProposalBernoulliBernoulli (proposal_bernoulli_bernoulli.py:16-20), n_out = 1. In the
                                           training loss the reference broadcasts probs [n, 1] against values [n] to an
                                           [n, n] log_prob matrix per sub-batch step and sums it (inference_network_lstm.py:
                                           195-202); the row's `prior` pair carries (n, sum of the n values) of its sub-batch
                                           step so that the row term sum_j log Bernoulli(v_j; p_row) is computed in place */
#define PP_HEAD_POISSON_TN_MIXTURE   3  /* ProposalPoissonTruncatedNormalMixture: prior Poisson; (p0, p1) = (low, high) = (0, 40) */

int         pp_abi_version(void);
const char* pp_last_error(void);
/* number of visible HIP devices whose arch is gfx950; 0 if none (never throws) */
int         pp_device_count(void);

/* ------------------------------------------------------------------------------------------------------
 * Network description. Offsets are in floats into one flat fp32 parameter buffer (and the identically laid
 * out gradient / Adam-moment buffers). Tensor shapes are the reference's.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct pp_addr {
    int32_t kind;        /* PP_HEAD_* */
    int32_t n_out;       /* head output width: 3K (mixtures) or C (categorical) */
    int32_t hid;         /* head hidden width int((H+n_out)/2), embedding_feedforward.py:26 */
    int32_t smp_in;      /* sample-embedding input width: 1, or C (one-hot) for categorical */
    int32_t dtype_id;    /* index of the distribution-type embedding this address uses */
    int32_t _pad;
    int64_t addr_emb;    /* [addr_dim]            _layers_address_embedding.<addr> */
    int64_t dtype_emb;   /* [dtype_dim]           _layers_distribution_type_embedding.<DistName> */
    int64_t smp_w;       /* [smp_dim, smp_in]     _layers_sample_embedding.<addr>._layers.0.weight */
    int64_t smp_b;       /* [smp_dim] */
    int64_t w1, b1;      /* [hid, H], [hid]       _layers_proposal.<addr>._ff._layers.0 (FeedForward network: [hid, e_obs]) */
    int64_t w2, b2;      /* [n_out, hid], [n_out] _layers_proposal.<addr>._ff._layers.1 */
} pp_addr;

typedef struct pp_net {
    int32_t n_obs;                    /* observables with a FEEDFORWARD depth-2 embedding (inference_network.py:110-118) */
    int32_t obs_in[PP_MAX_OBS];       /* flattened input width of observable o */
    int32_t obs_hid[PP_MAX_OBS];      /* int((in+out)/2) */
    int32_t obs_out[PP_MAX_OBS];      /* embedding dim of observable o */
    int64_t obs_w0[PP_MAX_OBS], obs_b0[PP_MAX_OBS], obs_w1[PP_MAX_OBS], obs_b1[PP_MAX_OBS];
    int32_t e_obs;                    /* sum of obs_out */
    int32_t smp_dim, addr_dim, dtype_dim;
    int64_t fin_w0, fin_b0, fin_w1, fin_b1;   /* _layers_observe_embedding_final (e_obs -> e_obs -> e_obs) */
    int32_t lstm_in;                  /* I = e_obs + smp_dim + 2*(addr_dim+dtype_dim), inference_network_lstm.py:30 */
    int32_t lstm_dim;                 /* H; 0 = InferenceNetworkFeedForward (inference_network_feedforward.py): no LSTM and
                                         no address / sample embeddings (lstm_in = 0, their offsets unused); the proposal
                                         layers [hid, e_obs] read the observe embedding of the trace */
    int64_t w_ih, w_hh, b_ih, b_hh;   /* _layers_lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l0 */
    int32_t n_addr;
    int32_t n_dtype;
    const pp_addr* addrs;             /* host array [n_addr] */
    const int64_t* addr_table;        /* dev  [n_addr, PP_ADDR_TABLE_COLS] same records for per-row dispatch */
    int64_t n_params;                 /* floats in the flat buffer (incl. padding) */
    int32_t lstm_depth;               /* layers of nn.LSTM(I, H, depth) (inference_network_lstm.py:31); 0 is read as 1 */
    int32_t _pad2;
    /* _layers_lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l<k> of every layer; entry 0 repeats w_ih .. b_hh above. Layer
     * k >= 1 reads the hidden states of layer k-1: weight_ih_l<k> is [4H, H] */
    int64_t lstm_w_ih[PP_MAX_LSTM_DEPTH], lstm_w_hh[PP_MAX_LSTM_DEPTH], lstm_b_ih[PP_MAX_LSTM_DEPTH], lstm_b_hh[PP_MAX_LSTM_DEPTH];
    /* observe embeddings of a depth other than 2 (EmbeddingFeedForward(num_layers = depth), embedding_feedforward.py:22-33,
     * inference_network.py:110-118): depth 1 = Linear(in, out); depth d >= 2 = Linear(in, hid), (d - 2) x Linear(hid, hid),
     * Linear(hid, out), ReLU after every layer. obs_depth[o] = 0 is read as 2 (obs_w0 .. obs_b1 above). For other depths
     * layer l of observable o is obs_w[o][l] / obs_b[o][l] (_layers_observe_embedding.<name>._layers.<l>). */
    int32_t obs_depth[PP_MAX_OBS];
    int64_t obs_w[PP_MAX_OBS][PP_MAX_OBS_DEPTH], obs_b[PP_MAX_OBS][PP_MAX_OBS_DEPTH];
    /* ObserveEmbedding.CNN2D5C (EmbeddingCNN2D5C, pyprob/nn/embedding_cnn_2d_5c.py; inference_network.py:119-120). Added
     * without a new ABI number: the fields trail the struct and zero means what the struct meant before.
     * obs_kind[o] = 0 is read as FEEDFORWARD (everything above). obs_kind[o] = PP_OBS_CNN2D5C: the observable is an image
     * obs_shape[o] = [C, H, W] (C in 1..4, H and W >= 20) of obs_in[o] = C*H*W floats in (c, y, x) order; five 3x3
     * convolutions obs_conv_w[o][l] ([Cout, Cin, 3, 3], _conv<l+1>.weight) / obs_conv_b[o][l] with two 2x2 max-pools
     * give obs_feat[o] = 128 * h5 * w5 features, flattened in (c, y, x) order; _lin1 [dim, F] / _lin2 [dim, dim] are
     * obs_w[o][0..1] / obs_b[o][0..1] with obs_depth[o] = 2 and obs_hid[o] = obs_out[o] = dim. */
    int32_t obs_kind[PP_MAX_OBS];
    int32_t obs_shape[PP_MAX_OBS][3];
    int32_t obs_feat[PP_MAX_OBS];
    int32_t _pad3;
    int64_t obs_conv_w[PP_MAX_OBS][5], obs_conv_b[PP_MAX_OBS][5];
} pp_net;

#define PP_OBS_FEEDFORWARD 0
#define PP_OBS_CNN2D5C     1
#define PP_PROF_CNN_FWD 32   /* kernel classes of the in-stream timing (pp_prof_arm below) */
#define PP_PROF_CNN_BWD 48

/* ------------------------------------------------------------------------------------------------------
 * The convolution stack of a CNN2D5C observable on its own (csrc/cnn2d.hip), for tests and timing. It replaces
 * EmbeddingCNN2D5C.forward up to the flatten (pyprob/nn/embedding_cnn_2d_5c.py:32-44: conv1 .. conv5 with ReLU, two
 * max-pools, view(batch, -1)) and autograd's backward through the same lines; _lin1 / _lin2 are ordinary linear layers.
 * x: dev [n_images, C*H*W]; features_out: dev [n_images, F]. The workspace (pp_cnn2d5c_workspace_bytes, 256-byte
 * aligned) keeps the activations: pp_cnn2d5c_backward must follow a pp_cnn2d5c_forward with the same net, o, params,
 * n_images and workspace. d_features: dev [n_images, F]; the gradients of conv1 .. conv5 (weights in the reference's
 * [Cout, Cin, 3, 3]) are ADDED to `grads` (flat buffer laid out like params). flags must be 0. The split-K partial
 * weight gradients are stored and added in a fixed order: results are bit-identical from run to run in every mode.
 * ---------------------------------------------------------------------------------------------------- */
size_t pp_cnn2d5c_workspace_bytes(const pp_net* net, int32_t o, int32_t n_images);
int pp_cnn2d5c_forward(const pp_net* net, int32_t o, const float* params, const float* x, int32_t n_images,
                       float* features_out, void* workspace, size_t workspace_bytes, void* stream);
int pp_cnn2d5c_backward(const pp_net* net, int32_t o, const float* params, const float* d_features, int32_t n_images,
                        float* grads, void* workspace, size_t workspace_bytes, int32_t flags, void* stream);

/* columns of the device address table */
#define PP_ADDR_TABLE_COLS 8
#define PP_AT_KIND 0
#define PP_AT_SMP_IN 1
#define PP_AT_ADDR_EMB 2
#define PP_AT_DTYPE_EMB 3
#define PP_AT_SMP_W 4
#define PP_AT_SMP_B 5
#define PP_AT_N_OUT 6
#define PP_AT_RESERVED 7

typedef struct pp_batch {
    int32_t n_traces;            /* B  (Batch.size, pyprob/nn/dataset.py:24) */
    int32_t n_rows;              /* R = sum of controlled trace lengths */
    int32_t t_max;               /* longest controlled trace */
    int32_t obs_width;           /* sum of obs_in */
    const int32_t* n_active;     /* host [t_max]   traces with length > t */
    const int32_t* row_off;      /* host [t_max+1] prefix sum of n_active */
    const int32_t* grp_off;      /* host [n_addr+1] rows grouped by address: group a = grp_rows[grp_off[a]:grp_off[a+1]] */
    const float*   obs;          /* dev [B, obs_width] observed values, trace order = packed order */
    const float*   value;        /* dev [R] sampled value of every controlled variable (category index as float) */
    const float*   prior;        /* dev [R, 2] (mean, stddev) | (low, high) | Poisson: (0, 40) | Bernoulli: (n, n1) of the
                                    row's sub-batch step (PP_HEAD_BERNOULLI) | Categorical: unused */
    const int32_t* addr;         /* dev [R] address id of the row */
    const int32_t* prev_row;     /* dev [R] row of the previous time step of the same trace, -1 at t = 0 */
    const int32_t* grp_rows;     /* dev [R] row ids sorted by address id */
    const int32_t* trace;        /* dev [R] trace index b of the row */
    const int32_t* row_off_dev;  /* dev [t_max+1] copy of row_off */
    const int32_t* nxt_off;      /* host [n_addr+1] rows grouped by the address of their PREVIOUS variable */
    const int32_t* nxt_rows;     /* dev [R - B] row ids (t >= 1) sorted by previous address id */
} pp_batch;

/* ------------------------------------------------------------------------------------------------------
 * Host-side minibatch packing (no device access): ragged trace-major columns -> the step-major pp_batch layout.
 * Replaces Batch.__init__ (pyprob/nn/dataset.py:21-37) and the per-trace torch.stack / torch.cat of _loss
 * (pyprob/nn/inference_network_lstm.py:146-196). `out` receives ONE buffer of 4-byte words: the first
 * info->device_words words are what the device needs (upload them with one copy), the rest are the host-side arrays of
 * pp_batch; every info field below is a word offset into `out`.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct pp_pack_info {
    int64_t n_traces, n_rows, t_max, device_words;
    int64_t obs, value, prior, addr, prev_row, grp_rows, trace, row_off_dev, nxt_rows;   /* device part */
    int64_t n_active, row_off, grp_off, nxt_off;                                         /* host part of pp_batch */
    int64_t order;      /* [B] packed trace position -> input trace index (traces are sorted longest-first) */
    int64_t src_row;    /* [R] packed row -> row of the trace-major input */
} pp_pack_info;

/* words `out` must hold; t_max = longest trace */
int64_t pp_pack_words(int32_t n_traces, int64_t n_rows, int32_t t_max, int32_t obs_width, int32_t n_addr);

/* trace_len [B]; addr_ids / values [R] and prior [R, prior_width] trace-major; obs [B, obs_width]. Errors: a trace of
 * length zero ("Trace of length zero.", dataset.py:28-29), an address id outside [0, n_addr), a short buffer. */
int pp_pack_ragged(const int32_t* trace_len, const int32_t* addr_ids, const float* values, const float* prior,
                   int32_t prior_width, const float* obs, int32_t n_traces, int32_t obs_width, int32_t n_addr,
                   void* out, int64_t out_words, pp_pack_info* info);

/* The same packing straight from the columns of a packed on-disk trace dataset (pyprob_amd/dataset.py: memory-mapped
 * .npy columns, one struct per shard): minibatch = the traces with global indices ids[0..n_ids). `first` [n_shards+1]
 * is the global index of every shard's first trace. addr_remap (or NULL) maps a shard's address ids to the network's;
 * an unmapped address (-1) is an error (the caller polymorphs first, inference_network_lstm.py:150-152). Replaces
 * OfflineDataset.__getitem__ + the DataLoader collate (pyprob/nn/dataset.py:197-205, 262). */
typedef struct pp_shard_columns {
    const int32_t* trace_len;   /* [n] */
    const int64_t* row_off;     /* [n+1] */
    const float*   obs;         /* [n, obs_width] */
    const float*   value;       /* [rows] */
    const float*   prior;       /* [rows, 2] */
    const int32_t* addr;        /* [rows] shard-local address ids */
    const int32_t* addr_remap;  /* [shard addresses] -> network address id, or NULL for identity */
} pp_shard_columns;

int pp_pack_indexed(const pp_shard_columns* shards, int32_t n_shards, const int64_t* first, const int64_t* ids,
                    int32_t n_ids, int32_t obs_width, int32_t n_addr, void* out, int64_t out_words, pp_pack_info* info);

/* ------------------------------------------------------------------------------------------------------
 * Whole-path entry points
 * ---------------------------------------------------------------------------------------------------- */

/* Bytes of scratch HBM pp_ic_loss needs for a batch of at most n_traces traces / n_rows rows.
 * The workspace must be ZERO-FILLED once when it is allocated and must not be written by the caller afterwards: its
 * first bytes (a size that depends on the network only) hold the exchange areas of the LSTM tail kernels
 * (csrc/lstm_tail.hip), whose tagged words must never be mistaken for fresh ones. Everything else in it is scratch
 * of a single call. */
size_t pp_ic_workspace_bytes(const pp_net* net, int32_t n_traces, int32_t n_rows);

#define PP_LOSS_BACKWARD   1   /* also write dLoss/dparams into `grads` */
#define PP_LOSS_ZERO_GRADS 2   /* zero `grads` (n_params floats) first: optimizer.zero_grad(), inference_network.py:486 */
#define PP_LOSS_KEEP_LP    4   /* write the per-row proposal log_prob (row order) to lp_out */

/*
 * InferenceNetworkLSTM._loss(batch) (+ loss.backward()):  pyprob/nn/inference_network_lstm.py:136-220,
 * pyprob/nn/inference_network.py:487,493. Computes
 *     loss = -(1/B) * sum_rows log q(value | lstm state)          (written to loss_out[0], dev)
 * with -inf log-probs replaced by log(1e-8) (:207-213); status_out[0] (dev int32) is set non-zero if the loss
 * is still non-finite (the reference then skips the batch, :216-217). With PP_LOSS_BACKWARD, `grads` receives
 * the gradient of every parameter in the layout of `params` (tensors that do not participate stay zero).
 */
int pp_ic_loss(const pp_net* net, const pp_batch* batch, const float* params /*dev*/, float* grads /*dev or NULL*/,
               void* workspace /*dev*/, size_t workspace_bytes, float* loss_out /*dev [1]*/,
               int32_t* status_out /*dev [1]*/, float* lp_out /*dev [R] or NULL*/, int32_t flags, void* stream);

/*
 * torch.optim.Adam.step() over the flat buffer (pyprob/nn/inference_network.py:348,496), per-tensor skipping
 * of parameters whose grad is None (tensors that did not take part in the loss) and per-tensor step counts.
 *   chunk_tensor  dev [n_params/1024]  tensor id owning each 1024-float chunk (tensors are padded to 1024 and laid
 *                                      out in id order: the ids ascend)
 *   active        dev [n_tensors]      float >0 -> tensor has a gradient this step (DP: all-reduced presence map,
 *                                      pyprob/nn/inference_network.py:300-315)
 *   tensor_step   dev [n_tensors]      int32 Adam step count per tensor, incremented here when active
 *   scratch       dev [PP_ADAM_SCRATCH * n_tensors] int32, opaque, owned by the optimizer state: ZERO before the
 *                                      first call and whenever chunk_tensor changes (two-level arrival counters - the
 *                                      last chunk of a tensor to finish advances its step count - the cached
 *                                      chunk run of each tensor, and word PP_ADAM_SEEN: non-zero once the tensor had a
 *                                      non-zero gradient. While it is 0 the tensor's moments are taken to be zero and
 *                                      all-zero gradient chunks are skipped: a caller that writes exp_avg / exp_avg_sq
 *                                      itself (checkpoint load) sets the word of every tensor to 1)
 *   grad_scale    1/world_size for data-parallel averaging (:324-325), else 1
 *   flags         PP_ADAM_ZERO_GRADS: clear every consumed gradient chunk (optimizer.zero_grad() of the next step,
 *                 inference_network.py:486); the next pp_ic_loss can then run without PP_LOSS_ZERO_GRADS
 *   skip          dev int32[1] or NULL: when non-zero the call does nothing - pass pp_ic_loss's status_out to skip a
 *                 batch whose loss is not finite (inference_network_lstm.py:216-217) without reading it on the host
 * One launch (bias corrections are derived per chunk from the tensor's step count).
 */
#define PP_ADAM_ZERO_GRADS 1
#define PP_ADAM_SCRATCH 1056
#define PP_ADAM_SEEN 1027
int pp_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n_params,
                 const int32_t* chunk_tensor, const float* active, int32_t* tensor_step, int32_t* scratch,
                 int32_t n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                 int32_t flags, const int32_t* skip, void* stream);

/*
 * The same step for the training paths: workgroups are launched for the LIVE chunks only. The library keeps, per bound
 * gradient buffer, a host-side mark per tensor - "its gradient or its moments may be non-zero" (touched). pp_ic_loss marks
 * the tensors its backward pass writes; every other entry of this header that can write into a bound gradient or moment
 * buffer (pp_dp_reduce_grads outside its skip ranges, pp_adam_step itself - its caller filled the gradients -, pp_sgd_step,
 * pp_larc_scale, pp_axpy, pp_gemm_f32, ...) and a live step with weight decay mark all tensors; a caller that writes the buffers itself (checkpoint load, its own collectives, torch operators) calls
 * pp_adam_live_mark_touched. Marks are never cleared. While a tensor is untouched its gradient and moments are exactly
 * zero, so without weight decay Adam only advances its step count: the launch covers the chunk runs of the touched tensors
 * (all tensors when weight_decay != 0) and one thread per remaining tensor. Same results as pp_adam_step, bit for bit; the
 * two may alternate on one state. Falls back to pp_adam_step's launch when `grads` is not bound, when the runs exceed the
 * kernel-argument table (4) and with PP_ADAM_LIVE=0 (read per call).
 *   pp_adam_live_bind     tensor_first host [n_tensors + 1]: first chunk of each tensor, ascending, [n_tensors] = n_params / 1024.
 *                         clean != 0: the three buffers were just zero-filled (no tensor touched); 0: all tensors touched.
 *                         Re-binding replaces the record; pp_adam_live_unbind forgets it (before the buffers are freed).
 *   pp_adam_live_mark_touched   buffer: any pointer into a bound gradient / moment buffer; marks all its tensors.
 *   pp_adam_live_info     out host int64 [4] = {bound, marks version, tables built so far, untouched tensors};
 *                         touched_out host uint8 [n_tensors] or NULL.
 *   pp_adam_live_plan     the run builder alone (host only): live host uint8 [n_tensors]; out host int32 [21] =
 *                         {runs, workgroups of the runs, gaps, 4 x {first workgroup, first chunk},
 *                         5 x {first tensor, end tensor} of the gaps}. Returns 0, or 1 when the runs exceed the table
 *                         (full grid), < 0 on a bad argument.
 */
int pp_adam_step_live(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n_params,
                      const int32_t* chunk_tensor, const float* active, int32_t* tensor_step, int32_t* scratch,
                      int32_t n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                      int32_t flags, const int32_t* skip, void* stream);
int pp_adam_live_bind(const float* grads /*dev*/, const float* exp_avg /*dev*/, const float* exp_avg_sq /*dev*/, int64_t n_params,
                      const int32_t* tensor_first /*host*/, int32_t n_tensors, int32_t clean);
int pp_adam_live_unbind(const float* grads);
int pp_adam_live_mark_touched(const void* buffer);
/* the tensors that hold floats [offset, offset + count) of the bound gradient buffer `grads` (the caller wrote those
 * gradients, or the moments at the same offsets) */
int pp_adam_live_mark_range(const float* grads, int64_t offset, int64_t count);
int pp_adam_live_info(const float* grads, int64_t* out /*host [4]*/, uint8_t* touched_out /*host or NULL*/);
int pp_adam_live_plan(const int32_t* tensor_first /*host*/, int32_t n_tensors, const uint8_t* live /*host*/,
                      int32_t* out /*host [21]*/);
/* the table pp_adam_step_live would launch with for these (bound) buffers now - built, or taken from the record's cache (host
 * only; `out` as above). Returns 1 when it would launch the full grid. */
int pp_adam_live_table(const float* grads, const float* exp_avg, const float* exp_avg_sq, int64_t n_params, int32_t n_tensors,
                       float weight_decay, int32_t* out /*host [21]*/);

/*
 * optimizer.step() for torch.optim.SGD(lr, momentum, nesterov, weight_decay) - Optimizer.SGD of
 * InferenceNetwork._create_optimizer (pyprob/nn/inference_network.py:349-350, nesterov=True there) - over the same flat
 * buffers as pp_adam_step (chunk_tensor / active / grad_scale / flags / skip mean the same):
 *   g = grad * grad_scale + weight_decay * p;  buf = momentum * buf + g;  p -= lr * (nesterov ? g + momentum * buf : buf)
 * momentum_buf (dev [n_params], may be NULL when momentum == 0) must be ZERO before a parameter's first step: that is
 * torch's `buf = clone(grad)` of a first step. Tensors with active[t] == 0 are not touched (no decay, buffer unchanged).
 * One launch.
 */
int pp_sgd_step(float* params, float* grads, float* momentum_buf, int64_t n_params, const int32_t* chunk_tensor,
                const float* active, int32_t n_tensors, float lr, float momentum, int32_t nesterov, float weight_decay,
                float grad_scale, int32_t flags, const int32_t* skip, void* stream);

/*
 * The LARC wrapper of Optimizer.ADAM_LARC / SGD_LARC (pyprob/nn/optimizer_larc.py:72-107; inference_network.py:351-352
 * constructs it with the defaults trust_coefficient 0.002, clip = 1, eps 1e-8, epsilon 1/16000): per tensor with a
 * gradient,  local = (|p| != 0 && |g| != 0) ? trust * |p| / (|g| + weight_decay * |p| + eps) : epsilon,
 * adaptive = clip ? min(local / lr, 1) : local,  and IN PLACE  grad = (grad * grad_scale + weight_decay * p) * adaptive
 * (|g| is the norm of grad * grad_scale: the reference divides by the world size before the optimizer runs, :324-325).
 * The wrapped optimizer then steps with weight_decay = 0 and grad_scale = 1 (optimizer_larc.py:81,105-107):
 *   pp_larc_scale(..., lr, wd, 1/world, ...);  pp_adam_step / pp_sgd_step(..., lr, ..., 0.0f, 1.0f, ...).
 * scratch: dev, PP_LARC_SCRATCH_FLOATS(n_params, n_tensors) floats, contents irrelevant. Three launches (chunk partial sums
 * of squares, stored; per-tensor norms in fp64 in a fixed order; the rescaling pass): bit-reproducible. skip as above.
 */
#define PP_LARC_SCRATCH_FLOATS(n_params, n_tensors) (2 * ((n_params) / 1024) + (n_tensors))
int pp_larc_scale(const float* params, float* grads, int64_t n_params, const int32_t* chunk_tensor, const float* active,
                  int32_t n_tensors, float lr, float weight_decay, float grad_scale, float trust_coefficient, float eps,
                  float epsilon, int32_t clip, float* scratch, const int32_t* skip, void* stream);

/*
 * The body of the training loop (InferenceNetwork.optimize, pyprob/nn/inference_network.py:461-499: next minibatch ->
 * zero_grad -> _loss -> backward -> optimizer.step) for a RUN of minibatches whose traces come from packed dataset
 * columns, without returning to the caller between steps. Per step i: the traces ids[step_off[i] .. step_off[i+1]) are
 * packed (pp_pack_indexed) into a pinned staging slot together with the minibatch's presence map, uploaded with one
 * asynchronous copy, and pp_ic_loss(PP_LOSS_BACKWARD) + pp_adam_step(lr[i], PP_ADAM_ZERO_GRADS, skip = the step's own
 * non-finite flag) are enqueued on `stream`. loss_ring[i] / status_ring[i] receive the step's loss and non-finite flag
 * (a flagged step leaves the parameters untouched, :493-499). Single rank (data parallel runs keep the per-step
 * all-reduce on the caller's side). The caller polymorphs beforehand: an address unknown to `net` is PP_EINVAL.
 *   pp_tensor_roles  which tensors a minibatch gives a gradient to (grad is not None in the reference): tensor t is
 *                    present if role[t] & 4, or if one of its addresses addr[off[t] .. off[t+1]) occurs as a current
 *                    (role & 1) / previous (role & 2) variable of the minibatch (inference_network_lstm.py:168-171).
 *   staging          pinned host memory, device_batch device memory: n_slots slots of slot_words 4-byte words each,
 *                    slot_words >= pp_train_slot_words(...) of the largest step. The slots form two halves: a group of
 *                    up to n_slots/2 consecutive steps is packed into one half and uploaded with ONE copy (group
 *                    sizes ramp 1, 2, 4, ...); a half is rewritten only after its upload completed.
 *   workspace        pp_ic_workspace_bytes(net, most traces, most rows of any step)
 *   grads_clean      non-zero: `grads` is all zero on entry (left so by PP_ADAM_ZERO_GRADS); it is on return.
 *   addr_iterations  host [n_addr] or NULL: += 1 per step in which the address occurs (proposal_layer.
 *                    _total_train_iterations, inference_network_lstm.py:198)
 * Returns as soon as the last step is enqueued (the last uploads may still be pending: the next call waits for them
 * before it rewrites a staging half; pp_train_sync() waits for them explicitly - call it before freeing or reusing the
 * staging memory). One training run at a time per process. The losses are read by the caller.
 */
typedef struct pp_train_buffers {
    float* params; float* grads; float* exp_avg; float* exp_avg_sq;             /* dev [n_params] */
    const int32_t* chunk_tensor; int32_t* tensor_step; int32_t* adam_scratch;   /* dev, as in pp_adam_step */
    void* workspace; size_t workspace_bytes;                                     /* dev */
    void* staging; void* device_batch; int64_t slot_words;                       /* pinned host / dev */
    float* loss_ring; int32_t* status_ring;                                      /* dev [n_steps] */
    int32_t n_tensors; int32_t n_slots;
    /* data parallel (ABI 6): dp_world = size of the communicator of pp_dp_init (0: single rank). `grads` is then the flat
     * buffer [n_params | n_tensors presence flags | loss | non-finite flag]; between backward and Adam of every step the
     * loop all-reduces it (minus the dp_n_skip ranges [dp_skip_off, + dp_skip_cnt) that are zero on every rank), Adam divides
     * by dp_world and every rank skips a step that any rank flagged (pyprob/nn/inference_network.py:296-333, 448) */
    int32_t dp_world; int32_t dp_n_skip;
    int64_t dp_skip_off[4], dp_skip_cnt[4];
} pp_train_buffers;

typedef struct pp_tensor_roles {
    const int32_t* off;    /* host [n_tensors + 1] */
    const int32_t* addr;   /* host [off[n_tensors]] address ids */
    const int32_t* role;   /* host [n_tensors] bit 0: current variable, bit 1: previous variable, bit 2: always */
} pp_tensor_roles;

int64_t pp_train_slot_words(int32_t n_traces, int64_t n_rows, int32_t t_max, int32_t obs_width, int32_t n_addr,
                            int32_t n_tensors);

int pp_train_sync(void);
/* The same loop body (optimize, inference_network.py:486-496: zero_grad -> _loss -> backward -> [all-reduce] -> Adam) for
 * minibatches that are ALREADY resident in HBM: batches[i] = pp_batch of step i (device arrays in place, host arrays valid
 * for the duration of the call), active[i] = dev [n_tensors] presence map of that minibatch, lr[i] its learning rate; losses
 * and flags go to tb->loss_ring / status_ring [n_steps] (staging / device_batch of tb are not used). One C call enqueues
 * n_steps steps; tb->dp_world selects the data-parallel branch like in pp_train_steps. */
int pp_train_resident(const pp_net* net, const pp_train_buffers* tb, const pp_batch* const* batches,
                      const float* const* active, int32_t n_steps, const float* lr, float beta1, float beta2, float eps,
                      float weight_decay, int32_t grads_clean, void* stream);

int pp_train_steps(const pp_net* net, const pp_train_buffers* buffers, const pp_tensor_roles* roles,
                   const pp_shard_columns* shards, int32_t n_shards, const int64_t* first, int32_t obs_width,
                   const int64_t* ids, const int64_t* step_off, int32_t n_steps, const float* lr /*host [n_steps]*/,
                   float beta1, float beta2, float eps, float weight_decay, int32_t grads_clean,
                   int64_t* addr_iterations, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Importance sampling with the inference network, lock-step over N particles
 * (pyprob/state.py:203-219, pyprob/nn/inference_network_lstm.py:82-134, pyprob/trace.py:123-125)
 * ---------------------------------------------------------------------------------------------------- */

/* Bytes of scratch for pp_is_step with n particles. The workspace must be ZERO-FILLED once when it is allocated (it holds an
 * arrival counter of the first-statement kernels, which every launch leaves at zero); everything else in it is scratch of a
 * single call. */
size_t pp_is_workspace_bytes(const pp_net* net, int32_t n);

/*
 * InferenceNetwork._infer_init(observe): observe embedding of the single observation, batch 1
 * (pyprob/nn/inference_network.py:141-148). obs: dev [obs_width]; e_out: dev [e_obs].
 */
int pp_is_init(const pp_net* net, const float* params, const float* obs, float* e_out, void* workspace,
               size_t workspace_bytes, void* stream);

/*
 * One controlled `pyprob.sample` statement for n particles at once: _infer_step (LSTM step with carried
 * (h, c)) -> proposal head -> value ~ q -> log q(value).
 *   addr_id / prev_addr_id   address of this / the previous controlled variable (-1: first variable of the trace)
 *   e_obs_vec  dev [e_obs]   output of pp_is_init (shared by all particles)
 *   prev_value dev [n]       values sampled at the previous statement (ignored when prev_addr_id < 0)
 *   prior      dev [n,2] or [2] (prior_stride 0 = same prior parameters for every particle)
 *   h, c       dev [depth, n, H] LSTM state of every layer (layer k at offset k * n * H), updated in place
 *   state_rows 1 or n: rows of (h, c) that are valid on entry. The first statement of a trace (prev_addr_id < 0) ignores
 *              the state, evaluates the network for ONE row (every particle has the same input and zero state) and
 *              writes row 0 only: the caller passes state_rows = 1 to the next call, which turns the shared recurrent
 *              term into a bias row and writes all n rows; afterwards state_rows = n.
 *              FeedForward network (lstm_dim 0; inference_network_feedforward.py:52-66): no state - h, c, prev_value,
 *              prev_addr_id and state_rows are ignored (h, c may be NULL); the layer of addr_id is applied to e_obs_vec.
 *   value_in   dev [n] or NULL: if given, score these values instead of sampling (re-scoring / parity tests)
 *   value_out  dev [n]       sampled (or copied) values
 *   logq_out   dev [n]       proposal log_prob of value (Mixture.log_prob / Categorical.log_prob)
 *   seed, offset             Philox4x32-10 counter-based RNG: particle i uses counter (offset + i)
 */
int pp_is_step(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n,
               const float* e_obs_vec, const float* prev_value, const float* prior, int32_t prior_stride,
               float* h, float* c, int32_t state_rows, const float* value_in, float* value_out, float* logq_out,
               uint64_t seed, uint64_t offset, void* workspace, size_t workspace_bytes, void* stream);

/* pp_is_step for the particles of a diverged control-flow path (pyprob/state.py:203-219 on a subset of the traces of
 * pyprob/model.py:59): particle i of the call owns row rows[i] of (h, c) (dev int64 [n], distinct rows; NULL = row i) - the
 * state is read and written in place through the list, every other per-particle array (prev_value, prior, value_in / out,
 * logq_out) is compact [n]. Statements after the first one only (prev_addr_id >= 0), and only where the fused statement
 * kernel exists (csrc/is_step_fused.hip: one-layer LSTM, H = 256, 512 or 1024; csrc/is_step_small.hip: H a multiple of 32 up to 256 with 1 ..
 * PP_MAX_LSTM_DEPTH layers; head at most 32 outputs wide); PP_EINVAL otherwise (the caller gathers / scatters the rows itself).
 * (ABI 14) state_rows with a row list: 1 = row 0 is everybody's previous state (one-layer LSTMs only), otherwise the ROW COUNT OF
 * ONE LAYER of the state buffer - (h, c) are [depth, state_rows, H], layer k at offset k * state_rows * H, and rows[i] < state_rows.
 * (Up to ABI 13 the callers passed n here, which made a path of exactly one particle read row 0 as a shared state.) pp_is_step_fused_supported(net, addr_id, n) != 0: the kernel exists AND is
 * the faster path for n particles (below ~3 000 rows a launch is one generation of latency-bound workgroups and pp_is_step's
 * chain of small launches wins; pp_is_step makes the same choice).
 * With that kernel a statement is ONE launch (+ one preparation launch): gates, LSTM cell, both head layers, the draw and
 * log q; the gate pre-activations never reach memory, (h, c) are read once and written once.
 * H = 32, 64 .. 256 (csrc/is_step_small.hip, one kernel at every n; H = 256 from two layers on): a workgroup owns 64 particles, wave (row block, unit block)
 * the four gates of 32 hidden units; the old hidden rows of every layer are staged in LDS once, layer l reads the fresh rows of
 * layer l - 1 from an LDS tile; the draw is the chain's own one-lane-per-particle tail.
 * H = 1024 (one layer): the statement is TWO launches - the LSTM step as one wide launch (two workgroups per 32 particles, half of
 * the hidden units each; gates on the accumulators, c in place, the new hidden rows through a scratch) and the head-only launch
 * (state rows, both head layers, draw, log q, whole-statement tail) - from 2 049 particles on (pp_is_step_fused_supported says so
 * per n); below that pp_is_step takes the chain of GEMM launches, pp_is_step_rows / pp_is_statement_rows still the two launches. */
int pp_is_step_rows(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n,
                    const float* e_obs_vec, const float* prev_value, const float* prior, int32_t prior_stride,
                    float* h, float* c, int32_t state_rows, const int64_t* rows, const float* value_in, float* value_out,
                    float* logq_out, uint64_t seed, uint64_t offset, void* workspace, size_t workspace_bytes, void* stream);
int pp_is_step_fused_supported(const pp_net* net, int32_t addr_id, int32_t n);
/* The WHOLE statement of state.sample's IC branch (pyprob/state.py:203-219) for the particles of one control-flow path in ONE
 * launch of the fused statement kernel: particle i owns row r = rows[i] (NULL: r = i) of the state AND of the full-width
 * per-particle vectors - its previous value is prev_value_full[r], the drawn value goes to value_full[r], and
 * lw_full[r] += log p(v) - log q(v) with p the program's own prior (prior_kind 0: Normal(prior[0], prior[1]), 1: Uniform[prior[0],
 * prior[1]); prior_stride as in pp_is_step, rows of `prior` are compact). Replaces gather of the previous values + pp_is_step_rows
 * + scatter of the values + pp_logweight_accumulate + pp_axpy. Statements after the first one, mixture heads, where
 * pp_is_step_fused_supported says so; PP_EINVAL otherwise. */
int pp_is_statement_rows(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n,
                         const float* e_obs_vec, const float* prev_value_full, const float* prior, int32_t prior_stride,
                         float* h, float* c, int32_t state_rows, const int64_t* rows, float* value_full, float* lw_full,
                         int32_t prior_kind, uint64_t seed, uint64_t offset, void* workspace, size_t workspace_bytes,
                         void* stream);

/* log p(value) of prior and likelihood terms, accumulated into the per-particle log-weight:
 *     lw[i] += scale * log_prob(dist(params_i); x_i)
 * (state.py:211-217: +prior, -proposal; state.py:147-149: +likelihood_importance * likelihood), evaluated in fp32 like
 * the torch.distributions classes behind pyprob/distributions/{normal,uniform,poisson,bernoulli,categorical}.py.
 *   kind: 0 Normal(p0=mean, p1=stddev), 1 Uniform(p0=low, p1=high) with support [low, high),
 *         3 Poisson(p0=rate), 4 Bernoulli(p0=probs) (p1 unused, may be NULL),
 *         5 Categorical: p0 = probs row(s) of p1_stride categories, row i at p0 + i * p0_stride (0 = one shared row);
 *           x = category index as float; p1 unused
 *   p0/p1/x strides: 0 broadcasts a single value, 1 reads per particle. lw and lp_out are optional (dev [n]). */
int pp_logweight_accumulate(int32_t kind, const float* p0, int32_t p0_stride, const float* p1, int32_t p1_stride,
                            const float* x, int32_t x_stride, float scale, float* lw /*dev [n]*/, float* lp_out,
                            int32_t n, void* stream);

/* The same term for the particles of ONE control-flow path of a lock-step run (the reference scores one trace at a time,
 * state.py:147-149, 211-217; a path is the set of particles that took the same branches):
 *     lw[r] += scale * log_prob(dist(params_r); x_r)   for r = rows[j], j < m
 * rows: dev int64 [m], ascending particle indices; strides as above (1 = indexed by the particle, not by j). */
int pp_logweight_accumulate_rows(int32_t kind, const float* p0, int32_t p0_stride, const float* p1, int32_t p1_stride,
                                 const float* x, int32_t x_stride, float scale, float* lw /*dev [n]*/,
                                 const int64_t* rows, int32_t m, void* stream);

/* dst[r] = src[r * src_stride] for r = rows[j], j < m (src_stride 0: one shared value): what a path's execution of the program
 * returned, into the call's per-particle result vector (model.py:66-74 collects one trace's result at a time). */
int pp_copy_rows(const float* src, int32_t src_stride, float* dst /*dev [n]*/, const int64_t* rows, int32_t m, void* stream);

/* A branch of the program taken per particle (`while s >= 1:` - the reference runs the Python condition per trace): stable
 * partition of a path's rows by a condition byte per particle.
 *   cond: dev uint8 [n] (torch.bool storage), indexed by the PARTICLE; rows: dev int64 [m] ascending, or NULL = particles 0..m-1
 *   rows_true / rows_false: dev int64 [m] each; the first counts[0] / counts[1] entries are written, ascending
 *   counts: dev int32 [2] = { rows whose condition is non-zero, the others };  scratch: dev int32 [PP_PARTITION_SCRATCH(m)]
 * Two launches, no host synchronisation (the caller reads `counts` when it needs the decision). */
#define PP_PARTITION_SCRATCH(m) (((m) + 1023) / 1024 + 1)
int pp_partition_rows(const uint8_t* cond, const int64_t* rows, int32_t m, int64_t* rows_true, int64_t* rows_false,
                      int32_t* counts, int32_t* scratch, void* stream);
/* (ABI 13) The same partition with the decision POLLED instead of copied back: counts = int32 [3] in host-mapped (pinned)
 * memory; the kernel stores counts[0], counts[1] and then, behind a system-scope fence, counts[2] = seq (non-zero; the caller
 * cleared the word before the call and spins on it). A branch of a lock-step run costs the host a poll of ~10 us instead of a
 * blocking 8-byte device-to-host copy of ~45 us (profiles/r04x_gumm_call_timeline_after.csv: the gap behind every
 * __amd_rocclr_copyBuffer). m must be > 0. */
int pp_partition_rows_polled(const uint8_t* cond, const int64_t* rows, int32_t m, int64_t* rows_true, int64_t* rows_false,
                             int32_t* counts /*host-mapped [3]*/, int32_t seq, int32_t* scratch, void* stream);

/* Up to four log-weight terms in ONE pass over the particles:
 *   lw[i] (+)= sum_t scale_t * term_t(i);  kind as in pp_logweight_accumulate, or 2: the value x itself (e.g. -log q)
 * overwrite != 0 starts from 0 instead of the current lw (saves the zero-fill). */
typedef struct pp_lw_term {
    int32_t kind, p0_stride, p1_stride, x_stride;
    const float *p0, *p1, *x;
    float scale;
} pp_lw_term;
int pp_logweight_terms(const pp_lw_term* terms, int32_t count, float* lw /*dev [n]*/, int32_t n, int32_t overwrite,
                       void* stream);

/* One posterior statement of a lock-step run in ONE pass over the particles (state.sample IC branch pyprob/state.py:203-219 +
 * the state.observe terms that follow it :118-155 + Trace.end's sum pyprob/trace.py:123-125 + the Empirical reductions
 * pyprob/distributions/empirical.py:298-309, 451-466, 758-766):
 *   pp_is_step_net  the network part of pp_is_step (LSTM step + proposal layer); the head outputs stay in the workspace.
 *   pp_is_fused     per particle: draw v ~ q (addr_id >= 0: the SHARED proposal of a trace's first statement, left in the
 *                   workspace by pp_is_step_net; mixture heads; same Philox stream as pp_is_step), lw (+)= -log q(v) +
 *                   sum_t scale_t term_t(i); value[i] = v. addr_id < 0: no draw, `value` is read. term_flags[t] bit 0 / 1 / 2:
 *                   p0 / p1 / x of term t IS the particle's value (e.g. the mean of the likelihood Normal(mu, s) after
 *                   mu = sample(...)). stats_out != NULL: the statistics of pp_is_stats over (lw, value) in the same pass.
 *                   At most 8 terms. 8 bytes per particle reach memory. */
int pp_is_step_net(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n,
                   const float* e_obs_vec, const float* prev_value, float* h, float* c, int32_t state_rows, void* workspace,
                   size_t workspace_bytes, void* stream);
/* (ABI 12) pp_is_init + pp_is_step_net(addr_id, prev_addr_id = -1) of a trace's FIRST statement as ONE launch: the observe
 * embedding of the one shared row (InferenceNetwork._infer_init, pyprob/nn/inference_network.py:141-148) is computed inside the
 * launch of the LSTM step (_infer_step with prev_variable None, pyprob/nn/inference_network_lstm.py:82-134), the proposal layer's
 * workgroups ride behind the LSTM's in the same launch (environment PP_IS_FIRST=2: as a second launch), its outputs stay in the
 * workspace for pp_is_fused. `obs` (the observation vector, as for pp_is_init) may be host-mapped (pinned)
 * memory: the kernel reads it in place, a posterior call needs no copy launch. e_out: [round4(e_obs) + 8]: the embedding, then the
 * first 8 observation values (device copies: the x of the call's observe terms). (h, c): row 0 is written (state_rows = 1).
 * Bit-identical to the two calls it replaces. pp_is_first_statement_supported: one-layer LSTM, lstm_in <= 256, an embedding
 * the fused embedding kernels take. A statistics buffer of pp_is_fused / pp_is_stats may likewise be host-mapped memory: its
 * element [5] (the count) is stored last, behind a system-scope fence - a caller that set it negative may poll it. */
int pp_is_first_statement_supported(const pp_net* net, int32_t addr_id);
int pp_is_first_statement(const pp_net* net, const float* params, const float* obs, int32_t addr_id, float* e_out, float* h, float* c,
                          void* workspace, size_t workspace_bytes, void* stream);
int pp_is_fused(const pp_net* net, int32_t addr_id, int32_t n, const float* prior /*dev [2]*/, const pp_lw_term* terms,
                const int32_t* term_flags, int32_t n_terms, float* value /*dev [n]*/, float* lw /*dev [n]*/, int32_t overwrite,
                uint64_t seed, uint64_t offset, double* stats_out /*dev [6] or NULL*/, double* stats_scratch, void* workspace,
                size_t workspace_bytes, void* stream);

/* Batched posteriors: M observations ("groups") with n_per particles each in ONE lock-step call. The reference serves one
 * observation per posterior call (pyprob/model.py:106-117; InferenceNetwork._infer_init embeds THE observation,
 * pyprob/nn/inference_network.py:141-148, and every trace's first _infer_step runs on it,
 * pyprob/nn/inference_network_lstm.py:82-134, inference_network_feedforward.py:52-66; state.sample / state.observe score one
 * trace at a time, pyprob/state.py:118-155, 203-219; Empirical reduces one posterior, pyprob/distributions/empirical.py:298-309,
 * 451-466, 758-766): posteriors for M observations are M calls there, and M pp_is_first_statement + pp_is_fused pairs here.
 *   pp_is_batch_workspace_bytes  scratch of the calls below (and of pp_is_batch_bias / pp_is_statement_groups, whose weight images
 *                       lie at its end) for n_groups observations (no zero-fill needed; independent of n_per).
 *   pp_is_batch_first   _infer_init + _infer_step(prev_variable = None) + the proposal layer of `addr_id` for M DIFFERENT
 *                       observations: obs dev [M, obs_width] (the observables' values in the network's order), y_out dev
 *                       [M, ldy] (ldy a multiple of 4, >= the head's n_out) receives the head outputs - row g is what
 *                       pp_is_first_statement leaves in its workspace for observation g, up to the rounding of another summation
 *                       order. h_out / c_out: dev [M, H] or NULL - the LSTM state after the statement (for a caller that
 *                       continues with a second statement; ignored by a FeedForward network). FEEDFORWARD and CNN2D5C observe
 *                       embeddings, a FeedForward network or an LSTM of depth 1; PP_EINVAL otherwise. The launches are those of
 *                       the training step's forward at T = 1: embedding GEMMs, input gather, gate GEMM, cell, head GEMMs. A
 *                       CNN2D5C observable (embedding_cnn_2d_5c.py): its M images - columns [ci, ci + C H W) of the obs rows, ci
 *                       the widths of the observables before it - go through the convolution stack in ONE pass at B = M
 *                       (pp_cnn2d5c_forward's launches, no backward images) into an [M, round4(F)] feature block of the
 *                       workspace that _lin1 / _lin2 read, as pp_is_init does for one image. An image's features have the same
 *                       bits whatever batch it sits in; the linear layers after them pick their shape by M. The workspace grows
 *                       by the feature block and pp_cnn2d5c_workspace_bytes(o, M) per CNN2D5C observable, laid between the
 *                       network rows and the fragment images; a network without one keeps its size byte for byte.
 *   pp_is_fused_groups  pp_is_fused for the M n_per particles: particle i = g n_per + j belongs to group g, draws from the
 *                       proposal in row g of `y` (mixture heads; Philox counter offset + i, the key and stream of pp_is_fused and
 *                       pp_is_step - an M-group call consumes exactly the counters of M one-group calls at offset + g n_per),
 *                       lw[i] (+)= - log q(v) + sum_t scale_t term_t(i), value[i] = v; addr_id < 0: no draw, `value` is read (y
 *                       and prior may be NULL). The terms are pp_lw_term's with the three stride fields holding an OPERAND CODE:
 *                       0 one shared value, 1 one value per particle (index i), 2 one value per group (index g); Categorical
 *                       (kind 5): p0_stride codes which row of p1_stride weights - the shared one, row i or row g. term_flags as
 *                       in pp_is_fused. stats_out != NULL: dev double [M, 6], row g = the six numbers of pp_is_stats over group g
 *                       (w = exp(lw - max lw) with exp in fp64), reduced by dependent launches on the same stream in a fixed
 *                       order that depends on n_per alone - bit-identical from run to run and between an M-group call and the
 *                       one-group call on the same particles. At most 8 terms, any n_per >= 1; 8 bytes per particle are
 *                       written, the statistics read them once more. `net` is required (also without a draw). Of the
 *                       workspace only the first PP_IS_GROUP_STATS_BYTES(n_groups) bytes are used, and only with stats_out.
 *                       overwrite | PP_GROUPS_PRIOR_PER_PARTICLE: `prior` is dev [M n_per, 2], one pair per particle (a later
 *                       statement of a FeedForward network whose prior depends on an earlier draw). */
#define PP_IS_GROUP_STATS_BYTES(m) ((size_t)((m) > 256 ? (m) : 256) * 48)
#define PP_GROUPS_PRIOR_PER_PARTICLE 2
size_t pp_is_batch_workspace_bytes(const pp_net* net, int32_t n_groups);
int pp_is_batch_first(const pp_net* net, const float* params, const float* obs /*dev [M, obs_width]*/, int32_t addr_id, int32_t n_groups,
                      float* y_out /*dev [M, ldy]*/, int64_t ldy, float* h_out, float* c_out /*dev [M, H] or NULL*/, void* workspace,
                      size_t workspace_bytes, void* stream);
int pp_is_fused_groups(const pp_net* net, int32_t addr_id, int32_t n_groups, int32_t n_per, const float* y /*dev [M, ldy]*/, int64_t ldy,
                       const float* prior /*dev [2]*/, const pp_lw_term* terms, const int32_t* term_flags, int32_t n_terms,
                       float* value /*dev [M n_per]*/, float* lw /*dev [M n_per]*/, int32_t overwrite, uint64_t seed, uint64_t offset,
                       double* stats_out /*dev double [M, 6] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* Later statements of a batched posterior call: the second, third, ... controlled sample statement of a straight-line program for
 * all M n_per particles at once. The reference runs one _infer_step per trace and statement (InferenceNetworkLSTM._infer_step
 * pyprob/nn/inference_network_lstm.py:82-134: the LSTM input row [E | s_prev | d_prev | a_prev | d_cur | a_cur] :116-121, one
 * nn.LSTM step :123-125, the proposal layer :127-131; state.sample's IC branch pyprob/state.py:203-219; Mixture.sample / log_prob
 * pyprob/distributions/mixture.py:38-63) inside one posterior call per observation (pyprob/model.py:106-117).
 *   pp_is_batch_bias    the per-group part of the gate pre-activations of statement (addr_id, prev_addr_id >= 0): bias_out dev
 *                       [M, 4H], row g = b_ih + b_hh + W_ih[:, shared columns] [E_g | 0 | d_prev | a_prev | d_cur | a_cur]
 *                       (+ h_prev[g] W_hh^T with h_prev dev [M, H]: the second statement, whose previous state is one row per
 *                       group). E_g are embedding rows the LAST pp_is_batch_first call left in `workspace` (kept, not recomputed):
 *                       that call embedded ws_groups observations, this one serves rows [first_group, first_group + n_groups)
 *                       of them - a caller that shards a call over groups embeds once and takes its slices, so that a shard's
 *                       rows do not depend on the shard's size (the GEMMs of pp_is_batch_first pick their shape by the row
 *                       count). One launch on a (gate column, group) grid running pp_is_step's own bias
 *                       code: the products and their order are those of the single call and do not depend on M. One-layer LSTM,
 *                       FEEDFORWARD or CNN2D5C observe embeddings (the rows are read, no image is embedded again), a mixture head
 *                       at addr_id (the only consumer is the call below).
 *   pp_is_statement_groups  the whole statement as ONE launch of the grouped fused statement kernel, whatever n_per: particle
 *                       i = g n_per + j starts from bias row g (`bias` dev [M, 4H]); c0 != NULL (dev [M, H]): every particle of
 *                       group g has the previous state (h_g, c_g) - h_g W_hh^T is part of bias row g, the cell reads c0[g] and
 *                       (h, c) dev [M n_per, H] are only written; c0 == NULL: (h, c) hold every particle's own previous state and
 *                       are updated in place. prev_value dev [M n_per] (the previous statement's draws), prior dev [2]
 *                       (prior_stride 0) or [M n_per, 2] (prior_stride 1: a prior that depends on an earlier draw), prior_kind 0
 *                       Normal / 1 Uniform; value[i] = the draw (Philox counter offset + i, key and stream of pp_is_step: an M-group
 *                       call consumes exactly the counters of M one-group calls at offset + g n_per), lw[i] += log p(v) - log q(v)
 *                       as pp_is_statement_rows does. y_out: NULL or dev [M n_per, ldy], a copy of the head outputs. PP_EINVAL
 *                       without a launch when the network has no fused statement kernel for the address (H = 1024, depth > 1, heads
 *                       wider than 32 outputs) or the head is not a Normal / Uniform mixture head. The workspace is
 *                       pp_is_batch_workspace_bytes(n_groups): the fragment images of W_hh, W1, W2 are written there per call. */
int pp_is_batch_bias(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n_groups,
                     int32_t ws_groups, int32_t first_group, const float* h_prev /*dev [M, H] or NULL*/,
                     float* bias_out /*dev [M, 4H]*/, void* workspace, size_t workspace_bytes, void* stream);
int pp_is_statement_groups(const pp_net* net, const float* params, int32_t addr_id, int32_t prev_addr_id, int32_t n_groups,
                           int32_t n_per, const float* bias /*dev [M, 4H]*/, const float* c0 /*dev [M, H] or NULL*/,
                           const float* prev_value /*dev [M n_per]*/, const float* prior, int32_t prior_stride, float* h, float* c,
                           float* value /*dev [M n_per]*/, float* lw /*dev [M n_per]*/, int32_t prior_kind, uint64_t seed, uint64_t offset,
                           float* y_out /*dev [M n_per, ldy] or NULL*/, int64_t ldy, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Resampling the particles of a lock-step posterior call on the device. The reference normalises the weights of an Empirical on
 * the host (finalize, pyprob/distributions/empirical.py:298-309), draws one index per call from a Categorical over them (sample,
 * pyprob/distributions/empirical.py:392-408) and resamples by one such call per drawn value (resample,
 * pyprob/distributions/empirical.py:617-637). Both entry points take the [M n_per] layout of a batched call; a single posterior is
 * M = 1.
 *   pp_is_cdf_groups    cdf_out[g n_per + i] = sum over particles 0..i of group g of w = exp((double)lw - max_g) in fp64 (finalize's
 *                       weights, :298-309, before the division by their sum); w = 0 where lw is not finite (-inf, +inf, NaN: the
 *                       particles pp_is_stats does not count). max_g = stats[6 g] when `stats` (dev double [M, 6], what pp_is_stats
 *                       or pp_is_fused_groups reduced) is given, else a first launch finds the maximum of the finite log-weights;
 *                       both give the same bits. Dependent launches on the caller's stream: a workgroup of 256 threads scans one
 *                       tile of PP_IS_CDF_TILE particles of one group, eight consecutive particles per thread; one workgroup per
 *                       group turns the tile totals into exclusive offsets in index order; the offsets are added in place (groups
 *                       of one tile: the first launch only). Inside a tile the running sum is carried forward from lane to lane
 *                       (wave shuffles of doubles) and through the four waves in LDS, every offset being the rounded value the
 *                       particle before it received: the cdf never decreases and is flat exactly across a particle of weight 0.
 *                       The order of the additions depends on n_per alone: group g of an M-group call equals the one-group call on
 *                       the same particles bit for bit, and so do two identical calls. No workgroup waits for another inside a
 *                       kernel, no atomics. Any n_per >= 1 and n_groups >= 0 (0: returns 0 without a launch; more than 65535 groups
 *                       are split over launches); nothing is written outside cdf_out[0 .. M n_per) and the workspace
 *                       (pp_is_cdf_workspace_bytes; PP_ENOSPACE when shorter).
 *   pp_is_resample_groups  n_out multinomial draws per group in ONE launch (one thread per draw, at most 2048 workgroups): draw j of
 *                       group g takes the Philox4x32-10 block with key `seed`, counter offset + g n_out + j and stream id 0x52, forms
 *                       the 53-bit uniform u = (((uint64)(word0 >> 5) << 26) + (word1 >> 6) + 0.5) 2^-53 and, with base = (lo > 0 ?
 *                       cdf[g, lo - 1] : 0) and total = cdf[g, hi - 1] - base, the target fl(base + fl(u total)) (two separately
 *                       rounded operations). index = lo + the number of i in [lo, hi) with cdf[g, i] <= target, by binary search, at
 *                       most hi - 1: numpy.searchsorted(cdf_g, target, side='right'). A particle of weight 0 inside the range is not
 *                       selected (but for a target that rounds up to the range's last cdf value, probability 2^-52 per draw, which
 *                       takes particle hi - 1 whatever its weight). index_out[g n_out + j] = that index within the group,
 *                       value_out[g n_out + j] = values[g n_per + index]; either may be NULL, not both; value_out needs `values`.
 *                       A group whose total is not positive and finite gets index -1 and value NaN, and none of its elements is
 *                       read beyond the two that form the total. lo / hi (0 <= lo < hi <= n_per: min_index / max_index of
 *                       Empirical.sample and resample) are shared by the groups. An M-group call consumes the counters of the M
 *                       one-group calls at offset + g n_out.
 * Both return PP_EINVAL without a launch for a NULL required pointer, n_per < 1, n_groups < 0, n_out < 0, lo / hi outside
 * 0 <= lo < hi <= n_per, or M n_per / M n_out above 2^31 - 1. */
#define PP_IS_CDF_TILE 2048
size_t pp_is_cdf_workspace_bytes(int32_t n_groups, int32_t n_per);
int pp_is_cdf_groups(const float* lw /*dev [M n_per]*/, int32_t n_groups, int32_t n_per,
                     const double* stats /*dev double [M, 6] or NULL*/, double* cdf_out /*dev double [M n_per]*/, void* workspace,
                     size_t workspace_bytes, void* stream);
int pp_is_resample_groups(const double* cdf /*dev [M n_per]*/, const float* values /*dev [M n_per] or NULL*/, int32_t n_groups,
                          int32_t n_per, int32_t lo, int32_t hi, int32_t n_out, uint64_t seed, uint64_t offset,
                          int64_t* index_out /*dev [M n_out] or NULL*/, float* value_out /*dev [M n_out] or NULL*/, void* stream);

/* Low-variance resampling. The reference's resample is sample() repeated (pyprob/distributions/empirical.py:617-637): multinomial
 * only. pp_is_resample_scheme_groups takes pp_is_resample_groups' arguments with a `scheme` in front of `seed`, in the same single
 * launch (one thread per draw):
 *   PP_RESAMPLE_MULTINOMIAL  pp_is_resample_groups itself: the same kernel, the same bits.
 *   PP_RESAMPLE_STRATIFIED   draw j of group g sits at position p = min(fl(fl((double)j + u) / (double)n_out), 1 - 2^-53) of the
 *                            group's mass, u the 53-bit uniform above of the block at counter offset + g n_out + j, stream id 0x52;
 *                            target = fl(base + fl(p total)); the index, the value and the rule for a group whose total is not
 *                            positive and finite (index -1, value NaN) are those of pp_is_resample_groups.
 *   PP_RESAMPLE_SYSTEMATIC   the same with ONE u per group: the block at counter offset + g, stream id 0x53.
 * With both new schemes p does not decrease in j, so the indices of a group never decrease in j. Every output is a function of the
 * inputs alone; group g of an M-group call equals the one-group call on its slice at offset + g n_out (stratified, multinomial) or
 * offset + g (systematic). PP_EINVAL without a launch for any other scheme and for what pp_is_resample_groups rejects. */
#define PP_RESAMPLE_MULTINOMIAL 0
#define PP_RESAMPLE_STRATIFIED 1
#define PP_RESAMPLE_SYSTEMATIC 2
int pp_is_resample_scheme_groups(const double* cdf /*dev [M n_per]*/, const float* values /*dev [M n_per] or NULL*/,
                                 int32_t n_groups, int32_t n_per, int32_t lo, int32_t hi, int32_t n_out, int32_t scheme,
                                 uint64_t seed, uint64_t offset, int64_t* index_out /*dev [M n_out] or NULL*/,
                                 float* value_out /*dev [M n_out] or NULL*/, void* stream);

/* Joint weighted moments of up to PP_IS_MOMENTS_MAX_COLS latent columns of a lock-step posterior call on the device. The reference
 * normalises the weights on the host (finalize, pyprob/distributions/empirical.py:298-309) and answers mean / variance as
 * expectations over the values of ONE mapped Empirical at a time (expectation :451-466, mean / variance :668-690); here the
 * moments of all requested latents of one weighted particle set, and of all M groups of a batched call, come from one call.
 *   pp_is_moments_groups  row g of `out` (PP_IS_MOMENTS_WIDTH(J) doubles) holds, in this order,
 *                           max lw, W = sum w, sum w^2, count of finite lw
 *                           c_j                                       (J values)
 *                           S_j  = sum w (x_j - c_j)                  (J values)
 *                           Q_jk = sum w (x_j - c_j)(x_k - c_k)       for j <= k, row-major upper triangle
 *                       over the n_per particles of group g, with x_j = cols[j] (a HOST array of J device pointers, each to
 *                       [M n_per] floats). w = exp((double)lw - max_g) in fp64. max_g = stats[6 g] when `stats` (dev double [M, 6],
 *                       what pp_is_stats or pp_is_fused_groups reduced) is given, else a first launch finds the maximum of the
 *                       finite log-weights (-inf where there is none); both give the same bits. A particle whose lw is not finite
 *                       (-inf, +inf, NaN: the particles pp_is_stats does not count) is SKIPPED entirely: its column values enter
 *                       no product, so 0 * NaN never reaches a sum (a lock-step run leaves arbitrary values in the rows of
 *                       particles that did not execute a statement). A non-finite value under a finite weight propagates, as in
 *                       pp_is_stats. The pivot c_j is x_j[g, 0] if that is finite, else 0; the caller forms
 *                       mean_j = c_j + S_j / W and cov_jk = Q_jk / W - (S_j / W)(S_k / W), the biased, weight-normalised form of
 *                       Empirical.variance. Sums about a pivot keep a narrow posterior far from zero accurate; raw second moments
 *                       cancel there. A group without a finite log-weight gives count 0 and sums 0.
 *                       Dependent launches on the caller's stream: a workgroup of 256 threads takes one tile of 2048 particles of
 *                       one group and one pair of 4-column blocks (eight particles per thread, 23 fp64 accumulators; the lanes
 *                       of a wave exchange doubles by DPP, the four waves meet in LDS) and STORES its partial sums in the workspace; one workgroup per
 *                       group adds them in tile order. No atomics, no workgroup waits for another. The order of the additions
 *                       depends on n_per and n_cols alone: group g of an M-group call equals the one-group call on the same
 *                       particles bit for bit, and so do two identical calls. Any n_per >= 1 and n_groups >= 0 (0: returns 0
 *                       without a launch; more than 65535 groups are split over launches); nothing is written outside
 *                       out[0 .. M PP_IS_MOMENTS_WIDTH(J)) and the workspace (pp_is_moments_workspace_bytes; PP_ENOSPACE when
 *                       shorter).
 * Returns PP_EINVAL without a launch for a NULL required pointer (lw, cols, any cols[j], out, workspace), n_cols outside
 * 1 .. PP_IS_MOMENTS_MAX_COLS, n_per < 1, n_groups < 0 or M n_per above 2^31 - 1. pp_is_moments_workspace_bytes returns 0 for
 * arguments outside that envelope. */
#define PP_IS_MOMENTS_MAX_COLS 16
#define PP_IS_MOMENTS_WIDTH(J) (4 + 2 * (J) + (J) * ((J) + 1) / 2)
size_t pp_is_moments_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_cols);
int pp_is_moments_groups(const float* lw /*dev [M n_per]*/, const float* const* cols /*host array of J dev pointers, each [M n_per]*/,
                         int32_t n_cols, int32_t n_groups, int32_t n_per, const double* stats /*dev double [M, 6] or NULL*/,
                         double* out /*dev double [M, PP_IS_MOMENTS_WIDTH(J)]*/, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Weighted histograms of one latent (1-D) or a pair of latents (2-D) of a lock-step posterior call on the device, and the extent
 * of a latent. The reference normalises the weights on the host (finalize, pyprob/distributions/empirical.py:298-309) and draws
 * its histogram from all values and weights on the host (plot_histogram, pyprob/distributions/empirical.py:889-914); here the M
 * groups of a batched call are binned by one call and only the rows of bins travel.
 *   pp_is_hist_groups   row g of `out` is [2][slots] 64-bit integers: out[g][0][s] the fixed-point mass of slot s, out[g][1][s] the
 *                       number of particles in it, over the n_per particles of group g.
 *                       WEIGHTS. w = exp((double)lw - max_g) in fp64; max_g = stats[6 g] when `stats` (dev double [M, 6], what
 *                       pp_is_stats or pp_is_fused_groups reduced) is given, else a first launch finds the maximum of the finite
 *                       log-weights; both give the same bits. A particle whose lw is not finite (-inf, +inf, NaN) is SKIPPED
 *                       entirely: it is in no slot and no count, and its x / y (rows a diverged path never wrote) are not
 *                       interpreted. No finite log-weight in the group: the row is all zero.
 *                       FIXED POINT. A particle adds q = llrint(min(w, 1) 2^S) to its slot and 1 to the slot's count, with
 *                       S = pp_is_hist_shift(n_per) = 62 - ceil(log2(n_per)): a group's total is at most n_per 2^S <= 2^62 and
 *                       cannot overflow (w <= 1 whenever max_g is the maximum; the clamp keeps the guarantee under a wrong `stats`).
 *                       Integer sums do not depend on the order of the additions: two identical calls give the same bits, group
 *                       g of an M-group call equals the one-group call on its slice, and so would any other tiling. The caller
 *                       forms the posterior mass of a slot as slot / total, total = the exact integer sum of all slots of the row.
 *                       Derived bound: |slot - sum_i w_i 2^S| <= 0.5 count + 2^-48 sum_i w_i 2^S (half a unit of rounding per
 *                       particle, 16 fp64 ulp for the device exp); S = 42 at n_per = 10^6.
 *                       BINS. edges_x holds bins_x + 1 strictly increasing finite doubles - the caller guarantees it; this layer
 *                       cannot check device memory without a launch and does not. edges_x_stride = 0: one array shared by the
 *                       groups, else group g reads edges_x + g edges_x_stride (stride >= bins_x + 1). In fp64, bin b holds
 *                       e_b <= x < e_{b+1} and the last bin also x == e_bins: numpy.searchsorted(edges, x, 'right') - 1 with
 *                       numpy.histogram's right-edge rule, by binary search over the edges staged in LDS (uniform or not).
 *                       1-D (y, edges_y NULL; bins_y = 1): slots = bins_x + 3 = [bins ..., below (x < e_0, -inf), above
 *                       (x > e_last, +inf), x is NaN]. 2-D: slots = bins_x bins_y + 2 = [bin ix bins_y + iy ..., outside (no
 *                       coordinate NaN, either out of its range), either coordinate NaN].
 *                       Dependent launches on the caller's stream: a workgroup of 256 threads bins one tile of one group (2048
 *                       particles up to 256 bins, 8192 above) into an LDS histogram (64-bit mass and 32-bit count by integer LDS
 *                       adds; with the edges about 41 KB at 2048 bins) and STORES its partial row in the workspace; a second launch
 *                       adds the partial rows of every group, one thread per slot (a group of one tile stores its row in `out`
 *                       directly). No global atomics, no workgroup waits for another.
 *   pp_is_extent_groups out[g] = { min x, max x, particles counted, particles whose x is NaN }: the exact fp32 minimum and maximum,
 *                       widened to double, over the particles of group g with a finite lw and a non-NaN x (+-inf count), the
 *                       number of those, and the number of particles with a finite lw whose x is NaN. Nothing counted:
 *                       +inf, -inf, 0, k. Minima, maxima and integer counts do not depend on the order: the identities above hold.
 * Both take any n_per >= 1 and n_groups >= 0 (0: return 0 without a launch; more than 65535 groups are split over launches) and
 * write nothing outside `out` and the workspace (pp_is_hist_workspace_bytes / pp_is_extent_workspace_bytes; PP_ENOSPACE when
 * shorter). Both return PP_EINVAL without a launch for a NULL required pointer (lw, x, edges_x, out, workspace), n_per < 1,
 * n_groups < 0, M n_per above 2^31 - 1, bins_x < 1, bins_y < 1, bins_x bins_y > PP_IS_HIST_MAX_BINS, y without edges_y or edges_y
 * without y (1-D: bins_y must be 1), or a stride that is neither 0 nor at least bins + 1. The workspace functions return 0 outside
 * that envelope. pp_is_hist_shift returns -1 for n_per < 1. */
#define PP_IS_HIST_MAX_BINS 2048          /* bins_x * bins_y (bins_y = 1 for 1-D) */
int32_t pp_is_hist_shift(int32_t n_per);  /* S = 62 - ceil(log2(n_per)), 62 for n_per = 1; -1 for n_per < 1 */
size_t pp_is_hist_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t bins_x, int32_t bins_y);
int pp_is_hist_groups(const float* lw /*dev [M n_per]*/, const float* x /*dev [M n_per]*/, const float* y /*dev [M n_per] or NULL = 1-D*/,
                      int32_t n_groups, int32_t n_per,
                      const double* edges_x /*dev*/, int32_t bins_x, int64_t edges_x_stride /*0 = shared by the groups, else >= bins_x + 1*/,
                      const double* edges_y /*dev or NULL*/, int32_t bins_y, int64_t edges_y_stride,
                      const double* stats /*dev double [M, 6] or NULL*/, int64_t* out /*dev [M, 2, slots]*/,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t pp_is_extent_workspace_bytes(int32_t n_groups, int32_t n_per);
int pp_is_extent_groups(const float* lw, const float* x, int32_t n_groups, int32_t n_per,
                        double* out /*dev [M, 4]: min x, max x, particles counted, particles whose x is NaN*/,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Order statistics of one latent of a lock-step posterior call on the device: the particles of every group in order of value,
 * exact weighted quantiles over them, and the distinct values with their masses. The reference estimates a weighted median from
 * 1000 resampled values on the host (median, pyprob/distributions/empirical.py:714-728) and combines duplicates by one host pass
 * over all values per distinct value (combine_duplicates, pyprob/distributions/empirical.py:809-834); here the M groups of a
 * batched call are sorted by one call and only the answers travel.
 *   pp_is_sort_groups   KEY. Particle i of group g gets the 32-bit key 0xFFFFFFFF if lw is not finite (-inf, +inf, NaN) or x is
 *                       NaN; else, with b the bits of x and -0.0 first made +0.0, ~b for a negative x and b | 0x80000000
 *                       otherwise - unsigned order of the keys is numeric order of the values, and +-inf under a finite weight
 *                       are ordinary keys at the two ends.
 *                       OUTPUTS. The STABLE ascending sort of the n_per particles of the group by that key (ties keep particle
 *                       order, so the permutation is unique): index_out[g n_per + k] = the index within the group of the k-th
 *                       particle, value_out[..] = x[index] (the original bits), lw_out[..] = lw[index]; counted_out[g] =
 *                       { c_g = particles with a key below 0xFFFFFFFF, particles with a finite lw whose x is NaN }. The first
 *                       c_g sorted particles are the counted ones; the others follow in particle order.
 *                       `stats` (dev double [M, 6] or NULL) is accepted for symmetry with the calls below: the keys do not
 *                       depend on the weights' maximum, so the outputs carry the same bits with and without it.
 *                       Dependent launches on the caller's stream, a least-significant-digit radix sort with 8-bit digits: a
 *                       group of at most PP_IS_SORT_TILE particles is sorted by one workgroup of 256 threads in LDS (33 KB) in
 *                       one launch; a longer group takes three launches per pass - per-tile digit counts, one workgroup per group
 *                       that turns the (tile, digit) counts into offsets, and a scatter with in-tile stable ranks (wave ballots)
 *                       between two buffers of the workspace (16 bytes per particle). No global atomics, no workgroup waits for
 *                       another. Every output is a function of the keys alone: two identical calls give the same bits and
 *                       group g of an M-group call equals the one-group call on its slice.
 *   cumulative weights  pp_is_cdf_groups over lw_out (same `stats`) gives the cumulative weights in sorted order; the particles
 *                       that are not counted lie at or beyond c_g and are never read below.
 *   pp_is_quantile_groups  out[g n_q + j] = the inverted-cdf quantile q[j] (dev double [n_q] in [0, 1], shared by the groups) of
 *                       group g, one thread per result, by binary search: T = cdf[g, c_g - 1], t = fl(q T); t > 0: k = the
 *                       number of i < c_g with cdf[g, i] < t (numpy.searchsorted(cdf[:c_g], t, 'left')); else k = the number
 *                       of i < c_g with cdf[g, i] <= 0 (the first particle of positive cumulative weight); k is at most
 *                       c_g - 1; the result is (double)value_sorted[g, k]. c_g == 0 or a T that is not positive and finite: NaN.
 *                       With uniform weights and q = 0.5 this is the lower of the two middle values.
 *   pp_is_unique_groups  A run is a maximal stretch of the first c_g sorted particles with equal keys. For run r of group g:
 *                       value_out[g n_per + r] = the value of its first particle, count_out[..] = its particles, mass_out[..] =
 *                       sum llrint(min(w, 1) 2^S), w = exp((double)lw - max_g), S = pp_is_hist_shift(n_per) - the fixed point
 *                       of pp_is_hist_groups with its order-independence and its derived bound |mass - sum w 2^S| <= 0.5 count
 *                       + 2^-48 sum w 2^S; max_g = stats[6 g] or, without `stats`, the maximum of the finite lw_sorted of the
 *                       whole group (both give the same bits). runs_out[g] = the number of runs; entries at or beyond it are
 *                       not written. Dependent launches: the runs that begin in every tile of PP_IS_SORT_TILE particles are
 *                       counted, one workgroup per group numbers them, a tile adds up its runs in LDS (integer adds) and a last
 *                       launch adds to a run that crosses tiles the parts the following tiles hold of it (one thread per run:
 *                       no global atomics).
 * All three take the [M n_per] layout, any n_per >= 1 and n_groups >= 0 (0: return 0 without a launch; more than 65535 groups are
 * split over launches), and write nothing outside their outputs and the workspace (pp_is_sort_workspace_bytes /
 * pp_is_unique_workspace_bytes; PP_ENOSPACE when shorter). They return PP_EINVAL without a launch for a NULL required pointer
 * (everything but `stats`), n_per < 1, n_groups < 0, n_q < 0, or M n_per / M n_q above 2^31 - 1. The workspace functions return 0
 * outside that envelope. */
#define PP_IS_SORT_TILE 2048
size_t pp_is_sort_workspace_bytes(int32_t n_groups, int32_t n_per);
int pp_is_sort_groups(const float* lw /*dev [M n_per]*/, const float* x /*dev [M n_per]*/, int32_t n_groups, int32_t n_per,
                      const double* stats /*dev double [M, 6] or NULL*/, float* value_out /*dev [M n_per]*/,
                      float* lw_out /*dev [M n_per]*/, int32_t* index_out /*dev [M n_per]*/, int32_t* counted_out /*dev [M, 2]*/,
                      void* workspace, size_t workspace_bytes, void* stream);
int pp_is_quantile_groups(const float* value_sorted /*dev [M n_per]*/, const double* cdf_sorted /*dev [M n_per]*/,
                          const int32_t* counted /*dev [M, 2]*/, int32_t n_groups, int32_t n_per, const double* q /*dev [n_q]*/,
                          int32_t n_q, double* out /*dev [M, n_q]*/, void* stream);
size_t pp_is_unique_workspace_bytes(int32_t n_groups, int32_t n_per);
int pp_is_unique_groups(const float* value_sorted /*dev [M n_per]*/, const float* lw_sorted /*dev [M n_per]*/,
                        const int32_t* counted /*dev [M, 2]*/, int32_t n_groups, int32_t n_per,
                        const double* stats /*dev double [M, 6] or NULL*/, float* value_out /*dev [M n_per]*/,
                        int64_t* mass_out /*dev [M n_per]*/, int32_t* count_out /*dev [M n_per]*/, int32_t* runs_out /*dev [M]*/,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The highest-posterior-density interval and the cdf at a point of one latent of a lock-step posterior call on the device. The
 * reference has neither an HPD interval nor a cdf: its Empirical answers moments, mode, min / max and a median of 1000 resampled
 * values (pyprob/distributions/empirical.py:668-728). Both calls take pp_is_sort_groups' value_out and counted_out and
 * pp_is_cdf_groups over its lw_out - what pp_is_quantile_groups takes. For group g let c = counted[g, 0], v and cdf its sorted values
 * and cumulative weights, T = cdf[c - 1].
 *   pp_is_hpd_groups    For level L = level[l] (dev double [n_l], shared by the groups): c == 0, a T that is not positive and
 *                       finite, or an L that is NaN or outside (0, 1]: out[g, l] = (NaN, NaN), index_out[g, l] = (-1, -1). Else
 *                       m = fl(L T); a start i < c is VALID when cdf[i] > prev_i (prev_i = i > 0 ? cdf[i - 1] : 0: the particle has
 *                       positive weight) and t_i = fl(prev_i + m) <= T; its end is j_i = max(i, #{k < c : cdf[k] < t_i}), that is
 *                       numpy.searchsorted(cdf[:c], t_i, 'left') clamped from below; its width (double)v[j_i] - (double)v[i], a NaN
 *                       width (inf - inf) counting as +inf. The result is the valid start of smallest width, ties to the smallest
 *                       i: out[g, l] = ((double)v[i], (double)v[j_i]), index_out[g, l] = (i, j_i), positions in sorted order
 *                       (index_out may be NULL). The first particle of positive weight is always valid, fl(L T) <= T.
 *                       One thread per start, eight independent binary searches per thread in flight; a workgroup of 256 threads
 *                       reduces the PP_IS_HPD_TILE starts of its tile to one (width, i, j) by wave shuffles and LDS. A group of one
 *                       tile is finished by that launch; a longer one stores a record of 16 bytes per (level, tile) in the
 *                       workspace and a second launch reduces them in tile order, one workgroup per (group, level).
 *   pp_is_ecdf_groups   For point x[g, q] (dev double [M, n_x]: PER GROUP): k = #{i < c : (double)v[i] <= x} (strict != 0: < x) by
 *                       binary search, one thread per result; rank_out[g, q] = k (may be NULL), out[g, q] = k == 0 ? 0.0 :
 *                       fl(cdf[k - 1] / T). A NaN x, c == 0 or a T that is not positive and finite: out NaN, rank -1.
 * Both take the [M n_per] layout, any n_per >= 1 and n_groups >= 0 (0: return 0 without a launch; more than 65535 groups are split
 * over launches), write nothing outside their outputs and the workspace (pp_is_hpd_workspace_bytes; PP_ENOSPACE when shorter) and
 * are dependent launches on the caller's stream: no global atomics, no workgroup waits for another. Every output is a function of
 * the inputs alone: two calls give the same bits, and group g of an M-group call equals the one-group call on its slice. PP_EINVAL
 * without a launch for a NULL required pointer (everything but index_out / rank_out), n_per < 1, n_groups < 0, n_l < 0, n_x < 0, or
 * M n_per, 2 M n_l or M n_x above 2^31 - 1. pp_is_hpd_workspace_bytes returns 0 outside that envelope. */
#define PP_IS_HPD_TILE 2048
size_t pp_is_hpd_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_l);
int pp_is_hpd_groups(const float* value_sorted /*dev [M n_per]*/, const double* cdf_sorted /*dev [M n_per]*/,
                     const int32_t* counted /*dev [M, 2]*/, int32_t n_groups, int32_t n_per, const double* level /*dev [n_l]*/,
                     int32_t n_l, double* out /*dev [M, n_l, 2]*/, int32_t* index_out /*dev [M, n_l, 2] or NULL*/, void* workspace,
                     size_t workspace_bytes, void* stream);
int pp_is_ecdf_groups(const float* value_sorted /*dev [M n_per]*/, const double* cdf_sorted /*dev [M n_per]*/,
                      const int32_t* counted /*dev [M, 2]*/, int32_t n_groups, int32_t n_per, const double* x /*dev [M, n_x]*/,
                      int32_t n_x, int32_t strict, double* out /*dev [M, n_x]*/, int32_t* rank_out /*dev [M, n_x] or NULL*/,
                      void* stream);

/* Pareto-smoothed importance weights and the k-hat diagnostic of a lock-step posterior call on the device (PSIS: Vehtari, Simpson,
 * Gelman, Yao, Gabry, JMLR 2024). The reference has no counterpart: the only reliability figure of its Empirical is
 * effective_sample_size (pyprob/distributions/empirical.py:758-766), which looks healthy exactly when the proposal misses a heavy tail.
 * INPUTS per group g of the [M n_per] layout: the outputs of pp_is_sort_groups called with x = lw - a sort keyed on the log-weight
 * itself, so particles with a non-finite lw have key 0xFFFFFFFF and lie last: lw_sorted, index_sorted and counted. Let
 * c = counted[g, 0], s[0..c-1] the sorted finite log-weights as doubles, M_g = s[c-1] (`stats`, dev double [M, 6] or NULL, is
 * accepted for symmetry: stats[6 g] has the same bits, M_g is the maximum either way).
 *   tail length     n_t = tail if tail > 0, else (int)ceil(fmin(c / 5.0, 3.0 * sqrt((double)c))).
 *   cutoff          b = c - n_t - 1. NO FIT (A) if c == 0 or b < 0.
 *   first tail position  f = #{i < c : s[i] <= s[b]} (ties with the cutoff are not in the tail); n = c - f; u = exp(s[b] - M_g).
 *   exceedances     y_r = exp(s[f + r] - M_g) - u for r < n (ascending). NO FIT (B) if n <= 4 or not (y_0 > 0).
 *   no fit          k-hat = +inf, sigma = NaN, and every log-weight of the group leaves with the bits it came with.
 *   grid            m = 30 + floor(sqrt(n)), q = y[(int)(n / 4.0 + 0.5) - 1]; for j = 1..m:
 *                   theta_j = 1 / y_{n-1} + (1 - sqrt(m / (j - 0.5))) / (3 q), kappa_j = (1/n) sum_r log1p(-theta_j y_r),
 *                   L_j = n (log(-theta_j / kappa_j) - kappa_j - 1).
 *   weights         omega_j = 1 / sum_l exp(L_l - L_j) (a sum that overflows: omega_j = 0); theta-hat = sum_j omega_j theta_j;
 *                   kappa = (1/n) sum_r log1p(-theta-hat y_r); sigma = -kappa / theta-hat; k-hat = (n kappa + 5) / (n + 10) (the
 *                   paper's weak prior: ten pseudo-observations at 0.5).
 *   smoothing       only where k-hat is finite. For tail rank r (sorted order, ties in particle order: the sort is stable):
 *                   p_r = (r + 0.5) / n, w_r = u + sigma expm1(-k-hat log1p(-p_r)) / k-hat (k-hat == 0: u - sigma log1p(-p_r)),
 *                   lw_out[g, index_sorted[f + r]] = (float)(fmin(log(w_r), 0.0) + M_g). Every other particle of the group gets
 *                   its input bits: non-tail particles, non-finite ones, NaN payloads. A k-hat that comes out NaN is reported as
 *                   such and the weights stay unchanged.
 *   out             row g, PP_IS_PSIS_WIDTH doubles: k-hat, sigma, n, m, f, s[b] (the cutoff log-weight), c, M_g. Without a
 *                   fit m = 0; under (A) n = f = 0 and s[b] = NaN; M_g = NaN where c == 0.
 * lw_out (float [M n_per], particle order) may be NULL: a diagnostic-only call that skips the smoothing launch and writes the
 * same `out` bits. Four dependent launches on the caller's stream: one thread per tail rank stores y (one fp64 exp) in the
 * workspace; one WAVE per (group, grid point) adds log1p(-theta_j y_r) - lane l over r = l, l + 64, ... in index order with a
 * compensated sum, the lane sums by a fixed butterfly; one workgroup per group turns L into omega and theta-hat and passes once
 * over y; one thread per sorted position scatters the smoothed or copied log-weight. No global atomics, no workgroup waits for
 * another, nothing is written outside the outputs and the workspace (pp_is_psis_workspace_bytes; PP_ENOSPACE when shorter). Every
 * sum's order is a function of n and m alone: two calls give the same bits, group g of an M-group call equals the one-group call
 * on its slice. Any n_per >= 1 and n_groups >= 0 (0: return 0 without a launch; more than 65535 groups are split over launches).
 * PP_EINVAL without a launch for a NULL required pointer (everything but `stats` and lw_out), n_per < 1, n_groups < 0, tail < 0 or
 * M n_per above 2^31 - 1. pp_is_psis_workspace_bytes returns 0 outside that envelope. */
#define PP_IS_PSIS_WIDTH 8
size_t pp_is_psis_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t tail);
int pp_is_psis_groups(const float* lw_sorted /*dev [M n_per]*/, const int32_t* index_sorted /*dev [M n_per]*/,
                      const int32_t* counted /*dev [M, 2]*/, int32_t n_groups, int32_t n_per,
                      const double* stats /*dev double [M, 6] or NULL*/, int32_t tail, float* lw_out /*dev [M n_per] or NULL*/,
                      double* out /*dev [M, PP_IS_PSIS_WIDTH]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Weighted Gaussian-mixture EM over one latent of a lock-step posterior call on the device. The reference's density_estimate
 * (pyprob/distributions/empirical.py:795-807) resamples 1000 values on the host, drops the weights and fits scikit-learn's
 * GaussianMixture(covariance_type='diag') to them; here the EM of that class runs in one dimension over ALL particles of each of
 * the M groups under their own weights, in fp64 (only x and lw are float32), from the caller's initial parameters.
 *   pp_is_gmm_groups    w_i = exp((double)lw_i - max_g) for the particles with a finite lw (max_g = stats[6 g] or, without `stats`,
 *                       the largest finite lw of the group: the same bits either way); every other particle is skipped - its value
 *                       is read but enters nothing. W = sum w_i. With pi_k, mu_k, v_k (k < K) the current weights, means and
 *                       variances of the group - at first params_init[g] = pi | mu | v - iteration t = 1 .. max_iter is
 *                         E-step  l_ik = log pi_k - 1/2 log(2 pi v_k) - (x_i - mu_k)^2 / (2 v_k),  L_i = logsumexp_k l_ik,
 *                                 r_ik = w_i exp(l_ik - L_i),  lb_t = sum_i w_i L_i / W
 *                         M-step  N_k = sum_i r_ik + 10 DBL_EPSILON,  d_k = sum_i r_ik (x_i - mu_k) / N_k,  mu'_k = mu_k + d_k,
 *                                 v'_k = max(sum_i r_ik (x_i - mu_k)^2 / N_k - d_k^2, 0) + reg_covar,  pi'_k = N_k / sum_k N_k
 *                         stop    |lb_t - lb_{t-1}| < tol (lb_0 = -inf): the group is converged, n_iter = t and the parameters are
 *                                 those AFTER this M-step, as in scikit-learn; tol = 0 runs exactly max_iter iterations.
 *                       The M-step's sums are taken about the current mean as pivot, so a narrow posterior far from zero keeps its
 *                       variance. Row g of `out` (PP_IS_GMM_WIDTH(K) doubles): pi [K] | mu [K] | v [K] | the last lower bound,
 *                       n_iter, converged (0 / 1), W, the count of finite lw, max_g. A group without a finite lw: NaN parameters
 *                       and lower bound, n_iter 0, converged 1, W 0, count 0, max_g -inf. A NaN value under a finite lw makes the
 *                       lower bound NaN: the group never converges and leaves NaN parameters after max_iter iterations.
 *                       Two dependent launches per iteration on the caller's stream (a workgroup per tile of 2048 particles stores a
 *                       partial row of 3 K + 3 sums, a workgroup per group adds them in tile order and updates its row of `out`);
 *                       no atomics, no workgroup waits for another. A converged group is frozen: its workgroups return at entry.
 *                       Every check_every iterations (< 1: 8) the host reads one word that says whether all groups converged and
 *                       stops enqueuing: this call SYNCHRONISES the stream there. The sums' order is a function of n_per and K
 *                       alone: the result of a group does not depend on check_every, on M or on the other groups of the call, and
 *                       a call repeated gives the same bits.
 * Any n_per >= 1 and n_groups >= 0 (0: return 0 without a launch); nothing is written outside `out` and the workspace
 * (pp_is_gmm_workspace_bytes; PP_ENOSPACE when shorter). PP_EINVAL without a launch for a NULL required pointer (lw, x, params_init,
 * out, workspace), n_components outside 1 .. PP_IS_GMM_MAX_K, n_per < 1, n_groups < 0, M n_per above 2^31 - 1, max_iter < 1, tol < 0
 * or reg_covar < 0 (NaN included). pp_is_gmm_workspace_bytes returns 0 outside that envelope. */
#define PP_IS_GMM_MAX_K 16
#define PP_IS_GMM_WIDTH(K) (3 * (K) + 6)
size_t pp_is_gmm_workspace_bytes(int32_t n_groups, int32_t n_per, int32_t n_components);
int pp_is_gmm_groups(const float* lw /*dev [M n_per]*/, const float* x /*dev [M n_per]*/, int32_t n_components, int32_t n_groups,
                     int32_t n_per, const double* stats /*dev double [M, 6] or NULL*/,
                     const double* params_init /*dev double [M, 3 K]*/, int32_t max_iter, double tol, double reg_covar,
                     int32_t check_every, double* out /*dev double [M, PP_IS_GMM_WIDTH(K)]*/, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Prior draws of vectorised trace generation (the per-trace generator: pyprob/nn/dataset.py:50-62 with state.sample's
 * prior branch pyprob/state.py:278-290): out[i] ~ Normal(p0, p1) (kind 0) | Uniform[p0, p1) (kind 1), parameters shared
 * (stride 0) or per trace (stride 1); Philox4x32-10, counter offset + i, key seed, `stream_id` distinguishes statements. */
int pp_prior_draw(int32_t kind, const float* p0, int32_t p0_stride, const float* p1, int32_t p1_stride, int32_t n, uint64_t seed,
                  uint64_t offset, uint32_t stream_id, float* out /*dev [n]*/, void* stream);

/* Observation blocks of vectorised trace generation (pyprob/nn/dataset.py:50-62 with the observe branch of pyprob/state.py,
 * which draws distribution.sample() for every observe of a PRIOR_FOR_INFERENCE_NETWORK trace): one row of k values per trace,
 *   out[r * k + e] ~ Normal(p0, p1) (kind 0) | Uniform[p0, p1) (kind 1),   r < n, e < k,
 * p0 read at p0[r * p0_row_stride + e * p0_elem_stride], p1 likewise. Strides are element counts: (row, elem) = (0, 0) a scalar,
 * (0, 1) one row shared by all traces (an image), (1, 0) one value per trace, (k, 1) a full [n, k] block; no caller materialises a
 * parameter to [n, k]. Any k >= 1 and any 4-byte aligned `out`; nothing is written outside out[0 .. n * k - 1].
 * Counter scheme (part of the ABI): element group q = e >> 2 of row r takes the Philox4x32-10 block with key `seed` and counter
 * words (lo(offset + r), hi(offset + r), stream_id, q). Uniform element e uses word e & 3 of its group's block with
 * pp_prior_draw's arithmetic (a + (b - a) * (word >> 8) * 2^-24, folded back to a where it rounds up to b). Normal elements
 * 4q and 4q + 1 are the cosine and the sine branch of Box-Muller on words (0, 1), elements 4q + 2 and 4q + 3 the cosine and the
 * sine branch on words (2, 3) (sqrtf / logf / cosf / sinf as in pp_prior_draw). Hence k = 1 is bit-identical to pp_prior_draw,
 * element 0 of any k is pp_prior_draw's value of that row, and a row depends on (seed, offset + r, stream_id) only - not on n,
 * nor on how rows were split into paths or chunks. Returns nonzero without a launch for kind not in {0, 1}, k < 1, n < 0, or a
 * NULL p0 / p1 / out when n > 0; n == 0 returns 0 without a launch. */
int pp_obs_draw(int32_t kind, const float* p0, int64_t p0_row_stride, int32_t p0_elem_stride, const float* p1, int64_t p1_row_stride,
                int32_t p1_elem_stride, int32_t n, int32_t k, uint64_t seed, uint64_t offset, uint32_t stream_id,
                float* out /*dev [n, k] contiguous*/, void* stream);

/* lw[i] += scale * term[i] (e.g. -log q). */
int pp_axpy(float scale, const float* term, float* lw, int32_t n, void* stream);

/* Wavefront-reduced importance statistics over n particles (pyprob/distributions/empirical.py:298-309,
 * 451-466, 758-766): out (dev, double[6]) = { max lw, sum w, sum w^2, sum w*x, sum w*x^2, count finite } with
 * w = exp(lw - max lw) evaluated in fp64. ESS = (sum w)^2 / sum w^2. One pass over the particles (per-workgroup maxima, rescaled by a
 * one-workgroup combine); `scratch` dev >= PP_IS_STATS_SCRATCH doubles. */
#define PP_IS_STATS_SCRATCH 6144
int pp_is_stats(const float* lw, const float* x, int32_t n, double* out, double* scratch, void* stream);

/* (ABI 15) Every distribution family of pyprob v1.5.0 on the device: log-densities and draws for the prior-proposal engine
 * (state.sample's prior branch pyprob/state.py:191-201 and its uncontrolled draws :218-221), the likelihoods of state.observe
 * (:118-155) and pyprob.factor (:113-115, distributions/factor.py). Kinds 0-5 are those of pp_logweight_accumulate; the
 * log-densities are evaluated in fp32 like the torch.distributions classes behind pyprob/distributions/<family>.py:
 *    0 Normal(p0 mean, p1 stddev)                 normal.py
 *    1 Uniform(p0 low, p1 high), support [low, high)        uniform.py
 *    2 Factor: the value x itself (log_prob given)          factor.py
 *    3 Poisson(p0 rate)  4 Bernoulli(p0 probs)              poisson.py, bernoulli.py
 *    5 Categorical: p0 = probs row(s), p_stride[0] = row stride (0 = one shared row), p_stride[1] = C   categorical.py
 *    6 Exponential(p0 rate)                                 exponential.py
 *    7 Gamma(p0 concentration, p1 rate)                     gamma.py
 *    8 Beta(p0 concentration1, p1 concentration0, p2 low, p3 high): torch Beta.log_prob of (x - low) / (high - low),
 *      WITHOUT the -log(high - low) Jacobian, as pyprob's beta.py:38-40 evaluates it
 *    9 LogNormal(p0 loc, p1 scale)                          log_normal.py
 *   10 Weibull(p0 scale, p1 concentration)                  weibull.py
 *   11 Binomial(p0 total_count, p1 logits)                  binomial.py (torch evaluates it from the logits)
 *   12 VonMises(p0 loc, p1 concentration)                   von_mises.py (torch's polynomial log I0)
 *   13 TruncatedNormal(p0 mean, p1 stddev, p2 low, p3 high), closed support: truncated_normal.py:40-45
 * A parameter is a pointer + a stride (0: one shared value, 1: one per particle). A value outside the family's support
 * gives -inf (the particle is then discarded like any non-finite weight, pyprob/model.py:63-65). */
#define PP_DIST_MAX_KIND 13
#define PP_DIST_MAX_TERMS 8
#define PP_DIST_MAX_ROUNDS 64
typedef struct pp_dist {
    int32_t kind;
    int32_t p_stride[4];
    const float* p[4];
} pp_dist;
typedef struct pp_dist_term {
    pp_dist d;
    const float* x; int32_t x_stride;   /* the value scored; x_stride 0 = one shared value (an observation) */
    float scale;                          /* likelihood_importance for an observe (state.py:147-149), 1 for a prior */
} pp_dist_term;

/* The log-weight pass of a lock-step run (state.py:147-149, 211; trace.py:123-125):
 *     lw[r] += sum_t scale_t * log p_t(x_t[r])    for r = rows[j], j < m (rows: dev int64 ascending), or rows NULL: r < n
 * At most PP_DIST_MAX_TERMS terms of any kind in one launch. lw may be NULL; lp_out (dev [n], count == 1 only) receives
 * log p(x[r]) unscaled at r. Rows that are not listed are not touched. */
int pp_dist_logweight(const pp_dist_term* terms, int32_t count, float* lw /*dev [n]*/, float* lp_out, const int64_t* rows,
                      int32_t m, int32_t n, void* stream);

/* Draws of a family: out[r] ~ family(params_r) for r = rows[j], j < m, or rows NULL: r < n (out is full-width, dev [n];
 * other rows are not touched). Philox4x32-10: key = seed, counter = offset + r, stream_id per statement - the counter
 * scheme of pp_prior_draw, so a particle's draw does not depend on how particles were split into paths or shards; kinds
 * 0 / 1 are bit-identical to pp_prior_draw. Rejection samplers (Gamma: Marsaglia-Tsang with the alpha < 1 boost in log
 * space; Beta: G1 / (G1 + G2) in log space; Poisson: multiplication / PTRS; Binomial: inversion / BTRS; VonMises:
 * Best-Fisher; TruncatedNormal: inverse CDF, redrawn when the fp32 value leaves [low, high]) take fresh Philox words per
 * round and stop after PP_DIST_MAX_ROUNDS rounds: such a lane writes NaN. Kind 2 (Factor) has no draw. */
int pp_dist_draw(const pp_dist* d, const int64_t* rows, int32_t m, int32_t n, uint64_t seed, uint64_t offset, uint32_t stream_id,
                 float* out /*dev [n]*/, void* stream);

/* Mixture(distributions, probs) (pyprob/distributions/mixture.py) as a prior or likelihood of a program: K = 1..16 scalar
 * components (kinds 0, 1, 3, 4, 6-13, families may differ; Factor, Categorical and nested mixtures are not components) and K
 * unnormalised weights >= 0, one shared row or one row per particle. */
#define PP_MIX_MAX_COMPONENTS 16
typedef struct pp_mixture {
    int32_t count;            /* K, 1..16 */
    int32_t probs_stride;     /* 0: one shared row of K weights; K: row r at probs + r*K */
    const float* probs;       /* unnormalised, >= 0 */
    pp_dist comp[PP_MIX_MAX_COMPONENTS];
} pp_mixture;

/* Mixture.log_prob (mixture.py:8-16, 38-45; util.clamp_probs) as a log-weight term:
 *     lp[r] = logsumexp_k( log clamp(w[r,k] / sum_k w[r,k], eps, 1 - eps) + log p_k(x[r]) ),  eps = 2^-23
 *     lw[r] += scale * lp[r], lp_out[r] = lp[r]   for r = rows[j], j < m, or rows NULL: r < n (m, n, rows as pp_dist_logweight)
 * The row of weights is summed on the device in index order. -inf when x is outside every component's support; a NaN
 * parameter gives NaN. lw or lp_out may be NULL (not both). */
int pp_mix_logweight(const pp_mixture* mix, const float* x, int32_t x_stride, float scale, float* lw /*dev [n]*/, float* lp_out,
                     const int64_t* rows, int32_t m, int32_t n, void* stream);

/* Mixture.sample (mixture.py:47-63): out[r] ~ component k_r, k_r ~ Categorical(w[r,:]) on the unclamped weights (the rule of
 * pp_dist_draw kind 5: the first k with u * sum < cumulative weight, else K - 1). The selection uniform is the first word of
 * Philox(seed, offset + r, stream_id | 0x80000000); the component's draw uses Philox(seed, offset + r, stream_id) - exactly
 * pp_dist_draw's stream, so a mixture of K = 1 or of K identical components is bit-identical to pp_dist_draw of the family.
 * stream_id must leave the top bit clear. One launch per distinct kind among the components; rows, m, n as pp_dist_draw. */
int pp_mix_draw(const pp_mixture* mix, const int64_t* rows, int32_t m, int32_t n, uint64_t seed, uint64_t offset,
                uint32_t stream_id, float* out /*dev [n]*/, void* stream);

/* The likelihood of a VECTOR-valued observe of a lock-step run (state.observe, pyprob/state.py:118-155; trace.py:123-125 sums an
 * observed variable's log_prob over its elements): the k-wide form of pp_dist_logweight, one row of k values per particle.
 *     lp[r] = sum_{e<k} log p_kind( x[r,e] | params[0..3][r,e] ),   operand[r,e] = p[r * row_stride + e * elem_stride]
 *     lw[r] += scale * lp[r],  lp_out[r] = lp[r]     for r = rows[j], j < m, or rows NULL: r < n (m, n, rows as pp_dist_logweight)
 * Kinds: the scalar families 0, 1, 3, 4, 6-13 of the table above (Factor and Categorical are refused); params[q] is read for the
 * parameters the kind has, the rest is ignored. Strides are element counts >= 0, as in pp_obs_draw: (row, elem) = (0, 0) a scalar,
 * (0, 1) one row shared by all particles (the observed image), (1, 0) one value per particle, (k, 1) a full [n, k] block; a row
 * stride above k is a padded view. Nothing is materialised to [n, k]. Rows that are not listed are not touched. lw or lp_out may
 * be NULL (not both).
 * Contracts:
 *  - ONE FORMULA. An element's log-density is scalar_log_prob_at (csrc/dist_math.hpp), the definition pp_dist_logweight and
 *    pp_mix_logweight evaluate, with its support guards: one element outside the support makes the row -inf, a NaN where that
 *    definition gives NaN (a NaN mean, stddev, rate ...) makes the row NaN. k = 1 is bit-identical to pp_dist_logweight with that
 *    single term, for lw (the product scale * lp is rounded, then added) and for lp_out.
 *  - FIXED SUMMATION ORDER. A row's sum is a function of k and the row's values only - not of n, m, rows, the grid, the stride
 *    form that delivered the values or the alignment of a pointer. A row has 256 slots, element e belongs to slot e & 255.
 *    A slot starts at -0 (so an empty slot changes no bit) and adds its elements' log-densities in ascending e. Then
 *    t[l] = (slot[4l] + slot[4l+1]) + (slot[4l+2] + slot[4l+3]) for l < 64, and the 64 values t are combined by a butterfly:
 *    in stage d = 1, 2, 4, 8, 16, 32 every t[l] becomes t[l] + t[l ^ d]. An element passes through at most ceil(k / 256) + 8
 *    additions. The lanes that work on a row are the smallest power of two >= ceil(k / 4), at most 64 (one wave per row;
 *    several rows per wave for k <= 128) - a function of k alone; the 16-byte and the 4-byte load path add in this same
 *    order. No float atomics: results are bit-identical from run to run.
 *  - ADDRESSING. All offsets are 64-bit (r * row_stride and n * k may pass 2^31); any 4-byte aligned operand is accepted.
 *    16-byte loads are used when k >= 4, p1..p3 are constant along a row (elem_stride 0) and params[0] and x are each constant
 *    along a row or a run (elem_stride 1) with a 16-byte aligned base and a row stride that is a multiple of 4; anything else
 *    is read with 4-byte loads. Both fill the same registers for one copy of the arithmetic.
 * Returns nonzero without a launch (pp_last_error names pp_obs_logweight) for a kind outside the list, k < 1, n < 0, m < 0,
 * m > n, m != n without rows, a NULL pointer or a negative stride of an operand the kind needs or of x, lw and lp_out both NULL.
 * m == 0 returns 0 without a launch. */
typedef struct pp_obs_operand { const float* p; int64_t row_stride; int32_t elem_stride; int32_t _pad; } pp_obs_operand;
int pp_obs_logweight(int32_t kind, const pp_obs_operand params[4], pp_obs_operand x, int32_t k, float scale, float* lw /*dev [n]*/,
                     float* lp_out, const int64_t* rows, int32_t m, int32_t n, void* stream);

/* pp_obs_logweight for the n_groups * n_per rows of a batched posterior call (pp_is_fused_groups' layout): row i = g * n_per + j
 * belongs to group g = i / n_per. per_group marks the operands that hold ONE ROW PER GROUP: bit q < 4 - params[q], bit 4 - x
 * (PP_OBS_PER_GROUP_X). A marked operand is read as p[g * row_stride + e * elem_stride], every other one as
 * p[i * row_stride + e * elem_stride], with all the stride forms of pp_obs_logweight. The normal use: x = the [n_groups, k]
 * observed images (bit 4), params[0] = the [n_groups * n_per, k] means of the particles. Nothing is materialised to
 * [n_groups * n_per, k]: the per-particle operands are read once, a group's row is re-read by its n_per rows from the caches.
 *     lw[i] += scale * lp[i],  lp_out[i] = lp[i]     for every i < n_groups * n_per (there is no row list)
 * Contracts:
 *  - ONE FORMULA, ONE SUMMATION ORDER: row i has the bits pp_obs_logweight gives a row with the same element values - the same
 *    compiled arithmetic (scalar_log_prob_at, the 256 slots, the butterfly, the two roundings of lw += scale * lp), the lanes
 *    per row a function of k alone.
 *  - THE GROUP SIZE CANNOT CHANGE A BIT: the group index selects row addresses and never enters the arithmetic; rows of
 *    different groups share a wave whenever k <= 128, n_per need not divide anything, any n_per >= 1 is accepted.
 *  - ADDRESSING: 64-bit offsets (n_groups * n_per and g * row_stride may pass 2^31). The 16-byte path has pp_obs_logweight's
 *    condition, applied to a per-group operand's own base and row stride (a [n_groups, k] block with k % 4 != 0 is read with
 *    4-byte loads); both paths give the same bits. No float atomics; one dependent launch on `stream`.
 * Returns nonzero without a launch (pp_last_error names pp_obs_logweight_groups) for a kind outside the list, k < 1,
 * n_groups < 0, n_per < 1, a per_group outside 0..31, a NULL pointer or a negative stride of an operand the kind needs or of x,
 * lw and lp_out both NULL. n_groups == 0 returns 0 without a launch. */
#define PP_OBS_PER_GROUP_X 16
int pp_obs_logweight_groups(int32_t kind, const pp_obs_operand params[4], pp_obs_operand x, int32_t per_group, int32_t k,
                            float scale, float* lw /*dev [n_groups * n_per]*/, float* lp_out, int32_t n_groups, int32_t n_per,
                            void* stream);

/* Empirical.reobserve (pyprob/distributions/empirical.py:469-544): the n_per particles of ONE lock-step posterior call re-scored
 * under n_groups new observations without running the program or the network again. Row i = g * n_per + j of `out` is particle j
 * under observation g. A term is one re-scored observe statement: a scalar family (kinds 0, 1, 3, 4, 6-13, pp_obs_logweight's
 * list), k values per observe, the program's parameters addressed with the PARTICLE j (params[q][j, e] =
 * p[j * row_stride + e * elem_stride]: (0, 0) a scalar, (0, 1) one shared row, (1, 0) one value per particle, (k, 1) [n_per, k])
 * and the new values addressed with the GROUP g (x[g, e] = p[g * row_stride + e * elem_stride]; row stride 0: one value / row for
 * all groups). `lw` holds the call's log-weights, `old` the sum of the terms that are replaced (NULL: zero).
 * THE FORMULA (fp32, no contraction), a contract:
 *   lp_t(g, j) = the summed log-density of x_t[g, :] under params_t[j, :], with the bits pp_obs_logweight writes to lp_out for a
 *                row with these element values (scalar_log_prob_at, the 256 slots, the butterfly: ONE compiled text,
 *                csrc/obs_row.hpp); for k = 1 these are pp_dist_logweight's bits.
 *   s_0 = +0,  s_t = s_{t-1} + (scale_t * lp_t): the product is rounded, then the sum, for t ascending - the chain the
 *                accumulate route builds on a zeroed vector.
 *   out[i] = lw[j]                     where lw[j] is not finite (the call dropped that particle; it stays dropped for every g)
 *   out[i] = lw[j] + (s_T - old[j])    otherwise: the difference is rounded, then the sum.
 * Consequences: re-scoring the original values at the original scales returns lw bit for bit (s_T == old); a new value outside
 * a particle's support gives -inf for that (g, j) only; NaN parameters give NaN; a group's row does not depend on n_groups, on
 * the other groups or on the grid; no atomics - the bits are equal from run to run. The per-particle operands are read from
 * memory once per chunk of groups (a workgroup keeps lw[j] and old[j] in registers and walks the chunk), not once per group.
 * All offsets are 64-bit (n_groups * n_per and j * row_stride may pass 2^31).
 * Returns nonzero without a launch (pp_last_error names pp_is_reobserve_groups) for a kind outside the list, count outside
 * 1..PP_REOBS_MAX_TERMS, k < 1, n_per < 1, n_groups < 0, a NULL pointer or a negative stride of an operand the kind needs or of
 * x, terms, lw or out NULL. n_groups == 0 returns 0 without a launch. */
#define PP_REOBS_MAX_TERMS 8
typedef struct pp_reobs_term {
    int32_t kind;
    int32_t k;                  /* values per observe, >= 1 */
    float   scale;              /* likelihood_importance of the NEW term */
    int32_t _pad;
    pp_obs_operand params[4];   /* rows indexed by the particle j */
    pp_obs_operand x;           /* rows indexed by the group g */
} pp_reobs_term;
int pp_is_reobserve_groups(const pp_reobs_term* terms /*host*/, int32_t count, const float* lw /*dev [n_per]*/,
                           const float* old /*dev [n_per] or NULL*/, float* out /*dev [n_groups * n_per]*/, int32_t n_groups,
                           int32_t n_per, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Individual kernels (used by the whole-path entry points; exported for unit parity tests and profiling)
 * ---------------------------------------------------------------------------------------------------- */
typedef struct pp_gemm_args {
    const float* A; int64_t lda; const int32_t* a_idx;  /* A(m,k) = a_kmajor ? A[ix(k)*lda + m] : A[ix(m)*lda + k] */
    const float* B; int64_t ldb; const int32_t* b_idx;  /* B(n,k) = b_kmajor ? B[ix(k)*ldb + n] : B[ix(n)*ldb + k] */
    float*       C; int64_t ldc; const int32_t* c_idx;  /* C[ix(m)*ldc + n] */
    int32_t M, N, K;
    int32_t a_kmajor, b_kmajor;
    const float* bias;   /* [N] or NULL, added to every row */
    const float* bias2;  /* [N] or NULL */
    const float* mask; int64_t ldmask;  /* optional: result = mask[ix_c(m)*ldmask + n] > 0 ? result : 0 (ReLU backward) */
    int32_t relu;        /* result = max(result, 0) */
    int32_t accumulate;  /* C += result instead of C = result */
    float*       colsum; /* optional [N]: colsum[n] += sum_m result[m,n] (after relu/mask): fused bias gradient */
    int32_t split_k;     /* 0: one workgroup per tile walks all of K (bit-reproducible); 1: the library may spread K over
                            several workgroups and combine with float atomics (used for the gradient products) */
    int32_t _pad;
} pp_gemm_args;

/* C[M,N] = epilogue( sum_k A(m,k) * B(n,k) ) on the fp32 matrix cores (nn.Linear / nn.LSTM GEMMs and their
 * gradients: embedding_feedforward.py:40, inference_network_lstm.py:188). *_idx are optional dev row-index
 * (gather/scatter) arrays: the "address-dispatch gather" of the proposal heads. */
int pp_gemm_f32(const pp_gemm_args* args, void* stream);
/* `count` independent products with identical operand layouts (a_kmajor/b_kmajor) in as few launches as possible
 * (up to 16 problems per launch): the weight-gradient leaves of a backward pass, the per-address head products. */
int pp_gemm_f32_grouped(const pp_gemm_args* args, int32_t count, void* stream);

/* out[c] += sum_i X[ix(i)*ldx + c] for c < n_cols (bias and embedding-table gradients). out2 optional. */
int pp_colsum_f32(const float* X, int64_t ldx, const int32_t* row_idx, int32_t n_rows, int32_t n_cols,
                  float* out, float* out2, void* stream);

/* LSTM input rows  x = [E | s_{t-1} | d_{t-1} | a_{t-1} | d_t | a_t]  (inference_network_lstm.py:146-181).
 * E: dev [B, e_obs] (trace b of row r = r - row_off[t]; given as trace_of_row dev [R]). X: dev [R, ldx]. */
int pp_lstm_input_gather(const pp_net* net, const float* params, const float* E, const int32_t* trace_of_row,
                         const float* value, const int32_t* addr, const int32_t* prev_row, int32_t n_rows,
                         float* X, int64_t ldx, void* stream);

/* Pointwise LSTM cell, gate order i,f,g,o (torch.nn.LSTM). G: [n,4H] pre-activations in, activated gates out.
 * c_prev NULL = first time step of a trace (c_{-1} = 0, inference_network_lstm.py:186-187): the forget gate multiplies zero,
 * its columns [H, 2H) of G are NOT read (pp_ic_loss leaves them uncomputed) and 0 is stored there for the backward pass. */
int pp_lstm_cell_fwd(float* G, const float* c_prev, float* c, float* h, int32_t n, int32_t H, void* stream);
/* Backward of the cell for one time step. G: gates in, dG (pre-activation grads) out. dc_carry: dev [n,H];
 * rows < n_next hold dL/dc_t from step t+1 on entry; on exit rows < n hold dL/dc_{t-1}. */
int pp_lstm_cell_bwd(float* G, const float* c_prev, const float* c, const float* dh, float* dc_carry,
                     int32_t n, int32_t n_next, int32_t H, void* stream);

/* Proposal transforms + Mixture/Categorical log_prob + its gradient w.r.t. the head output y
 * (proposal_normal_normal_mixture.py:20-35, proposal_uniform_truncated_normal_mixture.py:20-36,
 *  proposal_categorical_categorical.py:16-20, distributions/mixture.py:14-16,42-44,
 *  distributions/truncated_normal.py:25-30,40-54).
 *   y  dev [n, ldy]  head outputs, compact group order; rows dev [n] -> row id (value/prior/lp_out index) or NULL
 *   dy dev [n, ldy]  (NULL: forward only) receives grad_scale * d lp / d y  (0 for rows whose lp is -inf)
 *   loss_acc dev [1] += -sum lp (after the -inf -> log(1e-8) rescue); nonfinite dev [1] set if any lp is NaN/+inf */
int pp_head_logprob(int32_t kind, const float* y, int64_t ldy, const int32_t* rows, const float* value,
                    const float* prior, int32_t n, int32_t n_out, float grad_scale, float* lp_out, float* dy,
                    float* loss_acc, int32_t* nonfinite, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * In-stream kernel timing for bench.py's roofline leg: when armed, pp_ic_loss / pp_adam_step record a hipEvent pair
 * around the kernel class `which` on their stream, once per call:
 *   0  forward input GEMM X*W_ih^T                                   work = FLOPs
 *   1  the grouped weight-gradient launch of the backward pass       work = FLOPs
 *   2  observe embedding + LSTM input rows (the gather path)         work = algorithmic bytes
 *   3  pp_adam_step (optimizer pass over the flat buffers)           work = algorithmic bytes
 *   4  the draw + log q kernel of pp_is_step                         work = algorithmic bytes
 *   5  the fused statement kernel of pp_is_step / pp_is_step_rows    work = FLOPs (input + recurrent
 *                                                                    product and both head layers per particle)
 *   6  the device chain of a posterior call's first statement: every launch from pp_is_init to the end of pp_is_fused
 *      (observe embedding, the one-row network, the pass over the particles with its statistics)   work = 0
 *   PP_PROF_CNN_FWD + k, k = 0..7: the launches of pp_cnn2d5c_forward (weight images, conv1, conv2, pool 1, conv3, conv4,
 *      conv5, pool 2); PP_PROF_CNN_BWD + k, k = 0..10: those of pp_cnn2d5c_backward (pool 2, dW5, dZ4, dW4, dZ3, dW3, dP1,
 *      pool 1, dW2, dZ1, dW1; a dW class covers the split-K launch and its reduction). work = FLOPs executed (0: a copy)
 * pp_prof_collect returns the elapsed milliseconds and the work of every recorded launch (flops_out).
 * ---------------------------------------------------------------------------------------------------- */
/* Host-side plan of the streaming weight-gradient launch (csrc/wgrad_t1.hip) for `count` queued products dW += A^T B (both
 * operands k-major: torch.autograd's weight gradients of nn.Linear / nn.LSTM, inference_network_lstm.py:186-220 backward) -
 * no device work, for tests of the host logic. zero_blocks: [count][2][6] = {m0, m1, n0, n1, k0, k1} or NULL; out: [cap][10] =
 * {M, N, K, S, ks, gather, first workgroup, C offset, A offset, B (or index) offset}. Returns the number of problems (0: the
 * tile kernels take the flush). */
int pp_debug_wgrad_plan(const pp_gemm_args* products, const int32_t* zero_blocks, int32_t count, int64_t* out, int32_t cap,
                        int32_t* n_blocks);
/* The same plan, launched alone: wide_out[i] (host [cap], may be NULL) = 1 when problem i of the plan streams its operands with
 * 16-byte loads (both operand pointers 16-byte aligned after the cut, lda and ldb multiples of 4, every vector inside its row;
 * PP_WGRAD_WIDE=0: none), 0 for the dword loop. launch != 0: runs the weight-gradient launch on `stream` without reduction jobs
 * (products = dev pointers then). Returns the number of problems; 0: refused, nothing launched. */
int pp_debug_wgrad_run(const pp_gemm_args* products, const int32_t* zero_blocks, int32_t count, int32_t launch, void* stream,
                       int32_t* wide_out, int32_t cap);
int pp_prof_arm(int32_t which, int32_t max_samples);          /* allocate event pairs; 0 disarms */
int pp_prof_stride(int32_t stride);                           /* time every stride-th launch of the class (default 1):
                                                                 an event pair costs the stream ~3 us, a stride keeps the
                                                                 timed region of a benchmark within ~1 % of an untimed one */
int pp_prof_collect(float* ms_out, int32_t cap, int32_t* n_out, double* flops_out); /* syncs the events */

/* Diagnostic: one wave runs `iters` dependent FMAs; out[0] = elapsed shader cycles (s_memtime), out[1] = elapsed
 * 100 MHz wall ticks (s_memrealtime). Effective shader clock = out[0] / (out[1] * 10 ns): used by bench.py to report the
 * DVFS state the timed region ran in (MI355X_MICROARCH.md "DVFS give-back"). */
/* Diagnostic: when set, the fused head-tail kernel writes per-phase s_memtime stamps of workgroups 0 and 100 to buf. */
/* ---- data parallel: RCCL from the C side (csrc/dp.hip) --------------------------------------------------------------
 * Replaces _distributed_sync_grad (pyprob/nn/inference_network.py:296-333: one all-reduce per tensor + presence map + loss)
 * with ONE grouped launch over the flat buffer. librccl.so is dlopen'ed from `rccl_path` (the copy torch loaded); the
 * communicator belongs to this library: rank 0 creates a 128-byte id (pp_dp_unique_id), the host hands it to every rank
 * (torch.distributed broadcast, pyprob_amd/parallel.py), all ranks call pp_dp_init (collective, current HIP device). */
int pp_dp_unique_id(const char* rccl_path, void* id_out /*host [128]*/);
int pp_dp_init(const char* rccl_path, const void* unique_id /*host [128]*/, int32_t rank, int32_t world);
int pp_dp_world(void);       /* size of the communicator, 0 when there is none */
int pp_dp_destroy(void);
/* in-place sum over the ranks of the pieces [off[i], off[i] + cnt[i]) of base (floats): one grouped launch */
int pp_dp_allreduce(float* base /*dev*/, const int64_t* off /*host*/, const int64_t* cnt /*host*/, int32_t n, void* stream);
/* The exchange of one training step: grads_full = dev [n_params | n_tensors | loss | flag]. Copies `presence` (dev
 * [n_tensors], or NULL when the tail already holds the step's presence map) and the step's non-finite flag `status` (dev
 * int32) into the tail, all-reduces everything but the skip ranges, and writes the mean loss / the any-rank flag to
 * loss_out / status_out (dev, may be NULL). Adam then runs with grad_scale = 1 / world on the reduced tail. */
int pp_dp_reduce_grads(float* grads_full, int64_t n_params, int32_t n_tensors, const float* presence, const int32_t* status,
                       const int64_t* skip_off /*host*/, const int64_t* skip_cnt /*host*/, int32_t n_skip, float* loss_out,
                       int32_t* status_out, void* stream);

/* (ABI 13) Bucket 0 under the rest of the backward pass - what `distributed_num_buckets` is for in the reference
 * (pyprob/nn/inference_network.py:300-325: gradients reduced bucket by bucket). off / cnt (host, n <= 2 ascending ranges of the
 * flat gradient buffer, in floats; n = 0: off) name gradient tensors that the backward pass completes EARLY: pp_ic_loss then
 * issues its weight-gradient launch in two parts - the products (and reduction jobs) that write into the hull of the ranges
 * first, the remaining ones after - and starts the ranges' all-reduce on a side stream between the two; pp_dp_reduce_grads
 * leaves the ranges out of its own collective and makes its stream wait for the side stream before it returns the step to
 * Adam. Host-side state: every rank must set the same ranges (pyprob_amd.engine.ICEngine.enable_dp_overlap: the first LSTM
 * layer's weight and bias gradients, minus a skipped W_hh; PP_DP_OVERLAP=1 - measured on a one-rank group the two-part launch and
 * its two cross-stream waits cost a 67 us step ~26 us, so it is not the default). Same result as the unsplit exchange. */
int pp_dp_overlap(const int64_t* off /*host*/, const int64_t* cnt /*host*/, int32_t n);
/* arm = 1 / 0: HIP event pairs around the collectives of the following overlapped steps on / off. us_out (host [3] or NULL):
 * the LAST overlapped step's {ranges' all-reduce on the side stream, the rest's all-reduce, what the step's stream then still
 * waited for the side stream} in microseconds (synchronises on those events). Returns 1 when us_out was filled, else 0. */
int pp_dp_overlap_stats(int32_t arm, float* us_out);

int pp_debug_timeline(long long* buf /*dev [16] or NULL*/);
/* debug: per-workgroup {start, end, problem, split, operands ready, loads issued, first slab landed, K loop done} stamps (10 ns ticks) of the grouped async GEMM launches
 * (mode 1: weight-gradient groups, 2: data-gradient products); buf = dev int64 [8 * cap] or NULL (tools/wg_trace.py).
 * mode 3: the Adam launches - {start, tensor known, gradient arrived, p / m / v arrived, corrections ready, stores issued, end,
 * tensor id} per workgroup (tools/adam_wg_trace.py)
 * mode 4: the step's first launch (obs_embed_fwd_kernel) - embedding workgroups {start, entry loads issued, weights arrived, LDS
 * image complete, observation arrived and layer 0 done, last dense layer done, stores issued, end}, bias / image workgroups
 * {start, operands arrived, end, -, -, -, -, job kind: 1 bias, 2 image} (tools/first_launch_wg_trace.py) */
int pp_debug_wgtrace(long long* buf, int32_t cap, int32_t mode);
int pp_debug_clock_probe(int32_t iters, long long* out /*dev [2]*/, float* sink /*dev [1]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYPROB_AMD_H */
