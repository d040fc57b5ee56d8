// CNN2D5C observe embedding: pyprob's EmbeddingCNN2D5C (pyprob/nn/embedding_cnn_2d_5c.py) up to the flattened feature
// matrix, forward and backward, in exact fp32 on v_mfma_f32_32x32x2_f32.
//
//   conv1 C->64, conv2 64->64, max-pool 2, conv3 64->128, conv4 128->128, conv5 128->128, max-pool 2, flatten (c, y, x)
//   every convolution 3x3, stride 1, no padding, bias, ReLU; pools 2x2 stride 2 floor.
//
// Activations are NHWC between the kernels (a pixel's channels are contiguous: one MFMA operand row is one coalesced
// read). Parameters and gradients keep the reference's [Cout, Cin, 3, 3] inside the flat buffers; tap-major images of
// the weights ([tap][k][n], for the forward and the flipped one for the data gradient) are rebuilt in the workspace by
// every forward call.
//
// * conv3x3_mfma_kernel: implicit GEMM, M = B Ho Wo pixels, N = output channels, K = 9 x input channels walked tap by
//   tap. A wave owns 32 pixels x all N channels (N / 32 accumulator tiles of 32 x 32). No im2col buffer, no LDS: lane
//   (i, h) reads a float4 of its pixel's channels [8 j + 4 h, +4) and the matching rows of the weight image, so the K
//   order of every output element is a function of the layer alone - never of the batch size or of where the image sits
//   in the batch (tests rely on that: features are bit-equal whatever batch an image is in). The same kernel computes
//   the data gradient: `off` = 2 shifts the taps to a full correlation whose rows outside the image are zero, the weight
//   image is the flipped one, the epilogue multiplies with the ReLU mask of the layer below.
// * conv3x3_wgrad_kernel: dW[tap] = X_tap^T dY, M = Cin, N = Cout, K = B Ho Wo pixels. Both operands are k-major in
//   memory as they lie (NHWC), so fragments are plain coalesced loads (the wgrad_t1.hip scheme). K is cut into S ranges;
//   range s STORES its partial image, and wgrad_reduce_kernel adds the S images in a fixed order into the gradient
//   buffer (and transposes back to [Cout, Cin, 3, 3]): no float atomics, the result is the same on every run whether
//   PP_DETERMINISTIC is set or not. Bias gradients (column sums of dY) ride along in the waves of tap 0.
// * conv1 (Cin = C <= 4, K <= 36, 1 % of the FLOPs) forward and weight gradient are plain VALU kernels.
#include "cnn2d.hpp"

#include <algorithm>

namespace pp {

bool cnn_geom(const pp_net* net, int o, CnnGeom& g) {
    if (!net || o < 0 || o >= net->n_obs || net->obs_kind[o] != PP_OBS_CNN2D5C) return false;
    g.C = net->obs_shape[o][0]; g.H = net->obs_shape[o][1]; g.W = net->obs_shape[o][2];
    if (g.C < 1 || g.C > 4 || g.H < 20 || g.W < 20) return false;
    const int ci[5] = {g.C, 64, 64, 128, 128}, co[5] = {64, 64, 128, 128, 128};
    int h = g.H, w = g.W;
    for (int l = 0; l < 5; ++l) {
        g.cin[l] = ci[l]; g.cout[l] = co[l]; g.hin[l] = h; g.win[l] = w;
        h -= 2; w -= 2;
        if (l == 1) { g.hp1 = h / 2; g.wp1 = w / 2; h = g.hp1; w = g.wp1; }
    }
    g.hp2 = h / 2; g.wp2 = w / 2;
    g.F = 128 * g.hp2 * g.wp2;
    return g.hp2 >= 1 && g.wp2 >= 1;
}

// ---- weight images -------------------------------------------------------------------------------------------------
// wf[(tap Cin + cin) Cout + cout] = W[cout][cin][tap];  wd[(tap Cout + cout) Cin + cin] = W[cout][cin][8 - tap]
__global__ __launch_bounds__(256) void cnn_weight_images_kernel(const float* __restrict__ W, int Cin, int Cout,
                                                                float* __restrict__ wf, float* __restrict__ wd) {
    const int n = 9 * Cin * Cout;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    {
        const int cout = i % Cout, cin = (i / Cout) % Cin, tap = i / (Cout * Cin);
        wf[i] = W[((int64_t)cout * Cin + cin) * 9 + tap];
    }
    if (wd) {      // (only a backward pass reads the flipped image)
        const int cin = i % Cin, cout = (i / Cin) % Cout, tap = i / (Cout * Cin);
        wd[i] = W[((int64_t)cout * Cin + cin) * 9 + 8 - tap];
    }
}

// ---- conv1: C -> 64 on the VALU ------------------------------------------------------------------------------------
// x [B][C][H][W] -> a1 [B, H - 2, W - 2, 64], bias + ReLU. Thread = (output channel, pixel lane); 8 pixels per thread.
template <int C>
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ out, int H,
                                                        int Wd, int64_t M) {
    const int cout = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int Ho = H - 2, Wo = Wd - 2;
    float w[C * 9];
#pragma unroll
    for (int k = 0; k < C * 9; ++k) w[k] = W[cout * C * 9 + k];
    const float bv = bias[cout];
    for (int p = 0; p < 8; ++p) {
        const int64_t m = (int64_t)blockIdx.x * 32 + p * 4 + sub;
        if (m >= M) break;
        const int xx = (int)(m % Wo), yy = (int)((m / Wo) % Ho);
        const int64_t b = m / ((int64_t)Wo * Ho);
        const float* px = x + (b * C * H + yy) * Wd + xx;
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int t = 0; t < 9; ++t) acc = fmaf(px[((int64_t)c * H + t / 3) * Wd + t % 3], w[c * 9 + t], acc);
        out[m * 64 + cout] = relu_keep_nan(acc + bv);
    }
}

// partial weight / bias gradient of conv1 over the pixel range of block s:
// part[(s 9C + tap C + c) 64 + cout], dbp[s 64 + cout]
template <int C>
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                          float* __restrict__ part, float* __restrict__ dbp, int H, int Wd,
                                                          int64_t M, int64_t chunk) {
    __shared__ float red[4][C * 9 + 1][64];
    const int cout = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int Ho = H - 2, Wo = Wd - 2;
    const int64_t m0 = (int64_t)blockIdx.x * chunk, m1 = std::min<int64_t>(m0 + chunk, M);
    float acc[C * 9];
#pragma unroll
    for (int k = 0; k < C * 9; ++k) acc[k] = 0.0f;
    float db = 0.0f;
    for (int64_t m = m0 + sub; m < m1; m += 4) {
        const int xx = (int)(m % Wo), yy = (int)((m / Wo) % Ho);
        const int64_t b = m / ((int64_t)Wo * Ho);
        const float g = dz[m * 64 + cout];
        const float* px = x + (b * C * H + yy) * Wd + xx;
        db += g;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[c * 9 + t] = fmaf(px[((int64_t)c * H + t / 3) * Wd + t % 3], g, acc[c * 9 + t]);
    }
#pragma unroll
    for (int k = 0; k < C * 9; ++k) red[sub][k][cout] = acc[k];
    red[sub][C * 9][cout] = db;
    __syncthreads();
    for (int k = sub; k <= C * 9; k += 4) {
        const float v = (red[0][k][cout] + red[1][k][cout]) + (red[2][k][cout] + red[3][k][cout]);
        if (k == C * 9) {
            dbp[(int64_t)blockIdx.x * 64 + cout] = v;
        } else {
            const int c = k / 9, t = k % 9;
            part[((int64_t)blockIdx.x * 9 * C + t * C + c) * 64 + cout] = v;
        }
    }
}

// ---- 3x3 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 --------------------------------------------------
// in [B, Hin, Win, KC] (NHWC), wimg [9][KC][NC], out [B, Hout, Wout, NC]. Output pixel (y, x), tap (ty, tx) reads input
// pixel (y + ty - off, x + tx - off); outside the input the row is zero. off = 0, Hout = Hin - 2: the forward valid
// convolution (bias, ReLU). off = 2, Hout = Hin + 2: the data gradient (wimg flipped; mask = activations of the layer
// below, the result is zeroed where they are not positive).
template <int NT>
__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(const float* __restrict__ in, int Hin, int Win, int KC,
                                                           const float* __restrict__ wimg, const float* __restrict__ bias,
                                                           const float* __restrict__ mask, float* __restrict__ out, int Hout,
                                                           int Wout, int off, int relu, int64_t M) {
    constexpr int NC = NT * 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
    if (m0 >= M) return;
    const int i = lane & 31, h = lane >> 5;
    const int64_t m = std::min<int64_t>(m0 + i, M - 1);     // (rows past the end repeat the last pixel; never stored)
    const int x = (int)(m % Wout), y = (int)((m / Wout) % Hout);
    const int64_t b = m / ((int64_t)Wout * Hout);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = y + tap / 3 - off, ix = x + tap % 3 - off;
        const bool ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
        const float* pa = in + ((b * Hin + (ok ? iy : 0)) * Win + (ok ? ix : 0)) * KC + 4 * h;
        const float* pb = wimg + ((int64_t)tap * KC + 4 * h) * NC + i;
        for (int k0 = 0; k0 < KC; k0 += 8) {
            f32x4 a = *reinterpret_cast<const f32x4*>(pa + k0);
            if (!ok) a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            float bv[4][NT];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) bv[e][t] = pb[(int64_t)(k0 + e) * NC + 32 * t];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bv[e][t], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t mm = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (mm >= M) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int ch = 32 * t + i;
            float v = acc[t][r];
            if (bias) v += bias[ch];
            if (relu) v = relu_keep_nan(v);
            if (mask) v = mask[mm * NC + ch] > 0.0f ? v : 0.0f;
            out[mm * NC + ch] = v;
        }
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------
// X [B, Hin, Win, Cin], dY [B, Ho, Wo, Cout] (Ho = Hin - 2). Wave item = (s, tap, ct): the 32 input channels
// [32 ct, +32) x all Cout of tap `tap` over the pixels [s chunk, (s + 1) chunk) -> part[((s 9 + tap) Cin + cin) Cout + cout].
// Waves with tap == 0 and ct == 0 also write the column sums of dY over their range to dbp[s Cout + cout].
template <int NT>
__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(const float* __restrict__ X, int Hin, int Win, int Cin,
                                                            const float* __restrict__ dY, float* __restrict__ part,
                                                            float* __restrict__ dbp, int64_t M, int64_t chunk, int n_items) {
    constexpr int Cout = NT * 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= n_items) return;
    const int CT = Cin / 32;
    const int ct = item % CT, tap = (item / CT) % 9, s = item / (CT * 9);
    const int i = lane & 31, h = lane >> 5;
    const int Ho = Hin - 2, Wo = Win - 2;
    const int64_t k0 = (int64_t)s * chunk, k1 = std::min<int64_t>(k0 + chunk, M);
    int64_t mk = k0 + h;                    // this lane's pixel: advances by 2 per MFMA step
    int x = (int)(mk % Wo), y = (int)((mk / Wo) % Ho);
    int64_t b = mk / ((int64_t)Wo * Ho);
    const int dy = tap / 3, dx = tap % 3;
    const bool do_bias = tap == 0 && ct == 0;      // (wave-uniform: these waves also store the column sums of dY)
    f32x16 acc[NT];
    float bs[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        bs[t] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    }
    for (int64_t k = k0; k < k1; k += 2) {
        const bool ok = mk < k1;
        const int64_t mc = ok ? mk : k0;     // (a clamped address; the values are zeroed)
        const int xc = ok ? x : 0, yc = ok ? y : 0;
        const int64_t bc = ok ? b : k0 / ((int64_t)Wo * Ho);
        float a = X[((bc * Hin + yc + dy) * Win + xc + dx) * Cin + 32 * ct + i];
        float bv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bv[t] = dY[mc * Cout + 32 * t + i];
        if (!ok) {
            a = 0.0f;
#pragma unroll
            for (int t = 0; t < NT; ++t) bv[t] = 0.0f;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[t], acc[t], 0, 0, 0);
            if (do_bias) bs[t] += bv[t];
        }
        mk += 2; x += 2;
        if (x >= Wo) {
            x -= Wo; ++y;
            if (y >= Ho) { y = 0; ++b; }
        }
    }
    float* po = part + ((int64_t)(s * 9 + tap) * Cin + 32 * ct) * Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
        for (int t = 0; t < NT; ++t) po[(int64_t)row * Cout + 32 * t + i] = acc[t][r];
    }
    if (do_bias) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float tot = bs[t] + __shfl_xor(bs[t], 32, 64);
            if (h == 0) dbp[(int64_t)s * Cout + 32 * t + i] = tot;
        }
    }
}

// grads_w[(cout Cin + cin) 9 + tap] += sum_s part[s][tap Cin + cin][cout] (s ascending); grads_b[cout] += sum_s dbp[s][cout]
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dbp,
                                                           int S, int Cin, int Cout, float* __restrict__ gw,
                                                           float* __restrict__ gb) {
    const int n = 9 * Cin * Cout;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) {
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v += part[(int64_t)s * n + idx];
        const int cout = idx % Cout, r = idx / Cout, cin = r % Cin, tap = r / Cin;
        gw[((int64_t)cout * Cin + cin) * 9 + tap] += v;
    } else if (idx < n + Cout) {
        const int cout = idx - n;
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v += dbp[(int64_t)s * Cout + cout];
        gb[cout] += v;
    }
}

// ---- 2x2 max-pool ----------------------------------------------------------------------------------------------------
// in [B, Hin, Win, C] -> chw == 0: out [B, Hp, Wp, C]; chw == 1: out[b ldo + (c Hp + yp) Wp + xp] (the reference's flatten)
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ in, int Hin, int Win, int C,
                                                          float* __restrict__ out, int Hp, int Wp, int chw, int64_t ldo,
                                                          int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C), xp = (int)((idx / C) % Wp), yp = (int)((idx / ((int64_t)C * Wp)) % Hp);
    const int64_t b = idx / ((int64_t)C * Wp * Hp);
    const float* p = in + ((b * Hin + 2 * yp) * Win + 2 * xp) * C + c;
    float v = p[0];
    const float v1 = p[C], v2 = p[(int64_t)Win * C], v3 = p[(int64_t)Win * C + C];
    v = v1 > v ? v1 : v;
    v = v2 > v ? v2 : v;
    v = v3 > v ? v3 : v;
    if (chw) out[b * ldo + ((int64_t)c * Hp + yp) * Wp + xp] = v;
    else out[idx] = v;
}

// Gradient into the pool's input `act` (a ReLU output): element (y, x) receives its window's gradient if it is the
// window's first maximum in (y, x) scan order (torch's choice among equal values) and positive (the ReLU mask of the
// convolution that produced it); elements of rows / columns that the floor dropped receive zero.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ act, int Hin, int Win, int C,
                                                          const float* __restrict__ dout, int Hp, int Wp, int chw,
                                                          int64_t ldo, float* __restrict__ din, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C), x = (int)((idx / C) % Win), y = (int)((idx / ((int64_t)C * Win)) % Hin);
    const int64_t b = idx / ((int64_t)C * Win * Hin);
    const int yp = y >> 1, xp = x >> 1;
    float g = 0.0f;
    if (yp < Hp && xp < Wp) {
        const float* p = act + ((b * Hin + 2 * yp) * Win + 2 * xp) * C + c;
        const float v[4] = {p[0], p[C], p[(int64_t)Win * C], p[(int64_t)Win * C + C]};
        int best = 0;
        if (v[1] > v[best]) best = 1;
        if (v[2] > v[best]) best = 2;
        if (v[3] > v[best]) best = 3;
        const int self = (y & 1) * 2 + (x & 1);
        if (best == self && v[self] > 0.0f)
            g = chw ? dout[b * ldo + ((int64_t)c * Hp + yp) * Wp + xp] : dout[((b * Hp + yp) * Wp + xp) * C + c];
    }
    din[idx] = g;
}

// ---- workspace --------------------------------------------------------------------------------------------------------
struct CnnWs {
    float* a0;             // [B, C H W] copy of the images (conv1's weight gradient reads them again)
    float* wf[5];          // forward weight images of conv2..5 (index = layer)
    float* wd[5];          // flipped images for the data gradients
    float* a[5];           // ReLU outputs of conv1..5, NHWC
    float* p1;             // first pool's output
    float* g0; float* g1;  // gradient ping-pong
    float* part;           // split-K partial weight-gradient images + bias partials
    size_t bytes;
};

// K ranges of a weight-gradient launch over M pixels whose partial image has `image_floats` floats: ranges of >= 256 pixels,
// as many as 48 MB of partial images allow (at least 64, at most 1024) - a wave walks its range with few loads in flight, so
// the launch wants several waves per SIMD (conv2 at B = 1024 with 64 ranges of 9 216 pixels: 2.7 ms)
static int wgrad_splits(int64_t M, int64_t image_floats, int64_t* chunk) {
    const int64_t cap = std::min<int64_t>(1024, std::max<int64_t>(64, (int64_t(48) << 20) / (4 * image_floats)));
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(cap, (M + 255) / 256));
    int64_t c = (M + S - 1) / S;
    c += c & 1;                              // an MFMA step takes two pixels
    *chunk = c;
    return (int)((M + c - 1) / c);
}

static void cnn_carve(const CnnGeom& g, int B, void* p, CnnWs& w) {
    char* base = static_cast<char*>(p);
    size_t off = 0;
    auto take = [&](int64_t floats) {
        off = (off + 255) & ~size_t(255);
        float* r = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += (size_t)std::max<int64_t>(floats, 1) * sizeof(float);
        return r;
    };
    w.a0 = take((int64_t)B * g.C * g.H * g.W);
    w.wf[0] = w.wd[0] = nullptr;
    int64_t part = 0, amax = 0;
    for (int l = 0; l < 5; ++l) {
        const int64_t wn = 9 * (int64_t)g.cin[l] * g.cout[l];
        if (l > 0) { w.wf[l] = take(wn); w.wd[l] = take(wn); }
        const int64_t pix = (int64_t)B * (g.hin[l] - 2) * (g.win[l] - 2);
        w.a[l] = take(pix * g.cout[l]);
        int64_t chunk;
        const int S = wgrad_splits(pix, wn, &chunk);
        part = std::max(part, S * (wn + g.cout[l]));
        amax = std::max(amax, pix * g.cout[l]);
    }
    const int64_t p1n = (int64_t)B * g.hp1 * g.wp1 * 64;
    w.p1 = take(p1n);
    w.g0 = take(amax);        // dZ5, dZ3, dZ2
    w.g1 = take(amax);        // dZ4, dP1, dZ1   (both sized for the largest activation, conv1's)
    w.part = take(part);
    w.bytes = off + 256;
}

size_t cnn_workspace_bytes(const pp_net* net, int o, int B) {
    CnnGeom g;
    if (!cnn_geom(net, o, g) || B < 1) return 0;
    CnnWs w;
    cnn_carve(g, B, nullptr, w);
    return w.bytes;
}

static int check_cnn(const pp_net* net, int o, CnnGeom& g, int B, const void* ws, size_t ws_bytes, CnnWs& w, const char* who) {
    PP_CHECK_ARG(cnn_geom(net, o, g), "%s: observable %d is not a CNN2D5C embedding with C in 1..4 and sides >= 20", who, o);
    PP_CHECK_ARG(net->obs_feat[o] == g.F, "%s: obs_feat %d != 128 * h5 * w5 = %d", who, net->obs_feat[o], g.F);
    PP_CHECK_ARG(B >= 1 && ws, "%s: empty batch or null workspace", who);
    PP_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    cnn_carve(g, B, const_cast<void*>(ws), w);
    if (w.bytes > ws_bytes) {
        set_error("%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, w.bytes);
        return PP_ENOSPACE;
    }
    return 0;
}

// `cls`: kernel class of the in-stream timing (pp_prof_arm, PP_PROF_CNN_*); work = FLOPs executed
static int conv_mfma(int cls, const float* in, int Hin, int Win, int KC, int NC, const float* wimg, const float* bias,
                     const float* mask, float* out, int off, int relu, int B, hipStream_t st) {
    const int Hout = off ? Hin + 2 : Hin - 2, Wout = off ? Win + 2 : Win - 2;
    const int64_t M = (int64_t)B * Hout * Wout;
    const dim3 grid(cdiv(M, 128)), block(256);
    prof_begin(cls, st);
    if (NC == 64)
        hipLaunchKernelGGL(conv3x3_mfma_kernel<2>, grid, block, 0, st, in, Hin, Win, KC, wimg, bias, mask, out, Hout, Wout, off,
                           relu, M);
    else
        hipLaunchKernelGGL(conv3x3_mfma_kernel<4>, grid, block, 0, st, in, Hin, Win, KC, wimg, bias, mask, out, Hout, Wout, off,
                           relu, M);
    PP_LAUNCH_CHECK("conv3x3_mfma");
    prof_end(cls, 2.0 * (double)M * 9.0 * KC * NC, st);
    return 0;
}

int cnn_forward(const pp_net* net, int o, const float* P, const float* x, int64_t ldx, int B, float* feat, int64_t ldf,
                void* ws, size_t ws_bytes, bool for_backward, hipStream_t st) {
    CnnGeom g;
    CnnWs w;
    PP_TRY(check_cnn(net, o, g, B, ws, ws_bytes, w, "pp_cnn2d5c_forward"));
    PP_CHECK_ARG(P && x && feat && ldx >= g.C * g.H * g.W && ldf >= g.F, "pp_cnn2d5c_forward: null pointer or short rows");
    const size_t row = (size_t)g.C * g.H * g.W * sizeof(float);
    if (hipMemcpy2DAsync(w.a0, row, x, (size_t)ldx * sizeof(float), row, B, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("pp_cnn2d5c_forward: image copy failed");
        return PP_EHIP;
    }
    prof_begin(PP_PROF_CNN_FWD + 0, st);
    for (int l = 1; l < 5; ++l) {
        const int n = 9 * g.cin[l] * g.cout[l];
        hipLaunchKernelGGL(cnn_weight_images_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, P + net->obs_conv_w[o][l], g.cin[l],
                           g.cout[l], w.wf[l], for_backward ? w.wd[l] : nullptr);
        PP_LAUNCH_CHECK("cnn_weight_images");
    }
    prof_end(PP_PROF_CNN_FWD + 0, 0.0, st);
    {
        const int64_t M = (int64_t)B * (g.H - 2) * (g.W - 2);
        const dim3 grid(cdiv(M, 32)), block(256);
        const float* W1 = P + net->obs_conv_w[o][0];
        const float* b1 = P + net->obs_conv_b[o][0];
        prof_begin(PP_PROF_CNN_FWD + 1, st);
        switch (g.C) {
            case 1: hipLaunchKernelGGL(conv1_fwd_kernel<1>, grid, block, 0, st, w.a0, W1, b1, w.a[0], g.H, g.W, M); break;
            case 2: hipLaunchKernelGGL(conv1_fwd_kernel<2>, grid, block, 0, st, w.a0, W1, b1, w.a[0], g.H, g.W, M); break;
            case 3: hipLaunchKernelGGL(conv1_fwd_kernel<3>, grid, block, 0, st, w.a0, W1, b1, w.a[0], g.H, g.W, M); break;
            default: hipLaunchKernelGGL(conv1_fwd_kernel<4>, grid, block, 0, st, w.a0, W1, b1, w.a[0], g.H, g.W, M); break;
        }
        PP_LAUNCH_CHECK("conv1_fwd");
        prof_end(PP_PROF_CNN_FWD + 1, 2.0 * (double)M * 9.0 * g.C * 64, st);
    }
    PP_TRY(conv_mfma(PP_PROF_CNN_FWD + 2, w.a[0], g.hin[1], g.win[1], 64, 64, w.wf[1], P + net->obs_conv_b[o][1], nullptr, w.a[1], 0, 1, B, st));
    {
        const int64_t n = (int64_t)B * g.hp1 * g.wp1 * 64;
        prof_begin(PP_PROF_CNN_FWD + 3, st);
        hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w.a[1], g.hin[1] - 2, g.win[1] - 2, 64, w.p1,
                           g.hp1, g.wp1, 0, (int64_t)0, n);
        PP_LAUNCH_CHECK("maxpool_fwd");
        prof_end(PP_PROF_CNN_FWD + 3, 0.0, st);
    }
    PP_TRY(conv_mfma(PP_PROF_CNN_FWD + 4, w.p1, g.hin[2], g.win[2], 64, 128, w.wf[2], P + net->obs_conv_b[o][2], nullptr, w.a[2], 0, 1, B, st));
    PP_TRY(conv_mfma(PP_PROF_CNN_FWD + 5, w.a[2], g.hin[3], g.win[3], 128, 128, w.wf[3], P + net->obs_conv_b[o][3], nullptr, w.a[3], 0, 1, B, st));
    PP_TRY(conv_mfma(PP_PROF_CNN_FWD + 6, w.a[3], g.hin[4], g.win[4], 128, 128, w.wf[4], P + net->obs_conv_b[o][4], nullptr, w.a[4], 0, 1, B, st));
    {
        const int64_t n = (int64_t)B * g.hp2 * g.wp2 * 128;
        prof_begin(PP_PROF_CNN_FWD + 7, st);
        hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w.a[4], g.hin[4] - 2, g.win[4] - 2, 128, feat,
                           g.hp2, g.wp2, 1, ldf, n);
        PP_LAUNCH_CHECK("maxpool_fwd");
        prof_end(PP_PROF_CNN_FWD + 7, 0.0, st);
    }
    return 0;
}

// weight + bias gradient of convolution l (l >= 1) from its input X and dZ = gradient at its (masked) output
static int conv_wgrad(const pp_net* net, int o, const CnnGeom& g, int l, const float* X, const float* dZ, int B, CnnWs& w,
                      float* grads, hipStream_t st) {
    const int Cin = g.cin[l], Cout = g.cout[l];
    const int64_t M = (int64_t)B * (g.hin[l] - 2) * (g.win[l] - 2);
    int64_t chunk;
    const int64_t wn = 9 * (int64_t)Cin * Cout;
    const int S = wgrad_splits(M, wn, &chunk);
    float* dbp = w.part + S * wn;
    const int n_items = S * 9 * (Cin / 32);
    const int cls = PP_PROF_CNN_BWD + (l == 4 ? 1 : l == 3 ? 3 : l == 2 ? 5 : 8);
    prof_begin(cls, st);
    if (Cout == 64)
        hipLaunchKernelGGL(conv3x3_wgrad_kernel<2>, dim3(cdiv(n_items, 4)), dim3(256), 0, st, X, g.hin[l], g.win[l], Cin, dZ,
                           w.part, dbp, M, chunk, n_items);
    else
        hipLaunchKernelGGL(conv3x3_wgrad_kernel<4>, dim3(cdiv(n_items, 4)), dim3(256), 0, st, X, g.hin[l], g.win[l], Cin, dZ,
                           w.part, dbp, M, chunk, n_items);
    PP_LAUNCH_CHECK("conv3x3_wgrad");
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(wn + Cout, 256)), dim3(256), 0, st, w.part, dbp, S, Cin, Cout,
                       grads + net->obs_conv_w[o][l], grads + net->obs_conv_b[o][l]);
    PP_LAUNCH_CHECK("wgrad_reduce");
    prof_end(cls, 2.0 * (double)M * (double)wn, st);
    return 0;
}

// (the images, the activations and the weight images were saved in the workspace by the forward call)
int cnn_backward(const pp_net* net, int o, const float* dfeat, int64_t lddf, int B, float* grads, void* ws, size_t ws_bytes,
                 hipStream_t st) {
    CnnGeom g;
    CnnWs w;
    PP_TRY(check_cnn(net, o, g, B, ws, ws_bytes, w, "pp_cnn2d5c_backward"));
    PP_CHECK_ARG(dfeat && grads && lddf >= g.F, "pp_cnn2d5c_backward: null pointer or short rows");
    // dZ5 = pool2 backward (+ ReLU mask of conv5)
    {
        const int H5 = g.hin[4] - 2, W5 = g.win[4] - 2;
        const int64_t n = (int64_t)B * H5 * W5 * 128;
        prof_begin(PP_PROF_CNN_BWD + 0, st);
        hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w.a[4], H5, W5, 128, dfeat, g.hp2, g.wp2, 1,
                           lddf, w.g0, n);
        PP_LAUNCH_CHECK("maxpool_bwd");
        prof_end(PP_PROF_CNN_BWD + 0, 0.0, st);
    }
    // conv5, conv4: dW from (input activations, dZ), then dZ of the layer below = full correlation, masked
    PP_TRY(conv_wgrad(net, o, g, 4, w.a[3], w.g0, B, w, grads, st));
    PP_TRY(conv_mfma(PP_PROF_CNN_BWD + 2, w.g0, g.hin[4] - 2, g.win[4] - 2, 128, 128, w.wd[4], nullptr, w.a[3], w.g1, 2, 0, B, st));   // dZ4
    PP_TRY(conv_wgrad(net, o, g, 3, w.a[2], w.g1, B, w, grads, st));
    PP_TRY(conv_mfma(PP_PROF_CNN_BWD + 4, w.g1, g.hin[3] - 2, g.win[3] - 2, 128, 128, w.wd[3], nullptr, w.a[2], w.g0, 2, 0, B, st));   // dZ3
    PP_TRY(conv_wgrad(net, o, g, 2, w.p1, w.g0, B, w, grads, st));
    PP_TRY(conv_mfma(PP_PROF_CNN_BWD + 6, w.g0, g.hin[2] - 2, g.win[2] - 2, 128, 64, w.wd[2], nullptr, nullptr, w.g1, 2, 0, B, st));   // dP1
    {
        const int H2 = g.hin[1] - 2, W2 = g.win[1] - 2;
        const int64_t n = (int64_t)B * H2 * W2 * 64;
        prof_begin(PP_PROF_CNN_BWD + 7, st);
        hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w.a[1], H2, W2, 64, w.g1, g.hp1, g.wp1, 0,
                           (int64_t)0, w.g0, n);                                                                // dZ2
        PP_LAUNCH_CHECK("maxpool_bwd");
        prof_end(PP_PROF_CNN_BWD + 7, 0.0, st);
    }
    PP_TRY(conv_wgrad(net, o, g, 1, w.a[0], w.g0, B, w, grads, st));
    PP_TRY(conv_mfma(PP_PROF_CNN_BWD + 9, w.g0, g.hin[1] - 2, g.win[1] - 2, 64, 64, w.wd[1], nullptr, w.a[0], w.g1, 2, 0, B, st));     // dZ1
    {
        const int64_t M = (int64_t)B * (g.H - 2) * (g.W - 2);
        int64_t chunk;
        const int64_t wn = 9 * (int64_t)g.C * 64;
        const int S = wgrad_splits(M, wn, &chunk);
        float* dbp = w.part + S * wn;
        const dim3 grid(S), block(256);
        prof_begin(PP_PROF_CNN_BWD + 10, st);
        switch (g.C) {
            case 1: hipLaunchKernelGGL(conv1_wgrad_kernel<1>, grid, block, 0, st, w.a0, w.g1, w.part, dbp, g.H, g.W, M, chunk); break;
            case 2: hipLaunchKernelGGL(conv1_wgrad_kernel<2>, grid, block, 0, st, w.a0, w.g1, w.part, dbp, g.H, g.W, M, chunk); break;
            case 3: hipLaunchKernelGGL(conv1_wgrad_kernel<3>, grid, block, 0, st, w.a0, w.g1, w.part, dbp, g.H, g.W, M, chunk); break;
            default: hipLaunchKernelGGL(conv1_wgrad_kernel<4>, grid, block, 0, st, w.a0, w.g1, w.part, dbp, g.H, g.W, M, chunk); break;
        }
        PP_LAUNCH_CHECK("conv1_wgrad");
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(wn + 64, 256)), dim3(256), 0, st, w.part, dbp, S, g.C, 64,
                           grads + net->obs_conv_w[o][0], grads + net->obs_conv_b[o][0]);
        PP_LAUNCH_CHECK("wgrad_reduce");
        prof_end(PP_PROF_CNN_BWD + 10, 2.0 * (double)M * (double)wn, st);
    }
    return 0;
}

}  // namespace pp

extern "C" {

size_t pp_cnn2d5c_workspace_bytes(const pp_net* net, int32_t o, int32_t n_images) {
    return pp::cnn_workspace_bytes(net, o, n_images);
}

int pp_cnn2d5c_forward(const pp_net* net, int32_t o, const float* params, const float* x, int32_t n_images,
                       float* features_out, void* workspace, size_t workspace_bytes, void* stream) {
    pp::CnnGeom g;
    PP_CHECK_ARG(pp::cnn_geom(net, o, g), "pp_cnn2d5c_forward: observable %d is not a CNN2D5C embedding", o);
    return pp::cnn_forward(net, o, params, x, (int64_t)g.C * g.H * g.W, n_images, features_out, g.F, workspace, workspace_bytes,
                           true, pp::as_stream(stream));
}

int pp_cnn2d5c_backward(const pp_net* net, int32_t o, const float* params, const float* d_features, int32_t n_images,
                        float* grads, void* workspace, size_t workspace_bytes, int32_t flags, void* stream) {
    pp::CnnGeom g;
    PP_CHECK_ARG(pp::cnn_geom(net, o, g), "pp_cnn2d5c_backward: observable %d is not a CNN2D5C embedding", o);
    PP_CHECK_ARG(flags == 0, "pp_cnn2d5c_backward: flags must be 0");
    pp::grads_touch_all(grads);
    (void)params;      // (kept in the signature: the forward call's weight images are what backward reads)
    return pp::cnn_backward(net, o, d_features, g.F, n_images, grads, workspace, workspace_bytes, pp::as_stream(stream));
}

}  // extern "C"
