// CNN2D5C observe embedding (cnn2d.hip): the convolution stack of pyprob's EmbeddingCNN2D5C
// (pyprob/nn/embedding_cnn_2d_5c.py) from the image to the [B, F] feature matrix, and back.
#pragma once
#include "common.hpp"

namespace pp {

// Geometry of one CNN2D5C observable: conv1 C->64, conv2 64->64, pool, conv3 64->128, conv4, conv5 128->128, pool.
struct CnnGeom {
    int C, H, W;
    int cin[5], cout[5], hin[5], win[5];   // per convolution: channels and INPUT size (output = input - 2)
    int hp1, wp1, hp2, wp2;                // pooled sizes (floor)
    int F;                                 // 128 * hp2 * wp2
};
bool cnn_geom(const pp_net* net, int o, CnnGeom& g);

size_t cnn_workspace_bytes(const pp_net* net, int o, int B);
// x [B, C*H*W] rows of ldx floats (c, y, x order) -> feat [B, F] rows of ldf floats ((c, y, x) flatten order). The workspace keeps
// the images, the activations and the weight images; for_backward = false skips the flipped weight images that only
// cnn_backward reads (pp_is_init: no backward follows).
int cnn_forward(const pp_net* net, int o, const float* P, const float* x, int64_t ldx, int B, float* feat, int64_t ldf,
                void* ws, size_t ws_bytes, bool for_backward, hipStream_t st);
// dfeat [B, F] (lddf) -> grads of the five convolutions (added to the flat gradient buffer). Needs the workspace of a
// cnn_forward(..., for_backward = true) call with the same net, o and B.
int cnn_backward(const pp_net* net, int o, const float* dfeat, int64_t lddf, int B, float* grads, void* ws, size_t ws_bytes,
                 hipStream_t st);

}  // namespace pp
