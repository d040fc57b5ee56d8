"""The convolution stack of a CNN2D5C observe embedding on its own: pp_cnn2d5c_forward / pp_cnn2d5c_backward
(include/pyprob_amd.h, csrc/cnn2d.hip) behind torch tensors. Tests and tools/cnn_embed_bench.py use it; training and
inference reach the same kernels through pp_ic_loss / pp_is_init."""
import ctypes as C

import torch

from . import lib as L


class CNN2D5CStack:
    """Image [B, C*H*W] -> features [B, F] of observable `name` of `spec`, and the gradients of conv1..5 from dFeatures.
    `params` / `grads` are flat float32 device buffers laid out by the spec (an ICEngine's, or any of that size)."""

    def __init__(self, spec, name, device='cuda:0'):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.HipLibraryError('pyprob_amd needs a ROCm device (torch.cuda.is_available() is False); there is '
                                    'no CPU fallback.')
        self.spec = spec
        self.o = [o[0] for o in spec.obs].index(name)
        if spec.obs_kind[name] != L.PP_OBS_CNN2D5C:
            raise ValueError('observable %s is not a CNN2D5C embedding' % name)
        self.device = torch.device(device)
        self.net = spec.c_struct(None)
        self.width = spec.obs[self.o][1]
        self.F = spec.obs_feat[name]
        self.workspace = None
        self.ws_bytes = 0
        self.ws_images = 0

    def workspace_bytes(self, n_images):
        return int(self.lib.pp_cnn2d5c_workspace_bytes(C.byref(self.net), self.o, int(n_images)))

    def _ensure(self, n_images):
        if n_images != self.ws_images:       # (the carve depends on the image count: backward reads what forward placed)
            need = self.workspace_bytes(n_images)
            if need == 0:
                raise RuntimeError('pp_cnn2d5c_workspace_bytes failed')
            self.workspace = torch.zeros(need, dtype=torch.uint8, device=self.device)
            self.ws_bytes, self.ws_images = need, n_images

    def forward(self, params, x):
        x = x.to(self.device, torch.float32).reshape(-1, self.width).contiguous()
        B = x.shape[0]
        self._ensure(B)
        feat = torch.empty(B, self.F, dtype=torch.float32, device=self.device)
        L.check(self.lib.pp_cnn2d5c_forward(C.byref(self.net), self.o, params.data_ptr(), x.data_ptr(), B, feat.data_ptr(),
                                            self.workspace.data_ptr(), self.ws_bytes, L.stream_ptr()), 'pp_cnn2d5c_forward')
        return feat

    def backward(self, params, d_features, grads):
        """Adds the gradients of the five convolutions to `grads`; must follow forward() on the same images."""
        d = d_features.to(self.device, torch.float32).reshape(-1, self.F).contiguous()
        if d.shape[0] != self.ws_images:
            raise ValueError('backward of %d images after a forward of %d' % (d.shape[0], self.ws_images))
        L.check(self.lib.pp_cnn2d5c_backward(C.byref(self.net), self.o, params.data_ptr(), d.data_ptr(), d.shape[0],
                                             grads.data_ptr(), self.workspace.data_ptr(), self.ws_bytes, 0, L.stream_ptr()),
                'pp_cnn2d5c_backward')
