// Internal C++ launch entry points of the image encoder's training kernels (image_train_kernels.hip).
// Public C ABI: include/gmf_hip.h (gmf_conv2d_forward_f32, gmf_conv2d_dgrad, gmf_conv2d_wgrad, gmf_maxpool3x3s2_forward,
// gmf_maxpool3x3s2_backward, gmf_batchnorm_residual_forward).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gmf {

// One convolution of the ResNet-34 -> layer2 encoder: x [B, H, W, cin] -> y [B, Ho, Wo, cout], pad = ks / 2, weights as the
// nn.Conv2d parameter [cout, cin, ks, ks].  The five shapes: (3, 64, 7, 2) the stem, (64, 64, 3, 1), (128, 128, 3, 1),
// (64, 128, 3, 2), (64, 128, 1, 2).
struct Conv2dShape {
  int B, H, W, cin, cout, ks, stride;
  int pad() const { return ks / 2; }
  int Ho() const { return (H + 2 * pad() - ks) / stride + 1; }
  int Wo() const { return (W + 2 * pad() - ks) / stride + 1; }
  long long in_pixels() const { return (long long)B * H * W; }
  long long out_pixels() const { return (long long)B * Ho() * Wo(); }
  size_t weight_floats() const { return (size_t)cout * cin * ks * ks; }
  bool stem() const { return cin == 3; }
};
bool conv2d_shape_ok(const Conv2dShape& s);

// Forward and dgrad run ONE kernel, k_conv2d_f32<K, N, KS, ST, DG>: out[p][n] = sum over taps and k of in[src(p, tap)][k] *
// Wp[tap][n][k] (+ add[p][n]).  Forward: p an output pixel, src = p * ST + tap - pad.  dgrad (DG): p an INPUT pixel, src the
// output pixel (p + pad - tap) / ST where that division is exact and in range - a gather, every dx entry written.  Wp
// (weight_floats() floats of workspace) is the weight permuted by k_conv_wperm so that the contraction index is contiguous.
// The stem forward (k_stem_f32) reads the image through its element strides (sb, sc, sh, sw).
hipError_t launch_conv2d_forward(const Conv2dShape& s, const float* x, long long sb, long long sc, long long sh, long long sw,
                                 const float* w, float* wp, float* y, hipStream_t st);
hipError_t launch_conv2d_dgrad(const Conv2dShape& s, const float* dy, const float* w, float* wp, const float* dx_add, float* dx,
                               hipStream_t st);

// wgrad: dW[co][ci][tap] = sum over output pixels p of dy[p][co] * x[p * ST + tap - pad][ci].  The pixel range is cut into
// conv2d_wgrad_slabs(s) equal chunks; a one-wave workgroup per (tap, 64 x 64 tile of dW, chunk) writes its partial sum in dW's
// own layout into part[chunk], k_conv_wgrad_reduce adds the chunks in index order.  The count depends on the shape alone.
int conv2d_wgrad_slabs(const Conv2dShape& s);
hipError_t launch_conv2d_wgrad(const Conv2dShape& s, const float* x, long long sb, long long sc, long long sh, long long sw,
                               const float* dy, float* part, float* dw, hipStream_t st);

// Max-pool 3 x 3 stride 2 pad 1 on NHWC (C % 4 == 0).  Backward: every input pixel gathers dy of the at most four windows
// whose argmax (recomputed from x; first maximum in row-major window order) it is.
hipError_t launch_maxpool_fwd(const float* x, float* y, int B, int H, int W, int C, hipStream_t st);
hipError_t launch_maxpool_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, hipStream_t st);

}  // namespace gmf
