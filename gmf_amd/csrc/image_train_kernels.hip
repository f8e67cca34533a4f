// Training kernels of the image encoder (ResNet-34 -> layer2, GMF_PointDSC/models/resnet.py:36-75,195-216 in train()):
// what forward + backward of its convolutions and its max-pool need beyond train_kernels.hip, on dense NHWC fp32
// activations (an NHWC activation IS a rows x channels matrix: BatchNorm, ReLU and the column sums come from there).
//   k_conv_wperm          the nn.Conv2d parameter [cout, cin, ks, ks] -> the operand order of the kernel that reads it
//   k_conv2d_f32          forward of the four layer1 / layer2 shapes and, as a gather, their dgrad
//   k_stem_f32            forward of the 3 -> 64 7x7 stride-2 stem, the image read through its strides
//   k_conv2d_wgrad        dW of the four shapes, pixel range split over workgroups, partial slabs
//   k_stem_wgrad          dW of the stem (K = 147 taps x 64 outputs)
//   k_conv_wgrad_reduce   the slabs added in index order
//   k_maxpool_fwd / _bwd  max-pool 3x3 stride 2 pad 1; the backward a gather that recomputes each window's argmax
// Every contraction runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, a k-ordered fma chain): no operand ranges to
// guard, no weight image to re-pack per optimiser step.  No float atomics: every sum has one fixed order, so two runs give
// the same bits.  MFMA operand layout as in train_kernels.hip: lane (h, i) = (lane >> 5, lane & 31) holds for its row
// (column) i the contraction index h of a 2-deep step; D register r of lane (h, j) is C[8 (r >> 2) + 4 h + (r & 3)][j].
#include <algorithm>

#include "mfma_core.hpp"
#include "launchers_image_train.hpp"

namespace gmf {

namespace {
inline unsigned blocks_of_256(size_t total) { return (unsigned)((total + 255) / 256); }
}  // namespace

// mode 0 (forward): Wp[tap][co][ci]; mode 1 (dgrad): Wp[tap][ci][co]; mode 2 (stem): Wp[k][co], k = ci * kk + tap
__global__ void __launch_bounds__(256)
k_conv_wperm(const float* __restrict__ W, float* __restrict__ Wp, int cout, int cin, int kk, int mode) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= cout * cin * kk) return;
  int co, ci, tap;
  if (mode == 0) {
    ci = idx % cin; co = (idx / cin) % cout; tap = idx / (cin * cout);
  } else if (mode == 1) {
    co = idx % cout; ci = (idx / cout) % cin; tap = idx / (cin * cout);
  } else {
    co = idx % cout;
    const int k = idx / cout;
    ci = k / kk; tap = k - ci * kk;
  }
  Wp[idx] = W[((size_t)co * cin + ci) * kk + tap];
}

// =========================================================================================
// k_conv2d_f32<K, N, KS, ST, DG>: out [B, Ho, Wo, N] from in [B, Hi, Wi, K] and Wp [KS * KS][N][K].
//   DG = false (forward): source pixel of output (oy, ox) and tap (ky, kx) is (oy ST + ky - pad, ox ST + kx - pad).
//   DG = true (dgrad):    `out` is dx on the convolution's input grid, `in` is dy on its output grid; input pixel (y, x)
//                         takes tap (ky, kx) from output pixel ((y + pad - ky) / ST, (x + pad - kx) / ST) when both
//                         divisions are exact and the result exists.  A pixel no tap reaches gets 0 (+ add).
//   A workgroup is 4 waves; a wave owns 64 pixels x 64 channels (2 x 2 MFMA blocks), operands global -> registers with
//   16-byte loads (lane (h, i): its pixel's / channel's 8 contraction indices k0 + 8 h .. + 7 of a 16-wide k-step).
//   grid (ceil(P / 256), N / 64), block 256.
// =========================================================================================
template <int K, int N, int KS, int ST, bool DG>
__global__ void __launch_bounds__(256)
k_conv2d_f32(const float* __restrict__ in, const float* __restrict__ Wp, const float* __restrict__ add, float* __restrict__ out,
             int P, int Hi, int Wi, int Ho, int Wo) {
  constexpr int PAD = KS / 2;
  const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31, wave = threadIdx.x >> 6;
  const int m0 = (blockIdx.x * 4 + wave) * 64, n0 = blockIdx.y * 64;
  if (m0 >= P) return;
  int pb[2], py[2], px[2];
  bool pok[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int p = m0 + 32 * rb + i;
    pok[rb] = p < P;
    const int pc = min(p, P - 1);
    pb[rb] = pc / (Ho * Wo);
    const int r = pc - pb[rb] * (Ho * Wo);
    py[rb] = r / Wo;
    px[rb] = r - py[rb] * Wo;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = zero16();
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
  for (int tap = 0; tap < KS * KS; ++tap) {
    const int ky = tap / KS, kx = tap - ky * KS;
    const float4* pa[2];
    bool ok[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      int sy, sx;
      bool v = pok[rb];
      if (DG) {
        const int ty = py[rb] + PAD - ky, tx = px[rb] + PAD - kx;
        v = v && ty >= 0 && tx >= 0 && (ty % ST) == 0 && (tx % ST) == 0;
        sy = ty / ST;
        sx = tx / ST;
      } else {
        sy = py[rb] * ST + ky - PAD;
        sx = px[rb] * ST + kx - PAD;
      }
      v = v && sy >= 0 && sy < Hi && sx >= 0 && sx < Wi;
      ok[rb] = v;
      const size_t pix = v ? ((size_t)pb[rb] * Hi + sy) * Wi + sx : 0;
      pa[rb] = reinterpret_cast<const float4*>(in + pix * K + 8 * h);
    }
    const float4* pw[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
      pw[cb] = reinterpret_cast<const float4*>(Wp + ((size_t)tap * N + n0 + 32 * cb + i) * K + 8 * h);
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += 16) {
      float a[2][8], b[2][8];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const float4 u = ok[rb] ? pa[rb][k0 / 4] : z4, w = ok[rb] ? pa[rb][k0 / 4 + 1] : z4;
        a[rb][0] = u.x; a[rb][1] = u.y; a[rb][2] = u.z; a[rb][3] = u.w;
        a[rb][4] = w.x; a[rb][5] = w.y; a[rb][6] = w.z; a[rb][7] = w.w;
      }
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const float4 u = pw[cb][k0 / 4], w = pw[cb][k0 / 4 + 1];
        b[cb][0] = u.x; b[cb][1] = u.y; b[cb][2] = u.z; b[cb][3] = u.w;
        b[cb][4] = w.x; b[cb][5] = w.y; b[cb][6] = w.z; b[cb][7] = w.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = mfma32(a[rb][e], b[cb][e], acc[rb][cb]);
    }
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int col = n0 + 32 * cb + i;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = m0 + 32 * rb + 8 * (r >> 2) + 4 * h + (r & 3);
        if (p >= P) continue;
        const size_t o = (size_t)p * N + col;
        out[o] = add ? acc[rb][cb][r] + add[o] : acc[rb][cb][r];
      }
    }
}

// =========================================================================================
// k_stem_f32: y [B, Ho, Wo, 64] = conv 7x7 stride 2 pad 3 of the image x (element strides sb, sc, sh, sw), Wp [147][64] with
// k = c 49 + ky 7 + kx (the parameter's own order).  A wave owns 32 pixels x 64 channels; lane (h, i) gathers for pixel i the
// 8 image values k0 + 8 h .. + 7 of each of the 10 16-wide k-steps (k >= 147 contributes 0).  grid ceil(P / 128), block 256.
// =========================================================================================
__global__ void __launch_bounds__(256)
k_stem_f32(const float* __restrict__ x, long sb, long sc, long sh, long sw, const float* __restrict__ Wp, float* __restrict__ y,
           int P, int H, int W, int Ho, int Wo) {
  const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31, wave = threadIdx.x >> 6;
  const int m0 = (blockIdx.x * 4 + wave) * 32;
  if (m0 >= P) return;
  const int p = m0 + i;
  const bool pok = p < P;
  const int pc = min(p, P - 1);
  const int b = pc / (Ho * Wo), r0 = pc - b * (Ho * Wo), oy = r0 / Wo, ox = r0 - oy * Wo;
  const int iy0 = oy * 2 - 3, ix0 = ox * 2 - 3;
  const float* xb = x + (size_t)b * sb;
  f32x16 acc[2] = {zero16(), zero16()};
#pragma unroll 1
  for (int k0 = 0; k0 < 160; k0 += 16) {
    float a[8], w[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + 8 * h + e;
      const int c = k / 49, r = k - 49 * c, ky = r / 7, kx = r - 7 * ky;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = pok && k < 147 && iy >= 0 && iy < H && ix >= 0 && ix < W;
      a[e] = ok ? xb[(long)c * sc + (long)iy * sh + (long)ix * sw] : 0.f;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) w[cb][e] = k < 147 ? Wp[k * 64 + 32 * cb + i] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) acc[cb] = mfma32(a[e], w[cb][e], acc[cb]);
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = m0 + 8 * (r >> 2) + 4 * h + (r & 3);
      if (q < P) y[(size_t)q * 64 + 32 * cb + i] = acc[cb][r];
    }
}

// =========================================================================================
// k_conv2d_wgrad<CI, CO, KS, ST>: one wave per workgroup; blockIdx.x = tap, blockIdx.y = 64 x 64 tile of dW[.][.][tap]
// (rows co, columns ci), blockIdx.z = pixel chunk [z chunk, (z + 1) chunk) of the P output pixels (chunk even).  MFMA step t
// contracts the pixel pair pbeg + 2 t + h: A = dy[p][co], B = x[src(p, tap)][ci] (0 outside the image), both coalesced over
// the channel.  The pixel's (b, oy, ox) advances incrementally.  Writes part[z][co][ci][tap] (dW's layout).
// =========================================================================================
template <int CI, int CO, int KS, int ST>
__global__ void __launch_bounds__(64)
k_conv2d_wgrad(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, int P, int chunk, int H, int W,
               int Ho, int Wo) {
  constexpr int PAD = KS / 2, KK = KS * KS;
  const int lane = threadIdx.x, h = lane >> 5, i = lane & 31;
  const int tap = blockIdx.x, ky = tap / KS, kx = tap - ky * KS;
  const int co0 = (blockIdx.y / (CI / 64)) * 64, ci0 = (blockIdx.y % (CI / 64)) * 64;
  const int pbeg = blockIdx.z * chunk, pend = min(P, pbeg + chunk);
  f32x16 acc[2][2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = zero16();
  int p = pbeg + h;
  int b = p / (Ho * Wo), r0 = p - b * (Ho * Wo), oy = r0 / Wo, ox = r0 - oy * Wo;
  for (; p - h < pend; p += 2) {
    const bool pok = p < pend;
    const int iy = oy * ST + ky - PAD, ix = ox * ST + kx - PAD;
    const bool xok = pok && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const float* dyp = dy + (size_t)(pok ? p : 0) * CO + co0 + i;
    const float* xp = x + (xok ? ((size_t)b * H + iy) * W + ix : 0) * CI + ci0 + i;
    float a[2], bv[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) a[rb] = pok ? dyp[32 * rb] : 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) bv[cb] = xok ? xp[32 * cb] : 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = mfma32(a[rb], bv[cb], acc[rb][cb]);
    ox += 2;
    while (ox >= Wo) { ox -= Wo; ++oy; }
    while (oy >= Ho) { oy -= Ho; ++b; }
  }
  float* dst = part + (size_t)blockIdx.z * CO * CI * KK;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + 32 * rb + 8 * (r >> 2) + 4 * h + (r & 3), ci = ci0 + 32 * cb + i;
        dst[((size_t)co * CI + ci) * KK + tap] = acc[rb][cb][r];
      }
}

// =========================================================================================
// k_stem_wgrad: dW [64][147] of the stem, one wave per pixel chunk (blockIdx.x): rows co (2 blocks), columns k = c 49 + ky 7
// + kx (5 blocks, k >= 147 unused), 10 accumulators.  Lane (h, j) keeps the tap of its 5 columns; MFMA step t contracts the
// pixel pair pbeg + 2 t + h: A = dy[p][co], B = the image value the tap reads for pixel p (0 outside).  part[z][co][k].
// =========================================================================================
__global__ void __launch_bounds__(64)
k_stem_wgrad(const float* __restrict__ x, long sb, long sc, long sh, long sw, const float* __restrict__ dy, float* __restrict__ part,
             int P, int chunk, int H, int W, int Ho, int Wo) {
  const int lane = threadIdx.x, h = lane >> 5, i = lane & 31;
  const int pbeg = blockIdx.x * chunk, pend = min(P, pbeg + chunk);
  long koff[5];
  int kyv[5], kxv[5];
  bool kok[5];
#pragma unroll
  for (int cb = 0; cb < 5; ++cb) {
    const int k = 32 * cb + i;
    const int c = k / 49, r = k - 49 * c;
    kok[cb] = k < 147;
    kyv[cb] = r / 7;
    kxv[cb] = r - 7 * kyv[cb];
    koff[cb] = (long)c * sc;
  }
  f32x16 acc[2][5];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 5; ++cb) acc[rb][cb] = zero16();
  int p = pbeg + h;
  int b = p / (Ho * Wo), r0 = p - b * (Ho * Wo), oy = r0 / Wo, ox = r0 - oy * Wo;
  for (; p - h < pend; p += 2) {
    const bool pok = p < pend;
    const float* dyp = dy + (size_t)(pok ? p : 0) * 64 + i;
    const float* xb = x + (size_t)(pok ? b : 0) * sb;
    float a[2], bv[5];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) a[rb] = pok ? dyp[32 * rb] : 0.f;
#pragma unroll
    for (int cb = 0; cb < 5; ++cb) {
      const int iy = oy * 2 - 3 + kyv[cb], ix = ox * 2 - 3 + kxv[cb];
      const bool ok = pok && kok[cb] && iy >= 0 && iy < H && ix >= 0 && ix < W;
      bv[cb] = ok ? xb[koff[cb] + (long)iy * sh + (long)ix * sw] : 0.f;
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 5; ++cb) acc[rb][cb] = mfma32(a[rb], bv[cb], acc[rb][cb]);
    ox += 2;
    while (ox >= Wo) { ox -= Wo; ++oy; }
    while (oy >= Ho) { oy -= Ho; ++b; }
  }
  float* dst = part + (size_t)blockIdx.x * 64 * 147;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 5; ++cb) {
      const int k = 32 * cb + i;
      if (k >= 147) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = 32 * rb + 8 * (r >> 2) + 4 * h + (r & 3);
        dst[co * 147 + k] = acc[rb][cb][r];
      }
    }
}

// dW[e] = part[0][e] + part[1][e] + ... in slab order
__global__ void __launch_bounds__(256)
k_conv_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dW, int total, int nslab) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float s = part[e];
  for (int z = 1; z < nslab; ++z) s += part[(size_t)z * total + e];
  dW[e] = s;
}

// =========================================================================================
// Max-pool 3x3 stride 2 pad 1 on NHWC, a thread per (pixel, 4 channels).  The argmax of a window is its first maximum in
// row-major order (torch: a later element replaces the running maximum only when strictly greater).
// =========================================================================================
GMF_DEVINL float f4_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

__global__ void __launch_bounds__(256)
k_maxpool_fwd(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int Ho, int Wo, int C4) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * Ho * Wo * C4) return;
  const int c4 = (int)(idx % C4);
  const size_t pix = idx / C4;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((size_t)Wo * Ho));
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4 m;
  bool first = true;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * 2 - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * 2 - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const float4 v = x4[(((size_t)b * H + iy) * W + ix) * C4 + c4];
      if (first) { m = v; first = false; }
      else { m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w; }
    }
  }
  reinterpret_cast<float4*>(y)[idx] = m;
}

__global__ void __launch_bounds__(256)
k_maxpool_bwd(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int B, int H, int W, int Ho, int Wo,
              int C4) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * H * W * C4) return;
  const int c4 = (int)(idx % C4);
  const size_t pix = idx / C4;
  const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* dy4 = reinterpret_cast<const float4*>(dy);
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  // windows (oy, ox) that cover (iy, ix): oy 2 - 1 <= iy <= oy 2 + 1
  for (int oy = max(0, iy / 2); oy <= min(Ho - 1, (iy + 1) / 2); ++oy)
    for (int ox = max(0, ix / 2); ox <= min(Wo - 1, (ix + 1) / 2); ++ox) {
      float best[4];
      int arg[4];
      bool first = true;
      for (int ky = 0; ky < 3; ++ky) {
        const int y2 = oy * 2 - 1 + ky;
        if (y2 < 0 || y2 >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int x2 = ox * 2 - 1 + kx;
          if (x2 < 0 || x2 >= W) continue;
          const float4 v = x4[(((size_t)b * H + y2) * W + x2) * C4 + c4];
          const int at = y2 * W + x2;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float ve = f4_get(v, e);
            if (first || ve > best[e]) { best[e] = ve; arg[e] = at; }
          }
          first = false;
        }
      }
      const float4 d = dy4[(((size_t)b * Ho + oy) * Wo + ox) * C4 + c4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (arg[e] == iy * W + ix) g[e] += f4_get(d, e);
    }
  reinterpret_cast<float4*>(dx)[idx] = make_float4(g[0], g[1], g[2], g[3]);
}

// ---- launchers --------------------------------------------------------------------------------------------------------
bool conv2d_shape_ok(const Conv2dShape& s) {
  const int f[5][4] = {{3, 64, 7, 2}, {64, 64, 3, 1}, {128, 128, 3, 1}, {64, 128, 3, 2}, {64, 128, 1, 2}};
  for (const auto& e : f)
    if (s.cin == e[0] && s.cout == e[1] && s.ks == e[2] && s.stride == e[3]) return true;
  return false;
}

static hipError_t wperm(const Conv2dShape& s, const float* w, float* wp, int mode, hipStream_t st) {
  hipLaunchKernelGGL(k_conv_wperm, dim3(blocks_of_256(s.weight_floats())), dim3(256), 0, st, w, wp, s.cout, s.cin, s.ks * s.ks, mode);
  return hipGetLastError();
}

template <int K, int N, int KS, int ST, bool DG>
static hipError_t conv_launch(const float* in, const float* wp, const float* add, float* out, int P, int Hi, int Wi, int Ho, int Wo,
                              hipStream_t st) {
  hipLaunchKernelGGL((k_conv2d_f32<K, N, KS, ST, DG>), dim3((P + 255) / 256, N / 64), dim3(256), 0, st, in, wp, add, out, P, Hi, Wi,
                     Ho, Wo);
  return hipGetLastError();
}

hipError_t launch_conv2d_forward(const Conv2dShape& s, const float* x, long long sb, long long sc, long long sh, long long sw,
                                 const float* w, float* wp, float* y, hipStream_t st) {
  const int P = (int)s.out_pixels(), Ho = s.Ho(), Wo = s.Wo();
  if (hipError_t e = wperm(s, w, wp, s.stem() ? 2 : 0, st)) return e;
  if (s.stem()) {
    hipLaunchKernelGGL(k_stem_f32, dim3((P + 127) / 128), dim3(256), 0, st, x, (long)sb, (long)sc, (long)sh, (long)sw, wp, y, P, s.H,
                       s.W, Ho, Wo);
    return hipGetLastError();
  }
  if (s.cin == 64 && s.cout == 64) return conv_launch<64, 64, 3, 1, false>(x, wp, nullptr, y, P, s.H, s.W, Ho, Wo, st);
  if (s.cin == 128) return conv_launch<128, 128, 3, 1, false>(x, wp, nullptr, y, P, s.H, s.W, Ho, Wo, st);
  if (s.ks == 3) return conv_launch<64, 128, 3, 2, false>(x, wp, nullptr, y, P, s.H, s.W, Ho, Wo, st);
  return conv_launch<64, 128, 1, 2, false>(x, wp, nullptr, y, P, s.H, s.W, Ho, Wo, st);
}

hipError_t launch_conv2d_dgrad(const Conv2dShape& s, const float* dy, const float* w, float* wp, const float* dx_add, float* dx,
                               hipStream_t st) {
  const int P = (int)s.in_pixels(), Ho = s.Ho(), Wo = s.Wo();
  if (hipError_t e = wperm(s, w, wp, 1, st)) return e;
  // contraction over cout, output channels cin; `out` grid = the convolution's input, `in` grid = its output
  if (s.cin == 64 && s.cout == 64) return conv_launch<64, 64, 3, 1, true>(dy, wp, dx_add, dx, P, Ho, Wo, s.H, s.W, st);
  if (s.cin == 128) return conv_launch<128, 128, 3, 1, true>(dy, wp, dx_add, dx, P, Ho, Wo, s.H, s.W, st);
  if (s.ks == 3) return conv_launch<128, 64, 3, 2, true>(dy, wp, dx_add, dx, P, Ho, Wo, s.H, s.W, st);
  return conv_launch<128, 64, 1, 2, true>(dy, wp, dx_add, dx, P, Ho, Wo, s.H, s.W, st);
}

// chunks of at least 256 pixels, about 2048 waves over taps x tiles x chunks, at most 256 chunks
int conv2d_wgrad_slabs(const Conv2dShape& s) {
  const long long P = s.out_pixels();
  const int groups = s.stem() ? 1 : s.ks * s.ks * (s.cout / 64) * (s.cin / 64);
  const long long cap = std::min<long long>(256, std::max<long long>(1, 2048 / groups));
  return (int)std::max<long long>(1, std::min<long long>(cap, (P + 255) / 256));
}

template <int CI, int CO, int KS, int ST>
static hipError_t wgrad_launch(const float* x, const float* dy, float* part, int P, int chunk, int nslab, int H, int W, int Ho, int Wo,
                               hipStream_t st) {
  hipLaunchKernelGGL((k_conv2d_wgrad<CI, CO, KS, ST>), dim3(KS * KS, (CO / 64) * (CI / 64), nslab), dim3(64), 0, st, x, dy, part, P,
                     chunk, H, W, Ho, Wo);
  return hipGetLastError();
}

hipError_t launch_conv2d_wgrad(const Conv2dShape& s, const float* x, long long sb, long long sc, long long sh, long long sw,
                               const float* dy, float* part, float* dw, hipStream_t st) {
  const int P = (int)s.out_pixels(), Ho = s.Ho(), Wo = s.Wo();
  int nslab = conv2d_wgrad_slabs(s);
  const int chunk = ((P + nslab - 1) / nslab + 1) / 2 * 2;          // even: an MFMA step contracts a pixel pair
  nslab = (P + chunk - 1) / chunk;                                    // (never more than planned: no empty chunk)
  hipError_t e;
  if (s.stem()) {
    hipLaunchKernelGGL(k_stem_wgrad, dim3(nslab), dim3(64), 0, st, x, (long)sb, (long)sc, (long)sh, (long)sw, dy, part, P, chunk, s.H,
                       s.W, Ho, Wo);
    e = hipGetLastError();
  } else if (s.cin == 64 && s.cout == 64) {
    e = wgrad_launch<64, 64, 3, 1>(x, dy, part, P, chunk, nslab, s.H, s.W, Ho, Wo, st);
  } else if (s.cin == 128) {
    e = wgrad_launch<128, 128, 3, 1>(x, dy, part, P, chunk, nslab, s.H, s.W, Ho, Wo, st);
  } else if (s.ks == 3) {
    e = wgrad_launch<64, 128, 3, 2>(x, dy, part, P, chunk, nslab, s.H, s.W, Ho, Wo, st);
  } else {
    e = wgrad_launch<64, 128, 1, 2>(x, dy, part, P, chunk, nslab, s.H, s.W, Ho, Wo, st);
  }
  if (e != hipSuccess) return e;
  const int total = (int)s.weight_floats();
  hipLaunchKernelGGL(k_conv_wgrad_reduce, dim3(blocks_of_256(total)), dim3(256), 0, st, part, dw, total, nslab);
  return hipGetLastError();
}

hipError_t launch_maxpool_fwd(const float* x, float* y, int B, int H, int W, int C, hipStream_t st) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(k_maxpool_fwd, dim3(blocks_of_256((size_t)B * Ho * Wo * (C / 4))), dim3(256), 0, st, x, y, B, H, W, Ho, Wo, C / 4);
  return hipGetLastError();
}

hipError_t launch_maxpool_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, hipStream_t st) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(k_maxpool_bwd, dim3(blocks_of_256((size_t)B * H * W * (C / 4))), dim3(256), 0, st, x, dy, dx, B, H, W, Ho, Wo,
                     C / 4);
  return hipGetLastError();
}

}  // namespace gmf
