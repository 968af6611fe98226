// SSIM of a batch of image pairs in one pass: the `pytorch_ssim.ssim(rgb_map, var.image)` of the evaluation loop
// (model/nerf.py:550).  As stock ops that is five grouped conv2d calls (padding 5, an 11x11 window) and ~20 element-wise
// launches per image, in fp32, where the cancellation in E[x^2] - mu^2 costs four digits per pixel.  Here one launch stages a
// halo tile of both images in LDS, filters the five moments separably (11 + 11 taps) and evaluates the formula, everything
// after the fp32 loads in fp64; a second launch adds the per-workgroup partial sums of a view in a fixed order.  No atomics:
// the result is the same bits run to run, in either JT_DETERMINISTIC setting.
#include "jt_common.h"

namespace jt {

constexpr int kSsimTaps = 11, kSsimPad = 5;
constexpr int kSsimTW = 32, kSsimTH = 16;              // pixels of one workgroup's tile
constexpr int kSsimHW = kSsimTW + 2 * kSsimPad;        // 42: halo tile width
constexpr int kSsimHH = kSsimTH + 2 * kSsimPad;        // 26: halo tile height
constexpr int kSsimThreads = 256;

// g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, built as a float tensor and divided by its float sum: the package's 1-D
// window to the bit (hex literals: torch's vectorised sum of the eleven floats is not the sequential one).  The 2-D window is the
// outer product of these taps; in fp64 the separable form is that product up to the rounding of the sums.
__device__ constexpr double kSsimG[kSsimTaps] = {
    0x1.0d956cp-10, 0x1.f1fe02p-8, 0x1.26eb18p-5, 0x1.bff0fep-4, 0x1.b43c3ep-3, 0x1.10656p-2,
    0x1.b43c3ep-3,  0x1.bff0fep-4, 0x1.26eb18p-5, 0x1.f1fe02p-8, 0x1.0d956cp-10};

// the formula on the five filtered moments, every operation rounded on its own (no contraction): an identical pair then has a
// numerator and a denominator of the same bits and gives exactly 1
__device__ inline double ssim_pixel(double mu1, double mu2, double e11, double e22, double e12) {
#pragma clang fp contract(off)
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
  const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
  return ((2.0 * m12 + C1) * (2.0 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2));
}

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid (tiles along W, tiles along H, V * C); partial[(z * gridDim.y + y) * gridDim.x + x] = sum of the tile's ssim_map
__global__ __launch_bounds__(kSsimThreads) void k_ssim_tiles(const float* __restrict__ pred, const float* __restrict__ target,
                                                             int H, int W, double* __restrict__ partial,
                                                             float* __restrict__ map) {
  __shared__ float s_x[kSsimHH * kSsimHW], s_y[kSsimHH * kSsimHW];   // 2 x 4 368 B
  __shared__ double s_h[5][kSsimHH][kSsimTW];                        // 33 280 B: the row-filtered moments
  __shared__ double s_red[kSsimThreads / 64];
  const int x0 = blockIdx.x * kSsimTW, y0 = blockIdx.y * kSsimTH;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const float* __restrict__ px = pred + plane;
  const float* __restrict__ py = target + plane;
  // zero padding: what lies outside the image enters the sums as 0 and the window is not renormalised (conv2d(padding=5))
  for (int i = threadIdx.x; i < kSsimHH * kSsimHW; i += kSsimThreads) {
    const int r = i / kSsimHW, c = i - r * kSsimHW;
    const int yy = y0 + r - kSsimPad, xx = x0 + c - kSsimPad;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const size_t o = in ? (size_t)yy * W + xx : 0;
    s_x[i] = in ? px[o] : 0.f;
    s_y[i] = in ? py[o] : 0.f;
  }
  __syncthreads();
  // along W: consecutive lanes read consecutive words of a halo row and write consecutive doubles
  for (int i = threadIdx.x; i < kSsimHH * kSsimTW; i += kSsimThreads) {
    const int r = i / kSsimTW, c = i - r * kSsimTW;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0., a4 = 0.;
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const double u = (double)s_x[r * kSsimHW + c + k], v = (double)s_y[r * kSsimHW + c + k], g = kSsimG[k];
      a0 += g * u;
      a1 += g * v;
      a2 += g * (u * u);   // (the product of two floats is exact in fp64)
      a3 += g * (v * v);
      a4 += g * (u * v);
    }
    s_h[0][r][c] = a0;
    s_h[1][r][c] = a1;
    s_h[2][r][c] = a2;
    s_h[3][r][c] = a3;
    s_h[4][r][c] = a4;
  }
  __syncthreads();
  // along H, the formula, and this thread's share of the tile sum (its pixels in a fixed order)
  double sum = 0.;
  for (int i = threadIdx.x; i < kSsimTH * kSsimTW; i += kSsimThreads) {
    const int r = i / kSsimTW, c = i - r * kSsimTW;
    const int yy = y0 + r, xx = x0 + c;
    if (yy >= H || xx >= W) continue;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0., a4 = 0.;
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const double g = kSsimG[k];
      a0 += g * s_h[0][r + k][c];
      a1 += g * s_h[1][r + k][c];
      a2 += g * s_h[2][r + k][c];
      a3 += g * s_h[3][r + k][c];
      a4 += g * s_h[4][r + k][c];
    }
    const double v = ssim_pixel(a0, a1, a2, a3, a4);
    sum += v;
    if (map) map[plane + (size_t)yy * W + xx] = (float)v;
  }
  sum = wave_sum_f64(sum);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.;
    for (int w = 0; w < kSsimThreads / 64; ++w) t += s_red[w];
    partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
  }
}

// one workgroup per view: its per_view partials (contiguous: channel, tile row, tile column) in a fixed order, then the mean
__global__ __launch_bounds__(kSsimThreads) void k_ssim_finish(const double* __restrict__ partial, int per_view, double count,
                                                              double* __restrict__ ssim) {
  __shared__ double s_red[kSsimThreads / 64];
  const double* __restrict__ p = partial + (size_t)blockIdx.x * per_view;
  double sum = 0.;
  for (int i = threadIdx.x; i < per_view; i += kSsimThreads) sum += p[i];
  sum = wave_sum_f64(sum);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.;
    for (int w = 0; w < kSsimThreads / 64; ++w) t += s_red[w];
    ssim[blockIdx.x] = t / count;
  }
}

static bool ssim_shape(int V, int C, int H, int W, long* tiles_x, long* tiles_y) {
  if (V < 1 || C < 1 || H < 1 || W < 1) return false;
  *tiles_x = ((long)W + kSsimTW - 1) / kSsimTW;
  *tiles_y = ((long)H + kSsimTH - 1) / kSsimTH;
  return true;
}

}  // namespace jt

using namespace jt;

extern "C" size_t jt_ssim_workspace_bytes(int n_views, int n_channels, int height, int width) {
  long tx, ty;
  if (!ssim_shape(n_views, n_channels, height, width, &tx, &ty)) return 0;
  return (size_t)tx * (size_t)ty * (size_t)n_views * (size_t)n_channels * sizeof(double);
}

extern "C" int jt_ssim_forward(const float* pred, const float* target, int n_views, int n_channels, int height, int width,
                               double* ssim, float* ssim_map, void* workspace, size_t workspace_bytes, void* stream) {
  long tx, ty;
  if (!pred || !target || !ssim || !workspace || !ssim_shape(n_views, n_channels, height, width, &tx, &ty)) return JT_ERR_ARG;
  const long planes = (long)n_views * n_channels;
  if ((double)planes * (double)height * (double)width >= 2147483648.0 || planes > 65535 || ty > 65535 ||
      tx * ty * n_channels >= (1l << 31))
    return JT_ERR_UNSUPPORTED;
  if (workspace_bytes < jt_ssim_workspace_bytes(n_views, n_channels, height, width)) return JT_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(k_ssim_tiles, dim3((unsigned)tx, (unsigned)ty, (unsigned)planes), dim3(kSsimThreads), 0, st, pred, target,
                     height, width, partial, ssim_map);
  JT_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ssim_finish, dim3(n_views), dim3(kSsimThreads), 0, st, (const double*)partial,
                     (int)(tx * ty * n_channels), (double)n_channels * (double)height * (double)width, ssim);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
