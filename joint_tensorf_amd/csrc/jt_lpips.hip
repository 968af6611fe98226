// LPIPS with the AlexNet backbone, the `lpips.LPIPS(net="alex")(rgb_map * 2 - 1, image * 2 - 1)` of the evaluation loop
// (model/nerf.py:33,551), on the fp32-input matrix cores: five convolutions as implicit GEMMs, two max-pools, and the
// channel-normalised, linearly weighted squared difference of the five feature stacks in fp64.
//
// k_lpips_scale   pred and target [V][3][H][W] -> ONE batch [2V][3][H][W] (pictures 0..V-1 = pred, V..2V-1 = target), so every
//                 later layer is one launch for both pictures.  Per element, in fp32, each operation rounded on its own and in
//                 this order (no contraction):  t = 2 * x  (exact);  u = t - 1;  v = u - shift_c;  r = v / scale_c  (IEEE
//                 division), shift = (-.030, -.088, -.188), scale = (.458, .448, .450) rounded to fp32.  That is the sequence the
//                 stock ops run (`x * 2 - 1` at the call, `(inp - shift) / scale` in the package's scaling layer).
// k_conv_mfma     out = relu(conv2d(x, w) + b), NCHW fp32, as a GEMM with M = output channels, N = batch * OH * OW output pixels
//                 (flattened across pictures: a pixel tile may straddle two), K = Cin * KH * KW, on v_mfma_f32_32x32x2_f32.  The
//                 weights are read from the K-major image jt_conv_pack_weights writes ([Kpad][Cout], rows K..Kpad-1 zero); the B
//                 operand is gathered from the activation into LDS on the fly (no im2col in memory), taps outside the picture
//                 and rows k >= K as zeros.  An output element is ONE accumulator chain over k = (ci, ky, kx) ascending from 0:
//                 the matrix core's result is bit for bit the k-ordered fmaf chain, a zero product leaves the chain's value
//                 unchanged, there is no split-K and no atomic; the bias is one fp32 add after the chain, then ReLU.  So an
//                 element does not depend on the tile shape, on the workgroup count or on the other pictures of the batch.
// k_maxpool_3x3s2 floor mode, no padding, one lane per output element.
// k_lpips_head    per layer and pixel in fp64: n_i = sqrt(sum_c f_i^2) + 1e-10, sum_c lin_c (f0_c / n0 - f1_c / n1)^2; the pixel
//                 sum of a workgroup in a fixed order into a partial, and k_lpips_finish adds a layer's partials in a fixed
//                 order, divides by the pixel count and adds the five layers in ascending order.  No float atomics.
#include "jt_common.h"

namespace jt {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kConvBK = JT_CONV_K_STEP;   // k rows of one LDS stage: the same for every tile variant (Kpad is a multiple of it)
constexpr int kLpThreads = 256;
constexpr int kLpLayers = 5;

__device__ inline double lp_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- the scaling layer -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLpThreads) void k_lpips_scale(const float* __restrict__ pred, const float* __restrict__ target,
                                                            int per_side, int plane, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kLpThreads + threadIdx.x;   // index into one side: [V][3][H][W]
  if (i >= per_side) return;
  const int c = (i / plane) % 3;
  const float shift = c == 0 ? -.030f : c == 1 ? -.088f : -.188f;
  const float scale = c == 0 ? .458f : c == 1 ? .448f : .450f;
  const float* __restrict__ src = blockIdx.y == 0 ? pred : target;
  const float t = 2.0f * src[i];
  const float u = t - 1.0f;
  const float v = u - shift;
  out[(size_t)blockIdx.y * per_side + i] = __fdiv_rn(v, scale);
}

// ---- weights: [Cout][K] (torch's [Cout][Cin][KH][KW]) -> [Kpad][Cout], zero rows behind K ------------------------------------
__global__ __launch_bounds__(kLpThreads) void k_conv_pack(const float* __restrict__ w, int c_out, int K, int n,
                                                          float* __restrict__ packed) {
  const int i = blockIdx.x * kLpThreads + threadIdx.x;   // = k * c_out + m
  if (i >= n) return;
  const int k = i / c_out, m = i - k * c_out;
  packed[i] = k < K ? w[(size_t)m * K + k] : 0.f;
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------
// A workgroup of WM x WN waves owns 32 WM output channels x 32 WN pixels; each wave one 32 x 32 accumulator tile (16 registers).
// Per stage of kConvBK k rows: every thread fetches its share of the weight rows and of the gathered activation into registers,
// writes them to LDS ([k][m] and [k][n]: the lanes of a wave read and write consecutive words), and the fetch of stage s + 1 is
// in flight while the 16 MFMAs of stage s run.  grid (pixel tiles, Cout / (32 WM)).
template <int KH, int KW, int S, int P, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void k_conv_mfma(const float* __restrict__ x, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, float* __restrict__ out, int n_pix,
                                                            int Cin, int H, int W, int OH, int OW, int Cout, int n_stages) {
  constexpr int NT = 64 * WM * WN, BM = 32 * WM, BN = 32 * WN;
  constexpr int NA = kConvBK * BM / NT, NB = kConvBK * BN / NT;   // values per thread and stage: 16 / WN, 16 / WM
  constexpr int KA = NT / BM, KB = NT / BN;                       // k rows one pass of the workgroup covers
  constexpr int KHW = KH * KW;
  static_assert(NA * KA == kConvBK && NB * KB == kConvBK, "a stage is covered exactly");
  __shared__ float sA[kConvBK * BM], sB[kConvBK * BN];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int OHW = OH * OW;
  // this thread's weight column and gathered pixel: fixed for the whole k loop
  const int am = t % BM, ak = t / BM;
  const int bn = t % BN, bk = t / BN;
  const int gn = n0 + bn;
  const bool pix_ok = gn < n_pix;
  int iy0 = 0, ix0 = 0;
  const float* __restrict__ xim = x;
  if (pix_ok) {
    const int img = gn / OHW, rem = gn - img * OHW;
    const int oy = rem / OW, ox = rem - oy * OW;
    iy0 = oy * S - P;
    ix0 = ox * S - P;
    xim = x + (size_t)img * Cin * H * W;
  }
  float ra[NA], rb[NB];
  auto fetch = [&](int stage) {
    const int k0 = stage * kConvBK;
#pragma unroll
    for (int j = 0; j < NA; ++j) ra[j] = wp[(size_t)(k0 + ak + j * KA) * Cout + m0 + am];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = k0 + bk + j * KB;
      const int ci = k / KHW, r = k - ci * KHW;
      const int ky = r / KW, kx = r - ky * KW;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = pix_ok && ci < Cin && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      rb[j] = ok ? xim[((size_t)ci * H + iy) * W + ix] : 0.f;
    }
  };
  lp_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  fetch(0);
  const int half = lane >> 5, col = lane & 31;
  for (int stage = 0; stage < n_stages; ++stage) {
#pragma unroll
    for (int j = 0; j < NA; ++j) sA[(ak + j * KA) * BM + am] = ra[j];
#pragma unroll
    for (int j = 0; j < NB; ++j) sB[(bk + j * KB) * BN + bn] = rb[j];
    __syncthreads();
    if (stage + 1 < n_stages) fetch(stage + 1);
#pragma unroll
    for (int kk = 0; kk < kConvBK / 2; ++kk) {
      const float a = sA[(2 * kk + half) * BM + wm * 32 + col];
      const float b = sB[(2 * kk + half) * BN + wn * 32 + col];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int on = n0 + wn * 32 + col;
  if (on < n_pix) {
    const int img = on / OHW, rem = on - img * OHW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float v = acc[r] + bias[m];
      out[((size_t)img * Cout + m) * OHW + rem] = v < 0.f ? 0.f : v;
    }
  }
}

// ---- max-pool 3x3, stride 2, floor mode, no padding --------------------------------------------------------------------------
__global__ __launch_bounds__(kLpThreads) void k_maxpool_3x3s2(const float* __restrict__ x, int n_out, int H, int W, int OH,
                                                              int OW, float* __restrict__ out) {
  const int i = blockIdx.x * kLpThreads + threadIdx.x;
  if (i >= n_out) return;
  const int ox = i % OW, q = i / OW;
  const int oy = q % OH, plane = q / OH;
  const float* __restrict__ p = x + ((size_t)plane * H + 2 * oy) * W + 2 * ox;
  float m = p[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float v = p[dy * W + dx];
      m = (v > m || v != v) ? v : m;   // (a NaN wins, as in the stock op)
    }
  out[i] = m;
}

// ---- the head ----------------------------------------------------------------------------------------------------------------
// feat [2V][C][HW] fp32; grid (ceil(HW / 256), V); partial[v * n_blocks + block] = the workgroup's sum over its pixels
__global__ __launch_bounds__(kLpThreads) void k_lpips_head(const float* __restrict__ feat, const float* __restrict__ lin, int V,
                                                           int C, int HW, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double s_red[kLpThreads / 64];
  const int p = blockIdx.x * kLpThreads + threadIdx.x, v = blockIdx.y;
  double term = 0.;
  if (p < HW) {
    const float* __restrict__ f0 = feat + (size_t)v * C * HW + p;
    const float* __restrict__ f1 = feat + (size_t)(V + v) * C * HW + p;
    double s0 = 0., s1 = 0.;
    for (int c = 0; c < C; ++c) {
      const double a = (double)f0[(size_t)c * HW], b = (double)f1[(size_t)c * HW];
      s0 += a * a;
      s1 += b * b;
    }
    const double n0 = sqrt(s0) + 1e-10, n1 = sqrt(s1) + 1e-10;
    for (int c = 0; c < C; ++c) {
      const double d = (double)f0[(size_t)c * HW] / n0 - (double)f1[(size_t)c * HW] / n1;
      term += (double)lin[c] * (d * d);
    }
  }
  term = lp_wave_sum_f64(term);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.;
    for (int w = 0; w < kLpThreads / 64; ++w) t += s_red[w];
    partial[(size_t)v * gridDim.x + blockIdx.x] = t;
  }
}

struct LpFinish {
  long offset[kLpLayers];   // of a layer's partials, in doubles ([V][n_blocks] each)
  int n_blocks[kLpLayers];
  double count[kLpLayers];  // pixels of the layer
};

// one workgroup per view: a layer's partials in a fixed order, the mean, then the five layers in ascending order
__global__ __launch_bounds__(kLpThreads) void k_lpips_finish(const double* __restrict__ partial, LpFinish f,
                                                             double* __restrict__ out, double* __restrict__ layers) {
  __shared__ double s_red[kLpThreads / 64];
  __shared__ double s_layer[kLpLayers];
  const int v = blockIdx.x;
  for (int l = 0; l < kLpLayers; ++l) {
    const double* __restrict__ p = partial + f.offset[l] + (size_t)v * f.n_blocks[l];
    double sum = 0.;
    for (int i = threadIdx.x; i < f.n_blocks[l]; i += kLpThreads) sum += p[i];
    sum = lp_wave_sum_f64(sum);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.;
      for (int w = 0; w < kLpThreads / 64; ++w) t += s_red[w];
      s_layer[l] = t / f.count[l];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double t = 0.;
    for (int l = 0; l < kLpLayers; ++l) {
      if (layers) layers[(size_t)v * kLpLayers + l] = s_layer[l];
      t += s_layer[l];
    }
    out[v] = t;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
constexpr double kTwo31 = 2147483648.0;

static int conv_out(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }
static long conv_kpad(long K) { return (K + kConvBK - 1) / kConvBK * kConvBK; }

template <int KH, int KW, int S, int P, int WM, int WN>
static int conv_launch_tile(const float* x, const float* wp, const float* bias, float* out, int n_pix, int Cin, int H, int W,
                            int OH, int OW, int Cout, hipStream_t st) {
  const long tiles = ((long)n_pix + 32 * WN - 1) / (32 * WN);
  const int n_stages = (int)(conv_kpad((long)Cin * KH * KW) / kConvBK);
  hipLaunchKernelGGL((k_conv_mfma<KH, KW, S, P, WM, WN>), dim3((unsigned)tiles, (unsigned)(Cout / (32 * WM))), dim3(64 * WM * WN),
                     0, st, x, wp, bias, out, n_pix, Cin, H, W, OH, OW, Cout, n_stages);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

template <int KH, int KW, int S, int P>
static int conv_launch(int variant, const float* x, const float* wp, const float* bias, float* out, int n_pix, int Cin, int H,
                       int W, int OH, int OW, int Cout, hipStream_t st) {
  if (variant == JT_CONV_TILE_AUTO) {
    // fewer 64 x 64 tiles than the chip has CUs: the one-wave tile spreads the layer over four times as many workgroups
    const long tiles64 = (((long)n_pix + 63) / 64) * ((Cout + 63) / 64);
    variant = (Cout % 64 != 0 || tiles64 < 256) ? JT_CONV_TILE_32X32 : JT_CONV_TILE_64X64;
  }
  switch (variant) {
    case JT_CONV_TILE_64X64:
      if (Cout % 64) return JT_ERR_UNSUPPORTED;
      return conv_launch_tile<KH, KW, S, P, 2, 2>(x, wp, bias, out, n_pix, Cin, H, W, OH, OW, Cout, st);
    case JT_CONV_TILE_32X32:
      return conv_launch_tile<KH, KW, S, P, 1, 1>(x, wp, bias, out, n_pix, Cin, H, W, OH, OW, Cout, st);
  }
  return JT_ERR_ARG;
}

// every refusal of one layer, decided before a launch; *oh, *ow = its output size
static int conv_check(int batch, int c_in, int h, int w, int c_out, int kh, int kw, int stride, int pad, int* oh, int* ow) {
  if (batch < 1 || c_in < 1 || h < 1 || w < 1 || c_out < 1) return JT_ERR_ARG;
  const bool g11 = kh == 11 && kw == 11 && stride == 4 && pad == 2, g5 = kh == 5 && kw == 5 && stride == 1 && pad == 2,
             g3 = kh == 3 && kw == 3 && stride == 1 && pad == 1;
  if (!(g11 || g5 || g3) || c_out % 32 != 0) return JT_ERR_UNSUPPORTED;
  if (h + 2 * pad < kh || w + 2 * pad < kw) return JT_ERR_UNSUPPORTED;
  *oh = conv_out(h, kh, stride, pad);
  *ow = conv_out(w, kw, stride, pad);
  if ((double)batch * c_in * h * w >= kTwo31 || (double)batch * c_out * *oh * *ow >= kTwo31 ||
      (double)c_in * kh * kw * c_out >= kTwo31 || c_out / 32 > 65535)
    return JT_ERR_UNSUPPORTED;
  return JT_OK;
}

static int conv_forward(const float* x, const float* wp, const float* bias, int batch, int c_in, int h, int w, int c_out, int kh,
                        int stride, int variant, float* out, int oh, int ow, hipStream_t st) {
  const int n_pix = batch * oh * ow;
  if (kh == 11) return conv_launch<11, 11, 4, 2>(variant, x, wp, bias, out, n_pix, c_in, h, w, oh, ow, c_out, st);
  if (kh == 5) return conv_launch<5, 5, 1, 2>(variant, x, wp, bias, out, n_pix, c_in, h, w, oh, ow, c_out, st);
  (void)stride;
  return conv_launch<3, 3, 1, 1>(variant, x, wp, bias, out, n_pix, c_in, h, w, oh, ow, c_out, st);
}

static int pool_forward(const float* x, int planes, int h, int w, float* out, hipStream_t st) {
  const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
  const int n_out = planes * oh * ow;
  hipLaunchKernelGGL(k_maxpool_3x3s2, dim3((n_out + kLpThreads - 1) / kLpThreads), dim3(kLpThreads), 0, st, x, n_out, h, w, oh,
                     ow, out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

// the AlexNet feature stack of LPIPS: channels, and what precedes the convolution
constexpr int kLpC[kLpLayers] = {64, 192, 384, 256, 256};
constexpr int kLpCin[kLpLayers] = {3, 64, 192, 384, 256};
constexpr int kLpKernel[kLpLayers] = {11, 5, 3, 3, 3};
constexpr int kLpStride[kLpLayers] = {4, 1, 1, 1, 1};
constexpr int kLpPad[kLpLayers] = {2, 2, 1, 1, 1};

struct LpPlan {
  int fh[kLpLayers], fw[kLpLayers];   // feature sizes
  long feat[kLpLayers];               // offsets in floats
  long scaled, pool1, pool2;
  long floats;                        // the fp32 part
  LpFinish fin;
  long doubles;                       // the partials behind it
};

// JT_OK, JT_ERR_ARG or JT_ERR_UNSUPPORTED; fills the plan
static int lpips_plan(int V, int H, int W, LpPlan* pl) {
  if (V < 1 || H < 1 || W < 1) return JT_ERR_ARG;
  if (H < 31 || W < 31) return JT_ERR_UNSUPPORTED;   // the second pool needs 3 rows: 31 -> 7 -> 3 -> 1
  const double B = 2.0 * V;
  int h = H, w = W;
  double most = B * 3 * h * w;
  for (int l = 0; l < kLpLayers; ++l) {
    if (l == 1 || l == 2) {
      h = (h - 3) / 2 + 1;
      w = (w - 3) / 2 + 1;
    }
    h = conv_out(h, kLpKernel[l], kLpStride[l], kLpPad[l]);
    w = conv_out(w, kLpKernel[l], kLpStride[l], kLpPad[l]);
    pl->fh[l] = h;
    pl->fw[l] = w;
    const double n = B * kLpC[l] * h * w;
    most = n > most ? n : most;
  }
  if (most >= kTwo31 || V > 65535) return JT_ERR_UNSUPPORTED;
  const long b = 2l * V;
  auto up = [](long n) { return (n + 63) / 64 * 64; };   // 256-byte steps
  long at = 0;
  pl->scaled = at;
  at += up(b * 3 * H * W);
  pl->feat[0] = at;
  at += up(b * 64 * pl->fh[0] * pl->fw[0]);
  pl->pool1 = at;
  at += up(b * 64 * pl->fh[1] * pl->fw[1]);
  pl->feat[1] = at;
  at += up(b * 192 * pl->fh[1] * pl->fw[1]);
  pl->pool2 = at;
  at += up(b * 192 * pl->fh[2] * pl->fw[2]);
  for (int l = 2; l < kLpLayers; ++l) {
    pl->feat[l] = at;
    at += up(b * kLpC[l] * pl->fh[l] * pl->fw[l]);
  }
  pl->floats = at;
  long d = 0;
  for (int l = 0; l < kLpLayers; ++l) {
    const long hw = (long)pl->fh[l] * pl->fw[l];
    pl->fin.offset[l] = d;
    pl->fin.n_blocks[l] = (int)((hw + kLpThreads - 1) / kLpThreads);
    pl->fin.count[l] = (double)hw;
    d += (long)V * pl->fin.n_blocks[l];
  }
  pl->doubles = d;
  return JT_OK;
}

}  // namespace jt

using namespace jt;

extern "C" size_t jt_conv_packed_floats(int c_out, int c_in, int kh, int kw) {
  if (c_out < 1 || c_in < 1 || kh < 1 || kw < 1 || (double)c_in * kh * kw * c_out >= kTwo31) return 0;
  return (size_t)conv_kpad((long)c_in * kh * kw) * (size_t)c_out;
}

extern "C" int jt_conv_pack_weights(const float* w, int c_out, int c_in, int kh, int kw, float* packed, void* stream) {
  if (!w || !packed || c_out < 1 || c_in < 1 || kh < 1 || kw < 1) return JT_ERR_ARG;
  const size_t n = jt_conv_packed_floats(c_out, c_in, kh, kw);
  if (n == 0 || (double)n >= kTwo31) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_conv_pack, dim3((unsigned)((n + kLpThreads - 1) / kLpThreads)), dim3(kLpThreads), 0, (hipStream_t)stream,
                     w, c_out, c_in * kh * kw, (int)n, packed);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_conv2d_relu_forward(const float* x, const float* packed, const float* bias, int batch, int c_in, int h, int w,
                                      int c_out, int kh, int kw, int stride, int pad, int variant, float* out, void* stream) {
  if (!x || !packed || !bias || !out) return JT_ERR_ARG;
  if (variant < JT_CONV_TILE_AUTO || variant > JT_CONV_TILE_32X32) return JT_ERR_ARG;
  int oh = 0, ow = 0;
  const int rc = conv_check(batch, c_in, h, w, c_out, kh, kw, stride, pad, &oh, &ow);
  if (rc != JT_OK) return rc;
  if (variant == JT_CONV_TILE_64X64 && c_out % 64 != 0) return JT_ERR_UNSUPPORTED;
  return conv_forward(x, packed, bias, batch, c_in, h, w, c_out, kh, stride, variant, out, oh, ow, (hipStream_t)stream);
}

extern "C" int jt_maxpool_3x3s2_forward(const float* x, int planes, int h, int w, float* out, void* stream) {
  if (!x || !out || planes < 1 || h < 3 || w < 3) return JT_ERR_ARG;
  if ((double)planes * h * w >= kTwo31) return JT_ERR_UNSUPPORTED;
  return pool_forward(x, planes, h, w, out, (hipStream_t)stream);
}

extern "C" size_t jt_lpips_workspace_bytes(int n_views, int height, int width) {
  LpPlan pl;
  if (lpips_plan(n_views, height, width, &pl) != JT_OK) return 0;
  return (size_t)pl.floats * sizeof(float) + (size_t)pl.doubles * sizeof(double);
}

extern "C" int jt_lpips_feature_layout(int n_views, int height, int width, int64_t* table) {
  if (!table) return JT_ERR_ARG;
  LpPlan pl;
  const int rc = lpips_plan(n_views, height, width, &pl);
  if (rc != JT_OK) return rc;
  for (int l = 0; l < kLpLayers; ++l) {
    table[4 * l + 0] = pl.feat[l];
    table[4 * l + 1] = kLpC[l];
    table[4 * l + 2] = pl.fh[l];
    table[4 * l + 3] = pl.fw[l];
  }
  return JT_OK;
}

extern "C" int jt_lpips_forward(const float* pred, const float* target, int n_views, int height, int width,
                                const JtLpipsWeights* weights, double* out, double* layers, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!pred || !target || !weights || !out || !workspace) return JT_ERR_ARG;
  for (int l = 0; l < kLpLayers; ++l)
    if (!weights->conv[l] || !weights->bias[l] || !weights->lin[l]) return JT_ERR_ARG;
  LpPlan pl;
  const int rc = lpips_plan(n_views, height, width, &pl);
  if (rc != JT_OK) return rc;
  if (workspace_bytes < (size_t)pl.floats * sizeof(float) + (size_t)pl.doubles * sizeof(double)) return JT_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  double* partial = reinterpret_cast<double*>(ws + pl.floats);
  const int V = n_views, B = 2 * n_views;
  const int per_side = V * 3 * height * width;
  hipLaunchKernelGGL(k_lpips_scale, dim3((per_side + kLpThreads - 1) / kLpThreads, 2), dim3(kLpThreads), 0, st, pred, target,
                     per_side, height * width, ws + pl.scaled);
  JT_LAUNCH_CHECK();
  const float* in = ws + pl.scaled;
  int h = height, w = width, r;
  for (int l = 0; l < kLpLayers; ++l) {
    if (l == 1 || l == 2) {
      float* pooled = ws + (l == 1 ? pl.pool1 : pl.pool2);
      if ((r = pool_forward(in, B * kLpCin[l], h, w, pooled, st)) != JT_OK) return r;
      h = (h - 3) / 2 + 1;
      w = (w - 3) / 2 + 1;
      in = pooled;
    }
    float* f = ws + pl.feat[l];
    if ((r = conv_forward(in, weights->conv[l], weights->bias[l], B, kLpCin[l], h, w, kLpC[l], kLpKernel[l], kLpStride[l],
                          JT_CONV_TILE_AUTO, f, pl.fh[l], pl.fw[l], st)) != JT_OK)
      return r;
    h = pl.fh[l];
    w = pl.fw[l];
    in = f;
    hipLaunchKernelGGL(k_lpips_head, dim3(pl.fin.n_blocks[l], V), dim3(kLpThreads), 0, st, (const float*)f, weights->lin[l], V,
                       kLpC[l], h * w, partial + pl.fin.offset[l]);
    JT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_lpips_finish, dim3(V), dim3(kLpThreads), 0, st, (const double*)partial, pl.fin, out, layers);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
