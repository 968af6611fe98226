// Photometric loss of the training step in one kernel each way.
// Replaces tensorf.Graph.compute_loss's render term (model/tensorf.py:96-124) with Graph.MSE_loss =
// nanmean of squared error (model/base.py:259-261): the GT pixel gather `image[:, ray_idx]`, the hard
// edge-mask split  edge_factor * MSE(rgb*m, img*m) + non_edge_factor * MSE(rgb*(1-m), img*(1-m))  and the
// plain MSE; the stock-op version is ~30 tiny launches forward + backward.
#include <algorithm>

#include "jt_common.h"

namespace jt {

// Accumulators are cleared by a kernel, not hipMemsetAsync: the whole iteration is captured into a hipGraph
// (joint_tensorf_amd/graphed.py) and a captured 16-byte memset node was observed to leave stale accumulator contents
// in front of the kernel that follows it on replay.
__global__ void k_loss_zero(float* __restrict__ p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0.f;
}

// acc[0] = sum (m d)^2, acc[1] = #non-NaN of it, acc[2] = sum ((1-m) d)^2, acc[3] = #non-NaN
__global__ __launch_bounds__(256) void k_render_loss_fwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                         const int64_t* __restrict__ ray_idx,
                                                         const uint8_t* __restrict__ mask, int B, int r, int HW,
                                                         float* __restrict__ acc,
                                                         const unsigned long long* __restrict__ slots) {
  __shared__ float red[4][4];
  if (slots) {  // the supervising buffers are named by device memory (a replayed hipGraph, jt_render_loss_forward_ind)
    image = reinterpret_cast<const float*>(slots[0]);
    if (mask) mask = reinterpret_cast<const uint8_t*>(slots[1]);
  }
  const long n = (long)B * r * 3;
  float s0 = 0.f, c0 = 0.f, s1 = 0.f, c1 = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % 3);
    const long bk = i / 3;
    const int k = (int)(bk % r), b = (int)(bk / r);
    const long pix = ray_idx[k];
    const float d = rgb[i] - image[((long)b * 3 + ch) * HW + pix];
    const float m = mask ? (float)mask[(long)b * HW + pix] : 1.f;
    const float e = m * d, ne = (1.f - m) * d;
    if (e == e) {
      s0 += e * e;
      c0 += 1.f;
    }
    if (ne == ne) {
      s1 += ne * ne;
      c1 += 1.f;
    }
  }
  s0 = wave_sum(s0);
  c0 = wave_sum(c0);
  s1 = wave_sum(s1);
  c1 = wave_sum(c1);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[wv][0] = s0;
    red[wv][1] = c0;
    red[wv][2] = s1;
    red[wv][3] = c1;
  }
  __syncthreads();
  if (threadIdx.x < 4) atomicAdd(acc + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// A training batch is a few thousand colours: ONE workgroup clears, sums and finishes in a single launch (fixed summation
// order, no atomics) where the three-kernel form spends ~10 us of launch latency on 6 000 subtractions.
__global__ __launch_bounds__(1024) void k_render_loss_fwd_one(const float* __restrict__ rgb, const float* __restrict__ image,
                                                              const int64_t* __restrict__ ray_idx,
                                                              const uint8_t* __restrict__ mask, int B, int r, int HW,
                                                              float fe, float fne, float* __restrict__ acc,
                                                              float* __restrict__ loss,
                                                              const unsigned long long* __restrict__ slots) {
  __shared__ float red[16][4];
  if (slots) {
    image = reinterpret_cast<const float*>(slots[0]);
    if (mask) mask = reinterpret_cast<const uint8_t*>(slots[1]);
  }
  const long n = (long)B * r * 3;
  float s0 = 0.f, c0 = 0.f, s1 = 0.f, c1 = 0.f;
  // a thread's elements (i = t, t + 1024, ...) are summed in that order, but FETCHED eight at a time (the index -> pixel chain is
  // two dependent loads), with 32-bit index arithmetic (n < 2^31 is checked by the caller; with `long` the four divisions per
  // element were most of this kernel's 19 us)
  constexpr int U = 8;
  const unsigned un = (unsigned)n, ur = (unsigned)r;
  for (unsigned i0 = threadIdx.x; i0 < un; i0 += U * blockDim.x) {
    float dv[U], mv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned i = i0 + u * blockDim.x;
      const unsigned ii = i < un ? i : un - 1;
      const unsigned bk = ii / 3u, ch = ii - bk * 3u;
      const unsigned b = bk / ur, k = bk - b * ur;
      const long pix = ray_idx[k];
      dv[u] = rgb[ii] - image[((long)b * 3 + ch) * HW + pix];
      mv[u] = mask ? (float)mask[(long)b * HW + pix] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * blockDim.x >= un) break;
      const float d = dv[u], m = mv[u];
      const float e = m * d, ne = (1.f - m) * d;
      if (e == e) {
        s0 += e * e;
        c0 += 1.f;
      }
      if (ne == ne) {
        s1 += ne * ne;
        c1 += 1.f;
      }
    }
  }
  s0 = wave_sum(s0);
  c0 = wave_sum(c0);
  s1 = wave_sum(s1);
  c1 = wave_sum(c1);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[wv][0] = s0;
    red[wv][1] = c0;
    red[wv][2] = s1;
    red[wv][3] = c1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w)
      for (int c = 0; c < 4; ++c) a[c] += red[w][c];
    for (int c = 0; c < 4; ++c) acc[c] = a[c];
    const float edge = a[0] / a[1];  // nanmean of an all-NaN tensor is NaN (0/0), as in torch
    loss[0] = mask ? fe * edge + fne * (a[2] / a[3]) : edge;
  }
}

__global__ void k_render_loss_final(const float* __restrict__ acc, float fe, float fne, int masked,
                                    float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    // nanmean of an all-NaN tensor is NaN (0/0), as in torch
    const float edge = acc[0] / acc[1];
    loss[0] = masked ? fe * edge + fne * (acc[2] / acc[3]) : edge;
  }
}

// A NaN colour is excluded from the mean and gets the gradient g x 0 = 0.  torch's nanmean backward gives NaN there (0 x 2 NaN
// through the square): the difference is deliberate.  The reference takes nanmean "to ignore the nan pixels" (model/base.py:261);
// a NaN gradient would reach every parameter the ray touches, and the NaN colour itself is reported by the finiteness guard.
__global__ __launch_bounds__(256) void k_render_loss_bwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                         const int64_t* __restrict__ ray_idx,
                                                         const uint8_t* __restrict__ mask, int B, int r, int HW,
                                                         const float* __restrict__ acc, float fe, float fne,
                                                         const float* __restrict__ g, float* __restrict__ g_rgb,
                                                         const unsigned long long* __restrict__ slots) {
  if (slots) {
    image = reinterpret_cast<const float*>(slots[0]);
    if (mask) mask = reinterpret_cast<const uint8_t*>(slots[1]);
  }
  const long n = (long)B * r * 3;
  const float gg = g[0];
  const float ke = (mask ? fe : 1.f) * 2.f / acc[1], kne = mask ? fne * 2.f / acc[3] : 0.f;
  const unsigned un = (unsigned)n, ur = (unsigned)r;   // (n < 2^31: checked by the caller)
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < un; i += gridDim.x * blockDim.x) {
    const unsigned bk = i / 3u, ch = i - bk * 3u;
    const unsigned b = bk / ur, k = bk - b * ur;
    const long pix = ray_idx[k];
    const float d = rgb[i] - image[((long)b * 3 + ch) * HW + pix];
    const float m = mask ? (float)mask[(long)b * HW + pix] : 1.f;
    const float e = m * d, ne = (1.f - m) * d;
    float v = 0.f;
    if (e == e) v += ke * m * e;
    if (mask && ne == ne) v += kne * (1.f - m) * ne;
    g_rgb[i] = gg * v;
  }
}

// ---- one photometric mean PER VIEW over a ragged batch (batched test-time pose optimisation, model/bat.py:265-292) -------------
// view b owns rays voff[b] .. voff[b + 1] - 1 of rgb [n][3] / ray_idx [n]; image [V][3][HW].  One workgroup per view, with the
// summation structure of k_render_loss_fwd_one for a single view: loss[b] and the backward's per-element gradient are the
// single-view launch's bit for bit -- for views of 3 r <= 32 768 colours; past that the single-view entry point sums with
// k_render_loss_fwd (256-thread workgroups, atomic adds) and the two agree to rounding only.
__global__ __launch_bounds__(1024) void k_render_loss_views_fwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                                const int64_t* __restrict__ ray_idx,
                                                                const int* __restrict__ voff, int HW,
                                                                float* __restrict__ acc2, float* __restrict__ loss) {
  __shared__ float red[16][2];
  const int b = blockIdx.x, base = voff[b], r = voff[b + 1] - voff[b];
  const long n = (long)r * 3;
  float s0 = 0.f, c0 = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int ch = (int)(i % 3);
    const long k = i / 3;
    const long pix = ray_idx[base + k];
    const float d = rgb[(long)base * 3 + i] - image[((long)b * 3 + ch) * HW + pix];
    const float e = 1.f * d;
    if (e == e) {
      s0 += e * e;
      c0 += 1.f;
    }
  }
  s0 = wave_sum(s0);
  c0 = wave_sum(c0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv][0] = s0, red[wv][1] = c0;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a0 = 0.f, a1 = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) a0 += red[w][0], a1 += red[w][1];
    acc2[b * 2] = a0, acc2[b * 2 + 1] = a1;
    loss[b] = a0 / a1;
  }
}

__global__ __launch_bounds__(256) void k_render_loss_views_bwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                               const int64_t* __restrict__ ray_idx,
                                                               const int* __restrict__ voff, int V, int n_rays, int HW,
                                                               const float* __restrict__ acc2, const float* __restrict__ g,
                                                               float* __restrict__ g_rgb) {
  const long n = (long)n_rays * 3;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % 3);
    const int t = (int)(i / 3);
    int lo = 0, hi = V - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (voff[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const float ke = 1.f * 2.f / acc2[b * 2 + 1];
    const float d = rgb[i] - image[((long)b * 3 + ch) * HW + ray_idx[t]];
    const float e = 1.f * d;
    float v = 0.f;
    if (e == e) v += ke * 1.f * e;
    g_rgb[i] = g[b] * v;
  }
}

// total = w_render * render + w_reg . reg3  and its backward: the weighted sum of model/tensorf.py:31-47 as one launch
// each way (as stock ops: a multiply and an add per term, a select-backward fill + copy per regulariser, ...).
__global__ void k_loss_sum_fwd(const float* __restrict__ render, const float* __restrict__ reg3, float wr, float w0,
                               float w1, float w2, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float t = 0.f;
    // a term whose weight is zero does not enter the sum (the reference skips it: a NaN there must not spread)
    if (wr != 0.f) t += wr * render[0];
    t += w0 * reg3[0];  // the L1 term is always added (model/tensorf.py:39-41)
    if (w1 != 0.f) t += w1 * reg3[1];
    if (w2 != 0.f) t += w2 * reg3[2];
    out[0] = t;
  }
}

__global__ void k_loss_sum_bwd(const float* __restrict__ g, float wr, float w0, float w1, float w2,
                               float* __restrict__ g_render, float* __restrict__ g_reg3) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float gg = g[0];
    g_render[0] = gg * wr;
    g_reg3[0] = gg * w0;
    g_reg3[1] = gg * w1;
    g_reg3[2] = gg * w2;
  }
}

// the same with the four weights in device memory (a replayed hipGraph: the TV weights decay every iteration)
__global__ void k_loss_sum_fwd_dyn(const float* __restrict__ render, const float* __restrict__ reg3,
                                   const float* __restrict__ w, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float t = 0.f;
    if (w[0] != 0.f) t += w[0] * render[0];
    t += w[1] * reg3[0];
    if (w[2] != 0.f) t += w[2] * reg3[1];
    if (w[3] != 0.f) t += w[3] * reg3[2];
    out[0] = t;
  }
}

__global__ void k_loss_sum_bwd_dyn(const float* __restrict__ g, const float* __restrict__ w,
                                   float* __restrict__ g_render, float* __restrict__ g_reg3) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float gg = g[0];
    g_render[0] = gg * w[0];
    g_reg3[0] = gg * w[1];
    g_reg3[1] = gg * w[2];
    g_reg3[2] = gg * w[3];
  }
}

// TV of a depth lattice [B][H][W] (model/tensorf.py:126-135): sum_h (d[h+1] - d[h])^2 / H + sum_w (d[w+1] - d[w])^2 / W, value only
// (the BAT yamls weight the term 0.0: the reference still evaluates it for its logs with a dozen elementwise launches)
__global__ __launch_bounds__(1024) void k_tv_depth(const float* __restrict__ d, int B, int H, int W, float* __restrict__ out) {
  __shared__ float s_h[16], s_w[16];
  float sh = 0.f, sw = 0.f;
  const long n = (long)B * H * W;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const float v = d[i];
    if (h + 1 < H) { const float t = d[i + W] - v; sh += t * t; }
    if (w + 1 < W) { const float t = d[i + 1] - v; sw += t * t; }
  }
  sh = wave_sum(sh);
  sw = wave_sum(sw);
  if ((threadIdx.x & 63) == 0) s_h[threadIdx.x >> 6] = sh, s_w[threadIdx.x >> 6] = sw;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) a += s_h[k], b += s_w[k];
    out[0] = a / (float)H + b / (float)W;
  }
}

}  // namespace jt

using namespace jt;

extern "C" int jt_tv_depth_forward(const float* depth, int n_views, int grid_h, int grid_w, float* out, void* stream) {
  if (!depth || !out || n_views < 1 || grid_h < 1 || grid_w < 1) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_tv_depth, dim3(1), dim3(1024), 0, (hipStream_t)stream, depth, n_views, grid_h, grid_w, out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_loss_sum_forward_dyn(const float* render, const float* reg3, const float* w4, float* total,
                                       void* stream) {
  if (!render || !reg3 || !w4 || !total) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_fwd_dyn, dim3(1), dim3(64), 0, (hipStream_t)stream, render, reg3, w4, total);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_loss_sum_backward_dyn(const float* g_total, const float* w4, float* g_render, float* g_reg3,
                                        void* stream) {
  if (!g_total || !w4 || !g_render || !g_reg3) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_bwd_dyn, dim3(1), dim3(64), 0, (hipStream_t)stream, g_total, w4, g_render, g_reg3);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

static int render_loss_forward(const float* rgb, const float* image, const int64_t* ray_idx, const uint8_t* edge_mask,
                               int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                               float* acc4, float* loss, const uint64_t* slots, void* stream) {
  if (!rgb || !image || !ray_idx || !acc4 || !loss || n_views < 1 || rays_per_view < 1 || n_pixels < 1)
    return JT_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  long n = (long)n_views * rays_per_view * 3;
  if (n <= 32768) {
    hipLaunchKernelGGL(k_render_loss_fwd_one, dim3(1), dim3(1024), 0, st, rgb, image, ray_idx, edge_mask, n_views,
                       rays_per_view, n_pixels, edge_factor, non_edge_factor, acc4, loss,
                       (const unsigned long long*)slots);
    JT_LAUNCH_CHECK();
    return JT_OK;
  }
  hipLaunchKernelGGL(k_loss_zero, dim3(1), dim3(64), 0, st, acc4, 4);
  JT_LAUNCH_CHECK();
  int blocks = (int)min((n + 255) / 256, 512L);
  if (jt_deterministic()) blocks = 1;  // one workgroup: the four sums have a fixed order
  hipLaunchKernelGGL(k_render_loss_fwd, dim3(blocks), dim3(256), 0, st, rgb, image, ray_idx, edge_mask, n_views,
                     rays_per_view, n_pixels, acc4, (const unsigned long long*)slots);
  JT_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_render_loss_final, dim3(1), dim3(64), 0, st, (const float*)acc4, edge_factor,
                     non_edge_factor, edge_mask ? 1 : 0, loss);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

static int render_loss_backward(const float* rgb, const float* image, const int64_t* ray_idx, const uint8_t* edge_mask,
                                int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                                const float* acc4, const float* g_loss, float* g_rgb, const uint64_t* slots,
                                void* stream) {
  if (!rgb || !image || !ray_idx || !acc4 || !g_loss || !g_rgb || n_views < 1 || rays_per_view < 1 || n_pixels < 1)
    return JT_ERR_ARG;
  long n = (long)n_views * rays_per_view * 3;
  if (n >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  int blocks = (int)min((n + 255) / 256, 512L);
  hipLaunchKernelGGL(k_render_loss_bwd, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rgb, image, ray_idx,
                     edge_mask, n_views, rays_per_view, n_pixels, acc4, edge_factor, non_edge_factor, g_loss, g_rgb,
                     (const unsigned long long*)slots);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_render_loss_views_forward(const float* rgb, const float* image, const int64_t* ray_idx,
                                            const int32_t* view_offset, int n_views, int n_pixels, float* acc2, float* loss,
                                            void* stream) {
  if (!rgb || !image || !ray_idx || !view_offset || !acc2 || !loss || n_views < 1 || n_pixels < 1) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_render_loss_views_fwd, dim3(n_views), dim3(1024), 0, (hipStream_t)stream, rgb, image, ray_idx,
                     view_offset, n_pixels, acc2, loss);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_render_loss_views_backward(const float* rgb, const float* image, const int64_t* ray_idx,
                                             const int32_t* view_offset, int n_views, int n_rays, int n_pixels,
                                             const float* acc2, const float* g_loss, float* g_rgb, void* stream) {
  if (!rgb || !image || !ray_idx || !view_offset || !acc2 || !g_loss || !g_rgb || n_views < 1 || n_rays < 1 || n_pixels < 1)
    return JT_ERR_ARG;
  const long n = (long)n_rays * 3;
  hipLaunchKernelGGL(k_render_loss_views_bwd, dim3((int)min((n + 255) / 256, 512L)), dim3(256), 0, (hipStream_t)stream, rgb,
                     image, ray_idx, view_offset, n_views, n_rays, n_pixels, acc2, g_loss, g_rgb);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_render_loss_forward(const float* rgb, const float* image, const int64_t* ray_idx,
                                      const uint8_t* edge_mask, int n_views, int rays_per_view, int n_pixels,
                                      float edge_factor, float non_edge_factor, float* acc4, float* loss,
                                      void* stream) {
  return render_loss_forward(rgb, image, ray_idx, edge_mask, n_views, rays_per_view, n_pixels, edge_factor,
                             non_edge_factor, acc4, loss, nullptr, stream);
}

extern "C" int jt_render_loss_backward(const float* rgb, const float* image, const int64_t* ray_idx,
                                       const uint8_t* edge_mask, int n_views, int rays_per_view, int n_pixels,
                                       float edge_factor, float non_edge_factor, const float* acc4,
                                       const float* g_loss, float* g_rgb, void* stream) {
  return render_loss_backward(rgb, image, ray_idx, edge_mask, n_views, rays_per_view, n_pixels, edge_factor,
                              non_edge_factor, acc4, g_loss, g_rgb, nullptr, stream);
}

extern "C" int jt_render_loss_forward_ind(const float* rgb, const uint64_t* slots, const int64_t* ray_idx,
                                          int with_edge_mask, int n_views, int rays_per_view, int n_pixels,
                                          float edge_factor, float non_edge_factor, float* acc4, float* loss,
                                          void* stream) {
  if (!slots) return JT_ERR_ARG;
  // (the pointer arguments of the kernel only say "present"; the addresses are read from `slots` on the device)
  return render_loss_forward(rgb, reinterpret_cast<const float*>(slots), ray_idx,
                             with_edge_mask ? reinterpret_cast<const uint8_t*>(slots) : nullptr, n_views, rays_per_view,
                             n_pixels, edge_factor, non_edge_factor, acc4, loss, slots, stream);
}

extern "C" int jt_render_loss_backward_ind(const float* rgb, const uint64_t* slots, const int64_t* ray_idx,
                                           int with_edge_mask, int n_views, int rays_per_view, int n_pixels,
                                           float edge_factor, float non_edge_factor, const float* acc4,
                                           const float* g_loss, float* g_rgb, void* stream) {
  if (!slots) return JT_ERR_ARG;
  return render_loss_backward(rgb, reinterpret_cast<const float*>(slots), ray_idx,
                              with_edge_mask ? reinterpret_cast<const uint8_t*>(slots) : nullptr, n_views,
                              rays_per_view, n_pixels, edge_factor, non_edge_factor, acc4, g_loss, g_rgb, slots, stream);
}

// ---- device-side non-finite guard ------------------------------------------------------------------------------
// The reference raises on a NaN pose (model/tensorf.py:147-151) and asserts finite loss terms (model/tensorf.py:43-44)
// with one device->host read each per iteration.  Here ONE launch per iteration ORs a bit per checked tensor into a
// status word that stays on the device; the host reads the word when it chooses to (every opt.freq.scalar iterations).
struct FiniteArgs {
  const float* p[JT_FINITE_MAX];
  long n[JT_FINITE_MAX];
  int bit[JT_FINITE_MAX];
  int count;
};

__global__ __launch_bounds__(256) void k_finite_check(FiniteArgs A, int32_t* __restrict__ flag) {
  int bits = 0;
  for (int k = 0; k < A.count; ++k) {
    const float* p = A.p[k];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < A.n[k]; i += (long)gridDim.x * blockDim.x) {
      const float v = p[i];
      if (!(fabsf(v) <= 3.402823466e38f)) bits |= A.bit[k];  // NaN or +-Inf
    }
  }
  if (__any(bits != 0)) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o);
    if ((threadIdx.x & 63) == 0) atomicOr(flag, bits);
  }
}

// the loss head's tail in ONE launch: total = w . (render, reg3) as k_loss_sum_fwd / _dyn computes it, the finiteness of that
// total (loss_bit), and the finiteness of the listed tensors (pose, colours) -- two launches of ~4.5 us each before
__global__ __launch_bounds__(256) void k_loss_sum_check(const float* __restrict__ render, const float* __restrict__ reg3,
                                                        float wr, float w0, float w1, float w2,
                                                        const float* __restrict__ w4, float* __restrict__ out,
                                                        FiniteArgs A, int32_t* __restrict__ flag, int loss_bit) {
  int bits = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (w4) wr = w4[0], w0 = w4[1], w1 = w4[2], w2 = w4[3];
    float t = 0.f;
    if (wr != 0.f) t += wr * render[0];
    t += w0 * reg3[0];
    if (w1 != 0.f) t += w1 * reg3[1];
    if (w2 != 0.f) t += w2 * reg3[2];
    out[0] = t;
    if (!(fabsf(t) <= 3.402823466e38f)) bits |= loss_bit;
  }
  for (int k = 0; k < A.count; ++k) {
    const float* p = A.p[k];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < A.n[k]; i += (long)gridDim.x * blockDim.x) {
      const float v = p[i];
      if (!(fabsf(v) <= 3.402823466e38f)) bits |= A.bit[k];
    }
  }
  if (__any(bits != 0)) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o);
    if ((threadIdx.x & 63) == 0) atomicOr(flag, bits);
  }
}

extern "C" int jt_loss_sum_check_forward(const float* render, const float* reg3, const float* w4_host,
                                         const float* w4_dev, float* total, const JtFiniteItem* items, int n_items,
                                         int32_t loss_bit, int32_t* status_word, void* stream) {
  if (!render || !reg3 || !total || !status_word || (!w4_host && !w4_dev) || n_items < 0 || n_items > JT_FINITE_MAX ||
      (n_items > 0 && !items))
    return JT_ERR_ARG;
  FiniteArgs A;
  long most = 1;
  for (int k = 0; k < n_items; ++k) {
    if (!items[k].data || items[k].n < 0) return JT_ERR_ARG;
    A.p[k] = items[k].data;
    A.n[k] = items[k].n;
    A.bit[k] = items[k].bit;
    most = std::max(most, (long)items[k].n);
  }
  A.count = n_items;
  const int blocks = (int)std::min<long>((most + 255) / 256, 256);
  const float z = 0.f;
  const float* w = w4_host ? w4_host : &z;
  hipLaunchKernelGGL(k_loss_sum_check, dim3(std::max(blocks, 1)), dim3(256), 0, (hipStream_t)stream, render, reg3,
                     w4_host ? w[0] : 0.f, w4_host ? w[1] : 0.f, w4_host ? w[2] : 0.f, w4_host ? w[3] : 0.f, w4_dev, total, A,
                     status_word, (int)loss_bit);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_finite_check(const JtFiniteItem* items, int n_items, int32_t* status_word, void* stream) {
  if (!items || !status_word || n_items < 1 || n_items > JT_FINITE_MAX) return JT_ERR_ARG;
  FiniteArgs A;
  long total = 0;
  for (int k = 0; k < n_items; ++k) {
    if (!items[k].data || items[k].n < 0) return JT_ERR_ARG;
    A.p[k] = items[k].data;
    A.n[k] = items[k].n;
    A.bit[k] = items[k].bit;
    total = std::max(total, (long)items[k].n);
  }
  A.count = n_items;
  const int blocks = (int)std::min<long>((total + 255) / 256, 256);
  hipLaunchKernelGGL(k_finite_check, dim3(std::max(blocks, 1)), dim3(256), 0, (hipStream_t)stream, A, status_word);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_loss_sum_forward(const float* render, const float* reg3, float w_render, float w_l1,
                                   float w_tv_density, float w_tv_color, float* total, void* stream) {
  if (!render || !reg3 || !total) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_fwd, dim3(1), dim3(64), 0, (hipStream_t)stream, render, reg3, w_render, w_l1,
                     w_tv_density, w_tv_color, total);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_loss_sum_backward(const float* g_total, float w_render, float w_l1, float w_tv_density,
                                    float w_tv_color, float* g_render, float* g_reg3, void* stream) {
  if (!g_total || !g_render || !g_reg3) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, g_total, w_render, w_l1, w_tv_density,
                     w_tv_color, g_render, g_reg3);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
