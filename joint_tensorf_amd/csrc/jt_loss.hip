// The loss head of the training step: the photometric loss in one kernel each way, its per-view form, the weighted total and the
// finiteness guard.
// Replaces tensorf.Graph.compute_loss's render term (model/tensorf.py:96-124) with Graph.MSE_loss = nanmean of squared error
// (model/base.py:259-261): the GT pixel gather `image[:, ray_idx]`, the hard edge-mask split
// edge_factor * MSE(rgb*m, img*m) + non_edge_factor * MSE(rgb*(1-m), img*(1-m))  and the plain MSE; the stock-op version is ~30
// tiny launches forward + backward.
// Every kernel of the family is a few lines around ONE set of functions: colour_at (one colour against its pixel), walk_sums (a
// thread's share of the four sums), block_sums, loss_of, colour_grad, weighted_total and finite_scan.  What the kernels promise
// each other bit for bit (per view = single view, _ind = direct, the three forms of the total) follows from that sharing.
#include <algorithm>

#include "jt_common.h"

namespace jt {

// Accumulators are cleared by a kernel, not hipMemsetAsync: the whole iteration is captured into a hipGraph
// (joint_tensorf_amd/graphed.py) and a captured 16-byte memset node was observed to leave stale accumulator contents
// in front of the kernel that follows it on replay.
__global__ void k_loss_zero(float* __restrict__ p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0.f;
}

// ---- one colour ------------------------------------------------------------------------------------------------------------
// what a batch is judged against: image [views][3][HW], mask [views][HW] or nullptr
struct Target {
  const float* image;
  const uint8_t* mask;
  int HW;
};

// slots != nullptr: the supervising buffers are named by device memory (a replayed hipGraph, jt_render_loss_*_ind); the pointer
// arguments then only say "present"
__device__ inline Target target_of(const float* image, const uint8_t* mask, int HW, const unsigned long long* slots) {
  if (slots) {
    image = reinterpret_cast<const float*>(slots[0]);
    if (mask) mask = reinterpret_cast<const uint8_t*>(slots[1]);
  }
  return {image, mask, HW};
}

struct Colour {
  float m, e, ne;  // mask value (1 without a mask), m d and (1 - m) d of d = colour - pixel
};

// colour i of rgb [.][r][3]: channel i % 3 of ray (i / 3) % r of view b0 + i / (3 r), against that ray's pixel of that view.
// 32-bit index arithmetic (the launchers refuse 2^31 colours): with `long` the four divisions per colour were most of
// k_render_loss_fwd_one's time.
__device__ inline Colour colour_at(const Target& T, const float* __restrict__ rgb, const int64_t* __restrict__ ray_idx,
                                   unsigned b0, unsigned r, unsigned i) {
  const unsigned bk = i / 3u, ch = i - bk * 3u;
  const unsigned v = bk / r, k = bk - v * r;
  const long b = b0 + v, pix = ray_idx[k];
  const float d = rgb[i] - T.image[(b * 3 + ch) * T.HW + pix];
  const float m = T.mask ? (float)T.mask[b * T.HW + pix] : 1.f;
  return {m, m * d, (1.f - m) * d};
}

// nanmean: a NaN term enters neither its sum nor its count, and gets no gradient
__device__ inline bool counted(float x) { return x == x; }

// the four sums of a batch, in the order of acc4: sum (m d)^2, #non-NaN of it, sum ((1-m) d)^2, #non-NaN
// (named fields: a sum and its count then go through one packed add, the square rounded on its own)
struct Sums {
  float s0, c0, s1, c1;
};

__device__ inline void add_colour(Sums& a, const Colour& c) {
  if (counted(c.e)) {
    a.s0 += c.e * c.e;
    a.c0 += 1.f;
  }
  if (counted(c.ne)) {
    a.s1 += c.ne * c.ne;
    a.c1 += 1.f;
  }
}

// A thread's share of the four sums over colours 0 .. n - 1: first, first + stride, ... summed in that order, but FETCHED U at a
// time (the index -> pixel chain is two dependent loads).  A fetch past n is clamped to n - 1 and not summed, so U is what a
// thread is expected to own: 8 where one workgroup walks the whole batch, 1 where the grid leaves a thread one or two colours.
// The sums do not depend on U.
template <int U>
__device__ inline Sums walk_sums(const Target& T, const float* __restrict__ rgb, const int64_t* __restrict__ ray_idx,
                                 unsigned b0, unsigned r, unsigned n, unsigned first, unsigned stride) {
  Sums a = {0.f, 0.f, 0.f, 0.f};
  for (unsigned i0 = first; i0 < n; i0 += U * stride) {
    Colour c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned i = i0 + u * stride;
      c[u] = colour_at(T, rgb, ray_idx, b0, r, i < n ? i : n - 1);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * stride >= n) break;
      add_colour(a, c[u]);
    }
  }
  return a;
}

// The workgroup's four sums: wave sums, then the waves added in wave order.  Thread c < 4 returns sum c (the others 0); red holds
// a row per wave, and its size says how many waves the kernel is launched with (a count known here lets the W reads go out
// together; read off blockDim.x they went one after the other)
template <int W>
__device__ inline float block_sums(const Sums& a, float (&red)[W][4]) {
  const float s0 = wave_sum(a.s0), c0 = wave_sum(a.c0), s1 = wave_sum(a.s1), c1 = wave_sum(a.c1);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv][0] = s0, red[wv][1] = c0, red[wv][2] = s1, red[wv][3] = c1;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < 4) {
    t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < W; ++w) t += red[w][threadIdx.x];
  }
  return t;
}

// nanmean of an all-NaN tensor is NaN (0 / 0), as in torch
__device__ inline float loss_of(const float acc[4], bool masked, float fe, float fne) {
  const float edge = acc[0] / acc[1];
  return masked ? fe * edge + fne * (acc[2] / acc[3]) : edge;
}

// ONE workgroup of 16 waves sums colours 0 .. n - 1 and finishes: fixed summation order, no atomics.  Threads 0 .. 3 hold
// one of the four sums each; the first n_sums of them are stored, and thread 0 collects all four for loss_of.  Without a mask
// (the per-view kernel: n_sums = 2, fe / fne unused) the last two are sums of 0 x d that nothing reads.
template <int U>
__device__ inline void one_group_loss(const Target& T, const float* __restrict__ rgb, const int64_t* __restrict__ ray_idx,
                                      unsigned b0, unsigned r, unsigned n, float fe, float fne, float* __restrict__ sums,
                                      int n_sums, float* __restrict__ loss) {
  __shared__ float red[16][4];
  const float t = block_sums(walk_sums<U>(T, rgb, ray_idx, b0, r, n, threadIdx.x, blockDim.x), red);
  const float acc[4] = {__shfl(t, 0), __shfl(t, 1), __shfl(t, 2), __shfl(t, 3)};
  if ((int)threadIdx.x < n_sums) sums[threadIdx.x] = t;
  if (threadIdx.x == 0) loss[0] = loss_of(acc, T.mask != nullptr, fe, fne);
}

// U: 1 under the full grid, which leaves a thread one or two colours (three from 262 144 on); 8 for the ONE workgroup of
// deterministic mode, which walks the whole batch
template <int U>
__global__ __launch_bounds__(256) void k_render_loss_fwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                         const int64_t* __restrict__ ray_idx,
                                                         const uint8_t* __restrict__ mask, int B, int r, int HW,
                                                         float* __restrict__ acc,
                                                         const unsigned long long* __restrict__ slots) {
  __shared__ float red[4][4];
  const Sums a = walk_sums<U>(target_of(image, mask, HW, slots), rgb, ray_idx, 0, r, (unsigned)B * r * 3,
                              blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  const float t = block_sums(a, red);
  if (threadIdx.x < 4) atomicAdd(acc + threadIdx.x, t);
}

// A training batch is a few thousand colours: ONE workgroup clears, sums and finishes in a single launch where the three-kernel
// form spends ~10 us of launch latency on 6 000 subtractions.
__global__ __launch_bounds__(1024) void k_render_loss_fwd_one(const float* __restrict__ rgb, const float* __restrict__ image,
                                                              const int64_t* __restrict__ ray_idx,
                                                              const uint8_t* __restrict__ mask, int B, int r, int HW,
                                                              float fe, float fne, float* __restrict__ acc,
                                                              float* __restrict__ loss,
                                                              const unsigned long long* __restrict__ slots) {
  one_group_loss<8>(target_of(image, mask, HW, slots), rgb, ray_idx, 0, r, (unsigned)B * r * 3, fe, fne, acc, 4, loss);
}

__global__ void k_render_loss_final(const float* __restrict__ acc, float fe, float fne, int masked,
                                    float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) loss[0] = loss_of(acc, masked != 0, fe, fne);
}

// d loss / d colour for upstream gradient 1, ke = edge_factor 2 / count of the edge mean, kne the same of the non-edge mean.
// A NaN colour is excluded from the mean and gets the gradient g x 0 = 0.  torch's nanmean backward gives NaN there (0 x 2 NaN
// through the square): the difference is deliberate.  The reference takes nanmean "to ignore the nan pixels" (model/base.py:261);
// a NaN gradient would reach every parameter the ray touches, and the NaN colour itself is reported by the finiteness guard.
__device__ inline float colour_grad(const Colour& c, bool masked, float ke, float kne) {
  float v = 0.f;
  if (counted(c.e)) v += ke * c.m * c.e;
  if (masked && counted(c.ne)) v += kne * (1.f - c.m) * c.ne;
  return v;
}

__global__ __launch_bounds__(256) void k_render_loss_bwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                         const int64_t* __restrict__ ray_idx,
                                                         const uint8_t* __restrict__ mask, int B, int r, int HW,
                                                         const float* __restrict__ acc, float fe, float fne,
                                                         const float* __restrict__ g, float* __restrict__ g_rgb,
                                                         const unsigned long long* __restrict__ slots) {
  const Target T = target_of(image, mask, HW, slots);
  const unsigned n = (unsigned)B * r * 3;
  const float gg = g[0];
  const float ke = (mask ? fe : 1.f) * 2.f / acc[1], kne = mask ? fne * 2.f / acc[3] : 0.f;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    g_rgb[i] = gg * colour_grad(colour_at(T, rgb, ray_idx, 0, r, i), mask != nullptr, ke, kne);
}

// ---- one photometric mean PER VIEW over a ragged batch (batched test-time pose optimisation, model/bat.py:265-292) -------------
// view b owns rays voff[b] .. voff[b + 1] - 1 of rgb [n][3] / ray_idx [n]; image [V][3][HW], no mask.  One workgroup per view runs
// k_render_loss_fwd_one's body on that view: loss[b] and the backward's per-element gradient are the single-view launch's bit
// for bit -- for views of 3 r <= 32 768 colours; past that the single-view entry point sums with k_render_loss_fwd (256-thread
// workgroups, atomic adds) and the two agree to rounding only.  An empty view walks nothing: its loss is 0 / 0.
__global__ __launch_bounds__(1024) void k_render_loss_views_fwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                                const int64_t* __restrict__ ray_idx,
                                                                const int* __restrict__ voff, int HW,
                                                                float* __restrict__ acc2, float* __restrict__ loss) {
  const int b = blockIdx.x, base = voff[b], r = voff[b + 1] - base;
  one_group_loss<1>({image, nullptr, HW}, rgb + 3 * (long)base, ray_idx + base, b, r, 3u * r, 0.f, 0.f, acc2 + 2 * b, 2, loss + b);
}

__global__ __launch_bounds__(256) void k_render_loss_views_bwd(const float* __restrict__ rgb, const float* __restrict__ image,
                                                               const int64_t* __restrict__ ray_idx,
                                                               const int* __restrict__ voff, int V, int n_rays, int HW,
                                                               const float* __restrict__ acc2, const float* __restrict__ g,
                                                               float* __restrict__ g_rgb) {
  const Target T = {image, nullptr, HW};
  const unsigned n = 3u * n_rays;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int b = ragged_view(voff, V, (int)(i / 3u)), base = voff[b], r = voff[b + 1] - base;
    const Colour c = colour_at(T, rgb + 3 * (long)base, ray_idx + base, b, r, i - 3u * base);
    g_rgb[i] = g[b] * colour_grad(c, false, 2.f / acc2[b * 2 + 1], 0.f);
  }
}

// ---- total = w_render * render + w_reg . reg3  and its backward: the weighted sum of model/tensorf.py:31-47 as one launch
// each way (as stock ops: a multiply and an add per term, a select-backward fill + copy per regulariser, ...) -------------------
struct Weights {
  float render, l1, tv_density, tv_color;
};

// the four weights by value, or from device memory where w4 is given (a replayed hipGraph: the TV weights decay every iteration)
__device__ inline Weights weights_of(Weights w, const float* __restrict__ w4) {
  if (w4) w.render = w4[0], w.l1 = w4[1], w.tv_density = w4[2], w.tv_color = w4[3];
  return w;
}

__device__ inline float weighted_total(const Weights& w, const float* __restrict__ render, const float* __restrict__ reg3) {
  float t = 0.f;
  // a term whose weight is zero does not enter the sum (the reference skips it: a NaN there must not spread)
  if (w.render != 0.f) t += w.render * render[0];
  t += w.l1 * reg3[0];  // the L1 term is always added (model/tensorf.py:39-41)
  if (w.tv_density != 0.f) t += w.tv_density * reg3[1];
  if (w.tv_color != 0.f) t += w.tv_color * reg3[2];
  return t;
}

__global__ void k_loss_sum_fwd(const float* __restrict__ render, const float* __restrict__ reg3, Weights w,
                               const float* __restrict__ w4, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = weighted_total(weights_of(w, w4), render, reg3);
}

__global__ void k_loss_sum_bwd(const float* __restrict__ g, Weights w, const float* __restrict__ w4,
                               float* __restrict__ g_render, float* __restrict__ g_reg3) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const Weights u = weights_of(w, w4);
    const float gg = g[0];
    g_render[0] = gg * u.render;
    g_reg3[0] = gg * u.l1;
    g_reg3[1] = gg * u.tv_density;
    g_reg3[2] = gg * u.tv_color;
  }
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

__device__ inline bool non_finite(float v) { return !(fabsf(v) <= 3.402823466e38f); }  // NaN or +-Inf

// ORs into *flag the bit of every listed tensor that holds a non-finite value, and `bits` (what the caller found itself)
__device__ inline void finite_scan(const FiniteArgs& A, int bits, int32_t* __restrict__ flag) {
  for (int k = 0; k < A.count; ++k) {
    const float* p = A.p[k];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < A.n[k]; i += (long)gridDim.x * blockDim.x)
      if (non_finite(p[i])) bits |= A.bit[k];
  }
  if (__any(bits != 0)) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o);
    if ((threadIdx.x & 63) == 0) atomicOr(flag, bits);
  }
}

__global__ __launch_bounds__(256) void k_finite_check(FiniteArgs A, int32_t* __restrict__ flag) { finite_scan(A, 0, flag); }

// the loss head's tail in ONE launch: k_loss_sum_fwd's total, the finiteness of that total (loss_bit), and the finiteness of the
// listed tensors (pose, colours) -- two launches of ~4.5 us each before
__global__ __launch_bounds__(256) void k_loss_sum_check(const float* __restrict__ render, const float* __restrict__ reg3,
                                                        Weights w, const float* __restrict__ w4, float* __restrict__ out,
                                                        FiniteArgs A, int32_t* __restrict__ flag, int loss_bit) {
  int bits = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float t = out[0] = weighted_total(weights_of(w, w4), render, reg3);
    if (non_finite(t)) bits = loss_bit;
  }
  finite_scan(A, bits, flag);
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

// the grid of the kernels that take one thread per colour: min(ceil(n / 256), 512) workgroups of 256
static int colour_blocks(long n) { return (int)std::min((n + 255) / 256, 512L); }

static int render_loss_forward(const float* rgb, const float* image, const int64_t* ray_idx, const uint8_t* edge_mask,
                               int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                               float* acc4, float* loss, const uint64_t* slots, void* stream) {
  if (!rgb || !image || !ray_idx || !acc4 || !loss || n_views < 1 || rays_per_view < 1 || n_pixels < 1)
    return JT_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  long n = (long)n_views * rays_per_view * 3;
  if (n >= (1l << 31)) return JT_ERR_UNSUPPORTED;  // the kernels index colours with 32 bits
  if (n <= 32768) {
    hipLaunchKernelGGL(k_render_loss_fwd_one, dim3(1), dim3(1024), 0, st, rgb, image, ray_idx, edge_mask, n_views,
                       rays_per_view, n_pixels, edge_factor, non_edge_factor, acc4, loss,
                       (const unsigned long long*)slots);
    JT_LAUNCH_CHECK();
    return JT_OK;
  }
  hipLaunchKernelGGL(k_loss_zero, dim3(1), dim3(64), 0, st, acc4, 4);
  JT_LAUNCH_CHECK();
  const bool one = jt_deterministic() != 0;  // one workgroup: the four sums have a fixed order
  hipLaunchKernelGGL(one ? k_render_loss_fwd<8> : k_render_loss_fwd<1>, dim3(one ? 1 : colour_blocks(n)), dim3(256), 0, st, rgb,
                     image, ray_idx, edge_mask, n_views, rays_per_view, n_pixels, acc4, (const unsigned long long*)slots);
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
  hipLaunchKernelGGL(k_render_loss_bwd, dim3(colour_blocks(n)), dim3(256), 0, (hipStream_t)stream, rgb, image, ray_idx,
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
  if (n >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_render_loss_views_bwd, dim3(colour_blocks(n)), dim3(256), 0, (hipStream_t)stream, rgb, image, ray_idx,
                     view_offset, n_views, n_rays, n_pixels, acc2, g_loss, g_rgb);
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

// ---- weighted total and finiteness guard ---------------------------------------------------------------------------------
// `items` as the guard kernels take them, and their grid: min(ceil(max n / 256), 256) workgroups of 256, at least one
static int finite_args(const JtFiniteItem* items, int n_items, FiniteArgs* A, int* blocks) {
  if (n_items < 0 || n_items > JT_FINITE_MAX || (n_items > 0 && !items)) return JT_ERR_ARG;
  long most = 1;
  for (int k = 0; k < n_items; ++k) {
    if (!items[k].data || items[k].n < 0) return JT_ERR_ARG;
    A->p[k] = items[k].data;
    A->n[k] = items[k].n;
    A->bit[k] = items[k].bit;
    most = std::max(most, (long)items[k].n);
  }
  A->count = n_items;
  *blocks = (int)std::min<long>((most + 255) / 256, 256);
  return JT_OK;
}

extern "C" int jt_finite_check(const JtFiniteItem* items, int n_items, int32_t* status_word, void* stream) {
  FiniteArgs A;
  int blocks;
  if (!status_word || n_items < 1 || finite_args(items, n_items, &A, &blocks) != JT_OK) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_finite_check, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A, status_word);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

// the weights of a launch: four host floats by value, or (w4_host == nullptr) the device's w4
static Weights host_weights(const float* w4_host) {
  return w4_host ? Weights{w4_host[0], w4_host[1], w4_host[2], w4_host[3]} : Weights{0.f, 0.f, 0.f, 0.f};
}

extern "C" int jt_loss_sum_check_forward(const float* render, const float* reg3, const float* w4_host,
                                         const float* w4_dev, float* total, const JtFiniteItem* items, int n_items,
                                         int32_t loss_bit, int32_t* status_word, void* stream) {
  FiniteArgs A;
  int blocks;
  if (!render || !reg3 || !total || !status_word || (!w4_host && !w4_dev) || finite_args(items, n_items, &A, &blocks) != JT_OK)
    return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_check, dim3(blocks), dim3(256), 0, (hipStream_t)stream, render, reg3, host_weights(w4_host),
                     w4_dev, total, A, status_word, (int)loss_bit);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

static int loss_sum_forward(const float* render, const float* reg3, const float* w4_host, const float* w4_dev, float* total,
                            void* stream) {
  if (!render || !reg3 || !total || (!w4_host && !w4_dev)) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_fwd, dim3(1), dim3(64), 0, (hipStream_t)stream, render, reg3, host_weights(w4_host), w4_dev,
                     total);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

static int loss_sum_backward(const float* g_total, const float* w4_host, const float* w4_dev, float* g_render, float* g_reg3,
                             void* stream) {
  if (!g_total || !g_render || !g_reg3 || (!w4_host && !w4_dev)) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_loss_sum_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, g_total, host_weights(w4_host), w4_dev,
                     g_render, g_reg3);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_loss_sum_forward(const float* render, const float* reg3, float w_render, float w_l1,
                                   float w_tv_density, float w_tv_color, float* total, void* stream) {
  const float w[4] = {w_render, w_l1, w_tv_density, w_tv_color};
  return loss_sum_forward(render, reg3, w, nullptr, total, stream);
}

extern "C" int jt_loss_sum_backward(const float* g_total, float w_render, float w_l1, float w_tv_density,
                                    float w_tv_color, float* g_render, float* g_reg3, void* stream) {
  const float w[4] = {w_render, w_l1, w_tv_density, w_tv_color};
  return loss_sum_backward(g_total, w, nullptr, g_render, g_reg3, stream);
}

extern "C" int jt_loss_sum_forward_dyn(const float* render, const float* reg3, const float* w4, float* total,
                                       void* stream) {
  return loss_sum_forward(render, reg3, nullptr, w4, total, stream);
}

extern "C" int jt_loss_sum_backward_dyn(const float* g_total, const float* w4, float* g_render, float* g_reg3,
                                        void* stream) {
  return loss_sum_backward(g_total, nullptr, w4, g_render, g_reg3, stream);
}
