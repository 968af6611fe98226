// A triangle rasteriser for looking at an exported mesh from its cameras: project, draw into a 64-bit z-buffer, resolve.
//
// Coverage is decided in integers.  A projected vertex is snapped to 1/256 pixel (rintf(x * 256)); the three edge functions are
// evaluated at the pixel centre (256 i + 128, 256 j + 128) in int64 with the top-left fill rule, so two triangles that share an
// edge cover every pixel of their union exactly once whatever the floating-point unit does.  x is the column and y the row: the
// pixel of column i and row j has its centre at (i + 0.5, j + 0.5), the convention of the ray generator.
//
// Depth is q = 1 / w, interpolated linearly in screen space with the integer edge values as weights.  The nearest triangle
// (largest q) wins, at equal q the lower index: ONE atomicMin per covered pixel on key = (~bits(q)) << 32 | index (q > 0, so its
// bits order like the number).  A minimum over a set does not depend on the order it is taken in: the same bits on every run.
//
// Work distribution of k_raster_draw: one lane per (view, triangle).  A lane whose clipped bounding box holds at most 64 pixels
// walks it alone; the wave then takes its remaining triangles one at a time (ballot, set-up broadcast by shuffle) and strides
// all 64 lanes over the clipped box.  The meshes this is for (marching tetrahedra on a 400^3 lattice seen at 800 x 800) are
// millions of triangles a pixel or two across: nearly everything takes the first path, and a large triangle costs its wave, not
// one lane, the walk.
#include "jt_common.h"

namespace jt {

constexpr int kRasterThreads = 256;
constexpr int kRasterSmall = 64;                 // pixels of a clipped box one lane may walk alone
constexpr float kRasterGuard = 4194304.f;        // 2^22 sub-pixels: |snapped coordinate| beyond it drops the triangle
constexpr int kRasterMaxAttrs = 8;

struct RasterAttrBg {
  float v[kRasterMaxAttrs];
};

// One triangle of one view, ready to be tested against pixel centres.  x[k], y[k]: snapped sub-pixel coordinates; sign: +1 when
// the signed area (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) is positive (clockwise on a screen whose y runs down), -1 when negative:
// the edge values are multiplied by it, so the inside is always the positive side.  bias[k] = 0 for a top or left edge (a pixel
// centre exactly on it is inside), 1 otherwise (it is not).
struct RasterTri {
  int x[3], y[3];
  float q[3];
  int sign;
  int bias[3];
  int status;
};

__device__ inline bool raster_valid_q(float q) { return q > 0.f && q < __builtin_inff(); }

// status codes (include/jt_render.h): 0 drawn, 1 a vertex behind near / non-finite, 2 beyond the guard band, 3 zero area, 4 culled
__device__ inline RasterTri raster_setup(const float4 s0, const float4 s1, const float4 s2, int cull) {
  RasterTri t;
  t.status = 0;
  t.sign = 1;
  const float4 s[3] = {s0, s1, s2};
  bool dropped = false, far_out = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t.q[k] = s[k].z;
    dropped |= !raster_valid_q(s[k].z);
    const float fx = rintf(s[k].x * 256.f), fy = rintf(s[k].y * 256.f);
    const bool in = fabsf(fx) <= kRasterGuard && fabsf(fy) <= kRasterGuard;   // false for a NaN
    far_out |= !in;
    t.x[k] = in ? (int)fx : 0;
    t.y[k] = in ? (int)fy : 0;
    t.bias[k] = 1;
  }
  if (dropped) {
    t.status = 1;
    return t;
  }
  if (far_out) {
    t.status = 2;
    return t;
  }
  const long area = (long)(t.x[1] - t.x[0]) * (long)(t.y[2] - t.y[0]) - (long)(t.y[1] - t.y[0]) * (long)(t.x[2] - t.x[0]);
  if (area == 0) {
    t.status = 3;
    return t;
  }
  if (cull && area > 0) {
    t.status = 4;
    return t;
  }
  t.sign = area > 0 ? 1 : -1;
  // edge k runs from vertex (k + 1) % 3 to vertex (k + 2) % 3 and weighs vertex k; with the inside on its positive side, an edge
  // pointing up the screen (dy < 0) is a left edge and a horizontal one pointing right (dy == 0, dx > 0) a top edge
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const int dx = t.sign * (t.x[b] - t.x[a]), dy = t.sign * (t.y[b] - t.y[a]);
    t.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
  }
  return t;
}

// the three edge values of pixel (px, py)'s centre, inside-positive; true when the pixel is covered
__device__ inline bool raster_edges(const RasterTri& t, int px, int py, long b[3]) {
  const long cx = 256l * px + 128, cy = 256l * py + 128;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int u = (k + 1) % 3, v = (k + 2) % 3;
    const long e = (long)(t.x[v] - t.x[u]) * (cy - t.y[u]) - (long)(t.y[v] - t.y[u]) * (cx - t.x[u]);
    b[k] = t.sign * e;
    in &= b[k] >= t.bias[k];
  }
  return in;
}

// q at a covered pixel: (b0 q0 + b1 q1 + b2 q2) / (b0 + b1 + b2), every term positive or zero
__device__ inline float raster_q(const RasterTri& t, const long b[3]) {
  const float num = fmaf((float)b[0], t.q[0], fmaf((float)b[1], t.q[1], (float)b[2] * t.q[2]));
  return num / (float)(b[0] + b[1] + b[2]);
}

__device__ inline unsigned long long raster_key(float q, int tri) {
  return (unsigned long long)(~__float_as_uint(q)) << 32 | (unsigned)tri;
}

struct RasterBox {
  int x0, y0, w, h;      // w, h <= 0: nothing to walk
};

// the pixels whose centre can lie inside the triangle, clipped to the image
__device__ inline RasterBox raster_box(const RasterTri& t, int H, int W) {
  const int xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
  const int ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
  // 256 i + 128 >= xmin  <=>  i >= ceil((xmin - 128) / 256);  256 i + 128 <= xmax  <=>  i <= floor((xmax - 128) / 256)
  const int x0 = max((xmin + 127) >> 8, 0), x1 = min((xmax - 128) >> 8, W - 1);
  const int y0 = max((ymin + 127) >> 8, 0), y1 = min((ymax - 128) >> 8, H - 1);
  return RasterBox{x0, y0, x1 - x0 + 1, y1 - y0 + 1};
}

__device__ inline void raster_pixel(const RasterTri& t, int tri, int px, int py, int W, unsigned long long* __restrict__ zview) {
  long b[3];
  if (raster_edges(t, px, py, b)) atomicMin(zview + (size_t)py * W + px, raster_key(raster_q(t, b), tri));
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_project(const float* __restrict__ vertices, int nv,
                                                                   const float* __restrict__ proj, float near,
                                                                   float4* __restrict__ screen) {
  const long i = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i >= nv) return;
  const int view = blockIdx.y;
  const float* P = proj + 12 * view;
  const float vx = vertices[3 * i], vy = vertices[3 * i + 1], vz = vertices[3 * i + 2];
  const float xw = fmaf(P[0], vx, fmaf(P[1], vy, fmaf(P[2], vz, P[3])));
  const float yw = fmaf(P[4], vx, fmaf(P[5], vy, fmaf(P[6], vz, P[7])));
  const float w = fmaf(P[8], vx, fmaf(P[9], vy, fmaf(P[10], vz, P[11])));
  const bool finite = __builtin_isfinite(vx) && __builtin_isfinite(vy) && __builtin_isfinite(vz);
  float4 s = make_float4(0.f, 0.f, 0.f, w);
  if (finite && w >= near) {             // false for a NaN w
    const float q = 1.f / w;
    s = make_float4(xw / w, yw / w, raster_valid_q(q) ? q : 0.f, w);
  }
  screen[(size_t)view * nv + i] = s;
}

__global__ __launch_bounds__(kRasterThreads) void k_raster_draw(const float4* __restrict__ screen, int nv,
                                                                const int32_t* __restrict__ triangles, int nt, int H, int W,
                                                                int cull, unsigned long long* __restrict__ zbuf,
                                                                uint8_t* __restrict__ status) {
  const long ti = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  const int view = blockIdx.y;
  const float4* sv = screen + (size_t)view * nv;
  unsigned long long* zview = zbuf + (size_t)view * H * W;
  RasterTri t = {};
  t.status = 1;
  RasterBox box{0, 0, 0, 0};
  bool live = false;
  if (ti < nt) {
    const int i0 = triangles[3 * ti], i1 = triangles[3 * ti + 1], i2 = triangles[3 * ti + 2];
    if ((unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv) {
      t = raster_setup(sv[i0], sv[i1], sv[i2], cull);
      if (t.status == 0) {
        box = raster_box(t, H, W);
        live = box.w > 0 && box.h > 0;
      }
    }
    status[(size_t)view * nt + ti] = (uint8_t)t.status;
  }
  const bool small = live && (long)box.w * box.h <= kRasterSmall;
  if (small) {
    for (int y = 0; y < box.h; ++y)
      for (int x = 0; x < box.w; ++x) raster_pixel(t, (int)ti, box.x0 + x, box.y0 + y, W, zview);
  }
  // the wave's large triangles, one at a time, all 64 lanes striding over the clipped box
  unsigned long long large = __ballot(live && !small);
  const int lane = threadIdx.x & 63;
  while (large) {
    const int src = __ffsll((long long)large) - 1;
    large &= large - 1;
    RasterTri u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u.x[k] = __shfl(t.x[k], src);
      u.y[k] = __shfl(t.y[k], src);
      u.q[k] = __shfl(t.q[k], src);
      u.bias[k] = __shfl(t.bias[k], src);
    }
    u.sign = __shfl(t.sign, src);
    u.status = 0;
    const int bx = __shfl(box.x0, src), by = __shfl(box.y0, src), bw = __shfl(box.w, src), bh = __shfl(box.h, src);
    const int tri = (int)(ti - lane + src);
    const int n = bw * bh;               // at most 16384^2 = 2^28
    for (int p = lane; p < n; p += 64) {
      const int y = p / bw, x = p - y * bw;
      raster_pixel(u, tri, bx + x, by + y, W, zview);
    }
  }
}

template <bool kAttrs>
__global__ __launch_bounds__(kRasterThreads) void k_raster_resolve(const unsigned long long* __restrict__ zbuf,
                                                                   const float4* __restrict__ screen, int nv,
                                                                   const int32_t* __restrict__ triangles, int nt, long pixels,
                                                                   int W, const float* __restrict__ attrs, int C,
                                                                   RasterAttrBg bg, int32_t* __restrict__ tri_out,
                                                                   float* __restrict__ depth, float* __restrict__ out) {
  const long p = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (p >= pixels) return;
  const int view = blockIdx.y;
  const size_t at = (size_t)view * pixels + p;
  const unsigned long long key = zbuf[at];
  const int tri = (int)(unsigned)(key & 0xFFFFFFFFull);
  int i0 = -1, i1 = -1, i2 = -1;
  bool hit = key != ~0ull && (unsigned)tri < (unsigned)nt;
  if (hit) {
    i0 = triangles[3 * (size_t)tri], i1 = triangles[3 * (size_t)tri + 1], i2 = triangles[3 * (size_t)tri + 2];
    hit = (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv;
  }
  if (!hit) {
    tri_out[at] = -1;
    depth[at] = __builtin_inff();
    if (kAttrs)
      for (int c = 0; c < C; ++c) out[at * C + c] = bg.v[c];
    return;
  }
  tri_out[at] = tri;
  depth[at] = 1.f / __uint_as_float(~(unsigned)(key >> 32));
  if (!kAttrs) return;
  const float4* sv = screen + (size_t)view * nv;
  const RasterTri t = raster_setup(sv[i0], sv[i1], sv[i2], 0);
  long b[3];
  raster_edges(t, (int)(p % W), (int)(p / W), b);
  // perspective-correct weights l_k = b_k q_k / sum b q; out = a0 + l1 (a1 - a0) + l2 (a2 - a0): a constant comes back exactly
  const float w0 = (float)b[0] * t.q[0], w1 = (float)b[1] * t.q[1], w2 = (float)b[2] * t.q[2];
  const float den = w0 + w1 + w2;
  const float l1 = w1 / den, l2 = w2 / den;
  for (int c = 0; c < C; ++c) {
    const float a0 = attrs[(size_t)i0 * C + c], a1 = attrs[(size_t)i1 * C + c], a2 = attrs[(size_t)i2 * C + c];
    out[at * C + c] = fmaf(l1, a1 - a0, fmaf(l2, a2 - a0, a0));
  }
}

// one texel of the atlas as a colour in [0, 1]
struct RasterRgb {
  float c[3];
};

__device__ inline RasterRgb raster_texel(const uint8_t* __restrict__ atlas, int Wa, int x, int y) {
  const uint8_t* __restrict__ t = atlas + 3 * ((size_t)y * Wa + x);
  return RasterRgb{{__fdiv_rn((float)t[0], 255.f), __fdiv_rn((float)t[1], 255.f), __fdiv_rn((float)t[2], 255.f)}};
}

// k_raster_resolve<true> with a per-triangle texture atlas (csrc/jt_texture.hip) in place of vertex attributes: the same winner,
// depth and weights l1, l2; the colour is the bilinear sample of the winner's chart at chart coordinates (l1 L, l2 L), its four
// texels clamped into the block -- the upper chart of a block (odd triangles) is the lower one turned by 180 degrees.
__global__ __launch_bounds__(kRasterThreads) void k_raster_resolve_texture(const unsigned long long* __restrict__ zbuf,
                                                                           const float4* __restrict__ screen, int nv,
                                                                           const int32_t* __restrict__ triangles, int nt,
                                                                           long pixels, int W, const uint8_t* __restrict__ atlas,
                                                                           int S, int cols, int Wa, RasterRgb bg,
                                                                           int32_t* __restrict__ tri_out, float* __restrict__ depth,
                                                                           float* __restrict__ out) {
  const long p = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (p >= pixels) return;
  const int view = blockIdx.y;
  const size_t at = (size_t)view * pixels + p;
  const unsigned long long key = zbuf[at];
  const int tri = (int)(unsigned)(key & 0xFFFFFFFFull);
  int i0 = -1, i1 = -1, i2 = -1;
  bool hit = key != ~0ull && (unsigned)tri < (unsigned)nt;
  if (hit) {
    i0 = triangles[3 * (size_t)tri], i1 = triangles[3 * (size_t)tri + 1], i2 = triangles[3 * (size_t)tri + 2];
    hit = (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv;
  }
  if (!hit) {
    tri_out[at] = -1;
    depth[at] = __builtin_inff();
    for (int c = 0; c < 3; ++c) out[at * 3 + c] = bg.c[c];
    return;
  }
  tri_out[at] = tri;
  depth[at] = 1.f / __uint_as_float(~(unsigned)(key >> 32));
  const float4* sv = screen + (size_t)view * nv;
  const RasterTri t = raster_setup(sv[i0], sv[i1], sv[i2], 0);
  long b[3];
  raster_edges(t, (int)(p % W), (int)(p / W), b);
  const float w0 = (float)b[0] * t.q[0], w1 = (float)b[1] * t.q[1], w2 = (float)b[2] * t.q[2];
  const float den = w0 + w1 + w2;
  const float l1 = w1 / den, l2 = w2 / den;
  const float L = (float)(S - 3);
  const float s = l1 * L, u = l2 * L;
  const int ci = min(max((int)floorf(s), 0), S - 2), cj = min(max((int)floorf(u), 0), S - 2);
  const float fx = s - (float)ci, fy = u - (float)cj;
  const int block = tri >> 1;
  const int x0 = (block % cols) * S, y0 = (block / cols) * S;      // (the entry point has checked that block lies in the atlas)
  const bool upper = tri & 1;
  RasterRgb c[2][2];
#pragma unroll
  for (int dj = 0; dj < 2; ++dj)
#pragma unroll
    for (int di = 0; di < 2; ++di) {
      const int i = ci + di, j = cj + dj;
      c[dj][di] = raster_texel(atlas, Wa, x0 + (upper ? S - 1 - i : i), y0 + (upper ? S - 1 - j : j));
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float top = fmaf(fx, c[0][1].c[k] - c[0][0].c[k], c[0][0].c[k]);
    const float bot = fmaf(fx, c[1][1].c[k] - c[1][0].c[k], c[1][0].c[k]);
    out[at * 3 + k] = fmaf(fy, bot - top, top);
  }
}

// what all three entry points share: the image and batch sizes
static int raster_shape(int n_vertices, int n_views, int H, int W) {
  if (n_vertices < 1 || n_views < 1 || H < 1 || W < 1) return JT_ERR_ARG;
  if (H > 16384 || W > 16384 || n_views > 65535 || (long)n_views * H * W >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  return JT_OK;
}

}  // namespace jt

using namespace jt;

extern "C" int jt_raster_project(const float* vertices, int n_vertices, const float* proj, int n_views, float near, float* screen,
                                 void* stream) {
  if (!vertices || !proj || !screen || n_vertices < 1 || n_views < 1 || !__builtin_isfinite(near)) return JT_ERR_ARG;
  if (n_views > 65535) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_raster_project, dim3((unsigned)(((long)n_vertices + kRasterThreads - 1) / kRasterThreads), (unsigned)n_views),
                     dim3(kRasterThreads), 0, (hipStream_t)stream, vertices, n_vertices, proj, near, (float4*)screen);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_raster_draw(const float* screen, int n_vertices, const int32_t* triangles, long n_triangles, int n_views, int H,
                              int W, int cull, uint64_t* zbuf, uint8_t* status, void* stream) {
  if (!screen || !triangles || !zbuf || !status || n_triangles < 1) return JT_ERR_ARG;
  if (const int rc = raster_shape(n_vertices, n_views, H, W)) return rc;
  if (n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_raster_draw, dim3((unsigned)((n_triangles + kRasterThreads - 1) / kRasterThreads), (unsigned)n_views),
                     dim3(kRasterThreads), 0, (hipStream_t)stream, (const float4*)screen, n_vertices, triangles, (int)n_triangles,
                     H, W, cull, (unsigned long long*)zbuf, status);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_raster_resolve(const uint64_t* zbuf, const float* screen, int n_vertices, const int32_t* triangles,
                                 long n_triangles, int n_views, int H, int W, const float* attrs, int n_attrs,
                                 const float* background, int32_t* tri, float* depth, float* out, void* stream) {
  if (!zbuf || !screen || !triangles || !tri || !depth || n_triangles < 1 || n_attrs < 0) return JT_ERR_ARG;
  if (n_attrs > 0 && (!attrs || !background || !out)) return JT_ERR_ARG;
  if (const int rc = raster_shape(n_vertices, n_views, H, W)) return rc;
  if (n_triangles >= (1l << 31) || n_attrs > kRasterMaxAttrs) return JT_ERR_UNSUPPORTED;
  RasterAttrBg bg;
  for (int c = 0; c < kRasterMaxAttrs; ++c) bg.v[c] = c < n_attrs ? background[c] : 0.f;
  const long pixels = (long)H * W;
  const dim3 grid((unsigned)((pixels + kRasterThreads - 1) / kRasterThreads), (unsigned)n_views);
  if (n_attrs > 0)
    hipLaunchKernelGGL(k_raster_resolve<true>, grid, dim3(kRasterThreads), 0, (hipStream_t)stream,
                       (const unsigned long long*)zbuf, (const float4*)screen, n_vertices, triangles, (int)n_triangles, pixels, W,
                       attrs, n_attrs, bg, tri, depth, out);
  else
    hipLaunchKernelGGL(k_raster_resolve<false>, grid, dim3(kRasterThreads), 0, (hipStream_t)stream,
                       (const unsigned long long*)zbuf, (const float4*)screen, n_vertices, triangles, (int)n_triangles, pixels, W,
                       attrs, n_attrs, bg, tri, depth, out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_raster_resolve_texture(const uint64_t* zbuf, const float* screen, int n_vertices, const int32_t* triangles,
                                         long n_triangles, int n_views, int H, int W, const uint8_t* atlas, int S, int cols,
                                         int H_atlas, int W_atlas, const float* background, int32_t* tri, float* depth, float* out,
                                         void* stream) {
  if (!zbuf || !screen || !triangles || !atlas || !background || !tri || !depth || !out || n_triangles < 1) return JT_ERR_ARG;
  if (cols < 1 || H_atlas < 1 || W_atlas < 1) return JT_ERR_ARG;
  if (const int rc = raster_shape(n_vertices, n_views, H, W)) return rc;
  if (n_triangles >= (1l << 31) || S < JT_TEXTURE_MIN_BLOCK || S > JT_TEXTURE_MAX_BLOCK || H_atlas > JT_TEXTURE_MAX_SIDE ||
      W_atlas > JT_TEXTURE_MAX_SIDE)
    return JT_ERR_UNSUPPORTED;
  // the atlas is cols x (H_atlas / S) whole blocks and holds a chart for every triangle: no texel outside it is ever named
  if (W_atlas != (long)cols * S || H_atlas % S != 0 || 2l * (H_atlas / S) * cols < n_triangles) return JT_ERR_ARG;
  RasterRgb bg;
  for (int c = 0; c < 3; ++c) bg.c[c] = background[c];
  const long pixels = (long)H * W;
  const dim3 grid((unsigned)((pixels + kRasterThreads - 1) / kRasterThreads), (unsigned)n_views);
  hipLaunchKernelGGL(k_raster_resolve_texture, grid, dim3(kRasterThreads), 0, (hipStream_t)stream, (const unsigned long long*)zbuf,
                     (const float4*)screen, n_vertices, triangles, (int)n_triangles, pixels, W, atlas, S, cols, W_atlas, bg, tri,
                     depth, out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
