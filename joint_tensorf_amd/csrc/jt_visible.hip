// The surface the cameras see (include/jt_render.h: "Visible surface").  jt_raster_draw leaves, per pixel of every view, the index
// of the nearest triangle in the low word of a 64-bit key; here those winners are tallied per (view, triangle)
// (k_visible_tally), the tallies folded into per-triangle view and pixel counts (k_visible_fold), the seen set grown by rings of
// vertex neighbours (k_visible_mark, k_visible_spread: two launches, the step between them is a grid-wide dependency) and the
// triangles that stay marked for jt_mesh_filter_emit to compact (k_mesh_select_count).  256 threads, 64-bit indexing, no LDS.
// Integer work only, and the only atomics are integer additions: two runs give the same bits.
#include <stdlib.h>

#include "jt_common.h"

namespace jt {

constexpr int kVisibleThreads = 256;
constexpr uint64_t kVisibleEmpty = ~0ull;                      // the key jt_raster_draw's caller clears the z-buffer with

// One lane per pixel, lanes on consecutive pixels.  RUNS: neighbouring pixels mostly share a winner, so a wave adds a run of equal
// (view, index) once, with the run's length, from its first lane; the view is part of what is compared, so a run ends where a
// view does (hw need not be a multiple of 64: a wave can straddle two views).  Every lane of a workgroup reaches the shuffle and
// the ballot: lanes past the end carry the "nothing" destination.  !RUNS: one atomic per counted pixel.
template <bool RUNS>
__global__ __launch_bounds__(kVisibleThreads) void k_visible_tally(const uint64_t* __restrict__ zbuf, long n_pixels, unsigned hw,
                                                                    unsigned nt, uint32_t* __restrict__ pix) {
  const long i = (long)blockIdx.x * kVisibleThreads + threadIdx.x;
  const bool in = i < n_pixels;
  const uint64_t key = in ? zbuf[i] : kVisibleEmpty;
  const unsigned idx = (unsigned)(key & 0xffffffffull);
  const bool counted = in && key != kVisibleEmpty && idx < nt;   // (a low word >= nt is skipped, never an index)
  const unsigned view = in ? (unsigned)i / hw : 0u;              // (n_pixels < 2^31)
  const long dest = counted ? (long)view * (long)nt + (long)idx : -1l;
  if (!RUNS) {
    if (counted) atomicAdd(pix + dest, 1u);
    return;
  }
  const int lane = (int)(threadIdx.x & 63u);
  // the destination of the lane below, 64 bits as two words
  const int lo_below = __shfl_up((int)(unsigned)((uint64_t)dest & 0xffffffffull), 1, 64);
  const int hi_below = __shfl_up((int)(unsigned)((uint64_t)dest >> 32), 1, 64);
  const long below = (long)(((uint64_t)(unsigned)hi_below << 32) | (uint64_t)(unsigned)lo_below);
  const bool head = lane == 0 || below != dest;
  const unsigned long long heads = __ballot(head);
  if (head && counted) {
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const unsigned len = above ? (unsigned)__ffsll((long long)above) : (unsigned)(64 - lane);   // to the next head, or the wave's end
    atomicAdd(pix + dest, len);
  }
}

// One lane per triangle, walking the views of the slab in order: no atomics.
__global__ __launch_bounds__(kVisibleThreads) void k_visible_fold(const uint32_t* __restrict__ pix, int n_views, long nt,
                                                                   unsigned min_pixels, int32_t* __restrict__ views,
                                                                   int64_t* __restrict__ pixels) {
  const long t = (long)blockIdx.x * kVisibleThreads + threadIdx.x;
  if (t >= nt) return;
  int32_t nv = 0;
  int64_t np = 0;
  for (int v = 0; v < n_views; ++v) {
    const uint32_t c = pix[(long)v * nt + t];
    nv += c >= min_pixels ? 1 : 0;
    np += (int64_t)c;
  }
  views[t] += nv;
  pixels[t] += np;
}

// the three vertex ids of triangle t; false when one lies outside [0, nv)
__device__ inline bool visible_ids(const int32_t* __restrict__ triangles, long t, long nv, long id[3]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    id[c] = (long)triangles[3 * t + c];
    ok = ok && id[c] >= 0 && id[c] < nv;
  }
  return ok;
}

// flag[v] = 1 for the vertices of visible triangles (zeroed by the caller; lanes that store the same 1 do not race for a value)
__global__ __launch_bounds__(kVisibleThreads) void k_visible_mark(const int32_t* __restrict__ triangles, long nt, long nv,
                                                                   const uint8_t* __restrict__ visible, uint8_t* __restrict__ flag) {
  const long t = (long)blockIdx.x * kVisibleThreads + threadIdx.x;
  if (t >= nt || visible[t] == 0) return;
  long id[3];
  if (!visible_ids(triangles, t, nv, id)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) flag[id[c]] = 1;
}

__global__ __launch_bounds__(kVisibleThreads) void k_visible_spread(const int32_t* __restrict__ triangles, long nt, long nv,
                                                                     const uint8_t* __restrict__ visible_in,
                                                                     const uint8_t* __restrict__ flag, uint8_t* __restrict__ visible_out) {
  const long t = (long)blockIdx.x * kVisibleThreads + threadIdx.x;
  if (t >= nt) return;
  long id[3];
  bool touched = false;
  if (visible_ids(triangles, t, nv, id)) touched = (flag[id[0]] | flag[id[1]] | flag[id[2]]) != 0;
  visible_out[t] = (uint8_t)(visible_in[t] | (touched ? 1 : 0));
}

// keep_out[t] = keep_in[t] != 0 and ids in range; used[v] = 1 for the vertices of kept triangles (zeroed by the caller)
__global__ __launch_bounds__(kVisibleThreads) void k_mesh_select_count(const int32_t* __restrict__ triangles, long nt, long nv,
                                                                        const uint8_t* __restrict__ keep_in,
                                                                        uint8_t* __restrict__ keep_out, uint8_t* __restrict__ used) {
  const long t = (long)blockIdx.x * kVisibleThreads + threadIdx.x;
  if (t >= nt) return;
  long id[3];
  const bool k = visible_ids(triangles, t, nv, id) && keep_in[t] != 0;
  keep_out[t] = k ? 1 : 0;
  if (k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) used[id[c]] = 1;
  }
}

static unsigned visible_blocks(long n) { return (unsigned)((n + kVisibleThreads - 1) / kVisibleThreads); }

}  // namespace jt

using namespace jt;

extern "C" int jt_visible_tally(const uint64_t* zbuf, int n_views, int H, int W, long n_triangles, uint32_t* pix, void* stream) {
  if (!zbuf || !pix || n_views < 1 || H < 1 || W < 1 || n_triangles < 1) return JT_ERR_ARG;
  const long n_pixels = (long)n_views * H * W;
  if (n_pixels >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  // JT_VISIBLE_RUNS=0: one atomic per pixel instead of one per run of a wave (profiles/mesh_visible.txt has both timings)
  const char* e = getenv("JT_VISIBLE_RUNS");
  const bool runs = !e || atoi(e) != 0;
  const dim3 grid(visible_blocks(n_pixels)), block(kVisibleThreads);
  if (runs)
    hipLaunchKernelGGL(k_visible_tally<true>, grid, block, 0, (hipStream_t)stream, zbuf, n_pixels, (unsigned)((long)H * W),
                       (unsigned)n_triangles, pix);
  else
    hipLaunchKernelGGL(k_visible_tally<false>, grid, block, 0, (hipStream_t)stream, zbuf, n_pixels, (unsigned)((long)H * W),
                       (unsigned)n_triangles, pix);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_visible_fold(const uint32_t* pix, int n_views, long n_triangles, int min_pixels, int32_t* views, int64_t* pixels,
                               void* stream) {
  if (!pix || !views || !pixels || n_views < 1 || n_triangles < 1 || min_pixels < 1) return JT_ERR_ARG;
  if (3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_visible_fold, dim3(visible_blocks(n_triangles)), dim3(kVisibleThreads), 0, (hipStream_t)stream, pix, n_views,
                     n_triangles, (unsigned)min_pixels, views, pixels);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_visible_mark(const int32_t* triangles, long n_triangles, long n_vertices, const uint8_t* visible, uint8_t* flag,
                               void* stream) {
  if (!triangles || !visible || !flag || n_triangles < 1 || n_vertices < 1) return JT_ERR_ARG;
  if (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_visible_mark, dim3(visible_blocks(n_triangles)), dim3(kVisibleThreads), 0, (hipStream_t)stream, triangles,
                     n_triangles, n_vertices, visible, flag);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_visible_spread(const int32_t* triangles, long n_triangles, long n_vertices, const uint8_t* visible_in,
                                 const uint8_t* flag, uint8_t* visible_out, void* stream) {
  if (!triangles || !visible_in || !flag || !visible_out || n_triangles < 1 || n_vertices < 1) return JT_ERR_ARG;
  if (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_visible_spread, dim3(visible_blocks(n_triangles)), dim3(kVisibleThreads), 0, (hipStream_t)stream, triangles,
                     n_triangles, n_vertices, visible_in, flag, visible_out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_mesh_select_count(const int32_t* triangles, long n_triangles, long n_vertices, const uint8_t* keep_in,
                                    uint8_t* keep_out, uint8_t* used, void* stream) {
  if (!triangles || !keep_in || !keep_out || !used || n_triangles < 1 || n_vertices < 1) return JT_ERR_ARG;
  if (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_mesh_select_count, dim3(visible_blocks(n_triangles)), dim3(kVisibleThreads), 0, (hipStream_t)stream, triangles,
                     n_triangles, n_vertices, keep_in, keep_out, used);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
