// Depth-map fusion (include/jt_render.h: "Depth-map fusion"): the depth maps a field renders from its cameras fused into a
// truncated signed distance volume on the lattice jt_mesh_count / jt_mesh_emit extract.  k_fusion_integrate: one lane per lattice
// point, consecutive lanes along z, the views of the call walked in ascending order with the point's two accumulators in
// registers -- the state is read and written once per call, so slabs of views compose to the bits of one call.  k_fusion_finish:
// the state to an occupancy-like lattice (surface at 0.5) and a `seen` byte.  256 threads, no LDS, no atomics.
//
// Every fp32 operation is rounded on its own (#pragma clang fp contract(off), IEEE division): tests/fusion_ref.py states the same
// sequence in NumPy float32 and holds the kernels to its bits.  The twelve projection floats of a view are read at an index that
// depends on the loop counter alone, so they are wave-uniform: scalar loads into scalar registers, no vector memory traffic.
// What a lane gathers is one depth and one opacity texel per view it lies in front of and inside the frame of; a wave's 64
// points are a run along z, whose pixels lie on a short line segment of the image: a few cache lines per wave and view.
#include "jt_common.h"

namespace jt {

constexpr int kFusionThreads = 256;

struct FusionBox {
  float lo[3], hi[3];
};

// jt_mesh_emit's lattice coordinate (csrc/jt_mesh.hip: mesh_coord), operation for operation
__device__ inline float fusion_coord(float lo, float hi, int i, int n) {
#pragma clang fp contract(off)
  const float s = (float)i / (float)(n - 1);
  return lo * (1.f - s) + hi * s;
}

__global__ __launch_bounds__(kFusionThreads) void k_fusion_integrate(const float* __restrict__ depth, const float* __restrict__ opacity,
                                                                      const float* __restrict__ proj, int n_views, int H, int W,
                                                                      int nx, int ny, int nz, FusionBox box, float trunc,
                                                                      float min_opacity, int carve, float near,
                                                                      float* __restrict__ sum, int32_t* __restrict__ count) {
#pragma clang fp contract(off)
  const int n = nx * ny * nz;                                         // (at most 2^27: the entry point refuses more)
  const int idx = (int)(blockIdx.x * kFusionThreads + threadIdx.x);
  if (idx >= n) return;
  const int k = idx % nz;
  const int r = idx / nz;
  const int j = r % ny;
  const int i = r / ny;
  const float x = fusion_coord(box.lo[0], box.hi[0], i, nx);
  const float y = fusion_coord(box.lo[1], box.hi[1], j, ny);
  const float z = fusion_coord(box.lo[2], box.hi[2], k, nz);
  const float wf = (float)W, hf = (float)H, neg_trunc = -trunc;
  const size_t hw = (size_t)H * (size_t)W;
  float acc = sum[idx];
  int32_t cnt = count[idx];
  for (int view = 0; view < n_views; ++view) {
    const float* __restrict__ p = proj + 12 * (size_t)view;          // (wave-uniform: scalar loads)
    const float w = ((p[8] * x + p[9] * y) + p[10] * z) + p[11];
    if (!(w > near)) continue;
    const float xw = ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
    const float yw = ((p[4] * x + p[5] * y) + p[6] * z) + p[7];
    const float u = xw / w, v = yw / w;
    if (!(u >= 0.f && u < wf && v >= 0.f && v < hf)) continue;       // (a NaN fails)
    const int col = (int)u, row = (int)v;                            // (0 <= col < W, 0 <= row < H: the test above)
    const size_t at = (size_t)view * hw + (size_t)row * (size_t)W + (size_t)col;
    const float d = depth[at], a = opacity[at];
    if (!(__builtin_isfinite(d) && d > 0.f && a >= min_opacity)) {   // the ray found no surface: the point is seen empty
      if (carve) {
        acc = acc + 1.f;
        cnt += 1;
      }
      continue;
    }
    const float s = d - w;
    if (s < neg_trunc) continue;                                     // occluded
    float t = s / trunc;
    t = t > 1.f ? 1.f : t;
    acc = acc + t;
    cnt += 1;
  }
  sum[idx] = acc;
  count[idx] = cnt;
}

__global__ __launch_bounds__(kFusionThreads) void k_fusion_finish(const float* __restrict__ sum, const int32_t* __restrict__ count, long n,
                                                                   int min_views, float* __restrict__ lattice,
                                                                   uint8_t* __restrict__ seen) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * kFusionThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t c = count[i];
  const bool ok = c >= min_views;
  const float mean = sum[i] / (float)c;
  lattice[i] = ok ? 0.5f * (1.f - mean) : 0.f;
  seen[i] = ok ? 1 : 0;
}

}  // namespace jt

using namespace jt;

extern "C" int jt_fusion_integrate(const float* depth, const float* opacity, const float* proj, int n_views, int H, int W, int nx,
                                   int ny, int nz, const float* lo3, const float* hi3, float trunc, float min_opacity, int carve,
                                   float near, float* sum, int32_t* count, void* stream) {
  if (!lo3 || !hi3 || !sum || !count || nx < 2 || ny < 2 || nz < 2 || n_views < 0 || H < 1 || W < 1) return JT_ERR_ARG;
  if (!(trunc > 0.f) || !__builtin_isfinite(trunc) || min_opacity != min_opacity || near != near) return JT_ERR_ARG;
  const long n = (long)nx * (long)ny * (long)nz;
  if (n > (1l << 27)) return JT_ERR_UNSUPPORTED;
  if ((long)n_views * (long)H * (long)W >= (1l << 31)) return JT_ERR_UNSUPPORTED;      // (each factor < 2^31: no overflow)
  if (n_views == 0) return JT_OK;
  if (!depth || !opacity || !proj) return JT_ERR_ARG;
  FusionBox box;
  for (int a = 0; a < 3; ++a) {
    box.lo[a] = lo3[a];
    box.hi[a] = hi3[a];
  }
  hipLaunchKernelGGL(k_fusion_integrate, dim3((unsigned)((n + kFusionThreads - 1) / kFusionThreads)), dim3(kFusionThreads), 0,
                     (hipStream_t)stream, depth, opacity, proj, n_views, H, W, nx, ny, nz, box, trunc, min_opacity, carve ? 1 : 0,
                     near, sum, count);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_fusion_finish(const float* sum, const int32_t* count, long n, int min_views, float* lattice, uint8_t* seen,
                                void* stream) {
  if (!sum || !count || !lattice || !seen || n < 1 || min_views < 1) return JT_ERR_ARG;
  if (n > (1l << 27)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_fusion_finish, dim3((unsigned)((n + kFusionThreads - 1) / kFusionThreads)), dim3(kFusionThreads), 0,
                     (hipStream_t)stream, sum, count, n, min_views, lattice, seen);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
