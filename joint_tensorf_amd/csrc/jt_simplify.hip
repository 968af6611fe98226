// A triangle mesh simplified by vertex clustering with a quadric (Hermite) representative (include/jt_render.h: "Mesh
// simplification").  Vertices are binned into a uniform grid of cells over a box (k_simplify_keys, one lane per vertex); the
// caller sorts the keys stably and scans the run heads; every occupied cell becomes one vertex placed where the planes
// (position, normal) of its members meet in the least-squares sense, regularised towards their mean (k_simplify_clusters, one
// lane per cluster, walking its members serially in ascending vertex id: the order of every sum is part of the contract);
// triangles are re-indexed and the collapsed ones marked (k_simplify_triangles, one lane per triangle) for jt_mesh_filter_emit
// to compact.  256 threads, 64-bit indexing, no LDS, no atomics: two runs give the same bits.
//
// Numerics: the key is four correctly rounded fp32 operations, the representative a fixed sequence of correctly rounded fp64
// operations (contraction off, __fdiv_rn / __ddiv_rn / __dsqrt_rn), so a NumPy statement of the header reproduces both bit for bit.
#include "jt_common.h"

namespace jt {

constexpr int kSimplifyThreads = 256;

struct SimplifyGrid {
  float lo[3], hi[3];
  int cells[3];
};

// cell index of coordinate x on an axis: floorf(((x - lo) / (hi - lo)) * float(cells)) clamped to [0, cells - 1]
__device__ inline long simplify_cell(float x, float lo, float hi, int cells) {
#pragma clang fp contract(off)
  const float d = x - lo;
  const float w = hi - lo;
  const float s = __fdiv_rn(d, w);
  const float f = s * (float)cells;
  return f >= (float)cells ? (long)(cells - 1) : f < 0.f ? 0l : (long)floorf(f);      // (f is no NaN: x is finite, w > 0)
}

__global__ __launch_bounds__(kSimplifyThreads) void k_simplify_keys(const float* __restrict__ vertices, long n, SimplifyGrid g,
                                                                     int64_t* __restrict__ keys) {
  const long i = (long)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (i >= n) return;
  const float x = vertices[3 * i], y = vertices[3 * i + 1], z = vertices[3 * i + 2];
  const long cy = g.cells[1], cz = g.cells[2];
  long key = (long)g.cells[0] * cy * cz;                       // the "none" cluster
  if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) {
    const long ix = simplify_cell(x, g.lo[0], g.hi[0], g.cells[0]);
    const long iy = simplify_cell(y, g.lo[1], g.hi[1], g.cells[1]);
    const long iz = simplify_cell(z, g.lo[2], g.hi[2], g.cells[2]);
    key = (ix * cy + iy) * cz + iz;
  }
  keys[i] = key;
}

// One lane per cluster j: members order[seg_start[j] .. seg_start[j + 1]) in that order.  Everything in fp64 from the fp32
// inputs, every operation rounded on its own, every sum sequential from 0.0; the order of operations is the header's.
__global__ __launch_bounds__(kSimplifyThreads) void k_simplify_clusters(
    const float* __restrict__ vertices, const float* __restrict__ normals, long n, const int64_t* __restrict__ order,
    const int64_t* __restrict__ seg_start, long n_clusters, float lambda, float* __restrict__ positions,
    float* __restrict__ normals_out, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
  const long j = (long)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (j >= n_clusters) return;
  long first = seg_start[j], last = seg_start[j + 1];
  first = first < 0 ? 0 : first > n ? n : first;               // (no address outside order [n], whatever the scan says)
  last = last < first ? first : last > n ? n : last;
  // ---- pass 1: the mean and the members' box ----
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  float mn0 = INFINITY, mn1 = INFINITY, mn2 = INFINITY, mx0 = -INFINITY, mx1 = -INFINITY, mx2 = -INFINITY;
  long m = 0;
  for (long q = first; q < last; ++q) {
    const long v = order[q];
    if (v < 0 || v >= n) continue;                             // (an id outside [0, n) is no member)
    const float p0 = vertices[3 * v], p1 = vertices[3 * v + 1], p2 = vertices[3 * v + 2];
    s0 = s0 + (double)p0;
    s1 = s1 + (double)p1;
    s2 = s2 + (double)p2;
    mn0 = fminf(mn0, p0), mn1 = fminf(mn1, p1), mn2 = fminf(mn2, p2);
    mx0 = fmaxf(mx0, p0), mx1 = fmaxf(mx1, p1), mx2 = fmaxf(mx2, p2);
    ++m;
  }
  float* __restrict__ po = positions + 3 * j;
  float* __restrict__ no = normals_out + 3 * j;
  counts[j] = (int32_t)m;
  if (m == 0) {
    po[0] = po[1] = po[2] = 0.f;
    no[0] = no[1] = no[2] = 0.f;
    return;
  }
  const double dm = (double)m;
  const double c0 = __ddiv_rn(s0, dm), c1 = __ddiv_rn(s1, dm), c2 = __ddiv_rn(s2, dm);
  // ---- pass 2: the planes of the members about the mean ----
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  double sn0 = 0.0, sn1 = 0.0, sn2 = 0.0;
  for (long q = first; q < last; ++q) {
    const long v = order[q];
    if (v < 0 || v >= n) continue;
    const double d0 = (double)vertices[3 * v] - c0, d1 = (double)vertices[3 * v + 1] - c1, d2 = (double)vertices[3 * v + 2] - c2;
    const float f0 = normals[3 * v], f1 = normals[3 * v + 1], f2 = normals[3 * v + 2];
    const bool ok = __builtin_isfinite(f0) && __builtin_isfinite(f1) && __builtin_isfinite(f2);
    const double n0 = ok ? (double)f0 : 0.0, n1 = ok ? (double)f1 : 0.0, n2 = ok ? (double)f2 : 0.0;
    const double e = (n0 * d0 + n1 * d1) + n2 * d2;
    a00 = a00 + n0 * n0;
    a01 = a01 + n0 * n1;
    a02 = a02 + n0 * n2;
    a11 = a11 + n1 * n1;
    a12 = a12 + n1 * n2;
    a22 = a22 + n2 * n2;
    b0 = b0 + n0 * e;
    b1 = b1 + n1 * e;
    b2 = b2 + n2 * e;
    sn0 = sn0 + n0;
    sn1 = sn1 + n1;
    sn2 = sn2 + n2;
  }
  const double r = (double)lambda * dm;
  a00 = a00 + r;
  a11 = a11 + r;
  a22 = a22 + r;
  // ---- A x = b by the cofactors of the symmetric matrix ----
  const double k00 = a11 * a22 - a12 * a12;
  const double k01 = a02 * a12 - a01 * a22;
  const double k02 = a01 * a12 - a02 * a11;
  const double k11 = a00 * a22 - a02 * a02;
  const double k12 = a01 * a02 - a00 * a12;
  const double k22 = a00 * a11 - a01 * a01;
  const double det = (a00 * k00 + a01 * k01) + a02 * k02;
  const double x0 = __ddiv_rn((k00 * b0 + k01 * b1) + k02 * b2, det);
  const double x1 = __ddiv_rn((k01 * b0 + k11 * b1) + k12 * b2, det);
  const double x2 = __ddiv_rn((k02 * b0 + k12 * b1) + k22 * b2, det);
  po[0] = fminf(fmaxf((float)(c0 + x0), mn0), mx0);
  po[1] = fminf(fmaxf((float)(c1 + x1), mn1), mx1);
  po[2] = fminf(fmaxf((float)(c2 + x2), mn2), mx2);
  const double len = __dsqrt_rn((sn0 * sn0 + sn1 * sn1) + sn2 * sn2);
  const bool unit = len > 0.0 && __builtin_isfinite(len);      // (false for a NaN)
  no[0] = unit ? (float)__ddiv_rn(sn0, len) : 0.f;
  no[1] = unit ? (float)__ddiv_rn(sn1, len) : 0.f;
  no[2] = unit ? (float)__ddiv_rn(sn2, len) : 0.f;
}

constexpr uint8_t kSimplifyKept = 0, kSimplifyInvalid = 1, kSimplifyCollapsed = 2;

// t' = (cluster[a], cluster[b], cluster[c]); used[j] = 1 for the clusters of a kept triangle (zeroed by the caller; lanes that
// store the same 1 do not race for a value)
__global__ __launch_bounds__(kSimplifyThreads) void k_simplify_triangles(const int32_t* __restrict__ triangles, long nt,
                                                                          const int32_t* __restrict__ cluster, long nv, long nc,
                                                                          int32_t* __restrict__ triangles_out,
                                                                          uint8_t* __restrict__ keep, uint8_t* __restrict__ cause,
                                                                          uint8_t* __restrict__ used) {
  const long t = (long)blockIdx.x * kSimplifyThreads + threadIdx.x;
  if (t >= nt) return;
  long cl[3];
  bool invalid = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long id = triangles[3 * t + c];
    long j = (id >= 0 && id < nv) ? (long)cluster[id] : -1l;
    j = (j >= 0 && j < nc) ? j : -1l;
    invalid |= j < 0;
    cl[c] = j;
    triangles_out[3 * t + c] = (int32_t)j;
  }
  const bool collapsed = cl[0] == cl[1] || cl[1] == cl[2] || cl[0] == cl[2];
  const bool k = !invalid && !collapsed;
  keep[t] = k ? 1 : 0;
  cause[t] = invalid ? kSimplifyInvalid : collapsed ? kSimplifyCollapsed : kSimplifyKept;
  if (k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) used[cl[c]] = 1;
  }
}

}  // namespace jt

using namespace jt;

extern "C" int jt_simplify_keys(const float* vertices, long n, const float* lo3, const float* hi3, const int* cells3,
                                int64_t* keys, void* stream) {
  if (!vertices || !lo3 || !hi3 || !cells3 || !keys || n < 1) return JT_ERR_ARG;
  SimplifyGrid g;
  for (int a = 0; a < 3; ++a) {
    const float w = hi3[a] - lo3[a];
    if (!__builtin_isfinite(lo3[a]) || !__builtin_isfinite(hi3[a]) || !(hi3[a] > lo3[a]) || !__builtin_isfinite(w)) return JT_ERR_ARG;
    if (cells3[a] < 1 || cells3[a] > (1 << 20)) return JT_ERR_ARG;
    g.lo[a] = lo3[a];
    g.hi[a] = hi3[a];
    g.cells[a] = cells3[a];
  }
  if (n >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_simplify_keys, dim3((unsigned)((n + kSimplifyThreads - 1) / kSimplifyThreads)), dim3(kSimplifyThreads), 0,
                     (hipStream_t)stream, vertices, n, g, keys);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_simplify_clusters(const float* vertices, const float* normals, long n, const int64_t* order,
                                    const int64_t* seg_start, long n_clusters, float lambda, float* positions,
                                    float* normals_out, int32_t* counts, void* stream) {
  if (!vertices || !normals || !order || !seg_start || !positions || !normals_out || !counts || n < 1 || n_clusters < 1)
    return JT_ERR_ARG;
  if (!(lambda > 0.f) || !__builtin_isfinite(lambda) || n_clusters > n) return JT_ERR_ARG;
  if (n >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_simplify_clusters, dim3((unsigned)((n_clusters + kSimplifyThreads - 1) / kSimplifyThreads)),
                     dim3(kSimplifyThreads), 0, (hipStream_t)stream, vertices, normals, n, order, seg_start, n_clusters, lambda,
                     positions, normals_out, counts);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_simplify_triangles(const int32_t* triangles, long n_triangles, const int32_t* cluster, long n_vertices,
                                     long n_clusters, int32_t* triangles_out, uint8_t* keep, uint8_t* cause, uint8_t* used,
                                     void* stream) {
  if (!triangles || !cluster || !triangles_out || !keep || !cause || !used || n_triangles < 1 || n_vertices < 1 || n_clusters < 1)
    return JT_ERR_ARG;
  if (n_clusters > n_vertices) return JT_ERR_ARG;
  if (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_simplify_triangles, dim3((unsigned)((n_triangles + kSimplifyThreads - 1) / kSimplifyThreads)),
                     dim3(kSimplifyThreads), 0, (hipStream_t)stream, triangles, n_triangles, cluster, n_vertices, n_clusters,
                     triangles_out, keep, cause, used);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
