// Iso-surface of a scalar lattice as a triangle mesh: marching tetrahedra on the Kuhn (Freudenthal) triangulation of every
// lattice cell.  A cell splits into six tetrahedra, one per permutation (a, b, c) of the axes, with corners c0 = (0,0,0),
// c1 = c0 + e_a, c2 = c1 + e_b, c3 = (1,1,1): every face diagonal runs from the face's minimum to its maximum corner, so two
// cells triangulate their common face alike and the surface is a closed oriented 2-manifold wherever it does not leave the lattice.
//
// Every tetrahedron edge joins a lattice point p to p + d with d one of seven offsets, "kinds" 0..6 = +x, +y, +z, +x+y, +x+z,
// +y+z, +x+y+z; p OWNS the edge and the mesh vertex on it.  Two passes with a scan between them (the caller's): k_mesh_count
// writes per point which owned edges are cut and how many triangles its cell makes, k_mesh_emit writes vertex `vert_offset[p] +
// rank of the edge among p's cut edges` and the cell's triangles from tri_offset[p] on.  No atomics: the order of the output is
// a function of the lattice alone and two runs give the same bits.
//
// Lattice [nx][ny][nz] fp32, z fastest; a point is inside iff v > level (a NaN is outside).  One thread per point, consecutive
// threads along z; a corner is addressed by its offset mask m = dx | dy << 1 | dz << 2.
//
// Below the extraction: the mesh of a forward-facing (camera.ndc) scene carried from the scene box's NDC coordinates to world
// space, one lane per vertex (k_mesh_unwarp_ndc), and the triangles that lost a vertex on the way removed in the same count /
// scan / emit form (k_mesh_filter_count, k_mesh_filter_emit).  256 threads, 64-bit indexing, no LDS, no atomics.
#include "jt_common.h"

namespace jt {

constexpr int kMeshThreads = 256;

// offset mask of every kind, and the kind of every mask (mask 0 is no edge)
__host__ __device__ constexpr int mesh_mask_of_kind(int k) { return k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 4 : k == 3 ? 3 : k == 4 ? 5 : k == 5 ? 6 : 7; }
__host__ __device__ constexpr int mesh_kind_of_mask(int m) { return m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : m == 3 ? 3 : m == 5 ? 4 : m == 6 ? 5 : 6; }

// The 16 cases of a POSITIVELY oriented tetrahedron (det[c1 - c0, c2 - c0, c3 - c0] > 0: an even permutation of the axes), bit
// q of the case = corner q inside.  Tetrahedron edges: 0 = (0,1), 1 = (0,2), 2 = (0,3), 3 = (1,2), 4 = (1,3), 5 = (2,3).  An entry
// packs the triangle count (bits 0-1) and up to six edge numbers of three bits each from bit 2 on; normals (right-hand rule)
// point from inside to outside.  A lone inside corner q with (q; x, y, z) an even permutation of the corners gives (qx, qy, qz);
// two inside corners I0 < I1 and outside corners O0 < O1 give the quad a = (I0,O0), b = (I0,O1), c = (I1,O1), d = (I1,O0) as
// (a,b,c), (a,c,d) when (I0, I1, O0, O1) is an even permutation and (a,c,b), (a,d,c) when odd; the complement of a case is the
// case with every triangle reversed.  A negatively oriented tetrahedron swaps the last two corners of every triangle.  The
// winding never looks at a position, so a vertex that falls on a lattice point (a value equal to the level) flips nothing.
__host__ __device__ constexpr uint32_t mesh_tris(int n, int a0, int a1, int a2, int b0 = 0, int b1 = 0, int b2 = 0) {
  return (uint32_t)n | (uint32_t)a0 << 2 | (uint32_t)a1 << 5 | (uint32_t)a2 << 8 | (uint32_t)b0 << 11 | (uint32_t)b1 << 14 |
         (uint32_t)b2 << 17;
}
__device__ constexpr uint32_t kMeshCase[16] = {
    0,                                 // 0000
    mesh_tris(1, 0, 1, 2),             // 0001  corner 0 in
    mesh_tris(1, 0, 4, 3),             // 0010  corner 1 in
    mesh_tris(2, 1, 2, 4, 1, 4, 3),    // 0011  0, 1 in
    mesh_tris(1, 1, 3, 5),             // 0100  corner 2 in
    mesh_tris(2, 0, 5, 2, 0, 3, 5),    // 0101  0, 2 in (odd)
    mesh_tris(2, 0, 4, 5, 0, 5, 1),    // 0110  1, 2 in
    mesh_tris(1, 2, 4, 5),             // 0111  corner 3 out
    mesh_tris(1, 2, 5, 4),             // 1000  corner 3 in
    mesh_tris(2, 0, 1, 5, 0, 5, 4),    // 1001  0, 3 in
    mesh_tris(2, 0, 5, 3, 0, 2, 5),    // 1010  1, 3 in (odd)
    mesh_tris(1, 1, 5, 3),             // 1011  corner 2 out
    mesh_tris(2, 1, 3, 4, 1, 4, 2),    // 1100  2, 3 in
    mesh_tris(1, 0, 3, 4),             // 1101  corner 1 out
    mesh_tris(1, 0, 2, 1),             // 1110  corner 0 out
    0};                                // 1111

// the case of tetrahedron (A, B, .) from the cell's eight inside bits (bit m = the corner at offset mask m)
template <int A, int B>
__device__ inline int mesh_tet_case(int cube) {
  constexpr int m1 = 1 << A, m2 = m1 | (1 << B);
  return (cube & 1) | ((cube >> m1) & 1) << 1 | ((cube >> m2) & 1) << 2 | ((cube >> 7) & 1) << 3;
}

__device__ inline int mesh_tris_of_case(int c) {
  const int n = __popc(c);
  return n == 2 ? 2 : (n & 1);
}

// What both kernels need of a point: its indices, which of the three upper neighbours exist, and the eight corner values (a
// corner beyond the lattice reads the nearest one inside: no out-of-bounds address, and no edge or cell uses its value).  A
// thread past the last point works on the last point and stores nothing.
struct MeshPoint {
  int idx, i, j, k;
  bool live, ex, ey, ez;
  float v[8];
};

__device__ inline MeshPoint mesh_point(const float* __restrict__ lattice, int nx, int ny, int nz) {
  MeshPoint p;
  const int n = nx * ny * nz;
  const int t = (int)(blockIdx.x * kMeshThreads + threadIdx.x);
  p.live = t < n;
  p.idx = p.live ? t : n - 1;
  p.k = p.idx % nz;
  const int r = p.idx / nz;
  p.j = r % ny;
  p.i = r / ny;
  p.ex = p.i < nx - 1;
  p.ey = p.j < ny - 1;
  p.ez = p.k < nz - 1;
  const int sx = p.ex ? ny * nz : 0, sy = p.ey ? nz : 0, sz = p.ez ? 1 : 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) p.v[m] = lattice[p.idx + ((m & 1) ? sx : 0) + ((m & 2) ? sy : 0) + ((m & 4) ? sz : 0)];
  return p;
}

__device__ inline bool mesh_edge_exists(const MeshPoint& p, int m) {
  return (!(m & 1) || p.ex) && (!(m & 2) || p.ey) && (!(m & 4) || p.ez);
}

__device__ inline int mesh_cube(const MeshPoint& p, float level) {
  int cube = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) cube |= (p.v[m] > level ? 1 : 0) << m;
  return cube;
}

__device__ inline int mesh_flags(const MeshPoint& p, int cube) {
  int f = 0;
#pragma unroll
  for (int kind = 0; kind < 7; ++kind) {
    const int m = mesh_mask_of_kind(kind);
    f |= (mesh_edge_exists(p, m) && (((cube >> m) ^ cube) & 1)) ? 1 << kind : 0;
  }
  return f;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_count(const float* __restrict__ lattice, int nx, int ny, int nz, float level,
                                                             uint8_t* __restrict__ edge_flags, uint8_t* __restrict__ tri_count) {
  const MeshPoint p = mesh_point(lattice, nx, ny, nz);
  const int cube = mesh_cube(p, level);
  const int f = mesh_flags(p, cube);
  int t = mesh_tris_of_case(mesh_tet_case<0, 1>(cube)) + mesh_tris_of_case(mesh_tet_case<0, 2>(cube)) +
          mesh_tris_of_case(mesh_tet_case<1, 0>(cube)) + mesh_tris_of_case(mesh_tet_case<1, 2>(cube)) +
          mesh_tris_of_case(mesh_tet_case<2, 0>(cube)) + mesh_tris_of_case(mesh_tet_case<2, 1>(cube));
  t = (p.ex && p.ey && p.ez) ? t : 0;
  if (p.live) {
    edge_flags[p.idx] = (uint8_t)f;
    tri_count[p.idx] = (uint8_t)t;
  }
}

struct MeshBox {
  float lo[3], hi[3];
};

// lattice coordinate i of an axis with n points over [lo, hi]: every operation rounded on its own
__device__ inline float mesh_coord(float lo, float hi, int i, int n) {
#pragma clang fp contract(off)
  const float s = (float)i / (float)(n - 1);
  return lo * (1.f - s) + hi * s;
}

// The triangles of tetrahedron (A, B, C) of the cell.  fl[m] / vo[m]: edge flags and first vertex id of the corner at offset mask
// m (m = 0..6: corner 7 owns no edge of its cell).  Returns the number written; a triangle past n_triangles is not stored.
template <int A, int B, int C>
__device__ inline int mesh_emit_tet(int cube, const int (&fl)[7], const int (&vo)[7], long at, long n_triangles,
                                    int32_t* __restrict__ triangles) {
  constexpr int m1 = 1 << A, m2 = m1 | (1 << B);
  constexpr bool odd = (A == 0 && B == 2) || (A == 1 && B == 0) || (A == 2 && B == 1);   // parity of (A, B, C)
  static_assert(A != B && B != C && A != C && C == 3 - A - B, "a permutation of the axes");
  const int c = mesh_tet_case<A, B>(cube);
  const uint32_t e = kMeshCase[c];
  const int n = (int)(e & 3u);
  if (n == 0) return 0;
  // vertex id on tetrahedron edge (u, w): owner corner u's offset plus the rank of the edge's kind among the owner's cut edges
  auto vid = [&](int mu, int mw) { return vo[mu] + __popc(fl[mu] & ((1 << mesh_kind_of_mask(mw ^ mu)) - 1)); };
  const int id0 = vid(0, m1), id1 = vid(0, m2), id2 = vid(0, 7), id3 = vid(m1, m2), id4 = vid(m1, 7), id5 = vid(m2, 7);
  auto pick = [&](uint32_t s) {
    const int q = (int)((e >> s) & 7u);
    return q == 0 ? id0 : q == 1 ? id1 : q == 2 ? id2 : q == 3 ? id3 : q == 4 ? id4 : id5;
  };
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < n && (unsigned long)(at + t) < (unsigned long)n_triangles) {
      const int a = pick(2 + 9 * t), b = pick(5 + 9 * t), d = pick(8 + 9 * t);
      int32_t* __restrict__ o = triangles + 3 * (at + t);
      o[0] = a;
      o[1] = odd ? d : b;
      o[2] = odd ? b : d;
    }
  }
  return n;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_emit(const float* __restrict__ lattice, int nx, int ny, int nz, float level,
                                                            MeshBox box, const uint8_t* __restrict__ edge_flags,
                                                            const int64_t* __restrict__ vert_offset,
                                                            const int64_t* __restrict__ tri_offset, long n_vertices,
                                                            long n_triangles, float* __restrict__ vertices,
                                                            int32_t* __restrict__ triangles) {
#pragma clang fp contract(off)
  const MeshPoint p = mesh_point(lattice, nx, ny, nz);
  const int cube = mesh_cube(p, level);
  // edge flags and first vertex ids of the seven corners that own edges of this cell (clamped like the values)
  const int sx = p.ex ? ny * nz : 0, sy = p.ey ? nz : 0, sz = p.ez ? 1 : 0;
  int fl[7], vo[7];
#pragma unroll
  for (int m = 0; m < 7; ++m) {
    const int q = p.idx + ((m & 1) ? sx : 0) + ((m & 2) ? sy : 0) + ((m & 4) ? sz : 0);
    fl[m] = edge_flags[q];
    vo[m] = (int)vert_offset[q];      // (below 2^31: the entry point refuses more vertices)
  }
  // ---- the vertices this point owns ----
  const float pa[3] = {mesh_coord(box.lo[0], box.hi[0], p.i, nx), mesh_coord(box.lo[1], box.hi[1], p.j, ny),
                       mesh_coord(box.lo[2], box.hi[2], p.k, nz)};
  const float pb[3] = {mesh_coord(box.lo[0], box.hi[0], p.i + (p.ex ? 1 : 0), nx), mesh_coord(box.lo[1], box.hi[1], p.j + (p.ey ? 1 : 0), ny),
                       mesh_coord(box.lo[2], box.hi[2], p.k + (p.ez ? 1 : 0), nz)};
  const int f = p.live ? fl[0] : 0;
  const float va = p.v[0];
#pragma unroll
  for (int kind = 0; kind < 7; ++kind) {
    const int m = mesh_mask_of_kind(kind);
    const long id = (long)vo[0] + __popc(f & ((1 << kind) - 1));
    if (((f >> kind) & 1) && (unsigned long)id < (unsigned long)n_vertices) {
      const float vb = p.v[m];
      float t = (level - va) / (vb - va);
      t = (t != t) ? 0.5f : fminf(fmaxf(t, 0.f), 1.f);
      float* __restrict__ o = vertices + 3 * id;
      o[0] = pa[0] + t * (((m & 1) ? pb[0] : pa[0]) - pa[0]);
      o[1] = pa[1] + t * (((m & 2) ? pb[1] : pa[1]) - pa[1]);
      o[2] = pa[2] + t * (((m & 4) ? pb[2] : pa[2]) - pa[2]);
    }
  }
  // ---- the triangles of the cell whose minimum corner this point is, tetrahedra in the order of the permutations ----
  if (p.live && p.ex && p.ey && p.ez) {
    long at = tri_offset[p.idx];
    at += mesh_emit_tet<0, 1, 2>(cube, fl, vo, at, n_triangles, triangles);
    at += mesh_emit_tet<0, 2, 1>(cube, fl, vo, at, n_triangles, triangles);
    at += mesh_emit_tet<1, 0, 2>(cube, fl, vo, at, n_triangles, triangles);
    at += mesh_emit_tet<1, 2, 0>(cube, fl, vo, at, n_triangles, triangles);
    at += mesh_emit_tet<2, 0, 1>(cube, fl, vo, at, n_triangles, triangles);
    at += mesh_emit_tet<2, 1, 0>(cube, fl, vo, at, n_triangles, triangles);
  }
}

static int mesh_shape(const float* lattice, int nx, int ny, int nz, float level, long* n) {
  if (!lattice || nx < 2 || ny < 2 || nz < 2 || !__builtin_isfinite(level)) return JT_ERR_ARG;
  *n = (long)nx * (long)ny * (long)nz;
  return *n > (1l << 27) ? JT_ERR_UNSUPPORTED : JT_OK;
}

// ---- a mesh of an NDC scene carried to world space (include/jt_render.h: "NDC meshes in world space") ----------------------
// The ray generator's NDC (jt_camera.hip) is xn = sx x/z, yn = sy y/z, zn = 1 - 2n/z; its inverse with u = 1 - zn is z = 2n/u,
// x = xn z/sx, y = yn z/sy, defined for u > 0.  One lane per vertex; every operation is rounded on its own (__f*_rn, fmaf), so the
// bits do not depend on contraction: u one rounding (none for zn in [0.5, 2], Sterbenz), z two, x and y four.  A normal is a
// gradient direction and goes through J^T, scaled by the positive z: (sx nx, sy ny, u nz - xn nx - yn ny), then normalised.
constexpr uint8_t kUnwarpKept = 0, kUnwarpBeyond = 1, kUnwarpFar = 2;

__global__ __launch_bounds__(kMeshThreads) void k_mesh_unwarp_ndc(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                  long n, float sx, float sy, float two_near, float max_depth,
                                                                  float* __restrict__ world, float* __restrict__ world_normals,
                                                                  uint8_t* __restrict__ status) {
  const long i = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  if (i >= n) return;
  const float xn = vertices[3 * i], yn = vertices[3 * i + 1], zn = vertices[3 * i + 2];
  const float u = __fsub_rn(1.f, zn);
  const float z = __fdiv_rn(two_near, u);
  const float x = __fdiv_rn(__fmul_rn(xn, z), sx);
  const float y = __fdiv_rn(__fmul_rn(yn, z), sy);
  const bool finite_in = __builtin_isfinite(xn) && __builtin_isfinite(yn) && __builtin_isfinite(zn);
  const bool finite_out = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
  uint8_t st = kUnwarpKept;
  if (!finite_in || !(u > 0.f) || !finite_out) st = kUnwarpBeyond;
  else if (max_depth > 0.f && z > max_depth) st = kUnwarpFar;
  const bool kept = st == kUnwarpKept;
  world[3 * i] = kept ? x : 0.f;
  world[3 * i + 1] = kept ? y : 0.f;
  world[3 * i + 2] = kept ? z : 0.f;
  status[i] = st;
  if (normals) {
    const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    const float a = __fmul_rn(sx, nx), b = __fmul_rn(sy, ny);
    const float c = fmaf(u, nz, -fmaf(xn, nx, __fmul_rn(yn, ny)));
    const float len = __fsqrt_rn(fmaf(a, a, fmaf(b, b, __fmul_rn(c, c))));
    const bool ok = kept && len > 0.f && __builtin_isfinite(len);      // (false for a NaN; a zero normal stays zero)
    world_normals[3 * i] = ok ? __fdiv_rn(a, len) : 0.f;
    world_normals[3 * i + 1] = ok ? __fdiv_rn(b, len) : 0.f;
    world_normals[3 * i + 2] = ok ? __fdiv_rn(c, len) : 0.f;
  }
}

// The triangles whose three vertices were all kept, in count / scan / emit form like the extraction above.  k_mesh_filter_count:
// keep[t] = 1 iff the three ids are in range and their statuses 0; cause[t] = 0 kept, else the first that applies of 1 (an id out
// of range or a vertex beyond) and 2 (a vertex too far); used[v] = 1 for every vertex of a kept triangle (zeroed by the caller;
// lanes that store the same 1 do not race for a value).  The caller scans keep and used; k_mesh_filter_emit writes kept triangle
// t as row tri_offset[t] with ids vert_offset[id], and used vertex v (position, normal, colour) as row vert_offset[v]: the order
// of both is the original one and two runs give the same bits.
__global__ __launch_bounds__(kMeshThreads) void k_mesh_filter_count(const int32_t* __restrict__ triangles, long nt,
                                                                    const uint8_t* __restrict__ status, long nv,
                                                                    uint8_t* __restrict__ keep, uint8_t* __restrict__ cause,
                                                                    uint8_t* __restrict__ used) {
  const long t = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  if (t >= nt) return;
  const long id[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
  bool beyond = false, far = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const bool in_range = id[c] >= 0 && id[c] < nv;
    const uint8_t s = in_range ? status[id[c]] : kUnwarpBeyond;
    beyond |= s == kUnwarpBeyond || s > kUnwarpFar;
    far |= s == kUnwarpFar;
  }
  const bool k = !beyond && !far;
  keep[t] = k ? 1 : 0;
  cause[t] = k ? kUnwarpKept : beyond ? kUnwarpBeyond : kUnwarpFar;
  if (k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) used[id[c]] = 1;
  }
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_filter_emit(
    const float* __restrict__ vertices, const float* __restrict__ normals, const float* __restrict__ colors, long nv,
    const int32_t* __restrict__ triangles, long nt, const uint8_t* __restrict__ keep, const uint8_t* __restrict__ used,
    const int64_t* __restrict__ vert_offset, const int64_t* __restrict__ tri_offset, long nv_out, long nt_out,
    float* __restrict__ vertices_out, float* __restrict__ normals_out, float* __restrict__ colors_out,
    int32_t* __restrict__ triangles_out) {
  const long i = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  if (i < nt && keep[i]) {
    const long at = tri_offset[i];
    if ((unsigned long)at < (unsigned long)nt_out) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long id = triangles[3 * i + c];       // (in range: keep[i] says so)
        triangles_out[3 * at + c] = (id >= 0 && id < nv) ? (int32_t)vert_offset[id] : 0;
      }
    }
  }
  if (i < nv && used[i]) {
    const long at = vert_offset[i];
    if ((unsigned long)at < (unsigned long)nv_out) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        vertices_out[3 * at + c] = vertices[3 * i + c];
        if (normals) normals_out[3 * at + c] = normals[3 * i + c];
        if (colors) colors_out[3 * at + c] = colors[3 * i + c];
      }
    }
  }
}

}  // namespace jt

using namespace jt;

extern "C" int jt_mesh_count(const float* lattice, int nx, int ny, int nz, float level, uint8_t* edge_flags, uint8_t* tri_count,
                             void* stream) {
  long n = 0;
  if (!edge_flags || !tri_count) return JT_ERR_ARG;
  if (const int rc = mesh_shape(lattice, nx, ny, nz, level, &n)) return rc;
  hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)((n + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0,
                     (hipStream_t)stream, lattice, nx, ny, nz, level, edge_flags, tri_count);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_mesh_emit(const float* lattice, int nx, int ny, int nz, float level, const float* lo3, const float* hi3,
                            const uint8_t* edge_flags, const int64_t* vert_offset, const int64_t* tri_offset, long n_vertices,
                            long n_triangles, float* vertices, int32_t* triangles, void* stream) {
  long n = 0;
  if (!lo3 || !hi3 || !edge_flags || !vert_offset || !tri_offset || n_vertices < 0 || n_triangles < 0) return JT_ERR_ARG;
  if (const int rc = mesh_shape(lattice, nx, ny, nz, level, &n)) return rc;
  if (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  if (n_vertices == 0) return JT_OK;
  if (!vertices || (n_triangles > 0 && !triangles)) return JT_ERR_ARG;
  MeshBox box;
  for (int a = 0; a < 3; ++a) {
    box.lo[a] = lo3[a];
    box.hi[a] = hi3[a];
  }
  hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)((n + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0,
                     (hipStream_t)stream, lattice, nx, ny, nz, level, box, edge_flags, vert_offset, tri_offset, n_vertices,
                     n_triangles, vertices, triangles);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_mesh_unwarp_ndc(const float* vertices, const float* normals, long n, float sx, float sy, float ndc_near,
                                  float max_depth, float* world, float* world_normals, uint8_t* status, void* stream) {
  if (!vertices || !world || !status || (normals && !world_normals) || n < 1) return JT_ERR_ARG;
  if (!(sx > 0.f) || !(sy > 0.f) || !(ndc_near > 0.f) || !__builtin_isfinite(sx) || !__builtin_isfinite(sy) ||
      !__builtin_isfinite(ndc_near) || max_depth != max_depth)
    return JT_ERR_ARG;
  if (n >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_mesh_unwarp_ndc, dim3((unsigned)((n + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0,
                     (hipStream_t)stream, vertices, normals, n, sx, sy, 2.f * ndc_near, max_depth, world, world_normals, status);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

static int mesh_filter_shape(long n_vertices, long n_triangles) {
  if (n_vertices < 1 || n_triangles < 1) return JT_ERR_ARG;
  return (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) ? JT_ERR_UNSUPPORTED : JT_OK;
}

extern "C" int jt_mesh_filter_count(const int32_t* triangles, long n_triangles, const uint8_t* status, long n_vertices,
                                    uint8_t* keep, uint8_t* cause, uint8_t* used, void* stream) {
  if (!triangles || !status || !keep || !cause || !used) return JT_ERR_ARG;
  if (const int rc = mesh_filter_shape(n_vertices, n_triangles)) return rc;
  hipLaunchKernelGGL(k_mesh_filter_count, dim3((unsigned)((n_triangles + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0,
                     (hipStream_t)stream, triangles, n_triangles, status, n_vertices, keep, cause, used);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_mesh_filter_emit(const float* vertices, const float* normals, const float* colors, long n_vertices,
                                   const int32_t* triangles, long n_triangles, const uint8_t* keep, const uint8_t* used,
                                   const int64_t* vert_offset, const int64_t* tri_offset, long n_vertices_out,
                                   long n_triangles_out, float* vertices_out, float* normals_out, float* colors_out,
                                   int32_t* triangles_out, void* stream) {
  if (!vertices || !triangles || !keep || !used || !vert_offset || !tri_offset || n_vertices_out < 0 || n_triangles_out < 0)
    return JT_ERR_ARG;
  if (const int rc = mesh_filter_shape(n_vertices, n_triangles)) return rc;
  if (n_vertices_out > n_vertices || n_triangles_out > n_triangles) return JT_ERR_ARG;
  if (n_vertices_out == 0) return JT_OK;
  if (!vertices_out || (n_triangles_out > 0 && !triangles_out) || (normals && !normals_out) || (colors && !colors_out))
    return JT_ERR_ARG;
  const long lanes = n_vertices > n_triangles ? n_vertices : n_triangles;
  hipLaunchKernelGGL(k_mesh_filter_emit, dim3((unsigned)((lanes + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0,
                     (hipStream_t)stream, vertices, normals, colors, n_vertices, triangles, n_triangles, keep, used, vert_offset,
                     tri_offset, n_vertices_out, n_triangles_out, vertices_out, normals_out, colors_out, triangles_out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
