// A per-triangle texture atlas for an exported mesh (include/jt_render.h: "Texture atlas").  Square blocks of S x S texels, two
// right-isosceles charts of legs L = S - 3 per block, block b at (b % cols, b / cols); texel (i, j) of block b is entry
// e = b S S + j S + i.  k_texture_texels turns a range of entries into the points and view directions the appearance branch is
// asked at, k_texture_pack quantises the answers into the uint8 atlas.  One lane per entry, 256 threads, 64-bit indexing, no
// LDS, no atomics: distinct entries write distinct bytes and two runs give the same bits.
//
// Numerics: positions and interpolated normals are fixed sequences of correctly rounded fp32 operations (contraction off,
// __fdiv_rn), the direction a fixed sequence of correctly rounded fp64 operations rounded once to fp32, so a NumPy statement
// of the header reproduces them bit for bit; the quantisation is mesh_io.quantise_colors' floor(255 c + 0.5) in fp64.
#include "jt_common.h"

namespace jt {

constexpr int kTextureThreads = 256;
constexpr int kTextureMinBlock = JT_TEXTURE_MIN_BLOCK, kTextureMaxBlock = JT_TEXTURE_MAX_BLOCK;
constexpr int kTextureMaxSide = JT_TEXTURE_MAX_SIDE;

// where entry e lies: its block, its texel (i, j) in the block, the triangle that owns it and its chart coordinates
struct TextureEntry {
  long block, tri;
  int i, j, ci, cj;
};

__device__ inline TextureEntry texture_entry(long e, int S) {
  TextureEntry t;
  const int area = S * S;
  t.block = e / area;
  const int r = (int)(e - t.block * area);
  t.j = r / S;
  t.i = r - t.j * S;
  const bool lower = t.i + t.j <= S - 1;
  t.tri = 2 * t.block + (lower ? 0 : 1);
  t.ci = lower ? t.i : S - 1 - t.i;
  t.cj = lower ? t.j : S - 1 - t.j;
  return t;
}

// (x0 + a (x1 - x0)) + b (x2 - x0), every operation rounded on its own
__device__ inline float texture_lerp2(float x0, float x1, float x2, float a, float b) {
#pragma clang fp contract(off)
  const float e1 = x1 - x0;
  const float e2 = x2 - x0;
  const float p = x0 + a * e1;
  return p + b * e2;
}

__global__ __launch_bounds__(kTextureThreads) void k_texture_texels(const float* __restrict__ vertices,
                                                                     const float* __restrict__ normals, long nv,
                                                                     const int32_t* __restrict__ triangles, long nt, int S,
                                                                     long start, long count, float* __restrict__ xyz,
                                                                     float* __restrict__ dirs, uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
  const long k = (long)blockIdx.x * kTextureThreads + threadIdx.x;
  if (k >= count) return;
  const TextureEntry t = texture_entry(start + k, S);
  float p[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, -1.f};
  bool ok = t.tri < nt;
  long v0 = 0, v1 = 0, v2 = 0;
  if (ok) {
    v0 = triangles[3 * t.tri], v1 = triangles[3 * t.tri + 1], v2 = triangles[3 * t.tri + 2];
    ok = v0 >= 0 && v0 < nv && v1 >= 0 && v1 < nv && v2 >= 0 && v2 < nv;
  }
  if (ok) {
    const float L = (float)(S - 3);
    const float a = __fdiv_rn((float)t.ci, L), b = __fdiv_rn((float)t.cj, L);
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[c] = texture_lerp2(vertices[3 * v0 + c], vertices[3 * v1 + c], vertices[3 * v2 + c], a, b);
      m[c] = texture_lerp2(normals[3 * v0 + c], normals[3 * v1 + c], normals[3 * v2 + c], a, b);
    }
    const double m0 = (double)m[0], m1 = (double)m[1], m2 = (double)m[2];
    const double len = __dsqrt_rn((m0 * m0 + m1 * m1) + m2 * m2);
    if (len > 0.0 && __builtin_isfinite(len)) {                  // (false for a NaN)
      d[0] = (float)__ddiv_rn(-m0, len);
      d[1] = (float)__ddiv_rn(-m1, len);
      d[2] = (float)__ddiv_rn(-m2, len);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xyz[3 * k + c] = p[c];
    dirs[3 * k + c] = d[c];
  }
  valid[k] = ok ? 1 : 0;
}

// floor(255 c + 0.5) clamped to 0 .. 255 in fp64 (255 c is exact there); 0 for a NaN
__device__ inline uint8_t texture_quantise(float c) {
  const double v = floor(255.0 * (double)c + 0.5);
  return v >= 255.0 ? (uint8_t)255 : v >= 0.0 ? (uint8_t)(int)v : (uint8_t)0;      // (a NaN fails both tests)
}

__global__ __launch_bounds__(kTextureThreads) void k_texture_pack(const float* __restrict__ rgb, const uint8_t* __restrict__ valid,
                                                                   int S, int cols, long start, long count, int Ha, int Wa,
                                                                   uint8_t* __restrict__ atlas) {
  const long k = (long)blockIdx.x * kTextureThreads + threadIdx.x;
  if (k >= count || !valid[k]) return;
  const TextureEntry t = texture_entry(start + k, S);
  const long px = (t.block % cols) * S + t.i, py = (t.block / cols) * S + t.j;
  if (px >= Wa || py >= Ha) return;                              // (the entry point has refused such a range already)
  uint8_t* __restrict__ o = atlas + 3 * (py * Wa + px);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = texture_quantise(rgb[3 * k + c]);
}

// S in range and the atlas of `blocks` blocks in `cols` columns within what a viewer (and the rasteriser) addresses
static int texture_shape(int S, long cols, long blocks) {
  if (S < kTextureMinBlock || S > kTextureMaxBlock) return JT_ERR_UNSUPPORTED;
  const long rows = (blocks + cols - 1) / cols;
  if (cols * S > kTextureMaxSide || rows * S > kTextureMaxSide || blocks * S * S >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  return JT_OK;
}

}  // namespace jt

using namespace jt;

extern "C" int jt_texture_texels(const float* vertices, const float* normals, long n_vertices, const int32_t* triangles,
                                 long n_triangles, int S, int cols, long start, long count, float* xyz, float* dirs,
                                 uint8_t* valid, void* stream) {
  if (!vertices || !normals || !triangles || !xyz || !dirs || !valid) return JT_ERR_ARG;
  if (n_vertices < 1 || n_triangles < 1 || cols < 1 || start < 0 || count < 1) return JT_ERR_ARG;
  if (n_vertices >= (1l << 31) || 3 * n_triangles >= (1l << 31)) return JT_ERR_UNSUPPORTED;
  const long blocks = (n_triangles + 1) / 2;
  if (const int rc = texture_shape(S, cols, blocks)) return rc;
  if (start + count > blocks * S * S) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_texture_texels, dim3((unsigned)((count + kTextureThreads - 1) / kTextureThreads)), dim3(kTextureThreads), 0,
                     (hipStream_t)stream, vertices, normals, n_vertices, triangles, n_triangles, S, start, count, xyz, dirs, valid);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_texture_pack(const float* rgb, const uint8_t* valid, int S, int cols, long start, long count, uint8_t* atlas,
                               int H_atlas, int W_atlas, void* stream) {
  if (!rgb || !valid || !atlas || cols < 1 || start < 0 || count < 1 || H_atlas < 1 || W_atlas < 1) return JT_ERR_ARG;
  if (S < kTextureMinBlock || S > kTextureMaxBlock) return JT_ERR_UNSUPPORTED;
  if (W_atlas != (long)cols * S || H_atlas % S != 0) return JT_ERR_ARG;
  const long blocks = (long)(H_atlas / S) * cols;
  if (const int rc = texture_shape(S, cols, blocks)) return rc;
  if (start + count > blocks * S * S) return JT_ERR_ARG;
  hipLaunchKernelGGL(k_texture_pack, dim3((unsigned)((count + kTextureThreads - 1) / kTextureThreads)), dim3(kTextureThreads), 0,
                     (hipStream_t)stream, rgb, valid, S, cols, start, count, H_atlas, W_atlas, atlas);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
