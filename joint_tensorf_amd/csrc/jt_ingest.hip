// Picture preprocessing of the dataset loaders (data/base.py:92-107, data/blender.py:71-76) on the device: decoded uint8
// pictures [B][h][w][c] -> fp32 planar [3][H][W], EQUAL BIT FOR BIT to `PIL.Image.resize((W, H), LANCZOS)` + `to_tensor` + the
// Blender composite over opt.data.bgcolor done with Pillow and torch on the CPU.  That is possible because Pillow's 8-bit
// resampling is integer arithmetic: per axis a table of int32 weights (2^22 fixed point, built on the host in double precision:
// joint_tensorf_amd/datasets.py: resample_table), a 32-bit sum, a rounding shift and a clamp to a byte; the horizontal pass
// first, rounded to bytes, then the vertical pass on those bytes; RGBA resampled premultiplied and divided out afterwards.
//
// Two launches with the byte intermediate [B][h][W][c] in a caller-provided workspace, at every ratio: the tap count is a
// run-time quantity (12 per axis at the Blender ratio of 2, 38 at the LLFF ratio of 6.3, 60 at a ratio of 10), a source
// window staged in LDS would have to be sized for the largest ratio or fall back to this form above some ratio, and neither
// pass is near a limit of the chip (the upload of the decoded bytes is what an ingest waits for).  A pass whose sizes agree
// is skipped: without a horizontal pass the vertical kernel reads the source directly, without a vertical pass it runs one
// tap of weight 2^22, which returns its byte exactly.  No LDS, no atomics, ordinary vector stores only.
#include "jt_common.h"

namespace jt {

constexpr int kIngestBX = 64, kIngestBY = 4;   // one workgroup: 64 output columns x 4 rows
constexpr int kIngestBits = 22;                // Pillow's PRECISION_BITS = 32 - 8 - 2

// Pillow's MULDIV255: the rounded a * b / 255 of two bytes
__device__ inline int muldiv255(int a, int b) {
  const int t = a * b + 128;
  return ((t >> 8) + t) >> 8;
}

// clamp((acc) >> 22, 0, 255).  Written as "negative -> 0, then an UNSIGNED shift, then min 255" on purpose: for the textbook
// form (arithmetic shift, then clamp to [0, 255]) hipcc selects gfx950's v_ashr_pk_u8_i32 when two such bytes are packed into a
// word, and that instruction writes only the low 16 bits of its destination: the upper half kept what the register held before
// (here the output pixel index), so blue and alpha of the byte intermediate came out OR-ed with (pixel index >> 16) -- wrong
// from the 65 536th pixel of a 4-channel batch on (tests/test_gpu_ingest.py: 800 x 800 x 4 -> 400 x 400).  This form is the
// same function of acc and does not match that pattern; the build's ISA holds no v_ashr_pk_u8_i32.
__device__ inline int clip8(int acc) {
  const uint32_t v = (uint32_t)(acc < 0 ? 0 : acc) >> kIngestBits;
  return (int)(v > 255u ? 255u : v);
}

template <int C>
__device__ inline void load_pixel(const uint8_t* __restrict__ p, bool premul, int (&v)[C]) {
  if constexpr (C == 4) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p);   // (pixels of a 4-channel picture are 4-byte aligned)
    v[0] = q & 255, v[1] = (q >> 8) & 255, v[2] = (q >> 16) & 255, v[3] = q >> 24;
    if (premul) {
      v[0] = muldiv255(v[0], v[3]);
      v[1] = muldiv255(v[1], v[3]);
      v[2] = muldiv255(v[2], v[3]);
    }
  } else {
    v[0] = p[0], v[1] = p[1], v[2] = p[2];
  }
}

// table of one axis, n_out columns: row 0 = first source index, row 1 = number of taps, row 2 + i = weight of tap i.  Tap-major,
// so that the lanes of a wave (consecutive output columns) read consecutive words.  The window is clamped to the source here as
// well: a wrong table gives wrong pictures, never an access outside the picture.
__device__ inline void window(const int32_t* __restrict__ tab, int n_out, int taps, int o, int n_in, int* first, int* count) {
  int f = tab[o], n = tab[n_out + o];
  f = f < 0 ? 0 : f > n_in - 1 ? n_in - 1 : f;
  n = n < 0 ? 0 : n > taps ? taps : n;
  *first = f;
  *count = n > n_in - f ? n_in - f : n;
}

// horizontal pass: src [B][h][w][C] -> tmp [B][h][W][C] bytes.  grid (ceil(W / 64), ceil(h / 4), B)
template <int C>
__global__ __launch_bounds__(kIngestBX* kIngestBY) void k_ingest_rows(const uint8_t* __restrict__ src, int h, int w,
                                                                       const int32_t* __restrict__ tab, int taps, int W,
                                                                       uint8_t* __restrict__ tmp) {
  const int X = blockIdx.x * kIngestBX + threadIdx.x, y = blockIdx.y * kIngestBY + threadIdx.y;
  if (X >= W || y >= h) return;
  int x0, n;
  window(tab, W, taps, X, w, &x0, &n);
  const uint8_t* __restrict__ row = src + ((size_t)blockIdx.z * h + y) * (size_t)w * C;
  int acc[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) acc[ch] = 1 << (kIngestBits - 1);
  for (int i = 0; i < n; ++i) {
    const int k = tab[(size_t)(2 + i) * W + X];
    int v[C];
    load_pixel<C>(row + (size_t)(x0 + i) * C, C == 4, v);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] += k * v[ch];
  }
  uint8_t* __restrict__ o = tmp + (((size_t)blockIdx.z * h + y) * W + X) * C;
  if constexpr (C == 4) {
    *reinterpret_cast<uint32_t*>(o) = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) | ((uint32_t)clip8(acc[2]) << 16) |
                                      ((uint32_t)clip8(acc[3]) << 24);
  } else {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[ch] = (uint8_t)clip8(acc[ch]);
  }
}

// vertical pass and the tail: in [B][rows][W][C] bytes (the intermediate, or the source when there was no horizontal pass) ->
// out [B][3][H][W] fp32.  tab == nullptr: no vertical pass (rows == H), one tap of weight 2^22.  grid (ceil(W / 64), ceil(H / 4), B)
template <int C>
__global__ __launch_bounds__(kIngestBX* kIngestBY) void k_ingest_cols(const uint8_t* __restrict__ in, int rows, int W,
                                                                       const int32_t* __restrict__ tab, int taps, int H,
                                                                       int premul_on_load, int unpremul, int composite, float bg,
                                                                       float* __restrict__ out) {
  const int X = blockIdx.x * kIngestBX + threadIdx.x, Y = blockIdx.y * kIngestBY + threadIdx.y;
  if (X >= W || Y >= H) return;
  int y0 = Y, n = 1;
  if (tab) window(tab, H, taps, Y, rows, &y0, &n);
  const uint8_t* __restrict__ col = in + ((size_t)blockIdx.z * rows * W + X) * C;
  int acc[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) acc[ch] = 1 << (kIngestBits - 1);
  for (int i = 0; i < n; ++i) {
    const int k = tab ? tab[(size_t)(2 + i) * H + Y] : 1 << kIngestBits;
    int v[C];
    load_pixel<C>(col + (size_t)(y0 + i) * W * C, premul_on_load != 0, v);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] += k * v[ch];
  }
  int b[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) b[ch] = clip8(acc[ch]);
  if constexpr (C == 4) {
    // RGBa -> RGBA: the colour stays where alpha is 0 or 255, else 255 * c / a in integer division, clipped
    if (unpremul && b[3] != 0 && b[3] != 255) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int q = 255 * b[ch] / b[3];
        b[ch] = q > 255 ? 255 : q;
      }
    }
  }
  // to_tensor: byte / 255 in fp32 by IEEE division; then rgb * mask + bg * (1 - mask), four roundings as the four torch ops
  // round.  Contraction is switched off for this block: hipcc's default (-ffp-contract=fast) fuses v * m + bm into one
  // v_fma_f32 -- through __fmul_rn / __fadd_rn as well: they are inline operators of the HIP headers and carry the default --
  // and a fused multiply-add rounds once where torch rounds twice (last-bit differences on partially transparent pixels).
  {
#pragma clang fp contract(off)
    float m = 0.f, bm = 0.f;
    if constexpr (C == 4) {
      m = __fdiv_rn((float)b[3], 255.0f);
      bm = bg * (1.0f - m);
    }
    const size_t plane = (size_t)H * W;
    float* __restrict__ o = out + (size_t)blockIdx.z * 3 * plane + (size_t)Y * W + X;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v = __fdiv_rn((float)b[ch], 255.0f);
      if (C == 4 && composite) v = v * m + bm;
      o[ch * plane] = v;
    }
  }
}

static bool ingest_shape(int n, int h, int w, int c, int H, int W) {
  return n >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (c == 3 || c == 4);
}

}  // namespace jt

using namespace jt;

extern "C" size_t jt_image_ingest_workspace_bytes(int n_images, int in_h, int in_w, int channels, int out_h, int out_w) {
  if (!ingest_shape(n_images, in_h, in_w, channels, out_h, out_w) || in_w == out_w) return 0;
  return (size_t)n_images * (size_t)in_h * (size_t)out_w * (size_t)channels;
}

extern "C" int jt_image_ingest(const uint8_t* images, int n_images, int in_h, int in_w, int channels, const int32_t* table_x,
                               int taps_x, const int32_t* table_y, int taps_y, int out_h, int out_w, int composite, float bgcolor,
                               float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!images || !out || !ingest_shape(n_images, in_h, in_w, channels, out_h, out_w)) return JT_ERR_ARG;
  const bool pass_x = in_w != out_w, pass_y = in_h != out_h;
  if ((pass_x && (!table_x || taps_x < 1)) || (pass_y && (!table_y || taps_y < 1))) return JT_ERR_ARG;
  const size_t need = jt_image_ingest_workspace_bytes(n_images, in_h, in_w, channels, out_h, out_w);
  if (pass_x && (!workspace || workspace_bytes < need)) return JT_ERR_ARG;
  if (channels == 4 && ((((uintptr_t)images) | (uintptr_t)workspace) & 3)) return JT_ERR_ARG;   // pixels are read as one word
  const long rows_max = in_h > out_h ? in_h : out_h;
  if (n_images > 65535 || (rows_max + kIngestBY - 1) / kIngestBY > 65535) return JT_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(kIngestBX, kIngestBY);
  const unsigned gx = (unsigned)((out_w + kIngestBX - 1) / kIngestBX);
  const bool resampled = pass_x || pass_y;   // (equal sizes: the picture is returned untouched, no premultiply round trip)
  uint8_t* tmp = static_cast<uint8_t*>(workspace);
  if (pass_x) {
    const dim3 grid(gx, (unsigned)((in_h + kIngestBY - 1) / kIngestBY), (unsigned)n_images);
    if (channels == 4)
      hipLaunchKernelGGL(k_ingest_rows<4>, grid, block, 0, st, images, in_h, in_w, table_x, taps_x, out_w, tmp);
    else
      hipLaunchKernelGGL(k_ingest_rows<3>, grid, block, 0, st, images, in_h, in_w, table_x, taps_x, out_w, tmp);
    JT_LAUNCH_CHECK();
  }
  const uint8_t* in = pass_x ? tmp : images;
  const int32_t* ty = pass_y ? table_y : nullptr;
  const int premul_on_load = channels == 4 && resampled && !pass_x, unpremul = channels == 4 && resampled;
  const dim3 grid(gx, (unsigned)((out_h + kIngestBY - 1) / kIngestBY), (unsigned)n_images);
  if (channels == 4)
    hipLaunchKernelGGL(k_ingest_cols<4>, grid, block, 0, st, in, in_h, out_w, ty, taps_y, out_h, premul_on_load, unpremul,
                       composite, bgcolor, out);
  else
    hipLaunchKernelGGL(k_ingest_cols<3>, grid, block, 0, st, in, in_h, out_w, ty, taps_y, out_h, 0, 0, 0, 0.f, out);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
