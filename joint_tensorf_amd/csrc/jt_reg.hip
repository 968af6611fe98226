// Regularisers over a channel-last VM factor in one pass: sum|x| (density_L1, tensoRF.py:212-216) and the two
// total-variation sums  sum (x[y+1,x]-x[y,x])^2, sum (x[y,x+1]-x[y,x])^2  (TVLoss, tensorBase.py:16-41), and
// their gradient accumulated into the factor's gradient buffer.  The stock-op version makes ~10 passes over
// the 123 MB factor set per iteration; this reads it once (forward) and touches only the tensors that carry a
// non-zero weight in the backward.
#include "jt_common.h"

namespace jt {

__device__ inline float4 ld4z(const float* p, bool ok) { return ok ? ld4(p) : make_float4(0.f, 0.f, 0.f, 0.f); }
// a - b where the neighbour exists, 0 where it does not.  A select, not a product with a 0/1 mask: what stands in for the
// missing neighbour never reaches a sum or a gradient, whatever v is.
__device__ inline float4 diff4(bool ok, const float4& a, const float4& b) {
  return ok ? make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w) : make_float4(0.f, 0.f, 0.f, 0.f);
}

constexpr int kRegSeg = 16;  // rows a thread of the TV kernels walks (the vertical neighbours stay in its registers)
// what a pass over a tensor leaves behind: the three partial sums, the gradient, or both (one read of every texel)
constexpr int kRegSums = 1, kRegGrad = 2;

// One quad of four channels, v, between its neighbours (hu, hd, hl, hr: there is one above, below, to the left, to the right).
//   sums:      s0 += sum |v| ; s1 += sum (down - v)^2 ; s2 += sum (right - v)^2
//   gradient:  g (+)= c0 sign(v) + 2 (c1 A + c2 B),  A = [hu] (v - up) - [hd] (down - v),  B likewise along the row
// Without TV only s0 and c0 sign(v) are formed; up and left are read by the gradient alone.
template <bool TV, int OUT>
__device__ inline void reg_texel(const float4& v, const float4& up, const float4& dn, const float4& lf, const float4& rt,
                                 bool hu, bool hd, bool hl, bool hr, float c0, float c1, float c2, float& s0, float& s1,
                                 float& s2, float* __restrict__ g, int accumulate) {
  const float4 d = diff4(TV && hd, dn, v), e = diff4(TV && hr, rt, v);
  if (OUT & kRegSums) {
    s0 += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
    if (TV) {
      s1 += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
      s2 += e.x * e.x + e.y * e.y + e.z * e.z + e.w * e.w;
    }
  }
  if (OUT & kRegGrad) {
    float4 r;
    r.x = c0 * ((v.x > 0.f) - (v.x < 0.f));
    r.y = c0 * ((v.y > 0.f) - (v.y < 0.f));
    r.z = c0 * ((v.z > 0.f) - (v.z < 0.f));
    r.w = c0 * ((v.w > 0.f) - (v.w < 0.f));
    if (TV) {
      const float4 a = diff4(hu, v, up), b = diff4(hl, v, lf);
      r.x += 2.f * (c1 * (a.x - d.x) + c2 * (b.x - e.x));
      r.y += 2.f * (c1 * (a.y - d.y) + c2 * (b.y - e.y));
      r.z += 2.f * (c1 * (a.z - d.z) + c2 * (b.z - e.z));
      r.w += 2.f * (c1 * (a.w - d.w) + c2 * (b.w - e.w));
    }
    if (accumulate) {
      const float4 gg = ld4(g);
      r.x += gg.x;
      r.y += gg.y;
      r.z += gg.z;
      r.w += gg.w;
    }
    *reinterpret_cast<float4*>(g) = r;
  }
}

// workgroup `bid` of `nblocks` over the quads of x [H][W][C]: every quad through reg_texel, the sums into this thread's s0-s2
template <bool TV, int OUT>
__device__ inline void reg_body(const float* __restrict__ x, float* __restrict__ g, int H, int W, int C, float c0, float c1,
                                float c2, int accumulate, int bid, int nblocks, float& s0, float& s1, float& s2) {
  constexpr bool GRAD = (OUT & kRegGrad) != 0;
  // (four loads in flight in the sums' one-quad loop; the storing loop unrolled: not measured)
  constexpr int kLoopUnroll = GRAD ? 1 : 4;
  const unsigned C4 = C / 4;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (TV && H >= 2 * kRegSeg) {
    // TV items: a thread owns (quad, column) and walks kRegSeg rows downwards with (up, v, down) sliding through its
    // registers -- the row below is next step's own value, so the sums fetch a texel twice (itself / as somebody's right
    // neighbour) instead of three times, and the gradient three times (the new row, left, right) instead of five
    const unsigned nseg = ((unsigned)H + kRegSeg - 1) / kRegSeg, per_row = (unsigned)W * C4, items = nseg * per_row;
    const size_t rstride = (size_t)W * C;
    for (unsigned it = bid * blockDim.x + threadIdx.x; it < items; it += (unsigned)nblocks * blockDim.x) {
      const unsigned seg = it / per_row, q = it - seg * per_row;        // q = xx * C4 + c4: float offset 4 q inside a row
      const int xx = (int)(q / C4);
      const int y0 = (int)(seg * kRegSeg), y1 = min(y0 + kRegSeg, H);
      size_t off = (size_t)y0 * rstride + (size_t)q * 4;
      const bool hl = xx > 0, hr = xx + 1 < W;
      float4 up = GRAD ? ld4z(x + off - rstride, y0 > 0) : zero, v = ld4(x + off);
#pragma unroll 2
      for (int yy = y0; yy < y1; ++yy) {
        const bool hd = yy + 1 < H;
        const float4 dn = ld4z(x + off + rstride, hd);
        const float4 lf = GRAD ? ld4z(x + off - C, hl) : zero, rt = ld4z(x + off + C, hr);
        reg_texel<true, OUT>(v, up, dn, lf, rt, yy > 0, hd, hl, hr, c0, c1, c2, s0, s1, s2, g + off, accumulate);
        up = v;
        v = dn;
        off += rstride;
      }
    }
    return;
  }
  // (32-bit index arithmetic: with `long` the three divisions per item were most of the kernel's instructions)
  const unsigned total = (unsigned)H * W * C4;  // (< 2^31: checked by the callers)
#pragma unroll kLoopUnroll
  for (unsigned idx = bid * blockDim.x + threadIdx.x; idx < total; idx += (unsigned)nblocks * blockDim.x) {
    const size_t off = (size_t)idx * 4;   // [tex][C] with C = 4 C4: quad idx starts at float 4 idx
    const float4 v = ld4(x + off);
    if (TV) {
      const unsigned tex = idx / C4;
      const int yy = (int)(tex / (unsigned)W), xx = (int)(tex - (unsigned)yy * W);
      const bool hu = yy > 0, hd = yy + 1 < H, hl = xx > 0, hr = xx + 1 < W;
      const size_t rstride = (size_t)W * C;
      const float4 up = GRAD ? ld4z(x + off - rstride, hu) : zero, dn = ld4z(x + off + rstride, hd);
      const float4 lf = GRAD ? ld4z(x + off - C, hl) : zero, rt = ld4z(x + off + C, hr);
      reg_texel<true, OUT>(v, up, dn, lf, rt, hu, hd, hl, hr, c0, c1, c2, s0, s1, s2, g + off, accumulate);
    } else {
      reg_texel<false, OUT>(v, zero, zero, zero, zero, false, false, false, false, c0, c1, c2, s0, s1, s2, g + off, accumulate);
    }
  }
}

// One tensor's share of a launch.  tv is uniform over the workgroup (a template argument, an item's flag or "a TV coefficient
// is non-zero"), so the two loop pairs sit under a branch no wave diverges on.  With sums: out[0 .. 2] += this workgroup's.
template <int OUT>
__device__ inline void reg_run(bool tv, const float* __restrict__ x, float* __restrict__ g, int H, int W, int C, float c0,
                               float c1, float c2, int accumulate, float* __restrict__ out, int bid, int nblocks) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (tv)
    reg_body<true, OUT>(x, g, H, W, C, c0, c1, c2, accumulate, bid, nblocks, s0, s1, s2);
  else
    reg_body<false, OUT>(x, g, H, W, C, c0, c1, c2, accumulate, bid, nblocks, s0, s1, s2);
  if (OUT & kRegSums) {
    __shared__ float red[4][3];
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
      red[wv][0] = s0;
      red[wv][1] = s1;
      red[wv][2] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int k = threadIdx.x;
      atomicAdd(out + k, red[0][k] + red[1][k] + red[2][k] + red[3][k]);
    }
  }
}

// out[0] += sum |x| ; out[1] += sum (down - x)^2 ; out[2] += sum (right - x)^2
template <bool TV>
__global__ __launch_bounds__(256) void k_factor_reg_fwd(const float* __restrict__ x, int H, int W, int C,
                                                        float* __restrict__ out) {
  reg_run<kRegSums>(TV, x, nullptr, H, W, C, 0.f, 0.f, 0.f, 0, out, blockIdx.x, gridDim.x);
}

// g (+)= coef[0] * sign(x) + coef[1] * d/dx sum(down-x)^2 + coef[2] * d/dx sum(right-x)^2   (coef on the device)
__global__ __launch_bounds__(256) void k_factor_reg_bwd(const float* __restrict__ x, int H, int W, int C,
                                                        const float* __restrict__ coef, float* __restrict__ g,
                                                        int accumulate) {
  const float c0 = coef[0], c1 = coef[1], c2 = coef[2];
  reg_run<kRegGrad>(c1 != 0.f || c2 != 0.f, x, g, H, W, C, c0, c1, c2, accumulate, nullptr, blockIdx.x, gridDim.x);
}

// all tensors of a scene in ONE launch each way: block ranges per tensor, the same partition of every tensor as the
// per-tensor launches (nine launches of 4-10 us become one)
struct RegBatchItem {
  const float* x;
  float* g;
  int H, W, C, tv, slot, block0, nblocks;   // slot: 0-2 density planes, 3-5 density lines, 6-8 appearance planes
};
struct RegBatch {
  RegBatchItem t[9];
  int n;
};

// the tensor this workgroup works on
__device__ inline const RegBatchItem& reg_item(const RegBatch& B) {
  int it = 0;
#pragma unroll 1
  for (int i = 1; i < B.n; ++i)
    if ((int)blockIdx.x >= B.t[i].block0) it = i;
  return B.t[it];
}

// The coefficient triple of T's gradient under the upstream gradients dL/d{L1, TV_density, TV_color} = (g0, g1, g2): three
// divisions, which every block works out for itself instead of a launch of its own in front.
// (three scalars, not an array handed on by address: the array kept a 36-byte private segment alive in the kernel descriptor)
__device__ inline void reg_coef(const RegBatchItem& T, float g0, float g1, float g2, float& c0, float& c1, float& c2) {
  const int i = T.slot;
  c0 = c1 = c2 = 0.f;
  if (i < 6) c0 = g0 / ((float)T.H * T.W * T.C);
  if (i < 3 || i >= 6) {
    const float gt = i < 3 ? g1 : g2;
    if (T.H > 1) c1 = gt * 2e-2f / ((float)T.C * (T.H - 1) * T.W);
    if (T.W > 1) c2 = gt * 2e-2f / ((float)T.C * T.H * (T.W - 1));
  }
}

// the normalisation table of the combine step: (H, W, C) of the nine regularised tensors (0-2 density planes, 3-5 density
// lines, 6-8 appearance planes)
struct RegDims {
  int H[9], W[9], C[9];
};

// out3 = {L1, TV_density, TV_color} with the reference's normalisations (tensoRF.py:212-228, tensorBase.py:21-38)
__device__ inline void reg_combine(const float* sums, const RegDims& S, float* __restrict__ out3) {
  float l1 = 0.f, tvd = 0.f, tva = 0.f;
  // (unrolled: S is a kernel argument, and a rolled loop indexing it dynamically made the compiler copy nine words of it into
  //  scratch memory -- 36 bytes per lane in k_reg_batch_fused)
#pragma unroll
  for (int i = 0; i < 6; ++i) l1 += sums[i * 3] / ((float)S.H[i] * S.W[i] * S.C[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float ta = 0.f, tb = 0.f;
    if (S.H[i] > 1) ta += sums[i * 3 + 1] / ((float)S.C[i] * (S.H[i] - 1) * S.W[i]);
    if (S.W[i] > 1) ta += sums[i * 3 + 2] / ((float)S.C[i] * S.H[i] * (S.W[i] - 1));
    const int b = 6 + i;
    if (S.H[b] > 1) tb += sums[b * 3 + 1] / ((float)S.C[b] * (S.H[b] - 1) * S.W[b]);
    if (S.W[b] > 1) tb += sums[b * 3 + 2] / ((float)S.C[b] * S.H[b] * (S.W[b] - 1));
    tvd += 2.f * ta * 1e-2f;
    tva += 2.f * tb * 1e-2f;
  }
  out3[0] = l1;
  out3[1] = tvd;
  out3[2] = tva;
}

// ONE launch (round 4; before: a zero fill of the scratch, this kernel, a combine kernel).  Every workgroup adds its partial sums
// into one of kRegShards copies of the 36 sums and takes a ticket; the workgroup that draws the last ticket adds the copies up,
// combines the 27 sums into out3 and puts the scratch back to zero -- the scratch must be ZERO when the first call sees it and is
// left zero by every call.  Why copies: float atomics on ONE address are serialised at the memory side (~50 ns each), and 512
// workgroups per tensor adding into the same three words took 25 us whatever the tensor's size (30 MB of density factors:
// 37.6 us; one word per 32 workgroups: 17 us).  The tickets are two-level for the same reason: one counter per tensor, and the
// workgroup that completes a tensor draws from the master counter.
// scratch (floats): [shard][36] sums, then the master counter and nine per-tensor counters; the interface asks for 640.
constexpr int kRegShards = 16;
constexpr int kRegCounters = kRegShards * 36;
__device__ inline void reg_ticket(const RegBatchItem& T, int n_items, const RegDims& S, float* __restrict__ scratch,
                                  float* __restrict__ out3) {
  // (no __threadfence(): a release fence writes the XCD's L2 back, ~2-6 us per workgroup, 4 600 of them -- measured +115 us on
  //  the LLFF grid.  The sums and the tickets are float / integer atomics, which execute at the memory side and never sit in an
  //  L2: waiting for this workgroup's own atomics to be acknowledged is all the ordering a ticket needs.)
  __shared__ int s_last;
  __shared__ float s_sums[36];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* cnt = reinterpret_cast<unsigned*>(scratch + kRegCounters);
    bool last = false;
    if (atomicAdd(cnt + 1 + T.slot, 1u) == (unsigned)T.nblocks - 1u)   // this tensor is complete ...
      last = atomicAdd(cnt, 1u) == (unsigned)n_items - 1u;             // ... and it was the last one
    s_last = last;
  }
  __syncthreads();
  if (s_last) {   // (uniform over the workgroup) read AND reset in one returning atomic per word
    if (threadIdx.x < 36) {
      float a = 0.f;
      for (int sh = 0; sh < kRegShards; ++sh) a += atomicExch(scratch + sh * 36 + threadIdx.x, 0.f);
      s_sums[threadIdx.x] = a;
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + 10) atomicExch(reinterpret_cast<unsigned*>(scratch + kRegCounters) + (threadIdx.x - 64), 0u);
    __syncthreads();
    if (threadIdx.x == 0) reg_combine(s_sums, S, out3);
  }
}

__global__ __launch_bounds__(256) void k_reg_batch_fwd(RegBatch B, RegDims S, float* __restrict__ scratch,
                                                       float* __restrict__ out3) {
  const RegBatchItem& T = reg_item(B);
  const int bid = blockIdx.x - T.block0;
  reg_run<kRegSums>(T.tv, T.x, nullptr, T.H, T.W, T.C, 0.f, 0.f, 0.f, 0, scratch + (bid % kRegShards) * 36 + T.slot * 3, bid,
                    T.nblocks);
  reg_ticket(T, B.n, S, scratch, out3);
}

// ---- value AND gradient in one pass (round 5) ---------------------------------------------------------------------------------
// The gradient of a regulariser does not depend on its value, and the upstream gradients dL/d{L1, TV_density, TV_color} of a
// training step are the loss weights, which the caller knows BEFORE the forward (host floats, or device memory under hipGraph
// replay): one launch reads every texel once (plus its neighbours for TV), adds the partial sums AND writes the gradient --
// k_reg_batch_fwd + k_reg_batch_bwd streamed the same factors back to back (LLFF final grid: 285 MB twice, 107 + 151 us).
// The gradient is WRITTEN (the render backward's atomics land on top of it: ops.RenderRays, "reg_first").
struct RegWeights {
  float w[3];          // dL/d{L1, TV_density, TV_color} as host values ...
  const float* dev;    // ... or (non-NULL) three floats in device memory
};

__global__ __launch_bounds__(256) void k_reg_batch_fused(RegBatch B, RegDims S, RegWeights Wt, float* __restrict__ scratch,
                                                         float* __restrict__ out3) {
  const RegBatchItem& T = reg_item(B);
  const int bid = blockIdx.x - T.block0;
  const float g0 = Wt.dev ? Wt.dev[0] : Wt.w[0], g1 = Wt.dev ? Wt.dev[1] : Wt.w[1], g2 = Wt.dev ? Wt.dev[2] : Wt.w[2];
  float c0, c1, c2;
  reg_coef(T, g0, g1, g2, c0, c1, c2);
  if (!T.tv) c1 = c2 = 0.f;   // a TV term that is switched off: neither its value nor its gradient
  reg_run<kRegSums | kRegGrad>(T.tv, T.x, T.g, T.H, T.W, T.C, c0, c1, c2, 0, scratch + (bid % kRegShards) * 36 + T.slot * 3,
                               bid, T.nblocks);
  reg_ticket(T, B.n, S, scratch, out3);
}

// (the TV switch of a tensor is its coefficients: a plane whose TV weight is zero takes the one-load loop)
__global__ __launch_bounds__(256) void k_reg_batch_bwd(RegBatch B, const float* __restrict__ g3, int accumulate) {
  const RegBatchItem& T = reg_item(B);
  float c0, c1, c2;
  reg_coef(T, g3[0], g3[1], g3[2], c0, c1, c2);
  reg_run<kRegGrad>(c1 != 0.f || c2 != 0.f, T.x, T.g, T.H, T.W, T.C, c0, c1, c2, accumulate, nullptr, blockIdx.x - T.block0,
                    T.nblocks);
}

}  // namespace jt

using namespace jt;

// Workgroups of 256 threads a tensor gets at most, per entry point, {with TV, without}.  Measured for the
// batched forward, 400^3 L1-only / LLFF final grid with both TV terms: 128 workgroups per tensor 17 / 126 us, 512: 27 / 107,
// 1 024: 44 / 131 -- the three-load TV items want the parallelism, the one-load L1 items the shorter epilogue.
enum RegEntry { kRegFactorFwd, kRegFactorBwd, kRegBatchFwd, kRegBatchBwd, kRegFused };
static const long kRegCaps[][2] = {
    /* kRegFactorFwd */ {1024, 0},   // (always launched with TV)
    /* kRegFactorBwd */ {2048, 2048},
    /* kRegBatchFwd */ {512, 128},
    /* kRegBatchBwd */ {2048, 2048},
    /* kRegFused */ {1024, 256},
};

// the workgroups of an [H][W][C] tensor in `entry`'s launch, min(ceil(quads / 256), cap); 0: too many quads
static int reg_blocks(RegEntry entry, bool tv, int H, int W, int C) {
  const long quads = (long)H * W * (C / 4);
  if (quads >= (1l << 31)) return 0;  // the kernels index quads with 32 bits
  return (int)min((quads + 255) / 256, kRegCaps[entry][tv ? 0 : 1]);
}

extern "C" int jt_factor_reg_forward(const float* x, int H, int W, int C, float* out3, void* stream) {
  if (!x || !out3 || H < 1 || W < 1 || C < 4) return JT_ERR_ARG;
  if (C % 4) return JT_ERR_UNSUPPORTED;
  const int blocks = reg_blocks(kRegFactorFwd, true, H, W, C);
  if (!blocks) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_factor_reg_fwd<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, H, W, C, out3);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_factor_reg_backward(const float* x, int H, int W, int C, const float* coef3, float* g,
                                      int accumulate, void* stream) {
  if (!x || !coef3 || !g || H < 1 || W < 1 || C < 4) return JT_ERR_ARG;
  if (C % 4) return JT_ERR_UNSUPPORTED;
  const int blocks = reg_blocks(kRegFactorBwd, true, H, W, C);
  if (!blocks) return JT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_factor_reg_bwd, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, H, W, C, coef3, g, accumulate);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

// ---------------------------------------------------------------------------------------------
// All regularisers of one scene in one call: L1 over the six density factors, TV over the three density
// planes and over the three appearance planes.  One sums launch per tensor + one tiny combine kernel instead
// of ~150 elementwise / reduce launches of the stock-op formulation (which left the host launch-bound).
// ---------------------------------------------------------------------------------------------
namespace jt {

struct RegTensor {
  const float* x;
  float* g;
  int H, W, C;
};

struct RegSet {
  RegTensor t[12];  // 0-2 density planes, 3-5 density lines, 6-8 app planes, 9-11 app lines
};

}  // namespace jt

static int reg_set(const JtFactors* f, const JtFactors* g, const int32_t* hw, int Cd, int Ca, RegSet* S) {
  if (!f || !hw || Cd < 4 || Ca < 4 || (Cd % 4) || (Ca % 4)) return JT_ERR_ARG;
  for (int i = 0; i < 3; ++i) {
    const int H = hw[i * 3], W = hw[i * 3 + 1], L = hw[i * 3 + 2];
    if (H < 1 || W < 1 || L < 1) return JT_ERR_ARG;
    S->t[i] = {f->density_plane[i], g ? g->density_plane[i] : nullptr, H, W, Cd};
    S->t[3 + i] = {f->density_line[i], g ? g->density_line[i] : nullptr, L, 1, Cd};
    S->t[6 + i] = {f->app_plane[i], g ? g->app_plane[i] : nullptr, H, W, Ca};
    S->t[9 + i] = {f->app_line[i], g ? g->app_line[i] : nullptr, L, 1, Ca};
  }
  for (int i = 0; i < 12; ++i)
    if (!S->t[i].x) return JT_ERR_ARG;
  return JT_OK;
}

// The launch of a batched entry point over the tensors that take part: the six density factors always (L1), the appearance
// planes where TV on the colours is on (app lines, 9-11, enter no regulariser).  tv: a TV term whose weight is zero is not
// evaluated (it reads every texel three times) and out3 carries 0 for it; the backward reads that switch from the
// coefficients on the device instead.  D (may be NULL): the combine step's table.  Returns the workgroups in *nblk.
static int reg_batch(RegEntry entry, const RegSet& S, int with_tv_density, int with_tv_app, RegBatch* B, RegDims* D, int* nblk) {
  B->n = *nblk = 0;
  for (int i = 0; i < 9; ++i) {
    const bool tv = (i < 3 && with_tv_density) || (i >= 6 && with_tv_app);
    if (i >= 6 && !tv) continue;  // appearance planes only enter TV_color
    const RegTensor& t = S.t[i];
    if (entry != kRegBatchFwd && !t.g) return JT_ERR_ARG;
    int blocks = reg_blocks(entry, tv, t.H, t.W, t.C);
    if (!blocks) return JT_ERR_UNSUPPORTED;
    if (entry == kRegBatchFwd && jt_deterministic()) blocks = 1;  // one workgroup per tensor: a fixed summation order
    B->t[B->n++] = {t.x, t.g, t.H, t.W, t.C, tv ? 1 : 0, i, *nblk, blocks};
    *nblk += blocks;
  }
  if (D)
    for (int i = 0; i < 9; ++i) D->H[i] = S.t[i].H, D->W[i] = S.t[i].W, D->C[i] = S.t[i].C;
  return JT_OK;
}

extern "C" int jt_reg_losses_forward(const JtFactors* factors, const int32_t* plane_hw_line, int n_comp_density,
                                     int n_comp_app, int with_tv_density, int with_tv_app, float* scratch640,
                                     float* out3, void* stream) {
  RegSet S;
  int rc = reg_set(factors, nullptr, plane_hw_line, n_comp_density, n_comp_app, &S);
  if (rc) return rc;
  if (!scratch640 || !out3) return JT_ERR_ARG;
  RegBatch B;
  RegDims Dm;
  int nblk;
  if ((rc = reg_batch(kRegBatchFwd, S, with_tv_density, with_tv_app, &B, &Dm, &nblk))) return rc;
  hipLaunchKernelGGL(k_reg_batch_fwd, dim3(nblk), dim3(256), 0, (hipStream_t)stream, B, Dm, scratch640, out3);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_reg_losses_backward(const JtFactors* factors, const int32_t* plane_hw_line, int n_comp_density,
                                      int n_comp_app, const float* g3, int with_tv_density, int with_tv_app,
                                      const JtFactors* g_factors, int accumulate, float* scratch640, void* stream) {
  RegSet S;
  int rc = reg_set(factors, g_factors, plane_hw_line, n_comp_density, n_comp_app, &S);
  if (rc) return rc;
  if (!g3 || !scratch640 || !g_factors) return JT_ERR_ARG;
  RegBatch B;
  int nblk;
  if ((rc = reg_batch(kRegBatchBwd, S, with_tv_density, with_tv_app, &B, nullptr, &nblk))) return rc;
  hipLaunchKernelGGL(k_reg_batch_bwd, dim3(nblk), dim3(256), 0, (hipStream_t)stream, B, g3, accumulate ? 1 : 0);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_reg_losses_fused(const JtFactors* factors, const int32_t* plane_hw_line, int n_comp_density, int n_comp_app,
                                   int with_tv_density, int with_tv_app, const float* w3_host, const float* w3_dev,
                                   const JtFactors* g_factors, float* scratch640, float* out3, void* stream) {
  RegSet S;
  int rc = reg_set(factors, g_factors, plane_hw_line, n_comp_density, n_comp_app, &S);
  if (rc) return rc;
  if (!scratch640 || !out3 || !g_factors || (!w3_host && !w3_dev)) return JT_ERR_ARG;
  if (jt_deterministic()) return JT_ERR_UNSUPPORTED;  // (the fixed summation order lives in the two-launch form)
  RegBatch B;
  RegDims Dm;
  int nblk;
  if ((rc = reg_batch(kRegFused, S, with_tv_density, with_tv_app, &B, &Dm, &nblk))) return rc;
  RegWeights Wt;
  for (int k = 0; k < 3; ++k) Wt.w[k] = w3_host ? w3_host[k] : 0.f;
  Wt.dev = w3_host ? nullptr : w3_dev;
  hipLaunchKernelGGL(k_reg_batch_fused, dim3(nblk), dim3(256), 0, (hipStream_t)stream, B, Dm, Wt, scratch640, out3);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
