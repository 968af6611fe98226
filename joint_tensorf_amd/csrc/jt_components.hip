// Connected components of the inside points of a scalar lattice, with the connectivity of the mesh that csrc/jt_mesh.hip takes
// from the same lattice: two points are adjacent iff both are inside (v > level; a NaN is outside) and they differ by + or - one
// of the seven edge kinds +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z -- 14 neighbours, the edges of the Kuhn triangulation.  All four
// corners of a Kuhn tetrahedron are pairwise joined by such edges, so a tetrahedron's inside corners lie in ONE component and
// the surface splits exactly along components: dropping a component drops a closed piece of the mesh and touches no other.
//
// labels [nx][ny][nz] int32, z fastest: -1 outside, else the smallest flat index of the point's component.  That fixed point is
// unique, so the result is a function of the lattice alone, whatever the schedule.
//
// Min-label propagation.  k_components_init: label = own index (inside) or -1.  k_components_sweep: a workgroup owns an 8 x 8 x 8
// tile, holds it and a one-point halo in LDS, lowers every inside label to the minimum over its 14 neighbours until the tile is
// stable (every thread writes its own LDS word only; a pass ends in a workgroup vote), writes back the words of ITS tile that
// fell and raises *lowered.  k_components_jump: label[p] = label[label[...]] down the chain (labels are indices of points of the
// same component and only ever fall, so the chain ends).  The caller launches sweeps until one lowers nothing.
//
// No workgroup waits for another inside a launch.  A halo word that the neighbouring workgroup lowers during the same launch
// may or may not be seen, and may come from a stale cache line: any value it ever held is a valid (not yet minimal) label of
// that component, labels only fall, and the neighbour has raised the flag, so another sweep follows.  Values become visible at
// the kernel boundary.  A sweep that lowered nothing stored nothing, so every word it read was current: every inside point then
// holds a label <= each neighbour's, by symmetry the label is constant over a component, and since label[p] <= p throughout
// and a label is always the index of a point of the component, the constant is the component's smallest index.
//
// Labels are handled as unsigned words: -1 is the largest, so a minimum skips outside points and the halo beyond the lattice
// without a test.
#include "jt_common.h"

namespace jt {

constexpr int kCompTile = JT_COMPONENTS_TILE;            // points per tile edge
constexpr int kCompHalo = kCompTile + 2;
constexpr int kCompThreads = kCompTile * kCompTile * kCompTile;
constexpr int kCompCells = kCompHalo * kCompHalo * kCompHalo;
constexpr unsigned kCompOutside = 0xffffffffu;
static_assert(kCompThreads == 512, "one thread per tile point, eight waves");

__global__ __launch_bounds__(256) void k_components_init(const float* __restrict__ lattice, int n, float level,
                                                         int32_t* __restrict__ labels) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) labels[i] = lattice[i] > level ? i : -1;
}

__global__ __launch_bounds__(kCompThreads) void k_components_sweep(int nx, int ny, int nz, int tiles_y, int tiles_z,
                                                                   uint32_t* __restrict__ labels, int32_t* __restrict__ lowered) {
  __shared__ unsigned lab[kCompCells];
  const int t = (int)threadIdx.x;
  const int tile = (int)blockIdx.x;
  const int x0 = tile / (tiles_y * tiles_z) * kCompTile, y0 = tile / tiles_z % tiles_y * kCompTile, z0 = tile % tiles_z * kCompTile;
  // this thread's point: z fastest, like the lattice
  const int lz = t % kCompTile, ly = t / kCompTile % kCompTile, lx = t / (kCompTile * kCompTile);
  const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
  const bool live = x < nx && y < ny && z < nz;
  const int idx = live ? (x * ny + y) * nz + z : 0;
  const unsigned first = live ? labels[idx] : kCompOutside;
  if (!__syncthreads_or(first != kCompOutside)) return;    // a tile without an inside point
  for (int c = t; c < kCompCells; c += kCompThreads) {
    const int hx = x0 - 1 + c / (kCompHalo * kCompHalo), hy = y0 - 1 + c / kCompHalo % kCompHalo, hz = z0 - 1 + c % kCompHalo;
    const bool in = hx >= 0 && hx < nx && hy >= 0 && hy < ny && hz >= 0 && hz < nz;
    lab[c] = in ? labels[(hx * ny + hy) * nz + hz] : kCompOutside;
  }
  __syncthreads();
  const int me = ((lx + 1) * kCompHalo + (ly + 1)) * kCompHalo + (lz + 1);
  unsigned mine = first;             // (only this workgroup stores into its tile: lab[me] is the same word)
  for (;;) {
    int fell = 0;
    if (mine != kCompOutside) {
      unsigned m = mine;
#pragma unroll
      for (int k = 1; k < 8; ++k) {   // offset mask k = dx | dy << 1 | dz << 2: the seven kinds, each in both directions
        const int d = ((k & 1) * kCompHalo + ((k >> 1) & 1)) * kCompHalo + ((k >> 2) & 1);
        m = min(m, min(lab[me + d], lab[me - d]));
      }
      if (m < mine) {
        mine = m;
        lab[me] = m;
        fell = 1;
      }
    }
    if (!__syncthreads_or(fell)) break;
  }
  const bool store = live && mine < first;
  if (store) labels[idx] = mine;
  if (__syncthreads_or(store) && t == 0) atomicOr(lowered, 1);
}

__global__ __launch_bounds__(256) void k_components_jump(int n, int32_t* __restrict__ labels) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const int first = labels[i];
  if (first < 0 || first >= n) return;
  int l = first;
  for (;;) {                          // strictly falling and never below 0: at most `first` steps, in practice a handful
    const int up = labels[l];
    if (up < 0 || up >= l) break;
    l = up;
  }
  if (l < first) labels[i] = l;
}

// sizes[label] += 1 per inside point (sizes zeroed by the caller).  A wave whose live lanes all carry one label -- the inside of a
// large component -- adds once.
__global__ __launch_bounds__(256) void k_component_sizes(const int32_t* __restrict__ labels, int n, int32_t* __restrict__ sizes) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  int l = i < n ? labels[i] : -1;
  l = l < n ? l : -1;                 // (no label names a point beyond the lattice; one that did is not counted)
  const unsigned long long in = __ballot(l >= 0);
  if (!in) return;
  const int lead = __shfl(l, __ffsll((long long)in) - 1);
  const bool uniform = __ballot(l >= 0 && l != lead) == 0ull;
  if (uniform) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)in) - 1) atomicAdd(&sizes[lead], (int)__popcll(in));
  } else if (l >= 0) {
    atomicAdd(&sizes[l], 1);
  }
}

static int components_shape(const void* labels, int nx, int ny, int nz, long* n) {
  if (!labels || nx < 2 || ny < 2 || nz < 2) return JT_ERR_ARG;
  *n = (long)nx * (long)ny * (long)nz;
  return *n > (1l << 27) ? JT_ERR_UNSUPPORTED : JT_OK;
}

}  // namespace jt

using namespace jt;

extern "C" int jt_components_init(const float* lattice, int nx, int ny, int nz, float level, int32_t* labels, void* stream) {
  long n = 0;
  if (!lattice || !__builtin_isfinite(level)) return JT_ERR_ARG;
  if (const int rc = components_shape(labels, nx, ny, nz, &n)) return rc;
  hipLaunchKernelGGL(k_components_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lattice, (int)n, level,
                     labels);
  JT_LAUNCH_CHECK();
  return JT_OK;
}

extern "C" int jt_components_sweep(int32_t* labels, int nx, int ny, int nz, int32_t* lowered, int jump, void* stream) {
  long n = 0;
  if (!lowered) return JT_ERR_ARG;
  if (const int rc = components_shape(labels, nx, ny, nz, &n)) return rc;
  const int tx = (nx + kCompTile - 1) / kCompTile, ty = (ny + kCompTile - 1) / kCompTile, tz = (nz + kCompTile - 1) / kCompTile;
  hipLaunchKernelGGL(k_components_sweep, dim3((unsigned)((long)tx * ty * tz)), dim3(kCompThreads), 0, (hipStream_t)stream, nx, ny, nz,
                     ty, tz, reinterpret_cast<uint32_t*>(labels), lowered);
  JT_LAUNCH_CHECK();
  if (jump) {
    hipLaunchKernelGGL(k_components_jump, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)n, labels);
    JT_LAUNCH_CHECK();
  }
  return JT_OK;
}

extern "C" int jt_component_sizes(const int32_t* labels, int nx, int ny, int nz, int32_t* sizes, void* stream) {
  long n = 0;
  if (!sizes) return JT_ERR_ARG;
  if (const int rc = components_shape(labels, nx, ny, nz, &n)) return rc;
  hipLaunchKernelGGL(k_component_sizes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, labels, (int)n, sizes);
  JT_LAUNCH_CHECK();
  return JT_OK;
}
