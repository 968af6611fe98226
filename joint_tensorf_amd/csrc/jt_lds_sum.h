// Adding a float into a shared 32-bit cell WITHOUT a float atomic.
//
// On gfx950 ds_add_f32 retires one lane every three cycles (193 cycles per full wave instruction) while the integer LDS
// atomics, exchange and compare-and-swap among them, run at 5-8 cycles per instruction (tools/lds_atomic_rate.hip).  Where
// an LDS accumulator cannot be a double (RecWalker, LDSL == 1) the sum is therefore formed by the lanes themselves and only
// MOVED through the cell with an integer atomic.
//
// The routines are written against an abstract cell of 32 bits
//     uint32_t load();  uint32_t exchange(uint32_t v);  uint32_t cas(uint32_t expected, uint32_t desired);  (both return the
//     previous content)   void add(float v);   (the float atomic: the fallback)
// and are instantiated on the device for an LDS word (LdsCell) and on the host for std::atomic<uint32_t>
// (tests/csrc/lds_sum_host.cpp runs exactly this code under threads).
//
// Common properties of both forms:
//  * The cell always holds a valid partial sum or zero; what is not in the cell is held by exactly one lane.  cell + held
//    values = everything added so far, at every instant, under any interleaving (same-address lanes of one instruction are
//    serialised by the LDS in some order, which is one such interleaving).
//  * The loop runs kLdsSumRounds times at most and no exit waits for another lane: a lane that still holds something after
//    the last round adds it with the float atomic, which is correct whatever the cell holds.
//  * NaN: decisions are taken on BITS (cas) or on `!= 0.f` (exchange: true for a NaN), never on `==` of two floats, so a
//    NaN neither ends a loop early nor keeps one alive -- it is carried like any value, poisons the sum it is added to (as
//    the float atomic would) and the round bound ends the loop.
//  * -0: a held -0 is dropped and a returned -0 counts as "nothing came back".  The SUM does not change (x + -0 == x); at
//    most a cell that should read -0 reads +0, and readers of the line treat both as "nothing to add".
//  * Exact cancellation (held + taken == 0): the lane holds nothing any more and stops; the cell was left at zero by the
//    take, which is the right sum.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JT_LDS_SUM_HD __host__ __device__
#else
#define JT_LDS_SUM_HD
#endif

// which form sums the float LDS line (RecWalker::flush_lds, LDSL == 1): 0 = the float atomic itself (the form up to now, kept
// for A/B variants: tools/build_variant.py <name> -DJT_LDS_LINE_SUM=0), 1 = compare-and-swap, 2 = exchange
#ifndef JT_LDS_LINE_SUM
#define JT_LDS_LINE_SUM 1
#endif

namespace jt {

constexpr int kLdsSumRounds = 8;

JT_LDS_SUM_HD inline uint32_t lds_sum_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
JT_LDS_SUM_HD inline float lds_sum_float(uint32_t b) { return __builtin_bit_cast(float, b); }

// compare-and-swap: read, add, write back if the cell still holds what was read.  A cell that went A -> B -> A in between
// passes the comparison, and rightly so: old + a is the sum whichever way the cell came to hold `old`.
// ROUNDS = 0 is the fallback alone (tests).
template <int ROUNDS = kLdsSumRounds, class Cell>
JT_LDS_SUM_HD inline void lds_sum_cas(Cell c, float a) {
  if (ROUNDS > 0) {
    uint32_t old = c.load();
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
      const uint32_t want = lds_sum_bits(lds_sum_float(old) + a);
      const uint32_t got = c.cas(old, want);
      if (got == old) return;  // bits: a NaN in the cell compares equal to itself here
      old = got;
    }
  }
  c.add(a);
}

// exchange: take the cell's content out (leaving zero), add it to what the lane holds, put the sum back; whatever the
// second exchange returns was deposited by somebody else in between and is now held by this lane -- go round again.
template <int ROUNDS = kLdsSumRounds, class Cell>
JT_LDS_SUM_HD inline void lds_sum_xchg(Cell c, float a) {
  float v = a;
#pragma unroll 1
  for (int r = 0; r < ROUNDS; ++r) {
    if (!(v != 0.f)) return;  // nothing held (or -0): done.  A NaN is "something"
    v += lds_sum_float(c.exchange(0u));
    if (!(v != 0.f)) return;  // cancelled exactly: the cell keeps the zero the take left
    v = lds_sum_float(c.exchange(lds_sum_bits(v)));
  }
  if (v != 0.f) c.add(v);
}

template <int FORM, class Cell>
JT_LDS_SUM_HD inline void lds_sum(Cell c, float a) {
  if (FORM == 1) lds_sum_cas(c, a);
  else if (FORM == 2) lds_sum_xchg(c, a);
  else c.add(a);
}

#if defined(__HIPCC__)
// a word of the workgroup's LDS (the address space is inferred once the caller is inlined, as for the float atomic)
struct LdsCell {
  float* p;
  __device__ inline uint32_t load() const {
    return __hip_atomic_load(reinterpret_cast<uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ inline uint32_t exchange(uint32_t v) const {
    return __hip_atomic_exchange(reinterpret_cast<uint32_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ inline uint32_t cas(uint32_t expected, uint32_t desired) const {
    __hip_atomic_compare_exchange_strong(reinterpret_cast<uint32_t*>(p), &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_WORKGROUP);
    return expected;
  }
  __device__ inline void add(float v) const { atomicAdd(p, v); }
};
#endif

}  // namespace jt
