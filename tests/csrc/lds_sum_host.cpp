// Host instantiation of the float sums of joint_tensorf_amd/csrc/jt_lds_sum.h: the routines the walkers run on LDS words,
// here on std::atomic<uint32_t> cells under real threads (tests/test_lds_line_sum_host.py builds and runs this program, once
// plainly and once under ThreadSanitizer).
//
// T threads add integer-valued floats (so every total is exact whatever the order) into K cells, K from 1 to 36.  The threads
// differ in the form they use -- compare-and-swap, exchange, each with the full round bound, with ONE round (so that the
// float-atomic fallback is taken whenever another thread gets in between) and with no round at all (the fallback alone) --
// and in where they add: spread over the K cells, or all of them on cell 0.  Negative addends make partial sums pass through
// zero, the value the exchange form reads as "nothing there".  Exit status 0 iff every cell of every case holds its exact total.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "jt_lds_sum.h"

namespace {

struct HostCell {
  std::atomic<uint32_t>* p;
  uint32_t load() const { return p->load(std::memory_order_relaxed); }
  uint32_t exchange(uint32_t v) const { return p->exchange(v, std::memory_order_relaxed); }
  uint32_t cas(uint32_t expected, uint32_t desired) const {
    p->compare_exchange_strong(expected, desired, std::memory_order_relaxed, std::memory_order_relaxed);
    return expected;
  }
  // the float atomic (on the device one LDS instruction)
  void add(float v) const {
    uint32_t old = p->load(std::memory_order_relaxed);
    while (!p->compare_exchange_weak(old, jt::lds_sum_bits(jt::lds_sum_float(old) + v), std::memory_order_relaxed,
                                     std::memory_order_relaxed)) {
    }
  }
};

constexpr int kForms = 6;
void add_form(int form, HostCell c, float v) {
  switch (form) {
    case 0: jt::lds_sum_cas<jt::kLdsSumRounds>(c, v); break;
    case 1: jt::lds_sum_xchg<jt::kLdsSumRounds>(c, v); break;
    case 2: jt::lds_sum_cas<1>(c, v); break;
    case 3: jt::lds_sum_xchg<1>(c, v); break;
    case 4: jt::lds_sum_cas<0>(c, v); break;   // the fallback alone
    default: jt::lds_sum<JT_LDS_LINE_SUM>(c, v); break;  // whatever form the library is built with
  }
}

// forms: bit mask of the forms the threads of this case cycle through; one_cell: every thread adds to cell 0 only
bool run_case(int K, int T, int N, unsigned forms, bool one_cell) {
  std::vector<std::atomic<uint32_t>> cells(K);
  for (auto& c : cells) c.store(0u);
  std::vector<std::vector<long long>> want(T, std::vector<long long>(K, 0));
  std::vector<int> list;
  for (int f = 0; f < kForms; ++f)
    if (forms & (1u << f)) list.push_back(f);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) {
    th.emplace_back([&, t] {
      const int form = list[t % list.size()];
      uint32_t s = 2654435761u * (uint32_t)(t + 1) + (uint32_t)K;
      for (int i = 0; i < N; ++i) {
        s = s * 1664525u + 1013904223u;
        const int k = one_cell ? 0 : (int)((s >> 8) % (uint32_t)K);
        const int v = (int)((s >> 20) % 12u) - 4;  // -4 .. 7, zero among them
        add_form(form, HostCell{&cells[k]}, (float)v);
        want[t][k] += v;
      }
    });
  }
  for (auto& x : th) x.join();
  bool ok = true;
  for (int k = 0; k < K; ++k) {
    long long w = 0;
    for (int t = 0; t < T; ++t) w += want[t][k];
    const float got = jt::lds_sum_float(cells[k].load());
    if ((double)got != (double)w) {
      std::printf("  K %d T %d forms 0x%x one_cell %d: cell %d holds %.1f, expected %lld\n", K, T, forms, (int)one_cell, k,
                  (double)got, w);
      ok = false;
    }
  }
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  const int N = argc > 1 ? std::atoi(argv[1]) : 20000;  // adds per thread: 12 threads x 20 000 x 7 < 2^24, sums stay exact
  const int T = 12;
  const int Ks[] = {1, 2, 3, 5, 8, 13, 24, 36};
  int bad = 0, cases = 0;
  for (int K : Ks) {
    const unsigned mixes[] = {0x01u, 0x02u, 0x05u, 0x0au, 0x3fu};  // cas / exchange / each with its one-round twin / everything
    for (unsigned m : mixes) {
      bad += !run_case(K, T, N, m, false), ++cases;
      bad += !run_case(K, T, N, m, true), ++cases;
    }
  }
  std::printf("lds_sum_host: %d cases, %d wrong\n", cases, bad);
  return bad ? 1 : 0;
}
