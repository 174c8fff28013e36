// The host decisions between the locked LOBPCG sweeps (lobpcg_small.hpp: sweep_want, lock_prefix, unlocked_flag,
// sweep_args) as a plain C++ program: g++ -std=c++17 -fsanitize=address,undefined.  It replays the sweep loop
// of Engine::eigs_run on flag patterns -- full locks, partial prefixes, a converged column behind an unconverged one, p = 0 --
// and checks the bookkeeping: every wanted column is locked once, in order, the carried columns keep their order, nothing
// reads past a block.
#include <cstdio>
#include <vector>

#include "lobpcg_small.hpp"

using namespace hifamd;

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                               \
    }                                                        \
  } while (0)

// one replay: column ids instead of vectors.  locks(t, j): whether candidate j of sweep t converges.
template <class Conv>
static void replay(int nev, int k, int guard, Conv conv, int expect_locked, int expect_sweeps) {
  std::vector<int> block(k), out;  // ids of the start block's columns; the locked ids in lock order
  int next_id = 0, L = 0, sweeps = 0;
  for (int j = 0; j < k; ++j) block[j] = next_id++;
  for (int t = 0;; ++t) {
    const int want = lob::sweep_want(nev, L, k, guard);
    CHECK(want >= 1 && want <= k - guard && want <= nev - L);
    std::vector<int> fl(k);  // heap blocks of exactly k ints: an overrun is the sanitizer's
    for (int j = 0; j < k; ++j) fl[j] = conv(t, j) ? 0 : 2;
    const int p = lob::lock_prefix(fl.data(), want);
    ++sweeps;
    CHECK(p >= 0 && p <= want);
    for (int j = 0; j < p; ++j) CHECK(fl[j] == 0);
    if (p < want) CHECK(fl[p] != 0);
    if (p == 0) break;
    for (int j = 0; j < p; ++j) out.push_back(block[j]);
    L += p;
    if (L == nev) break;
    // the next start block as Engine::eigs_run builds it: columns p .. k - 1 carried in their order, then p generated ones
    std::vector<int> nxt;
    for (int j = p; j < k; ++j) nxt.push_back(block[j]);
    for (int j = 0; j < p; ++j) nxt.push_back(next_id++);
    CHECK((int)nxt.size() == k);
    block = nxt;
  }
  CHECK(L == expect_locked && sweeps == expect_sweeps && (int)out.size() == L);
  for (size_t i = 0; i < out.size(); ++i)
    for (size_t j = i + 1; j < out.size(); ++j) CHECK(out[i] != out[j]);
}

int main() {
  // the table's shapes: everything wanted converges
  replay(40, 16, 4, [](int, int) { return true; }, 40, 4);   // 12 12 12 4
  replay(30, 8, 2, [](int, int) { return true; }, 30, 5);    // five sweeps of 6
  replay(20, 16, 4, [](int, int) { return true; }, 20, 2);   // 12 8
  replay(1, 1, 0, [](int, int) { return true; }, 1, 1);
  replay(13, 16, 4, [](int, int) { return true; }, 13, 2);   // the last sweep wants one column
  replay(128, 16, 0, [](int, int) { return true; }, 128, 8);  // p == k: nothing carried
  // a partial prefix, then the rest
  replay(10, 8, 2, [](int t, int j) { return t > 0 || j < 2; }, 10, 3);  // 2, 6, 2
  // a converged column behind an unconverged one is not locked
  replay(6, 8, 2, [](int t, int j) { return t > 0 || j != 1; }, 6, 2);   // 1, then 5
  // p == 0 in the second sweep: the earlier columns stay locked
  replay(12, 8, 2, [](int t, int) { return t == 0; }, 6, 2);
  replay(12, 8, 2, [](int, int j) { return j > 0; }, 0, 1);

  CHECK(lob::sweep_want(40, 36, 16, 4) == 4 && lob::sweep_want(40, 0, 16, 4) == 12 && lob::sweep_want(1, 0, 1, 0) == 1);
  const int f0[4] = {0, 0, 2, 0}, f1[4] = {1, 0, 0, 0}, f2[4] = {0, 0, 0, 0};
  CHECK(lob::lock_prefix(f0, 4) == 2 && lob::lock_prefix(f0, 1) == 1 && lob::lock_prefix(f1, 4) == 0);
  CHECK(lob::lock_prefix(f2, 4) == 4 && lob::lock_prefix(f2, 3) == 3 && lob::lock_prefix(f2, 0) == 0);
  CHECK(lob::unlocked_flag(0) == 2 && lob::unlocked_flag(1) == 1 && lob::unlocked_flag(2) == 2);
  CHECK(lob::sweep_args(40, 16, 4, 0) == nullptr && lob::sweep_args(32, 16, 4, 96) == nullptr);
  CHECK(lob::sweep_args(1, 1, 0, 0) == nullptr && lob::sweep_args(128, 16, 15, 0) == nullptr);
  CHECK(lob::sweep_args(33, 16, 4, 96) != nullptr && lob::sweep_args(129, 16, 4, 0) != nullptr);
  CHECK(lob::sweep_args(4, 17, 4, 0) != nullptr && lob::sweep_args(4, 0, 0, 0) != nullptr);
  CHECK(lob::sweep_args(4, 8, 8, 0) != nullptr && lob::sweep_args(4, 8, -1, 0) != nullptr);
  CHECK(lob::sweep_args(0, 8, 2, 0) != nullptr && lob::sweep_args(4, 8, 2, -1) != nullptr);
  if (fails) {
    std::printf("%d FAILED\n", fails);
    return 1;
  }
  std::printf("EIGS SMALL TEST OK\n");
  return 0;
}
