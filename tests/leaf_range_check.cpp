// Host-only check of gi_layout.h's leaf ranges (built and run by test_leaf_range.py):
// kd_leaf_start(n, levels, j) against the division it replaced, j * n / (1 << levels), for every
// j in [0, L]; the starts are monotone, start(0) = 0 and start(L) = n; kd_leaf_range returns two
// consecutive starts; kd_levels_ok accepts exactly nleaves == 1 << levels.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gi_layout.h"

using namespace gi;

static long long g_checked = 0;

static int check(int64_t n, int levels) {
  const int64_t L = (int64_t)1 << levels;
  KdView v{};
  v.n = n;
  v.nleaves = (int32_t)L;
  v.levels = levels;
  int64_t prev = 0;
  for (int64_t j = 0; j <= L; j++) {
    const int64_t got = kd_leaf_start(n, levels, j);
    const int64_t want = j * n / L;  // the formula of the layout before the shift
    if (got != want || got < prev) {
      fprintf(stderr, "n %lld levels %d j %lld: start %lld, division %lld, previous %lld\n",
              (long long)n, levels, (long long)j, (long long)got, (long long)want, (long long)prev);
      return 1;
    }
    if (j < L) {
      int64_t s0 = -1, s1 = -1;
      kd_leaf_range(v, (int)j, s0, s1);
      if (s0 != got || s1 != (j + 1) * n / L) {
        fprintf(stderr, "n %lld levels %d leaf %lld: range [%lld, %lld)\n", (long long)n, levels,
                (long long)j, (long long)s0, (long long)s1);
        return 1;
      }
    }
    prev = got;
    g_checked++;
  }
  if (kd_leaf_start(n, levels, 0) != 0 || kd_leaf_start(n, levels, L) != n) {
    fprintf(stderr, "n %lld levels %d: ends %lld, %lld\n", (long long)n, levels,
            (long long)kd_leaf_start(n, levels, 0), (long long)kd_leaf_start(n, levels, L));
    return 1;
  }
  return 0;
}

int main() {
  const int64_t big = 2147483647;  // 2^31 - 1
  for (int levels = 0; levels <= 20; levels++) {
    const int64_t L = (int64_t)1 << levels;
    // around L (fewer photons than leaves: empty leaves), around the leaf sizes in use, where
    // j * n crosses 2^32 inside the map, and the largest photon count an int32 index holds
    std::vector<int64_t> ns = {0, 1, 2, 17, 1000, 300001, 1000011, L - 1, L, L + 1, 16 * L - 1, 16 * L,
                               64 * L + 63, 256 * L - 255, ((int64_t)1 << 32) / L + 1, big - 1, big};
    for (int64_t n : ns)
      if (n >= 0 && n <= big && check(n, levels)) return 1;
  }
  if (check(10000000, 17)) return 1;  // C4's caustic map
  for (int levels = -1; levels <= 32; levels++)
    for (int64_t nl : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)4096, (int64_t)16384,
                       (int64_t)1 << 30, ((int64_t)1 << 31) - 1}) {
      const bool want = levels >= 0 && levels <= 30 && nl == (int64_t)1 << levels;
      if (kd_levels_ok((int32_t)nl, levels) != want) {
        fprintf(stderr, "kd_levels_ok(%lld, %d) != %d\n", (long long)nl, levels, (int)want);
        return 1;
      }
    }
  printf("ok %lld starts\n", g_checked);
  return 0;
}
