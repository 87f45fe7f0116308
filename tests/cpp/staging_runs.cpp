// make_runs / rebase of cbird_amd/csrc/cbh_runs.h on cases from stdin (tests/test_staging_runs.py).  Host code only: links nothing.
// In:  per case "n budget max_m" and then n pairs "off end".
// Out: per case one line "i0 m lo hi rel[0] .. rel[m-1]" per run joined by " | ".
#include <cinttypes>
#include <cstdio>

#include "cbh_runs.h"

int main() {
  unsigned long long n, budget, max_m;
  while (scanf("%llu %llu %llu", &n, &budget, &max_m) == 3) {
    std::vector<uint64_t> off(n), end(n), rel;
    for (size_t i = 0; i < n; ++i) {
      unsigned long long a, b;
      if (scanf("%llu %llu", &a, &b) != 2) return 2;
      off[i] = a, end[i] = b;
    }
    const std::vector<cbh::Run> runs = cbh::make_runs(n, off.data(), end.data(), budget, max_m);
    for (size_t k = 0; k < runs.size(); ++k) {
      const cbh::Run& r = runs[k];
      printf("%s%zu %zu %" PRIu64 " %" PRIu64, k ? " | " : "", r.i0, r.m, r.lo, r.hi);
      cbh::rebase(r, off.data(), &rel);
      for (uint64_t v : rel) printf(" %" PRIu64, v);
    }
    printf("\n");
  }
  return 0;
}
