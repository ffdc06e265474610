// The planner of the sample-space solve's Gram launch (plan.hpp: plan_sr_gram*) under AddressSanitizer +
// UndefinedBehaviourSanitizer on the CPU (`make -C cgs_vmc_amd/csrc hostcheck_srgram`, tests/test_sr_gram.py).  For every
// number of stored samples of interest it walks the linear grid of k_sr_gram as the kernel does and marks the tiles in a
// real nt x nt array:
//   * every tile (i, j) with j >= i is produced exactly once, no tile below the diagonal;
//   * no tile starts at or beyond row / column n;
//   * the grid is nt (nt + 1) / 2 workgroups; the LDS of a workgroup fits a CU;
//   * the cap refuses n > 16,384 (16,385 here) and nothing at or below it; n < 1 is refused too.
#include "plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static long long g_checks = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    ++g_checks;                                                                             \
    if (!(cond)) { fprintf(stderr, "hostcheck_srgram: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

static void check_n(long long n) {
  SrGramPlan p{};
  char msg[256] = "";
  const int rc = plan_sr_gram(n, &p, msg, sizeof(msg));
  if (n > 16384) {
    CHECK(rc == VMC_ERR_UNSUPPORTED);
    CHECK(msg[0] != 0);
    return;
  }
  CHECK(rc == VMC_OK);
  const int nt = p.nt;
  CHECK((long long)nt * SRG_TILE >= n && (long long)(nt - 1) * SRG_TILE < n);
  CHECK(p.grid == (long long)nt * (nt + 1) / 2);
  CHECK(p.lds_bytes == plan_sr_gram_lds_bytes() && p.lds_bytes <= PLAN_LDS_PER_CU);
  CHECK(p.lds_bytes == sizeof(float) * 2 * SRG_TILE * SRG_LD);
  std::vector<int> seen((size_t)nt * (size_t)nt, 0);
  int last_i = 0, last_j = -1;
  for (long long idx = 0; idx < p.grid; ++idx) {
    int i = -1, j = -1;
    plan_sr_gram_tile(idx, nt, &i, &j);
    CHECK(i >= 0 && i < nt && j >= i && j < nt);
    CHECK((long long)i * SRG_TILE < n && (long long)j * SRG_TILE < n);
    CHECK(i > last_i ? (i == last_i + 1 && j == i) : (i == last_i && j == last_j + 1));     // row by row, ascending
    last_i = i; last_j = j;
    seen[(size_t)i * (size_t)nt + (size_t)j] += 1;
  }
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nt; ++j) CHECK(seen[(size_t)i * (size_t)nt + (size_t)j] == (j >= i ? 1 : 0));
}

int main() {
  int cases = 0;
  for (long long n = 1; n <= 300; ++n, ++cases) check_n(n);
  for (long long n : {516LL, 1024LL, 1025LL, 1040LL, 1100LL}) { check_n(n); ++cases; }      // tests/sr_gram_shape_cases.py
  for (long long n : {4095LL, 4096LL, 4097LL, 16384LL, 16385LL}) { check_n(n); ++cases; }
  {
    SrGramPlan p{};
    char msg[256] = "";
    CHECK(plan_sr_gram(0, &p, msg, sizeof(msg)) == VMC_ERR_STATE);
    CHECK(plan_sr_gram(-5, &p, msg, sizeof(msg)) == VMC_ERR_STATE);
    CHECK(plan_sr_gram(16384, &p, msg, sizeof(msg)) == VMC_OK && p.nt == 16384 / SRG_TILE);
    CHECK(plan_sr_gram(16385, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
    CHECK(plan_sr_gram(1LL << 40, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  }
  printf("hostcheck_srgram ok: %d cases, %lld assertions\n", cases, g_checks);
  return 0;
}
