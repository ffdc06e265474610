// The planner of the Lanczos-step energies (plan.hpp: plan_moment_*) under AddressSanitizer + UndefinedBehaviourSanitizer
// on the CPU (`make -C cgs_vmc_amd/csrc hostcheck_moments`, tests/test_moments.py).  It re-derives every index the kernels
// of moments.hip take from the plan into real arrays of the planned size:
//   * the 32-bit index rule against exact 128-bit arithmetic;
//   * the pass size against its budget, the caller's limit and the request;
//   * for lists of random per-row counts and every pass size of interest: the slice of a pass a first-order row fills
//     (k_mom_fill: desc[q - q0]) and the rows a lane of a chain adds (k_mom_accum: plan_moment_first_row, step 64) --
//     every row of the list is written once and read once, by the lane (place mod 64), in ascending order per lane
//     whatever the pass size.
#include "plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

static long long g_checks = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    ++g_checks;                                                                             \
    if (!(cond)) { fprintf(stderr, "hostcheck_moments: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

static void check_index_rule() {
  const long long Bs[] = {1, 2, 40, 1024, 4096, 65536, 1LL << 20, 0x7fffffffLL, 0, -1};
  const long long nbs[] = {1, 2, 32, 64, 200, 724, 725, 46340, 46341, 1LL << 20, 0x7fffffffLL, 0x80000000LL, 0, -3};
  for (long long B : Bs)
    for (long long nb : nbs) {
      const bool exact = B >= 1 && nb >= 1 && (__int128)B * nb * nb <= (__int128)0x7fffffff;
      CHECK(plan_moment_index_ok(B, nb) == exact);
    }
  CHECK(plan_moment_index_ok(4096, 200));          // config 3's shape
  CHECK(!plan_moment_index_ok(4096, 725));
}

static void check_per_pass() {
  const long long n2s[] = {0, 1, 7, 64, 65, 1000, 1LL << 24, (1LL << 24) + 1, 0x7fffffffLL};
  const long long reqs[] = {0, 1, 7, 64, 1000, 1LL << 30};
  const long long limits[] = {0, 1, 5, 1LL << 20, 1LL << 40};
  for (long long n2 : n2s)
    for (long long req : reqs)
      for (long long lim : limits) {
        const long long per = plan_list_per_pass(n2, req, lim);
        CHECK(per >= 1 && per <= PLAN_MEASURE_ROW_BUDGET);
        if (lim > 0) CHECK(per <= lim);
        if (req > 0) CHECK(per <= req);
        if (n2 > 0) CHECK(per <= n2);
        CHECK((long long)(int)per == per);
        const long long passes = plan_measure_passes(n2, (int)per);
        CHECK(passes * per >= n2 && (passes == 0 || (passes - 1) * per < n2));
      }
  CHECK(plan_list_per_pass(-1, 0, 0) == -1 && plan_list_per_pass(5, -1, 0) == -1 && plan_list_per_pass(5, 0, -1) == -1);
}

// a list: B chains, first-order rows per chain, second-order rows per first-order row
static void check_list(std::mt19937& rng, int B, int max_first, int max_second, const std::vector<long long>& pass_sizes) {
  std::vector<int> off((size_t)B + 1, 0);
  for (int c = 0; c < B; ++c) off[(size_t)c + 1] = off[(size_t)c] + (int)(rng() % (unsigned)(max_first + 1));
  const int n1 = off[(size_t)B];
  std::vector<int> off2((size_t)n1 + 1, 0);
  for (int r = 0; r < n1; ++r) off2[(size_t)r + 1] = off2[(size_t)r] + (int)(rng() % (unsigned)(max_second + 1));
  const long long n2 = off2[(size_t)n1];
  std::vector<int> last_by_lane((size_t)B * 64);
  for (long long req : pass_sizes) {
    const long long per = plan_list_per_pass(n2, req, 0);
    std::vector<int> written((size_t)n2, 0), read((size_t)n2, 0);
    std::fill(last_by_lane.begin(), last_by_lane.end(), -1);
    bool inside = false;
    for (long long q0 = 0; q0 < n2; q0 += per) {
      const int n = (int)(n2 - q0 < per ? n2 - q0 : per);
      std::vector<int> desc((size_t)per, -1);                  // the pass's descriptor buffer, exactly as reserved
      for (int r = 0; r < n1; ++r) {                           // k_mom_fill
        if (off2[(size_t)r + 1] <= q0 || off2[(size_t)r] >= q0 + n) continue;
        for (long long at = off2[(size_t)r]; at < off2[(size_t)r + 1]; ++at)
          if (at >= q0 && at < q0 + n) { CHECK(desc[(size_t)(at - q0)] == -1); desc[(size_t)(at - q0)] = r; written[(size_t)at] += 1; }
      }
      for (int k = 0; k < n; ++k) CHECK(desc[(size_t)k] >= 0);
      for (int c = 0; c < B; ++c) {                            // k_mom_accum
        const long long s = off2[(size_t)off[(size_t)c]], e = off2[(size_t)off[(size_t)c + 1]];
        const long long lo = s > q0 ? s : q0, hi = e < q0 + n ? e : q0 + n;
        if (lo >= hi) continue;
        if (hi < e && hi == q0 + n) inside = true;             // the pass ends inside this chain's rows
        long long owned = 0;
        for (int lane = 0; lane < 64; ++lane) {
          long long q = plan_moment_first_row(s, lo, lane);
          CHECK(q >= lo && q < lo + 64 && ((q - s) & 63) == lane);
          owned += plan_moment_rows_of_lane(s, lo, hi, lane);
          for (; q < hi; q += 64) {
            CHECK(desc[(size_t)(q - q0)] >= off[(size_t)c] && desc[(size_t)(q - q0)] < off[(size_t)c + 1]);
            read[(size_t)q] += 1;
            int& last = last_by_lane[(size_t)c * 64 + (size_t)lane];
            CHECK(last < (int)q);
            if (last >= 0) CHECK((int)q - last == 64);         // the lane's walk continues where the last pass left it
            last = (int)q;
          }
        }
        CHECK(owned == hi - lo);
      }
    }
    for (long long q = 0; q < n2; ++q) CHECK(written[(size_t)q] == 1 && read[(size_t)q] == 1);
    if (req == 7 && n2 > 7 * (long long)B) CHECK(inside);
  }
}

int main() {
  check_index_rule();
  check_per_pass();
  std::mt19937 rng(20261019u);
  const std::vector<long long> sizes = {1, 7, 63, 64, 65, 1000, 0};
  int lists = 0;
  for (int B : {1, 3, 40, 70})
    for (int max_first : {0, 1, 16, 70})
      for (int max_second : {0, 1, 12, 90}) {
        check_list(rng, B, max_first, max_second, sizes);
        ++lists;
      }
  printf("hostcheck_moments ok: %d lists, %lld assertions\n", lists, g_checks);
  return 0;
}
