// The host side of the four-spin (J-Q) terms (plan.hpp: plan_fourspin_*) under AddressSanitizer +
// UndefinedBehaviourSanitizer on the CPU (`make -C cgs_vmc_amd/csrc hostcheck_fourspin`, tests/test_fourspin.py).  It walks
//   * the validation of vmc_set_four_spin_terms: sites, couplings, the exchange sign, the request, and the three caps
//     (terms, distinct pairs, the 32-bit row index against exact 128-bit arithmetic);
//   * the pair table: pairs strictly ascending, at most 2 n_terms of them, every term's two indices naming its own two
//     unordered site pairs -- with duplicate pairs across terms and a pair that terms share in both orientations;
//   * the pass planner over lists built from random chains exactly as k_fs_count / k_fs_fill build them, into real arrays
//     of the planned size: for pass sizes 1, a prime, one larger than the list and the library's own, every row of the
//     list is written once, into the descriptor slot of its pass, and the fold's place of every row (the chain's offset
//     plus the rows before it) finds the descriptor of exactly that pair or term;
//   * the rows reserved for the result buffers that span the list.
#include "plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

static long long g_checks = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    ++g_checks;                                                                             \
    if (!(cond)) { fprintf(stderr, "hostcheck_fourspin: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

static int g_cases = 0;

static int check_terms(int N, long long B, const std::vector<int32_t>& ijkl, const std::vector<float>& q, int sign,
                       long long rows_per_pass, std::string* message = nullptr) {
  char msg[256];
  const int rc = plan_fourspin_check(N, B, (int)q.size(), ijkl.data(), q.data(), sign, rows_per_pass, msg, sizeof(msg));
  CHECK((rc == VMC_OK) == (msg[0] == 0));
  if (rc != VMC_OK) CHECK(strstr(msg, "vmc_set_four_spin_terms") == msg);      // the message names the entry
  if (message) *message = msg;
  ++g_cases;
  return rc;
}

static void check_validation() {
  const std::vector<int32_t> good = {0, 1, 2, 3, 4, 5, 6, 7};
  const std::vector<float> q2 = {1.f, -2.5f};
  CHECK(check_terms(8, 40, good, q2, 1, 0) == VMC_OK);
  CHECK(check_terms(8, 40, good, q2, -1, 7) == VMC_OK);
  CHECK(check_terms(8, 40, good, q2, 0, 0) == VMC_ERR_INVALID);
  CHECK(check_terms(8, 40, good, q2, 2, 0) == VMC_ERR_INVALID);
  CHECK(check_terms(8, 40, good, q2, 1, -1) == VMC_ERR_INVALID);
  CHECK(check_terms(7, 40, good, q2, 1, 0) == VMC_ERR_INVALID);                 // site 7 out of range
  CHECK(check_terms(8, 0, good, q2, 1, 0) == VMC_ERR_INVALID);
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      if (a == b) continue;
      std::vector<int32_t> twice = good;
      twice[4 + (size_t)a] = twice[4 + (size_t)b];                              // term 1 names a site twice
      std::string msg;
      CHECK(check_terms(8, 40, twice, q2, 1, 0, &msg) == VMC_ERR_INVALID);
      CHECK(msg.find("term 1") != std::string::npos);
    }
  std::vector<int32_t> negative = good;
  negative[2] = -1;
  CHECK(check_terms(8, 40, negative, q2, 1, 0) == VMC_ERR_INVALID);
  for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                    std::numeric_limits<float>::quiet_NaN()}) {
    std::string msg;
    CHECK(check_terms(8, 40, good, {1.f, bad}, 1, 0, &msg) == VMC_ERR_INVALID);
    CHECK(msg.find("term 1") != std::string::npos);
  }
  char msg[64];
  CHECK(plan_fourspin_check(8, 40, 2, nullptr, q2.data(), 1, 0, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_fourspin_check(8, 40, 2, good.data(), nullptr, 1, 0, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_fourspin_check(8, 40, 0, good.data(), q2.data(), 1, 0, msg, sizeof(msg)) == VMC_ERR_INVALID);
  g_cases += 3;
}

// n_terms terms over N sites: term t takes the t-th pair of even sites and the t-th pair of odd sites (i-major lists,
// i < j), so its four sites are distinct and, while n_terms does not exceed the pairs of N / 2 sites, so are all the
// 2 n_terms pairs; beyond that the lists start over
static std::vector<int32_t> many_terms(int N, int n_terms) {
  std::vector<int32_t> out;
  out.reserve((size_t)n_terms * 4);
  const int half = N / 2;
  int i = 0, j = 1;
  for (int t = 0; t < n_terms; ++t) {
    out.insert(out.end(), {2 * i, 2 * j, 2 * i + 1, 2 * j + 1});
    if (++j >= half) { ++i; j = i + 1; }
    if (i >= half - 1) { i = 0; j = 1; }
  }
  return out;
}

static void check_caps() {
  std::string msg;
  // the term cap
  {
    const int n = PLAN_FOURSPIN_MAX_TERMS + 1;
    std::vector<int32_t> ijkl;
    for (int t = 0; t < n; ++t) ijkl.insert(ijkl.end(), {0, 1, 2, 3});
    CHECK(check_terms(8, 1, ijkl, std::vector<float>((size_t)n, 1.f), 1, 0, &msg) == VMC_ERR_UNSUPPORTED);
    CHECK(msg.find("65536") != std::string::npos);
    ijkl.resize((size_t)PLAN_FOURSPIN_MAX_TERMS * 4);
    CHECK(check_terms(8, 1, ijkl, std::vector<float>((size_t)PLAN_FOURSPIN_MAX_TERMS, 1.f), 1, 0) == VMC_OK);
  }
  // the pair cap: 2,049 terms of all-distinct pairs are 4,098 pairs, 2,048 terms exactly the cap
  {
    const std::vector<int32_t> over = many_terms(200, PLAN_FOURSPIN_MAX_PAIRS / 2 + 1);
    CHECK(plan_fourspin_pairs(PLAN_FOURSPIN_MAX_PAIRS / 2 + 1, over.data()).n_pairs() == PLAN_FOURSPIN_MAX_PAIRS + 2);
    CHECK(check_terms(200, 1, over, std::vector<float>(over.size() / 4, 1.f), 1, 0, &msg) == VMC_ERR_UNSUPPORTED);
    CHECK(msg.find("4096") != std::string::npos);
    const std::vector<int32_t> at = many_terms(200, PLAN_FOURSPIN_MAX_PAIRS / 2);
    CHECK(plan_fourspin_pairs(PLAN_FOURSPIN_MAX_PAIRS / 2, at.data()).n_pairs() == PLAN_FOURSPIN_MAX_PAIRS);
    CHECK(check_terms(200, 1, at, std::vector<float>(at.size() / 4, 1.f), 1, 0) == VMC_OK);
    CHECK(plan_fourspin_fold_lds(PLAN_FOURSPIN_MAX_PAIRS) <= (size_t)64 * 1024);     // one workgroup's LDS
  }
  // the 32-bit row index: B (n_pairs + n_terms) <= 2^31 - 1, against exact arithmetic
  {
    const std::vector<int32_t> ijkl = many_terms(100, 200);
    const std::vector<float> q(200, 1.f);
    const long long items = plan_fourspin_pairs(200, ijkl.data()).n_pairs() + 200;
    CHECK(items == 600);
    for (long long B : {1LL, 4096LL, 3579139LL, 3579140LL, 1LL << 30, 0x7fffffffLL}) {
      const bool exact = (__int128)B * items <= (__int128)0x7fffffff;
      CHECK((check_terms(100, B, ijkl, q, 1, 0, &msg) == VMC_OK) == exact);
      if (!exact) CHECK(msg.find("32-bit row index") != std::string::npos);
    }
  }
}

static void check_table_of(int N, const std::vector<int32_t>& ijkl) {
  const int n_terms = (int)(ijkl.size() / 4);
  const FourSpinTable t = plan_fourspin_pairs(n_terms, ijkl.data());
  const int n_pairs = t.n_pairs();
  CHECK(n_pairs >= 2 && n_pairs <= 2 * n_terms);
  CHECK((int)t.term_pairs.size() == 2 * n_terms);
  for (int p = 0; p < n_pairs; ++p) {
    const int32_t a = t.pairs[2 * (size_t)p], b = t.pairs[2 * (size_t)p + 1];
    CHECK(a >= 0 && a < b && b < N);
    if (p > 0) {
      const int32_t pa = t.pairs[2 * (size_t)p - 2], pb = t.pairs[2 * (size_t)p - 1];
      CHECK(pa < a || (pa == a && pb < b));                                     // strictly ascending: no pair twice
    }
  }
  std::vector<int> used((size_t)n_pairs, 0);
  for (int k = 0; k < 2 * n_terms; ++k) {
    const int32_t p = t.term_pairs[(size_t)k];
    CHECK(p >= 0 && p < n_pairs);
    const int32_t a = ijkl[2 * (size_t)k], b = ijkl[2 * (size_t)k + 1];
    CHECK(t.pairs[2 * (size_t)p] == (a < b ? a : b) && t.pairs[2 * (size_t)p + 1] == (a < b ? b : a));
    used[(size_t)p] += 1;
  }
  for (int p = 0; p < n_pairs; ++p) CHECK(used[(size_t)p] >= 1);
  for (int k = 0; k < n_terms; ++k) CHECK(t.term_pairs[2 * (size_t)k] != t.term_pairs[2 * (size_t)k + 1]);
  ++g_cases;
}

static void check_tables(std::mt19937& rng) {
  // the J-Q chain of 8 sites: 8 terms, every bond in two terms -- 8 pairs
  std::vector<int32_t> chain;
  for (int i = 0; i < 8; ++i) chain.insert(chain.end(), {i, (i + 1) % 8, (i + 2) % 8, (i + 3) % 8});
  check_table_of(8, chain);
  CHECK(plan_fourspin_pairs(8, chain.data()).n_pairs() == 8);
  // a pair shared in both orientations, and as the first pair of one term and the second of another
  const std::vector<int32_t> both = {0, 1, 2, 3, 1, 0, 4, 5, 6, 7, 1, 0, 3, 2, 0, 1};
  check_table_of(8, both);
  CHECK(plan_fourspin_pairs(4, both.data()).n_pairs() == 4);                    // (0,1) (2,3) (4,5) (6,7)
  const FourSpinTable t = plan_fourspin_pairs(4, both.data());
  CHECK(t.term_pairs[0] == t.term_pairs[2] && t.term_pairs[2] == t.term_pairs[5] && t.term_pairs[5] == t.term_pairs[7]);
  CHECK(t.term_pairs[1] == t.term_pairs[6]);
  // the same term twice
  check_table_of(8, {0, 1, 2, 3, 0, 1, 2, 3});
  for (int trial = 0; trial < 40; ++trial) {
    const int N = 4 + (int)(rng() % 30u), n_terms = 1 + (int)(rng() % 90u);
    std::vector<int32_t> ijkl;
    for (int k = 0; k < n_terms; ++k) {
      int32_t s[4];
      for (int a = 0; a < 4; ++a) {
        bool fresh;
        do {
          s[a] = (int32_t)(rng() % (unsigned)N);
          fresh = true;
          for (int b = 0; b < a; ++b) fresh = fresh && s[b] != s[a];
        } while (!fresh);
      }
      ijkl.insert(ijkl.end(), s, s + 4);
    }
    CHECK(check_terms(N, 40, ijkl, std::vector<float>((size_t)n_terms, 0.5f), -1, 0) == VMC_OK);
    check_table_of(N, ijkl);
  }
}

static void check_per_pass() {
  const long long totals[] = {0, 1, 7, 64, 65, 1000, 1LL << 24, (1LL << 24) + 1, 0x7fffffffLL};
  const long long reqs[] = {0, 1, 7, 64, 1000, 1LL << 30};
  const long long limits[] = {0, 1, 5, 1LL << 20, 1LL << 40};
  for (long long total : totals)
    for (long long req : reqs)
      for (long long lim : limits) {
        const long long per = plan_list_per_pass(total, req, lim);
        CHECK(per >= 1 && per <= PLAN_MEASURE_ROW_BUDGET);
        if (lim > 0) CHECK(per <= lim);
        if (req > 0) CHECK(per <= req);
        if (total > 0) CHECK(per <= total);
        CHECK((long long)(int)per == per);
        const long long passes = plan_measure_passes(total, (int)per);
        CHECK(passes * per >= total && (passes == 0 || (passes - 1) * per < total));
        ++g_cases;
      }
  CHECK(plan_list_per_pass(-1, 0, 0) == -1 && plan_list_per_pass(5, -1, 0) == -1 && plan_list_per_pass(5, 0, -1) == -1);
}

// the rows reserved for the result buffers: never fewer than the list, never more than the a-priori maximum, the maximum
// at once where it fits the budget, at least doubling beyond it
static void check_result_rows() {
  for (long long B : {1LL, 40LL, 4096LL, 1LL << 20})
    for (long long items : {3LL, 68LL, 400LL, 2000LL}) {
      const long long most = B * items;
      long long held = 0;
      int grown = 0;
      for (long long total : {0LL, 1LL, most / 7, most / 2, most / 2 + 1, most - 1, most, most / 3}) {
        const long long rows = plan_fourspin_result_rows(B, items / 2, items - items / 2, total, held);
        CHECK(rows >= total && rows >= held && rows <= (most > held ? most : held));
        if (rows > held) {
          ++grown;
          CHECK(most <= PLAN_FOURSPIN_RESULT_ROWS ? rows == most : (rows >= 2 * held || rows == most));
        }
        held = rows;
        ++g_cases;
      }
      if (most <= PLAN_FOURSPIN_RESULT_ROWS) CHECK(grown == 1);                 // one allocation for good
      CHECK(grown <= 6);
    }
  CHECK(plan_fourspin_result_rows(4096, 200, 200, 622830, 0) == 4096LL * 400);   // config 3's shape
}

// B random chains at Sz = 0 (with a Neel chain and, where the terms allow, one without an active term), the list as the
// kernels build it, and the passes of every size of interest
static void check_list(std::mt19937& rng, int N, int B, const std::vector<int32_t>& ijkl) {
  const int n_terms = (int)(ijkl.size() / 4);
  const FourSpinTable t = plan_fourspin_pairs(n_terms, ijkl.data());
  const int n_pairs = t.n_pairs();
  std::vector<int> x((size_t)B * N);
  for (int c = 0; c < B; ++c) {
    int* row = x.data() + (size_t)c * N;
    for (int i = 0; i < N; ++i) row[i] = (i % 2 == 0) ? 1 : -1;                 // the Neel configuration
    if (c > 0) std::shuffle(row, row + N, rng);
    if (c == 1) for (int i = 0; i < N; ++i) row[i] = i < N / 2 ? 1 : -1;         // a domain wall: few active terms
  }
  auto anti = [&](int c, int p) { return x[(size_t)c * N + t.pairs[2 * (size_t)p]] != x[(size_t)c * N + t.pairs[2 * (size_t)p + 1]]; };
  auto active = [&](int c, int k) { return anti(c, t.term_pairs[2 * (size_t)k]) && anti(c, t.term_pairs[2 * (size_t)k + 1]); };
  std::vector<int> off((size_t)B + 1, 0);                                        // k_fs_count, k_fs_scan
  for (int c = 0; c < B; ++c) {
    int n = 0;
    for (int p = 0; p < n_pairs; ++p) n += anti(c, p);
    for (int k = 0; k < n_terms; ++k) n += active(c, k);
    off[(size_t)c + 1] = off[(size_t)c] + n;
  }
  const long long total = off[(size_t)B];
  CHECK(total <= (long long)B * (n_pairs + n_terms));
  for (long long req : {1LL, 7LL, 61LL, total + 5, 0LL}) {
    const long long per = plan_list_per_pass(total, req, 0);
    std::vector<int> written((size_t)total, 0), code_of((size_t)total, -1), chain_of((size_t)total, -1);
    bool inside = false;
    for (long long q0 = 0; q0 < total; q0 += per) {
      const int n = (int)(total - q0 < per ? total - q0 : per);
      std::vector<int> desc_chain((size_t)per, -1), desc_code((size_t)per, -1);    // the pass's descriptors, as reserved
      for (int c = 0; c < B; ++c) {                                              // k_fs_fill
        long long q = off[(size_t)c];
        if (off[(size_t)c + 1] <= q0 || q >= q0 + n) continue;
        if (off[(size_t)c + 1] > q0 + n) inside = true;                          // the pass ends inside this chain's rows
        for (int code = 0; code < n_pairs + n_terms; ++code) {
          const bool emit = code < n_pairs ? anti(c, code) : active(c, code - n_pairs);
          if (!emit) continue;
          if (q >= q0 && q < q0 + n) {
            CHECK(desc_chain[(size_t)(q - q0)] == -1);
            desc_chain[(size_t)(q - q0)] = c; desc_code[(size_t)(q - q0)] = code;
            written[(size_t)q] += 1; chain_of[(size_t)q] = c; code_of[(size_t)q] = code;
          }
          ++q;
        }
        CHECK(q == off[(size_t)c + 1]);
      }
      for (int k = 0; k < n; ++k) CHECK(desc_chain[(size_t)k] >= 0 && desc_code[(size_t)k] >= 0);
    }
    for (long long q = 0; q < total; ++q) CHECK(written[(size_t)q] == 1);
    for (int c = 0; c < B; ++c) {                                                // k_fs_fold's places
      long long q = off[(size_t)c];
      for (int p = 0; p < n_pairs; ++p)
        if (anti(c, p)) { CHECK(chain_of[(size_t)q] == c && code_of[(size_t)q] == p); ++q; }
      for (int k = 0; k < n_terms; ++k)
        if (active(c, k)) { CHECK(chain_of[(size_t)q] == c && code_of[(size_t)q] == n_pairs + k); ++q; }
      CHECK(q == off[(size_t)c + 1]);
    }
    if (req == 7 && B > 1 && total > 7LL * B) CHECK(inside);
    ++g_cases;
  }
}

int main() {
  std::mt19937 rng(20261021u);
  check_validation();
  check_caps();
  check_tables(rng);
  check_per_pass();
  check_result_rows();
  for (int N : {8, 12, 66, 130}) {
    std::vector<int32_t> chain;
    for (int i = 0; i < N; ++i) chain.insert(chain.end(), {i, (i + 1) % N, (i + 2) % N, (i + 3) % N});
    for (int B : {1, 5, 17}) check_list(rng, N, B, chain);
  }
  check_list(rng, 16, 40, many_terms(16, 34));
  printf("hostcheck_fourspin ok: %d cases, %lld assertions\n", g_cases, g_checks);
  return 0;
}
