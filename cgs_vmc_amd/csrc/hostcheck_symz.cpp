// The planners of the symmetrized ctx (plan.hpp: plan_symz_*) under AddressSanitizer + UndefinedBehaviourSanitizer on the
// CPU (`make -C cgs_vmc_amd/csrc hostcheck_symz`, tests/test_symmetrized.py):
//   * plan_symz_check: which base is taken (the product's factor types), a composite or an owned base refused, the row
//     rule base_B = batch_size x n_ops with both numbers in the message, 1 <= n_ops <= 1024, bijections, flips in {0, 1},
//     finite characters that are not all zero -- and the order of the refusals (type before state before arguments);
//   * the grids cover every chain and overshoot by less than one workgroup;
//   * the structural-zero rule: exact cancellation fires, the fp64 sum's worst rounding (2^-43 A) fires, the fp32 logits'
//     noise (2^-24 A) never does, NaN counts as a zero (no chain may sit on it).
#include "plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static long long g_checks = 0, g_cases = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    ++g_checks;                                                                             \
    if (!(cond)) { fprintf(stderr, "hostcheck_symz: %s failed at line %d\n", #cond, __LINE__); exit(1); } \
  } while (0)

static std::vector<int32_t> translations(int N, int n_ops) {
  std::vector<int32_t> p((size_t)n_ops * N);
  for (int k = 0; k < n_ops; ++k)
    for (int i = 0; i < N; ++i) p[(size_t)k * N + i] = (i + k) % N;
  return p;
}

static int check(int ansatz, int oact, bool composite, bool owned, long long base_B, int N, long long B, long long n_ops,
                 const int32_t* perms, const uint8_t* flips, const double* chi, char* msg, size_t len) {
  ++g_cases;
  return plan_symz_check(ansatz, oact, composite, owned, base_B, N, B, n_ops, perms, flips, chi, msg, len);
}

static void base_types() {
  const int N = 8, n_ops = 8, B = 5;
  const std::vector<int32_t> p = translations(N, n_ops);
  const std::vector<double> chi((size_t)n_ops, 1.0);
  char msg[320];
  for (int ansatz = 0; ansatz <= VMC_ANSATZ_SYMMETRIZED; ++ansatz)
    for (int oact = 0; oact <= 6; ++oact) {
      const int rc = check(ansatz, oact, false, false, (long long)B * n_ops, N, B, n_ops, p.data(), nullptr, chi.data(), msg, sizeof(msg));
      const bool dense = ansatz == VMC_ANSATZ_FULLY_CONNECTED || ansatz == VMC_ANSATZ_RBM;
      const bool table = ansatz == VMC_ANSATZ_PBDG || ansatz == VMC_ANSATZ_ED_VECTOR;
      const bool ok = table || (dense && oact == VMC_ACT_EXP);
      CHECK(rc == (ok ? VMC_OK : VMC_ERR_UNSUPPORTED));
      CHECK((msg[0] == 0) == ok);
      // a composite base is refused whatever else holds; an owned one of a taken type with VMC_ERR_STATE
      CHECK(check(ansatz, oact, true, false, (long long)B * n_ops, N, B, n_ops, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
      CHECK(check(ansatz, oact, false, true, (long long)B * n_ops, N, B, n_ops, p.data(), nullptr, chi.data(), msg, sizeof(msg)) ==
            (ok ? VMC_ERR_STATE : VMC_ERR_UNSUPPORTED));
    }
}

static void arguments() {
  const int N = 8;
  char msg[320];
  const std::vector<int32_t> p = translations(N, 8);
  std::vector<double> chi(8, 1.0);
  const int fc = VMC_ANSATZ_FULLY_CONNECTED, ex = VMC_ACT_EXP;
  // the row rule names both numbers
  CHECK(check(fc, ex, false, false, 41, N, 5, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(strstr(msg, "41") && strstr(msg, "40"));
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_OK);
  CHECK(check(fc, ex, false, false, 0, N, 0, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  // n_ops: 1 .. 1024
  CHECK(check(fc, ex, false, false, 0, N, 5, 0, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  {
    const int big = PLAN_SYMZ_MAX_OPS + 1;
    std::vector<int32_t> pb((size_t)big * N);
    for (int k = 0; k < big; ++k) for (int i = 0; i < N; ++i) pb[(size_t)k * N + i] = (i + k) % N;
    std::vector<double> cb((size_t)big, 1.0);
    CHECK(check(fc, ex, false, false, 2LL * big, N, 2, big, pb.data(), nullptr, cb.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(check(fc, ex, false, false, 2LL * (big - 1), N, 2, big - 1, pb.data(), nullptr, cb.data(), msg, sizeof(msg)) == VMC_OK);
  }
  CHECK(check(fc, ex, false, false, 5, N, 5, 1, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_OK);
  // nulls
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, nullptr, nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), nullptr, nullptr, msg, sizeof(msg)) == VMC_ERR_INVALID);
  // a perm that is no bijection, an entry out of range, a flip above 1: the op is named
  {
    std::vector<int32_t> q = p;
    q[3 * N + 2] = q[3 * N + 1];
    CHECK(check(fc, ex, false, false, 40, N, 5, 8, q.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(strstr(msg, "op 3"));
    q = p; q[5 * N] = N;
    CHECK(check(fc, ex, false, false, 40, N, 5, 8, q.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(strstr(msg, "op 5"));
    std::vector<uint8_t> f(8, 0);
    f[6] = 2;
    CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), f.data(), chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(strstr(msg, "op 6"));
    f[6] = 1;
    CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), f.data(), chi.data(), msg, sizeof(msg)) == VMC_OK);
  }
  // characters: finite, not all zero; zeros among them are fine
  chi[2] = NAN;
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(strstr(msg, "character 2"));
  chi[2] = INFINITY;
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  chi.assign(8, 0.0);
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  chi[7] = -1.0;
  CHECK(check(fc, ex, false, false, 40, N, 5, 8, p.data(), nullptr, chi.data(), msg, sizeof(msg)) == VMC_OK);
}

static void grids() {
  for (long long B : {1LL, 3LL, 4LL, 5LL, 63LL, 64LL, 255LL, 256LL, 257LL, 4096LL, 100001LL}) {
    ++g_cases;
    CHECK((long long)plan_symz_chain_blocks(B) * PLAN_SYMZ_THREADS >= B);
    CHECK(((long long)plan_symz_chain_blocks(B) - 1) * PLAN_SYMZ_THREADS < B);
    CHECK((long long)plan_symz_wave_grid(B) * PLAN_SYMZ_CHAINS_PER_WG >= B);
    CHECK(((long long)plan_symz_wave_grid(B) - 1) * PLAN_SYMZ_CHAINS_PER_WG < B);
  }
  CHECK(plan_symz_acc_floats(577) == 2 * 577 + 8);
  CHECK(PLAN_SYMZ_THREADS % 64 == 0);
}

static void zero_rule() {
  ++g_cases;
  CHECK(PLAN_SYMZ_ZERO == ldexp(1.0, PLAN_SYMZ_ZERO_LOG2));
  for (double A : {1.0, 2.0, 1024.0, 1e-30, 1e30}) {
    CHECK(plan_symz_is_zero(0.0, A));
    CHECK(plan_symz_is_zero(-0.0, A));
    CHECK(plan_symz_is_zero(ldexp(A, -43), A));          // the fp64 sum's worst rounding over 1,024 terms
    CHECK(plan_symz_is_zero(-ldexp(A, -43), A));
    CHECK(plan_symz_is_zero(ldexp(A, -40), A));          // the bound itself belongs to the zero
    CHECK(!plan_symz_is_zero(ldexp(A, -39), A));
    CHECK(!plan_symz_is_zero(ldexp(A, -24), A));         // the fp32 logits' noise: a near miss is no zero
    CHECK(!plan_symz_is_zero(-ldexp(A, -24), A));
    CHECK(!plan_symz_is_zero(A, A));
    CHECK(plan_symz_is_zero(NAN, A));
  }
  CHECK(plan_symz_is_zero(0.0, 0.0));
}

int main() {
  base_types();
  arguments();
  grids();
  zero_rule();
  printf("hostcheck_symz ok: %lld cases, %lld assertions\n", g_cases, g_checks);
  return 0;
}
