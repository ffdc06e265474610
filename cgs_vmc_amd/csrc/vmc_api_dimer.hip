// Dimer-dimer correlations (extension, no reference counterpart): vmc_dimer_correlations over the ctx's current chains.
// Per bond a = (i, j): bond_sum = sum_c bond(a; x_c); per ordered pair of bonds (a, b): dd_sum = sum_c dd(a, b; x_c), the
// local value of (S_i . S_j)(S_k . S_l) (dimer.hip states both); the host forms <A B> ~ dd_sum / B, <A> ~ bond_sum / B
// and the connected part.
//
// Phase 1: B rows per bond, the single exchanges (k_dimer_rows1), through the family's own full forward
// (rows_forward_device, vmc_api.hip) in as many passes as the row buffer of vmc_amplitude takes (fewer bonds per pass
// where pairs_per_pass asks for fewer); their ln|psi| and signs
// stay in the ctx's [n_bonds][B] buffers.  Phase 2: passes of pairs, B rows per pair, the double exchanges
// (k_dimer_rows2), forwarded the same way and folded per pair (k_dimer_fold) against phase 1's buffers and the chains'
// cached ln|psi| and signs.  (n_bonds + n_pairs) B full forwards in all.  The call is a pure measurement: chains, step
// counter, accumulators, the Hamiltonian and the validity of the amplitude and activation caches are as before when it
// returns.
#include "vmc_ctx.hpp"

using namespace vmcapi;

namespace {

int dimer_reserve(vmc_ctx* c, long long n_bonds, long long n_pairs) {
  if (n_bonds <= c->dimer_cap_bonds && n_pairs <= c->dimer_cap_pairs) return VMC_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_bonds < c->dimer_cap_bonds) n_bonds = c->dimer_cap_bonds;
  if (n_pairs < c->dimer_cap_pairs) n_pairs = c->dimer_cap_pairs;
  for (void* q : {(void*)c->dimer_bonds, (void*)c->dimer_pairs, (void*)c->dimer_logit, (void*)c->dimer_sign,
                  (void*)c->dimer_out}) if (q) hipFree(q);
  c->dimer_bonds = nullptr; c->dimer_pairs = nullptr; c->dimer_logit = nullptr; c->dimer_sign = nullptr;
  c->dimer_out = nullptr; c->dimer_cap_bonds = 0; c->dimer_cap_pairs = 0;
  HIPCHK(c, dalloc(&c->dimer_bonds, n_bonds));
  HIPCHK(c, dalloc(&c->dimer_pairs, n_pairs));
  HIPCHK(c, dalloc(&c->dimer_logit, n_bonds * c->B));
  if (c->sgn) HIPCHK(c, dalloc(&c->dimer_sign, n_bonds * c->B));
  HIPCHK(c, dalloc(&c->dimer_out, n_bonds + n_pairs));
  c->dimer_cap_bonds = n_bonds; c->dimer_cap_pairs = n_pairs;
  return VMC_OK;
}

// bonds [a0, a0 + n): rows, forward into the [n_bonds][B] buffers
int dimer_single_pass(vmc_ctx* c, int which, long long a0, int n) {
  const long long rows = (long long)n * c->B;
  {
    Timer t(c, "dimer_rows");
    HIPCHK(c, launch_dimer_rows1(c->stream, c->configs, c->dimer_bonds + a0, c->B, c->N, n, c->num_cus, c->tmp_cfg));
  }
  Timer t(c, "dimer_forward");
  PROPAGATE(rows_forward_device(c, which, c->tmp_cfg, rows, c->dimer_logit + a0 * c->B,
                                c->sgn ? c->dimer_sign + a0 * c->B : c->tmp_sign));
  return VMC_OK;
}

// pairs [p0, p0 + n): rows, forward, fold
int dimer_double_pass(vmc_ctx* c, int which, long long p0, int n, double* dd_out) {
  const ParamSet& p = c->ps[which];
  const long long rows = (long long)n * c->B;
  {
    Timer t(c, "dimer_rows");
    HIPCHK(c, launch_dimer_rows2(c->stream, c->configs, c->dimer_bonds, c->dimer_pairs + p0, c->B, c->N, n, c->num_cus,
                                 c->tmp_cfg));
  }
  {
    Timer t(c, "dimer_forward");
    PROPAGATE(rows_forward_device(c, which, c->tmp_cfg, rows, c->tmp_out, c->tmp_sign));
  }
  Timer t(c, "dimer_fold");
  HIPCHK(c, launch_dimer_fold(c->stream, c->configs, c->dimer_bonds, c->dimer_pairs + p0, p.logit,
                              c->sgn ? p.sign : nullptr, c->dimer_logit, c->sgn ? c->dimer_sign : nullptr, c->tmp_out,
                              c->sgn ? c->tmp_sign : nullptr, c->B, c->N, n, dd_out + p0));
  return VMC_OK;
}

}  // namespace

extern "C" {

int vmc_dimer_correlations(vmc_ctx* c, int which, int32_t n_bonds, const int32_t* bonds, int32_t n_pairs,
                           const int32_t* pairs, int32_t pairs_per_pass, double* bond_sum, double* dd_sum) {
  ENTER(c);
  REFUSE_PRODUCT(c, "vmc_dimer_correlations");
  REFUSE_COMPOSED(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  if (n_bonds < 1 || !bonds || n_pairs < 0 || (n_pairs > 0 && !pairs) || pairs_per_pass < 0)
    return fail(c, VMC_ERR_INVALID, "bad bond / pair arguments");
  std::vector<int2> hb((size_t)n_bonds), hp((size_t)n_pairs);
  for (int a = 0; a < n_bonds; ++a) {
    const int i = bonds[2 * a], j = bonds[2 * a + 1];
    if (i < 0 || j < 0 || i >= c->N || j >= c->N || i == j) {
      char msg[128];
      snprintf(msg, sizeof(msg), "bond %d = (%d, %d): two distinct sites in 0 .. %d required", a, i, j, c->N - 1);
      return fail(c, VMC_ERR_INVALID, msg);
    }
    hb[(size_t)a] = make_int2(i, j);
  }
  for (int p = 0; p < n_pairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || b < 0 || a >= n_bonds || b >= n_bonds) {
      char msg[128];
      snprintf(msg, sizeof(msg), "pair %d = (%d, %d): bond indices in 0 .. %d required", p, a, b, n_bonds - 1);
      return fail(c, VMC_ERR_INVALID, msg);
    }
    hp[(size_t)p] = make_int2(a, b);
  }
  if (!c->sgn && c->oact != VMC_ACT_EXP_)
    return fail(c, VMC_ERR_UNSUPPORTED, "vmc_dimer_correlations needs the exp output activation (the logit is ln psi only then)");
  const long long row_limit = plan_dimer_row_limit(c->N, c->Hp);
  const int per1 = plan_dimer_pairs_per_pass(c->B, n_bonds, pairs_per_pass, row_limit);    // (a request splits both phases)
  const int per2 = n_pairs > 0 ? plan_dimer_pairs_per_pass(c->B, n_pairs, pairs_per_pass, row_limit) : 0;
  if (per1 < 1 || (n_pairs > 0 && per2 < 1) || !plan_dimer_bond_rows_ok(c->B, n_bonds))
    return fail(c, VMC_ERR_UNSUPPORTED, "batch_size x bonds does not fit the 32-bit row index");
  const bool cache_was[2] = {c->ps[0].cache_valid, c->ps[1].cache_valid};
  const bool acts_were = c->acts_valid;
  int rc = ensure_cache(c, which);           // ln|psi(x_c)| and the signs, as the local energies take them
  if (rc == VMC_OK) rc = dimer_reserve(c, n_bonds, n_pairs);
  if (rc == VMC_OK) rc = grow_tmp(c, (long long)(per1 > per2 ? per1 : per2) * c->B);
  if (rc == VMC_OK) {
    hipError_t e = hipMemcpyAsync(c->dimer_bonds, hb.data(), hb.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_pairs > 0)
      e = hipMemcpyAsync(c->dimer_pairs, hp.data(), hp.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  for (long long a0 = 0; a0 < n_bonds && rc == VMC_OK; a0 += per1) {
    const int n = (int)(n_bonds - a0 < per1 ? n_bonds - a0 : per1);
    rc = dimer_single_pass(c, which, a0, n);
  }
  if (rc == VMC_OK) {
    const ParamSet& p = c->ps[which];
    Timer t(c, "dimer_fold");
    hipError_t e = launch_dimer_bond_fold(c->stream, c->configs, c->dimer_bonds, p.logit, c->sgn ? p.sign : nullptr,
                                          c->dimer_logit, c->sgn ? c->dimer_sign : nullptr, c->B, c->N, n_bonds,
                                          c->dimer_out);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("k_dimer_bond_fold: ") + hipGetErrorString(e));
  }
  for (long long p0 = 0; p0 < n_pairs && rc == VMC_OK; p0 += per2) {
    const int n = (int)(n_pairs - p0 < per2 ? n_pairs - p0 : per2);
    rc = dimer_double_pass(c, which, p0, n, c->dimer_out + n_bonds);
  }
  std::vector<double> out(rc == VMC_OK ? (size_t)n_bonds + (size_t)n_pairs : 0);
  if (rc == VMC_OK) {
    hipError_t e = hipMemcpyAsync(out.data(), c->dimer_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("vmc_dimer_correlations read-back: ") + hipGetErrorString(e));
  } else {
    hipStreamSynchronize(c->stream);         // (the two lists are the sources of asynchronous copies)
  }
  // what was not valid before is not vouched for now either: the next consumer fills it exactly as it would have
  for (int w = 0; w < 2; ++w) if (!cache_was[w]) c->ps[w].cache_valid = false;
  if (!acts_were) c->acts_valid = false;
  if (rc != VMC_OK) return rc;
  for (int a = 0; a < n_bonds && bond_sum; ++a) bond_sum[a] = out[(size_t)a];
  for (int p = 0; p < n_pairs && dd_sum; ++p) dd_sum[p] = out[(size_t)n_bonds + (size_t)p];
  return VMC_OK;
}

}  // extern "C"
