// Spin-correlation measurement (extension, no reference counterpart): vmc_pair_correlations.  Per pair (i, j) over the
// ctx's current chains: zz = sum_c s_i s_j and ex = sum_c [s_i s_j < 0] psi(swap_ij x_c) / psi(x_c); the host forms
// <S_i . S_j> = (zz / 4 + ex / 2) / B.
//
// The ratios are the rows the local energies already evaluate: a pass of pairs is a bond set of its own (j_x = 2, so that
// val is the bare ratio; j_z = 0) that takes the place of the Hamiltonian's five buffers + n_bonds in the ctx while
// ensure_list and the family's row launch (connected_rows_device) run, and is swapped out again afterwards.  The fold per
// pair over chains is corr.hip.  The call is a pure measurement: chains, step counter, accumulators, the Hamiltonian's
// set and the validity of the amplitude caches are as before when it returns.
#include "vmc_ctx.hpp"

using namespace vmcapi;

namespace {

struct BondSet {
  int n_bonds; int2* bonds; float *half_jx, *quarter_jz; int2* rowinfo; float* val;
};

BondSet current_set(const vmc_ctx* c) { return BondSet{c->n_bonds, c->bonds, c->half_jx, c->quarter_jz, c->rowinfo, c->val}; }

// cnt / diag / off / the list belong to whichever set was counted last: nothing of them survives a swap
void install_set(vmc_ctx* c, const BondSet& s) {
  c->n_bonds = s.n_bonds; c->bonds = s.bonds; c->half_jx = s.half_jx; c->quarter_jz = s.quarter_jz;
  c->rowinfo = s.rowinfo; c->val = s.val;
  c->bonds_epoch += 1;        // (the bond-difference tables of the row kernel belong to the list they were built from)
  c->list_valid = false;
  c->cnt_valid = false;
}

int corr_reserve(vmc_ctx* c, long long per, long long n_pairs) {
  if (n_pairs > c->corr_cap_all) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->corr_pairs) hipFree(c->corr_pairs);
    if (c->corr_out) hipFree(c->corr_out);
    c->corr_pairs = nullptr; c->corr_out = nullptr; c->corr_cap_all = 0;
    HIPCHK(c, dalloc(&c->corr_pairs, n_pairs));
    HIPCHK(c, dalloc(&c->corr_out, 2 * n_pairs));
    c->corr_cap_all = n_pairs;
  }
  if (per > c->corr_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (void* q : {(void*)c->corr_hx, (void*)c->corr_qz, (void*)c->corr_rowinfo, (void*)c->corr_val, (void*)c->corr_dense})
      if (q) hipFree(q);
    c->corr_hx = c->corr_qz = c->corr_val = c->corr_dense = nullptr; c->corr_rowinfo = nullptr; c->corr_cap = 0;
    HIPCHK(c, dalloc(&c->corr_hx, per)); HIPCHK(c, dalloc(&c->corr_qz, per));
    HIPCHK(c, dalloc(&c->corr_rowinfo, (long long)c->B * per));
    HIPCHK(c, dalloc(&c->corr_val, (long long)c->B * per));
    HIPCHK(c, dalloc(&c->corr_dense, (long long)c->B * per));
    HIPCHK(c, launch_fill(c->stream, c->corr_hx, 1.f, (int)per));      // 0.5 j_x with j_x = 2
    HIPCHK(c, hipMemsetAsync(c->corr_qz, 0, (size_t)per * sizeof(float), c->stream));
    c->corr_cap = per;
  }
  return VMC_OK;
}

// pairs [k0, k0 + n) with their set installed: list, rows, fold
int corr_pass(vmc_ctx* c, int which, long long k0, int n, long long n_pairs) {
  PROPAGATE(ensure_list(c));
  PROPAGATE(connected_rows_device(c, which, false));
  Timer t(c, "corr_fold");
  HIPCHK(c, launch_pair_fold(c->stream, c->configs, c->bonds, c->rowinfo, c->val, c->off + c->B, c->B, c->N, n,
                             c->num_cus, c->corr_dense, c->corr_out + k0, c->corr_out + n_pairs + k0));
  return VMC_OK;
}

}  // namespace

extern "C" {

int vmc_pair_correlations(vmc_ctx* c, int which, int32_t n_pairs, const int32_t* ij, int32_t pairs_per_pass,
                          double* zz_sum, double* ex_sum) {
  ENTER(c);
  REFUSE_PRODUCT(c, "vmc_pair_correlations");
  REFUSE_COMPOSED(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  if (n_pairs < 1 || !ij || pairs_per_pass < 0) return fail(c, VMC_ERR_INVALID, "bad pair arguments");
  std::vector<int2> pairs((size_t)n_pairs);
  for (int k = 0; k < n_pairs; ++k) {
    const int i = ij[2 * k], j = ij[2 * k + 1];
    if (i < 0 || j < 0 || i >= c->N || j >= c->N || i == j)
      return fail(c, VMC_ERR_INVALID, "pair site index out of range (or i == j)");
    pairs[(size_t)k] = make_int2(i, j);
  }
  const int per = plan_corr_pairs_per_pass(c->B, n_pairs, pairs_per_pass);
  if (per < 1) return fail(c, VMC_ERR_UNSUPPORTED, "batch_size does not leave room for one pair in the 32-bit row index");
  const bool cache_was[2] = {c->ps[0].cache_valid, c->ps[1].cache_valid};
  const bool acts_were = c->acts_valid;
  int rc = ensure_cache(c, which);           // (before the swap: it reads no bond set; gnn / ed_vector readiness, parameters)
  if (rc == VMC_OK) rc = corr_reserve(c, per, n_pairs);
  if (rc == VMC_OK) {
    hipError_t e = hipMemcpyAsync(c->corr_pairs, pairs.data(), (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  if (rc == VMC_OK) {
    const BondSet hamiltonian = current_set(c);
    for (long long k0 = 0; k0 < n_pairs && rc == VMC_OK; k0 += per) {
      const int n = (int)(n_pairs - k0 < per ? n_pairs - k0 : per);
      install_set(c, BondSet{n, c->corr_pairs + k0, c->corr_hx, c->corr_qz, c->corr_rowinfo, c->corr_val});
      rc = corr_pass(c, which, k0, n, n_pairs);
    }
    install_set(c, hamiltonian);
  }
  std::vector<double> out(rc == VMC_OK ? 2 * (size_t)n_pairs : 0);
  if (rc == VMC_OK) {
    hipError_t e = hipMemcpyAsync(out.data(), c->corr_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("vmc_pair_correlations read-back: ") + hipGetErrorString(e));
  } else {
    hipStreamSynchronize(c->stream);         // (`pairs` is the source of an asynchronous copy)
  }
  // what was not valid before is not vouched for now either: the next consumer fills it exactly as it would have
  for (int w = 0; w < 2; ++w) if (!cache_was[w]) c->ps[w].cache_valid = false;
  if (!acts_were) c->acts_valid = false;
  if (rc != VMC_OK) return rc;
  for (int k = 0; k < n_pairs; ++k) {
    if (zz_sum) zz_sum[k] = out[(size_t)k];
    if (ex_sum) ex_sum[k] = out[(size_t)n_pairs + (size_t)k];
  }
  return VMC_OK;
}

}  // extern "C"
