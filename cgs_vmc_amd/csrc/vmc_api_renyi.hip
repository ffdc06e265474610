// Renyi-2 entanglement entropy (extension, no reference counterpart): vmc_renyi2_swap, the replica swap estimator over the
// ctx's current chains taken as the B / 2 pairs (c, c + B / 2).  Per region A: swap_sum = sum over the pairs that hold
// the same sum of spins on A of psi(x~) psi(y~) / (psi(x) psi(y)), with the spins of A exchanged between the two chains,
// and match_count = the number of such pairs; the host forms Tr rho_A^2 ~ swap_sum / (B / 2) and S2 = -ln of it.
//
// A pass of regions is B rows per region in the row buffer of vmc_amplitude (renyi.hip: k_swap_rows), evaluated by the
// family's own full forward (rows_forward_device, vmc_api.hip) and folded per region (k_swap_fold) against the chains'
// cached ln|psi| and signs.  The call is a pure measurement: chains, step counter, accumulators, the Hamiltonian and the
// validity of the amplitude and activation caches are as before when it returns.
#include "vmc_ctx.hpp"

using namespace vmcapi;

namespace {

int renyi_reserve(vmc_ctx* c, long long n_regions) {
  if (n_regions <= c->renyi_cap) return VMC_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->renyi_mask) hipFree(c->renyi_mask);
  if (c->renyi_out) hipFree(c->renyi_out);
  c->renyi_mask = nullptr; c->renyi_out = nullptr; c->renyi_cap = 0;
  HIPCHK(c, dalloc(&c->renyi_mask, n_regions * c->N));
  HIPCHK(c, dalloc(&c->renyi_out, 2 * n_regions));
  c->renyi_cap = n_regions;
  return VMC_OK;
}

// regions [k0, k0 + n): rows, forward, fold
int renyi_pass(vmc_ctx* c, int which, long long k0, int n, long long n_regions) {
  const ParamSet& p = c->ps[which];
  const unsigned char* mask = c->renyi_mask + k0 * c->N;
  const long long rows = (long long)n * c->B;
  {
    Timer t(c, "renyi_rows");
    HIPCHK(c, launch_swap_rows(c->stream, c->configs, mask, c->B, c->N, n, c->num_cus, c->tmp_cfg));
  }
  {
    Timer t(c, "renyi_forward");
    PROPAGATE(rows_forward_device(c, which, c->tmp_cfg, rows, c->tmp_out, c->tmp_sign));
  }
  Timer t(c, "renyi_fold");
  HIPCHK(c, launch_swap_fold(c->stream, c->configs, mask, p.logit, c->sgn ? p.sign : nullptr, c->tmp_out,
                             c->sgn ? c->tmp_sign : nullptr, c->B, c->N, n, c->renyi_out + k0,
                             c->renyi_out + n_regions + k0));
  return VMC_OK;
}

}  // namespace

extern "C" {

int vmc_renyi2_swap(vmc_ctx* c, int which, int32_t n_regions, const uint8_t* region_mask, int32_t regions_per_pass,
                    double* swap_sum, double* match_count) {
  ENTER(c);
  REFUSE_PRODUCT(c, "vmc_renyi2_swap");
  REFUSE_COMPOSED(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  if (n_regions < 1 || !region_mask || regions_per_pass < 0) return fail(c, VMC_ERR_INVALID, "bad region arguments");
  if (c->B % 2 != 0) return fail(c, VMC_ERR_INVALID, "vmc_renyi2_swap pairs chain c with chain c + batch_size / 2: batch_size must be even");
  if (!c->sgn && c->oact != VMC_ACT_EXP_)
    return fail(c, VMC_ERR_UNSUPPORTED, "vmc_renyi2_swap needs the exp output activation (the logit is ln psi only then)");
  std::vector<unsigned char> mask((size_t)n_regions * (size_t)c->N);
  for (size_t k = 0; k < mask.size(); ++k) {
    if (region_mask[k] > 1) return fail(c, VMC_ERR_INVALID, "region mask entries are 0 or 1");
    mask[k] = region_mask[k];
  }
  const int per = plan_renyi_regions_per_pass(c->B, n_regions, regions_per_pass, plan_renyi_row_limit(c->N, c->Hp));
  if (per < 1) return fail(c, VMC_ERR_UNSUPPORTED, "batch_size does not leave room for one region in the 32-bit row index");
  const bool cache_was[2] = {c->ps[0].cache_valid, c->ps[1].cache_valid};
  const bool acts_were = c->acts_valid;
  int rc = ensure_cache(c, which);           // l(x), l(y) and their signs, as the local energies take them
  if (rc == VMC_OK) rc = renyi_reserve(c, n_regions);
  if (rc == VMC_OK) rc = grow_tmp(c, (long long)per * c->B);
  if (rc == VMC_OK) {
    hipError_t e = hipMemcpyAsync(c->renyi_mask, mask.data(), mask.size(), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  for (long long k0 = 0; k0 < n_regions && rc == VMC_OK; k0 += per) {
    const int n = (int)(n_regions - k0 < per ? n_regions - k0 : per);
    rc = renyi_pass(c, which, k0, n, n_regions);
  }
  std::vector<double> out(rc == VMC_OK ? 2 * (size_t)n_regions : 0);
  if (rc == VMC_OK) {
    hipError_t e = hipMemcpyAsync(out.data(), c->renyi_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, VMC_ERR_HIP, std::string("vmc_renyi2_swap read-back: ") + hipGetErrorString(e));
  } else {
    hipStreamSynchronize(c->stream);         // (`mask` is the source of an asynchronous copy)
  }
  // what was not valid before is not vouched for now either: the next consumer fills it exactly as it would have
  for (int w = 0; w < 2; ++w) if (!cache_was[w]) c->ps[w].cache_valid = false;
  if (!acts_were) c->acts_valid = false;
  if (rc != VMC_OK) return rc;
  for (int k = 0; k < n_regions; ++k) {
    if (swap_sum) swap_sum[k] = out[(size_t)k];
    if (match_count) match_count[k] = out[(size_t)n_regions + (size_t)k];
  }
  return VMC_OK;
}

}  // extern "C"
