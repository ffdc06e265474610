// ProductOfWavefunctions ('prod'): the launchers of prod.hip (what a product ctx keeps beside the members of vmc_ctx:
// ProdState, vmc_api_prod.hip).
// Included by vmc_api_prod.hip and prod.hip only.
#pragma once
#include "common.hpp"

// cand_a = cand_b = the chains with the proposed pair exchanged (k_nnb_candidates' rule: a proposal that would not exchange
// an up with a down spin leaves the copy as it is; the accept kernel rejects it)
hipError_t launch_prod_candidates(hipStream_t st, const float* configs, const int* iup, const int* idn, int B, int N,
                                  float* cand_a, float* cand_b);
struct ProdAcceptArgs {
  float* configs; int B, N;
  int* iup; int* idn; float* u;             // the proposal under test; overwritten by the next one when draw_next
  float* la; float* sa; float* lb; float* sb;                          // the chains' logits / signs (updated on accept)
  const float* ca_l; const float* ca_s; const float* cb_l; const float* cb_s;   // the candidates' (a sign may be null: +1)
  unsigned char* acc_mask;                  // [B] or null
  unsigned* acc_cnt;                        // [B] += accepted
  int draw_next; unsigned long long next_step;
  uint32_t seed_lo, seed_hi; int chain_offset;
};
hipError_t launch_prod_accept(hipStream_t st, const ProdAcceptArgs& a);
// *accepted += sum_b acc_cnt[b], folded in a fixed order by one workgroup (no atomics)
hipError_t launch_prod_count_fold(hipStream_t st, const unsigned* acc_cnt, int B, unsigned long long* accepted);
// val[r] = val_a[r] val_b[r] / half_jx[bond(r)] for the rows r < off[B] of the shared row list: the factors' terms each
// carry the coupling once (0 where the coupling is 0)
hipError_t launch_prod_row_combine(hipStream_t st, const float* val_a, const float* val_b, const int* off, int B,
                                   long long max_rows, const int2* rowinfo, const float* half_jx, float* val);
// ratio_b = (psi_w / psi)(1 - beta E_loc^w) of the whole product: both signs, both shift differences
hipError_t launch_prod_itswo_ratio(hipStream_t st, const float* lpa, const float* spa, const float* lpb, const float* spb,
                                   const float* lwa, const float* swa, const float* lwb, const float* swb,
                                   const float* eloc_w, float log_factor_a, float log_factor_b, float beta, int B,
                                   float* ratio);
