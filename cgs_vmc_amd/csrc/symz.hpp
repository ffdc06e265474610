// The symmetrized ansatz, psi_s(x) = sum_k chi_k psi(g_k x): the launchers of symz.hip (what a symmetrized ctx keeps beside
// the members of vmc_ctx: SymzState, vmc_api_symz.hip).  Rows of the base are op-major, row = k B + chain.
// Included by vmc_api_symz.hip and symz.hip only.
#pragma once
#include "common.hpp"

// the base's amplitudes of the n_ops B rows and the sector: what every fold reads
struct SymzRows {
  const float* logit; const float* sign;    // [n_ops][B] ln|psi(g_k x)| and the sign (null: +1)
  const double* chi;                        // [n_ops] characters
  int n_ops, B;
  int amp;                                  // 1: `sign` holds the amplitudes themselves (an ed_vector base)
};

// rows[k B + c][i] = f_k x'_c[perm_k[i]], x'_c = chain c with the proposed pair exchanged (k_prod_candidates' rule: a
// proposal that would not exchange an up with a down spin leaves the chain as it is; the accept kernel rejects it)
hipError_t launch_symz_candidates(hipStream_t st, const float* configs, const int* iup, const int* idn, const int* perm,
                                  const unsigned char* flip, int B, int N, int n_ops, int num_cus, float* rows);
// logit[c] = fl32(m + ln|S|), sign[c] = sgn(S) (amp: fl32(sum_k chi_k psi_k)); -inf and 0 at a structural zero
hipError_t launch_symz_fold(hipStream_t st, const SymzRows& r, float* logit, float* sign);
struct SymzAcceptArgs {
  float* configs; int N;
  int* iup; int* idn; float* u;             // the proposal under test; overwritten by the next one when draw_next
  SymzRows cand;                            // the base's amplitudes of the candidates' rows
  float* logit; float* sign;                // [B] psi_s of the chains (updated on accept)
  unsigned char* acc_mask;                  // [B] or null
  unsigned* acc_cnt;                        // [B] += accepted
  int draw_next; unsigned long long next_step;
  uint32_t seed_lo, seed_hi; int chain_offset;
};
hipError_t launch_symz_accept(hipStream_t st, const SymzAcceptArgs& a);
// E_s(c) = sum_k c_k E_k, diag likewise, c_k = chi_k s_k exp(l_k - m) / S into ck [n_ops][B], wk = E_s c_k.  r.amp: an op
// whose amplitude is 0 adds chi_k row_offdiag / psi_s, row_offdiag [n_ops][B] the base's off-diagonal sums (undivided there)
hipError_t launch_symz_eloc_fold(hipStream_t st, const SymzRows& r, const float* row_eloc, const float* row_diag,
                                 const float* row_offdiag, float* eloc, float* diag, float* offdiag, float* ck, float* wk);
