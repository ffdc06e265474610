// The symmetrized ansatz on gfx950: psi_s(x) = sum_k chi_k psi(g_k x) over one set of B chains.  The base ctx evaluates
// the n_ops B permuted rows with its own kernels (vmc_api_symz.hip drives it); the kernels here are what only the
// composite has: the permuted candidates of a Monte Carlo step (exchange and permutation fused), the signed log-domain
// fold of the base's amplitudes, the accept kernel (fold of the candidates, Metropolis test, commit, cache update, count,
// next proposal) and the fold of the base's local energies with the weights c_k for the gradient.
//
// Every fold is ONE serial loop over the ops in ascending order in fp64 (symz_sum below), whoever runs it: an output
// depends on its chain and the ops alone -- not on the grid, not on the kernel that asked -- so the sampler's cached
// logits are vmc_amplitude's bit for bit and reruns are bit-identical.  Rows are op-major (row = k B + c): with one thread
// per chain the loads of an op coalesce over the chains.  No atomics; everything goes through global memory with
// vector loads and stores.
#include "symz.hpp"
#include "measure_dev.hpp"
#include "plan.hpp"

struct SymzSum {
  double m, S, A, amp;
  bool zero;
};

// does op k count for chain c: a character and an amplitude that are not zero.  A NaN amplitude of the base (diverged
// parameters) counts: it makes m, S and A NaN, which the zero rule takes for a zero -- the row is refused, the candidate
// rejected --, never a finite psi_s from the ops that are left
__device__ __forceinline__ bool symz_counts(const SymzRows& r, int k, long long at) {
  if (r.chi[k] == 0.0) return false;
  if (r.sign && r.sign[at] == 0.f) return false;
  return !(r.logit[at] == -INFINITY);
}

// m = max_k l_k over the ops that count, S = sum_k chi_k s_k exp(l_k - m), A = sum_k |chi_k| exp(l_k - m); amp (an
// ed_vector base): sum_k chi_k psi_k itself.  zero: no op counts, or |S| <= 2^-40 A (plan.hpp: the structural zero)
__device__ __forceinline__ SymzSum symz_sum(const SymzRows& r, int c) {
  SymzSum o;
  o.m = -INFINITY; o.S = 0.0; o.A = 0.0; o.amp = 0.0;
  for (int k = 0; k < r.n_ops; ++k) {
    const long long at = (long long)k * r.B + c;
    if (!symz_counts(r, k, at)) continue;
    const double l = (double)r.logit[at];
    if (l > o.m || l != l) o.m = l;                 // (a NaN sticks: no later logit compares above it)
  }
  if (!(o.m > -INFINITY)) { o.zero = true; return o; }      // no op counts, or a NaN among them
  for (int k = 0; k < r.n_ops; ++k) {
    const long long at = (long long)k * r.B + c;
    if (!symz_counts(r, k, at)) continue;
    const double chi = r.chi[k];
    const double sg = r.sign ? (double)sgn_of(r.sign[at]) : 1.0;
    const double e = exp((double)r.logit[at] - o.m);
    o.S += chi * sg * e;
    o.A += fabs(chi) * e;
    if (r.amp) o.amp += chi * (double)r.sign[at];
  }
  o.zero = plan_symz_is_zero(o.S, o.A);
  return o;
}

__device__ __forceinline__ float symz_logit(const SymzSum& s) { return s.zero ? -INFINITY : (float)(s.m + log(fabs(s.S))); }
__device__ __forceinline__ float symz_sign(const SymzRows& r, const SymzSum& s) {
  if (s.zero) return 0.f;
  return r.amp ? (float)s.amp : (s.S > 0.0 ? 1.f : -1.f);
}

// One wavefront per (op, chain), the lanes along the site axis (k_symm_rows' shape)
__global__ __launch_bounds__(256) void k_symz_candidates(const float* __restrict__ configs, const int* __restrict__ iup,
                                                         const int* __restrict__ idn, const int* __restrict__ perm,
                                                         const unsigned char* __restrict__ flip, int B, int N, int n_ops,
                                                         float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const long long items = (long long)n_ops * B;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
    const int k = (int)(it / B), c = (int)(it - (long long)k * B);
    const float* x = configs + (long long)c * N;
    const int* g = perm + (long long)k * N;
    const float f = flip[k] ? -1.f : 1.f;
    const int u = iup[c], d = idn[c];
    const bool ex = u >= 0 && u < N && d >= 0 && d < N && x[u] > 0.f && x[d] < 0.f;
    float* row = rows + it * N;
    for (int i = lane; i < N; i += 64) {
      const int j = g[i];
      float v = x[j];
      if (ex && (j == u || j == d)) v = -v;
      row[i] = f * v;
    }
  }
}

__global__ __launch_bounds__(PLAN_SYMZ_THREADS) void k_symz_fold(SymzRows r, float* __restrict__ logit,
                                                                 float* __restrict__ sign) {
  const int c = blockIdx.x * PLAN_SYMZ_THREADS + threadIdx.x;
  if (c >= r.B) return;
  const SymzSum s = symz_sum(r, c);
  logit[c] = symz_logit(s);
  sign[c] = symz_sign(r, s);
}

// One wave per chain.  Every lane runs the chain's fold (the same addresses: the loads broadcast), so the candidates'
// psi_s has symz_sum's bits.  Accept where |psi_s'|^2 / |psi_s|^2 > u, i.e. 2 (logit' - logit) > ln u (strict); a candidate
// at a structural zero is always rejected (with vmc_set_configs' refusal: no chain is ever at one).  Then the next proposal
// in k_wide_propose's arithmetic from the chain as it stands after the commit (k_prod_accept's second half).
__global__ __launch_bounds__(64 * PLAN_SYMZ_CHAINS_PER_WG) void k_symz_accept(SymzAcceptArgs a) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * PLAN_SYMZ_CHAINS_PER_WG + (threadIdx.x >> 6);
  if (ch >= a.cand.B) return;
  const int N = a.N;
  float* x = a.configs + (long long)ch * N;
  const int iu = a.iup[ch], id = a.idn[ch];
  const float uu = a.u[ch];
  bool acc = false;
  if (iu >= 0 && iu < N && id >= 0 && id < N && x[iu] > 0.f && x[id] < 0.f) {
    const SymzSum s = symz_sum(a.cand, ch);
    if (!s.zero) {
      const float l_new = symz_logit(s), l_cur = a.logit[ch];
      acc = a.sign[ch] == 0.f ? true : 2.f * (l_new - l_cur) > logf(uu);
      if (acc && lane == 0) { a.logit[ch] = l_new; a.sign[ch] = symz_sign(a.cand, s); }
    }
  }
  if (lane == 0) {
    if (acc) { x[iu] = -1.f; x[id] = 1.f; }
    if (a.acc_mask) a.acc_mask[ch] = acc ? 1 : 0;
    a.acc_cnt[ch] += acc ? 1u : 0u;
  }
  if (!a.draw_next) return;
  const uint2 key = make_uint2(a.seed_lo, a.seed_hi);
  const uint32_t gid = (uint32_t)(a.chain_offset + ch);
  const unsigned long long step = a.next_step;
  float best_hi = -INFINITY, best_lo = INFINITY;
  int idx_hi = 0x7fffffff, idx_lo = 0x7fffffff;
  const int nblk = (N + 3) >> 2;
  for (int b = lane; b < nblk; b += 64) {
    const uint4 r = philox4x32_10(make_uint4((uint32_t)b, gid, (uint32_t)step, (uint32_t)(step >> 32)), key);
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * b + e;
      if (i < N) {
        float xi = x[i];
        if (acc && i == iu) xi = -1.f;
        if (acc && i == id) xi = 1.f;
        const float v = xi * u32_to_uniform(rr[e]);
        if (v > best_hi) { best_hi = v; idx_hi = i; }
        if (v < best_lo) { best_lo = v; idx_lo = i; }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float oh = __shfl_xor(best_hi, d); const int ih = __shfl_xor(idx_hi, d);
    if (oh > best_hi || (oh == best_hi && ih < idx_hi)) { best_hi = oh; idx_hi = ih; }
    const float ol = __shfl_xor(best_lo, d); const int il = __shfl_xor(idx_lo, d);
    if (ol < best_lo || (ol == best_lo && il < idx_lo)) { best_lo = ol; idx_lo = il; }
  }
  if (lane == 0) {
    const uint4 ra = philox4x32_10(make_uint4(VMC_ACCEPT_BLOCK, gid, (uint32_t)step, (uint32_t)(step >> 32)), key);
    a.iup[ch] = idx_hi; a.idn[ch] = idx_lo; a.u[ch] = u32_to_uniform(ra.x);
  }
}

// One thread per chain: E_s = sum_k c_k E_k and the diagonal likewise, fp64, ops ascending, rounded once; an op that
// does not count has c_k = 0 and its E_k (which may be anything: the base divided by a vanishing amplitude) is never read.
// c_k E_k is chi_k (H psi)(g_k x) / psi_s, though, and (H psi)(g_k x) need not vanish where psi(g_k x) does: an ed_vector
// base hands over that row's off-diagonal sum undivided (row_offdiag, k_edvec_eloc's undivided_at_zero), and the op adds
// chi_k (H psi)(g_k x) / psi_s to E_s -- nothing to the diagonal, whose term carries psi(g_k x) = 0, and c_k stays 0.
// A chain at a structural zero (none is, by the sampler's rule) gets NaN, not a number that looks like an energy.
__global__ __launch_bounds__(PLAN_SYMZ_THREADS) void k_symz_eloc_fold(SymzRows r, const float* __restrict__ row_eloc,
                                                                      const float* __restrict__ row_diag,
                                                                      const float* __restrict__ row_offdiag,
                                                                      float* __restrict__ eloc, float* __restrict__ diag,
                                                                      float* __restrict__ offdiag, float* __restrict__ ck,
                                                                      float* __restrict__ wk) {
  const int c = blockIdx.x * PLAN_SYMZ_THREADS + threadIdx.x;
  if (c >= r.B) return;
  const SymzSum s = symz_sum(r, c);
  double E = 0.0, D = 0.0;
  for (int k = 0; k < r.n_ops; ++k) {
    const long long at = (long long)k * r.B + c;
    double w = 0.0;
    if (!s.zero && symz_counts(r, k, at)) {
      const double sg = r.sign ? (double)sgn_of(r.sign[at]) : 1.0;
      w = r.chi[k] * sg * exp((double)r.logit[at] - s.m) / s.S;
      E += w * (double)row_eloc[at];
      D += w * (double)row_diag[at];
    } else if (!s.zero && r.amp && r.chi[k] != 0.0 && r.sign[at] == 0.f) {
      E += r.chi[k] * (double)row_offdiag[at] / s.amp;
    }
    ck[at] = (float)w;
  }
  const float e32 = s.zero ? __builtin_nanf("") : (float)E;
  const float d32 = s.zero ? __builtin_nanf("") : (float)D;
  eloc[c] = e32; diag[c] = d32; offdiag[c] = e32 - d32;
  for (int k = 0; k < r.n_ops; ++k) {
    const long long at = (long long)k * r.B + c;
    wk[at] = s.zero ? 0.f : e32 * ck[at];
  }
}

hipError_t launch_symz_candidates(hipStream_t st, const float* configs, const int* iup, const int* idn, const int* perm,
                                  const unsigned char* flip, int B, int N, int n_ops, int num_cus, float* rows) {
  if (B <= 0 || n_ops <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_symz_candidates, dim3(measure_rows_grid((long long)n_ops * B, num_cus)), dim3(256), 0, st, configs,
                     iup, idn, perm, flip, B, N, n_ops, rows);
  return hipGetLastError();
}

hipError_t launch_symz_fold(hipStream_t st, const SymzRows& r, float* logit, float* sign) {
  if (r.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_symz_fold, dim3(plan_symz_chain_blocks(r.B)), dim3(PLAN_SYMZ_THREADS), 0, st, r, logit, sign);
  return hipGetLastError();
}

hipError_t launch_symz_accept(hipStream_t st, const SymzAcceptArgs& a) {
  if (a.cand.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_symz_accept, dim3(plan_symz_wave_grid(a.cand.B)), dim3(64 * PLAN_SYMZ_CHAINS_PER_WG), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_symz_eloc_fold(hipStream_t st, const SymzRows& r, const float* row_eloc, const float* row_diag,
                                 const float* row_offdiag, float* eloc, float* diag, float* offdiag, float* ck, float* wk) {
  if (r.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_symz_eloc_fold, dim3(plan_symz_chain_blocks(r.B)), dim3(PLAN_SYMZ_THREADS), 0, st, r, row_eloc,
                     row_diag, row_offdiag, eloc, diag, offdiag, ck, wk);
  return hipGetLastError();
}
