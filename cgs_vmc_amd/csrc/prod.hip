// ProductOfWavefunctions ('prod', wavefunctions.py:61-165) on gfx950: psi = psi_a psi_b over one set of chains.  The two
// factors are evaluated by their own kernels (vmc_api_prod.hip drives them); the kernels here are what only the product
// has: the candidates of a Monte Carlo step, the accept kernel (combined Metropolis test, commit, cache update, count,
// next proposal), the row combine of the local energies and the ITSWO ratio.  Everything goes through global memory
// with vector loads and stores; nothing here uses an atomic, so reruns with one seed are bit-identical.
#include "prod.hpp"
#include "plan.hpp"

__device__ __forceinline__ float prod_sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void k_prod_candidates(const float* __restrict__ configs, const int* __restrict__ iup,
                                                         const int* __restrict__ idn, int B, int N,
                                                         float* __restrict__ cand_a, float* __restrict__ cand_b) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)B * N) return;
  const int ch = (int)(q / N), i = (int)(q - (long long)ch * N);
  const float* x = configs + (long long)ch * N;
  const int u = iup[ch], d = idn[ch];
  float v = x[i];
  if (u >= 0 && u < N && d >= 0 && d < N && x[u] > 0.f && x[d] < 0.f && (i == u || i == d)) v = -v;
  cand_a[q] = v;
  cand_b[q] = v;
}

// One wave per chain.  graph_builders.py:75-88 in the logit domain: accept where |psi'|^2 / |psi|^2 > u, i.e.
// dlogit_a + dlogit_b > 0.5 log u (strict); a candidate with psi' = 0 is rejected, a chain at psi = 0 accepts any candidate
// that is not (the rule of the pbdg, nnb and ed_vector samplers).  Then the next proposal (graph_builders.py:59-65) in
// k_wide_propose's arithmetic from the chain as it stands after the commit: the exchanged spins are patched into the
// loaded values, so no lane depends on another lane's store.
__global__ __launch_bounds__(64 * PLAN_PROD_CHAINS_PER_WG) void k_prod_accept(ProdAcceptArgs a) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * PLAN_PROD_CHAINS_PER_WG + (threadIdx.x >> 6);
  if (ch >= a.B) return;
  const int N = a.N;
  float* x = a.configs + (long long)ch * N;
  const int iu = a.iup[ch], id = a.idn[ch];
  const float uu = a.u[ch];
  bool acc = false;
  if (iu >= 0 && iu < N && id >= 0 && id < N && x[iu] > 0.f && x[id] < 0.f) {
    const float cla = a.ca_l[ch], clb = a.cb_l[ch];
    const float csa = a.ca_s ? a.ca_s[ch] : 1.f, csb = a.cb_s ? a.cb_s[ch] : 1.f;
    const float s_new = prod_sgn(csa) * prod_sgn(csb);
    const float s_cur = prod_sgn(a.sa[ch]) * prod_sgn(a.sb[ch]);
    if (s_new != 0.f) {
      if (s_cur == 0.f) acc = true;
      else acc = (cla - a.la[ch]) + (clb - a.lb[ch]) > 0.5f * logf(uu);
    }
    if (acc && lane == 0) {
      a.la[ch] = cla; a.lb[ch] = clb;
      a.sa[ch] = csa; a.sb[ch] = csb;
    }
  }
  // the chain's spins as they stand after the commit; lane 0 stores the exchanged pair
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

__global__ __launch_bounds__(PLAN_PROD_FOLD_THREADS) void k_prod_count_fold(const unsigned* __restrict__ cnt, int B,
                                                                            unsigned long long* __restrict__ accepted) {
  __shared__ unsigned long long s[PLAN_PROD_FOLD_THREADS];
  unsigned long long t = 0;
  for (int i = threadIdx.x; i < B; i += PLAN_PROD_FOLD_THREADS) t += cnt[i];
  s[threadIdx.x] = t;
  __syncthreads();
  for (int d = PLAN_PROD_FOLD_THREADS / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) accepted[0] += s[0];
}

__global__ __launch_bounds__(256) void k_prod_row_combine(const float* __restrict__ va, const float* __restrict__ vb,
                                                          const int* __restrict__ off, int B, long long max_rows,
                                                          const int2* __restrict__ rowinfo,
                                                          const float* __restrict__ half_jx, float* __restrict__ val) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= max_rows || r >= (long long)off[B]) return;
  const int bs = rowinfo[r].y;
  const float h = half_jx[(bs > 0 ? bs : -bs) - 1];
  // each factor's term is half_jx psi'/psi: the coupling is taken once (a bond without exchange coupling adds nothing)
  val[r] = h == 0.f ? 0.f : __fdiv_rn(__fmul_rn(va[r], vb[r]), h);
}

__global__ __launch_bounds__(256) void k_prod_itswo_ratio(const float* __restrict__ lpa, const float* __restrict__ spa,
                                                          const float* __restrict__ lpb, const float* __restrict__ spb,
                                                          const float* __restrict__ lwa, const float* __restrict__ swa,
                                                          const float* __restrict__ lwb, const float* __restrict__ swb,
                                                          const float* __restrict__ ew, float lfa, float lfb, float beta,
                                                          int B, float* __restrict__ ratio) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  // psi_w = 0: the ratio is 0 whatever the logits hold; psi = 0: the reference's x / 0
  const float sw = prod_sgn(swa[i]) * prod_sgn(swb[i]);
  const float sp = prod_sgn(spa[i]) * prod_sgn(spb[i]);
  float r;
  if (sp == 0.f) r = __builtin_nanf("");
  else if (sw == 0.f) r = 0.f;
  else r = sw * sp * expf((lwa[i] - lpa[i] + lfa) + (lwb[i] - lpb[i] + lfb)) * (1.f - beta * ew[i]);
  ratio[i] = r;
}

hipError_t launch_prod_candidates(hipStream_t st, const float* configs, const int* iup, const int* idn, int B, int N,
                                  float* cand_a, float* cand_b) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prod_candidates, dim3(plan_prod_elem_grid((long long)B * N)), dim3(256), 0, st, configs, iup, idn,
                     B, N, cand_a, cand_b);
  return hipGetLastError();
}

hipError_t launch_prod_accept(hipStream_t st, const ProdAcceptArgs& a) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prod_accept, dim3(plan_prod_chain_grid(a.B)), dim3(64 * PLAN_PROD_CHAINS_PER_WG), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_prod_count_fold(hipStream_t st, const unsigned* acc_cnt, int B, unsigned long long* accepted) {
  hipLaunchKernelGGL(k_prod_count_fold, dim3(1), dim3(PLAN_PROD_FOLD_THREADS), 0, st, acc_cnt, B, accepted);
  return hipGetLastError();
}

hipError_t launch_prod_row_combine(hipStream_t st, const float* val_a, const float* val_b, const int* off, int B,
                                   long long max_rows, const int2* rowinfo, const float* half_jx, float* val) {
  if (max_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prod_row_combine, dim3(plan_prod_elem_grid(max_rows)), dim3(256), 0, st, val_a, val_b, off, B,
                     max_rows, rowinfo, half_jx, val);
  return hipGetLastError();
}

hipError_t launch_prod_itswo_ratio(hipStream_t st, const float* lpa, const float* spa, const float* lpb, const float* spb,
                                   const float* lwa, const float* swa, const float* lwb, const float* swb,
                                   const float* eloc_w, float log_factor_a, float log_factor_b, float beta, int B,
                                   float* ratio) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prod_itswo_ratio, dim3(plan_prod_elem_grid(B)), dim3(256), 0, st, lpa, spa, lpb, spb, lwa, swa,
                     lwb, swb, eloc_w, log_factor_a, log_factor_b, beta, B, ratio);
  return hipGetLastError();
}
