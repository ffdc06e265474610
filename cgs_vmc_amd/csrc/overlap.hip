// Overlap with the frozen parameter set (vmc_overlap, vmc_api_measure.hip; vmc_accumulate's mode PENALIZED_ENERGY,
// vmc_api_train.hip).  The chains x_c are drawn from |psi|^2 and r_c = omega(x_c) / psi(x_c):
//   <omega|psi>^2 / (<psi|psi><omega|omega>) = <r>^2 / <r^2> ~ S1^2 / (alive S2),  S1 = sum_c r_c, S2 = sum_c r_c^2.
// Both amplitudes live in the log domain and their scales are unrelated (two exponent shifts, two trainings), so no
// r_c is ever formed on its own: d_c = ln|r_c| in fp64 from the two fp32 amplitude caches, m = max_c d_c, and every
// exponential is of d_c - m <= 0.  The estimator does not depend on m; sum_c r_c = exp(m) S1 is left to the host.
//
// Dead chains.  A chain whose own amplitude vanishes (the signed types: a stored sign / entry of 0) is dead: code
// OVERLAP_DEAD, ratio 0, in no sum, not alive.  A vanishing omega(x_c) gives code 0 and a ratio of 0 exactly: its
// logarithm is never read, it takes no part in the max, the chain stays alive.  (measure_ratio's rule, measure_dev.hpp.)
//
// Summation order.  k_overlap_ratio is the only kernel whose grid touches the sums, and only through the blocks' maxima
// of d, which are exact in any order.  k_overlap_fold is ONE workgroup of 256: thread t adds the chains t, t + 256, ...
// in ascending order, then the 256 partial sums meet in a fixed butterfly (stride 128, 64, ... 1).  S1, S2, alive and m
// are therefore the same bits from call to call and for any grid of the other two kernels; nothing is added atomically.
//
// Weights.  w_c = E_loc(c) + lambda (S1 / S2) s_c exp(d_c - m) in fp64, rounded once to fp32: by Cauchy-Schwarz
// |S1 s_c exp(d_c - m) / S2| <= sqrt(B), and S1 / S2 has no 0 / 0 when the states are orthogonal on the batch.  A dead
// chain keeps E_loc(c); S2 = 0 (every ratio vanishes) leaves w = E_loc.
#include "measure_dev.hpp"

__global__ __launch_bounds__(256) void k_overlap_ratio(const float* __restrict__ lp, const float* __restrict__ sp,
                                                       double shift_p, const float* __restrict__ lw,
                                                       const float* __restrict__ sw, double shift_w, int B,
                                                       double* __restrict__ d, int* __restrict__ code,
                                                       double* __restrict__ bmax) {
  __shared__ double sm[256];
  const int c = blockIdx.x * 256 + threadIdx.x;
  double dv = -INFINITY;
  if (c < B) {
    int cd = OVERLAP_DEAD;
    const int own = sp ? sgn_of(sp[c]) : 1;
    if (own != 0) {
      cd = own * (sw ? sgn_of(sw[c]) : 1);
      if (cd != 0) dv = __dsub_rn(__dsub_rn((double)lw[c], shift_w), __dsub_rn((double)lp[c], shift_p));
    }
    d[c] = cd == 1 || cd == -1 ? dv : 0.0;
    code[c] = cd;
  }
  sm[threadIdx.x] = dv;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) bmax[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(256) void k_overlap_fold(const double* __restrict__ d, const int* __restrict__ code,
                                                      const double* __restrict__ bmax, int n_blocks, int B,
                                                      double* __restrict__ out) {
  __shared__ double s1s[256], s2s[256], als[256];
  const int t = threadIdx.x;
  double m = -INFINITY;
  for (int i = t; i < n_blocks; i += 256) m = fmax(m, bmax[i]);
  s1s[t] = m;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) s1s[t] = fmax(s1s[t], s1s[t + s]);
    __syncthreads();
  }
  m = s1s[0];
  if (!(m > -INFINITY)) m = 0.0;                // no chain with a ratio: every sum is 0 whatever the scale
  __syncthreads();
  double s1 = 0.0, s2 = 0.0, al = 0.0;
  for (int c = t; c < B; c += 256) {
    const int cd = code[c];
    if (cd == OVERLAP_DEAD) continue;
    al = __dadd_rn(al, 1.0);
    if (cd == 0) continue;
    const double e = exp(__dsub_rn(d[c], m));
    s1 = __dadd_rn(s1, cd > 0 ? e : -e);
    s2 = __dadd_rn(s2, __dmul_rn(e, e));
  }
  s1s[t] = s1; s2s[t] = s2; als[t] = al;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) {
      s1s[t] = __dadd_rn(s1s[t], s1s[t + s]);
      s2s[t] = __dadd_rn(s2s[t], s2s[t + s]);
      als[t] = __dadd_rn(als[t], als[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) { out[0] = s1s[0]; out[1] = s2s[0]; out[2] = als[0]; out[3] = m; }
}

__global__ __launch_bounds__(256) void k_overlap_weights(const double* __restrict__ d, const int* __restrict__ code,
                                                         const double* __restrict__ sums,
                                                         const float* __restrict__ eloc, float lambda, int B,
                                                         float* __restrict__ w, double* __restrict__ ratio) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= B) return;
  const double s1 = sums[0], s2 = sums[1], m = sums[3];
  const int cd = code[c];
  double r = 0.0;
  if (cd == 1 || cd == -1) {
    const double e = exp(__dsub_rn(d[c], m));
    r = cd > 0 ? e : -e;
  }
  if (ratio) ratio[c] = r;
  if (w) {
    double v = (double)eloc[c];
    if (s2 > 0.0 && cd != OVERLAP_DEAD) v += (double)lambda * (s1 / s2) * r;
    w[c] = (float)v;
  }
}

// slots 5 and 6 of the accumulators' scalar tail: the call's fidelity estimate and the number of calls
__global__ void k_overlap_tail(const double* __restrict__ sums, float* __restrict__ sc) {
  const double s1 = sums[0], s2 = sums[1], alive = sums[2];
  const double f = (s2 > 0.0 && alive > 0.0) ? s1 * s1 / (alive * s2) : 0.0;
  sc[5] += (float)f;
  sc[6] += 1.f;
}

hipError_t launch_overlap_ratio(hipStream_t s, AmpPair psi, double shift_psi, AmpPair omega, double shift_omega, int B,
                                double* d, int* code, double* bmax) {
  hipLaunchKernelGGL(k_overlap_ratio, dim3(plan_overlap_blocks(B)), dim3(256), 0, s, psi.logit, psi.sign, shift_psi,
                     omega.logit, omega.sign, shift_omega, B, d, code, bmax);
  return hipGetLastError();
}

hipError_t launch_overlap_fold(hipStream_t s, const double* d, const int* code, const double* bmax, int B, double* out) {
  hipLaunchKernelGGL(k_overlap_fold, dim3(1), dim3(256), 0, s, d, code, bmax, plan_overlap_blocks(B), B, out);
  return hipGetLastError();
}

hipError_t launch_overlap_weights(hipStream_t s, const double* d, const int* code, const double* sums, const float* eloc,
                                  float lambda, int B, float* w, double* ratio) {
  hipLaunchKernelGGL(k_overlap_weights, dim3(plan_overlap_blocks(B)), dim3(256), 0, s, d, code, sums, eloc, lambda, B, w,
                     ratio);
  return hipGetLastError();
}

hipError_t launch_overlap_tail(hipStream_t s, const double* sums, float* acc_scalars) {
  hipLaunchKernelGGL(k_overlap_tail, dim3(1), dim3(1), 0, s, sums, acc_scalars);
  return hipGetLastError();
}
