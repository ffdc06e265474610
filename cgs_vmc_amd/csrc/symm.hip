// Symmetry expectation values (vmc_symmetry_expectations, vmc_api_measure.hip).  An op k is a site permutation perm_k,
// optionally followed by the global spin flip: row[i] = f_k x[perm_k[i]], f_k = -1 where flip[k] and +1 otherwise, and
// <P_k> = <psi(row_k(x)) / psi(x)> over chains x sampled from |psi|^2.
//
// k_symm_rows writes the rows the family's own forward evaluates: row = op * B + chain.  perm_k is a bijection (checked on
// the host, plan_symm_check_ops), so every row stays at Sz = 0, which the kernels that index by up / down counts (pbdg,
// nnb, ed_vector) rely on.  k_symm_fold gives one wavefront per op: lane l adds the chains l, l + 64, ... in ascending
// order in fp64 and the 64 partial sums meet in a fixed butterfly, so that an op's sum depends on the chains alone -- not
// on the pass the op is in, not on the other ops, not on the grid -- and the B fp64 exponentials of an op are spread over
// the wavefront instead of one serial lane.
#include "measure_dev.hpp"

// One wavefront per (op, chain): the lanes run along the site axis, so the loads of perm_k and the stores of the row
// are contiguous per wavefront; the gather reads the chain's own N floats, which stay in cache.  Spins stay the fp32
// +-1 the family kernels read.
__global__ __launch_bounds__(256) void k_symm_rows(const float* __restrict__ configs, const int* __restrict__ perm,
                                                   const unsigned char* __restrict__ flip, int B, int N, int n_ops,
                                                   float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const long long items = (long long)n_ops * B;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
    const int k = (int)(it / B), c = (int)(it - (long long)k * B);
    const float* x = configs + (long long)c * N;
    const int* g = perm + (long long)k * N;
    const float f = flip[k] ? -1.f : 1.f;
    float* row = rows + it * N;
    for (int i = lane; i < N; i += 64) row[i] = f * x[g[i]];
  }
}

// One wavefront per op k: ratio_sum[k] = sum_c sigma exp(l(row_{k,c}) - l(x_c)), fp64.  logit / sign [B]: the chains' own
// (the ctx's cache); row_logit / row_sign [n_ops][B]: the rows'.  sign / row_sign == nullptr: unsigned amplitudes.  A
// vanishing amplitude on either side (sign 0; ed_vector has such entries) gives the term 0 exactly: its logarithm is
// never read.
__global__ __launch_bounds__(64) void k_symm_fold(const float* __restrict__ logit, const float* __restrict__ sign,
                                                  const float* __restrict__ row_logit,
                                                  const float* __restrict__ row_sign, int B, int n_ops,
                                                  double* __restrict__ ratio_sum) {
  const int k = blockIdx.x;
  if (k >= n_ops) return;
  const long long base = (long long)k * B;
  double sum = 0.0;
  for (int c = threadIdx.x; c < B; c += 64) {
    const int own = sign ? sgn_of(sign[c]) : 1;
    sum += own == 0 ? 0.0 : measure_ratio(row_logit, row_sign, base + c, (double)logit[c], own);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (threadIdx.x == 0) ratio_sum[k] = sum;
}

hipError_t launch_symm_rows(hipStream_t s, const float* configs, const int* perm, const unsigned char* flip, int B,
                            int N, int n_ops, int num_cus, float* rows) {
  hipLaunchKernelGGL(k_symm_rows, dim3(measure_rows_grid((long long)n_ops * B, num_cus)), dim3(256), 0, s, configs, perm,
                     flip, B, N, n_ops, rows);
  return hipGetLastError();
}

hipError_t launch_symm_fold(hipStream_t s, AmpPair own, AmpPair rows, int B, int n_ops, double* ratio_sum) {
  hipLaunchKernelGGL(k_symm_fold, dim3((unsigned)n_ops), dim3(64), 0, s, own.logit, own.sign, rows.logit, rows.sign, B, n_ops,
                     ratio_sum);
  return hipGetLastError();
}
