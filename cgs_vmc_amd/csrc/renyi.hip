// Renyi-2 entanglement entropy by the replica swap estimator (vmc_renyi2_swap, vmc_api_measure.hip).  The replica pairs
// are the chains (c, c + B/2); for a region A (a 0/1 mask over the sites) pair c MATCHES when both chains hold the same
// sum of spins on A, and then contributes psi(x~) psi(y~) / (psi(x) psi(y)) with the spins of A exchanged between the
// two; a pair that does not match would leave the Sz = 0 sector (psi = 0) and contributes 0.
//
// k_swap_rows writes the rows the family's own forward evaluates: row = region * B + chain, the swapped configuration
// for a matching pair and the chain's own for any other -- every row stays at Sz = 0, which the kernels that index by
// up / down counts (pbdg, nnb, ed_vector) rely on; the forward of an unswapped row is wasted work, the price of
// no compaction and no atomics.  k_swap_fold gives one thread per region, which walks the pairs in ascending order,
// re-derives the match from the spins it gathers under the mask and adds the terms in fp64: a region's sums depend on
// the chains alone -- not on the pass the region is in, not on the other regions, not on the grid.
#include "measure_dev.hpp"

// One wavefront per (region, pair): the lanes run along the site axis, so the loads of the two chains and of the mask
// and the stores of the two rows are contiguous per wavefront.  Spins stay the fp32 +-1 the family kernels read.
__global__ __launch_bounds__(256) void k_swap_rows(const float* __restrict__ configs,
                                                   const unsigned char* __restrict__ mask, int B, int N,
                                                   int n_regions, float* __restrict__ rows) {
  const int half = B / 2;
  const int lane = threadIdx.x & 63;
  const long long items = (long long)n_regions * half;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
    const int r = (int)(it / half), c = (int)(it - (long long)r * half);
    const float* x = configs + (long long)c * N;
    const float* y = configs + (long long)(c + half) * N;
    const unsigned char* m = mask + (long long)r * N;
    float d = 0.f;                                   // sum over A of x - y: small even integers, exact in fp32
    for (int i = lane; i < N; i += 64) d += m[i] ? x[i] - y[i] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    const bool match = d == 0.f;
    float* rx = rows + ((long long)r * B + c) * N;
    float* ry = rows + ((long long)r * B + c + half) * N;
    for (int i = lane; i < N; i += 64) {
      const float xi = x[i], yi = y[i];
      const bool sw = match && m[i];
      rx[i] = sw ? yi : xi;
      ry[i] = sw ? xi : yi;
    }
  }
}

// One thread per region k: swap_sum[k] = sum over matching pairs of sigma exp((l(x~) + l(y~)) - (l(x) + l(y))), pairs
// ascending, fp64; match_count[k] = the number of matching pairs.  logit / sign [B]: the chains' own (the ctx's
// cache); row_logit / row_sign [n_regions][B]: the swapped rows'.  sign / row_sign == nullptr: unsigned amplitudes.
// A vanishing amplitude among the four (sign 0; ed_vector has such entries) gives the term 0 exactly: its logarithm
// is never read.  A pair that does not match adds +0.0, which leaves the sum as it is.
__global__ __launch_bounds__(64) void k_swap_fold(const float* __restrict__ configs,
                                                  const unsigned char* __restrict__ mask,
                                                  const float* __restrict__ logit, const float* __restrict__ sign,
                                                  const float* __restrict__ row_logit,
                                                  const float* __restrict__ row_sign, int B, int N, int n_regions,
                                                  double* __restrict__ swap_sum, double* __restrict__ match_count) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_regions) return;
  const int half = B / 2;
  const unsigned char* m = mask + (long long)k * N;
  const float* rl = row_logit + (long long)k * B;
  const float* rs = row_sign ? row_sign + (long long)k * B : nullptr;
  double sum = 0.0;
  long long matches = 0;
  for (int c = 0; c < half; ++c) {
    const float* x = configs + (long long)c * N;
    const float* y = configs + (long long)(c + half) * N;
    float d = 0.f;
    for (int i = 0; i < N; ++i) d += m[i] ? x[i] - y[i] : 0.f;
    double term = 0.0;
    if (d == 0.f) {
      ++matches;
      int sigma = 1;
      if (sign) sigma = sgn_of(sign[c]) * sgn_of(sign[c + half]) * sgn_of(rs[c]) * sgn_of(rs[c + half]);
      if (sigma != 0)
        term = (double)sigma * exp(((double)rl[c] + (double)rl[c + half]) - ((double)logit[c] + (double)logit[c + half]));
    }
    sum += term;
  }
  swap_sum[k] = sum;
  match_count[k] = (double)matches;
}

hipError_t launch_swap_rows(hipStream_t s, const float* configs, const unsigned char* mask, int B, int N,
                            int n_regions, int num_cus, float* rows) {
  hipLaunchKernelGGL(k_swap_rows, dim3(measure_rows_grid((long long)n_regions * (B / 2), num_cus)), dim3(256), 0, s, configs,
                     mask, B, N, n_regions, rows);
  return hipGetLastError();
}

hipError_t launch_swap_fold(hipStream_t s, const float* configs, const unsigned char* mask, AmpPair own, AmpPair rows, int B,
                            int N, int n_regions, double* swap_sum, double* match_count) {
  hipLaunchKernelGGL(k_swap_fold, dim3(plan_measure_fold_grid(n_regions)), dim3(64), 0, s, configs, mask, own.logit, own.sign,
                     rows.logit, rows.sign, B, N, n_regions, swap_sum, match_count);
  return hipGetLastError();
}
