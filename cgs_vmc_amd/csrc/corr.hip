// Spin-correlation measurement (vmc_pair_correlations, vmc_api_measure.hip): the TRANSPOSED reduction of the
// connected-row list -- per pair over chains, where k_eloc_reduce (eloc.hip) sums per chain over bonds.
//
// A pass of pairs is a bond set like the Hamiltonian's (j_x = 2, j_z = 0), so after the family's row launch
// val[row] = psi(swap_ij x_c) / psi(x_c) for the rows {chain, +-(pair + 1)} of the compact, chain-ordered list.
// k_pair_scatter writes every row to its slot dense[chain][pair] (a chain holds a pair at most once: no two rows
// share a slot); k_pair_fold then gives one thread per pair, which walks the chains in ascending order and adds
// in fp64.  The sum of a pair therefore depends on the chains alone: not on the pass the pair is in, not on the
// other pairs of the list, not on the grid.  No atomics.  Slots of parallel pairs are never written and never
// read (the fold re-derives the mask from the spins it gathers for s_i s_j anyway).
#include "common.hpp"

// rows [0, *n_rows_dev) of the list -> dense[chain * ld + pair]
__global__ __launch_bounds__(256) void k_pair_scatter(const int2* __restrict__ rowinfo,
                                                      const float* __restrict__ val,
                                                      const int* __restrict__ n_rows_dev, int B, int n_pairs,
                                                      float* __restrict__ dense) {
  const long long n = *n_rows_dev;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long long)gridDim.x * 256) {
    const int2 ri = rowinfo[r];
    const int k = (ri.y < 0 ? -ri.y : ri.y) - 1;
    if (ri.x >= 0 && ri.x < B && k >= 0 && k < n_pairs) dense[(long long)ri.x * n_pairs + k] = val[r];
  }
}

// one thread per pair k: zz[k] = sum_c s_i s_j (integers: exact), ex[k] = sum_c [s_i s_j < 0] dense[c][k], chains
// ascending.  Four chains per trip so that their loads travel together; the adds stay in chain order (a parallel
// pair adds +0.0, which leaves the sum as it is).
__global__ __launch_bounds__(64) void k_pair_fold(const float* __restrict__ configs,
                                                  const int2* __restrict__ pairs,
                                                  const float* __restrict__ dense, int B, int N, int n_pairs,
                                                  double* __restrict__ zz, double* __restrict__ ex) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_pairs) return;
  const int2 ab = pairs[k];
  double e = 0.0;
  long long z = 0;
  int c = 0;
  for (; c + 4 <= B; c += 4) {
    float sz[4], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* x = configs + (long long)(c + u) * N;
      sz[u] = x[ab.x] * x[ab.y];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = sz[u] < 0.f ? dense[(long long)(c + u) * n_pairs + k] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) { e += (double)v[u]; z += sz[u] < 0.f ? -1 : 1; }
  }
  for (; c < B; ++c) {
    const float* x = configs + (long long)c * N;
    const float sz = x[ab.x] * x[ab.y];
    const float v = sz < 0.f ? dense[(long long)c * n_pairs + k] : 0.f;
    e += (double)v; z += sz < 0.f ? -1 : 1;
  }
  zz[k] = (double)z;
  ex[k] = e;
}

hipError_t launch_pair_fold(hipStream_t s, const float* configs, const int2* pairs, const int2* rowinfo,
                            const float* val, const int* n_rows_dev, int B, int N, int n_pairs, int num_cus,
                            float* dense, double* zz, double* ex) {
  long long blocks = ((long long)B * n_pairs + 255) / 256;        // at most one row per chain and pair
  const long long cap = 8LL * (num_cus > 0 ? num_cus : 1);
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_pair_scatter, dim3((unsigned)blocks), dim3(256), 0, s, rowinfo, val, n_rows_dev, B, n_pairs,
                     dense);
  hipLaunchKernelGGL(k_pair_fold, dim3(plan_measure_fold_grid(n_pairs)), dim3(64), 0, s, configs, pairs, dense, B, N,
                     n_pairs, zz, ex);
  return hipGetLastError();
}
