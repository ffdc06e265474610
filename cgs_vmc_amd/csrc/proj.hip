// Symmetry-projected energies (vmc_projected_energy, vmc_api_measure.hip).  With the ops g_k of vmc_symmetry_expectations
// (row_{k,c}[i] = f_k x_c[perm_k[i]]), real characters chi[s][k] of a sector s and r_{k,c} = psi(row_{k,c}) / psi(x_c),
//   w_s(c) = sum_k chi[s][k] r_{k,c},   E_s = <E_loc w_s> / <w_s>   over chains x_c sampled from |psi|^2
// is the energy of the projected state P_s psi.  The rows and their forward are symm.hip's k_symm_rows and the family's
// own full forward; this file holds the two accumulations.
//
// k_proj_accum adds the ops [k0, k0 + n) of a launch into the per-chain accumulator acc [n_sectors][B] (fp64, sector
// major: the loads and stores of a wavefront run along the chains).  A thread owns one chain and one tile of sectors:
// it forms each r_{k,c} once (one fp64 exponential), walks the ops in ascending k and adds fma(chi, r, acc) into the
// tile's accumulators in registers; the tile's characters [n][tile] are staged in LDS and read as broadcasts.  acc
// carries across launches and passes, so acc[s][c] is one chain of fp64 fmas in ascending k whatever the passes, the
// other sectors, the tiling or the grid.  A chain whose own amplitude vanishes adds nothing: its acc stays 0.
//
// k_proj_fold folds the chains in k_symm_fold's order -- one wavefront per sector, lane l the chains l, l + 64, ...
// ascending, then the fixed butterfly -- into w_sum[s] = sum_c w_s(c) and we_sum[s] = sum_c w_s(c) E_loc(c); one more
// wavefront gives e_sum = sum_c E_loc(c) and the number of chains alive.  E_loc of a chain whose own amplitude vanishes is
// never read (ed_vector: it is a division by zero).
#include "measure_dev.hpp"
#include "plan.hpp"

// grid chain blocks x sector tiles (block = chain block + chain blocks x tile), PLAN_PROJ_THREADS threads; LDS: chi of the tile [n][tile] doubles.
// logit / sign [B]: the chains' own (the ctx's cache); row_logit / row_sign [n][B]: the rows of the launch's ops;
// chi [n_sectors][n_ops_all] with the launch's first op at column k0.  sign / row_sign == nullptr: unsigned amplitudes.
__global__ __launch_bounds__(PLAN_PROJ_THREADS) void k_proj_accum(
    const float* __restrict__ logit, const float* __restrict__ sign, const float* __restrict__ row_logit,
    const float* __restrict__ row_sign, const double* __restrict__ chi, int B, int n_sectors, int n_ops_all, int k0, int n,
    int tile, double* __restrict__ acc) {
  extern __shared__ double s_chi[];
  const int chain_blocks = (B + PLAN_PROJ_THREADS - 1) / PLAN_PROJ_THREADS;
  const int s0 = (int)(blockIdx.x / chain_blocks) * tile;
  const int ts = n_sectors - s0 < tile ? n_sectors - s0 : tile;
  for (int e = threadIdx.x; e < n * tile; e += blockDim.x) {
    const int k = e / tile, j = e - k * tile;
    s_chi[e] = j < ts ? chi[(long long)(s0 + j) * n_ops_all + k0 + k] : 0.0;
  }
  __syncthreads();
  const int c = (int)(blockIdx.x % chain_blocks) * PLAN_PROJ_THREADS + threadIdx.x;
  if (c >= B) return;
  const int own = sign ? sgn_of(sign[c]) : 1;
  if (own == 0) return;
  const double own_logit = (double)logit[c];
  double a[PLAN_PROJ_MAX_TILE];
#pragma unroll
  for (int j = 0; j < PLAN_PROJ_MAX_TILE; ++j) a[j] = j < ts ? acc[(long long)(s0 + j) * B + c] : 0.0;
  for (int k = 0; k < n; ++k) {
    const double r = measure_ratio(row_logit, row_sign, (long long)k * B + c, own_logit, own);
    const double* x = s_chi + k * tile;
#pragma unroll
    for (int j = 0; j < PLAN_PROJ_MAX_TILE; ++j)
      if (j < tile) a[j] = fma(x[j], r, a[j]);
  }
#pragma unroll
  for (int j = 0; j < PLAN_PROJ_MAX_TILE; ++j)
    if (j < ts) acc[(long long)(s0 + j) * B + c] = a[j];
}

// n_sectors + 1 wavefronts.  out: [n_sectors] w_sum, [n_sectors] we_sum, e_sum, the chains alive (a count, as a double)
__global__ __launch_bounds__(64) void k_proj_fold(const float* __restrict__ sign, const float* __restrict__ eloc,
                                                  const double* __restrict__ acc, int B, int n_sectors,
                                                  double* __restrict__ out) {
  const int s = blockIdx.x;
  if (s > n_sectors) return;
  double u = 0.0, v = 0.0;
  if (s < n_sectors) {
    const double* w = acc + (long long)s * B;
    for (int c = threadIdx.x; c < B; c += 64) {
      if (sign && sgn_of(sign[c]) == 0) continue;
      const double wc = w[c];
      u += wc;
      v = fma(wc, (double)eloc[c], v);
    }
  } else {
    for (int c = threadIdx.x; c < B; c += 64) {
      if (sign && sgn_of(sign[c]) == 0) continue;
      u += (double)eloc[c];
      v += 1.0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    u += __shfl_xor(u, o, 64);
    v += __shfl_xor(v, o, 64);
  }
  if (threadIdx.x != 0) return;
  if (s < n_sectors) { out[s] = u; out[n_sectors + s] = v; }
  else { out[2 * n_sectors] = u; out[2 * n_sectors + 1] = v; }
}

hipError_t launch_proj_accum(hipStream_t s, AmpPair own, AmpPair rows, const double* chi, int B, int n_sectors, int n_ops_all,
                             int k0, int n, double* acc) {
  const int tile = plan_measure_sector_tile(n_sectors, n);
  if (tile < 1 || n > PLAN_PROJ_LAUNCH_OPS) return hipErrorInvalidValue;
  const dim3 grid(plan_proj_chain_blocks(B) * plan_proj_sector_tiles(n_sectors, tile));
  hipLaunchKernelGGL(k_proj_accum, grid, dim3(PLAN_PROJ_THREADS), plan_proj_accum_lds_bytes(tile, n), s, own.logit, own.sign,
                     rows.logit, rows.sign, chi, B, n_sectors, n_ops_all, k0, n, tile, acc);
  return hipGetLastError();
}

hipError_t launch_proj_fold(hipStream_t s, const float* sign, const float* eloc, const double* acc, int B, int n_sectors,
                            double* out) {
  hipLaunchKernelGGL(k_proj_fold, dim3((unsigned)n_sectors + 1), dim3(64), 0, s, sign, eloc, acc, B, n_sectors, out);
  return hipGetLastError();
}
