// Dimer-dimer correlations <(S_i . S_j)(S_k . S_l)> (vmc_dimer_correlations, vmc_api_measure.hip).  With a = (i, j),
// b = (k, l), r(y) = psi(y) / psi(x), x' = swap_ij x and s' the spins of x':
//   bond(a; x)  = s_i s_j / 4 + [s_i != s_j] r(x') / 2
//   dd(a, b; x) = s_i s_j / 4 (s_k s_l / 4 + [s_k != s_l] r(swap_kl x) / 2)
//               + [s_i != s_j] / 2 (s'_k s'_l r(x') / 4 + [s'_k != s'_l] r(swap_kl x') / 2)
// i.e. <x| A B |psi> / psi(x): B acts on the intermediate configuration x', so bonds that share a site and a == b are
// the same lines of code as disjoint ones.
//
// k_dimer_rows1 / k_dimer_rows2 write the rows the family's own forward evaluates (each decodes its item and its
// indicator, then calls write_exchanged_row; spin_after gives the spins on x': measure_dev.hpp): an exchanged configuration where the
// exchange acts (the bond antiparallel) and the chain's own elsewhere -- an exchange of two opposite spins keeps
// Sz = 0, which the kernels that index by up / down counts (pbdg, nnb, ed_vector) rely on; the forward of an unexchanged
// row is wasted work, the price of no compaction and no atomics.  The folds give one thread per bond / pair, which walks
// the chains in ascending order, re-derives the indicator bits from the spins it gathers and adds the terms in fp64: a
// sum depends on the chains alone -- not on the pass the pair is in, not on the other entries of the lists, not on the grid.
#include "measure_dev.hpp"

// One wavefront per (bond, chain): the lanes run along the site axis, so the loads of the chain and the stores of the
// row are contiguous per wavefront.  Spins stay the fp32 +-1 the family kernels read.
__global__ __launch_bounds__(256) void k_dimer_rows1(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                     int B, int N, int n_bonds, float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const long long items = (long long)n_bonds * B;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
    const int a = (int)(it / B), c = (int)(it - (long long)a * B);
    const float* x = configs + (long long)c * N;
    const int2 ij = bonds[a];
    const float si = x[ij.x], sj = x[ij.y];
    write_exchanged_row(rows + it * N, x, N, lane, ij, si, sj, si != sj, ij, si, sj, false);
  }
}

// One wavefront per (pair, chain): swap_kl swap_ij x where [s_i != s_j] holds on x and [s'_k != s'_l] on x' = swap_ij x
__global__ __launch_bounds__(256) void k_dimer_rows2(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                     const int2* __restrict__ pairs, int B, int N, int n_pairs,
                                                     float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const long long items = (long long)n_pairs * B;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * 4) {
    const int p = (int)(it / B), c = (int)(it - (long long)p * B);
    const float* x = configs + (long long)c * N;
    const int2 ab = pairs[p];
    const int2 ij = bonds[ab.x], kl = bonds[ab.y];
    const float si = x[ij.x], sj = x[ij.y];
    const float sk = spin_after(x, kl.x, ij, si, sj), sl = spin_after(x, kl.y, ij, si, sj);       // on x'
    const bool both = si != sj && sk != sl;          // (the chain's own row unless BOTH exchanges act)
    write_exchanged_row(rows + it * N, x, N, lane, ij, si, sj, both, kl, sk, sl, both);
  }
}

// One thread per bond a: bond_sum[a] = sum_c s_i s_j / 4 + [s_i != s_j] r(swap_ij x_c) / 2, chains ascending, fp64
__global__ __launch_bounds__(64) void k_dimer_bond_fold(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                        const float* __restrict__ logit, const float* __restrict__ sign,
                                                        const float* __restrict__ one_logit,
                                                        const float* __restrict__ one_sign, int B, int N, int n_bonds,
                                                        double* __restrict__ bond_sum) {
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= n_bonds) return;
  const int2 ij = bonds[a];
  double sum = 0.0;
  for (int c = 0; c < B; ++c) {
    const float* x = configs + (long long)c * N;
    const int own = sign ? sgn_of(sign[c]) : 1;
    double term = 0.0;
    if (own != 0) {
      const float si = x[ij.x], sj = x[ij.y];
      term = 0.25 * (double)(si * sj);
      if (si != sj) term += 0.5 * measure_ratio(one_logit, one_sign, (long long)a * B + c, (double)logit[c], own);
    }
    sum += term;
  }
  bond_sum[a] = sum;
}

// One thread per pair p = (a, b): dd_sum[p] = sum_c dd(a, b; x_c), chains ascending, fp64.  The four terms of a chain
// are added in the order of the formula above.
__global__ __launch_bounds__(64) void k_dimer_fold(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                   const int2* __restrict__ pairs, const float* __restrict__ logit,
                                                   const float* __restrict__ sign, const float* __restrict__ one_logit,
                                                   const float* __restrict__ one_sign, const float* __restrict__ two_logit,
                                                   const float* __restrict__ two_sign, int B, int N, int n_pairs,
                                                   double* __restrict__ dd_sum) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_pairs) return;
  const int2 ab = pairs[p];
  const int2 ij = bonds[ab.x], kl = bonds[ab.y];
  double sum = 0.0;
  for (int c = 0; c < B; ++c) {
    const float* x = configs + (long long)c * N;
    const int own = sign ? sgn_of(sign[c]) : 1;
    double term = 0.0;
    if (own != 0) {
      const double l0 = (double)logit[c];
      const float si = x[ij.x], sj = x[ij.y], sk = x[kl.x], sl = x[kl.y];
      // B on x, weighted by the diagonal part of A
      double inner = 0.25 * (double)(sk * sl);
      if (sk != sl) inner += 0.5 * measure_ratio(one_logit, one_sign, (long long)ab.y * B + c, l0, own);
      term = 0.25 * (double)(si * sj) * inner;
      if (si != sj) {
        // B on x' = swap_ij x
        const float tk = spin_after(x, kl.x, ij, si, sj), tl = spin_after(x, kl.y, ij, si, sj);
        double outer = 0.25 * (double)(tk * tl) * measure_ratio(one_logit, one_sign, (long long)ab.x * B + c, l0, own);
        if (tk != tl) outer += 0.5 * measure_ratio(two_logit, two_sign, (long long)p * B + c, l0, own);
        term += 0.5 * outer;
      }
    }
    sum += term;
  }
  dd_sum[p] = sum;
}

hipError_t launch_dimer_rows1(hipStream_t s, const float* configs, const int2* bonds, int B, int N, int n_bonds,
                              int num_cus, float* rows) {
  hipLaunchKernelGGL(k_dimer_rows1, dim3(measure_rows_grid((long long)n_bonds * B, num_cus)), dim3(256), 0, s, configs,
                     bonds, B, N, n_bonds, rows);
  return hipGetLastError();
}

hipError_t launch_dimer_rows2(hipStream_t s, const float* configs, const int2* bonds, const int2* pairs, int B, int N,
                              int n_pairs, int num_cus, float* rows) {
  hipLaunchKernelGGL(k_dimer_rows2, dim3(measure_rows_grid((long long)n_pairs * B, num_cus)), dim3(256), 0, s, configs,
                     bonds, pairs, B, N, n_pairs, rows);
  return hipGetLastError();
}

hipError_t launch_dimer_bond_fold(hipStream_t s, const float* configs, const int2* bonds, AmpPair own, AmpPair one, int B,
                                  int N, int n_bonds, double* bond_sum) {
  hipLaunchKernelGGL(k_dimer_bond_fold, dim3(plan_measure_fold_grid(n_bonds)), dim3(64), 0, s, configs, bonds, own.logit,
                     own.sign, one.logit, one.sign, B, N, n_bonds, bond_sum);
  return hipGetLastError();
}

hipError_t launch_dimer_fold(hipStream_t s, const float* configs, const int2* bonds, const int2* pairs, AmpPair own,
                             AmpPair one, AmpPair two, int B, int N, int n_pairs, double* dd_sum) {
  hipLaunchKernelGGL(k_dimer_fold, dim3(plan_measure_fold_grid(n_pairs)), dim3(64), 0, s, configs, bonds, pairs, own.logit,
                     own.sign, one.logit, one.sign, two.logit, two.sign, B, N, n_pairs, dd_sum);
  return hipGetLastError();
}
