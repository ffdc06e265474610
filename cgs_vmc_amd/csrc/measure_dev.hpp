// Device pieces the measurement kernels and the list kernels share (gfx950 only; .hip files alone include it -- the
// host-only hostcheck programs see plan.hpp and nothing of this).  Everything here is integer work, a copy of +-1
// floats, or an fp64 chain whose order the callers' file headers state.
#pragma once
#include "common.hpp"

// sign of a stored sign / amplitude: +-1, 0 for a vanishing amplitude
__device__ inline int sgn_of(float v) { return (v > 0.f) - (v < 0.f); }
// psi(row) / psi(x) from ln|psi| and, signed types, the signs (own_sgn = +-1: the caller has dropped a chain whose own
// amplitude vanishes).  A vanishing amplitude of the row gives 0 exactly: its logarithm is never read.
__device__ inline double measure_ratio(const float* __restrict__ row_logit, const float* __restrict__ row_sign, long long at,
                                       double own_logit, int own_sgn) {
  int sg = own_sgn;
  if (row_sign) sg *= sgn_of(row_sign[at]);
  if (sg == 0) return 0.0;
  return (double)sg * exp((double)row_logit[at] - own_logit);
}
// the grid of the kernels that give one wavefront to an item -- the row writers (k_swap_rows, k_dimer_rows1 / 2,
// k_symm_rows, k_symz_candidates, k_mom_rows, k_fs_rows) and the list kernels (k_mom_count / fill, k_fs_count / fill):
// blocks of 4 wavefronts, at most 16 blocks per CU, grid-stride beyond
inline unsigned measure_rows_grid(long long items, int num_cus) {
  long long blocks = (items + 3) / 4;
  const long long cap = 16LL * (num_cus > 0 ? num_cus : 1);
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// the fixed butterfly of the fp64 folds: xor 32, 16, ..., 1
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the place of `lane` among the set lanes of a ballot
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// the spin of site q on swap_ij x, with si = x[ij.x] and sj = x[ij.y]: the exchange hands q = i the spin of j and the
// reverse (where si == sj it changes nothing, so the callers need not ask whether it acts)
__device__ __forceinline__ float spin_after(const float* __restrict__ x, int q, int2 ij, float si, float sj) {
  return q == ij.x ? sj : (q == ij.y ? si : x[q]);
}

// One wavefront writes row[0 .. N) (the lanes along the site axis): x with the sites of ij exchanged where `first`, then
// the sites of kl exchanged where `second`.  si, sj: the spins of ij on x; sk, sl: the spins of kl BEFORE the second
// exchange (on swap_ij x where the first acts).  k or l may be i or j: the later exchange decides.
__device__ __forceinline__ void write_exchanged_row(float* __restrict__ row, const float* __restrict__ x, int N, int lane,
                                                    int2 ij, float si, float sj, bool first, int2 kl, float sk, float sl,
                                                    bool second) {
  for (int q = lane; q < N; q += 64) {
    float v = x[q];
    if (first && q == ij.x) v = sj;
    if (first && q == ij.y) v = si;
    if (second && q == kl.x) v = sl;
    if (second && q == kl.y) v = sk;
    row[q] = v;
  }
}

// One workgroup of 1024 threads: off[i] = sum of cnt[0 .. i) for i <= n, tiles of 1024 entries with a running carry
// (integers: the order of the additions does not matter).  s_wave: 16 ints of LDS the call owns until it returns.  Every
// thread of the workgroup calls it, with the same n.
__device__ __forceinline__ void tile_scan_1024(const int* __restrict__ cnt, int n, int* __restrict__ off, int* s_wave) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + t;
    const int v = i < n ? cnt[i] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int sw = s_wave[w];
      if (w < wave) before += sw;
      total += sw;
    }
    if (i < n) off[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (t == 0) off[n] = carry;
}
