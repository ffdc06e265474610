// Four-spin (J-Q) Hamiltonian terms (vmc_set_four_spin_terms; host side: vmc_api_measure.hip, four_spin_device).  A term
// t = (i, j, k, l; q_t) with four distinct sites is -q_t (1/4 - S_i . S_j)(1/4 - S_k . S_l); with r(y) = psi(y) / psi(x)
// and the exchange sign sigma of the term set its local value on a configuration x is
//   e_t(x) = -(q_t / 4) [s_i != s_j][s_k != s_l] (1 - sigma r(swap_ij x) - sigma r(swap_kl x) + r(swap_kl swap_ij x))
// and the chains' local energies take sum_t e_t(x_c) on top of the Heisenberg part.
//
// The host hands the terms over as the table of their distinct unordered site pairs, pairs [n_pairs] ascending, and two
// pair indices per term, term_pairs [n_terms] (plan.hpp: plan_fourspin_pairs).
//
// The list.  Chain-major and compacted: per chain first one SINGLE row for every pair antiparallel on the chain, pairs
// ascending, then one DOUBLE row for every term with both pairs antiparallel, terms ascending.  k_fs_count counts both
// per chain, k_fs_scan is the exclusive prefix off [B + 1] over the chains (tile_scan_1024), and k_fs_fill writes the
// descriptors {chain, code} -- code = the pair index of a single row, n_pairs + the term index of a double row -- of the
// rows [q0, q0 + n) of ONE pass.  The place of a row within its chain is a ballot and a popcount over the lanes, which
// run along the pairs or terms: fs_walk states this order once, for the fill and the fold.  No atomics: the list depends
// on the configurations alone.  (The prefix, the row writer, lanes_below, measure_ratio and the fp64 butterfly
// wave_sum_f64 are the shared pieces of measure_dev.hpp.)  k_fs_rows writes the exchanged configurations of a pass's
// rows (one wavefront per row, the lanes along the site axis) for the family's own full
// forward, which leaves ln|psi| and the sign of every row in a result buffer that spans the whole list.
//
// The fold (k_fs_fold), once, after the last pass; one wavefront per chain:
//   * the ratios of the chain's single rows are formed in fp64 (measure_ratio: the row's and the chain's cached ln|psi|
//     and signs) and kept in LDS by pair index, 0 for a pair that is parallel on the chain;
//   * lane l walks the terms l, l + 64, ... ascending; per active term, with w = -q_t / 4 (exact in fp64), it adds
//     w, then fma(-sigma w, r_ij, .), fma(-sigma w, r_kl, .), fma(w, r_ijkl, .) in this order; then the butterfly
//     (xor 32, 16, ..., 1);
//   * eloc[c] = fp32((double)eloc[c] + sum): one rounding.
// For vmc_local_energy_terms alone a second instantiation of the fold (PARTS) also keeps the sum's two parts per chain in
// fp64 -- dsum, the w alone, and osum, the three ratio terms in the same order; the sum itself is the same chain of
// operations in both.  Every output is the same bits for every pass size, batch size and grid.
// A chain whose own amplitude vanishes (ed_vector) keeps what the Heisenberg part gave it: nothing is added, its rows are
// in the list but their values are never read.  A row at a vanishing amplitude gives r = 0.
#include "measure_dev.hpp"
#include "plan.hpp"

namespace {

__device__ __forceinline__ bool pair_anti(const float* __restrict__ x, const int2* __restrict__ pairs, int n_pairs, int p) {
  if (p >= n_pairs) return false;
  const int2 ij = pairs[p];
  return x[ij.x] != x[ij.y];
}

__device__ __forceinline__ bool term_active(const float* __restrict__ x, const int2* __restrict__ pairs,
                                            const int2* __restrict__ term_pairs, int n_terms, int t) {
  if (t >= n_terms) return false;
  const int2 ab = term_pairs[t];
  const int2 ij = pairs[ab.x], kl = pairs[ab.y];
  return x[ij.x] != x[ij.y] && x[kl.x] != x[kl.y];
}

// The order of a chain's part of the list, stated once: the pairs in groups of 64 (lane = place in the group), then the
// terms.  Per group the lanes within the table call f(emit, code, at) -- emit: this lane's pair / term has a row; code: the
// pair index, or n_pairs + the term index; at: the row's place in the list, q + the emitting lanes below.  between() runs
// once, behind the pair groups.  Returns q behind the chain's rows.  The whole wavefront calls it.  (A callable may tell
// a pair from a term by code < n_pairs: the term's code is formed as n_pairs + t with t >= 0 in sight, so that the
// compiler drops the other half in each loop -- profiles/list_scaffold_resources.txt has what it costs otherwise.)
template <class F, class G>
__device__ __forceinline__ long long fs_walk(const float* __restrict__ x, const int2* __restrict__ pairs,
                                             const int2* __restrict__ term_pairs, int n_pairs, int n_terms, int lane,
                                             long long q, F f, G between) {
  for (int p0 = 0; p0 < n_pairs; p0 += 64) {
    const int p = p0 + lane;
    const bool emit = pair_anti(x, pairs, n_pairs, p);
    const unsigned long long m = __ballot(emit);
    if (p < n_pairs) f(emit, p, q + lanes_below(m, lane));
    q += __popcll(m);
  }
  between();
  for (int t0 = 0; t0 < n_terms; t0 += 64) {
    const int t = t0 + lane;
    const bool emit = term_active(x, pairs, term_pairs, n_terms, t);
    const unsigned long long m = __ballot(emit);
    if (t < n_terms) f(emit, n_pairs + t, q + lanes_below(m, lane));
    q += __popcll(m);
  }
  return q;
}

}  // namespace

// One wavefront per chain (grid-stride): n_single[c] single rows, cnt[c] = single + double rows.  (Not over fs_walk: it
// wants the two totals and no place -- the order of the list does not enter a count.)
__global__ __launch_bounds__(256) void k_fs_count(const float* __restrict__ configs, const int2* __restrict__ pairs,
                                                  const int2* __restrict__ term_pairs, int B, int N, int n_pairs,
                                                  int n_terms, int* __restrict__ n_single, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < B; c += (long long)gridDim.x * 4) {
    const float* x = configs + c * N;
    int ns = 0, nd = 0;
    for (int p0 = 0; p0 < n_pairs; p0 += 64) ns += __popcll(__ballot(pair_anti(x, pairs, n_pairs, p0 + lane)));
    for (int t0 = 0; t0 < n_terms; t0 += 64) nd += __popcll(__ballot(term_active(x, pairs, term_pairs, n_terms, t0 + lane)));
    if (lane == 0) { n_single[c] = ns; cnt[c] = ns + nd; }
  }
}

// One workgroup: off[c] = sum of cnt[0 .. c) for c <= B (tile_scan_1024, measure_dev.hpp) and off[B + 1] = the sum of
// n_single (integers: the order of the additions does not matter)
__global__ __launch_bounds__(1024) void k_fs_scan(const int* __restrict__ cnt, const int* __restrict__ n_single, int B,
                                                  int* __restrict__ off) {
  __shared__ int s_wave[16];
  __shared__ int s_single[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  tile_scan_1024(cnt, B, off, s_wave);
  int singles = 0;
  for (int i = t; i < B; i += 1024) singles += n_single[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) singles += __shfl_xor(singles, o, 64);
  if (lane == 0) s_single[wave] = singles;
  __syncthreads();
  if (t == 0) {
    int all = 0;
    for (int w = 0; w < 16; ++w) all += s_single[w];
    off[B + 1] = all;
  }
}

// One wavefront per chain (grid-stride); a chain whose part of the list misses the pass [q0, q0 + n) leaves at once.
// desc[q - q0] = {chain, code}
__global__ __launch_bounds__(256) void k_fs_fill(const float* __restrict__ configs, const int2* __restrict__ pairs,
                                                 const int2* __restrict__ term_pairs, const int* __restrict__ off, int B,
                                                 int N, int n_pairs, int n_terms, long long q0, int n,
                                                 int2* __restrict__ desc) {
  const int lane = threadIdx.x & 63;
  const long long q1 = q0 + n;
  for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < B; c += (long long)gridDim.x * 4) {
    if (off[c + 1] <= q0 || off[c] >= q1) continue;
    fs_walk(configs + c * N, pairs, term_pairs, n_pairs, n_terms, lane, off[c],
            [&](bool emit, int code, long long at) {
              if (emit && at >= q0 && at < q1) desc[at - q0] = make_int2((int)c, code);
            },
            [] {});
  }
}

// One wavefront per row of the pass: swap_ij x of a single row, swap_kl swap_ij x of a double row (four distinct sites:
// the two exchanges do not meet).  The lanes run along the site axis.
__global__ __launch_bounds__(256) void k_fs_rows(const float* __restrict__ configs, const int2* __restrict__ pairs,
                                                 const int2* __restrict__ term_pairs, const int2* __restrict__ desc, int N,
                                                 int n_pairs, int n, float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < n; it += (long long)gridDim.x * 4) {
    const int2 cd = desc[it];
    const float* x = configs + (long long)cd.x * N;
    const bool two = cd.y >= n_pairs;
    int2 ij, kl = make_int2(0, 0);
    float sk = 0.f, sl = 0.f;                        // (a single row has no second exchange: never read)
    if (two) {
      const int2 ab = term_pairs[cd.y - n_pairs];
      ij = pairs[ab.x];
      kl = pairs[ab.y];
      sk = x[kl.x]; sl = x[kl.y];
    } else {
      ij = pairs[cd.y];
    }
    write_exchanged_row(rows + it * N, x, N, lane, ij, x[ij.x], x[ij.y], true, kl, sk, sl, two);
  }
}

// One wavefront per chain, one chain per workgroup; s_r [n_pairs] doubles of dynamic LDS (file header).  PARTS: dsum / osum
// are wanted too (null otherwise)
template <bool PARTS>
__global__ __launch_bounds__(64) void k_fs_fold(const float* __restrict__ configs, const int2* __restrict__ pairs,
                                                const int2* __restrict__ term_pairs, const double* __restrict__ wq,
                                                const int* __restrict__ off, const float* __restrict__ logit,
                                                const float* __restrict__ sign, const float* __restrict__ row_logit,
                                                const float* __restrict__ row_sign, int B, int N, int n_pairs, int n_terms,
                                                double sigma, float* __restrict__ eloc, double* __restrict__ dsum,
                                                double* __restrict__ osum) {
  extern __shared__ double s_r[];
  const int lane = threadIdx.x;
  const int c = blockIdx.x;
  if (c >= B) return;
  const int own = sign ? sgn_of(sign[c]) : 1;
  if (own == 0) {                                    // (the whole wavefront: nothing is added)
    if (PARTS && lane == 0) { dsum[c] = 0.0; osum[c] = 0.0; }
    return;
  }
  const double l0 = (double)logit[c];
  const float* x = configs + (long long)c * N;
  double s = 0.0, d = 0.0, o = 0.0;
  fs_walk(x, pairs, term_pairs, n_pairs, n_terms, lane, off[c],
          [&](bool emit, int code, long long at) {
            if (code < n_pairs) {                    // a pair: its ratio by pair index, 0 where it is parallel
              s_r[code] = emit ? measure_ratio(row_logit, row_sign, at, l0, own) : 0.0;
            } else if (emit) {                       // an active term
              const int t = code - n_pairs;
              const int2 ab = term_pairs[t];
              const double w = wq[t], ws = -sigma * w;
              const double r1 = s_r[ab.x], r2 = s_r[ab.y];
              const double r12 = measure_ratio(row_logit, row_sign, at, l0, own);
              s += w;
              s = fma(ws, r1, s);
              s = fma(ws, r2, s);
              s = fma(w, r12, s);
              if (PARTS) {
                d += w;
                o = fma(ws, r1, o);
                o = fma(ws, r2, o);
                o = fma(w, r12, o);
              }
            }
          },
          [] { __syncthreads(); });                  // the terms read every pair's ratio
  s = wave_sum_f64(s);
  if (PARTS) {
    d = wave_sum_f64(d);
    o = wave_sum_f64(o);
  }
  if (lane == 0) {
    eloc[c] = (float)((double)eloc[c] + s);
    if (PARTS) { dsum[c] = d; osum[c] = o; }
  }
}

hipError_t launch_fs_count(hipStream_t s, const float* configs, const int2* pairs, const int2* term_pairs, int B, int N,
                           int n_pairs, int n_terms, int num_cus, int* n_single, int* cnt, int* off) {
  hipLaunchKernelGGL(k_fs_count, dim3(measure_rows_grid(B, num_cus)), dim3(256), 0, s, configs, pairs, term_pairs, B, N,
                     n_pairs, n_terms, n_single, cnt);
  hipLaunchKernelGGL(k_fs_scan, dim3(1), dim3(1024), 0, s, cnt, n_single, B, off);
  return hipGetLastError();
}

hipError_t launch_fs_fill(hipStream_t s, const float* configs, const int2* pairs, const int2* term_pairs, const int* off,
                          int B, int N, int n_pairs, int n_terms, long long q0, int n, int num_cus, int2* desc) {
  hipLaunchKernelGGL(k_fs_fill, dim3(measure_rows_grid(B, num_cus)), dim3(256), 0, s, configs, pairs, term_pairs, off, B, N,
                     n_pairs, n_terms, q0, n, desc);
  return hipGetLastError();
}

hipError_t launch_fs_rows(hipStream_t s, const float* configs, const int2* pairs, const int2* term_pairs, const int2* desc,
                          int N, int n_pairs, int n, int num_cus, float* rows) {
  hipLaunchKernelGGL(k_fs_rows, dim3(measure_rows_grid(n, num_cus)), dim3(256), 0, s, configs, pairs, term_pairs, desc, N,
                     n_pairs, n, rows);
  return hipGetLastError();
}

hipError_t launch_fs_fold(hipStream_t s, const float* configs, const int2* pairs, const int2* term_pairs, const double* wq,
                          const int* off, AmpPair own, AmpPair rows, int B, int N, int n_pairs, int n_terms,
                          int exchange_sign, float* eloc, double* dsum, double* osum) {
  if (dsum && osum)
    hipLaunchKernelGGL(k_fs_fold<true>, dim3((unsigned)B), dim3(64), plan_fourspin_fold_lds(n_pairs), s, configs, pairs,
                       term_pairs, wq, off, own.logit, own.sign, rows.logit, rows.sign, B, N, n_pairs, n_terms,
                       (double)exchange_sign, eloc, dsum, osum);
  else
    hipLaunchKernelGGL(k_fs_fold<false>, dim3((unsigned)B), dim3(64), plan_fourspin_fold_lds(n_pairs), s, configs, pairs,
                       term_pairs, wq, off, own.logit, own.sign, rows.logit, rows.sign, B, N, n_pairs, n_terms,
                       (double)exchange_sign, eloc, nullptr, nullptr);
  return hipGetLastError();
}
