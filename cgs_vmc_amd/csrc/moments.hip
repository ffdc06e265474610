// Lanczos-step energies (vmc_energy_moments, vmc_api_measure.hip): per chain x the local energy e(x) = (H psi)(x) / psi(x)
// and the local value of H^2, g(x) = (H^2 psi)(x) / psi(x).  With hx_b = j_x[b] / 2, qz_b = j_z[b] / 4,
// diag(y) = sum_b qz_b y_i y_j, y^a = y with the sites of bond a exchanged and r(y) = psi(y) / psi(x):
//   g(x) = diag(x) e(x) + sum_{a anti on x} hx_a [ r(x^a) diag(x^a) + sum_{b anti on x^a} hx_b r(x^{ab}) ]
// e(x) and the products val[r] = hx_a r(x^a) are what one local-energy call leaves (fp32: eloc, val over the chain-ordered
// first-order list rowinfo / off of eloc.hip); everything added on top is fp64.
//
// The second-order list.  For a first-order row (c, a) the bonds b antiparallel on x^a are walked in ascending order:
//   1. b names the unordered site pair of a (b == a or a twin bond): x^{ab} = x, r = 1 -- the term hx_a hx_b, no row;
//   2. b shares no site with a: x^{ab} = x^{ba}, (b, a) occurs too -- one row for a < b alone, coefficient 2 hx_a hx_b;
//   3. b shares exactly one site with a: one row, coefficient hx_a hx_b.
// The list is chain-major, then a, then b: k_mom_count counts the rows of every first-order row (and leaves diag(x^a) and
// the sum of rule 1's hx_b per first-order row), k_mom_scan is the exclusive prefix off2 over the first-order rows, and
// k_mom_fill writes the descriptors {first-order row, b} and coefficients of the rows [q0, q0 + n) of ONE pass -- the list
// itself never exists as a whole.  No atomics: the same list on every run.  k_mom_rows writes the configurations of a
// pass's rows (lanes along the site axis) for the family's own full forward.  The prefix, the row writer, spin_after,
// lanes_below and the fp64 butterfly wave_sum_f64 are the shared pieces of measure_dev.hpp.
//
// Summation order (every output is the same bits for every pass size; a pass may end inside a chain's rows):
//   * diag(y) of any configuration: lane l adds qz_b y_i y_j of the bonds b = l, l + 64, ... ascending by fused
//     multiply-adds, then the butterfly (xor 32, 16, ..., 1).  Rule 1's sum of hx_b: the same order.
//   * second-order rows of chain c: row q of the list, at place q - off2[off[c]] within the chain, belongs to lane
//     (place mod 64) of lanes[c][64]; k_mom_accum adds fma(coef, r, lane) in ascending q.  The passes arrive in ascending q
//     on one stream, so a lane's chain of fmas does not depend on where they end.
//   * g(c) (k_mom_chain): lane l starts from lanes[c][l] and walks the chain's first-order rows off[c] + l, + 64, ...
//     ascending, adding fma(val, diag(x^a), .) then fma(hx_a, rule 1's sum, .) per row; the butterfly; last
//     fma(diag(x), e(x), .).
//   * the six sums (k_mom_sums): one wavefront, lane j < 6 one sum each, the chains strictly ascending:
//     sum e, sum e^2, sum g, sum e g, sum g^2 (each product rounded to fp64, then added) and the chains alive.
// A chain whose own amplitude vanishes (ed_vector) has e = g = 0, adds to no sum and is not alive; its rows are in the
// list (the list depends on the configurations alone) but their values are never read.
#include "measure_dev.hpp"
#include "plan.hpp"

namespace {

// bond b = kl against a = ij: 1 the same unordered pair, 2 no common site, 3 exactly one common site
__device__ __forceinline__ int bond_rule(int2 ij, int2 kl) {
  const int common = (kl.x == ij.x || kl.x == ij.y) + (kl.y == ij.x || kl.y == ij.y);
  return common == 2 ? 1 : (common == 0 ? 2 : 3);
}

struct SecondOrder {     // what lane `lane` finds at bond b of a first-order row (c, a)
  bool emit;             // a row of the list
  bool self;             // rule 1
  int rule;
  float hx;
  double qz, ss;         // qz_b and s_k s_l on x^a
};

__device__ __forceinline__ SecondOrder second_order(const float* __restrict__ x, const int2* __restrict__ bonds,
                                                    const float* __restrict__ half_jx, const float* __restrict__ quarter_jz,
                                                    int n_bonds, int a, int2 ij, float si, float sj, int b) {
  SecondOrder s{false, false, 0, 0.f, 0.0, 0.0};
  if (b >= n_bonds) return s;
  const int2 kl = bonds[b];
  const float sk = spin_after(x, kl.x, ij, si, sj), sl = spin_after(x, kl.y, ij, si, sj);
  s.qz = (double)quarter_jz[b];
  s.ss = (double)(sk * sl);
  if (sk == sl) return s;
  s.rule = bond_rule(ij, kl);
  s.hx = half_jx[b];
  s.self = s.rule == 1;
  s.emit = s.rule == 3 || (s.rule == 2 && a < b);
  return s;
}

}  // namespace

// One wavefront per first-order row r < *n1_dev (grid-stride): cnt2[r] rows of the second-order list, diag1[r] = diag(x^a),
// self1[r] = the sum of hx_b over rule 1's bonds.  The lanes run along the bonds.
__global__ __launch_bounds__(256) void k_mom_count(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                   const float* __restrict__ half_jx, const float* __restrict__ quarter_jz,
                                                   const int2* __restrict__ rowinfo, const int* __restrict__ n1_dev, int N,
                                                   int n_bonds, int* __restrict__ cnt2, double* __restrict__ diag1,
                                                   double* __restrict__ self1) {
  const int lane = threadIdx.x & 63;
  const int n1 = *n1_dev;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < n1; r += (long long)gridDim.x * 4) {
    const int2 ri = rowinfo[r];
    const int a = (ri.y < 0 ? -ri.y : ri.y) - 1;
    const float* x = configs + (long long)ri.x * N;
    const int2 ij = bonds[a];
    const float si = x[ij.x], sj = x[ij.y];
    double d = 0.0, self = 0.0;
    int n = 0;
    for (int b0 = 0; b0 < n_bonds; b0 += 64) {
      const SecondOrder s = second_order(x, bonds, half_jx, quarter_jz, n_bonds, a, ij, si, sj, b0 + lane);
      d = fma(s.qz, s.ss, d);
      if (s.self) self += (double)s.hx;
      n += __popcll(__ballot(s.emit));
    }
    d = wave_sum_f64(d);
    self = wave_sum_f64(self);
    if (lane == 0) { cnt2[r] = n; diag1[r] = d; self1[r] = self; }
  }
}

// One workgroup: off2[r] = sum of cnt2[0 .. r) for r <= *n1_dev (tile_scan_1024, measure_dev.hpp)
__global__ __launch_bounds__(1024) void k_mom_scan(const int* __restrict__ cnt2, const int* __restrict__ n1_dev,
                                                   int* __restrict__ off2) {
  __shared__ int s_wave[16];
  tile_scan_1024(cnt2, *n1_dev, off2, s_wave);
}

// One wavefront per first-order row (grid-stride); a row whose part of the list misses the pass [q0, q0 + n) leaves at
// once.  desc[q - q0] = {first-order row, b}, coef[q - q0] = hx_a hx_b (rule 3) or 2 hx_a hx_b (rule 2), exact in fp64
__global__ __launch_bounds__(256) void k_mom_fill(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                  const float* __restrict__ half_jx, const float* __restrict__ quarter_jz,
                                                  const int2* __restrict__ rowinfo, const int* __restrict__ n1_dev,
                                                  const int* __restrict__ off2, int N, int n_bonds, long long q0, int n,
                                                  int2* __restrict__ desc, double* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int n1 = *n1_dev;
  const long long q1 = q0 + n;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < n1; r += (long long)gridDim.x * 4) {
    long long q = off2[r];
    if (off2[r + 1] <= q0 || q >= q1) continue;
    const int2 ri = rowinfo[r];
    const int a = (ri.y < 0 ? -ri.y : ri.y) - 1;
    const float* x = configs + (long long)ri.x * N;
    const int2 ij = bonds[a];
    const float si = x[ij.x], sj = x[ij.y];
    const double hxa = (double)half_jx[a];
    for (int b0 = 0; b0 < n_bonds; b0 += 64) {
      const int b = b0 + lane;
      const SecondOrder s = second_order(x, bonds, half_jx, quarter_jz, n_bonds, a, ij, si, sj, b);
      const unsigned long long m = __ballot(s.emit);
      const long long at = q + lanes_below(m, lane);
      if (s.emit && at >= q0 && at < q1) {
        desc[at - q0] = make_int2((int)r, b);
        coef[at - q0] = (s.rule == 2 ? 2.0 : 1.0) * hxa * (double)s.hx;
      }
      q += __popcll(m);
    }
  }
}

// One wavefront per row of the pass: x^{ab} of its chain.  The lanes run along the site axis.
__global__ __launch_bounds__(256) void k_mom_rows(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                  const int2* __restrict__ rowinfo, const int2* __restrict__ desc, int N,
                                                  int n, float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < n; it += (long long)gridDim.x * 4) {
    const int2 rb = desc[it];
    const int2 ri = rowinfo[rb.x];
    const int a = (ri.y < 0 ? -ri.y : ri.y) - 1;
    const float* x = configs + (long long)ri.x * N;
    const int2 ij = bonds[a], kl = bonds[rb.y];
    const float si = x[ij.x], sj = x[ij.y];
    const float sk = spin_after(x, kl.x, ij, si, sj), sl = spin_after(x, kl.y, ij, si, sj);
    write_exchanged_row(rows + it * N, x, N, lane, ij, si, sj, true, kl, sk, sl, true);      // x^a, then b on x^a
  }
}

// One wavefront per chain: the rows of the pass [q0, q0 + n) that are the chain's, into lanes[c][64] (file header)
__global__ __launch_bounds__(256) void k_mom_accum(const float* __restrict__ logit, const float* __restrict__ sign,
                                                   const float* __restrict__ row_logit, const float* __restrict__ row_sign,
                                                   const double* __restrict__ coef, const int* __restrict__ off,
                                                   const int* __restrict__ off2, int B, long long q0, int n,
                                                   double* __restrict__ lanes) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= B) return;
  const long long s = off2[off[c]], e = off2[off[c + 1]];
  const long long lo = s > q0 ? s : q0, hi = e < q0 + n ? e : q0 + n;
  if (lo >= hi) return;
  const int own = sign ? sgn_of(sign[c]) : 1;
  if (own == 0) return;
  const double own_logit = (double)logit[c];
  long long q = plan_moment_first_row(s, lo, lane);             // the first row >= lo at place = lane (mod 64)
  if (q >= hi) return;
  double acc = lanes[(long long)c * 64 + lane];
  for (; q < hi; q += 64) acc = fma(coef[q - q0], measure_ratio(row_logit, row_sign, q - q0, own_logit, own), acc);
  lanes[(long long)c * 64 + lane] = acc;
}

// One wavefront per chain: chain[c] = e(x_c) and chain[B + c] = g(x_c) in fp64 (0 where the chain's own amplitude vanishes)
__global__ __launch_bounds__(256) void k_mom_chain(const float* __restrict__ configs, const int2* __restrict__ bonds,
                                                   const float* __restrict__ half_jx, const float* __restrict__ quarter_jz,
                                                   const int2* __restrict__ rowinfo, const int* __restrict__ off,
                                                   const float* __restrict__ val, const float* __restrict__ eloc,
                                                   const float* __restrict__ sign, const double* __restrict__ diag1,
                                                   const double* __restrict__ self1, const double* __restrict__ lanes, int B,
                                                   int N, int n_bonds, double* __restrict__ chain) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= B) return;
  if (sign && sgn_of(sign[c]) == 0) {
    if (lane == 0) { chain[c] = 0.0; chain[(long long)B + c] = 0.0; }
    return;
  }
  const float* x = configs + (long long)c * N;
  double d = 0.0;
  for (int b = lane; b < n_bonds; b += 64) {
    const int2 kl = bonds[b];
    d = fma((double)quarter_jz[b], (double)(x[kl.x] * x[kl.y]), d);
  }
  d = wave_sum_f64(d);
  double u = lanes[(long long)c * 64 + lane];
  const int r1 = off[c + 1];
  for (int r = off[c] + lane; r < r1; r += 64) {
    const int ya = rowinfo[r].y;
    const int a = (ya < 0 ? -ya : ya) - 1;
    u = fma((double)val[r], diag1[r], u);
    u = fma((double)half_jx[a], self1[r], u);
  }
  u = wave_sum_f64(u);
  if (lane == 0) {
    const double e = (double)eloc[c];
    chain[c] = e;
    chain[(long long)B + c] = fma(d, e, u);
  }
}

// One wavefront.  out[0 .. 6) = sum e, sum e^2, sum g, sum e g, sum g^2, the chains alive; lane j adds term j of the
// chains in strictly ascending order (64 chains per load, handed round by broadcasts)
__global__ __launch_bounds__(64) void k_mom_sums(const double* __restrict__ chain, const float* __restrict__ sign, int B,
                                                 double* __restrict__ out) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int c0 = 0; c0 < B; c0 += 64) {
    const int c = c0 + lane;
    const double e = c < B ? chain[c] : 0.0, g = c < B ? chain[(long long)B + c] : 0.0;
    const int alive = c < B && (!sign || sgn_of(sign[c]) != 0) ? 1 : 0;
    const int m = B - c0 < 64 ? B - c0 : 64;
    for (int k = 0; k < m; ++k) {
      const double ek = __shfl(e, k, 64), gk = __shfl(g, k, 64);
      if (!__shfl(alive, k, 64)) continue;
      const double term = lane == 0 ? ek : lane == 1 ? __dmul_rn(ek, ek) : lane == 2 ? gk : lane == 3 ? __dmul_rn(ek, gk)
                        : lane == 4 ? __dmul_rn(gk, gk) : 1.0;
      s = __dadd_rn(s, term);
    }
  }
  if (lane < 6) out[lane] = s;
}

hipError_t launch_mom_count(hipStream_t s, const float* configs, const int2* bonds, const float* half_jx,
                            const float* quarter_jz, const int2* rowinfo, const int* n1_dev, int n1, int N, int n_bonds,
                            int num_cus, int* cnt2, int* off2, double* diag1, double* self1) {
  hipLaunchKernelGGL(k_mom_count, dim3(measure_rows_grid(n1, num_cus)), dim3(256), 0, s, configs, bonds, half_jx, quarter_jz,
                     rowinfo, n1_dev, N, n_bonds, cnt2, diag1, self1);
  hipLaunchKernelGGL(k_mom_scan, dim3(1), dim3(1024), 0, s, cnt2, n1_dev, off2);
  return hipGetLastError();
}

hipError_t launch_mom_fill(hipStream_t s, const float* configs, const int2* bonds, const float* half_jx,
                           const float* quarter_jz, const int2* rowinfo, const int* n1_dev, int n1, const int* off2, int N,
                           int n_bonds, long long q0, int n, int num_cus, int2* desc, double* coef) {
  hipLaunchKernelGGL(k_mom_fill, dim3(measure_rows_grid(n1, num_cus)), dim3(256), 0, s, configs, bonds, half_jx, quarter_jz,
                     rowinfo, n1_dev, off2, N, n_bonds, q0, n, desc, coef);
  return hipGetLastError();
}

hipError_t launch_mom_rows(hipStream_t s, const float* configs, const int2* bonds, const int2* rowinfo, const int2* desc,
                           int N, int n, int num_cus, float* rows) {
  hipLaunchKernelGGL(k_mom_rows, dim3(measure_rows_grid(n, num_cus)), dim3(256), 0, s, configs, bonds, rowinfo, desc, N, n,
                     rows);
  return hipGetLastError();
}

hipError_t launch_mom_accum(hipStream_t s, AmpPair own, AmpPair rows, const double* coef, const int* off, const int* off2,
                            int B, long long q0, int n, double* lanes) {
  hipLaunchKernelGGL(k_mom_accum, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, own.logit, own.sign, rows.logit, rows.sign,
                     coef, off, off2, B, q0, n, lanes);
  return hipGetLastError();
}

hipError_t launch_mom_fold(hipStream_t s, const float* configs, const int2* bonds, const float* half_jx,
                           const float* quarter_jz, const int2* rowinfo, const int* off, const float* val, const float* eloc,
                           const float* sign, const double* diag1, const double* self1, const double* lanes, int B, int N,
                           int n_bonds, double* chain, double* out) {
  hipLaunchKernelGGL(k_mom_chain, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, configs, bonds, half_jx, quarter_jz, rowinfo,
                     off, val, eloc, sign, diag1, self1, lanes, B, N, n_bonds, chain);
  hipLaunchKernelGGL(k_mom_sums, dim3(1), dim3(64), 0, s, chain, sign, B, out);
  return hipGetLastError();
}
