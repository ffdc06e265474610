// ProjectedBDG (wavefunctions.py:876-928) on gfx950: the Gutzwiller-projected BCS state psi(x) = det M(x),
// M[r][c] = F[U_r][D_c] over the up sites U and the down sites D of x (ascending; the reference's boolean_mask order).
//
// Every kernel here keeps one chain (or one row) per wave, its matrix in LDS (plan_pbdg_*: n = N/2 <= 128, an odd row
// stride, up to four chains per workgroup):
//   k_pbdg_rows   logit = ln|det M| and sign(det M) of arbitrary rows by Gauss-Jordan elimination with partial pivoting
//                 (optionally M^-1 and the slot of every site, for the gradient sums);
//   k_pbdg_sweep  the sampler: n_steps mc_steps of graph_builders.py:38-89 per launch, M^-1 resident in LDS, each
//                 proposal's ratio from a 2 x 2 determinant in O(n^2), a rank-2 update of M^-1 per accepted move, a fresh
//                 factorisation at launch start and every plan_pbdg_refresh_interval accepted moves;
//   k_pbdg_eloc   the local energies: a fresh M^-1 per chain, then one O(n^2) ratio per antiparallel bond of the row list;
//   k_pbdg_grad_* O_ik = d ln|psi| / d F_ik = M^-1[pos k][pos i] summed over the chains in which i is up and k down, in
//                 chain slices of a fixed order and folded in slice order (no float atomics).
//
// Exchange ratio.  The sampler keeps the rows / columns of M in slot order: U slot r holds an up site, D slot c a down
// site.  Exchanging the up site a (slot r) with the down site b (slot c) puts b into U slot r and a into D slot c, which
// changes row r and column c of M: M' = M + e_r x^T + y e_c^T with
//   x_j = F[b][D_j] - F[a][D_j] (j != c),  x_c = F[b][a] - F[a][b];   y_i = F[U_i][a] - F[U_i][b] (i != r),  y_r = 0,
// so det M' / det M = det K, K = [[1 + x.M^-1[:, r], x.M^-1.y], [M^-1[c, r], 1 + M^-1[c, :].y]] (rows of M^-1 are D slots,
// its columns U slots) and M'^-1 = M^-1 - [M^-1[:, r], M^-1 y] K^-1 [x^T M^-1; M^-1[c, :]].  Slot order differs from the
// sorted order of the amplitude by a permutation whose sign changes by (-1)^(|a-b|-1) per exchange (every site strictly
// between a and b is up or down): the local energies, which start from sorted slots, apply it; the sampler compares
// |det K| only and leaves its logits and signs to a k_pbdg_rows launch on the final chains (vmc_api_sweep.hip), which
// is what makes the cache identical to vmc_amplitude's.
#include "pb_det.hpp"

namespace {

// det K of exchanging the up site a (U slot r) with the down site b (D slot c), from M^-1 in s.A (header comment);
// leaves x, y, M^-1 y in s.vx / s.vy / s.a1 and K in k[4] for pb_update
__device__ float pb_ratio(const float* __restrict__ F, int N, int n, int ld, PbChain& s, int lane, int a, int b, int r,
                          int c, float* k) {
  const float* fa = F + (long long)a * N;
  const float* fb = F + (long long)b * N;
  for (int j = lane; j < n; j += 64) {
    s.vx[j] = j == c ? fb[a] - fa[b] : fb[s.dn[j]] - fa[s.dn[j]];
    const float* fu = F + (long long)s.up[j] * N;
    s.vy[j] = j == r ? 0.f : fu[a] - fu[b];
  }
  float k00 = 0.f, k01 = 0.f;
  for (int i = lane; i < n; i += 64) {
    const float* row = s.A + i * ld;
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc = fmaf(row[j], s.vy[j], acc);
    s.a1[i] = acc;
    k00 = fmaf(s.vx[i], row[r], k00);
    k01 = fmaf(s.vx[i], acc, k01);
  }
  k[0] = 1.f + pb_wave_sum(k00);
  k[1] = pb_wave_sum(k01);
  k[2] = s.A[c * ld + r];
  k[3] = 1.f + s.a1[c];
  return k[0] * k[3] - k[1] * k[2];
}

// M^-1 <- M^-1 - [M^-1[:, r], M^-1 y] K^-1 [x^T M^-1; M^-1[c, :]] after pb_ratio of the same move
__device__ void pb_update(int n, int ld, PbChain& s, int lane, int r, int c, const float* k, float det) {
  float b0[2], b1[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = lane + 64 * t;
    b0[t] = b1[t] = 0.f;
    if (j < n) {
      float acc = 0.f;
      for (int i = 0; i < n; ++i) acc = fmaf(s.vx[i], s.A[i * ld + j], acc);
      b0[t] = acc;
      b1[t] = s.A[c * ld + j];
      s.a0[j] = s.A[j * ld + r];
    }
  }
  const float id = 1.f / det;
  const float i00 = k[3] * id, i01 = -k[1] * id, i10 = -k[2] * id, i11 = k[0] * id;
  float t0[2], t1[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    t0[t] = fmaf(i00, b0[t], i01 * b1[t]);
    t1[t] = fmaf(i10, b0[t], i11 * b1[t]);
  }
  __builtin_amdgcn_wave_barrier();
  for (int i = 0; i < n; ++i) {
    const float p0 = s.a0[i], p1 = s.a1[i];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = lane + 64 * t;
      if (j < n) s.A[i * ld + j] -= fmaf(p0, t0[t], p1 * t1[t]);
    }
  }
}


}  // namespace

__global__ __launch_bounds__(256) void k_pbdg_rows(const float* __restrict__ F, int N, int cpw,
                                                   const float* __restrict__ configs, int n_rows,
                                                   float* __restrict__ logit, float* __restrict__ sign,
                                                   float* __restrict__ inv_out, int* __restrict__ pos_out) {
  extern __shared__ __attribute__((aligned(16))) char pb_lds[];
  const int n = N / 2, ld = plan_pbdg_ld(n);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * cpw + w;
  if (row >= n_rows) return;
  PbChain s = pb_carve(pb_lds + (size_t)w * plan_pbdg_chain_lds_bytes(N), N, n, ld);
  pb_load_spins(s, configs + row * N, N, lane);
  float lg = __builtin_nanf(""), sg = 0.f;
  const bool ok = pb_lists(s, N, n, lane);          // (the host refuses rows with nonzero magnetisation)
  if (ok) sg = pb_factor(F, N, n, ld, s, lane, &lg);
  if (lane == 0) { logit[row] = lg; sign[row] = sg; }
  if (inv_out && ok) {
    float* o = inv_out + row * n * n;
    for (int c = 0; c < n; ++c)
      for (int r = lane; r < n; r += 64) o[c * n + r] = sg != 0.f ? s.A[c * ld + r] : 0.f;
    for (int i = lane; i < N; i += 64) pos_out[row * N + i] = s.pos[i];
  }
}

__global__ __launch_bounds__(256) void k_pbdg_sweep(PbdgSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) char pb_lds[];
  const int N = a.N, n = N / 2, ld = plan_pbdg_ld(n);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ch = blockIdx.x * a.cpw + w;
  if (ch >= a.B) return;
  PbChain s = pb_carve(pb_lds + (size_t)w * plan_pbdg_chain_lds_bytes(N), N, n, ld);
  pb_load_spins(s, a.configs_in + (long long)ch * N, N, lane);
  float lg = 0.f, sg = 0.f;
  const bool listed = pb_lists(s, N, n, lane);        // (false only for chains never set: all spins 0, nothing moves)
  if (listed) sg = pb_factor(a.F, N, n, ld, s, lane, &lg);
  bool singular = sg == 0.f;
  int since = 0;
  unsigned cnt = 0;
  const uint2 key = make_uint2(a.seed_lo, a.seed_hi);
  const uint32_t gid = (uint32_t)(a.chain_offset + ch);
  for (long long st = 0; st < a.n_steps; ++st) {
    const unsigned long long step = a.step0 + (unsigned long long)st;
    int iu, id;
    float uu;
    if (a.inj_up) {
      iu = a.inj_up[ch]; id = a.inj_dn[ch]; uu = a.inj_u[ch];
    } else {
      // graph_builders.py:59-65 in k_wide_propose's arithmetic (wide.hip): the same proposals as every other sampler
      float best_hi = -INFINITY, best_lo = INFINITY;
      int idx_hi = 0x7fffffff, idx_lo = 0x7fffffff;
      const int nblk = (N + 3) >> 2;
      for (int bk = lane; bk < nblk; bk += 64) {
        const uint4 rn = philox4x32_10(make_uint4((uint32_t)bk, gid, (uint32_t)step, (uint32_t)(step >> 32)), key);
        const uint32_t rr[4] = {rn.x, rn.y, rn.z, rn.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * bk + e;
          if (i < N) {
            const float v = s.x[i] * u32_to_uniform(rr[e]);
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
      const uint4 ra = philox4x32_10(make_uint4(VMC_ACCEPT_BLOCK, gid, (uint32_t)step, (uint32_t)(step >> 32)), key);
      iu = idx_hi; id = idx_lo; uu = u32_to_uniform(ra.x);
    }
    bool acc = false;
    // (a move that would not exchange an up with a down spin -- ties at u = 0 -- leaves the chain alone)
    if (listed && iu >= 0 && iu < N && id >= 0 && id < N && s.x[iu] > 0.f && s.x[id] < 0.f) {
      const int r = s.pos[iu], c = s.pos[id];
      if (singular) {
        // psi = 0: |psi'| / |psi| is +inf (accept) where psi' != 0 and NaN (reject) where psi' = 0 -- factorise the candidate
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) { s.up[r] = id; s.dn[c] = iu; }
        float lg2 = 0.f;
        if (pb_factor(a.F, N, n, ld, s, lane, &lg2) != 0.f) {
          acc = true; singular = false; since = 0;
        } else if (lane == 0) {
          s.up[r] = iu; s.dn[c] = id;
        }
      } else {
        float k[4];
        const float det = pb_ratio(a.F, N, n, ld, s, lane, iu, id, r, c, k);
        acc = fabsf(det) > sqrtf(uu);                    // graph_builders.py:75-79
        if (acc) {
          pb_update(n, ld, s, lane, r, c, k, det);
          ++since;
          if (since >= a.refresh || !(fabsf(det) >= PLAN_PBDG_TINY_RATIO)) since = -1;   // refresh below
        }
      }
      if (acc) {
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
          s.up[r] = id; s.dn[c] = iu; s.pos[id] = r; s.pos[iu] = c;
          s.x[iu] = -1.f; s.x[id] = 1.f;                 // graph_builders.py:67-71
        }
        if (since < 0) {
          float lg2 = 0.f;
          pb_lists(s, N, n, lane);
          singular = pb_factor(a.F, N, n, ld, s, lane, &lg2) == 0.f;
          since = 0;
        }
      }
    }
    cnt += acc ? 1u : 0u;
    if (a.acc_mask && lane == 0) a.acc_mask[ch] = acc ? 1 : 0;
  }
  for (int i = lane; i < N; i += 64) a.configs_out[(long long)ch * N + i] = s.x[i];
  if (lane == 0 && cnt && a.accepted) atomicAdd(a.accepted, (unsigned long long)cnt);
}

// 0.5 jx psi(x')/psi(x) of every row {chain, +-(bond + 1)} of the antiparallel-bond list (k_bond_fill, eloc.hip)
__global__ __launch_bounds__(256) void k_pbdg_eloc(const float* __restrict__ F, int N, int cpw,
                                                   const float* __restrict__ configs, int B,
                                                   const int* __restrict__ off, const int2* __restrict__ rowinfo,
                                                   const int2* __restrict__ bonds, const float* __restrict__ half_jx,
                                                   float* __restrict__ val) {
  extern __shared__ __attribute__((aligned(16))) char pb_lds[];
  const int n = N / 2, ld = plan_pbdg_ld(n);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ch = blockIdx.x * cpw + w;
  if (ch >= B) return;
  const int r0 = off[ch], r1 = off[ch + 1];
  if (r0 == r1) return;
  PbChain s = pb_carve(pb_lds + (size_t)w * plan_pbdg_chain_lds_bytes(N), N, n, ld);
  pb_load_spins(s, configs + (long long)ch * N, N, lane);
  float lg = 0.f, sg = 0.f;
  if (pb_lists(s, N, n, lane)) sg = pb_factor(F, N, n, ld, s, lane, &lg);
  for (int q = r0; q < r1; ++q) {
    const int2 ri = rowinfo[q];
    const int kb = (ri.y > 0 ? ri.y : -ri.y) - 1;
    const int2 ij = bonds[kb];
    const int a = ri.y > 0 ? ij.x : ij.y, b = ri.y > 0 ? ij.y : ij.x;   // a up, b down
    float v = __builtin_nanf("");                         // psi = 0: the reference's x / 0
    if (sg != 0.f) {
      float k[4];
      const float det = pb_ratio(F, N, n, ld, s, lane, a, b, s.pos[a], s.pos[b], k);
      const int dist = a > b ? a - b : b - a;
      v = half_jx[kb] * (((dist - 1) & 1) ? -det : det);
    }
    if (lane == 0) val[q] = v;
  }
}

// partial sums of O_ik and w_b O_ik over the chains of slice blockIdx.y, in chain order
__global__ __launch_bounds__(256) void k_pbdg_grad_part(const float* __restrict__ configs, const int* __restrict__ pos,
                                                        const float* __restrict__ inv, const float* __restrict__ w,
                                                        int B, int N, int slices, double* __restrict__ ws) {
  const long long P = (long long)N * N;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= P) return;
  const int n = N / 2, sl = blockIdx.y;
  const int b0 = (int)((long long)B * sl / slices), b1 = (int)((long long)B * (sl + 1) / slices);
  const int i = (int)(q / N), k = (int)(q % N);
  double s1 = 0.0, s2 = 0.0;
  for (int b = b0; b < b1; ++b) {
    const float* x = configs + (long long)b * N;
    if (x[i] > 0.f && x[k] < 0.f) {
      const int* p = pos + (long long)b * N;
      const int pk = p[k], pi = p[i];
      if ((unsigned)pk < (unsigned)n && (unsigned)pi < (unsigned)n) {     // (always, for a chain at Sz = 0)
        const double v = (double)inv[(long long)b * n * n + (long long)pk * n + pi];
        s1 += v;
        s2 += (double)w[b] * v;
      }
    }
  }
  ws[(2LL * sl) * P + q] = s1;
  ws[(2LL * sl + 1) * P + q] = s2;
}

__global__ __launch_bounds__(256) void k_pbdg_grad_fold(const double* __restrict__ ws, int slices, long long P,
                                                        float* __restrict__ g1, float* __restrict__ g2) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= P) return;
  double s1 = 0.0, s2 = 0.0;
  for (int sl = 0; sl < slices; ++sl) {
    s1 += ws[(2LL * sl) * P + q];
    s2 += ws[(2LL * sl + 1) * P + q];
  }
  g1[q] += (float)s1;
  g2[q] += (float)s2;
}

// ratio_b = (psi_w - beta H psi_w) / psi (training.py:665-672) with signed amplitudes:
//         = sign_w sign_psi exp(logit_w - logit_psi + shift_psi - shift_w) (1 - beta E_loc^w)
__global__ void k_pbdg_itswo_ratio(const float* __restrict__ lp, const float* __restrict__ sp,
                                   const float* __restrict__ lw, const float* __restrict__ sw,
                                   const float* __restrict__ ew, float log_factor, float beta, int B,
                                   float* __restrict__ ratio) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  ratio[i] = sw[i] * sp[i] * expf(lw[i] - lp[i] + log_factor) * (1.f - beta * ew[i]);
}

// max of the logits of the chains with psi > 0 (-inf when there is none): log(max_b psi_b) + shift of update_norm
__global__ __launch_bounds__(1024) void k_pbdg_signed_max(const float* __restrict__ logit, const float* __restrict__ sign,
                                                          int B, float* __restrict__ out) {
  __shared__ float sm[1024];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < B; i += 1024)
    if (sign[i] > 0.f && logit[i] > m) m = logit[i];
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int d = 512; d >= 1; d >>= 1) {
    if (threadIdx.x < d) sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + d]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sm[0];
}

hipError_t launch_pbdg_rows(hipStream_t st, const float* F, int N, const float* configs, int n_rows, float* logit,
                            float* sign, float* inv_out, int* pos_out) {
  if (n_rows <= 0) return hipSuccess;
  const int cpw = plan_pbdg_chains_per_wg(N);
  const size_t lds = (size_t)cpw * plan_pbdg_chain_lds_bytes(N);
  hipError_t e = pb_allow_lds(k_pbdg_rows, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pbdg_rows, dim3((n_rows + cpw - 1) / cpw), dim3(64 * cpw), lds, st, F, N, cpw, configs, n_rows,
                     logit, sign, inv_out, pos_out);
  return hipGetLastError();
}

hipError_t launch_pbdg_sweep(hipStream_t st, PbdgSweepArgs a) {
  if (a.B <= 0) return hipSuccess;
  a.cpw = plan_pbdg_chains_per_wg(a.N);
  a.refresh = plan_pbdg_refresh_interval(a.N);
  const size_t lds = (size_t)a.cpw * plan_pbdg_chain_lds_bytes(a.N);
  hipError_t e = pb_allow_lds(k_pbdg_sweep, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pbdg_sweep, dim3((a.B + a.cpw - 1) / a.cpw), dim3(64 * a.cpw), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_pbdg_eloc(hipStream_t st, const float* F, int N, const float* configs, int B, const int* off,
                            const int2* rowinfo, const int2* bonds, const float* half_jx, float* val) {
  if (B <= 0) return hipSuccess;
  const int cpw = plan_pbdg_chains_per_wg(N);
  const size_t lds = (size_t)cpw * plan_pbdg_chain_lds_bytes(N);
  hipError_t e = pb_allow_lds(k_pbdg_eloc, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pbdg_eloc, dim3((B + cpw - 1) / cpw), dim3(64 * cpw), lds, st, F, N, cpw, configs, B, off,
                     rowinfo, bonds, half_jx, val);
  return hipGetLastError();
}

hipError_t launch_pbdg_grad(hipStream_t st, const float* configs, const int* pos, const float* inv, const float* w,
                            int B, int N, int slices, double* ws, float* g1, float* g2) {
  const long long P = (long long)N * N;
  const unsigned blocks = (unsigned)((P + 255) / 256);
  hipLaunchKernelGGL(k_pbdg_grad_part, dim3(blocks, (unsigned)slices), dim3(256), 0, st, configs, pos, inv, w, B, N,
                     slices, ws);
  hipLaunchKernelGGL(k_pbdg_grad_fold, dim3(blocks), dim3(256), 0, st, (const double*)ws, slices, P, g1, g2);
  return hipGetLastError();
}

hipError_t launch_pbdg_itswo_ratio(hipStream_t st, const float* logit_psi, const float* sign_psi,
                                   const float* logit_omega, const float* sign_omega, const float* eloc_omega,
                                   float log_factor, float beta, int B, float* ratio) {
  hipLaunchKernelGGL(k_pbdg_itswo_ratio, dim3((B + 255) / 256), dim3(256), 0, st, logit_psi, sign_psi, logit_omega,
                     sign_omega, eloc_omega, log_factor, beta, B, ratio);
  return hipGetLastError();
}

hipError_t launch_pbdg_signed_max(hipStream_t st, const float* logit, const float* sign, int B, float* out) {
  hipLaunchKernelGGL(k_pbdg_signed_max, dim3(1), dim3(1024), 0, st, logit, sign, B, out);
  return hipGetLastError();
}
