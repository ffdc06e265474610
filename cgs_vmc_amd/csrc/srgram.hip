// Sample-space stochastic reconfiguration (MinSR, the "kernel trick").  With n stored samples, centred
// log-derivatives Obar = O - 1 obar^T and eps_b = E_b - Ebar, the update of sr.hip is also
//
//   x = Obar^T (Obar Obar^T + n lambda I)^-1 eps = O^T C (C T C + n lambda I)^-1 eps,   T = O O^T,  C v = v - mean(v)
//
// an n x n system whose matrix-vector product does not depend on the number of parameters.  T is formed from the dense
// sample store without forming O: per layer the weight block of O_b is a_{l-1}[b] (x) delta_l[b] and the bias block
// delta_l[b], so
//
//   T[b][b'] = sum_l (a_{l-1}[b] . a_{l-1}[b'] + 1) (delta_l[b] . delta_l[b'])  +  (a_last[b] . a_last[b'] + 1)
//
// two Gram products per layer joined by a Hadamard product (k_sr_gram).  The conjugate gradients on C T C + n lambda I
// (k_sr_gram_matvec and the single-workgroup length-n kernels) follow the recurrence of sr.hip: x0 = 0, scalars in fp64,
// every sum in a fixed order.  The last step, x = sum_b t_b O_b with t = y - ybar, is the weighted sum of the
// parameter-space matvec (vmc_api_sr.hip).
#include "common.hpp"

// acc[m][q] += X[i0 + wr 32 + m 16 + ..][0 .. K) . X[j0 + wc 64 + q 16 + ..][0 .. K): one wave's 32 x 64 part of a
// Gram tile on v_mfma_f32_16x16x4_f32.  Both operands are row panels, K contiguous: lane l supplies row (l & 15) of
// its 16-row block and, in the MFMA e of a 16-column group, column 4 (l >> 4) + e -- the same column on both sides,
// which is all the sum over k needs; the chunks and the columns inside them come in ascending order for every tile.
// Rows >= n and columns >= K are staged as zeros (nothing is read there).  The next chunk's global loads are in
// flight, in registers, under the MFMAs of the current one.
#define SRG_THREADS 512
#define SRG_PASSES (SRG_TILE * SRG_KC / SRG_THREADS)      // rows of a panel per staging thread
__device__ __forceinline__ void gram_accumulate(const float* __restrict__ X, long long ldx, int K, int i0, int j0, int n,
                                                float (*sI)[SRG_LD], float (*sJ)[SRG_LD], f32x4 (&acc)[2][4]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ra = (w >> 1) * 32 + fr, rb = (w & 1) * 64 + fr;
  const int sc = tid & (SRG_KC - 1), sr = tid / SRG_KC;          // staging: 32 columns x 16 rows per pass
  float pi[SRG_PASSES], pj[SRG_PASSES];
  auto fetch = [&](int k0) {
    const int k = k0 + sc;
#pragma unroll
    for (int u = 0; u < SRG_PASSES; ++u) {
      const int gi = i0 + sr + u * (SRG_THREADS / SRG_KC), gj = j0 + sr + u * (SRG_THREADS / SRG_KC);
      pi[u] = (gi < n && k < K) ? X[(long long)gi * ldx + k] : 0.f;
      pj[u] = (gj < n && k < K) ? X[(long long)gj * ldx + k] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += SRG_KC) {
    __syncthreads();                                             // the previous chunk (or product) has been read
#pragma unroll
    for (int u = 0; u < SRG_PASSES; ++u) {
      sI[sr + u * (SRG_THREADS / SRG_KC)][sc] = pi[u];
      sJ[sr + u * (SRG_THREADS / SRG_KC)][sc] = pj[u];
    }
    __syncthreads();
    if (k0 + SRG_KC < K) fetch(k0 + SRG_KC);
#pragma unroll
    for (int kg = 0; kg < SRG_KC; kg += 16) {
      f32x4 a[2], b[4];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const f32x4*>(&sI[ra + 16 * m][kg + 4 * fq]);
#pragma unroll
      for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const f32x4*>(&sJ[rb + 16 * q][kg + 4 * fq]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][e], b[q][e], acc[m][q], 0, 0, 0);
    }
  }
}

// One workgroup (eight waves as 4 x 2) per 128 x 128 tile (i, j), j >= i, of the uncentred T [n][n]; the layer terms in
// table order, the output / onsite term (no delta: GA + 1) last.  The tile goes to (i, j) and, from the same registers,
// to (j, i); on a diagonal tile only the elements on and above the diagonal are written (and mirrored).
__global__ __launch_bounds__(SRG_THREADS) void k_sr_gram(SrGramArgs g) {
  __shared__ __attribute__((aligned(16))) float sI[SRG_TILE][SRG_LD];
  __shared__ __attribute__((aligned(16))) float sJ[SRG_TILE][SRG_LD];
  static_assert(SRG_TILE == 128 && SRG_KC == 32 && SRG_TILE * SRG_KC % SRG_THREADS == 0, "the wave layout below");
  int ti, tj;
  plan_sr_gram_tile(blockIdx.x, g.nt, &ti, &tj);
  const int i0 = ti * SRG_TILE, j0 = tj * SRG_TILE, n = g.n;
  f32x4 t[2][4], ga[2][4], gd[2][4];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) t[m][q] = zero;
  for (int l = 0; l < g.n_terms; ++l) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) ga[m][q] = gd[m][q] = zero;
    gram_accumulate(g.a[l], g.lda[l], g.ka[l], i0, j0, n, sI, sJ, ga);
    if (g.d[l]) {
      gram_accumulate(g.d[l], g.ldd[l], g.kd[l], i0, j0, n, sI, sJ, gd);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) t[m][q][e] += (ga[m][q][e] + 1.f) * gd[m][q][e];
    } else {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) t[m][q][e] += ga[m][q][e] + 1.f;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = i0 + (w >> 1) * 32 + 16 * m + 4 * fq + e;      // C/D map: row = 4 (lane >> 4) + e, col = lane & 15
        const int c = j0 + (w & 1) * 64 + 16 * q + fr;
        if (r < n && c < n && (ti != tj || c >= r)) {
          g.T[(long long)r * n + c] = t[m][q][e];
          g.T[(long long)c * n + r] = t[m][q][e];
        }
      }
}

hipError_t launch_sr_gram(hipStream_t s, const SrGramArgs& g, long long grid) {
  hipLaunchKernelGGL(k_sr_gram, dim3((unsigned)grid), dim3(SRG_THREADS), 0, s, g);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the conjugate gradients on C T C + n lambda I
// sc (double[4]) = [rr, rr of the first residual, iterations done, 1 once the solve has stopped].  The host enqueues
// iterations in groups and reads sc between them; an iteration enqueued behind the stop does nothing.
// The six vectors of the recurrence (y, r, p, C p, w, q) and every sum are fp64: T stays fp32 -- a fixed, symmetric
// rounding of the operator, which the recurrence follows as it would the exact one -- but fp32 vectors round anew in
// every iteration, and conjugate gradients answer that with delayed convergence: measured 17 .. 28 % more iterations
// than the fp64 recurrence at 129 .. 1100 samples, 5 % off in x after 13 of them.  Rounding C p to fp32
// for the matvec alone undoes all of it (restated on the CPU), so the matvec reads v and sums in fp64: the same time
// per launch at n = 4,096, 6 % more at 8,192, 30 % more at 16,384.

__device__ __forceinline__ double wave_sum_g(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// the sum over the workgroup (1024 threads) in a fixed order, to every thread
__device__ __forceinline__ double block_sum_g(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int d = 512; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// w = T v: one wave per row, 16-byte loads of T where the rows are 16-byte aligned (n a multiple of 4), lane partials
// in ascending column order folded by the xor butterfly
__global__ __launch_bounds__(256) void k_sr_gram_matvec(const float* __restrict__ T, const double* __restrict__ v, int n,
                                                        const double* __restrict__ sc, double* __restrict__ w) {
  if (sc && sc[3] != 0.0) return;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* t = T + (long long)row * n;
  double s = 0.0;
  if ((n & 3) == 0) {
    const float4* t4 = reinterpret_cast<const float4*>(t);
    for (int k = lane; k < (n >> 2); k += 64) {
      const float4 a = t4[k];
      const double* b = v + 4 * k;
      s = fma((double)a.x, b[0], s); s = fma((double)a.y, b[1], s); s = fma((double)a.z, b[2], s); s = fma((double)a.w, b[3], s);
    }
  } else {
    for (int k = lane; k < n; k += 64) s = fma((double)t[k], v[k], s);
  }
  s = wave_sum_g(s);
  if (lane == 0) w[row] = s;
}

hipError_t launch_sr_gram_matvec(hipStream_t s, const float* T, const double* v, int n, const double* sc, double* w) {
  hipLaunchKernelGGL(k_sr_gram_matvec, dim3((n + 3) / 4), dim3(256), 0, s, T, v, n, sc, w);
  return hipGetLastError();
}

// right-hand side: eps = E - Ebar; y = 0, r = p = eps, pc = C p; sc = [|eps|^2, |eps|^2, 0, stop]
__global__ __launch_bounds__(1024) void k_srg_rhs(const float* __restrict__ e, int n, float tol, double* __restrict__ y,
                                                  double* __restrict__ r, double* __restrict__ p, double* __restrict__ pc,
                                                  double* __restrict__ sc) {
  __shared__ double s[1024];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) a += (double)e[i];
  const double ebar = block_sum_g(a, s) / n;
  double rr = 0.0, ps = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double f = (double)e[i] - ebar;
    y[i] = 0.0; r[i] = f; p[i] = f;
    rr += f * f; ps += f;
  }
  rr = block_sum_g(rr, s);
  const double pbar = block_sum_g(ps, s) / n;
  for (int i = threadIdx.x; i < n; i += 1024) pc[i] = p[i] - pbar;
  if (threadIdx.x == 0) {
    sc[0] = rr; sc[1] = rr; sc[2] = 0.0;
    sc[3] = (rr > 0.0 && rr > (double)tol * (double)tol * rr) ? 0.0 : 1.0;
  }
}

// one iteration behind w = T (C p): q = C w + n lambda p; alpha = rr / p.q; y += alpha p; r -= alpha q;
// beta = rr' / rr; p = r + beta p; pc = C p
__global__ __launch_bounds__(1024) void k_srg_step(const double* __restrict__ w, int n, double nlambda, float tol,
                                                   double* __restrict__ q, double* __restrict__ y, double* __restrict__ r,
                                                   double* __restrict__ p, double* __restrict__ pc, double* __restrict__ sc) {
  __shared__ double s[1024];
  if (sc[3] != 0.0) return;
  const double rr = sc[0], rr0 = sc[1];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) a += w[i];
  const double wbar = block_sum_g(a, s) / n;
  a = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double qi = (w[i] - wbar) + nlambda * p[i];
    q[i] = qi;
    a += p[i] * qi;
  }
  const double pq = block_sum_g(a, s);
  const double alpha = pq > 0.0 ? rr / pq : 0.0;
  a = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    y[i] += alpha * p[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    a += ri * ri;
  }
  const double rr1 = block_sum_g(a, s);
  const double beta = rr > 0.0 ? rr1 / rr : 0.0;
  a = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double pi = r[i] + beta * p[i];
    p[i] = pi;
    a += pi;
  }
  const double pbar = block_sum_g(a, s) / n;
  for (int i = threadIdx.x; i < n; i += 1024) pc[i] = p[i] - pbar;
  if (threadIdx.x == 0) {
    sc[0] = rr1; sc[2] += 1.0;
    if (!(rr1 > (double)tol * (double)tol * rr0)) sc[3] = 1.0;
  }
}

// t = y - ybar: the per-sample weights of x = sum_b t_b O_b (fp32, as sr_weighted_sum takes them)
__global__ __launch_bounds__(1024) void k_srg_centre(const double* __restrict__ y, int n, float* __restrict__ t) {
  __shared__ double s[1024];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) a += y[i];
  const double ybar = block_sum_g(a, s) / n;
  for (int i = threadIdx.x; i < n; i += 1024) t[i] = (float)(y[i] - ybar);
}

hipError_t launch_srg_rhs(hipStream_t s, const float* e, int n, float tol, double* y, double* r, double* p, double* pc,
                          double* sc) {
  hipLaunchKernelGGL(k_srg_rhs, dim3(1), dim3(1024), 0, s, e, n, tol, y, r, p, pc, sc);
  return hipGetLastError();
}

hipError_t launch_srg_step(hipStream_t s, const double* w, int n, double nlambda, float tol, double* q, double* y, double* r,
                           double* p, double* pc, double* sc) {
  hipLaunchKernelGGL(k_srg_step, dim3(1), dim3(1024), 0, s, w, n, nlambda, tol, q, y, r, p, pc, sc);
  return hipGetLastError();
}

hipError_t launch_srg_centre(hipStream_t s, const double* y, int n, float* t) {
  hipLaunchKernelGGL(k_srg_centre, dim3(1), dim3(1024), 0, s, y, n, t);
  return hipGetLastError();
}
