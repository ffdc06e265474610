// The determinant core shared by pbdg.hip and nnb.hip: one wave keeps an n x n matrix (n = N/2 <= 128) in LDS with an odd
// row stride (plan_pbdg_*), lists the up / down sites of a configuration in ascending order and inverts the matrix in
// place, which gives ln|det M|, sign(det M) and M^-1.
#pragma once
#include "common.hpp"

namespace {

// one wave's slices of the workgroup's LDS (plan_pbdg_chain_lds_bytes)
struct PbChain {
  float* A;                       // [n][ld]: M, then M^-1 (rows: D slots, columns: U slots)
  float *vx, *vy, *a1, *a0;       // [n] x, y, M^-1 y, M^-1[:, r]
  float* x;                       // [N] spins
  int *up, *dn, *perm;            // [n] slot lists, pivot rows
  int* pos;                       // [N] slot of every site (in U or in D)
};

__device__ __forceinline__ PbChain pb_carve(char* base, int N, int n, int ld) {
  PbChain s;
  float* f = (float*)base;
  s.A = f; f += n * ld;
  s.vx = f; f += n; s.vy = f; f += n; s.a1 = f; f += n; s.a0 = f; f += n;
  f += 2 * n;                     // (the planner's two spare vectors: b0 and M^-1[c, :] stay in registers)
  s.x = f; f += N;
  int* i = (int*)f;
  s.up = i; i += n; s.dn = i; i += n; s.perm = i; i += n; s.pos = i;
  return s;
}

__device__ __forceinline__ float pb_wave_sum(float v) {
  // butterfly: every lane ends with the same bits (each stage adds the same two values)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// sorted slot lists of the spins in s.x; false unless there are exactly n up and n down spins
__device__ bool pb_lists(PbChain& s, int N, int n, int lane) {
  int nu = 0, nd = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    const float v = i < N ? s.x[i] : 0.f;
    const unsigned long long mu = __ballot(v > 0.f), md = __ballot(v < 0.f);
    if (v > 0.f) { const int r = nu + __popcll(mu & below); if (r < n) { s.up[r] = i; s.pos[i] = r; } }
    if (v < 0.f) { const int c = nd + __popcll(md & below); if (c < n) { s.dn[c] = i; s.pos[i] = c; } }
    nu += __popcll(mu); nd += __popcll(md);
  }
  return nu == n && nd == n;
}

// In place M^-1 of the n x n matrix in s.A by Gauss-Jordan elimination with partial pivoting (the row of largest
// magnitude, the lowest index among equals); `scale` is this lane's max |M| over the entries it wrote.  Returns
// sign(det M) (0 when singular -- a pivot below n eps32 max|M| --, s.A is then garbage) and *logit = ln|det M| (-inf
// when singular).  Every lane returns the same values.
// Two equal rows of M (two equal rows of F, both sites up) stay equal bit for bit until one of them is the pivot row;
// the other is then cancelled exactly (its multiplier is 1: `twin` below), so a later pivot search meets a zero column
// and psi = 0 comes out exactly, as from the oracle's LU.  Through the scaled pivot row the cancellation would leave
// eps32 |M| per entry, which the remaining steps amplify by about kappa of the other rows: at n = 65 that residue
// reached the last pivot at 2.5 times the threshold.
__device__ float pb_eliminate(int n, int ld, PbChain& s, int lane, float scale, float* logit) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) scale = fmaxf(scale, __shfl_xor(scale, m));
  // a pivot below n eps32 max|M| is rounding noise: singular
  const float tiny = scale * (float)n * 1.1920929e-7f;
  double lsum = 0.0;
  float sg = 1.f;
  for (int k = 0; k < n; ++k) {
    float best = -1.f;
    int bi = n;
    for (int i = k + lane; i < n; i += 64) {
      const float v = fabsf(s.A[i * ld + k]);
      if (v > best) { best = v; bi = i; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ob = __shfl_xor(best, m);
      const int oi = __shfl_xor(bi, m);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (!(best > tiny)) { *logit = -INFINITY; return 0.f; }    // (a NaN entry lands here too)
    if (lane == 0) s.perm[k] = bi;
    if (bi != k) {
      for (int j = lane; j < n; j += 64) {
        const float t = s.A[k * ld + j];
        s.A[k * ld + j] = s.A[bi * ld + j];
        s.A[bi * ld + j] = t;
      }
      sg = -sg;
    }
    const float piv = s.A[k * ld + k];
    if (piv < 0.f) sg = -sg;
    lsum += log((double)fabsf(piv));
    const float ip = 1.f / piv;
    float rk[2], ru[2];                      // the pivot row, scaled by 1 / pivot and as it was
    unsigned long long twin[2];              // rows whose multiplier is exactly 1 (almost always none)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = lane + 64 * t;
      rk[t] = ru[t] = 0.f;
      twin[t] = __ballot(j < n && j != k && s.A[j * ld + k] == piv);
      if (j < n) {
        ru[t] = j == k ? 1.f : s.A[k * ld + j];
        const float v = ru[t] * ip;
        s.A[k * ld + j] = v;
        rk[t] = v;
      }
    }
    if ((twin[0] | twin[1]) == 0ull) {
      for (int i = 0; i < n; ++i) {
        if (i == k) continue;
        const float f = s.A[i * ld + k];     // read by every lane before the owner of column k overwrites it
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int j = lane + 64 * t;
          if (j < n) s.A[i * ld + j] = fmaf(-f, rk[t], j == k ? 0.f : s.A[i * ld + j]);
        }
      }
    } else {
      for (int i = 0; i < n; ++i) {
        if (i == k) continue;
        const float f = s.A[i * ld + k];
        const bool same = ((i < 64 ? twin[0] : twin[1]) >> (i & 63)) & 1ull;   // subtract the pivot row as it was
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int j = lane + 64 * t;
          if (j < n) {
            const float v = j == k ? 0.f : s.A[i * ld + j];
            s.A[i * ld + j] = same ? v - ru[t] : fmaf(-f, rk[t], v);
          }
        }
      }
    }
  }
  // the row interchanges of the elimination become column interchanges of the inverse, last first
  for (int k = n - 1; k >= 0; --k) {
    const int p = s.perm[k];
    if (p != k)
      for (int i = lane; i < n; i += 64) {
        const float t = s.A[i * ld + k];
        s.A[i * ld + k] = s.A[i * ld + p];
        s.A[i * ld + p] = t;
      }
  }
  *logit = (float)lsum;
  return sg;
}

// M[r][c] = F[up[r]][dn[c]] into s.A, then in place M^-1 by Gauss-Jordan elimination with partial pivoting (the row of
// largest magnitude, the lowest index among equals).  Returns sign(det M) (0 when singular -- a pivot below n eps32 max|M| --,
// s.A is then garbage) and
// *logit = ln|det M| (-inf when singular).  Every lane returns the same values.
__device__ float pb_factor(const float* __restrict__ F, int N, int n, int ld, PbChain& s, int lane, float* logit) {
  float scale = 0.f;
  for (int r = 0; r < n; ++r) {
    const float* fr = F + (long long)s.up[r] * N;
    for (int c = lane; c < n; c += 64) {
      const float v = fr[s.dn[c]];
      s.A[r * ld + c] = v;
      scale = fmaxf(scale, fabsf(v));
    }
  }
  return pb_eliminate(n, ld, s, lane, scale, logit);
}

__device__ __forceinline__ void pb_load_spins(PbChain& s, const float* __restrict__ cfg, int N, int lane) {
  for (int i = lane; i < N; i += 64) s.x[i] = cfg[i];
}

template <typename K>
hipError_t pb_allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace
