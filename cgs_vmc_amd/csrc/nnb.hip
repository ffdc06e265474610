// FullyConnectedNNB (wavefunctions.py:931-998) on gfx950: neural-network backflow.  A dense relu trunk maps the
// configuration x to a pairing matrix of its own, F(x) = out.reshape(N, N), and psi(x) = det M(x) with
// M[r][c] = F(x)[U_r][D_c] over the up sites U and the down sites D of x in ascending order (the convention of pbdg.hip).
//
// The trunk and the pairing layer run on the general dense path (wide.hip, the fp32-MFMA GEMMs of grad.hip): the host
// (vmc_api*.hip, nnb_forward) walks the rows in blocks of plan_nnb_block_rows and leaves the pairing layer of a block
// as a dense [rows][N^2] matrix.  The kernels here take it from there:
//   k_nnb_rows        one wave per row: the row's configuration (a chain, or a chain with one bond exchanged), its sorted
//                     up / down lists, the n x n gather M out of the row's pairing layer into LDS, and the elimination
//                     of pb_det.hpp: logit = ln|det M| and sign(det M); as a local-energy row the term
//                     0.5 jx sign' sign exp(logit' - logit); on the gradient path the row of the pairing layer is
//                     overwritten by d ln|psi| / d out = (M^-1)^T scattered to the (up, down) entries, zero elsewhere;
//   k_nnb_candidates  the proposed configuration of every chain;
//   k_nnb_accept      the Metropolis test in the logit domain and the in-place update of chains, logits and signs.
// Every amplitude stays (logit, sign): ratios are logit differences, psi = sign exp(logit) is formed on the host only.
#include "pb_det.hpp"

// block: the rows [0, n_rows) the pointers below are already offset to
__global__ __launch_bounds__(256) void k_nnb_rows(NnbRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char pb_lds[];
  const int N = a.N, n = N / 2, ld = plan_pbdg_ld(n);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * a.cpw + w;
  if (row >= a.n_rows) return;
  PbChain s = pb_carve(pb_lds + (size_t)w * plan_pbdg_chain_lds_bytes(N), N, n, ld);
  // the row's configuration: chain ri.x, with the two sites of bond |ri.y| - 1 exchanged when ri.y != 0
  const int2 ri = a.rowinfo[row];
  int fa = -1, fb = -1, kb = 0;
  if (ri.y != 0) {
    kb = (ri.y > 0 ? ri.y : -ri.y) - 1;
    const int2 ab = a.bonds[kb];
    fa = ab.x; fb = ab.y;
  }
  const float* cfg = a.configs + (long long)ri.x * N;
  for (int i = lane; i < N; i += 64) {
    const float v = cfg[i];
    s.x[i] = (i == fa || i == fb) ? -v : v;
  }
  float lg = __builtin_nanf(""), sg = 0.f;
  const bool ok = pb_lists(s, N, n, lane);          // (the host refuses rows with nonzero magnetisation)
  float* orow = a.out + row * a.ldo;
  if (ok) {
    float scale = 0.f;
    for (int r = 0; r < n; ++r) {
      const float* fr = orow + (long long)s.up[r] * N;
      for (int c = lane; c < n; c += 64) {
        const float v = fr[s.dn[c]];
        s.A[r * ld + c] = v;
        scale = fmaxf(scale, fabsf(v));
      }
    }
    sg = pb_eliminate(n, ld, s, lane, scale, &lg);
  }
  if (lane == 0) {
    if (a.val) {
      // psi(x') / psi(x) = sign' sign exp(logit' - logit); psi(x) = 0: the reference's x / 0
      const float sb = a.sign_base[ri.x];
      float v = __builtin_nanf("");
      if (ok && sb != 0.f) v = sg == 0.f ? 0.f : a.half_jx[kb] * (sg * sb) * expf(lg - a.logit_base[ri.x]);
      a.val[row] = v;
    } else {
      a.logit[row] = lg; a.sign[row] = sg;
    }
  }
  if (a.write_delta) {
    // every entry of the row is written once: (M^-1)[c][r] at (U_r, D_c), zero elsewhere (and for a singular M)
    const int NN = N * N;
    const bool live = ok && sg != 0.f;
    for (int j = lane; j < NN; j += 64) {
      const int i = j / N, k = j - i * N;
      float v = 0.f;
      if (live && s.x[i] > 0.f && s.x[k] < 0.f) v = s.A[s.pos[k] * ld + s.pos[i]];
      orow[j] = v;
    }
  }
}

// cand[ch] = chain ch with the proposed pair exchanged (iup -> down, idn -> up); a proposal that would not exchange an
// up with a down spin -- ties at u = 0 -- leaves the copy as it is (k_nnb_accept rejects it)
__global__ __launch_bounds__(256) void k_nnb_candidates(const float* __restrict__ configs, const int* __restrict__ iup,
                                                        const int* __restrict__ idn, int B, int N,
                                                        float* __restrict__ cand) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)B * N) return;
  const int ch = (int)(q / N), i = (int)(q - (long long)ch * N);
  const float* x = configs + (long long)ch * N;
  const int u = iup[ch], d = idn[ch];
  float v = x[i];
  if (u >= 0 && u < N && d >= 0 && d < N && x[u] > 0.f && x[d] < 0.f && (i == u || i == d)) v = -v;
  cand[q] = v;
}

// graph_builders.py:75-88 in the logit domain: accept where |psi'|^2 / |psi|^2 > u, i.e. exp(logit' - logit) > sqrt(u)
// (strict); a singular candidate is rejected, a chain at psi = 0 accepts any nonsingular candidate.  One wave per chain.
__global__ __launch_bounds__(256) void k_nnb_accept(float* __restrict__ configs, const float* __restrict__ cand,
                                                    const int* __restrict__ iup, const int* __restrict__ idn,
                                                    const float* __restrict__ u, float* __restrict__ logit,
                                                    float* __restrict__ sign, const float* __restrict__ lcand,
                                                    const float* __restrict__ scand, int B, int N,
                                                    unsigned char* __restrict__ acc_mask,
                                                    unsigned long long* __restrict__ accepted) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= B) return;
  float* x = configs + (long long)ch * N;
  const int iu = iup[ch], id = idn[ch];
  bool acc = false;
  if (iu >= 0 && iu < N && id >= 0 && id < N && x[iu] > 0.f && x[id] < 0.f) {
    const float sc = scand[ch], lc = lcand[ch];
    if (sc != 0.f) acc = sign[ch] == 0.f ? true : expf(lc - logit[ch]) > sqrtf(u[ch]);
    if (acc) {
      __builtin_amdgcn_wave_barrier();
      for (int i = lane; i < N; i += 64) x[i] = cand[(long long)ch * N + i];
      if (lane == 0) { logit[ch] = lc; sign[ch] = sc; }
    }
  }
  if (lane == 0) {
    if (acc_mask) acc_mask[ch] = acc ? 1 : 0;
    if (acc && accepted) atomicAdd(accepted, 1ull);
  }
}

hipError_t launch_nnb_rows(hipStream_t st, NnbRowsArgs a) {
  if (a.n_rows <= 0) return hipSuccess;
  a.cpw = plan_pbdg_chains_per_wg(a.N);
  const size_t lds = (size_t)a.cpw * plan_pbdg_chain_lds_bytes(a.N);
  hipError_t e = pb_allow_lds(k_nnb_rows, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_nnb_rows, dim3((unsigned)((a.n_rows + a.cpw - 1) / a.cpw)), dim3(64 * a.cpw), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_nnb_candidates(hipStream_t st, const float* configs, const int* iup, const int* idn, int B, int N,
                                 float* cand) {
  if (B <= 0) return hipSuccess;
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(k_nnb_candidates, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, configs, iup, idn, B, N,
                     cand);
  return hipGetLastError();
}

hipError_t launch_nnb_accept(hipStream_t st, float* configs, const float* cand, const int* iup, const int* idn,
                             const float* u, float* logit, float* sign, const float* lcand, const float* scand, int B,
                             int N, unsigned char* acc_mask, unsigned long long* accepted) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_nnb_accept, dim3((B + 3) / 4), dim3(256), 0, st, configs, cand, iup, idn, u, logit, sign, lcand,
                     scand, B, N, acc_mask, accepted);
  return hipGetLastError();
}
