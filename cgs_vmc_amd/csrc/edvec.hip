// FullVector ('ed_vector', wavefunctions.py:1001-1080) for gfx950: psi(x) = v[top_t[top(x)] + bot_t[bot(x)]], one entry of
// a trainable state vector addressed through Lin's two tables.  bit i of bot = [s_i > 0] (i < N/2), bit i of top =
// [s_{N/2+i} > 0]; a configuration is one 32-bit word (bot in the low N/2 bits).  Nothing here is arithmetic: every
// kernel is dependent gathers -- table, table, vector -- and the gradient is a scatter into 2 P floats.
//   k_edvec_rows   one thread per row: psi (the gathered entry, bit for bit) and ln|psi| (-inf at psi = 0)
//   k_edvec_sweep  persistent sampler: one thread per chain keeps word, psi and step counter in registers for all
//                  n_steps; the two tables sit in LDS where plan_edvec_tables_in_lds says so
//   k_edvec_eloc   one wave per chain, one antiparallel bond per lane: the gathers of a chain are in flight together
//   k_edvec_keys / rocPRIM radix sort / k_edvec_segsum: the gradient scatter.  (idx << 32 | chain) keys are sorted, the
//                  first thread of every run of equal idx sums its chains in chain order (double) and adds once into
//                  g1 / g2: distinct runs write distinct entries, so there is no atomic and no arrival order
// A row that is not at Sz = 0 (a ctx whose chains were never set) or whose index leaves the vector reads nothing:
// psi = NaN.  vmc_set_lin_tables has checked every Sz = 0 configuration (plan_edvec_check_tables).
#include "common.hpp"

#include <rocprim/rocprim.hpp>

namespace {

// key bits the sort has to look at: the chain in the low word, above it an index of [0, len] -- len itself marks a chain
// that contributes nothing (psi = 0 or NaN) and sorts behind every entry
inline int ed_key_bits(int len) {
  int bits = 0;
  while (bits < 31 && (1ll << bits) <= (long long)len) ++bits;
  return 32 + bits;
}

// spins [N] (+-1 floats) -> word
__device__ __forceinline__ uint32_t ed_word(const float* __restrict__ x, int N) {
  uint32_t w = 0;
  for (int i = 0; i < N; ++i) w |= (x[i] > 0.f ? 1u : 0u) << i;
  return w;
}

// the entry of `word`, or -1 where the word is not at Sz = 0 or the tables send it outside [0, len)
__device__ __forceinline__ int ed_index(uint32_t word, int N, const int* __restrict__ top, const int* __restrict__ bot,
                                        int len) {
  const int h = N >> 1;
  if (__popc(word) != h) return -1;
  const long long idx = (long long)top[word >> h] + (long long)bot[word & ((1u << h) - 1u)];
  return idx >= 0 && idx < len ? (int)idx : -1;
}

__device__ __forceinline__ float ed_gather(uint32_t word, int N, const int* __restrict__ top,
                                           const int* __restrict__ bot, const float* __restrict__ vec, int len) {
  const int idx = ed_index(word, N, top, bot, len);
  return idx >= 0 ? vec[idx] : __builtin_nanf("");
}

// ln|psi| rounded once from the double-precision logarithm (-inf at psi = 0): logf is 2 ulp off near |psi| = 1, where
// ln|psi| is small; one value per row or chain, so its cost does not show
__device__ __forceinline__ float ed_logit(float p) { return (float)log((double)fabsf(p)); }

}  // namespace

__global__ __launch_bounds__(256) void k_edvec_rows(const float* __restrict__ vec, int len, const int* __restrict__ top,
                                                    const int* __restrict__ bot, int N,
                                                    const float* __restrict__ configs, int n_rows,
                                                    float* __restrict__ logit, float* __restrict__ psi) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const float p = ed_gather(ed_word(configs + (long long)r * N, N), N, top, bot, vec, len);
  psi[r] = p;
  logit[r] = ed_logit(p);
}

__global__ __launch_bounds__(1024) void k_edvec_sweep(EdvecSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) int ed_lds[];
  const int N = a.N, h = N >> 1, n_half = 1 << h;
  const int* top = a.top;
  const int* bot = a.bot;
  if (a.tables_lds) {
    for (int i = threadIdx.x; i < n_half; i += blockDim.x) { ed_lds[i] = a.top[i]; ed_lds[n_half + i] = a.bot[i]; }
    __syncthreads();
    top = ed_lds; bot = ed_lds + n_half;
  }
  // (threads past the last chain shadow it and write nothing: the wave stays whole for the final count)
  const bool mine = (int)(blockIdx.x * blockDim.x + threadIdx.x) < a.B;
  const int ch = mine ? (int)(blockIdx.x * blockDim.x + threadIdx.x) : a.B - 1;
  uint32_t word = ed_word(a.configs_in + (long long)ch * N, N);
  const bool live = __popc(word) == h;        // (false only for chains never set: nothing moves)
  float psi = ed_gather(word, N, top, bot, a.vec, a.len);
  unsigned cnt = 0;
  const uint2 key = make_uint2(a.seed_lo, a.seed_hi);
  const uint32_t gid = (uint32_t)(a.chain_offset + ch);
  const int nblk = (N + 3) >> 2;
  for (long long st = 0; st < a.n_steps; ++st) {
    const unsigned long long step = a.step0 + (unsigned long long)st;
    int iu, id;
    float uu;
    if (a.inj_up) {
      iu = a.inj_up[ch]; id = a.inj_dn[ch]; uu = a.inj_u[ch];
    } else {
      // graph_builders.py:59-65 in k_wide_propose's arithmetic (wide.hip): the same proposals as every other sampler.
      // Sites in ascending order with strict comparisons: the largest / smallest value at its smallest index
      float best_hi = -INFINITY, best_lo = INFINITY;
      iu = id = 0x7fffffff;
      for (int bk = 0; bk < nblk; ++bk) {
        const uint4 rn = philox4x32_10(make_uint4((uint32_t)bk, gid, (uint32_t)step, (uint32_t)(step >> 32)), key);
        const uint32_t rr[4] = {rn.x, rn.y, rn.z, rn.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * bk + e;
          if (i < N) {
            const float v = ((word >> i) & 1u ? 1.f : -1.f) * u32_to_uniform(rr[e]);
            if (v > best_hi) { best_hi = v; iu = i; }
            if (v < best_lo) { best_lo = v; id = i; }
          }
        }
      }
      const uint4 ra = philox4x32_10(make_uint4(VMC_ACCEPT_BLOCK, gid, (uint32_t)step, (uint32_t)(step >> 32)), key);
      uu = u32_to_uniform(ra.x);
    }
    bool acc = false;
    // (a move that would not exchange an up with a down spin -- ties at u = 0 -- leaves the chain alone)
    if (live && iu >= 0 && iu < N && id >= 0 && id < N && ((word >> iu) & 1u) && !((word >> id) & 1u)) {
      const uint32_t cand = word ^ (1u << iu) ^ (1u << id);     // graph_builders.py:67-71
      const float pc = ed_gather(cand, N, top, bot, a.vec, a.len);
      // graph_builders.py:75-79 with the reference's IEEE behaviour at zeros: psi' = 0 gives 0 (or 0/0 = NaN) and
      // rejects, psi = 0 with psi' != 0 gives inf and accepts
      const float q = __fdiv_rn(pc, psi);
      acc = __fmul_rn(q, q) > uu;
      if (acc) { word = cand; psi = pc; }
    }
    cnt += acc ? 1u : 0u;
    if (a.acc_mask && mine) a.acc_mask[ch] = acc ? 1 : 0;
  }
  if (mine) {
    for (int i = 0; i < N; ++i)
      a.configs_out[(long long)ch * N + i] = live ? ((word >> i) & 1u ? 1.f : -1.f) : a.configs_in[(long long)ch * N + i];
    a.psi_out[ch] = psi;
    a.logit_out[ch] = ed_logit(psi);
  }
  // one add per wave (integers: the total does not depend on the order)
  unsigned wsum = mine ? cnt : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d);
  if (a.accepted && (threadIdx.x & 63) == 0 && wsum) atomicAdd(a.accepted, (unsigned long long)wsum);
}

// val[q] = 0.5 jx psi(x')/psi(x) of every row {chain, +-(bond + 1)} of the antiparallel-bond list (k_bond_fill,
// eloc.hip); k_eloc_reduce then folds each chain's rows in its fixed order.  undivided_at_zero (the base of a symmetrized
// ctx): a chain with psi(x) = 0 gets 0.5 jx psi(x') itself, so that its off-diagonal sum is (H psi)(x) -- what the
// composite's fold needs of an op whose row hits a zero entry
__global__ __launch_bounds__(256) void k_edvec_eloc(const float* __restrict__ vec, int len, const int* __restrict__ top,
                                                    const int* __restrict__ bot, int N,
                                                    const float* __restrict__ configs, const float* __restrict__ psi,
                                                    int B, const int* __restrict__ off,
                                                    const int2* __restrict__ rowinfo, const int2* __restrict__ bonds,
                                                    const float* __restrict__ half_jx, int undivided_at_zero,
                                                    float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= B) return;
  const int r0 = off[ch], r1 = off[ch + 1];
  if (r0 == r1) return;
  const uint32_t word = (uint32_t)__ballot(lane < N && configs[(long long)ch * N + (lane < N ? lane : 0)] > 0.f);
  const float p = psi[ch];
  for (int q = r0 + lane; q < r1; q += 64) {
    const int kb = abs(rowinfo[q].y) - 1;
    const int2 ij = bonds[kb];
    const float pc = ed_gather(word ^ (1u << ij.x) ^ (1u << ij.y), N, top, bot, vec, len);
    val[q] = __fmul_rn(half_jx[kb], undivided_at_zero && p == 0.f ? pc : __fdiv_rn(pc, p));      // operators.py:166-168; psi = 0: the reference's x / 0
  }
}

// ratio_b = (psi_w - beta H psi_w) / psi (training.py:665-672) on the amplitudes themselves: no exponent shift
__global__ void k_edvec_itswo_ratio(const float* __restrict__ psi, const float* __restrict__ psi_w,
                                    const float* __restrict__ ew, float beta, int B, float* __restrict__ ratio) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  ratio[i] = __fmul_rn(__fdiv_rn(psi_w[i], psi[i]), __fsub_rn(1.f, __fmul_rn(beta, ew[i])));
}

__global__ __launch_bounds__(256) void k_edvec_keys(const int* __restrict__ top, const int* __restrict__ bot, int N,
                                                    int len, const float* __restrict__ configs,
                                                    const float* __restrict__ psi, int B,
                                                    unsigned long long* __restrict__ keys) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float p = psi[b];
  int idx = ed_index(ed_word(configs + (long long)b * N, N), N, top, bot, len);
  if (idx < 0 || !(p != 0.f)) idx = len;                     // O_k = delta(k, idx) / psi: nothing at psi = 0 (or NaN)
  keys[b] = ((unsigned long long)(uint32_t)idx << 32) | (uint32_t)b;
}

__global__ __launch_bounds__(256) void k_edvec_segsum(const unsigned long long* __restrict__ keys,
                                                      const float* __restrict__ psi, const float* __restrict__ w, int B,
                                                      int len, float* __restrict__ g1, float* __restrict__ g2) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= B) return;
  const uint32_t idx = (uint32_t)(keys[t] >> 32);
  if (idx >= (uint32_t)len || (t > 0 && (uint32_t)(keys[t - 1] >> 32) == idx)) return;    // not the head of a run
  double s1 = 0.0, s2 = 0.0;
  for (int j = t; j < B && (uint32_t)(keys[j] >> 32) == idx; ++j) {                        // chains in ascending order
    const int b = (int)(uint32_t)keys[j];
    const double p = (double)psi[b];
    s1 += 1.0 / p;
    s2 += (double)w[b] / p;
  }
  g1[idx] += (float)s1;
  g2[idx] += (float)s2;
}

hipError_t launch_edvec_rows(hipStream_t st, const float* vec, int len, const int* top, const int* bot, int N,
                             const float* configs, int n_rows, float* logit, float* psi) {
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_edvec_rows, dim3((n_rows + 255) / 256), dim3(256), 0, st, vec, len, top, bot, N, configs, n_rows,
                     logit, psi);
  return hipGetLastError();
}

// Once per ctx, on its device: tables past 64 KB of LDS (N = 28) need the sampler's dynamic limit raised.
hipError_t edvec_sweep_reserve_lds(int N) {
  const size_t lds = plan_edvec_tables_bytes(N);
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)k_edvec_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t launch_edvec_sweep(hipStream_t st, EdvecSweepArgs a, int num_cus) {
  if (a.B <= 0) return hipSuccess;
  const int threads = plan_edvec_sweep_threads(a.B, num_cus);
  const size_t lds = a.tables_lds ? plan_edvec_tables_bytes(a.N) : 0;
  hipLaunchKernelGGL(k_edvec_sweep, dim3(plan_edvec_sweep_grid(a.B, threads)), dim3(threads), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_edvec_eloc(hipStream_t st, const float* vec, int len, const int* top, const int* bot, int N,
                             const float* configs, const float* psi, int B, const int* off, const int2* rowinfo,
                             const int2* bonds, const float* half_jx, int undivided_at_zero, float* val) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_edvec_eloc, dim3((B + 3) / 4), dim3(256), 0, st, vec, len, top, bot, N, configs, psi, B, off,
                     rowinfo, bonds, half_jx, undivided_at_zero, val);
  return hipGetLastError();
}

hipError_t launch_edvec_itswo_ratio(hipStream_t st, const float* psi, const float* psi_omega, const float* eloc_omega,
                                    float beta, int B, float* ratio) {
  hipLaunchKernelGGL(k_edvec_itswo_ratio, dim3((B + 255) / 256), dim3(256), 0, st, psi, psi_omega, eloc_omega, beta, B,
                     ratio);
  return hipGetLastError();
}

hipError_t edvec_sort_bytes(int B, int len, size_t* bytes) {
  unsigned long long* none = nullptr;
  return rocprim::radix_sort_keys(nullptr, *bytes, none, none, (size_t)B, 0, ed_key_bits(len), (hipStream_t) nullptr);
}

hipError_t launch_edvec_grad(hipStream_t st, const int* top, const int* bot, int N, int len, const float* configs,
                             const float* psi, const float* w, int B, unsigned long long* keys,
                             unsigned long long* keys_sorted, void* sort_tmp, size_t sort_bytes, float* g1, float* g2) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_edvec_keys, dim3((B + 255) / 256), dim3(256), 0, st, top, bot, N, len, configs, psi, B, keys);
  hipError_t e = rocprim::radix_sort_keys(sort_tmp, sort_bytes, keys, keys_sorted, (size_t)B, 0, ed_key_bits(len), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_edvec_segsum, dim3((B + 255) / 256), dim3(256), 0, st, (const unsigned long long*)keys_sorted,
                     psi, w, B, len, g1, g2);
  return hipGetLastError();
}
