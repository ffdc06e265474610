// Internal header of the host side of libcgsvmc_hip.so (round 6: vmc_api.hip split by kernel path behind the same
// include/cgsvmc.h): the ctx, the entry-point macros, the small inline helpers and the prototypes of what the
// translation units vmc_api*.hip share.  Not installed; nothing outside csrc/ includes it.
// Which family of kernels a ctx runs is ONE member, vmc_ctx::path (enum KernelPath, plan.hpp): code that differs by
// family switches over it without a `default`, yes/no questions go through plan.hpp's path_* predicates.  The ctx holds
// no per-family flag beside it; rbm (orthogonal to the path) and sgn (on a product: the OR of its factors) stay.
#pragma once
#include "../../include/cgsvmc.h"
#include "common.hpp"
#include "conv.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <string>
#include <utility>
#include <vector>

// The owner of one device allocation: every device buffer of a ctx (and every local scratch buffer of an entry point) is a
// DevBuf, freed by its destructor -- vmc_destroy is `delete c`, no list names the buffers.  It converts to T*, so call
// sites read like a raw pointer (function templates that deduce T* take .p); kernel argument structs keep raw pointers.
// alloc(c, n, name): exactly n elements (at least one); whatever was held is freed first, after a synchronisation of the
// stream (work in flight may read the old buffer).  reserve(c, n, name): grow-only -- a no-op while n <= cap, otherwise
// alloc; the contents are not kept, `grew` tells.  A failed allocation leaves the buffer empty (cap 0) and names it in
// the message.  (Definitions: the end of this file.)
template <class T>
struct DevBuf {
  T* p = nullptr;
  long long cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  int alloc(vmc_ctx* c, long long n, const char* name);
  int reserve(vmc_ctx* c, long long n, const char* name, bool* grew = nullptr);
  void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};

namespace vmcapi {


extern std::string g_create_error;   // vmc_api.hip

struct ParamSet {
  DevBuf<float> theta;
  DevBuf<float> w1p, b1p, bh, p16, p16t,
        woutp, bout, won;
  DevBuf<float> z1;     // [B][Hp] cache for the ctx's chains
  DevBuf<float> onsite; // [B] cached x . w_on (RBM)
  DevBuf<float> logit;  // [B]
  DevBuf<float> sign;   // [B] pbdg: sign(det M) of the chains (+-1, 0 singular); psi = sign exp(logit - shift); ed_vector: psi itself
  // psi only: the buffers the NEXT sampler launch writes (see vmc_ctx::configs_alt)
  DevBuf<float> z1_alt, onsite_alt, logit_alt, sign_alt;
  DevBuf<float> eloc;   // [B]
  // convolutional ansatz types: fragment images of conv.hpp ConvParams
  DevBuf<float> cw0, cwf, cwb, cbias;
  DevBuf<unsigned> p16s;   // CGS_VMC_SPLIT_BF16=1: the H x H layers as three bf16 terms (tail_split.hip)
  // bond-difference table of k_tail16 (launch_bond_diff): the differences of the packed w1p / won over the bond
  // list `bdiff_bonds`.  Rebuilt by launch_rows when the image was re-packed (ensure_packed clears bdiff_valid) or
  // another bond list is current (vmc_set_bonds and the spin-correlation passes bump vmc_ctx::bonds_epoch)
  DevBuf<float> bdiff, bdiff_on;
  long long bdiff_cap = 0;            // rows allocated
  bool bdiff_valid = false;
  unsigned long long bdiff_epoch = 0; // vmc_ctx::bonds_epoch the table was built at
  bool packed_valid = false, cache_valid = false, has_params = false;
  float shift = -10.f;     // wavefunctions.py:209
  PackedParams packed() const { return PackedParams{w1p, b1p, bh, p16, woutp, bout, won}; }
};

struct TimedRegion {
  std::string name;
  hipEvent_t start, stop;
};

}  // namespace vmcapi
using vmcapi::ParamSet;
using vmcapi::TimedRegion;

struct ProdState;      // vmc_api_prod.hip: what a product ctx keeps beside the members below
struct SymzState;      // vmc_api_symz.hip: what a symmetrized ctx keeps beside them

// spin correlations: the bond set of a pass of pairs -- swapped with the five Hamiltonian members of the ctx for the
// pass -- the scatter target, the sums
struct CorrBufs {
  DevBuf<int2> pairs;            // every pair of the call (a pass reads a slice)
  DevBuf<float> hx, qz;          // [pairs per pass] 1 (j_x = 2) and 0 (j_z = 0); these five are the set of a pass
  DevBuf<int2> rowinfo;          // [B pairs per pass]
  DevBuf<float> val, dense;      // [B pairs per pass] rows; [B][pairs of the pass] the rows by (chain, pair)
  DevBuf<double> out;            // [2][n_pairs] zz sums, exchange sums
  void release_pass() { hx.release(); qz.release(); rowinfo.release(); val.release(); dense.release(); }
};
// Renyi-2 swap estimator: the region masks of a call and its sums
struct RenyiBufs {
  DevBuf<unsigned char> mask;    // [n_regions][N] 0/1
  DevBuf<double> out;            // [2][n_regions] swap sums, match counts
};
// symmetry expectation values: the ops of a call and their sums
struct SymmBufs {
  DevBuf<int> perm;              // [n_ops][N] site permutations
  DevBuf<unsigned char> flip;    // [n_ops] 0/1
  DevBuf<double> out;            // [n_ops] ratio sums
};
// symmetry-projected energies: the characters of a call, the per-chain accumulator and the sums (the ops live in SymmBufs)
struct ProjBufs {
  DevBuf<double> chi;            // [n_sectors][n_ops]
  DevBuf<double> acc;            // [n_sectors][B] w_s(c), sector major
  DevBuf<double> out;            // [n_sectors] w sums, [n_sectors] w E_loc sums, the E_loc sum, the chains alive
};
// Lanczos-step energies (moments.hip): per first-order row the count, prefix, diag(x^a) and rule 1's sum; the descriptors
// and coefficients of one pass of second-order rows; the per-chain lanes, e and g; the sums
struct MomentBufs {
  DevBuf<int> cnt2, off2;        // [n1], [n1 + 1]
  DevBuf<double> diag1, self1;   // [n1]
  DevBuf<int2> desc;             // [rows per pass] {first-order row, b}
  DevBuf<double> coef;           // [rows per pass]
  DevBuf<double> lanes;          // [B][64]
  DevBuf<double> chain;          // [2][B] e, g
  DevBuf<double> out;            // [6]
};
// overlap with the frozen set (overlap.hip): per chain ln|omega / psi| and the sign code, the blocks' maxima, the four
// sums and the scaled ratios
struct OverlapBufs {
  DevBuf<double> d;              // [B]
  DevBuf<int> code;              // [B] +-1, 0, OVERLAP_DEAD
  DevBuf<double> bmax;           // [plan_overlap_blocks(B)]
  DevBuf<double> out;            // [4] S1, S2, alive, m
  DevBuf<double> ratio;          // [B] s exp(d - m) (vmc_overlap's per-chain output)
};
// dimer-dimer correlations: the two lists of a call, ln|psi| (and, signed types, the sign) of every single exchange,
// and the sums
struct DimerBufs {
  DevBuf<int2> bonds;            // sites (i, j)
  DevBuf<int2> pairs;            // indices (a, b) into bonds
  DevBuf<float> logit, sign;     // [n_bonds][B]; sign: signed types only
  DevBuf<double> out;            // [n_bonds + n_pairs] bond sums, then dd sums
};

// four-spin (J-Q) terms of the Hamiltonian (fourspin.hip): the term set as vmc_set_four_spin_terms reduced it, the list
// of an evaluation, and the result buffers that span it
struct FourSpinBufs {
  int n_terms = 0, n_pairs = 0;     // n_terms 0: no terms set -- the ctx is what it is without this struct
  int exchange_sign = 1;
  long long rows_per_pass = 0;      // the caller's request (0: the library decides)
  DevBuf<int2> pairs, term_pairs;   // [n_pairs] sites (min, max); [n_terms] indices into pairs
  DevBuf<double> wq;                // [n_terms] -q / 4
  DevBuf<int> n_single, cnt, off;   // [B], [B], [B + 2] (the prefix, then the single rows of all chains)
  DevBuf<int2> desc;                // [rows per pass] {chain, code}
  DevBuf<float> logit, sign;        // [rows of the list]; sign: signed types only
  DevBuf<double> dsum, osum;        // [B] the constant and the ratio part of the chains' term sums (vmc_local_energy_terms)
  bool want_parts = false;          // the evaluation in flight is vmc_local_energy_terms': the fold keeps dsum / osum too
  long long last_single = 0, last_double = 0;   // the list lengths of the last evaluation
};

struct vmc_ctx {
  vmc_desc d;
  // ProductOfWavefunctions (vmc_api_prod.hip, prod.hip): a ctx made by vmc_create_product owns the chains, the accumulators
  // and the Adam state of psi = psi_a psi_b and borrows its two factors (prod: its state; null on every other ctx).  owner:
  // set on a factor while it is composed -- its chain-state entries return VMC_ERR_STATE, its parameter entries invalidate
  // the owner's caches.  The dense members of a product ctx keep minimal shapes (unused); P = P_a + P_b.
  ProdState* prod = nullptr;
  vmc_ctx* owner = nullptr;
  // The symmetrized ansatz (vmc_api_symz.hip, symz.hip): a ctx made by vmc_create_symmetrized owns the chains, the
  // accumulators and the Adam state of psi_s = sum_k chi_k psi(g_k .) and borrows its base, whose `owner` it is (symz: its
  // state; null on every other ctx).  P and theta are the base's.
  SymzState* symz = nullptr;
  KernelPath path = PATH_FUSED;   // the kernel family (plan.hpp); vmc_debug_kernel_path reports it
  int N = 0, B = 0, L = 0, H = 0, Hp = 0;
  bool rbm = false;        // RestrictedBoltzmannNetwork instead of FullyConnectedNetwork
  // PATH_PBDG (pbdg.hip): theta is the pairing matrix; the network members keep minimal shapes (unused).  The
  // gradient path factorises psi on the chains into pbdg_inv [B][n][n] / pbdg_pos [B][N] and folds the partial sums
  // of pbdg_slices chain slices (pbdg_ws, double) in slice order
  DevBuf<float> pbdg_inv; DevBuf<int> pbdg_pos; DevBuf<double> pbdg_ws; int pbdg_slices = 1;
  DevBuf<float> tmp_sign;   // [tmp_rows] signs of vmc_amplitude's rows
  // PATH_NNB (nnb.hip): the general dense path whose output stage is the pairing layer of a
  // block of nnb_rows rows (nnb_out [nnb_rows][N^2], wbuf[] [nnb_rows][Hp]) and the determinant rows kernel.  sgn: signed
  // amplitudes (pbdg, nnb, ed_vector, a product with such a factor: sign buffers, Sz = 0 configurations only).  nnb_delta
  // [B][N^2]: the pairing layer of psi on the chains, overwritten by d ln|psi| / d out (gradient path); nnb_cl / nnb_cs [B]:
  // logits and signs of the sampler's candidates; nnb_wg_slices: K slices of the weight-gradient launch
  bool sgn = false;
  long long nnb_rows = 0;
  DevBuf<float> nnb_out, nnb_delta, nnb_cl, nnb_cs;
  int nnb_wg_slices = 1;
  // PATH_EDVEC (edvec.hip): theta is the state vector, ed_top / ed_bot the Lin tables [2^(N/2)] (null until
  // vmc_set_lin_tables).  ParamSet::sign holds the chains' amplitudes themselves (psi, not a sign), logit = ln|psi|,
  // the shift stays 0.  ed_keys / ed_keys_sorted [B], ed_sort_tmp: the gradient scatter's sort (launch_edvec_grad)
  bool ed_tables_lds = false;
  DevBuf<int> ed_top, ed_bot;
  DevBuf<unsigned long long> ed_keys, ed_keys_sorted;
  DevBuf<unsigned char> ed_sort_tmp; size_t ed_sort_bytes = 0;
  // PATH_CONV / PATH_CONV_GENERAL (conv.hip, conv_general.hip).  The dense-ansatz members below keep harmless minimal
  // shapes (H = filters, Hp = 64, no H x H layer); acts_valid tells whether the forward tapes
  // hold the inputs of every convolution for psi on the current chains.
  ConvGeom cg;
  int cG = 1, cGs = 1;     // samples per workgroup pass of the row / backward kernels, of the sampler
  DevBuf<float> ctape, cdelta, cws;
  long long ctape_stride = 0, cdelta_stride = 0;
  int c_slices = 64;       // sample slices of the weight-gradient kernel
  // more than 256 hidden units (path_wide): the general path's row buffers (wide.hip).  PATH_FUSED_LDS (at most 512
  // units) keeps them for its gradient path only: its sampler and row kernel are instantiations of the fused kernels
  // (k_sweep16<24|32>, k_tail_lds).  CGS_VMC_WIDE_FAST=0 forces PATH_DENSE_GENERAL.
  long long wrows = 0;     // rows of the two activation row buffers
  DevBuf<float> wbuf[2], wide_zero;
  DevBuf<double> wide_dot;          // [ceil(H / 128)][wrows] row-dot partials of the last H x H layer (GemmArgs epilogue 10)
  // PATH_CONV_GENERAL (conv_general.hip; plan.hpp: conv beyond the fused kernels' limits): block buffers
  long long cg_rows = 0;                   // row configurations per block (sized by the im2col matrix: the GEMM form, the gradient path)
  long long cg_rows_fwd = 0;               // ... of an untaped forward whose convolutions all run on the band kernel (sized by the two maps)
  DevBuf<float> cg_A;                   // im2col rows [cg_rows * N][plan_cgen_lda]
  DevBuf<float> cg_fm[2];                // feature maps [cg_rows][N][Fp] (cgen_post: activations; the cosine: pre-activations)
  DevBuf<double> cg_sum;                // [cg_rows] sums of the last map
  DevBuf<float> cg_zero;                // one 0.f (the "b_out" of wide_out_finish)
  DevBuf<float> cg_lnew;                // [B] candidate logits of the sampler
  // the sampler's chain groups (run_sweep_cgen): group 0 on `stream`, the others on streams of their own, so that the
  // partly filled last round of one group's launch runs beside the next launch of another
  hipStream_t cg_grp_stream[3] = {nullptr, nullptr, nullptr};
  hipEvent_t cg_grp_ev[4] = {nullptr, nullptr, nullptr, nullptr};    // [0]: `stream` is ready; [g]: group g has finished
  hipStream_t cg_stream_cur = nullptr;     // the stream cgen_conv / cgen_forward launch on (null: `stream`)
  long long cg_map_row0 = 0;               // first row of cg_fm / cg_A an untaped forward writes (a group's slice)
  DevBuf<float> cg_pmaps;               // [n_conv][B][N][Fp] the chains' maps of every convolution (the patch sampler, conv_patch.hip)
  // ... its gradient path (allocated by the first gradient call): the map of every convolution (the tape), two
  // d logit / d map buffers, per-position weights, the transposed weight images, the split-K workspace
  DevBuf<float> cg_tape, cg_gl, cg_g[2], cg_wpos, cg_wt;
  DevBuf<float> cg_ws; long long cg_ws_floats = 0;
  DevBuf<double> cg_td;                 // [cg_rows] O_b . v of a block (SR)
  long long cg_sr_tape_rows = 0;           // > 0: cg_tape / cg_gl hold the taped forward and the backward of the first that many STORED chains
                                           // at the parameters of the running solve (one block: kept across its CG iterations)
  DevBuf<float> cg_centre;              // [1] mean of O_b . v over the stored samples (SR)
  // gnn (cg.graph): the adjacency list [N][k] and its inverse lists (plan_gnn_inverse: [N + 1] offsets, [N k] entries m k + t),
  // set by vmc_set_adjacency; every compute entry of a gnn ctx refuses to run without them (late_inputs_set)
  DevBuf<int> gnn_adj, gnn_inv_ptr, gnn_inv;
  bool sr_centre = false;                  // the SR matvec may centre its weights: a single-rank solve is running
  bool sr_phase1_done = false;             // vmc_sr_matvec_phase1 has run for the current CG direction (general convolution path)
  // the proposal in flight of the step-at-a-time samplers (dense general, general convolution, nnb): [B] sites, [B] uniforms
  DevBuf<int> prop_iup, prop_idn;
  DevBuf<float> prop_u;
  int hact = VMC_ACT_RELU_;  // hidden activation (layers.NONLINEARITIES id)
  int oact = VMC_ACT_EXP_;   // output activation; exp: psi = exp(x - shift), else psi = g(x), no shift
  DevBuf<float> oscale;   // [B] (1/psi) d psi / d x of a non-exp output activation
  DevBuf<float> dact_all, dact_alt;   // [L][B][Hp] f'(z) next to act_all (cosine only)
  int n_hh = 0;            // H x H layers: L - 1 (FC) or L (RBM)
  int A = 0;               // activation buffers = n_hh + 1
  ParamLayout lay;
  long long P = 0;
  hipStream_t stream = nullptr;
  ParamSet ps[2];
  DevBuf<float> configs;
  // Double-buffered chain state.  A sampler launch reads {configs, z1, logit} and writes
  // {configs_alt, z1_alt, logit_alt, onsite_alt, act_alt}; the two sets are swapped on the host
  // right after the launch.  accumulate(R_t) on `stream` and sweep(R_t -> R_t+1) on
  // `sweep_stream` therefore touch disjoint buffers and run concurrently (training.py:614-617:
  // the two ops of a batch iteration are independent given the chains R_t).
  DevBuf<float> configs_alt;
  DevBuf<float> act_alt;
  int parity = 0;                 // which physical buffer set is current (GEMM tables are per set)
  hipStream_t sweep_stream = nullptr;   // private non-blocking stream of the sampler
  bool overlap = true;            // CGS_VMC_OVERLAP=0: everything on `stream`
  bool overlap_full = false;      // CGS_VMC_OVERLAP=2: overtake even when the sampler fills every CU
  bool side_sweep_once = false;   // the next vmc_mc_steps goes to sweep_stream BEHIND everything enqueued so far, so that
                                  // what follows on `stream` (the accumulator all-reduce of a sharded epoch) runs beside it
  hipEvent_t ev_mark = nullptr;   // recorded on `stream` at the start of the latest accumulate
  hipEvent_t ev_now = nullptr;    // scratch: "everything enqueued on `stream` so far"
  hipEvent_t ev_sweep_done = nullptr;
  bool sweep_pending = false;     // a sampler launch on sweep_stream that `stream` has not waited for
  bool token = false;             // the latest entry point was an accumulate the next sweep may overtake
  bool expect_sweep = false;      // the previous accumulate was overtaken by a sweep: leave it CUs
  bool acc_since_sweep = false;   // a gradient accumulate may follow: the sampler hands over activations
  // Hamiltonian
  // the current bond set: non-owning views -- of the Hamiltonian's buffers (ham_*, vmc_set_bonds), or of a
  // spin-correlation pass's set while that pass runs (install_set, vmc_api_measure.hip)
  int n_bonds = 0;
  int2* bonds = nullptr;
  float *half_jx = nullptr, *quarter_jz = nullptr, *val = nullptr;
  int2* rowinfo = nullptr;
  DevBuf<int2> ham_bonds, ham_rowinfo;
  DevBuf<float> ham_half_jx, ham_quarter_jz, ham_val;
  DevBuf<int> cnt, off;
  DevBuf<float> diag, offdiag;
  DevBuf<int2> bond_dummy;   // {0,0}: stands in for the bond table before vmc_set_bonds
  DevBuf<int2> rowinfo_id;   // identity list {r, 0} for plain rows (cache refresh)
  DevBuf<int2> tmp_rowinfo;
  unsigned long long bonds_epoch = 1;   // bumped whenever `bonds` / `n_bonds` name another list (ParamSet::bdiff)
  bool list_valid = false;
  bool cnt_valid = false;          // cnt / diag hold the census of `configs` (left by the sampler's last launch)
  DevBuf<int> cnt_alt; DevBuf<float> diag_alt;   // the census the NEXT sampler launch writes (swapped with the chains)
  long long last_rows = 0;
  // the measurements (vmc_api_measure.hip); the rows of a Renyi-2 / dimer pass live in the tmp_* buffers of vmc_amplitude
  CorrBufs corr;
  RenyiBufs renyi;
  DimerBufs dimer;
  SymmBufs symm;
  ProjBufs proj;
  MomentBufs mom;
  OverlapBufs ovl;
  FourSpinBufs fs;
  // the Hamiltonian as vmc_set_bonds was given it (vmc_projected_energy asks whether its ops are symmetries of it)
  std::vector<int32_t> ham_ij;
  std::vector<float> ham_jx, ham_jz;
  // gradient path
  std::vector<float*> act;   // L views [B][Hp] into act_all
  DevBuf<float> act_all;  // [L][B][Hp]
  bool acts_valid = false;   // act[] hold the activations of psi on the current chains
  std::vector<float*> delta;   // L views [B][Hp] into delta_all: d logit / d z_l
  DevBuf<float> delta_all;
  DevBuf<unsigned char> d_batch[2][2];   // weight-gradient problem tables [w = eloc / ratio][parity]
  bool batch_ready[2][2] = {{false, false}, {false, false}};
  int wg_tiles = 0;                // MFMA tiles of the weight-gradient launch (plan.hpp)
  bool wg_out_partials = false;    // the output layer's sums come from k_backprop16's partials (OutLayerSums)
  DevBuf<float> wg_outpart;     // [ceil(B / 16)][2][Hp + 4]
  DevBuf<int> wg_tickets;       // [wg_tiles] arrival tickets of the split-K fold, zero between launches
  DevBuf<float> ratio, ones;
  DevBuf<float> acc, adam_m, adam_v, grad_tmp;
  // reset_gradients does not zero `acc` at once: the first dense accumulate after it WRITES its sums
  // (no 1.3 MB memset + read-modify-write per optimizer step); everything else that touches `acc`
  // materialises the zeros first (acc_zeros)
  bool acc_fresh = false;
  long long adam_t = 0;
  DevBuf<float> gemm_ws;  // partial tiles of the weight-gradient launch: plan_wgrad_ws_floats(wg_tiles, WG_MAX_SPLIT)
  int num_cus = 256;
  int sweep_waves = 8;       // waves per sweep workgroup at Hp = 256 (CGS_VMC_SWEEP_WAVES=4|8)
  int sweep_no_w1l = 0;      // CGS_VMC_SWEEP_W1L=0: W1 stays in L2 (smaller LDS footprint)
  int sweep_tile = 16;       // chains per sampler workgroup: 16 (k_sweep16) or 8 (k_sweep8; plan_sweep_tile)
  bool sweep8_ok = false;    // the shape has a k_sweep8
  // stochastic reconfiguration (extension, sr.hip): sample store + CG vectors
  int sr_cap = 0, sr_n = 0, sr_iter = 0;
  DevBuf<float> sr_cfg, sr_act, sr_delta;   // [cap B][N], [L][cap B][Hp] x2
  // convolutional ansatz types: stored tapes / deltas [n_conv-1 | n_conv][cap B][CS], the CG direction
  // packed like a parameter set, and the slices of the weight-gradient kernel over the stored samples
  DevBuf<float> sr_ctape, sr_cdelta, sr_cws;
  DevBuf<float> sr_cw0, sr_cwf, sr_cwb, sr_cbias;
  int sr_cslices = 0;
  DevBuf<float> sr_ws, sr_t, sr_ones;        // [slices][(max(N,H)+1) H], [cap B] x2
  DevBuf<float> sr_tpart;                                          // [layers x column blocks][cap B] partial t
  DevBuf<float> sr_u, sr_x, sr_r, sr_p, sr_q;
  DevBuf<double> sr_partial, sr_sc;
  bool sr_begun = false;
  // the sample-space solve (srgram.hip): the stored samples' local energies [cap B] (recorded with the store), the Gram
  // matrix [n][n] and the six CG vectors [n] (y, r, p, C p, w, q; fp64) -- both allocated by the first solve, released
  // by vmc_sr_reserve -- and the solve's scalars [4]
  DevBuf<float> sr_eloc, sr_gram;
  DevBuf<double> sr_gvec, sr_gsc;
  // collectives over sharded chains: host hook for non-RCCL transports + its staging
  vmc_host_allreduce_fn host_reduce = nullptr;
  void* host_reduce_user = nullptr;
  int host_reduce_caps = 0;                       // VMC_HOST_REDUCE_CAP_*: what the registered host hook has declared
  vmc_device_allreduce_fn dev_reduce = nullptr;   // in-stream transport of the host's own collective library
  void* dev_reduce_user = nullptr;
  DevBuf<double> d_eval;      // vmc_evaluate: batch sums / means of the samples (grow-only)
  float* h_stage = nullptr;      // pinned
  DevBuf<float> d_stage;      // vmc_debug_allreduce only
  long long h_stage_n = 0;
  // scratch
  DevBuf<unsigned long long> d_accepted;
  DevBuf<double> d_sum;
  DevBuf<float> d_max;
  DevBuf<float> tmp_cfg, tmp_z1, tmp_out, tmp_on;
  long long tmp_rows = 0;
  DevBuf<int> inj_up, inj_dn;
  DevBuf<float> inj_u;
  DevBuf<unsigned char> acc_mask;
  unsigned long long step = 0;
  // timing
  int timing = 0;            // 0 off, 1 every region, 2 the two roofline kernels only
  std::vector<TimedRegion> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> event_pool;
  std::map<std::string, std::pair<double, long long>> timings;
  std::string err;
};


namespace vmcapi {


inline int fail(vmc_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg; else g_create_error = msg;
  return code;
}

#define HIPCHK(c, expr)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail((c), VMC_ERR_HIP,                                                      \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                    \
  } while (0)

// Every entry point runs on the ctx's device whatever the calling thread's current device is
// (HIP's current device is per thread), and restores the caller's device on return.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// entry points that only touch the accumulators / scalars / host state
#define CHECK_CTX(c)                                                      \
  if (!(c)) return fail(nullptr, VMC_ERR_INVALID, "null ctx");            \
  DeviceGuard device_guard_((c)->d.device)

// every other entry point: the work it enqueues on `stream` may depend on the chains, so
// `stream` first waits for a sampler launch still in flight on sweep_stream
#define ENTER(c)                                                          \
  CHECK_CTX(c);                                                           \
  (c)->token = false;                                                     \
  do { int rc_join_ = join_sweep(c); if (rc_join_ != VMC_OK) return rc_join_; } while (0)

#define PROPAGATE(expr) \
  do { int rc_ = (expr); if (rc_ != VMC_OK) return rc_; } while (0)

// a factor of a product ctx: its chains, accumulators and sampler state belong to the product
// (the base of a symmetrized ctx likewise: they belong to the symmetrized ctx)
#define REFUSE_COMPOSED(c) \
  do { if ((c)->owner) return fail((c), VMC_ERR_STATE, (c)->owner->symz \
      ? "the ctx is the base of a symmetrized ctx (vmc_create_symmetrized): its chain-state entries are the symmetrized ctx's" \
      : "the ctx is a factor of a product ctx (vmc_create_product): its chain-state entries are the product's"); } while (0)
// entries a symmetrized ctx does not have
#define REFUSE_SYMZ(c, what) \
  do { if ((c)->symz) return fail((c), VMC_ERR_UNSUPPORTED, what " is not available on a symmetrized ctx ('symmetrized')"); } while (0)
// entries a product ctx does not have (a symmetrized ctx has none of them either)
#define REFUSE_PRODUCT(c, what) \
  do { if ((c)->prod) return fail((c), VMC_ERR_UNSUPPORTED, what " is not available on a product ctx ('prod')"); \
       REFUSE_SYMZ(c, what); } while (0)
// the PATH_PRODUCT arm of a switch no product ctx reaches (its entries go to the factors, which run their own paths)
inline int product_has_none(vmc_ctx* c, const char* what) {
  return fail(c, VMC_ERR_STATE, std::string("prod: a product ctx has no ") + what + " of its own (its factors run theirs)");
}

// CUs a sampler launch occupies (8 waves at 255 registers, or LDS, fill a CU per workgroup)
inline int sweep_cus(const vmc_ctx* c) { return c->sweep_tile == 8 ? (c->B + 7) / 8 : (c->B + 15) / 16; }

// The sampler may overtake the accumulate enqueued just before it when it leaves the local-energy
// kernel at least a quarter of the CUs; with one 16-chain tile per CU (config 3) there is nothing
// to share and the launch stays on `stream`.
inline bool can_overlap(const vmc_ctx* c) {
  return c->overlap && (c->overlap_full || sweep_cus(c) <= (3 * c->num_cus) / 4);
}

// `acc` is about to be read or partially written: turn a pending reset into real zeros
inline int acc_zeros(vmc_ctx* c) {
  if (c->acc_fresh) {
    hipError_t e = hipMemsetAsync(c->acc, 0, (2 * c->P + 8) * sizeof(float), c->stream);
    if (e != hipSuccess) return fail(c, VMC_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    c->acc_fresh = false;
  }
  return VMC_OK;
}

inline int join_sweep(vmc_ctx* c) {
  if (c->sweep_pending) {
    hipError_t e = hipStreamWaitEvent(c->stream, c->ev_sweep_done, 0);
    if (e != hipSuccess) return fail(c, VMC_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
    c->sweep_pending = false;
  }
  return VMC_OK;
}

inline void swap_chain_buffers(vmc_ctx* c) {
  ParamSet& p = c->ps[0];
  std::swap(c->configs, c->configs_alt);
  std::swap(p.z1, p.z1_alt); std::swap(p.logit, p.logit_alt); std::swap(p.onsite, p.onsite_alt);
  std::swap(p.sign, p.sign_alt);
  std::swap(c->act_all, c->act_alt);
  std::swap(c->dact_all, c->dact_alt);
  std::swap(c->cnt, c->cnt_alt); std::swap(c->diag, c->diag_alt);
  for (size_t l = 0; l < c->act.size(); ++l) c->act[l] = c->act_all + (long long)l * c->B * c->Hp;
  c->parity ^= 1;
}

// Per-kernel timing: event pairs come from a pool (creating two events per region costs more
// than recording them); regions whose stop event has completed are folded into the totals and
// their events recycled without blocking.
inline void account(vmc_ctx* c, const TimedRegion& r) {
  float ms = 0.f;
  hipEventElapsedTime(&ms, r.start, r.stop);
  auto& t = c->timings[r.name];
  t.first += ms; t.second += 1;
  c->event_pool.emplace_back(r.start, r.stop);
}

inline void harvest_finished(vmc_ctx* c) {
  size_t done = 0;
  while (done < c->pending.size() && hipEventQuery(c->pending[done].stop) == hipSuccess) {
    account(c, c->pending[done]);
    ++done;
  }
  if (done) c->pending.erase(c->pending.begin(), c->pending.begin() + done);
}

struct Timer {
  vmc_ctx* c; hipStream_t st; bool on; TimedRegion r;
  Timer(vmc_ctx* ctx, const char* name, hipStream_t stream = nullptr, bool own_stream = false)
      : c(ctx), st(own_stream ? stream : ctx->stream),      // (a null name: no region -- the caller times the call itself)
        on(name && (ctx->timing == 1 || (ctx->timing == 2 && (!strcmp(name, "sweep") || !strcmp(name, "tail_eloc"))))) {
    if (on) {
      r.name = name;
      if (c->event_pool.empty()) harvest_finished(c);
      if (c->event_pool.empty()) {
        hipEventCreate(&r.start); hipEventCreate(&r.stop);
      } else {
        r.start = c->event_pool.back().first; r.stop = c->event_pool.back().second;
        c->event_pool.pop_back();
      }
      hipEventRecord(r.start, st);
    }
  }
  ~Timer() {
    if (on) { hipEventRecord(r.stop, st); c->pending.push_back(r); }
  }
};

inline void drain_timings(vmc_ctx* c) {
  for (auto& r : c->pending) {
    hipEventSynchronize(r.stop);
    account(c, r);
  }
  c->pending.clear();
}

// ---- the host scaffold of the samplers (run_sweep and the run_sweep_* of vmc_api_sweep.hip, prod_run_sweep): what a call
// is, the Philox key, the proposal launch, the injected proposals, and what is declared before and after the launches.
// Whatever a sampler writes out beside these is where it differs from the others.

// One sampler call.  dump_*: a proposal dump of step `step0` into these three [B] buffers -- nothing is sampled, nothing
// written back.  overtake / dep: the fused arm's launch goes to sweep_stream and only waits for `dep` (an event on `stream`)
struct SweepCall {
  long long n_steps = 0;
  unsigned long long step0 = 0;
  bool injected = false;          // the proposals are c->inj_up / inj_dn / inj_u, the accept mask goes to c->acc_mask
  bool count_accepted = false;    // the caller reads c->d_accepted back: zero it first
  bool overtake = false;
  hipEvent_t dep = nullptr;
  int *dump_up = nullptr, *dump_dn = nullptr;
  float* dump_u = nullptr;
  bool dump() const { return dump_up != nullptr; }
};

// The Philox key of a ctx's chains: the one place the seed is split.  set_key: onto any kernel argument struct
struct PhiloxKey { uint32_t seed_lo, seed_hi; int chain_offset; };
inline PhiloxKey philox_key(const vmc_ctx* c) {
  return PhiloxKey{(uint32_t)(c->d.seed & 0xFFFFFFFFull), (uint32_t)(c->d.seed >> 32), c->d.chain_offset};
}
template <class Args>
inline void set_key(const vmc_ctx* c, Args& a) {
  const PhiloxKey k = philox_key(c);
  a.seed_lo = k.seed_lo; a.seed_hi = k.seed_hi; a.chain_offset = k.chain_offset;
}

// injected proposals (vmc_mc_step_injected) onto any kernel argument struct
template <class Args>
inline void set_injected(const vmc_ctx* c, Args& a) {
  a.inj_up = c->inj_up; a.inj_dn = c->inj_dn; a.inj_u = c->inj_u; a.acc_mask = c->acc_mask;
}

// k_wide_propose for the chains as they stand: the proposals of `step` (or the injected ones) into iup / idn / u
inline hipError_t launch_proposals(const vmc_ctx* c, hipStream_t st, unsigned long long step, bool injected, int* iup,
                                   int* idn, float* u) {
  const PhiloxKey k = philox_key(c);
  return launch_wide_propose(st, c->configs, c->B, c->N, k.seed_lo, k.seed_hi, k.chain_offset, step,
                             injected ? c->inj_up.p : nullptr, injected ? c->inj_dn.p : nullptr,
                             injected ? c->inj_u.p : nullptr, iup, idn, u);
}

// the device counter of acceptances is only zeroed when the caller will read it back
inline int zero_accepted(vmc_ctx* c, const SweepCall& s, hipStream_t st) {
  if (s.count_accepted) HIPCHK(c, hipMemsetAsync(c->d_accepted, 0, sizeof(unsigned long long), st));
  return VMC_OK;
}

// The chains moved: what a sampler declares once its launches are enqueued.  acts / census: the launch left the final
// chains' activations (the gradient hand-over) and their bond census -- only the fused arm's can; an overtaking launch
// (the fused arm alone) leaves the event `stream` will wait for
inline int chains_moved(vmc_ctx* c, const SweepCall& s, bool acts = false, bool census = false) {
  c->cnt_valid = census;
  c->acts_valid = acts;
  c->acc_since_sweep = false;
  if (s.overtake) {
    HIPCHK(c, hipEventRecord(c->ev_sweep_done, c->sweep_stream));
    c->sweep_pending = true;
  }
  return VMC_OK;
}

// What an entry point declares after its sampler call.  psi_cache: psi's z1 / logit cache is that of the new chains (every
// sampler writes an exact one back but the general dense path's, which keeps an incrementally updated z1: recomputed on
// demand).  census_stays: cnt_valid is left as the sampler set it (vmc_mc_steps); otherwise the census is dropped
inline void sampler_returned(vmc_ctx* c, bool psi_cache, bool census_stays) {
  c->ps[0].cache_valid = psi_cache;
  c->ps[1].cache_valid = false;
  c->list_valid = false;
  if (!census_stays) c->cnt_valid = false;
}

// The two amplitude pairs of the measurements' folds, the one place that asks whether the ctx holds signs.  own_amps: the
// chains' cache of ps[which] (ensure_cache has run); row_amps: the rows of vmc_amplitude's buffers from row `at` on
inline AmpPair own_amps(const vmc_ctx* c, int which) {
  const ParamSet& p = c->ps[which];
  return AmpPair{p.logit, c->sgn ? p.sign.p : nullptr};
}
inline AmpPair row_amps(const vmc_ctx* c, long long at = 0) {
  return AmpPair{c->tmp_out + at, c->sgn ? c->tmp_sign + at : nullptr};
}

inline long long off_w(const vmc_ctx* c, int l) { return plan_off_w(c->lay, c->H, l); }   // weight matrix of layer l (0 = first)
inline long long off_b(const vmc_ctx* c, int l) { return plan_off_b(c->lay, c->H, l); }   // biases sit right behind their weights
inline long long off_wout(const vmc_ctx* c) { return c->lay.off_wout; }
inline long long off_bout(const vmc_ctx* c) { return c->lay.off_bout; }


// ---- shared across the translation units (definitions: the file named)
// vmc_api.hip
int ensure_packed(vmc_ctx* c, int which);
hipError_t launch_rows(vmc_ctx* c, int which, const TailArgs& a, bool ratio);
TailArgs tail_args(vmc_ctx* c, int which);
ConvParams conv_params(const ParamSet& p);
int ensure_cache(vmc_ctx* c, int which);
int conv_rows(vmc_ctx* c, int which, const float* configs, const int2* rowinfo, int rows,
              const int* rows_dev, bool ratio, float* out, bool with_tape);
int first_layer(vmc_ctx* c, const ParamSet& p, const float* configs, float* z1, int rows);
int wide_stage_act(const vmc_ctx* c, int l);
// hidden layer l (1 .. n_hh) of the dense trunk on `rows` rows: C = act(A W_l + b_l), A and C row buffers of pitch Hp
GemmArgs trunk_gemm(const vmc_ctx* c, const ParamSet& p, int l, const float* A, int rows, float* C, int act);
// nnb's pairing layer on `rows` rows: C [rows][N^2] = A W_out + b_out
GemmArgs nnb_pairing_gemm(const vmc_ctx* c, const ParamSet& p, const float* A, int rows, float* C);
bool wide_rowdot(vmc_ctx* c, const ParamSet& p, GemmArgs& g);
int wide_forward(vmc_ctx* c, int which, const float* z1, const int2* rowinfo, long long n_rows, bool ratio,
                 float* out, const float* onsite);
void invalidate_configs(vmc_ctx* c);
int ensure_list(vmc_ctx* c);
int local_energy_device(vmc_ctx* c, int which, bool defer_reduce = false, bool* deferred = nullptr);
// the row launch of local_energy_device alone: c->val of the ctx's current bond set over the current list (ensure_cache and
// ensure_list have run); share_cus: leave CUs to a sampler launch that is expected to overtake (expect_sweep)
int connected_rows_device(vmc_ctx* c, int which, bool share_cus);
int grow_tmp(vmc_ctx* c, long long rows);
// VMC_ERR_INVALID (with the message) when `c` holds signed amplitudes and a row of `configs` (host) is not at Sz = 0
int check_sz0_rows(vmc_ctx* c, const float* configs, long long n_rows);
const char* signed_family_name(KernelPath path);     // "pbdg", "fully_connected_nnb", "ed_vector", "prod (a signed factor)"
// the full forward on n_rows rows of a device buffer of configurations -> log|psi| and, for the signed types, the sign per
// row (vmc_amplitude, vmc_renyi2_swap); ensure_packed and grow_tmp(n_rows) have run
int rows_forward_device(vmc_ctx* c, int which, const float* configs, long long n_rows, float* logit, float* sign);
// neural-network backflow: rows {chain, bond} of a row list over `configs` and the chains' first-layer cache z1 -> logits
// and signs (ratio == false) or the local-energy terms (ratio: out = val, out_sign unused), in blocks of c->nnb_rows
int nnb_forward(vmc_ctx* c, int which, const float* z1, const float* configs, const int2* rowinfo, long long n_rows,
                bool ratio, float* out, float* out_sign);
// vmc_api_cgen.hip (the general convolution path)
int cgen_forward(vmc_ctx* c, int which, const float* configs, const int2* rowinfo, long long n_rows,
                 const int* iup, const int* idn, bool ratio, float* out, float* tape = nullptr,
                 long long tape_stride = 0, long long first_row = 0);
// VMC_ERR_INVALID (with the message) while an input the ctx takes after vmc_create is missing: a gnn ctx's adjacency
// list (vmc_set_adjacency), an ed_vector ctx's Lin tables (vmc_set_lin_tables)
int late_inputs_set(vmc_ctx* c);
int cgen_patch_mode(const vmc_ctx* c);
int cgen_patch_maps(vmc_ctx* c, int which);
void cgen_patch_args(const vmc_ctx* c, int which, CgenPatchArgs* a);
bool cgen_single_block(const vmc_ctx* c, long long n_rows);
const float* cgen_last_map(const vmc_ctx* c);
int cgen_gradient_sums(vmc_ctx* c, const float* w);
int cgen_sr_phase1(vmc_ctx* c, const float* v, int n_rows);
int cgen_sr_phase2(vmc_ctx* c, int n_rows);
int cgen_sr_matvec(vmc_ctx* c, const float* v, int n_rows);
// vmc_api_coll.hip
int reduce_buffer(vmc_ctx* c, void* comm, int world, void* buf, long long n, int op);
bool sharded(void* comm, int world);
int reduce_accumulators(vmc_ctx* c, void* comm, int world);
// vmc_api_train.hip: the gradient sums of a factor for an external weight vector into external accumulators (+=)
int child_gradient_sums(vmc_ctx* c, const float* w, float* g1, float* g2);
// vmc_api_prod.hip (the product ctx; every function takes the PRODUCT unless named child)
int prod_ensure_cache(vmc_ctx* c, int which);
int prod_local_energy(vmc_ctx* c, int which);
int prod_alive(vmc_ctx* c);                         // VMC_ERR_STATE (with the message) once a factor has been destroyed
int prod_run_sweep(vmc_ctx* c, const SweepCall& s);
int prod_accumulate(vmc_ctx* c, int mode, float beta);
int prod_set_bonds(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z);
int prod_gather_params(vmc_ctx* c, int which);      // the factors' theta -> the product's [a | b]
int prod_scatter_params(vmc_ctx* c, int which);     // ... and back
int prod_transfer_params(vmc_ctx* c);
int prod_amplitude(vmc_ctx* c, int which, const float* configs, int64_t n_rows, float* logit, float* psi);
void prod_chains_changed(vmc_ctx* c);
void prod_child_params_changed(vmc_ctx* child, int which);
void prod_release(vmc_ctx* c);                       // vmc_destroy of a product: the factors are free again
void prod_child_destroyed(vmc_ctx* child);           // vmc_destroy of a factor that is still composed
// vmc_api_symz.hip (the symmetrized ctx; every function takes the COMPOSITE unless named base)
int symz_alive(vmc_ctx* c);                         // VMC_ERR_STATE (with the message) once the base has been destroyed
int symz_ensure_cache(vmc_ctx* c, int which);
int symz_local_energy(vmc_ctx* c, int which);
int symz_run_sweep(vmc_ctx* c, const SweepCall& s);
int symz_accumulate(vmc_ctx* c, int mode, float beta);
int symz_set_bonds_check(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z);
int symz_set_bonds(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z);
int symz_set_params(vmc_ctx* c, int which, const float* theta);     // theta is the base's: the three forward
int symz_get_params(vmc_ctx* c, int which, float* theta);
int symz_transfer_params(vmc_ctx* c);
int symz_adam_theta(vmc_ctx* c, float** theta);      // the buffer Adam runs on (the base's psi set)
void symz_adam_applied(vmc_ctx* c);
int symz_amplitude(vmc_ctx* c, int which, const float* configs, int64_t n_rows, float* logit, float* psi);
int symz_check_configs(vmc_ctx* c, const float* configs);     // vmc_set_configs: no row at a structural zero
void symz_chains_changed(vmc_ctx* c);
void symz_base_params_changed(vmc_ctx* base, int which);
void symz_release(vmc_ctx* c);                       // vmc_destroy of a symmetrized ctx: the base is free again
void symz_base_destroyed(vmc_ctx* base);             // vmc_destroy of a base that is still composed
// the PATH_SYMMETRIZED arm of a switch no symmetrized ctx reaches (its entries go to the base, which runs its own path)
inline int symmetrized_has_none(vmc_ctx* c, const char* what) {
  return fail(c, VMC_ERR_STATE, std::string("symmetrized: a symmetrized ctx has no ") + what + " of its own (its base runs its)");
}
// vmc_api_measure.hip: what vmc_overlap and mode PENALIZED_ENERGY share -- the front of their refusals, and the ratio pass
// and the fold over the two amplitude caches (ensure_cache of both sets has run) into c->ovl.out
int overlap_refusals(vmc_ctx* c, const char* what);
int overlap_sums_device(vmc_ctx* c);
// vmc_api_measure.hip: the four-spin terms of the Hamiltonian on top of the Heisenberg local energies in ps[which].eloc
// (local_energy_device calls it while c->fs.n_terms > 0)
int four_spin_device(vmc_ctx* c, int which);
// vmc_api_sweep.hip
bool sampler_refresh_ok(const vmc_ctx* c);
int refresh_cache_by_sampler(vmc_ctx* c, int which);
}  // namespace vmcapi

template <class T>
int DevBuf<T>::alloc(vmc_ctx* c, long long n, const char* name) {
  using vmcapi::fail;
  if (p) HIPCHK(c, hipStreamSynchronize(c->stream));
  release();
  if (n < 1) n = 1;
  const hipError_t e = hipMalloc((void**)&p, (size_t)n * sizeof(T));
  if (e != hipSuccess) {
    p = nullptr;
    return fail(c, VMC_ERR_HIP, std::string("hipMalloc(") + name + "): " + hipGetErrorString(e));
  }
  cap = n;
  return VMC_OK;
}

template <class T>
int DevBuf<T>::reserve(vmc_ctx* c, long long n, const char* name, bool* grew) {
  if (grew) *grew = false;
  if (n < 1) n = 1;
  if (n <= cap) return VMC_OK;
  PROPAGATE(alloc(c, n, name));
  if (grew) *grew = true;
  return VMC_OK;
}
