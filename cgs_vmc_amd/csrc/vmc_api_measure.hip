// The measurements over the ctx's current chains (extensions, no reference counterpart): vmc_pair_correlations,
// vmc_renyi2_swap, vmc_dimer_correlations, vmc_symmetry_expectations, vmc_projected_energy, vmc_energy_moments and
// vmc_overlap.  Each is a pure measurement: chains, step counter, accumulators, the Hamiltonian's bond set and the
// validity of the amplitude and activation caches are as before when it returns.
//
// One scaffold serves the seven.  An entry is straight-line code: its refusals (MEASURE_GATE in front, needs_ln_psi where
// the logit must be ln psi), then the host buffers of its asynchronous copies, then ONE guard, PureMeasurement, and behind
// it plain PROPAGATE / HIPCHK steps that return as soon as one fails.  The guard makes that safe: on every way out it
// synchronises the stream (unless read_back, the last step, already has) and un-vouches the caches that were not valid
// before; its declaration rule is stated where it is defined.  HamiltonianSet is the same idea for the bond set the spin
// correlations swap out.  upload copies a host list into its device buffer; for_passes walks the items in passes of
// plan_measure_per_pass (plan.hpp); row_pass is a pass of all but the spin correlations: the measurement's rows kernel
// into the row buffer of vmc_amplitude, then the family's own full forward; read_back brings the fp64 sums down.  The
// amplitudes a fold compares travel as AmpPair (common.hpp): own_amps, the chains' cache, and row_amps, the rows of the
// pass (vmc_ctx.hpp).  The device buffers are the grow-only DevBufs of vmc_ctx.hpp.  What differs per measurement is its
// own checks, which rows kernel and which fold a pass launches, and how the sums are handed out:
//
// Spin correlations.  Per pair (i, j): zz = sum_c s_i s_j and ex = sum_c [s_i s_j < 0] psi(swap_ij x_c) / psi(x_c); the
// host forms <S_i . S_j> = (zz / 4 + ex / 2) / B.  The ratios are the rows the local energies already evaluate: a pass of
// pairs is a bond set of its own (j_x = 2, so that val is the bare ratio; j_z = 0) that takes the place of the
// Hamiltonian's five buffers + n_bonds in the ctx while ensure_list and the family's row launch (connected_rows_device)
// run, and is swapped out again afterwards.  The fold per pair over chains is corr.hip.
//
// Renyi-2 entanglement entropy, the replica swap estimator over the chains taken as the B / 2 pairs (c, c + B / 2).  Per
// region A: swap_sum = sum over the pairs that hold the same sum of spins on A of psi(x~) psi(y~) / (psi(x) psi(y)), with
// the spins of A exchanged between the two chains, and match_count = the number of such pairs; the host forms
// Tr rho_A^2 ~ swap_sum / (B / 2) and S2 = -ln of it.  A pass of regions is B rows per region (renyi.hip: k_swap_rows),
// folded per region (k_swap_fold) against the chains' cached ln|psi| and signs.
//
// Dimer-dimer correlations.  Per bond a = (i, j): bond_sum = sum_c bond(a; x_c); per ordered pair of bonds (a, b):
// dd_sum = sum_c dd(a, b; x_c), the local value of (S_i . S_j)(S_k . S_l) (dimer.hip states both); the host forms
// <A B> ~ dd_sum / B, <A> ~ bond_sum / B and the connected part.  Phase 1: B rows per bond, the single exchanges
// (k_dimer_rows1), through the full forward in as many passes as the row buffer of vmc_amplitude takes (fewer bonds per
// pass where pairs_per_pass asks for fewer); their ln|psi| and signs stay in the ctx's [n_bonds][B] buffers.  Phase 2:
// passes of pairs, B rows per pair, the double exchanges (k_dimer_rows2), forwarded the same way and folded per pair
// (k_dimer_fold) against phase 1's buffers and the chains' cached ln|psi| and signs.  (n_bonds + n_pairs) B full
// forwards in all.
//
// Symmetry expectation values.  Per op k -- a site permutation perm_k, optionally followed by the global spin flip:
// ratio_sum = sum_c psi(row_{k,c}) / psi(x_c) with row[i] = f_k x_c[perm_k[i]]; the host forms <P_k> ~ ratio_sum / B.  A
// pass of ops is B rows per op (symm.hip: k_symm_rows), folded per op (k_symm_fold) against the chains' cached ln|psi|
// and signs.  Every perm_k is checked to be a bijection before anything is launched (symm_ops_check): the rows must stay
// at Sz = 0.
//
// Symmetry-projected energies.  The ops of the symmetry expectation values (symm_ops_check / symm_ops_upload serve both)
// and, per sector s, real characters chi[s][k]: w_s(c) = sum_k chi[s][k] psi(row_{k,c}) / psi(x_c), and the host forms
// E_s = sum_c w_s(c) E_loc(c) / sum_c w_s(c), the energy of P_s psi.  One local-energy call first (it uses the row
// buffers the passes then take), then the passes of the symmetry expectation values with k_proj_accum (proj.hip) in the
// fold's place: it adds a pass's ops into the per-chain fp64 accumulator [n_sectors][B]; k_proj_fold folds the chains at
// the end.  Beside the bijection check every perm_k is checked to map the Hamiltonian's bonds onto themselves, couplings
// included (plan_symm_check_hamiltonian): the estimator means nothing otherwise.  What a vmc_local_energy call leaves
// behind (the chains' local energies of `which`, vmc_last_connected_rows) is the one thing this measurement changes.
//
// Lanczos-step energies.  Per chain e = (H psi)(x) / psi(x) and g = (H^2 psi)(x) / psi(x) (moments.hip states the estimator,
// the list rules and every summation order).  One local-energy call first; its row list, val and eloc are the first
// order.  Then the second-order list: counted per first-order row and prefixed (k_mom_count, k_mom_scan), its length read
// back, and walked in passes of ROWS (plan_list_per_pass): k_mom_fill writes the descriptors of the pass alone,
// k_mom_rows the configurations, the family's full forward evaluates them and k_mom_accum adds coef r into the chains'
// lanes.  k_mom_chain / k_mom_sums fold at the end.  Like the projected energies it leaves what vmc_local_energy leaves.
//
// Overlap with the frozen set.  No rows: one ratio pass and one fold over the two amplitude caches (overlap.hip), shared
// with the penalised-energy mode of the training entries (overlap_refusals, overlap_sums_device).
//
// Beside the measurements, on the same scaffold: the four-spin (J-Q) terms of the Hamiltonian (four_spin_device,
// vmc_set_four_spin_terms; fourspin.hip) -- no measurement but a part of every local energy while terms are set; its
// section below states it.
#include "vmc_ctx.hpp"

using namespace vmcapi;

namespace {

// the front of every measurement's refusals; returns from the entry
#define MEASURE_GATE(c, which, name)                                                     \
  ENTER(c);                                                                              \
  REFUSE_PRODUCT(c, name);                                                               \
  REFUSE_COMPOSED(c);                                                                    \
  if ((which) != 0 && (which) != 1) return fail((c), VMC_ERR_INVALID, "bad which")

// the refusal of every entry that takes the logit for ln psi
int needs_ln_psi(vmc_ctx* c, const std::string& entry) {
  if (c->sgn || c->oact == VMC_ACT_EXP_) return VMC_OK;
  return fail(c, VMC_ERR_UNSUPPORTED, entry + " needs the exp output activation (the logit is ln psi only then)");
}

// The scope guard of a measurement entry: behind it the entry may return wherever a step fails.  On every way out it
// first synchronises the stream -- the entry's host buffers are sources and targets of asynchronous copies -- unless
// read_back has (a call that succeeds synchronises once), then un-vouches: what was not valid before the measurement is
// not vouched for after it either, the next consumer fills it exactly as it would have.
// THE RULE: every host buffer that is the source or the target of an asynchronous copy of the entry is declared BEFORE
// the guard, so that it outlives the guard's synchronisation.
struct PureMeasurement {
  vmc_ctx* c;
  const bool cache_was[2], acts_were;
  bool synchronised = false;
  explicit PureMeasurement(vmc_ctx* ctx)
      : c(ctx), cache_was{ctx->ps[0].cache_valid, ctx->ps[1].cache_valid}, acts_were(ctx->acts_valid) {}
  ~PureMeasurement() {
    if (!synchronised) hipStreamSynchronize(c->stream);
    for (int w = 0; w < 2; ++w) if (!cache_was[w]) c->ps[w].cache_valid = false;
    if (!acts_were) c->acts_valid = false;
  }
  PureMeasurement(const PureMeasurement&) = delete;
  PureMeasurement& operator=(const PureMeasurement&) = delete;
};

template <class T>
int upload(vmc_ctx* c, T* dst, const std::vector<T>& src) {
  HIPCHK(c, hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return VMC_OK;
}

// items [k0, k0 + n) per call of pass(k0, n), `per` at a time, until one fails
template <class Pass>
int for_passes(long long n_items, int per, Pass pass) {
  for (long long k0 = 0; k0 < n_items; k0 += per) PROPAGATE(pass(k0, (int)(n_items - k0 < per ? n_items - k0 : per)));
  return VMC_OK;
}

// One pass of rows: rows_kernel() launches the measurement's rows kernel, which writes n_rows configurations into
// tmp_cfg; the family's own full forward (rows_forward_device, vmc_api.hip) leaves their ln|psi| and signs in logit / sign
template <class Rows>
int row_pass(vmc_ctx* c, int which, const char* rows_region, const char* forward_region, long long n_rows, float* logit,
             float* sign, Rows rows_kernel) {
  {
    Timer t(c, rows_region);
    HIPCHK(c, rows_kernel());
  }
  Timer t(c, forward_region);
  return rows_forward_device(c, which, c->tmp_cfg, n_rows, logit, sign);
}

// the last step of every measurement: n sums to the host (out: declared before the guard), and the one synchronisation
// of a call that succeeds
int read_back(PureMeasurement& pure, const double* sums, size_t n, std::vector<double>* out) {
  vmc_ctx* c = pure.c;
  out->resize(n);
  HIPCHK(c, hipMemcpyAsync(out->data(), sums, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pure.synchronised = true;
  return VMC_OK;
}

// ---- spin correlations

struct BondSet {
  int n_bonds; int2* bonds; float *half_jx, *quarter_jz; int2* rowinfo; float* val;
};

BondSet current_set(const vmc_ctx* c) { return BondSet{c->n_bonds, c->bonds, c->half_jx, c->quarter_jz, c->rowinfo, c->val}; }

// cnt / diag / off / the list belong to whichever set was counted last: nothing of them survives a swap
void install_set(vmc_ctx* c, const BondSet& s) {
  c->n_bonds = s.n_bonds; c->bonds = s.bonds; c->half_jx = s.half_jx; c->quarter_jz = s.quarter_jz;
  c->rowinfo = s.rowinfo; c->val = s.val;
  c->bonds_epoch += 1;        // (the bond-difference tables of the row kernel belong to the list they were built from)
  c->list_valid = false;
  c->cnt_valid = false;
}

// the set that is current where the guard is made -- the Hamiltonian's -- is installed again on every way out of the scope
struct HamiltonianSet {
  vmc_ctx* c;
  const BondSet set;
  explicit HamiltonianSet(vmc_ctx* ctx) : c(ctx), set(current_set(ctx)) {}
  ~HamiltonianSet() { install_set(c, set); }
  HamiltonianSet(const HamiltonianSet&) = delete;
  HamiltonianSet& operator=(const HamiltonianSet&) = delete;
};

// the set of a pass for `per` pairs; hx and qz are (re)filled whenever one of the five grew
int corr_reserve_pass(vmc_ctx* c, long long per) {
  CorrBufs& m = c->corr;
  const long long rows = (long long)c->B * per;
  bool g[5];
  PROPAGATE(m.hx.reserve(c, per, "corr.hx", &g[0]));
  PROPAGATE(m.qz.reserve(c, per, "corr.qz", &g[1]));
  PROPAGATE(m.rowinfo.reserve(c, rows, "corr.rowinfo", &g[2]));
  PROPAGATE(m.val.reserve(c, rows, "corr.val", &g[3]));
  PROPAGATE(m.dense.reserve(c, rows, "corr.dense", &g[4]));
  if (!(g[0] || g[1] || g[2] || g[3] || g[4])) return VMC_OK;
  HIPCHK(c, launch_fill(c->stream, m.hx, 1.f, (int)m.hx.cap));      // 0.5 j_x with j_x = 2
  HIPCHK(c, hipMemsetAsync(m.qz, 0, (size_t)m.qz.cap * sizeof(float), c->stream));
  return VMC_OK;
}

int corr_reserve(vmc_ctx* c, long long per, long long n_pairs) {
  PROPAGATE(c->corr.pairs.reserve(c, n_pairs, "corr.pairs"));
  PROPAGATE(c->corr.out.reserve(c, 2 * n_pairs, "corr.out"));
  const int rc = corr_reserve_pass(c, per);
  // a set that did not grow, or was not filled, as a whole is no set: the next call allocates and fills it afresh
  if (rc != VMC_OK) { hipStreamSynchronize(c->stream); c->corr.release_pass(); }
  return rc;
}

// pairs [k0, k0 + n) with their set installed: list, rows, fold
int corr_pass(vmc_ctx* c, int which, long long k0, int n, long long n_pairs) {
  PROPAGATE(ensure_list(c));
  PROPAGATE(connected_rows_device(c, which, false));
  Timer t(c, "corr_fold");
  HIPCHK(c, launch_pair_fold(c->stream, c->configs, c->bonds, c->rowinfo, c->val, c->off + c->B, c->B, c->N, n,
                             c->num_cus, c->corr.dense, c->corr.out + k0, c->corr.out + n_pairs + k0));
  return VMC_OK;
}

// ---- Renyi-2 swap estimator

int renyi_reserve(vmc_ctx* c, long long n_regions) {
  PROPAGATE(c->renyi.mask.reserve(c, n_regions * c->N, "renyi.mask"));
  return c->renyi.out.reserve(c, 2 * n_regions, "renyi.out");
}

// regions [k0, k0 + n): rows, forward, fold
int renyi_pass(vmc_ctx* c, int which, long long k0, int n, long long n_regions) {
  const unsigned char* mask = c->renyi.mask + k0 * c->N;
  double* out = c->renyi.out;
  PROPAGATE(row_pass(c, which, "renyi_rows", "renyi_forward", (long long)n * c->B, c->tmp_out, c->tmp_sign, [&] {
    return launch_swap_rows(c->stream, c->configs, mask, c->B, c->N, n, c->num_cus, c->tmp_cfg);
  }));
  Timer t(c, "renyi_fold");
  HIPCHK(c, launch_swap_fold(c->stream, c->configs, mask, own_amps(c, which), row_amps(c), c->B, c->N, n, out + k0,
                             out + n_regions + k0));
  return VMC_OK;
}

// ---- dimer-dimer correlations

int dimer_reserve(vmc_ctx* c, long long n_bonds, long long n_pairs) {
  DimerBufs& m = c->dimer;
  PROPAGATE(m.bonds.reserve(c, n_bonds, "dimer.bonds"));
  PROPAGATE(m.pairs.reserve(c, n_pairs, "dimer.pairs"));
  PROPAGATE(m.logit.reserve(c, n_bonds * c->B, "dimer.logit"));
  if (c->sgn) PROPAGATE(m.sign.reserve(c, n_bonds * c->B, "dimer.sign"));
  return m.out.reserve(c, n_bonds + n_pairs, "dimer.out");
}

// phase 1's rows [n_bonds][B]: dimer.sign is allocated on a signed ctx alone, so the sign is null on every other
AmpPair dimer_single_amps(const vmc_ctx* c) { return AmpPair{c->dimer.logit, c->dimer.sign}; }

// bonds [a0, a0 + n): rows, forward into the [n_bonds][B] buffers
int dimer_single_pass(vmc_ctx* c, int which, long long a0, int n) {
  const DimerBufs& m = c->dimer;
  float* sign = c->tmp_sign;                 // (an unsigned ctx keeps no sign per bond: the forward's goes to the scratch rows)
  if (c->sgn) sign = m.sign + a0 * c->B;
  return row_pass(c, which, "dimer_rows", "dimer_forward", (long long)n * c->B, m.logit + a0 * c->B, sign, [&] {
    return launch_dimer_rows1(c->stream, c->configs, m.bonds + a0, c->B, c->N, n, c->num_cus, c->tmp_cfg);
  });
}

// pairs [p0, p0 + n): rows, forward, fold
int dimer_double_pass(vmc_ctx* c, int which, long long p0, int n, double* dd_out) {
  const DimerBufs& m = c->dimer;
  PROPAGATE(row_pass(c, which, "dimer_rows", "dimer_forward", (long long)n * c->B, c->tmp_out, c->tmp_sign, [&] {
    return launch_dimer_rows2(c->stream, c->configs, m.bonds, m.pairs + p0, c->B, c->N, n, c->num_cus, c->tmp_cfg);
  }));
  Timer t(c, "dimer_fold");
  HIPCHK(c, launch_dimer_fold(c->stream, c->configs, m.bonds, m.pairs + p0, own_amps(c, which), dimer_single_amps(c),
                              row_amps(c), c->B, c->N, n, dd_out + p0));
  return VMC_OK;
}

// ---- the ops of the symmetry expectation values and of the symmetry-projected energies (c->symm.perm / flip)

struct SymmOps {
  std::vector<int> perm;                 // [n_ops][N]
  std::vector<unsigned char> flip;       // [n_ops]; a null flip of the caller: zeros
};

// the checking half: the arguments, every op a bijection with a 0 / 1 flip (plan_symm_check_ops), the host copies
int symm_ops_check(vmc_ctx* c, int32_t n_ops, const int32_t* perm, const uint8_t* flip, int32_t ops_per_pass, SymmOps* ops) {
  if (n_ops < 1 || !perm || ops_per_pass < 0) return fail(c, VMC_ERR_INVALID, "bad symmetry op arguments");
  char msg[160];
  if (plan_symm_check_ops(c->N, n_ops, perm, flip, msg, sizeof(msg)) != VMC_OK) return fail(c, VMC_ERR_INVALID, msg);
  ops->perm.assign(perm, perm + (size_t)n_ops * (size_t)c->N);
  ops->flip.assign((size_t)n_ops, 0);
  if (flip) ops->flip.assign(flip, flip + n_ops);
  return VMC_OK;
}

// the device half: the two buffers and the two uploads (ops: declared before the entry's guard)
int symm_ops_upload(vmc_ctx* c, const SymmOps& ops) {
  PROPAGATE(c->symm.perm.reserve(c, (long long)ops.perm.size(), "symm.perm"));
  PROPAGATE(c->symm.flip.reserve(c, (long long)ops.flip.size(), "symm.flip"));
  PROPAGATE(upload(c, c->symm.perm.p, ops.perm));
  return upload(c, c->symm.flip.p, ops.flip);
}

// the rows and the forward of ops [k0, k0 + n), under the region names of the measurement
int symm_row_pass(vmc_ctx* c, int which, const char* rows_region, const char* forward_region, long long k0, int n) {
  const SymmBufs& m = c->symm;
  return row_pass(c, which, rows_region, forward_region, (long long)n * c->B, c->tmp_out, c->tmp_sign, [&] {
    return launch_symm_rows(c->stream, c->configs, m.perm + k0 * c->N, m.flip + k0, c->B, c->N, n, c->num_cus, c->tmp_cfg);
  });
}

// ops [k0, k0 + n): rows, forward, fold
int symm_pass(vmc_ctx* c, int which, long long k0, int n) {
  PROPAGATE(symm_row_pass(c, which, "symm_rows", "symm_forward", k0, n));
  Timer t(c, "symm_fold");
  HIPCHK(c, launch_symm_fold(c->stream, own_amps(c, which), row_amps(c), c->B, n, c->symm.out + k0));
  return VMC_OK;
}

// ---- symmetry-projected energies

int proj_reserve(vmc_ctx* c, long long n_ops, long long n_sectors) {
  PROPAGATE(c->proj.chi.reserve(c, n_sectors * n_ops, "proj.chi"));
  PROPAGATE(c->proj.acc.reserve(c, n_sectors * c->B, "proj.acc"));
  return c->proj.out.reserve(c, 2 * n_sectors + 2, "proj.out");
}

// ops [k0, k0 + n): rows, forward, then their terms into the per-chain accumulator, PLAN_PROJ_LAUNCH_OPS ops a launch
int proj_pass(vmc_ctx* c, int which, long long k0, int n, int n_ops, int n_sectors) {
  PROPAGATE(symm_row_pass(c, which, "proj_rows", "proj_forward", k0, n));
  Timer t(c, "proj_accum");
  for (int j0 = 0; j0 < n; j0 += PLAN_PROJ_LAUNCH_OPS) {
    const int nj = n - j0 < PLAN_PROJ_LAUNCH_OPS ? n - j0 : PLAN_PROJ_LAUNCH_OPS;
    HIPCHK(c, launch_proj_accum(c->stream, own_amps(c, which), row_amps(c, (long long)j0 * c->B), c->proj.chi, c->B,
                                n_sectors, n_ops, (int)k0 + j0, nj, c->proj.acc));
  }
  return VMC_OK;
}

// ---- Lanczos-step energies

int mom_reserve_list(vmc_ctx* c, long long n1) {
  MomentBufs& m = c->mom;
  PROPAGATE(m.cnt2.reserve(c, n1, "mom.cnt2"));
  PROPAGATE(m.off2.reserve(c, n1 + 1, "mom.off2"));
  PROPAGATE(m.diag1.reserve(c, n1, "mom.diag1"));
  PROPAGATE(m.self1.reserve(c, n1, "mom.self1"));
  PROPAGATE(m.lanes.reserve(c, 64LL * c->B, "mom.lanes"));
  PROPAGATE(m.chain.reserve(c, 2LL * c->B, "mom.chain"));
  return m.out.reserve(c, 6, "mom.out");
}

// rows [q0, q0 + n) of the second-order list: descriptors, configurations, forward, into the chains' lanes
int mom_pass(vmc_ctx* c, int which, long long q0, int n, int n1) {
  const MomentBufs& m = c->mom;
  {
    Timer t(c, "mom_list");
    HIPCHK(c, launch_mom_fill(c->stream, c->configs, c->bonds, c->half_jx, c->quarter_jz, c->rowinfo, c->off + c->B, n1,
                              m.off2, c->N, c->n_bonds, q0, n, c->num_cus, m.desc, m.coef));
  }
  PROPAGATE(row_pass(c, which, "mom_rows", "mom_forward", n, c->tmp_out, c->tmp_sign, [&] {
    return launch_mom_rows(c->stream, c->configs, c->bonds, c->rowinfo, m.desc, c->N, n, c->num_cus, c->tmp_cfg);
  }));
  Timer t(c, "mom_fold");
  HIPCHK(c, launch_mom_accum(c->stream, own_amps(c, which), row_amps(c), m.coef, c->off, m.off2, c->B, q0, n, m.lanes));
  return VMC_OK;
}

// n ints the device holds, on the host (host: declared before the entry's guard; the stream is synchronised)
int read_ints(vmc_ctx* c, const int* dev, int* host, int n) {
  HIPCHK(c, hipMemcpyAsync(host, dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VMC_OK;
}

}  // namespace

namespace vmcapi {

// ---- overlap with the frozen set

int overlap_refusals(vmc_ctx* c, const char* what) {
  if (c->prod) return fail(c, VMC_ERR_UNSUPPORTED, std::string(what) + " is not available on a product ctx ('prod')");
  if (c->symz) return fail(c, VMC_ERR_UNSUPPORTED, std::string(what) + " is not available on a symmetrized ctx ('symmetrized')");
  PROPAGATE(needs_ln_psi(c, what));
  if (!c->ps[1].has_params)
    return fail(c, VMC_ERR_STATE, std::string(what) + ": the frozen parameters are not set (vmc_set_params(VMC_OMEGA) / vmc_transfer_params)");
  return VMC_OK;
}

int overlap_sums_device(vmc_ctx* c) {
  OverlapBufs& m = c->ovl;
  PROPAGATE(m.d.reserve(c, c->B, "ovl.d"));
  PROPAGATE(m.code.reserve(c, c->B, "ovl.code"));
  PROPAGATE(m.bmax.reserve(c, plan_overlap_blocks(c->B), "ovl.bmax"));
  PROPAGATE(m.out.reserve(c, 4, "ovl.out"));
  Timer t(c, "overlap_fold");
  HIPCHK(c, launch_overlap_ratio(c->stream, own_amps(c, 0), (double)c->ps[0].shift, own_amps(c, 1), (double)c->ps[1].shift,
                                 c->B, m.d, m.code, m.bmax));
  HIPCHK(c, launch_overlap_fold(c->stream, m.d, m.code, m.bmax, c->B, m.out));
  return VMC_OK;
}

// ---- four-spin (J-Q) terms of the Hamiltonian (fourspin.hip)
//
// Not a measurement: local_energy_device calls it behind the Heisenberg fold whenever the ctx holds terms, so every
// reader of eloc (the modes of vmc_accumulate, the fused epochs, vmc_evaluate, the SR store) sees H_J + H_Q.  It uses the
// measurements' scaffold: the list (count, prefix, its two lengths read back once), passes of ROWS through row_pass --
// k_fs_fill and k_fs_rows into tmp_cfg, the family's own full forward into the result buffers that span the list -- and
// ONE fold after the last pass.  The caches it reads (ensure_cache(which)) are the ones the Heisenberg part has filled.

// rows [q0, q0 + n) of the list: descriptors, configurations, forward into the list's result buffers
static int four_spin_pass(vmc_ctx* c, int which, long long q0, int n) {
  FourSpinBufs& m = c->fs;
  {
    Timer t(c, "fs_list");
    HIPCHK(c, launch_fs_fill(c->stream, c->configs, m.pairs, m.term_pairs, m.off, c->B, c->N, m.n_pairs, m.n_terms, q0, n,
                             c->num_cus, m.desc));
  }
  float* sign = c->tmp_sign;                 // (an unsigned ctx keeps no sign per row: the forward's goes to the scratch rows)
  if (c->sgn) sign = m.sign + q0;
  return row_pass(c, which, "fs_rows", "fs_forward", n, m.logit + q0, sign, [&] {
    return launch_fs_rows(c->stream, c->configs, m.pairs, m.term_pairs, m.desc, c->N, m.n_pairs, n, c->num_cus, c->tmp_cfg);
  });
}

int four_spin_device(vmc_ctx* c, int which) {
  FourSpinBufs& m = c->fs;
  PROPAGATE(ensure_cache(c, which));         // ln|psi(x_c)| and the signs, as the Heisenberg part took them
  PROPAGATE(m.n_single.reserve(c, c->B, "fs.n_single"));
  PROPAGATE(m.cnt.reserve(c, c->B, "fs.cnt"));
  PROPAGATE(m.off.reserve(c, (long long)c->B + 2, "fs.off"));
  if (m.want_parts) {
    PROPAGATE(m.dsum.reserve(c, c->B, "fs.dsum"));
    PROPAGATE(m.osum.reserve(c, c->B, "fs.osum"));
  }
  int lengths[2] = {0, 0};                   // the rows of the list, its single rows
  {
    Timer t(c, "fs_list");
    HIPCHK(c, launch_fs_count(c->stream, c->configs, m.pairs, m.term_pairs, c->B, c->N, m.n_pairs, m.n_terms, c->num_cus,
                              m.n_single, m.cnt, m.off));
    PROPAGATE(read_ints(c, m.off + c->B, lengths, 2));
  }
  const long long total = lengths[0];
  const long long per = plan_list_per_pass(total, m.rows_per_pass, plan_measure_row_limit(c->N, c->Hp));
  if (per < 1 || lengths[1] < 0 || lengths[1] > total) return fail(c, VMC_ERR_HIP, "the four-spin list has a negative length");
  PROPAGATE(m.desc.reserve(c, per, "fs.desc"));
  // (for the a-priori maximum where that fits, so that the list growing with the chains reallocates nothing: plan.hpp)
  PROPAGATE(m.logit.reserve(c, plan_fourspin_result_rows(c->B, m.n_pairs, m.n_terms, total, m.logit.cap), "fs.logit"));
  if (c->sgn) PROPAGATE(m.sign.reserve(c, plan_fourspin_result_rows(c->B, m.n_pairs, m.n_terms, total, m.sign.cap), "fs.sign"));
  PROPAGATE(grow_tmp(c, per));
  PROPAGATE(for_passes(total, (int)per, [&](long long q0, int n) { return four_spin_pass(c, which, q0, n); }));
  {
    Timer t(c, "fs_fold");
    HIPCHK(c, launch_fs_fold(c->stream, c->configs, m.pairs, m.term_pairs, m.wq, m.off, own_amps(c, which),
                             AmpPair{m.logit, c->sgn ? m.sign.p : nullptr}, c->B, c->N, m.n_pairs, m.n_terms,
                             m.exchange_sign, c->ps[which].eloc, m.want_parts ? m.dsum.p : nullptr,
                             m.want_parts ? m.osum.p : nullptr));
  }
  m.last_single = lengths[1];
  m.last_double = total - lengths[1];
  return VMC_OK;
}

}  // namespace vmcapi

extern "C" {

int vmc_set_four_spin_terms(vmc_ctx* c, int32_t n_terms, const int32_t* ijkl, const float* q, int32_t exchange_sign,
                            int64_t rows_per_pass) {
  ENTER(c);
  if (n_terms < 0) return fail(c, VMC_ERR_INVALID, "vmc_set_four_spin_terms: n_terms < 0");
  if (n_terms == 0) {                        // the ctx is what it was before it took terms
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fs = FourSpinBufs();
    return VMC_OK;
  }
  REFUSE_PRODUCT(c, "vmc_set_four_spin_terms");
  if (c->owner)
    return fail(c, VMC_ERR_STATE, c->owner->symz
        ? "vmc_set_four_spin_terms is not available on the base of a symmetrized ctx (vmc_create_symmetrized)"
        : "vmc_set_four_spin_terms is not available on a factor of a product ctx (vmc_create_product)");
  PROPAGATE(needs_ln_psi(c, "vmc_set_four_spin_terms"));
  char msg[256];
  const int rc = plan_fourspin_check(c->N, c->B, n_terms, ijkl, q, exchange_sign, rows_per_pass, msg, sizeof(msg));
  if (rc != VMC_OK) return fail(c, rc, msg);
  const FourSpinTable table = plan_fourspin_pairs(n_terms, ijkl);
  std::vector<double> wq((size_t)n_terms);
  for (int t = 0; t < n_terms; ++t) wq[(size_t)t] = -0.25 * (double)q[t];
  // the new set in buffers of its own: a failure below leaves the previous set in place
  FourSpinBufs next;
  next.n_terms = n_terms; next.n_pairs = table.n_pairs();
  next.exchange_sign = exchange_sign; next.rows_per_pass = rows_per_pass;
  PROPAGATE(next.pairs.alloc(c, next.n_pairs, "fs.pairs"));
  PROPAGATE(next.term_pairs.alloc(c, n_terms, "fs.term_pairs"));
  PROPAGATE(next.wq.alloc(c, n_terms, "fs.wq"));
  HIPCHK(c, hipMemcpy(next.pairs, table.pairs.data(), table.pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(next.term_pairs, table.term_pairs.data(), table.term_pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(next.wq, wq.data(), wq.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (work in flight may read the previous set)
  c->fs = std::move(next);
  return VMC_OK;
}

int vmc_last_four_spin_rows(vmc_ctx* c, int64_t* single_rows, int64_t* double_rows) {
  CHECK_CTX(c);
  if (!single_rows || !double_rows) return fail(c, VMC_ERR_INVALID, "null");
  *single_rows = c->fs.last_single;
  *double_rows = c->fs.last_double;
  return VMC_OK;
}

int vmc_pair_correlations(vmc_ctx* c, int which, int32_t n_pairs, const int32_t* ij, int32_t pairs_per_pass,
                          double* zz_sum, double* ex_sum) {
  MEASURE_GATE(c, which, "vmc_pair_correlations");
  if (n_pairs < 1 || !ij || pairs_per_pass < 0) return fail(c, VMC_ERR_INVALID, "bad pair arguments");
  std::vector<int2> pairs((size_t)n_pairs);
  for (int k = 0; k < n_pairs; ++k) {
    const int i = ij[2 * k], j = ij[2 * k + 1];
    if (i < 0 || j < 0 || i >= c->N || j >= c->N || i == j)
      return fail(c, VMC_ERR_INVALID, "pair site index out of range (or i == j)");
    pairs[(size_t)k] = make_int2(i, j);
  }
  const int per = plan_measure_per_pass(c->B, n_pairs, pairs_per_pass);
  if (per < 1) return fail(c, VMC_ERR_UNSUPPORTED, "batch_size does not leave room for one pair in the 32-bit row index");
  std::vector<double> out;
  PureMeasurement pure(c);
  PROPAGATE(ensure_cache(c, which));         // (before the swap: it reads no bond set; gnn / ed_vector readiness, parameters)
  PROPAGATE(corr_reserve(c, per, n_pairs));
  PROPAGATE(upload(c, c->corr.pairs.p, pairs));
  const CorrBufs& m = c->corr;
  HamiltonianSet hamiltonian(c);
  PROPAGATE(for_passes(n_pairs, per, [&](long long k0, int n) {
    install_set(c, BondSet{n, m.pairs + k0, m.hx, m.qz, m.rowinfo, m.val});
    return corr_pass(c, which, k0, n, n_pairs);
  }));
  PROPAGATE(read_back(pure, m.out, 2 * (size_t)n_pairs, &out));
  for (int k = 0; k < n_pairs; ++k) {
    if (zz_sum) zz_sum[k] = out[(size_t)k];
    if (ex_sum) ex_sum[k] = out[(size_t)n_pairs + (size_t)k];
  }
  return VMC_OK;
}

int vmc_renyi2_swap(vmc_ctx* c, int which, int32_t n_regions, const uint8_t* region_mask, int32_t regions_per_pass,
                    double* swap_sum, double* match_count) {
  MEASURE_GATE(c, which, "vmc_renyi2_swap");
  if (n_regions < 1 || !region_mask || regions_per_pass < 0) return fail(c, VMC_ERR_INVALID, "bad region arguments");
  if (c->B % 2 != 0) return fail(c, VMC_ERR_INVALID, "vmc_renyi2_swap pairs chain c with chain c + batch_size / 2: batch_size must be even");
  PROPAGATE(needs_ln_psi(c, "vmc_renyi2_swap"));
  std::vector<unsigned char> mask((size_t)n_regions * (size_t)c->N);
  for (size_t k = 0; k < mask.size(); ++k) {
    if (region_mask[k] > 1) return fail(c, VMC_ERR_INVALID, "region mask entries are 0 or 1");
    mask[k] = region_mask[k];
  }
  const int per = plan_measure_per_pass(c->B, n_regions, regions_per_pass, plan_measure_row_limit(c->N, c->Hp));
  if (per < 1) return fail(c, VMC_ERR_UNSUPPORTED, "batch_size does not leave room for one region in the 32-bit row index");
  std::vector<double> out;
  PureMeasurement pure(c);
  PROPAGATE(ensure_cache(c, which));         // l(x), l(y) and their signs, as the local energies take them
  PROPAGATE(renyi_reserve(c, n_regions));
  PROPAGATE(grow_tmp(c, (long long)per * c->B));
  PROPAGATE(upload(c, c->renyi.mask.p, mask));
  PROPAGATE(for_passes(n_regions, per, [&](long long k0, int n) { return renyi_pass(c, which, k0, n, n_regions); }));
  PROPAGATE(read_back(pure, c->renyi.out, 2 * (size_t)n_regions, &out));
  for (int k = 0; k < n_regions; ++k) {
    if (swap_sum) swap_sum[k] = out[(size_t)k];
    if (match_count) match_count[k] = out[(size_t)n_regions + (size_t)k];
  }
  return VMC_OK;
}

int vmc_dimer_correlations(vmc_ctx* c, int which, int32_t n_bonds, const int32_t* bonds, int32_t n_pairs,
                           const int32_t* pairs, int32_t pairs_per_pass, double* bond_sum, double* dd_sum) {
  MEASURE_GATE(c, which, "vmc_dimer_correlations");
  if (n_bonds < 1 || !bonds || n_pairs < 0 || (n_pairs > 0 && !pairs) || pairs_per_pass < 0)
    return fail(c, VMC_ERR_INVALID, "bad bond / pair arguments");
  std::vector<int2> hb((size_t)n_bonds), hp((size_t)n_pairs);
  for (int a = 0; a < n_bonds; ++a) {
    const int i = bonds[2 * a], j = bonds[2 * a + 1];
    if (i < 0 || j < 0 || i >= c->N || j >= c->N || i == j) {
      char msg[128];
      snprintf(msg, sizeof(msg), "bond %d = (%d, %d): two distinct sites in 0 .. %d required", a, i, j, c->N - 1);
      return fail(c, VMC_ERR_INVALID, msg);
    }
    hb[(size_t)a] = make_int2(i, j);
  }
  for (int p = 0; p < n_pairs; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || b < 0 || a >= n_bonds || b >= n_bonds) {
      char msg[128];
      snprintf(msg, sizeof(msg), "pair %d = (%d, %d): bond indices in 0 .. %d required", p, a, b, n_bonds - 1);
      return fail(c, VMC_ERR_INVALID, msg);
    }
    hp[(size_t)p] = make_int2(a, b);
  }
  PROPAGATE(needs_ln_psi(c, "vmc_dimer_correlations"));
  const long long row_limit = plan_measure_row_limit(c->N, c->Hp);
  const int per1 = plan_measure_per_pass(c->B, n_bonds, pairs_per_pass, row_limit);    // (a request splits both phases)
  const int per2 = n_pairs > 0 ? plan_measure_per_pass(c->B, n_pairs, pairs_per_pass, row_limit) : 0;
  if (per1 < 1 || (n_pairs > 0 && per2 < 1) || !plan_measure_rows_ok(c->B, n_bonds))
    return fail(c, VMC_ERR_UNSUPPORTED, "batch_size x bonds does not fit the 32-bit row index");
  std::vector<double> out;
  PureMeasurement pure(c);
  const DimerBufs& m = c->dimer;
  PROPAGATE(ensure_cache(c, which));         // ln|psi(x_c)| and the signs, as the local energies take them
  PROPAGATE(dimer_reserve(c, n_bonds, n_pairs));
  PROPAGATE(grow_tmp(c, (long long)(per1 > per2 ? per1 : per2) * c->B));
  PROPAGATE(upload(c, m.bonds.p, hb));
  if (n_pairs > 0) PROPAGATE(upload(c, m.pairs.p, hp));
  PROPAGATE(for_passes(n_bonds, per1, [&](long long a0, int n) { return dimer_single_pass(c, which, a0, n); }));
  {
    Timer t(c, "dimer_fold");
    HIPCHK(c, launch_dimer_bond_fold(c->stream, c->configs, m.bonds, own_amps(c, which), dimer_single_amps(c), c->B, c->N,
                                     n_bonds, m.out));
  }
  PROPAGATE(for_passes(n_pairs, per2, [&](long long p0, int n) { return dimer_double_pass(c, which, p0, n, m.out + n_bonds); }));
  PROPAGATE(read_back(pure, m.out, (size_t)n_bonds + (size_t)n_pairs, &out));
  for (int a = 0; a < n_bonds && bond_sum; ++a) bond_sum[a] = out[(size_t)a];
  for (int p = 0; p < n_pairs && dd_sum; ++p) dd_sum[p] = out[(size_t)n_bonds + (size_t)p];
  return VMC_OK;
}

int vmc_symmetry_expectations(vmc_ctx* c, int which, int32_t n_ops, const int32_t* perm, const uint8_t* flip,
                              int32_t ops_per_pass, double* ratio_sum) {
  MEASURE_GATE(c, which, "vmc_symmetry_expectations");
  SymmOps ops;
  PROPAGATE(symm_ops_check(c, n_ops, perm, flip, ops_per_pass, &ops));
  PROPAGATE(needs_ln_psi(c, "vmc_symmetry_expectations"));
  const int per = plan_measure_per_pass(c->B, n_ops, ops_per_pass, plan_measure_row_limit(c->N, c->Hp));
  if (per < 1) return fail(c, VMC_ERR_UNSUPPORTED, "batch_size does not leave room for one op in the 32-bit row index");
  std::vector<double> out;
  PureMeasurement pure(c);
  PROPAGATE(ensure_cache(c, which));         // ln|psi(x_c)| and the signs, as the local energies take them
  PROPAGATE(symm_ops_upload(c, ops));
  PROPAGATE(c->symm.out.reserve(c, n_ops, "symm.out"));
  PROPAGATE(grow_tmp(c, (long long)per * c->B));
  PROPAGATE(for_passes(n_ops, per, [&](long long k0, int n) { return symm_pass(c, which, k0, n); }));
  PROPAGATE(read_back(pure, c->symm.out, (size_t)n_ops, &out));
  for (int k = 0; k < n_ops && ratio_sum; ++k) ratio_sum[k] = out[(size_t)k];
  return VMC_OK;
}

int vmc_projected_energy(vmc_ctx* c, int which, int32_t n_ops, const int32_t* perm, const uint8_t* flip,
                         int32_t n_sectors, const double* chi, int32_t ops_per_pass, double* w_sum, double* we_sum,
                         double* e_sum, int64_t* n_alive) {
  MEASURE_GATE(c, which, "vmc_projected_energy");
  if (c->fs.n_terms > 0)
    return fail(c, VMC_ERR_UNSUPPORTED, "vmc_projected_energy is not available while four-spin terms are set (vmc_set_four_spin_terms): the symmetry check does not cover them");
  SymmOps ops;
  PROPAGATE(symm_ops_check(c, n_ops, perm, flip, ops_per_pass, &ops));
  char msg[256];
  if (n_sectors < 1 || !chi) return fail(c, VMC_ERR_INVALID, "bad sector arguments: n_sectors >= 1 and the characters chi [n_sectors][n_ops] required");
  if (!plan_proj_acc_ok(c->B, n_sectors)) {
    snprintf(msg, sizeof(msg), "n_sectors x batch_size = %lld beyond the accumulator budget of 2^26 doubles", (long long)n_sectors * c->B);
    return fail(c, VMC_ERR_UNSUPPORTED, msg);
  }
  for (size_t e = 0; e < (size_t)n_sectors * (size_t)n_ops; ++e)
    if (!std::isfinite(chi[e])) {
      snprintf(msg, sizeof(msg), "sector %d: the character of op %d is not finite", (int)(e / (size_t)n_ops), (int)(e % (size_t)n_ops));
      return fail(c, VMC_ERR_INVALID, msg);
    }
  PROPAGATE(needs_ln_psi(c, "vmc_projected_energy"));
  const int per = plan_measure_per_pass(c->B, n_ops, ops_per_pass, plan_measure_row_limit(c->N, c->Hp));
  if (per < 1) return fail(c, VMC_ERR_UNSUPPORTED, "batch_size does not leave room for one op in the 32-bit row index");
  if (c->n_bonds <= 0) return fail(c, VMC_ERR_STATE, "bonds not set (vmc_set_bonds)");
  if (plan_symm_check_hamiltonian(c->N, c->n_bonds, c->ham_ij.data(), c->ham_jx.data(), c->ham_jz.data(), n_ops, perm, msg,
                                  sizeof(msg)) != VMC_OK)
    return fail(c, VMC_ERR_INVALID, msg);
  const std::vector<double> hchi(chi, chi + (size_t)n_sectors * (size_t)n_ops);
  int cnt_total = 0;
  std::vector<double> out;
  PureMeasurement pure(c);
  ProjBufs& m = c->proj;
  PROPAGATE(ensure_cache(c, which));         // ln|psi(x_c)| and the signs, as the local energies take them
  {
    Timer t(c, "proj_eloc");                 // first: its rows go through the buffers the passes then take
    PROPAGATE(local_energy_device(c, which));
  }
  PROPAGATE(symm_ops_upload(c, ops));
  PROPAGATE(proj_reserve(c, n_ops, n_sectors));
  PROPAGATE(grow_tmp(c, (long long)per * c->B));
  PROPAGATE(upload(c, m.chi.p, hchi));
  HIPCHK(c, hipMemsetAsync(m.acc, 0, (size_t)n_sectors * (size_t)c->B * sizeof(double), c->stream));
  PROPAGATE(for_passes(n_ops, per, [&](long long k0, int n) { return proj_pass(c, which, k0, n, n_ops, n_sectors); }));
  {
    Timer t(c, "proj_fold");
    HIPCHK(c, launch_proj_fold(c->stream, own_amps(c, which).sign, c->ps[which].eloc, m.acc, c->B, n_sectors, m.out));
    HIPCHK(c, hipMemcpyAsync(&cnt_total, c->off + c->B, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  PROPAGATE(read_back(pure, m.out, 2 * (size_t)n_sectors + 2, &out));
  c->last_rows = cnt_total;                  // (as vmc_local_energy leaves it)
  for (int s = 0; s < n_sectors; ++s) {
    if (w_sum) w_sum[s] = out[(size_t)s];
    if (we_sum) we_sum[s] = out[(size_t)n_sectors + (size_t)s];
  }
  if (e_sum) *e_sum = out[2 * (size_t)n_sectors];
  if (n_alive) *n_alive = (int64_t)out[2 * (size_t)n_sectors + 1];
  return VMC_OK;
}

int vmc_energy_moments(vmc_ctx* c, int which, int64_t rows_per_pass, double sums[6], double* e_loc, double* h2_loc,
                       int64_t* n_rows2) {
  MEASURE_GATE(c, which, "vmc_energy_moments");
  if (c->fs.n_terms > 0)
    return fail(c, VMC_ERR_UNSUPPORTED, "vmc_energy_moments is not available while four-spin terms are set (vmc_set_four_spin_terms): the rows of H^2 do not cover them");
  if (rows_per_pass < 0) return fail(c, VMC_ERR_INVALID, "bad rows_per_pass (0: the library decides)");
  PROPAGATE(needs_ln_psi(c, "vmc_energy_moments"));
  if (c->n_bonds <= 0) return fail(c, VMC_ERR_STATE, "bonds not set (vmc_set_bonds)");
  if (!plan_moment_index_ok(c->B, c->n_bonds))
    return fail(c, VMC_ERR_UNSUPPORTED, "batch_size x n_bonds^2 does not fit the 32-bit row index of the second-order list");
  int n1 = 0, n2 = 0;
  std::vector<double> chain, out;
  PureMeasurement pure(c);
  MomentBufs& m = c->mom;
  PROPAGATE(ensure_cache(c, which));         // ln|psi(x_c)| and the signs, as the local energies take them
  {
    Timer t(c, "mom_eloc");                  // first: its rows go through the buffers the passes then take
    PROPAGATE(local_energy_device(c, which));
  }
  PROPAGATE(read_ints(c, c->off + c->B, &n1, 1));
  PROPAGATE(mom_reserve_list(c, n1));
  {
    Timer t(c, "mom_list");
    HIPCHK(c, launch_mom_count(c->stream, c->configs, c->bonds, c->half_jx, c->quarter_jz, c->rowinfo, c->off + c->B, n1,
                               c->N, c->n_bonds, c->num_cus, m.cnt2, m.off2, m.diag1, m.self1));
    HIPCHK(c, hipMemsetAsync(m.lanes, 0, 64 * (size_t)c->B * sizeof(double), c->stream));
  }
  PROPAGATE(read_ints(c, m.off2 + n1, &n2, 1));
  const long long per = plan_list_per_pass(n2, rows_per_pass, plan_measure_row_limit(c->N, c->Hp));
  if (per < 1) return fail(c, VMC_ERR_HIP, "the second-order list has a negative length");
  PROPAGATE(m.desc.reserve(c, per, "mom.desc"));
  PROPAGATE(m.coef.reserve(c, per, "mom.coef"));
  PROPAGATE(grow_tmp(c, per));
  PROPAGATE(for_passes(n2, (int)per, [&](long long q0, int n) { return mom_pass(c, which, q0, n, n1); }));
  {
    Timer t(c, "mom_fold");
    HIPCHK(c, launch_mom_fold(c->stream, c->configs, c->bonds, c->half_jx, c->quarter_jz, c->rowinfo, c->off, c->val,
                              c->ps[which].eloc, own_amps(c, which).sign, m.diag1, m.self1, m.lanes, c->B, c->N, c->n_bonds,
                              m.chain, m.out));
    if (e_loc || h2_loc) {
      chain.resize(2 * (size_t)c->B);
      HIPCHK(c, hipMemcpyAsync(chain.data(), m.chain, chain.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
  }
  PROPAGATE(read_back(pure, m.out, 6, &out));
  c->last_rows = n1;                         // (as vmc_local_energy leaves it)
  for (int k = 0; k < 6 && sums; ++k) sums[k] = out[(size_t)k];
  for (int k = 0; k < c->B && e_loc; ++k) e_loc[k] = chain[(size_t)k];
  for (int k = 0; k < c->B && h2_loc; ++k) h2_loc[k] = chain[(size_t)c->B + (size_t)k];
  if (n_rows2) *n_rows2 = n2;
  return VMC_OK;
}

int vmc_overlap(vmc_ctx* c, double sums[4], double* ratio) {
  MEASURE_GATE(c, 0, "vmc_overlap");
  PROPAGATE(overlap_refusals(c, "vmc_overlap"));
  std::vector<double> chain, out;
  PureMeasurement pure(c);
  OverlapBufs& m = c->ovl;
  PROPAGATE(ensure_cache(c, VMC_OMEGA));
  PROPAGATE(ensure_cache(c, VMC_PSI));
  PROPAGATE(overlap_sums_device(c));
  if (ratio) {
    PROPAGATE(m.ratio.reserve(c, c->B, "ovl.ratio"));
    chain.resize((size_t)c->B);
    HIPCHK(c, launch_overlap_weights(c->stream, m.d, m.code, m.out, nullptr, 0.f, c->B, nullptr, m.ratio));
    HIPCHK(c, hipMemcpyAsync(chain.data(), m.ratio, chain.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  PROPAGATE(read_back(pure, m.out, 4, &out));
  for (int k = 0; k < 4 && sums; ++k) sums[k] = out[(size_t)k];
  for (int k = 0; k < c->B && ratio; ++k) ratio[k] = chain[(size_t)k];
  return VMC_OK;
}

}  // extern "C"
