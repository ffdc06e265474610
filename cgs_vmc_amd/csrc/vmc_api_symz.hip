// The symmetrized ctx of the C ABI (include/cgsvmc.h, vmc_create_symmetrized): psi_s(x) = sum_k chi_k psi(g_k x) over one
// set of B chains, the g_k site permutations optionally followed by the global spin flip, chi the real characters of one
// sector.  When every g_k is a symmetry of the Hamiltonian, with c_k(x) = chi_k psi(g_k x) / psi_s(x) (sum_k c_k = 1):
//   E_loc^s(x) = sum_k c_k(x) E_loc^psi(g_k x)        O^s_j(x) = sum_k c_k(x) O_j(g_k x)
// so the composite needs no connected-row machinery of its own: the base ctx holds the n_ops B permuted rows (row = k B + c)
// as ITS chains and does all network arithmetic through three of its host-side primitives (ensure_cache,
// local_energy_device, child_gradient_sums), and symz.hip adds the kernels in between.
//
// Ownership, as for a product: the symmetrized ctx is a vmc_ctx of its own (made by vmc_create with a minimal dense shape
// whose network members stay unused) that owns the chains, the step counter, the bond tables it needs, the accumulators
// [2 P + 8] and the Adam state.  theta IS the base's: the parameter entries of the composite forward to the base, Adam runs
// on the base's buffer.  The base's `configs` holds the permuted chains (SymzState::on_chains) or whatever rows the
// sampler / vmc_amplitude put there last.
#include "vmc_ctx.hpp"
#include "prod.hpp"
#include "symz.hpp"

using namespace vmcapi;

struct SymzState {
  vmc_ctx* base = nullptr;
  int n_ops = 0;
  bool on_chains = false;                   // the base's configs are the permuted chains
  bool dead = false;                        // the base was destroyed while composed: every entry refuses
  std::vector<int32_t> h_perm;              // [n_ops][N] (vmc_set_bonds asks whether the ops are symmetries)
  DevBuf<int> perm;                         // [n_ops][N]
  DevBuf<unsigned char> flip;               // [n_ops]
  DevBuf<double> chi;                       // [n_ops]
  DevBuf<float> l[2], s[2];                 // [which][B] psi_s of the CHAINS: fl32(m + ln|S|) and the sign (ed_vector base: psi_s
                                            // itself); what vmc_ctx::ps[which].cache_valid of the composite vouches for
  DevBuf<float> rl, rs;                     // [B] psi_s of a block of vmc_amplitude's host rows
  DevBuf<float> ck, wk;                     // [n_ops][B] c_k and E_s c_k of the latest local energies (the gradient's weights)
  DevBuf<float> g_scratch;                  // [P] the unweighted sum child_gradient_sums yields beside the one that is wanted
  DevBuf<int> iup, idn;                     // [B] the proposal in flight
  DevBuf<float> u;
  DevBuf<unsigned> acc_cnt;                 // [B] acceptances of a launch, per chain
};

namespace vmcapi {

int symz_alive(vmc_ctx* c) {
  if (c->symz->dead) return fail(c, VMC_ERR_STATE, "symmetrized: the base of this symmetrized ctx has been destroyed");
  return VMC_OK;
}

static int base_rc(vmc_ctx* c, vmc_ctx* b, int rc) {
  if (rc != VMC_OK) c->err = b->err;
  return rc;
}
#define BASE(c, b, expr) do { int rc_b_ = base_rc((c), (b), (expr)); if (rc_b_ != VMC_OK) return rc_b_; } while (0)

static SymzRows base_rows(const vmc_ctx* c, int which) {
  const SymzState* st = c->symz;
  const vmc_ctx* b = st->base;
  SymzRows r;
  r.logit = b->ps[which].logit; r.sign = b->sgn ? b->ps[which].sign.p : nullptr;
  r.chi = st->chi; r.n_ops = st->n_ops; r.B = c->B;
  r.amp = b->path == PATH_EDVEC ? 1 : 0;
  return r;
}

void symz_chains_changed(vmc_ctx* c) { c->symz->on_chains = false; }

void symz_base_params_changed(vmc_ctx* base, int which) {
  vmc_ctx* o = base->owner;
  if (!o || !o->symz) return;
  o->ps[which].cache_valid = false;
}

void symz_base_destroyed(vmc_ctx* base) {
  vmc_ctx* o = base->owner;
  if (o && o->symz) { o->symz->dead = true; o->symz->base = nullptr; }
  base->owner = nullptr;
}

void symz_release(vmc_ctx* c) {
  SymzState* st = c->symz;
  if (!st) return;
  if (st->base) { st->base->owner = nullptr; invalidate_configs(st->base); }
  delete st;
  c->symz = nullptr;
}

// the base reads the permuted chains: k_symm_rows per change of the chains
static int symz_sync_base(vmc_ctx* c) {
  SymzState* st = c->symz;
  PROPAGATE(symz_alive(c));
  if (st->on_chains) return VMC_OK;
  {
    Timer t(c, "symz_rows");
    HIPCHK(c, launch_symm_rows(c->stream, c->configs, st->perm, st->flip, c->B, c->N, st->n_ops, c->num_cus, st->base->configs));
  }
  invalidate_configs(st->base);
  st->on_chains = true;
  return VMC_OK;
}

// psi_s of the chains for parameter set `which`
int symz_ensure_cache(vmc_ctx* c, int which) {
  SymzState* st = c->symz;
  PROPAGATE(symz_alive(c));
  if (c->ps[which].cache_valid) return VMC_OK;      // (also what the sampler left: psi_s of the final chains)
  PROPAGATE(symz_sync_base(c));
  BASE(c, st->base, ensure_cache(st->base, which));
  {
    Timer t(c, "symz_fold");
    HIPCHK(c, launch_symz_fold(c->stream, base_rows(c, which), st->l[which], st->s[which]));
  }
  c->ps[which].cache_valid = true;
  return VMC_OK;
}

// E_s(c) = sum_k c_k E_loc^psi(g_k x_c): the base's own local energies on the permuted chains, folded
int symz_local_energy(vmc_ctx* c, int which) {
  SymzState* st = c->symz;
  PROPAGATE(symz_alive(c));
  if (c->n_bonds <= 0) return fail(c, VMC_ERR_STATE, "bonds not set (vmc_set_bonds)");
  PROPAGATE(symz_sync_base(c));
  vmc_ctx* b = st->base;
  BASE(c, b, local_energy_device(b, which));
  {
    Timer t(c, "eloc_fold");
    HIPCHK(c, launch_symz_eloc_fold(c->stream, base_rows(c, which), b->ps[which].eloc, b->diag, b->offdiag,
                                    c->ps[which].eloc, c->diag, c->offdiag, st->ck, st->wk));
  }
  // (vmc_local_energy / vmc_evaluate read the row count off the composite: the base's, over all ops)
  HIPCHK(c, hipMemcpyAsync(c->off + c->B, b->off + b->B, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  return VMC_OK;
}

// n_steps x mc_step: per step the permuted candidates straight into the base's `configs`, a full forward of the base on
// them -- the route vmc_amplitude takes --, and one kernel that folds, accepts and draws the next proposal
int symz_run_sweep(vmc_ctx* c, const SweepCall& call) {
  SymzState* st = c->symz;
  PROPAGATE(symz_alive(c));
  const int B = c->B, N = c->N;
  PROPAGATE(symz_ensure_cache(c, VMC_PSI));
  PROPAGATE(zero_accepted(c, call, c->stream));
  if (call.n_steps <= 0) return VMC_OK;
  vmc_ctx* b = st->base;
  Timer t(c, "sweep");
  HIPCHK(c, hipMemsetAsync(st->acc_cnt, 0, (size_t)B * sizeof(unsigned), c->stream));
  HIPCHK(c, launch_proposals(c, c->stream, call.step0, call.injected, st->iup, st->idn, st->u));
  for (long long s = 0; s < call.n_steps; ++s) {
    HIPCHK(c, launch_symz_candidates(c->stream, c->configs, st->iup, st->idn, st->perm, st->flip, B, N, st->n_ops,
                                     c->num_cus, b->configs));
    st->on_chains = false;
    invalidate_configs(b);
    BASE(c, b, ensure_cache(b, VMC_PSI));
    SymzAcceptArgs x;
    memset((void*)&x, 0, sizeof(x));
    x.configs = c->configs; x.N = N;
    x.iup = st->iup; x.idn = st->idn; x.u = st->u;
    x.cand = base_rows(c, VMC_PSI);
    x.logit = st->l[0]; x.sign = st->s[0];
    x.acc_mask = call.injected ? c->acc_mask.p : nullptr;
    x.acc_cnt = st->acc_cnt;
    x.draw_next = (!call.injected && s + 1 < call.n_steps) ? 1 : 0;
    x.next_step = call.step0 + (unsigned long long)s + 1;
    set_key(c, x);
    HIPCHK(c, launch_symz_accept(c->stream, x));
  }
  HIPCHK(c, launch_prod_count_fold(c->stream, st->acc_cnt, B, c->d_accepted));
  return chains_moved(c, call);
}

// TrainOps.accumulate_gradients of psi_s (EnergyGradient): g1 = sum_c sum_k c_k O(g_k x_c), g2 = sum_c E_s(c) sum_k c_k O(g_k x_c)
// through the base's gradient path over its n_ops B rows, once per weight vector: child_gradient_sums yields the
// unweighted sum (into the scratch) and ONE weighted sum per call
int symz_accumulate(vmc_ctx* c, int mode, float beta) {
  (void)beta;
  SymzState* st = c->symz;
  PROPAGATE(symz_alive(c));
  if (mode != VMC_MODE_ENERGY_GRADIENT)
    return fail(c, VMC_ERR_UNSUPPORTED, "vmc_accumulate: only VMC_MODE_ENERGY_GRADIENT is available on a symmetrized ctx ('symmetrized')");
  PROPAGATE(symz_local_energy(c, VMC_PSI));
  PROPAGATE(acc_zeros(c));
  vmc_ctx* b = st->base;
  {
    Timer t(c, "grad");
    BASE(c, b, ensure_cache(b, VMC_PSI));
    HIPCHK(c, hipMemsetAsync(st->g_scratch, 0, (size_t)c->P * sizeof(float), c->stream));
    BASE(c, b, child_gradient_sums(b, st->ck, st->g_scratch, c->acc));
    BASE(c, b, child_gradient_sums(b, st->wk, st->g_scratch, c->acc + c->P));
    HIPCHK(c, launch_scalar_accum(c->stream, c->ps[0].eloc, nullptr, c->B, c->acc + 2 * c->P, mode, false));
  }
  c->acc_fresh = false;
  c->acc_since_sweep = true;
  c->token = false;
  return VMC_OK;
}

// the ops must map the bond set onto itself: the two identities above hold only then
int symz_set_bonds_check(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z) {
  PROPAGATE(symz_alive(c));
  char msg[320];
  const int rc = plan_symm_check_hamiltonian(c->N, n_bonds, ij, j_x, j_z, c->symz->n_ops, c->symz->h_perm.data(), msg, sizeof(msg));
  if (rc != VMC_OK) return fail(c, rc, std::string("symmetrized: ") + msg);
  return VMC_OK;
}

int symz_set_bonds(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z) {
  PROPAGATE(symz_alive(c));
  BASE(c, c->symz->base, vmc_set_bonds(c->symz->base, n_bonds, ij, j_x, j_z));
  return VMC_OK;
}

int symz_set_params(vmc_ctx* c, int which, const float* theta) {
  PROPAGATE(symz_alive(c));
  BASE(c, c->symz->base, vmc_set_params(c->symz->base, which, theta));     // (the base tells its owner: symz_base_params_changed)
  return VMC_OK;
}

int symz_get_params(vmc_ctx* c, int which, float* theta) {
  PROPAGATE(symz_alive(c));
  BASE(c, c->symz->base, vmc_get_params(c->symz->base, which, theta));
  return VMC_OK;
}

int symz_transfer_params(vmc_ctx* c) {
  PROPAGATE(symz_alive(c));
  BASE(c, c->symz->base, vmc_transfer_params(c->symz->base));
  return VMC_OK;
}

// Adam on the base's theta from the composite's accumulators and moments
int symz_adam_theta(vmc_ctx* c, float** theta) {
  PROPAGATE(symz_alive(c));
  vmc_ctx* b = c->symz->base;
  if (!b->ps[0].has_params) return fail(c, VMC_ERR_STATE, "parameters not set");
  *theta = b->ps[0].theta;
  return VMC_OK;
}

void symz_adam_applied(vmc_ctx* c) {
  vmc_ctx* b = c->symz->base;
  b->ps[0].packed_valid = b->ps[0].cache_valid = false;
  b->acts_valid = false;
  c->ps[0].cache_valid = false;
}

// logit = fl32(m + ln|S|) - shift_base, psi = sgn(S) exp(logit) (an ed_vector base: the folded amplitude itself); psi = 0,
// logit = -inf at a structural zero.  Host rows go through the base in blocks of batch_size rows by the route the sampler's
// candidates take (a short last block repeats its first row).
int symz_amplitude(vmc_ctx* c, int which, const float* configs, int64_t n_rows, float* logit, float* psi) {
  SymzState* st = c->symz;
  PROPAGATE(symz_alive(c));
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  if (n_rows < 0) return fail(c, VMC_ERR_INVALID, "n_rows < 0");
  const int B = c->B, N = c->N;
  vmc_ctx* b = st->base;
  const float shift = b->ps[which].shift;
  const bool amp = b->path == PATH_EDVEC;
  std::vector<float> hl((size_t)B), hs((size_t)B);
  auto finish = [&](const float* dl, const float* ds, int64_t row0, int n) -> int {
    HIPCHK(c, hipMemcpyAsync(hl.data(), dl, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hs.data(), ds, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
      const bool zero = hs[i] == 0.f;
      const float lg = zero ? -INFINITY : hl[i] - shift;
      if (logit) logit[row0 + i] = lg;
      if (psi) psi[row0 + i] = zero ? 0.f : amp ? hs[i] : (hs[i] > 0.f ? 1.f : -1.f) * expf(lg);
    }
    return VMC_OK;
  };
  if (!configs) {
    if (n_rows != B) return fail(c, VMC_ERR_INVALID, "n_rows must equal batch_size when configs == NULL");
    PROPAGATE(symz_ensure_cache(c, which));
    return finish(st->l[which], st->s[which], 0, B);
  }
  PROPAGATE(check_sz0_rows(c, configs, n_rows));
  for (int64_t i = 0; i < n_rows * N; ++i)
    if (configs[i] != 1.f && configs[i] != -1.f) return fail(c, VMC_ERR_INVALID, "configs must be +-1");
  PROPAGATE(grow_tmp(c, B));
  std::vector<float> blk((size_t)B * N);
  for (int64_t row0 = 0; row0 < n_rows; row0 += B) {
    const int n = (int)(n_rows - row0 < B ? n_rows - row0 : B);
    for (int r = 0; r < B; ++r)
      memcpy(blk.data() + (size_t)r * N, configs + (size_t)(row0 + (r < n ? r : 0)) * N, (size_t)N * sizeof(float));
    HIPCHK(c, hipMemcpyAsync(c->tmp_cfg, blk.data(), blk.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    {
      Timer t(c, "symz_rows");
      HIPCHK(c, launch_symm_rows(c->stream, c->tmp_cfg, st->perm, st->flip, B, N, st->n_ops, c->num_cus, b->configs));
    }
    st->on_chains = false;
    invalidate_configs(b);
    HIPCHK(c, hipStreamSynchronize(c->stream));       // (blk is reused by the next block)
    BASE(c, b, ensure_cache(b, which));
    {
      Timer t(c, "symz_fold");
      HIPCHK(c, launch_symz_fold(c->stream, base_rows(c, which), st->rl, st->rs));
    }
    PROPAGATE(finish(st->rl, st->rs, row0, n));
  }
  return VMC_OK;
}

// vmc_set_configs: a batch with a row at a structural zero is refused before the chains are touched.  The zero is read
// off the logit (-inf there and nowhere else): psi = exp(logit - shift) also rounds to 0 below fp32's range, on rows the
// sampler -- which compares logits -- may well hold
int symz_check_configs(vmc_ctx* c, const float* configs) {
  const int B = c->B;
  std::vector<float> logit((size_t)B);
  PROPAGATE(symz_amplitude(c, VMC_PSI, configs, B, logit.data(), nullptr));
  int first = -1, zeros = 0;
  for (int r = 0; r < B; ++r)
    if (logit[(size_t)r] == -INFINITY) { if (first < 0) first = r; ++zeros; }
  if (zeros == B)
    return fail(c, VMC_ERR_INVALID, "symmetrized: every row is at a structural zero of psi_s: the state has no weight in this sector");
  if (zeros > 0) {
    char msg[200];
    snprintf(msg, sizeof(msg), "symmetrized: row %d is at a structural zero of psi_s in this sector (%d of %d rows are): the chains need psi_s != 0",
             first, zeros, B);
    return fail(c, VMC_ERR_INVALID, msg);
  }
  return VMC_OK;
}

}  // namespace vmcapi

extern "C" {

int vmc_create_symmetrized(vmc_ctx* base, int32_t batch_size, int32_t n_ops, const int32_t* perms, const uint8_t* flips,
                           const double* characters, vmc_ctx** out) {
  if (!base || !out) return fail(nullptr, VMC_ERR_INVALID, "null argument");
  *out = nullptr;
  {
    char msg[320];
    const int rc = plan_symz_check(base->d.ansatz, base->oact, base->prod != nullptr || base->symz != nullptr,
                                   base->owner != nullptr, base->B, base->N, batch_size, n_ops, perms, flips, characters, msg,
                                   sizeof(msg));
    if (rc != VMC_OK) return fail(nullptr, rc, msg);
  }
  if (base->fs.n_terms > 0)
    return fail(nullptr, VMC_ERR_UNSUPPORTED, "vmc_create_symmetrized: the base holds four-spin terms (vmc_set_four_spin_terms); a symmetrized ctx has none -- remove them first (n_terms = 0)");
  bool any_flip = false;
  for (int k = 0; flips && k < n_ops; ++k) any_flip = any_flip || flips[k] != 0;
  // the composite's own ctx: chains, bond tables, accumulators, scratch -- a minimal dense shape whose network stays unused
  vmc_desc d;
  memset(&d, 0, sizeof(d));
  d.n_sites = base->N; d.batch_size = batch_size; d.num_layers = 1; d.layer_size = 1;
  d.nonlinearity = VMC_ACT_RELU; d.output_activation = VMC_ACT_EXP;
  d.device = base->d.device; d.chain_offset = base->d.chain_offset; d.ansatz = VMC_ANSATZ_FULLY_CONNECTED;
  d.seed = base->d.seed; d.stream = base->d.stream;
  vmc_ctx* c = nullptr;
  PROPAGATE(vmc_create(&d, &c));
  DeviceGuard device_guard_(c->d.device);
  c->d.ansatz = VMC_ANSATZ_SYMMETRIZED;
  c->path = PATH_SYMMETRIZED;
  c->overlap = false;
  c->sweep8_ok = false; c->sweep_tile = 16;
  c->sgn = base->sgn || any_flip;             // Sz = 0 rows only: a flip keeps only those in their sector (check_sz0_rows)
  c->ps[0].shift = c->ps[1].shift = 0.f;
  SymzState* st = new SymzState();
  c->symz = st;
  st->base = base; st->n_ops = n_ops;
  const long long P = base->P, B = c->B, N = c->N, R = (long long)n_ops * B;
#define CP(expr) do { hipError_t e2 = (expr); if (e2 != hipSuccess) { \
    g_create_error = std::string(#expr) + ": " + hipGetErrorString(e2); st->base = nullptr; vmc_destroy(c); return VMC_ERR_HIP; } } while (0)
#define NEW(buf, n) do { if ((buf).alloc(c, (n), #buf) != VMC_OK) { g_create_error = c->err; st->base = nullptr; vmc_destroy(c); return VMC_ERR_HIP; } } while (0)
  // everything sized by P, allocated anew at the base's P (alloc frees what vmc_create put there)
  c->P = P;
  NEW(c->acc, plan_symz_acc_floats(P)); NEW(c->adam_m, P); NEW(c->adam_v, P); NEW(c->grad_tmp, P);
  NEW(st->g_scratch, P);
  CP(hipMemsetAsync(c->acc, 0, (size_t)plan_symz_acc_floats(P) * sizeof(float), c->stream));
  CP(hipMemsetAsync(c->adam_m, 0, P * sizeof(float), c->stream));
  CP(hipMemsetAsync(c->adam_v, 0, P * sizeof(float), c->stream));
  st->h_perm.assign(perms, perms + (size_t)n_ops * N);
  std::vector<unsigned char> hf((size_t)n_ops, 0);
  for (int k = 0; flips && k < n_ops; ++k) hf[(size_t)k] = flips[k];
  NEW(st->perm, (long long)n_ops * N); NEW(st->flip, n_ops); NEW(st->chi, n_ops);
  CP(hipMemcpy(st->perm, perms, (size_t)n_ops * N * sizeof(int32_t), hipMemcpyHostToDevice));
  CP(hipMemcpy(st->flip, hf.data(), (size_t)n_ops, hipMemcpyHostToDevice));
  CP(hipMemcpy(st->chi, characters, (size_t)n_ops * sizeof(double), hipMemcpyHostToDevice));
  for (int w = 0; w < 2; ++w) {
    NEW(st->l[w], B); NEW(st->s[w], B);
    CP(hipMemsetAsync(st->l[w], 0, B * sizeof(float), c->stream));
    CP(launch_fill(c->stream, st->s[w], 1.f, B));
  }
  NEW(st->rl, B); NEW(st->rs, B);
  NEW(st->ck, R); NEW(st->wk, R);
  CP(hipMemsetAsync(st->ck, 0, R * sizeof(float), c->stream));
  CP(hipMemsetAsync(st->wk, 0, R * sizeof(float), c->stream));
  NEW(st->iup, B); NEW(st->idn, B); NEW(st->u, B); NEW(st->acc_cnt, B);
  CP(hipMemsetAsync(st->acc_cnt, 0, B * sizeof(unsigned), c->stream));
  CP(hipStreamSynchronize(c->stream));
#undef NEW
#undef CP
  base->owner = c;
  invalidate_configs(base);
  *out = c;
  return VMC_OK;
}

}  // extern "C"
