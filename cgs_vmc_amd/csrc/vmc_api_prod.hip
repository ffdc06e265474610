// The product ctx of the C ABI (include/cgsvmc.h, vmc_create_product): psi = psi_a psi_b over one set of chains
// (wavefunctions.py:61-165 ProductOfWavefunctions, 1178-1194).  ln|psi| = ln|psi_a| + ln|psi_b|: the Metropolis test adds two
// logit differences, the signs multiply, a connected configuration's ratio is the product of the factors' ratios, and
// O_k of a factor is unchanged -- so the factors' own kernels do all the network arithmetic, through three of their
// host-side primitives (ensure_cache: amplitudes of B device rows; local_energy_device: the row values; child_gradient_sums:
// sum O and sum w O for an external weight vector), and prod.hip adds the kernels in between.
//
// Ownership: the product ctx is a vmc_ctx of its own (made by vmc_create with a minimal dense shape whose network members
// stay unused) that owns the chains, the step counter, the bond tables it needs, the accumulators [2 P + 8], the Adam
// state and a concatenated theta [a | b] that is scratch between the factors' own theta (gathered before, scattered after
// every entry that reads or writes it).  A factor's `configs` is a device copy: of the chains (ProdState::on_chains) or of
// the sampler's candidates.
#include "vmc_ctx.hpp"
#include "prod.hpp"

using namespace vmcapi;

// psi = psi_a psi_b.  The product ctx owns the chains (vmc_ctx::configs); a factor reads them through a device copy in
// its own `configs` (on_chains tells whether that copy is the chains -- the sampler overwrites it with the candidates).
// l / s: the factors' logits and signs of the CHAINS, per parameter set; they are what vmc_ctx::ps[which].cache_valid of
// the product vouches for.  A factor without a sign keeps s = 1; ed_vector keeps psi itself there (its sign is what counts).
struct ProdState {
  vmc_ctx* child[2] = {nullptr, nullptr};
  long long P[2] = {0, 0};
  bool on_chains = false;
  bool dead = false;                        // a factor was destroyed while composed (its child[] entry is null): every entry refuses
  DevBuf<float> l[2][2], s[2][2];           // [which][factor][B]
  DevBuf<int> iup, idn;                     // [B] the proposal in flight
  DevBuf<float> u;
  DevBuf<unsigned> acc_cnt;                 // [B] acceptances of a launch, per chain
};

namespace vmcapi {

int prod_alive(vmc_ctx* c) {
  if (c->prod->dead) return fail(c, VMC_ERR_STATE, "prod: a factor of this product ctx has been destroyed");
  return VMC_OK;
}

// the factors read the chains: a device copy per change of the chains
static int prod_sync_children(vmc_ctx* c) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  if (st->on_chains) return VMC_OK;
  const size_t bytes = (size_t)c->B * c->N * sizeof(float);
  for (int i = 0; i < 2; ++i) {
    HIPCHK(c, hipMemcpyAsync(st->child[i]->configs, c->configs, bytes, hipMemcpyDeviceToDevice, c->stream));
    invalidate_configs(st->child[i]);
  }
  st->on_chains = true;
  return VMC_OK;
}

// a factor's error message travels to the product
static int child_rc(vmc_ctx* c, vmc_ctx* ch, int rc) {
  if (rc != VMC_OK) c->err = ch->err;
  return rc;
}
#define CHILD(c, ch, expr) do { int rc_c_ = child_rc((c), (ch), (expr)); if (rc_c_ != VMC_OK) return rc_c_; } while (0)

void prod_chains_changed(vmc_ctx* c) { c->prod->on_chains = false; }

void prod_child_params_changed(vmc_ctx* child, int which) {
  vmc_ctx* o = child->owner;
  if (!o || !o->prod) return;
  o->ps[which].cache_valid = false;
}

void prod_child_destroyed(vmc_ctx* child) {
  vmc_ctx* o = child->owner;
  if (o && o->prod) {
    o->prod->dead = true;
    for (int i = 0; i < 2; ++i)
      if (o->prod->child[i] == child) o->prod->child[i] = nullptr;     // (prod_release frees only the factor still alive)
  }
  child->owner = nullptr;
}

void prod_release(vmc_ctx* c) {
  ProdState* st = c->prod;
  if (!st) return;
  for (int i = 0; i < 2; ++i)
    if (st->child[i]) { st->child[i]->owner = nullptr; invalidate_configs(st->child[i]); }
  delete st;
  c->prod = nullptr;
}

// the factors' logits / signs of the chains for parameter set `which`
int prod_ensure_cache(vmc_ctx* c, int which) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  if (c->ps[which].cache_valid) return VMC_OK;
  PROPAGATE(prod_sync_children(c));
  for (int i = 0; i < 2; ++i) {
    vmc_ctx* ch = st->child[i];
    CHILD(c, ch, ensure_cache(ch, which));
    HIPCHK(c, hipMemcpyAsync(st->l[which][i], ch->ps[which].logit, c->B * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (ch->sgn)
      HIPCHK(c, hipMemcpyAsync(st->s[which][i], ch->ps[which].sign, c->B * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  c->ps[which].cache_valid = true;
  return VMC_OK;
}

// E_loc of psi_a psi_b on the chains: both factors see the same chains and bonds, so their row lists are identical row
// for row; the off-diagonal row term is the product of their ratios times the coupling, taken once; the diagonal once
int prod_local_energy(vmc_ctx* c, int which) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  if (c->n_bonds <= 0) return fail(c, VMC_ERR_STATE, "bonds not set (vmc_set_bonds)");
  PROPAGATE(prod_ensure_cache(c, which));
  PROPAGATE(prod_sync_children(c));
  vmc_ctx *a = st->child[0], *b = st->child[1];
  CHILD(c, a, local_energy_device(a, which));
  CHILD(c, b, local_energy_device(b, which));
  const long long max_rows = (long long)c->B * c->n_bonds;
  {
    Timer t(c, "eloc_reduce");
    HIPCHK(c, launch_prod_row_combine(c->stream, a->val, b->val, a->off, c->B, max_rows, a->rowinfo, c->half_jx, c->val));
    HIPCHK(c, launch_eloc_reduce(c->stream, a->off, a->diag, c->val, c->B, c->offdiag, c->ps[which].eloc));
  }
  // (vmc_local_energy / _terms / vmc_evaluate read the row count and the diagonal term off the product ctx)
  HIPCHK(c, hipMemcpyAsync(c->off, a->off, (size_t)(c->B + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->diag, a->diag, (size_t)c->B * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return VMC_OK;
}

// n_steps x mc_step (graph_builders.py:38-89): per step the candidates (written straight into the factors' `configs`), a
// full forward of both factors on them -- the route vmc_amplitude takes, so the cached logits of the final chains are
// vmc_amplitude's bit for bit --, and one accept kernel that also draws the next proposal
int prod_run_sweep(vmc_ctx* c, const SweepCall& call) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  const int B = c->B, N = c->N;
  const long long n_steps = call.n_steps;
  const bool injected = call.injected;
  PROPAGATE(prod_ensure_cache(c, VMC_PSI));
  PROPAGATE(zero_accepted(c, call, c->stream));
  if (n_steps <= 0) return VMC_OK;
  vmc_ctx *a = st->child[0], *b = st->child[1];
  Timer t(c, "sweep");
  HIPCHK(c, hipMemsetAsync(st->acc_cnt, 0, (size_t)B * sizeof(unsigned), c->stream));
  HIPCHK(c, launch_proposals(c, c->stream, call.step0, injected, st->iup, st->idn, st->u));
  for (long long s = 0; s < n_steps; ++s) {
    HIPCHK(c, launch_prod_candidates(c->stream, c->configs, st->iup, st->idn, B, N, a->configs, b->configs));
    st->on_chains = false;
    invalidate_configs(a); invalidate_configs(b);
    CHILD(c, a, ensure_cache(a, VMC_PSI));
    CHILD(c, b, ensure_cache(b, VMC_PSI));
    ProdAcceptArgs x;
    memset((void*)&x, 0, sizeof(x));
    x.configs = c->configs; x.B = B; x.N = N;
    x.iup = st->iup; x.idn = st->idn; x.u = st->u;
    x.la = st->l[0][0]; x.sa = st->s[0][0]; x.lb = st->l[0][1]; x.sb = st->s[0][1];
    x.ca_l = a->ps[0].logit; x.ca_s = a->sgn ? a->ps[0].sign : nullptr;
    x.cb_l = b->ps[0].logit; x.cb_s = b->sgn ? b->ps[0].sign : nullptr;
    x.acc_mask = injected ? c->acc_mask : nullptr;      // (k_prod_accept never sees the injected proposals: only the mask)
    x.acc_cnt = st->acc_cnt;
    x.draw_next = (!injected && s + 1 < n_steps) ? 1 : 0;
    x.next_step = call.step0 + (unsigned long long)s + 1;
    set_key(c, x);
    HIPCHK(c, launch_prod_accept(c->stream, x));
  }
  // (also when !count_accepted: vmc_evaluate zeroes d_accepted once and lets the sweeps of all its samples add to it)
  HIPCHK(c, launch_prod_count_fold(c->stream, st->acc_cnt, B, c->d_accepted));
  return chains_moved(c, call);
}

// TrainOps.accumulate_gradients of the product: its E_loc (EnergyGradient) or its signed ITSWO ratio is the weight vector
// each factor's gradient path receives; factor i adds sum O and sum w O into its segment of [g1_a g1_b | g2_a g2_b | 8]
int prod_accumulate(vmc_ctx* c, int mode, float beta) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  vmc_ctx *a = st->child[0], *b = st->child[1];
  const float* w = nullptr;
  const float* e = nullptr;
  if (mode == VMC_MODE_ENERGY_GRADIENT) {
    PROPAGATE(prod_local_energy(c, VMC_PSI));
    w = e = c->ps[0].eloc;
  } else {
    if (!a->ps[1].has_params || !b->ps[1].has_params)
      return fail(c, VMC_ERR_STATE, "supervisor parameters not set (vmc_transfer_params)");
    PROPAGATE(prod_local_energy(c, VMC_OMEGA));
    PROPAGATE(prod_ensure_cache(c, VMC_PSI));
    HIPCHK(c, launch_prod_itswo_ratio(c->stream, st->l[0][0], st->s[0][0], st->l[0][1], st->s[0][1], st->l[1][0], st->s[1][0],
                                      st->l[1][1], st->s[1][1], c->ps[1].eloc, a->ps[0].shift - a->ps[1].shift,
                                      b->ps[0].shift - b->ps[1].shift, beta, c->B, c->ratio));
    w = c->ratio; e = c->ps[1].eloc;
  }
  PROPAGATE(prod_sync_children(c));
  PROPAGATE(acc_zeros(c));           // (a pending reset becomes real zeros: the factors add into their segments)
  {
    Timer t(c, "grad");
    long long off = 0;
    for (int i = 0; i < 2; ++i) {
      vmc_ctx* ch = st->child[i];
      CHILD(c, ch, ensure_cache(ch, VMC_PSI));
      CHILD(c, ch, child_gradient_sums(ch, w, c->acc + off, c->acc + c->P + off));
      off += st->P[i];
    }
    HIPCHK(c, launch_scalar_accum(c->stream, e, mode == 1 ? c->ratio : nullptr, c->B, c->acc + 2 * c->P, mode, false));
  }
  c->acc_fresh = false;
  c->acc_since_sweep = true;
  c->token = false;
  return VMC_OK;
}

int prod_set_bonds(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z) {
  PROPAGATE(prod_alive(c));
  for (int i = 0; i < 2; ++i) CHILD(c, c->prod->child[i], vmc_set_bonds(c->prod->child[i], n_bonds, ij, j_x, j_z));
  return VMC_OK;
}

int prod_gather_params(vmc_ctx* c, int which) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  long long off = 0;
  bool has = true;
  for (int i = 0; i < 2; ++i) {
    const ParamSet& p = st->child[i]->ps[which];
    has = has && p.has_params;
    if (p.has_params)
      HIPCHK(c, hipMemcpyAsync(c->ps[which].theta + off, p.theta, st->P[i] * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    off += st->P[i];
  }
  c->ps[which].has_params = has;
  return VMC_OK;
}

int prod_scatter_params(vmc_ctx* c, int which) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  long long off = 0;
  for (int i = 0; i < 2; ++i) {
    vmc_ctx* ch = st->child[i];
    ParamSet& p = ch->ps[which];
    HIPCHK(c, hipMemcpyAsync(p.theta, c->ps[which].theta + off, st->P[i] * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    p.has_params = true;
    p.packed_valid = p.cache_valid = false;
    if (which == VMC_PSI) ch->acts_valid = false;
    off += st->P[i];
  }
  c->ps[which].has_params = true;
  c->ps[which].cache_valid = false;
  return VMC_OK;
}

int prod_transfer_params(vmc_ctx* c) {
  PROPAGATE(prod_alive(c));
  for (int i = 0; i < 2; ++i) CHILD(c, c->prod->child[i], vmc_transfer_params(c->prod->child[i]));
  c->ps[1].cache_valid = false;
  return VMC_OK;
}

// Wavefunction.__call__ of the product: logit = (logit_a - shift_a) + (logit_b - shift_b), psi = sign_a sign_b exp(logit);
// a zero or singular factor gives psi = 0 (logit = -inf), never NaN.  Host rows go through the factors in blocks of
// batch_size rows by the route the sampler's candidates take (a short last block repeats its first row).
int prod_amplitude(vmc_ctx* c, int which, const float* configs, int64_t n_rows, float* logit, float* psi) {
  ProdState* st = c->prod;
  PROPAGATE(prod_alive(c));
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  if (n_rows < 0) return fail(c, VMC_ERR_INVALID, "n_rows < 0");
  const int B = c->B, N = c->N;
  const float sha = st->child[0]->ps[which].shift, shb = st->child[1]->ps[which].shift;
  std::vector<float> h[4];
  for (auto& v : h) v.resize((size_t)B);
  auto finish = [&](int64_t row0, int n) {
    for (int i = 0; i < n; ++i) {
      const float sa = h[1][i], sb = h[3][i];
      const float sg = (sa > 0.f ? 1.f : sa < 0.f ? -1.f : 0.f) * (sb > 0.f ? 1.f : sb < 0.f ? -1.f : 0.f);
      const float lg = sg == 0.f ? -INFINITY : (h[0][i] - sha) + (h[2][i] - shb);
      if (logit) logit[row0 + i] = lg;
      if (psi) psi[row0 + i] = sg == 0.f ? 0.f : sg * expf(lg);
    }
  };
  auto fetch = [&](const float* la, const float* sa, const float* lb, const float* sb) -> int {
    const float* src[4] = {la, sa, lb, sb};
    for (int k = 0; k < 4; ++k) {
      if (src[k]) HIPCHK(c, hipMemcpyAsync(h[k].data(), src[k], (size_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      else std::fill(h[k].begin(), h[k].end(), 1.f);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VMC_OK;
  };
  if (!configs) {
    if (n_rows != B) return fail(c, VMC_ERR_INVALID, "n_rows must equal batch_size when configs == NULL");
    PROPAGATE(prod_ensure_cache(c, which));
    PROPAGATE(fetch(st->l[which][0], st->s[which][0], st->l[which][1], st->s[which][1]));
    finish(0, B);
    return VMC_OK;
  }
  PROPAGATE(check_sz0_rows(c, configs, n_rows));
  vmc_ctx *a = st->child[0], *b = st->child[1];
  std::vector<float> blk((size_t)B * N);
  for (int64_t row0 = 0; row0 < n_rows; row0 += B) {
    const int n = (int)(n_rows - row0 < B ? n_rows - row0 : B);
    for (int r = 0; r < B; ++r)
      memcpy(blk.data() + (size_t)r * N, configs + (size_t)(row0 + (r < n ? r : 0)) * N, (size_t)N * sizeof(float));
    for (float v : blk) if (v != 1.f && v != -1.f) return fail(c, VMC_ERR_INVALID, "configs must be +-1");
    for (vmc_ctx* ch : {a, b}) {
      HIPCHK(c, hipMemcpyAsync(ch->configs, blk.data(), blk.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
      invalidate_configs(ch);
    }
    st->on_chains = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));       // (blk is reused by the next block)
    CHILD(c, a, ensure_cache(a, which));
    CHILD(c, b, ensure_cache(b, which));
    PROPAGATE(fetch(a->ps[which].logit, a->sgn ? a->ps[which].sign : nullptr, b->ps[which].logit,
                    b->sgn ? b->ps[which].sign : nullptr));
    finish(row0, n);
  }
  return VMC_OK;
}

}  // namespace vmcapi

extern "C" {

int vmc_create_product(vmc_ctx* a, vmc_ctx* b, vmc_ctx** out) {
  if (!a || !b || !out) return fail(nullptr, VMC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (a == b) return fail(nullptr, VMC_ERR_INVALID, "prod: the two factors must be two ctxs");
  for (vmc_ctx* ch : {a, b}) {
    if (ch->symz) return fail(nullptr, VMC_ERR_UNSUPPORTED, "prod: a symmetrized ctx ('symmetrized') cannot be a factor of a product");
    char msg[256];
    const int rc = plan_prod_child_check(ch->d.ansatz, ch->oact, ch->prod != nullptr, msg, sizeof(msg));
    if (rc != VMC_OK) return fail(nullptr, rc, msg);
    if (ch->owner) return fail(nullptr, VMC_ERR_STATE, "prod: a factor already belongs to a product ctx");
    if (ch->fs.n_terms > 0)
      return fail(nullptr, VMC_ERR_UNSUPPORTED, "vmc_create_product: a factor holds four-spin terms (vmc_set_four_spin_terms); a product ctx has none -- remove them first (n_terms = 0)");
  }
  if (a->N != b->N || a->B != b->B || a->d.device != b->d.device || a->d.chain_offset != b->d.chain_offset ||
      a->stream != b->stream)
    return fail(nullptr, VMC_ERR_INVALID, "prod: the factors must agree in n_sites, batch_size, device, chain_offset and stream");
  // the product's own ctx: chains, bond tables, accumulators, scratch -- a minimal dense shape whose network stays unused
  vmc_desc d;
  memset(&d, 0, sizeof(d));
  d.n_sites = a->N; d.batch_size = a->B; d.num_layers = 1; d.layer_size = 1;
  d.nonlinearity = VMC_ACT_RELU; d.output_activation = VMC_ACT_EXP;
  d.device = a->d.device; d.chain_offset = a->d.chain_offset; d.ansatz = VMC_ANSATZ_FULLY_CONNECTED;
  d.seed = a->d.seed; d.stream = a->d.stream;
  vmc_ctx* c = nullptr;
  PROPAGATE(vmc_create(&d, &c));
  DeviceGuard device_guard_(c->d.device);
  c->d.ansatz = VMC_ANSATZ_PRODUCT;
  c->path = PATH_PRODUCT;
  c->overlap = false;
  c->sweep8_ok = false; c->sweep_tile = 16;
  c->sgn = a->sgn || b->sgn;                  // Sz = 0 rows only, as for the signed factor alone (check_sz0_rows)
  c->ps[0].shift = c->ps[1].shift = 0.f;
  ProdState* st = new ProdState();
  c->prod = st;
  st->child[0] = a; st->child[1] = b;
  st->P[0] = a->P; st->P[1] = b->P;
  const long long P = a->P + b->P, B = c->B;
#define CP(expr) do { hipError_t e2 = (expr); if (e2 != hipSuccess) { \
    g_create_error = std::string(#expr) + ": " + hipGetErrorString(e2); vmc_destroy(c); return VMC_ERR_HIP; } } while (0)
#define NEW(buf, n) do { if ((buf).alloc(c, (n), #buf) != VMC_OK) { g_create_error = c->err; vmc_destroy(c); return VMC_ERR_HIP; } } while (0)
  // everything sized by P, allocated anew (alloc frees what vmc_create put there): theta of both sets, accumulators,
  // Adam moments, the gradient scratch
  c->P = P;
  NEW(c->ps[0].theta, P); NEW(c->ps[1].theta, P);
  NEW(c->acc, plan_prod_acc_floats(a->P, b->P)); NEW(c->adam_m, P); NEW(c->adam_v, P);
  NEW(c->grad_tmp, P);
  CP(hipMemsetAsync(c->acc, 0, (size_t)plan_prod_acc_floats(a->P, b->P) * sizeof(float), c->stream));
  CP(hipMemsetAsync(c->adam_m, 0, P * sizeof(float), c->stream));
  CP(hipMemsetAsync(c->adam_v, 0, P * sizeof(float), c->stream));
  for (int w = 0; w < 2; ++w)
    for (int i = 0; i < 2; ++i) {
      NEW(st->l[w][i], B); NEW(st->s[w][i], B);
      CP(hipMemsetAsync(st->l[w][i], 0, B * sizeof(float), c->stream));
      CP(launch_fill(c->stream, st->s[w][i], 1.f, B));          // (a factor without a sign never writes it)
    }
  NEW(st->iup, B); NEW(st->idn, B); NEW(st->u, B); NEW(st->acc_cnt, B);
  CP(hipMemsetAsync(st->acc_cnt, 0, B * sizeof(unsigned), c->stream));
  CP(hipStreamSynchronize(c->stream));
#undef NEW
#undef CP
  a->owner = c; b->owner = c;
  *out = c;
  return VMC_OK;
}

}  // extern "C"
