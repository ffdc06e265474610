// Host side of libcgsvmc_hip.so: the C ABI of include/cgsvmc.h on top of the gfx950 kernels.  One vmc_ctx per GPU, all
// work on ctx->stream.  This file: ctx life cycle, parameters, chains, amplitudes, local energies, timing; the other
// entry points live in vmc_api_sweep.hip (samplers), vmc_api_train.hip (accumulators, Adam, epochs, evaluation),
// vmc_api_coll.hip (collectives), vmc_api_sr.hip (stochastic reconfiguration), vmc_api_measure.hip (the measurements
// beside the energy: spin correlations, Renyi-2 entropy, dimer-dimer correlations, symmetry expectation values,
// symmetry-projected energies, Lanczos-step energies, the overlap with the frozen set), vmc_api_prod.hip (product ctxs);
// vmc_api_cgen.hip is the general convolution path's machinery.  Shared state and helpers: vmc_ctx.hpp.
#include "vmc_ctx.hpp"

using namespace vmcapi;

namespace vmcapi { std::string g_create_error; }

namespace vmcapi {

int late_inputs_set(vmc_ctx* c) {
  if (c->cg.graph && !c->gnn_adj) return fail(c, VMC_ERR_INVALID, "gnn: no adjacency list (vmc_set_adjacency)");
  if (c->path == PATH_EDVEC && !c->ed_top) return fail(c, VMC_ERR_INVALID, "ed_vector: no Lin tables (vmc_set_lin_tables)");
  return VMC_OK;
}

int ensure_packed(vmc_ctx* c, int which) {
  PROPAGATE(late_inputs_set(c));
  ParamSet& p = c->ps[which];
  if (!p.has_params) return fail(c, VMC_ERR_STATE, "parameters not set (vmc_set_params)");
  if (p.packed_valid) return VMC_OK;
  switch (c->path) {
    case PATH_PBDG: case PATH_EDVEC:      // (the kernels read theta as it lies)
    case PATH_CONV_GENERAL:               // (the parameter slices are the B matrices of its GEMMs as they lie in theta)
      break;
    case PATH_CONV:
      HIPCHK(c, launch_conv_pack(c->stream, p.theta, c->cg, p.cw0, p.cwf, p.cwb, p.cbias));
      break;
    case PATH_FUSED: case PATH_FUSED_LDS: case PATH_DENSE_GENERAL: case PATH_SPLIT_ROWS: case PATH_SPLIT_SWEEP: case PATH_NNB:
      HIPCHK(c, launch_pack(c->stream, p.theta, c->N, c->H, c->Hp, c->lay, p.w1p, p.b1p, p.bh, p.p16,
                            p.p16t, p.woutp, p.bout, p.won));
      if (path_split(c->path)) HIPCHK(c, launch_pack_split(c->stream, p.theta, c->H, c->lay, p.p16s));
      p.bdiff_valid = false;      // (differences of the image just replaced)
      break;
    case PATH_PRODUCT: return product_has_none(c, "parameter image");
    case PATH_SYMMETRIZED: return symmetrized_has_none(c, "parameter image");
  }
  p.packed_valid = true;
  return VMC_OK;
}

// The bond-difference table of parameter set `which` for the bond list `bonds` the row launch is about to read
// (the Hamiltonian's, a spin-correlation pass's, or the dummy bond before vmc_set_bonds): built on `stream` in front
// of the first row launch after a re-pack or a change of the list, constant until the next one.
static hipError_t ensure_bond_diff(vmc_ctx* c, int which, const int2* bonds) {
  ParamSet& p = c->ps[which];
  if (p.bdiff_valid && p.bdiff_epoch == c->bonds_epoch) return hipSuccess;
  const int nb = c->bonds ? c->n_bonds : 1;
  if (nb > p.bdiff_cap) {      // both or neither: the table counts as allocated only once bdiff_on is there
    p.bdiff_cap = 0;
    if (p.bdiff.alloc(c, (long long)nb * c->Hp, "bdiff") != VMC_OK || p.bdiff_on.alloc(c, nb, "bdiff_on") != VMC_OK)
      return hipErrorOutOfMemory;
    p.bdiff_cap = nb;
  }
  hipError_t e = launch_bond_diff(c->stream, p.w1p, c->rbm ? p.won : nullptr, bonds, nb, c->Hp, p.bdiff, p.bdiff_on);
  if (e != hipSuccess) return e;
  p.bdiff_valid = true; p.bdiff_epoch = c->bonds_epoch;
  return hipSuccess;
}

// rows through the fused row kernel of this ctx (the 3 x bf16 split experiment when it is switched on)
hipError_t launch_rows(vmc_ctx* c, int which, const TailArgs& a, bool ratio) {
  if (path_split(c->path)) return launch_tail16_split(c->stream, a, c->ps[which].p16s, ratio);
  if (a.n_hidden == 0) return launch_tail(c->stream, a, c->Hp, ratio, c->rbm);     // k_tail0 reads w1p itself
  TailArgs t = a;
  hipError_t e = ensure_bond_diff(c, which, a.bonds);
  if (e != hipSuccess) return e;
  t.bdiff = c->ps[which].bdiff; t.bdiff_on = c->ps[which].bdiff_on;
  return launch_tail(c->stream, t, c->Hp, ratio, c->rbm);
}

TailArgs tail_args(vmc_ctx* c, int which) {
  TailArgs a;
  memset(&a, 0, sizeof(a));
  a.pp = c->ps[which].packed();
  a.bonds = c->bonds ? c->bonds : c->bond_dummy;   // the kernel loads bonds[0] unconditionally
  a.half_jx = c->half_jx;
  a.n_hidden = c->n_hh;
  a.n_sites = c->N;
  a.n_units = c->H;
  a.on_base = c->ps[which].onsite;
  a.num_cus = c->num_cus;
  a.act = c->hact; a.oact = c->oact;
  return a;
}

ConvParams conv_params(const ParamSet& p) { return ConvParams{p.cw0, p.cwf, p.cwb, p.cbias}; }

// Conv2DNetwork / ResNet2D forward (wavefunctions.py:596-598, 790-792) of parameter set `which` on
// the rows of a row list over `configs`: logits (ratio == false) or 0.5 jx psi'/psi of the
// bond-exchanged configurations.  with_tape: the inputs of every convolution go to c->ctape.
// The same on the general path (conv_general.hip): blocks of cg_rows row configurations; per convolution an im2col
// gather (explicit, or inside the product's A operand; what the maps hold: cgen_post below) and one
// GEMM against the parameter slice in theta; ResBlock2d's `v + h` (layers.py:227) is the accumulate epilogue.
// iup / idn != nullptr: row r is chain r with that pair exchanged (the sampler's candidates).
int conv_rows(vmc_ctx* c, int which, const float* configs, const int2* rowinfo, int rows,
              const int* rows_dev, bool ratio, float* out, bool with_tape) {
  if (c->path == PATH_CONV_GENERAL) {
    // (the gradient path of the general convolution re-runs its own taped forward, cgen_gradient: the row entry keeps none)
    if (with_tape) return fail(c, VMC_ERR_UNSUPPORTED, "conv_rows keeps no tape on the general convolution path (its gradient entries run their own taped forward)");
    int n_rows = rows;
    if (rows_dev) {            // the blocks need the row count on the host
      HIPCHK(c, hipMemcpyAsync(&n_rows, rows_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return cgen_forward(c, which, configs, rowinfo, n_rows, nullptr, nullptr, ratio, out);
  }
  ConvRowsArgs a;
  memset(&a, 0, sizeof(a));
  a.g = c->cg; a.p = conv_params(c->ps[which]);
  a.configs = configs; a.rowinfo = rowinfo;
  a.bonds = c->bonds ? c->bonds : c->bond_dummy; a.half_jx = c->half_jx;
  a.logit_base = c->ps[which].logit;
  a.n_rows_dev = rows_dev; a.n_rows = rows; a.ratio = ratio ? 1 : 0; a.oact = c->oact;
  a.G = c->cG; a.out = out;
  a.tape = with_tape ? c->ctape : nullptr; a.tape_stride = c->ctape_stride;
  HIPCHK(c, launch_conv_rows(c->stream, a, c->num_cus));
  return VMC_OK;
}

// First layer of raw configurations on the matrix cores: z1[rows,Hp] = X[rows,N] W1p[N,Hp] + b1
// through the LDS-tiled fp32-MFMA GEMM (64x64x32 tiles of spins and weights staged in LDS,
// dwordx4 loads of the configuration batch).  wavefunctions.py:345-349, first snt.Linear.
int first_layer(vmc_ctx* c, const ParamSet& p, const float* configs, float* z1, int rows) {
  GemmArgs g; memset(&g, 0, sizeof(g));
  g.A = configs; g.sam = c->N; g.sak = 1;
  g.B = p.w1p; g.sbk = c->Hp; g.sbn = 1;
  g.M = rows; g.N = c->Hp; g.K = c->N; g.C = z1; g.ldc = c->Hp;
  g.bias = p.b1p; g.epilogue = 4; g.splitk = 1;
  HIPCHK(c, launch_gemm(c->stream, g));
  return VMC_OK;
}

// activation behind linear stage l (0 = the N x H layer) on the general path
int wide_stage_act(const vmc_ctx* c, int l) {
  return (c->rbm && l == c->n_hh) ? VMC_ACT_LOGCOSH_ : c->hact;
}

// Hidden layer l of the dense trunk as a GEMM: the weights [H][H] and biases of theta, row buffers of pitch Hp
GemmArgs trunk_gemm(const vmc_ctx* c, const ParamSet& p, int l, const float* A, int rows, float* C, int act) {
  GemmArgs g; memset(&g, 0, sizeof(g));
  g.A = A; g.sam = c->Hp; g.sak = 1;
  g.B = p.theta + off_w(c, l); g.sbk = c->H; g.sbn = 1;
  g.M = rows; g.N = c->H; g.K = c->H; g.C = C; g.ldc = c->Hp;
  g.bias = p.theta + off_b(c, l); g.epilogue = 1; g.splitk = 1; g.act = act;
  return g;
}

// nnb's pairing layer: out[rows][N^2] = a_L W_out + b_out
GemmArgs nnb_pairing_gemm(const vmc_ctx* c, const ParamSet& p, const float* A, int rows, float* C) {
  const long long NN = (long long)c->N * c->N;
  GemmArgs g; memset(&g, 0, sizeof(g));
  g.A = A; g.sam = c->Hp; g.sak = 1;
  g.B = p.theta + off_wout(c); g.sbk = NN; g.sbn = 1;
  g.M = rows; g.N = (int)NN; g.K = c->H; g.C = C; g.ldc = NN;
  g.bias = p.theta + off_bout(c); g.epilogue = 4; g.splitk = 1;
  return g;
}

// The last H x H layer of a forward whose activations nobody reads: turn its GEMM into the row-dot form (the output
// layer's dot product as column-tile partials in c->wide_dot, nothing stored to C) where a tile kernel takes the
// shape.  CGS_VMC_ROWDOT=0: never (A/B measurements, tests).  Returns whether `g` was changed.
bool wide_rowdot(vmc_ctx* c, const ParamSet& p, GemmArgs& g) {
  const char* e = getenv("CGS_VMC_ROWDOT");
  if (e && atoi(e) == 0) return false;
  GemmArgs t = g;
  t.epilogue = 10; t.dot_w = p.woutp; t.dot_out = c->wide_dot; t.C = nullptr;
  if (!gemm_rowdot_ok(t)) return false;
  g = t;
  return true;
}

// fc_layer_size > 256: rows {chain, bond} of a row list over the cached z1 -> logits / ratios,
// `wrows` rows at a time: rank-2 first layer written out, H x H layers as GEMMs, output dot
// RBM (wavefunctions.py:418-437): the last linear stage goes through log cosh instead of the hidden
// activation, the output "dot" is against ones (+ b_on) and `onsite` holds x . w_on of the base rows
int wide_forward(vmc_ctx* c, int which, const float* z1, const int2* rowinfo, long long n_rows, bool ratio,
                 float* out, const float* onsite) {
  ParamSet& p = c->ps[which];
  const int H = c->H, Hp = c->Hp, NH = c->n_hh;
  const int2* bonds = c->bonds ? c->bonds : c->bond_dummy;
  const WideOnsite on{c->rbm ? onsite : nullptr, p.won, bonds, nullptr, nullptr};
  if (c->path == PATH_FUSED_LDS) {
    TailArgs a = tail_args(c, which);
    a.z1 = z1; a.logit_base = p.logit; a.rowinfo = rowinfo; a.on_base = onsite;
    a.n_rows = (int)n_rows; a.out = out;
    if (NH == 0) HIPCHK(c, launch_tail(c->stream, a, Hp, ratio, c->rbm));      // k_tail0 takes any Hp
    else HIPCHK(c, launch_tail_lds(c->stream, a, Hp, ratio, c->rbm));
    return VMC_OK;
  }
  for (long long row0 = 0; row0 < n_rows; row0 += c->wrows) {
    const int rows = (int)(n_rows - row0 < c->wrows ? n_rows - row0 : c->wrows);
    HIPCHK(c, launch_wide_rows_act(c->stream, z1, p.w1p, rowinfo, bonds, row0, rows,
                                   Hp, wide_stage_act(c, 0), c->wbuf[0]));
    bool dot_fused = false;          // the output dot rode in the last layer's GEMM (row-dot epilogue)
    for (int l = 1; l <= NH; ++l) {
      GemmArgs g = trunk_gemm(c, p, l, c->wbuf[(l - 1) & 1], rows, c->wbuf[l & 1], wide_stage_act(c, l));
      if (l == NH) dot_fused = wide_rowdot(c, p, g);
      HIPCHK(c, launch_gemm(c->stream, g));
    }
    if (dot_fused)
      HIPCHK(c, launch_wide_out_part(c->stream, c->wide_dot, gemm_rowdot_tiles(H), p.bout, rows, rowinfo, row0,
                                     c->half_jx, p.logit, c->oact, ratio, out, on));
    else
    HIPCHK(c, launch_wide_out(c->stream, c->wbuf[NH & 1], p.woutp, p.bout, rows, H, Hp, rowinfo, row0, c->half_jx,
                              p.logit, c->oact, ratio, out, on));
  }
  return VMC_OK;
}

int nnb_forward(vmc_ctx* c, int which, const float* z1, const float* configs, const int2* rowinfo, long long n_rows,
                bool ratio, float* out, float* out_sign) {
  ParamSet& p = c->ps[which];
  const int Hp = c->Hp, NH = c->n_hh;
  const long long NN = (long long)c->N * c->N;
  const int2* bonds = c->bonds ? c->bonds : c->bond_dummy;
  for (long long row0 = 0; row0 < n_rows; row0 += c->nnb_rows) {
    const int rows = (int)(n_rows - row0 < c->nnb_rows ? n_rows - row0 : c->nnb_rows);
    HIPCHK(c, launch_wide_rows_act(c->stream, z1, p.w1p, rowinfo, bonds, row0, rows, Hp, VMC_ACT_RELU_, c->wbuf[0]));
    for (int l = 1; l <= NH; ++l)
      HIPCHK(c, launch_gemm(c->stream, trunk_gemm(c, p, l, c->wbuf[(l - 1) & 1], rows, c->wbuf[l & 1], VMC_ACT_RELU_)));
    // the pairing layer of the block
    HIPCHK(c, launch_gemm(c->stream, nnb_pairing_gemm(c, p, c->wbuf[NH & 1], rows, c->nnb_out)));
    NnbRowsArgs a; memset((void*)&a, 0, sizeof(a));
    a.out = c->nnb_out; a.ldo = NN; a.N = c->N; a.configs = configs; a.rowinfo = rowinfo + row0; a.bonds = bonds;
    a.n_rows = rows;
    if (ratio) { a.half_jx = c->half_jx; a.logit_base = p.logit; a.sign_base = p.sign; a.val = out + row0; }
    else { a.logit = out + row0; a.sign = out_sign + row0; }
    HIPCHK(c, launch_nnb_rows(c->stream, a));
  }
  return VMC_OK;
}

// The full forward of parameter set `which` on n_rows rows of a device buffer of configurations, by the ctx's kernel
// family: log|psi| (the logit) per row into `logit` and, for the signed types, the sign (ed_vector: the entry itself) into
// `sign`.  z1 [n_rows][Hp], onsite [n_rows] and rowinfo (the identity list of n_rows rows) are the scratch of the dense
// trunk.  tape: the fused convolutions leave the inputs of every convolution in c->ctape.  timed: the regions of a cache
// refill, "z1" for the first layer and "tail_amp" for the rest (otherwise none: the caller times the call).
static int full_forward(vmc_ctx* c, int which, const float* configs, int n_rows, float* z1, float* onsite,
                        const int2* rowinfo, float* logit, float* sign, bool tape, bool timed) {
  ParamSet& p = c->ps[which];
  const char* tail_region = timed ? "tail_amp" : nullptr;
  auto trunk_first_layer = [&]() -> int {
    Timer t(c, timed ? "z1" : nullptr);
    PROPAGATE(first_layer(c, p, configs, z1, n_rows));
    if (c->rbm) HIPCHK(c, launch_onsite(c->stream, configs, p.won, n_rows, c->N, onsite));
    return VMC_OK;
  };
  switch (c->path) {
    case PATH_EDVEC: {
      Timer t(c, tail_region);
      HIPCHK(c, launch_edvec_rows(c->stream, p.theta, (int)c->P, c->ed_top, c->ed_bot, c->N, configs, n_rows, logit, sign));
      return VMC_OK;
    }
    case PATH_PBDG: {
      Timer t(c, tail_region);
      HIPCHK(c, launch_pbdg_rows(c->stream, p.theta, c->N, configs, n_rows, logit, sign, nullptr, nullptr));
      return VMC_OK;
    }
    case PATH_CONV: case PATH_CONV_GENERAL: {
      Timer t(c, tail_region);
      return conv_rows(c, which, configs, rowinfo, n_rows, nullptr, false, logit, tape);
    }
    case PATH_NNB: {
      PROPAGATE(trunk_first_layer());
      Timer t(c, tail_region);
      return nnb_forward(c, which, z1, configs, rowinfo, n_rows, false, logit, sign);
    }
    case PATH_FUSED_LDS: case PATH_DENSE_GENERAL: {
      PROPAGATE(trunk_first_layer());
      Timer t(c, tail_region);
      return wide_forward(c, which, z1, rowinfo, n_rows, false, logit, onsite);
    }
    case PATH_FUSED: case PATH_SPLIT_ROWS: case PATH_SPLIT_SWEEP: {
      PROPAGATE(trunk_first_layer());
      Timer t(c, tail_region);
      TailArgs a = tail_args(c, which);
      a.z1 = z1; a.on_base = onsite; a.n_rows = n_rows; a.out = logit; a.rowinfo = rowinfo;
      HIPCHK(c, launch_rows(c, which, a, false));
      return VMC_OK;
    }
    case PATH_PRODUCT: return product_has_none(c, "forward");
    case PATH_SYMMETRIZED: return symmetrized_has_none(c, "forward");
  }
  return VMC_OK;
}

// z1 / logit cache of parameter set `which` for the ctx's chains
int ensure_cache(vmc_ctx* c, int which) {
  PROPAGATE(ensure_packed(c, which));
  ParamSet& p = c->ps[which];
  if (p.cache_valid) return VMC_OK;
  const bool tape = which == VMC_PSI && c->path == PATH_CONV;       // (the general path keeps no gradient tape)
  PROPAGATE(full_forward(c, which, c->configs, c->B, p.z1, p.onsite, c->rowinfo_id, p.logit, p.sign, tape, true));
  if (tape) c->acts_valid = true;
  p.cache_valid = true;
  return VMC_OK;
}

void invalidate_configs(vmc_ctx* c) {
  c->acts_valid = false;
  c->ps[0].cache_valid = c->ps[1].cache_valid = false;
  c->list_valid = false;
  c->cnt_valid = false;
  if (c->prod) prod_chains_changed(c);
  if (c->symz) symz_chains_changed(c);
}

int ensure_list(vmc_ctx* c) {
  if (c->n_bonds <= 0) return fail(c, VMC_ERR_STATE, "bonds not set (vmc_set_bonds)");
  if (c->list_valid) return VMC_OK;
  Timer t(c, "bond_list");
  HIPCHK(c, launch_bond_list(c->stream, c->configs, c->bonds, c->quarter_jz, c->B, c->N,
                             c->n_bonds, c->cnt, c->off, c->diag, c->rowinfo, c->cnt_valid));
  c->list_valid = true;
  return VMC_OK;
}

// eloc[which] on device
// defer_reduce: the caller folds the rows into eloc itself (vmc_accumulate lets k_backprop16 do it: one
// dependent launch less per step); *deferred tells whether that is still owed
int local_energy_device(vmc_ctx* c, int which, bool defer_reduce, bool* deferred) {
  if (deferred) *deferred = false;
  if (c->prod) return prod_local_energy(c, which);
  if (c->symz) return symz_local_energy(c, which);
  PROPAGATE(ensure_cache(c, which));
  PROPAGATE(ensure_list(c));
  PROPAGATE(connected_rows_device(c, which, true));
  ParamSet& p = c->ps[which];
  if (c->fs.n_terms == 0 && defer_reduce && deferred && path_fused_dense(c->path)) {
    *deferred = true;              // the fused back-propagation launch folds val into eloc
    return VMC_OK;
  }
  {
    Timer t(c, "eloc_reduce");
    HIPCHK(c, launch_eloc_reduce(c->stream, c->off, c->diag, c->val, c->B, c->offdiag, p.eloc));
  }
  if (c->fs.n_terms > 0) PROPAGATE(four_spin_device(c, which));     // the four-spin terms on top, never deferred
  return VMC_OK;
}

// val[row] of every row of the list, by the ctx's kernel family (the spin-correlation passes run it over their own bond set)
int connected_rows_device(vmc_ctx* c, int which, bool share_cus) {
  ParamSet& p = c->ps[which];
  Timer t(c, "tail_eloc");
  switch (c->path) {
  case PATH_EDVEC:
    HIPCHK(c, launch_edvec_eloc(c->stream, p.theta, (int)c->P, c->ed_top, c->ed_bot, c->N, c->configs, p.sign, c->B, c->off,
                                c->rowinfo, c->bonds, c->half_jx, c->owner && c->owner->symz ? 1 : 0, c->val));
    break;
  case PATH_PBDG:      // (a fresh M^-1 per chain: never the sampler's incrementally updated one)
    HIPCHK(c, launch_pbdg_eloc(c->stream, p.theta, c->N, c->configs, c->B, c->off, c->rowinfo, c->bonds, c->half_jx,
                               c->val));
    break;
  case PATH_CONV: case PATH_CONV_GENERAL:
    PROPAGATE(conv_rows(c, which, c->configs, c->rowinfo, (int)((long long)c->B * c->n_bonds), c->off + c->B,
                        true, c->val, false));
    break;
  case PATH_DENSE_GENERAL: case PATH_NNB: {
    int n_rows = 0;      // the GEMM grids need the row count on the host
    HIPCHK(c, hipMemcpyAsync(&n_rows, c->off + c->B, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->path == PATH_NNB) PROPAGATE(nnb_forward(c, which, p.z1, c->configs, c->rowinfo, n_rows, true, c->val, nullptr));
    else PROPAGATE(wide_forward(c, which, p.z1, c->rowinfo, n_rows, true, c->val, p.onsite));
    break;
  }
  case PATH_FUSED: case PATH_FUSED_LDS: case PATH_SPLIT_ROWS: case PATH_SPLIT_SWEEP: {
    TailArgs a = tail_args(c, which);
    a.z1 = p.z1; a.logit_base = p.logit; a.rowinfo = c->rowinfo;
    a.n_rows_dev = c->off + c->B;                 // the row count stays on the device
    a.n_rows = (int)((long long)c->B * c->n_bonds);
    a.out = c->val;
    if (c->path == PATH_FUSED_LDS) {              // the LDS-operand kernel (without an H x H layer: k_tail0, any Hp)
      if (c->n_hh == 0) HIPCHK(c, launch_tail(c->stream, a, c->Hp, true, c->rbm));
      else HIPCHK(c, launch_tail_lds(c->stream, a, c->Hp, true, c->rbm));
      break;
    }
    // a sampler launch is expected to overtake this accumulate: its workgroups need a whole
    // CU each, so the persistent grid leaves them free
    if (share_cus && c->expect_sweep && can_overlap(c) && c->num_cus - sweep_cus(c) >= c->num_cus / 4) {
      a.num_cus = c->num_cus - sweep_cus(c);
      // Long row lists (config 5: 4,100 tiles of ~170 us) as SHORT-LIVED workgroups instead: a grid of
      // tiles / K workgroups of K tiles each (about CGS_VMC_TAIL_CHUNK_US of work), which the dispatcher hands to
      // whichever CU is free -- the CUs of the sampler too once it has finished (its launch, on the high-priority
      // sweep_stream, takes the CUs the first workgroups free).  A persistent grid on the CUs the sampler leaves
      // cannot grow when the sampler ends before it (eight-chain tiles: 3.6 ms against 5.1 ms on 128 CUs).
      static const int chunk_us = getenv("CGS_VMC_TAIL_CHUNK_US") ? atoi(getenv("CGS_VMC_TAIL_CHUNK_US")) : 150;
      if (chunk_us > 0 && !path_split(c->path) && c->n_hh > 0) {
        const long long tiles = ((long long)a.n_rows + 127) / 128;
        const double tile_us = 128.0 * c->n_hh * 2.0 * c->Hp * c->Hp / 491520.0;   // 0.8 of a CU's 256 flops per clock at 2.4 GHz
        long long k = (long long)(chunk_us / tile_us);
        if (k < 1) k = 1;
        const long long wgs = (tiles + k - 1) / k;
        if (wgs >= 4LL * c->num_cus) a.num_cus = (int)wgs;
      }
    }
    HIPCHK(c, launch_rows(c, which, a, true));
    break;
  }
  case PATH_PRODUCT: return product_has_none(c, "row kernel");
  case PATH_SYMMETRIZED: return symmetrized_has_none(c, "row kernel");
  }
  return VMC_OK;
}

int grow_tmp(vmc_ctx* c, long long rows) {
  if (rows <= c->tmp_rows) return VMC_OK;
  c->tmp_rows = 0;      // all six or none: a failure below leaves the group absent, the next call allocates it anew
  PROPAGATE(c->tmp_on.alloc(c, rows, "tmp_on"));
  PROPAGATE(c->tmp_sign.alloc(c, rows, "tmp_sign"));
  PROPAGATE(c->tmp_rowinfo.alloc(c, rows, "tmp_rowinfo"));
  HIPCHK(c, launch_iota_rows(c->stream, c->tmp_rowinfo, (int)rows));
  PROPAGATE(c->tmp_cfg.alloc(c, rows * c->N, "tmp_cfg"));
  PROPAGATE(c->tmp_z1.alloc(c, rows * c->Hp, "tmp_z1"));
  PROPAGATE(c->tmp_out.alloc(c, rows, "tmp_out"));
  c->tmp_rows = rows;
  return VMC_OK;
}

// The full forward of parameter set `which` on n_rows rows of a DEVICE buffer of configurations (vmc_amplitude's rows, the
// swapped rows of vmc_renyi2_swap): log|psi| (the logit) per row into `logit`, and for the signed types the sign (ed_vector:
// the entry itself) into `sign`.  The caller has run ensure_packed and grow_tmp(n_rows): tmp_z1 / tmp_on / tmp_rowinfo are
// the scratch; `configs`, `logit`, `sign` may be the tmp buffers of the same rows or any others.
int rows_forward_device(vmc_ctx* c, int which, const float* configs, long long n_rows, float* logit, float* sign) {
  if (n_rows <= 0) return VMC_OK;
  return full_forward(c, which, configs, (int)n_rows, c->tmp_z1, c->tmp_on, c->tmp_rowinfo, logit, sign, false, false);
}

// the name a signed ctx's refusals go by (Sz = 0 rows, stochastic reconfiguration)
const char* signed_family_name(KernelPath path) {
  switch (path) {
    case PATH_PRODUCT: return "prod (a signed factor)";
    case PATH_SYMMETRIZED: return "symmetrized (spin flips or a signed base)";
    case PATH_EDVEC: return "ed_vector";
    case PATH_NNB: return "fully_connected_nnb";
    case PATH_PBDG: return "pbdg";
    case PATH_FUSED: case PATH_FUSED_LDS: case PATH_DENSE_GENERAL: case PATH_CONV: case PATH_SPLIT_ROWS:
    case PATH_SPLIT_SWEEP: case PATH_CONV_GENERAL: break;      // (unsigned amplitudes: never asked)
  }
  return "unsigned";
}

// signed amplitudes (pbdg, nnb, ed_vector, a product with such a factor): every row must hold as many up as down spins
// (the determinants and the Lin tables live at Sz = 0); host rows
int check_sz0_rows(vmc_ctx* c, const float* configs, long long n_rows) {
  if (!c->sgn) return VMC_OK;
  for (long long r = 0; r < n_rows; ++r) {
    double m = 0.0;
    for (int i = 0; i < c->N; ++i) m += configs[r * c->N + i];
    if (m != 0.0) {
      char msg[160];
      snprintf(msg, sizeof(msg), "%s: configuration %lld has magnetisation %g; the ansatz needs as many up as down spins", signed_family_name(c->path), r, m);
      return fail(c, VMC_ERR_INVALID, msg);
    }
  }
  return VMC_OK;
}

// layers.NONLINEARITIES on the host (the psi values vmc_amplitude hands back)
float host_activation(int act, float x) {
  switch (act) {
    case VMC_ACT_RELU_: return x > 0.f ? x : 0.f;
    case VMC_ACT_EXP_: return expf(x);
    case VMC_ACT_COS_: return cosf(x);
    case VMC_ACT_TAN_: return tanf(x);
    case VMC_ACT_TANH_: return tanhf(x);
    case VMC_ACT_SIGMOID_: return 1.f / (1.f + expf(-x));
    default: return x;
  }
}

// ---- the device buffers of vmc_create: what every ctx has (the non-dense paths keep minimal dense-side shapes), then the
// groups of the ctx's path.  A failure names itself in g_create_error and returns VMC_ERR_HIP; vmc_create destroys the ctx.
#define CA(expr) do { hipError_t e2 = (expr); if (e2 != hipSuccess) { \
    g_create_error = std::string(#expr) + ": " + hipGetErrorString(e2); return VMC_ERR_HIP; } } while (0)
#define NEW(buf, n) do { if ((buf).alloc(c, (n), #buf) != VMC_OK) { g_create_error = c->err; return VMC_ERR_HIP; } } while (0)

// path_wide: the two activation row buffers of c->wrows rows, and the proposal buffers of a step-at-a-time sampler (the
// general dense sampler and nnb's; PATH_FUSED_LDS allocates them too and never reads them)
static int create_wide_rows(vmc_ctx* c) {
  const long long B = c->B, Hp = c->Hp;
  NEW(c->wbuf[0], c->wrows * Hp); NEW(c->wbuf[1], c->wrows * Hp);
  NEW(c->prop_u, B);
  NEW(c->wide_dot, (long long)gemm_rowdot_tiles(c->H) * c->wrows);
  NEW(c->prop_iup, B); NEW(c->prop_idn, B); NEW(c->wide_zero, Hp);
  CA(hipMemsetAsync(c->wide_zero, 0, Hp * sizeof(float), c->stream));
  return VMC_OK;
}

// PATH_NNB: blocks of rows whose dense pairing layer takes CGS_VMC_NNB_BLOCK_MB (default 256) MiB; they size the row buffers
static int create_nnb_blocks(vmc_ctx* c) {
  const long long B = c->B, N = c->N;
  long long mb = PLAN_NNB_BLOCK_MB_DEFAULT;
  if (const char* e = getenv("CGS_VMC_NNB_BLOCK_MB")) mb = atoll(e);
  c->nnb_rows = plan_nnb_block_rows((int)N, mb);
  if (const char* e = getenv("CGS_VMC_NNB_BLOCK_ROWS")) { const long long r = atoll(e); if (r >= 1 && r < c->nnb_rows) c->nnb_rows = r; }   // tests: several blocks at small shapes
  c->wrows = c->nnb_rows;
  NEW(c->nnb_out, c->nnb_rows * N * N);
  NEW(c->nnb_delta, B * N * N);
  NEW(c->nnb_cl, B); NEW(c->nnb_cs, B);
  return VMC_OK;
}

// signed amplitudes: the sign beside the logit of both parameter sets (alt: the set the next sampler launch writes)
static int create_sign(vmc_ctx* c, bool alt) {
  const long long B = c->B;
  for (int w = 0; w < 2; ++w) {
    NEW(c->ps[w].sign, B);
    CA(hipMemsetAsync(c->ps[w].sign, 0, B * sizeof(float), c->stream));
  }
  if (alt) {
    NEW(c->ps[0].sign_alt, B);
    CA(hipMemsetAsync(c->ps[0].sign_alt, 0, B * sizeof(float), c->stream));
  }
  return VMC_OK;
}

static int create_edvec(vmc_ctx* c) {
  const long long B = c->B;
  NEW(c->ed_keys, B); NEW(c->ed_keys_sorted, B);
  CA(edvec_sort_bytes((int)B, (int)c->P, &c->ed_sort_bytes));
  NEW(c->ed_sort_tmp, (long long)c->ed_sort_bytes);
  c->ed_tables_lds = plan_edvec_tables_in_lds(c->N) && !(getenv("CGS_VMC_EDVEC_TABLES_LDS") && atoi(getenv("CGS_VMC_EDVEC_TABLES_LDS")) == 0);
  if (c->ed_tables_lds) CA(edvec_sweep_reserve_lds(c->N));
  return VMC_OK;
}

static int create_pbdg(vmc_ctx* c) {
  const long long B = c->B, N = c->N, n = N / 2;
  NEW(c->pbdg_inv, B * n * n); NEW(c->pbdg_pos, B * N);
  c->pbdg_slices = plan_pbdg_grad_slices(c->P, B, c->num_cus);
  NEW(c->pbdg_ws, plan_pbdg_grad_ws_doubles(c->P, c->pbdg_slices));
  return VMC_OK;
}

static int create_conv_general(vmc_ctx* c) {
  const ConvGeom& cg = c->cg;
  const long long B = c->B;
  // blocks of at most ~768 MB of im2col rows (one row configuration at least), at least B rows when that fits
  const long long per_row = (long long)cg.N * plan_cgen_lda(cg) * (long long)sizeof(float);
  long long block_mb = 768;
  if (const char* e = getenv("CGS_VMC_CONV_GENERAL_BLOCK_MB")) { block_mb = atoll(e); if (block_mb < 1) block_mb = 1; if (block_mb > 16384) block_mb = 16384; }
  long long rows = (block_mb << 20) / per_row;
  if (rows < 1) rows = 1;
  if (rows > (1LL << 30) / cg.N) rows = (1LL << 30) / cg.N;          // rows * N: the M of a GEMM (int)
  if (rows > (B > 65536 ? B : 65536)) rows = B > 65536 ? B : 65536;  // (small shapes: no point in hundreds of MB of maps)
  // whole rounds of the chip for the 128-row tiles of a block's products (the local energies run many full blocks:
  // 5.09 rounds of 256 CUs are paid as 6)
  if (rows * cg.N / 128 >= 2LL * c->num_cus) {
    const long long rounds = rows * cg.N / (128LL * c->num_cus);
    rows = rounds * 128LL * c->num_cus / cg.N;
  }
  if (const char* e = getenv("CGS_VMC_CONV_GENERAL_BLOCK_ROWS")) { const long long r = atoll(e); if (r >= 1 && r < rows) rows = r; }   // tests: several blocks at small shapes
  c->cg_rows = rows;
  // (cg_A, the im2col matrix: allocated by the first launch that writes one -- cgen_need_A, vmc_api_cgen.hip)
  // the band kernel (conv_band.hip) needs no im2col matrix: an untaped forward on it runs blocks sized by the two
  // maps alone, up to 2 GB of them (36 x 36 x 16 filters: 370 rows per im2col block against 12,900 -- the local
  // energies' 58 k rows were 110 blocks of partly filled launches)
  long long rows_fwd = rows;
  if (plan_cgen_band_ok(cg)) {
    const long long per_row_maps = 2LL * cg.N * cgen_fp(cg) * (long long)sizeof(float);
    rows_fwd = (2048LL << 20) / per_row_maps;
    if (rows_fwd > (1LL << 30) / cg.N) rows_fwd = (1LL << 30) / cg.N;
    if (rows_fwd > 131072) rows_fwd = 131072;
    if (rows_fwd < rows) rows_fwd = rows;
    if (getenv("CGS_VMC_CONV_GENERAL_BLOCK_ROWS")) rows_fwd = rows;      // tests: several blocks at small shapes
  }
  c->cg_rows_fwd = rows_fwd;
  for (int i = 0; i < 2; ++i) NEW(c->cg_fm[i], rows_fwd * cg.N * cgen_fp(cg));
  NEW(c->cg_sum, rows_fwd); NEW(c->cg_zero, 1); NEW(c->cg_lnew, B);
  CA(hipMemsetAsync(c->cg_zero, 0, sizeof(float), c->stream));
  NEW(c->prop_u, B); NEW(c->prop_iup, B); NEW(c->prop_idn, B);
  return VMC_OK;
}

static int create_conv_fused(vmc_ctx* c) {
  const ConvGeom& cg = c->cg;
  const long long B = c->B;
  const long long nl = cg.n_conv > 1 ? cg.n_conv - 1 : 1;
  for (int w = 0; w < 2; ++w) {
    ParamSet& p = c->ps[w];
    NEW(p.cw0, plan_conv_w0_floats(cg)); NEW(p.cwf, plan_conv_wf_floats(cg));
    NEW(p.cwb, plan_conv_wf_floats(cg));
    NEW(p.cbias, plan_conv_bias_floats(cg));
  }
  const int nw = conv_waves(cg);
  c->cG = conv_pick_group(cg, nw);
  if (c->cG > B) c->cG = (int)B;
  c->cGs = conv_pick_sweep_group(cg, B, c->num_cus, nw);     // chains per sampler workgroup (plan.hpp)
  if (const char* e = getenv("CGS_VMC_CONV_SWEEP_G")) {     // measurement knob: chains per sampler workgroup
    const int G = atoi(e);
    if (G >= 1 && G <= 64 && conv_rows_lds(cg, G) <= conv_lds_cap(cg)) c->cGs = G < B ? G : (int)B;
  }
  c->ctape_stride = B * cg.CS; c->cdelta_stride = B * cg.CS;
  NEW(c->ctape, nl * c->ctape_stride); NEW(c->cdelta, (long long)cg.n_conv * c->cdelta_stride);
  c->c_slices = plan_conv_dw_slices(cg, B, c->num_cus);
  NEW(c->cws, plan_conv_dw_ws_floats(cg, c->c_slices));
  return VMC_OK;
}

static int create_buffers(vmc_ctx* c) {
  const long long B = c->B, N = c->N, Hp = c->Hp, P = c->P, L = c->A, NH = c->n_hh;   // L: activation buffers
  const bool nnb = c->path == PATH_NNB;
  for (int w = 0; w < 2; ++w) {
    ParamSet& p = c->ps[w];
    NEW(p.theta, P);
    NEW(p.w1p, N * Hp); NEW(p.b1p, Hp); NEW(p.bh, NH * Hp);
    NEW(p.p16, (NH > 0 ? NH : 1) * Hp * Hp);
    NEW(p.p16t, (NH > 0 ? NH : 1) * Hp * Hp);
    CA(hipMemsetAsync(p.p16t, 0, (size_t)(NH > 0 ? NH : 1) * Hp * Hp * sizeof(float), c->stream));
    CA(hipMemsetAsync(p.p16, 0, (size_t)(NH > 0 ? NH : 1) * Hp * Hp * sizeof(float), c->stream));
    NEW(p.won, N); NEW(p.onsite, B);
    CA(hipMemsetAsync(p.won, 0, N * sizeof(float), c->stream));
    CA(hipMemsetAsync(p.onsite, 0, B * sizeof(float), c->stream));
    NEW(p.woutp, Hp); NEW(p.bout, 1);
    if (path_split(c->path)) NEW(p.p16s, pack_split_dwords((int)NH));
    NEW(p.z1, B * Hp); NEW(p.logit, B); NEW(p.eloc, B);
    if (w == 0) {
      NEW(p.z1_alt, B * Hp); NEW(p.logit_alt, B); NEW(p.onsite_alt, B);
      CA(hipMemsetAsync(p.onsite_alt, 0, B * sizeof(float), c->stream));
    }
  }
  NEW(c->configs, B * N); NEW(c->configs_alt, B * N);
  CA(hipMemsetAsync(c->configs, 0, B * N * sizeof(float), c->stream));
  CA(hipMemsetAsync(c->configs_alt, 0, B * N * sizeof(float), c->stream));
  c->act.resize(L, nullptr);
  NEW(c->act_all, L * B * Hp); NEW(c->act_alt, L * B * Hp);
  CA(hipMemsetAsync(c->act_all, 0, L * B * Hp * sizeof(float), c->stream));
  CA(hipMemsetAsync(c->act_alt, 0, L * B * Hp * sizeof(float), c->stream));
  {  // the sampler's stream outranks `stream`: where both have workgroups waiting for a CU, the sampler's go first
    int least = 0, greatest = 0;
    CA(hipDeviceGetStreamPriorityRange(&least, &greatest));
    CA(hipStreamCreateWithPriority(&c->sweep_stream, hipStreamNonBlocking, greatest));
  }
  CA(hipEventCreateWithFlags(&c->ev_mark, hipEventDisableTiming));
  CA(hipEventCreateWithFlags(&c->ev_now, hipEventDisableTiming));
  CA(hipEventCreateWithFlags(&c->ev_sweep_done, hipEventDisableTiming));
  for (int l = 0; l < L; ++l) c->act[l] = c->act_all + l * B * Hp;
  c->delta.resize(L, nullptr);
  NEW(c->delta_all, L * B * Hp);
  CA(hipMemsetAsync(c->delta_all, 0, L * B * Hp * sizeof(float), c->stream));
  for (int l = 0; l < L; ++l) c->delta[l] = c->delta_all + l * B * Hp;
  for (int i = 0; i < 4; ++i) NEW(c->d_batch[i / 2][i % 2], (L + 1) * (long long)wgrad_problem_bytes());
  {  // weight-gradient launch: the tiles of all layers
    // fully_connected on the kernels that run k_backprop16: the N = 1 output layer leaves the MFMA tile grid
    // (CGS_VMC_WGRAD_OUT_TILES=1 keeps it there: A/B measurements)
    const char* e_out = getenv("CGS_VMC_WGRAD_OUT_TILES");
    c->wg_out_partials = !c->rbm && path_fused_dense(c->path) && !(e_out && atoi(e_out) == 1);
    c->wg_tiles = nnb ? plan_nnb_wgrad_total_tiles((int)N, c->H, (int)NH)
                      : plan_wgrad_total_tiles((int)N, c->H, (int)NH, c->rbm, !c->wg_out_partials);
    // (nnb: hundreds of tiles and more -- the workspace follows the planned slices, not the bound)
    if (nnb) c->nnb_wg_slices = plan_wgrad_slices(c->wg_tiles, B, c->num_cus, 1, 0);
    if (c->wg_out_partials) NEW(c->wg_outpart, ((B + 15) / 16) * 2 * (Hp + 4));
    NEW(c->wg_tickets, c->wg_tiles > 0 ? c->wg_tiles : 1);
    CA(hipMemsetAsync(c->wg_tickets, 0, (size_t)(c->wg_tiles > 0 ? c->wg_tiles : 1) * sizeof(int), c->stream));
  }
  NEW(c->ratio, B); NEW(c->ones, B); NEW(c->oscale, B);
  CA(launch_fill(c->stream, c->ones, 1.f, B));
  CA(launch_fill(c->stream, c->oscale, 1.f, B));
  if (c->hact == VMC_ACT_COS_) {
    NEW(c->dact_all, L * B * Hp); NEW(c->dact_alt, L * B * Hp);
    CA(hipMemsetAsync(c->dact_all, 0, L * B * Hp * sizeof(float), c->stream));
    CA(hipMemsetAsync(c->dact_alt, 0, L * B * Hp * sizeof(float), c->stream));
  }
  // (vmc_create_product allocates the members sized by P -- theta of both sets, acc, adam_m, adam_v, grad_tmp -- anew
  // at P_a + P_b: alloc frees what vmc_create put there)
  NEW(c->acc, 2 * P + 8); NEW(c->adam_m, P); NEW(c->adam_v, P);
  NEW(c->grad_tmp, P);
  CA(hipMemsetAsync(c->acc, 0, (2 * P + 8) * sizeof(float), c->stream));
  CA(hipMemsetAsync(c->adam_m, 0, P * sizeof(float), c->stream));
  CA(hipMemsetAsync(c->adam_v, 0, P * sizeof(float), c->stream));
  NEW(c->gemm_ws, plan_wgrad_ws_floats(c->wg_tiles, nnb ? c->nnb_wg_slices : WG_MAX_SPLIT));
  NEW(c->d_accepted, 1); NEW(c->d_sum, 1); NEW(c->d_max, 1);
  NEW(c->inj_up, B); NEW(c->inj_dn, B); NEW(c->inj_u, B);
  NEW(c->acc_mask, B);
  NEW(c->cnt, B); NEW(c->off, B + 1); NEW(c->diag, B);
  NEW(c->cnt_alt, B); NEW(c->diag_alt, B);
  NEW(c->rowinfo_id, B); CA(launch_iota_rows(c->stream, c->rowinfo_id, (int)B));
  NEW(c->bond_dummy, 1); CA(hipMemsetAsync(c->bond_dummy, 0, sizeof(int2), c->stream));
  NEW(c->offdiag, B);
  switch (c->path) {
    case PATH_FUSED: case PATH_SPLIT_ROWS: case PATH_SPLIT_SWEEP:
    case PATH_PRODUCT:      // (vmc_create_product starts from a minimal PATH_FUSED ctx and adds its own)
    case PATH_SYMMETRIZED:  // (vmc_create_symmetrized likewise)
      break;
    case PATH_FUSED_LDS: case PATH_DENSE_GENERAL:
      c->wrows = B > 131072 ? B : 131072;
      PROPAGATE(create_wide_rows(c));
      break;
    case PATH_NNB:
      PROPAGATE(create_nnb_blocks(c));
      PROPAGATE(create_wide_rows(c));
      PROPAGATE(create_sign(c, false));
      break;
    case PATH_EDVEC:
      PROPAGATE(create_sign(c, true));
      PROPAGATE(create_edvec(c));
      break;
    case PATH_PBDG:
      PROPAGATE(create_sign(c, true));
      PROPAGATE(create_pbdg(c));
      break;
    case PATH_CONV_GENERAL: PROPAGATE(create_conv_general(c)); break;
    case PATH_CONV: PROPAGATE(create_conv_fused(c)); break;
  }
  CA(hipStreamSynchronize(c->stream));
  return VMC_OK;
}
#undef NEW
#undef CA


}  // namespace vmcapi

extern "C" {

int64_t vmc_num_params(int32_t n_sites, int32_t layer_size, int32_t num_layers) {
  return plan_num_params_dense(VMC_ANSATZ_FULLY_CONNECTED, n_sites, layer_size, num_layers);
}

int64_t vmc_num_params_ansatz(int32_t ansatz, int32_t n_sites, int32_t layer_size, int32_t num_layers) {
  return plan_num_params_dense(ansatz, n_sites, layer_size, num_layers);
}

int64_t vmc_num_params_conv(int32_t ansatz, int32_t num_layers, int32_t num_filters, int32_t kernel_size) {
  if (ansatz == VMC_ANSATZ_GNN) return conv_num_params(num_layers, num_filters, kernel_size);   // k taps of 1 x k
  const bool resnet = ansatz == VMC_ANSATZ_RES_NET_2D || ansatz == VMC_ANSATZ_RES_NET_1D;
  const bool one_d = ansatz == VMC_ANSATZ_CONV_1D || ansatz == VMC_ANSATZ_RES_NET_1D;
  const int n_conv = resnet ? 1 + 2 * num_layers : num_layers;
  return conv_num_params(n_conv, num_filters, one_d ? kernel_size : kernel_size * kernel_size);
}

const char* vmc_last_error(const vmc_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int vmc_create(const vmc_desc* d, vmc_ctx** out) {
  if (!d || !out) return fail(nullptr, VMC_ERR_INVALID, "null argument");
  *out = nullptr;
  // every shape decision (ansatz, limits, LDS budgets, padded sizes, parameter layout): plan_desc, plan.hpp
  DescPlan dp;
  {
    char msg[256];
    const char* wf = getenv("CGS_VMC_WIDE_FAST");
    const char* fg = getenv("CGS_VMC_CONV_GENERAL");      // =1: the general convolution path for every shape (tests, A/B runs); =0: only where the fused kernels refuse
    const int rc = plan_desc(d, !(wf && atoi(wf) == 0), &dp, msg, sizeof(msg), fg ? (atoi(fg) != 0 ? 1 : -1) : 0);
    if (rc != VMC_OK) return fail(nullptr, rc, msg);
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, VMC_ERR_HIP, "no HIP device available: the VMC hot path has no CPU fallback");
  if (d->device < 0 || d->device >= ndev) return fail(nullptr, VMC_ERR_INVALID, "bad device ordinal");
  if ((e = hipSetDevice(d->device)) != hipSuccess)
    return fail(nullptr, VMC_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

  const bool no_network = path_no_network(dp.path);     // minimal dense-side shapes, no network buffers in use
  vmc_ctx* c = new vmc_ctx();
  c->d = *d;
  c->N = d->n_sites; c->B = d->batch_size; c->L = d->num_layers; c->H = d->layer_size;
  c->rbm = dp.rbm != 0;
  c->path = dp.path; c->cg = dp.cg;
  if (path_conv(dp.path)) { c->L = 1; c->overlap = false; }   // minimal dense-side shapes (unused)
  if (no_network) { c->L = 1; c->H = 1; c->overlap = false; c->hact = VMC_ACT_RELU_; }
  c->sgn = no_network || dp.path == PATH_NNB;
  if (dp.path == PATH_NNB || dp.path == PATH_EDVEC) c->ps[0].shift = c->ps[1].shift = 0.f;     // no exponent shift: psi = det M itself
  // more than 256 units: no overtaking sampler.  Of those, 257 .. 512 units (PATH_FUSED_LDS) run the fused sampler padded
  // to 384 / 512 units (k_sweep16<24|32>), rows on the LDS-operand kernel (k_tail_lds; without an H x H layer: k_tail0)
  // and the fused back-propagation (k_backprop16<24|32>); both dense ansatz types, every hidden activation
  if (path_wide(dp.path)) c->overlap = false;
  // (pbdg, nnb: the activations of the desc are ignored -- relu trunk, amplitudes kept as (logit, sign))
  c->hact = c->sgn ? VMC_ACT_RELU_ : d->nonlinearity; c->oact = c->sgn ? VMC_ACT_EXP_ : d->output_activation;
  c->lay = dp.lay;
  c->Hp = dp.Hp;
  c->n_hh = c->lay.n_hh; c->A = c->n_hh + 1;
  c->P = dp.P;
  c->stream = (hipStream_t)d->stream;
  if (const char* e = getenv("CGS_VMC_SWEEP_W1L")) c->sweep_no_w1l = atoi(e) == 0 ? 1 : 0;
  if (const char* e = getenv("CGS_VMC_SPLIT_BF16"))
    c->path = plan_split_path(dp, c->hact, atoi(e), sweep16_split_supported(c->N, c->Hp, c->n_hh));
  if (const char* e = getenv("CGS_VMC_OVERLAP")) {
    c->overlap = !path_conv(c->path) && !path_wide(c->path) && !no_network && atoi(e) != 0;
    c->overlap_full = atoi(e) == 2;
  }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) == hipSuccess && prop.multiProcessorCount > 0)
      c->num_cus = prop.multiProcessorCount;
  }
  // eight-chain sampler tiles where sixteen-chain tiles would leave half of the chip idle (sweep8.hip)
  c->sweep8_ok = (c->path == PATH_FUSED || c->path == PATH_SPLIT_ROWS) && !c->rbm && c->hact == VMC_ACT_RELU_ &&
                 plan_sweep8(c->N, c->Hp, c->n_hh, c->sweep_no_w1l != 0).ok;
  {
    int forced = 0;
    if (const char* e = getenv("CGS_VMC_SWEEP_TILE")) forced = atoi(e);
    c->sweep_tile = plan_sweep_tile(c->B, c->num_cus, c->sweep8_ok, forced);
  }
  if (create_buffers(c) != VMC_OK) { vmc_destroy(c); return VMC_ERR_HIP; }     // (g_create_error names the failure)
  *out = c;
  return VMC_OK;
}

void vmc_destroy(vmc_ctx* c) {
  if (!c) return;
  DeviceGuard device_guard_(c->d.device);
  if (c->sweep_stream) hipStreamSynchronize(c->sweep_stream);
  hipStreamSynchronize(c->stream);
  if (c->prod) prod_release(c);            // the factors are borrowed: they stay alive, free again
  if (c->symz) symz_release(c);            // (the base of a symmetrized ctx likewise)
  if (c->owner && c->owner->symz) symz_base_destroyed(c);
  if (c->owner) prod_child_destroyed(c);   // (a factor destroyed before its product: the product refuses from now on)
  drain_timings(c);
  if (c->sweep_stream) hipStreamDestroy(c->sweep_stream);
  for (hipStream_t q : c->cg_grp_stream) if (q) { hipStreamSynchronize(q); hipStreamDestroy(q); }
  for (hipEvent_t e : c->cg_grp_ev) if (e) hipEventDestroy(e);
  for (hipEvent_t e : {c->ev_mark, c->ev_now, c->ev_sweep_done}) if (e) hipEventDestroy(e);
  for (auto& e : c->event_pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (c->h_stage) hipHostFree(c->h_stage);
  delete c;      // every device buffer is a DevBuf: freed here, still on the ctx's device
}

int vmc_set_bonds(vmc_ctx* c, int32_t n_bonds, const int32_t* ij, const float* j_x, const float* j_z) {
  ENTER(c);
  if (n_bonds < 1 || !ij || !j_x || !j_z) return fail(c, VMC_ERR_INVALID, "bad bond arguments");
  // a symmetrized ctx, before anything changes: the ops must be symmetries, and the base -- whose batch_size x n_ops rows
  // are the larger demand -- takes the set first, so that a refusal of either leaves both ctxs as they were
  if (c->symz) {
    PROPAGATE(symz_set_bonds_check(c, n_bonds, ij, j_x, j_z));
    PROPAGATE(symz_set_bonds(c, n_bonds, ij, j_x, j_z));
  }
  // (the base of a symmetrized ctx called directly: the same question, asked of its owner's ops)
  if (c->owner && c->owner->symz) {
    const int rc = symz_set_bonds_check(c->owner, n_bonds, ij, j_x, j_z);
    if (rc != VMC_OK) { c->err = c->owner->err; return rc; }
  }
  // connected rows are indexed with 32-bit integers (at most one row per chain and bond)
  if ((long long)c->B * n_bonds > 0x7fffffffLL - c->B)
    return fail(c, VMC_ERR_UNSUPPORTED, "batch_size x n_bonds does not fit the 32-bit row index");
  std::vector<int2> b(n_bonds);
  std::vector<float> hx(n_bonds), qz(n_bonds);
  for (int k = 0; k < n_bonds; ++k) {
    const int i = ij[2 * k], j = ij[2 * k + 1];
    if (i < 0 || j < 0 || i >= c->N || j >= c->N || i == j)
      return fail(c, VMC_ERR_INVALID, "bond site index out of range (or i == j)");
    b[k] = make_int2(i, j);
    hx[k] = 0.5f * j_x[k];     // 0.25 * jx * 2   (operators.py:168-169)
    qz[k] = 0.25f * j_z[k];    // operators.py:169
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the five buffers of a bond list, all or none: the ctx has no bond set (n_bonds 0, null views) from here until the last
  // allocation and copy have succeeded
  c->n_bonds = 0;
  c->bonds = nullptr; c->half_jx = c->quarter_jz = c->val = nullptr; c->rowinfo = nullptr;
  c->ham_ij.assign(ij, ij + 2 * (size_t)n_bonds);
  c->ham_jx.assign(j_x, j_x + n_bonds); c->ham_jz.assign(j_z, j_z + n_bonds);
  c->bonds_epoch += 1;
  c->list_valid = false;
  c->cnt_valid = false;
  PROPAGATE(c->ham_bonds.alloc(c, n_bonds, "ham_bonds")); PROPAGATE(c->ham_half_jx.alloc(c, n_bonds, "ham_half_jx"));
  PROPAGATE(c->ham_quarter_jz.alloc(c, n_bonds, "ham_quarter_jz"));
  PROPAGATE(c->ham_rowinfo.alloc(c, (long long)c->B * n_bonds, "ham_rowinfo"));
  PROPAGATE(c->ham_val.alloc(c, (long long)c->B * n_bonds, "ham_val"));
  HIPCHK(c, hipMemcpy(c->ham_bonds, b.data(), n_bonds * sizeof(int2), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->ham_half_jx, hx.data(), n_bonds * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->ham_quarter_jz, qz.data(), n_bonds * sizeof(float), hipMemcpyHostToDevice));
  c->bonds = c->ham_bonds; c->half_jx = c->ham_half_jx; c->quarter_jz = c->ham_quarter_jz;
  c->rowinfo = c->ham_rowinfo; c->val = c->ham_val;
  c->n_bonds = n_bonds;
  if (c->prod) PROPAGATE(prod_set_bonds(c, n_bonds, ij, j_x, j_z));
  return VMC_OK;
}

int vmc_set_adjacency(vmc_ctx* c, int32_t n_sites, int32_t k, const int32_t* adj) {
  ENTER(c);
  if (!c->cg.graph) return fail(c, VMC_ERR_INVALID, "vmc_set_adjacency: not a gnn ctx");
  {
    char msg[256];
    const int rc = plan_gnn_check_adjacency(n_sites, k, c->N, c->cg.KW, adj, msg, sizeof(msg));
    if (rc != VMC_OK) return fail(c, rc, msg);
  }
  std::vector<int32_t> ptr((size_t)n_sites + 1), inv((size_t)n_sites * k);
  plan_gnn_inverse(n_sites, k, adj, ptr.data(), inv.data());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->gnn_adj) {
    PROPAGATE(c->gnn_adj.alloc(c, (long long)n_sites * k, "gnn_adj"));
    PROPAGATE(c->gnn_inv_ptr.alloc(c, (long long)n_sites + 1, "gnn_inv_ptr"));
    PROPAGATE(c->gnn_inv.alloc(c, (long long)n_sites * k, "gnn_inv"));
  }
  HIPCHK(c, hipMemcpy(c->gnn_adj, adj, (size_t)n_sites * k * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->gnn_inv_ptr, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->gnn_inv, inv.data(), inv.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  c->ps[0].cache_valid = c->ps[1].cache_valid = false;     // (the logits of the chains belong to the previous graph)
  c->cg_sr_tape_rows = 0;
  return VMC_OK;
}

int vmc_set_lin_tables(vmc_ctx* c, int32_t n_half, const int32_t* top, const int32_t* bot) {
  ENTER(c);
  if (c->path != PATH_EDVEC) return fail(c, VMC_ERR_INVALID, "vmc_set_lin_tables: not an ed_vector ctx");
  {
    char msg[256];
    const int rc = plan_edvec_check_tables(c->N, n_half, top, bot, c->P, msg, sizeof(msg));
    if (rc != VMC_OK) return fail(c, rc, msg);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->ed_bot) PROPAGATE(c->ed_bot.alloc(c, n_half, "ed_bot"));
  HIPCHK(c, hipMemcpy(c->ed_bot, bot, (size_t)n_half * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!c->ed_top) PROPAGATE(c->ed_top.alloc(c, n_half, "ed_top"));      // (set last: late_inputs_set takes it as "tables present")
  HIPCHK(c, hipMemcpy(c->ed_top, top, (size_t)n_half * sizeof(int32_t), hipMemcpyHostToDevice));
  c->ps[0].cache_valid = c->ps[1].cache_valid = false;     // (the amplitudes of the chains belong to the previous tables)
  return VMC_OK;
}

int vmc_set_params(vmc_ctx* c, int which, const float* theta) {
  ENTER(c);
  if ((which != 0 && which != 1) || !theta) return fail(c, VMC_ERR_INVALID, "bad arguments");
  if (c->symz) return symz_set_params(c, which, theta);      // theta is the base's
  HIPCHK(c, hipMemcpyAsync(c->ps[which].theta, theta, c->P * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ps[which].has_params = true;
  c->ps[which].packed_valid = c->ps[which].cache_valid = false;
  if (which == VMC_PSI) c->acts_valid = false;
  if (c->prod) PROPAGATE(prod_scatter_params(c, which));      // theta = a's floats followed by b's
  if (c->owner) { prod_child_params_changed(c, which); symz_base_params_changed(c, which); }
  return VMC_OK;
}

int vmc_get_params(vmc_ctx* c, int which, float* theta) {
  ENTER(c);
  if ((which != 0 && which != 1) || !theta) return fail(c, VMC_ERR_INVALID, "bad arguments");
  if (c->prod) PROPAGATE(prod_gather_params(c, which));
  if (c->symz) return symz_get_params(c, which, theta);
  if (!c->ps[which].has_params) return fail(c, VMC_ERR_STATE, "parameters not set");
  HIPCHK(c, hipMemcpyAsync(theta, c->ps[which].theta, c->P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VMC_OK;
}

int vmc_transfer_params(vmc_ctx* c) {
  ENTER(c);
  if (c->prod) return prod_transfer_params(c);
  if (c->symz) return symz_transfer_params(c);
  if (c->owner) { prod_child_params_changed(c, VMC_OMEGA); symz_base_params_changed(c, VMC_OMEGA); }
  if (!c->ps[0].has_params) return fail(c, VMC_ERR_STATE, "parameters not set");
  HIPCHK(c, hipMemcpyAsync(c->ps[1].theta, c->ps[0].theta, c->P * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  c->ps[1].has_params = true;
  c->ps[1].packed_valid = c->ps[1].cache_valid = false;
  return VMC_OK;
}

int vmc_set_configs(vmc_ctx* c, const float* configs) {
  ENTER(c);
  REFUSE_COMPOSED(c);
  if (!configs) return fail(c, VMC_ERR_INVALID, "null configs");
  PROPAGATE(check_sz0_rows(c, configs, c->B));
  if (c->symz) PROPAGATE(symz_check_configs(c, configs));      // (no row at a structural zero of the sector)
  const long long n = (long long)c->B * c->N;
  // staged in the alternate chain buffer (free between sampler launches), validated on the
  // device, and only then made current: a rejected batch leaves the chains untouched
  HIPCHK(c, hipMemcpyAsync(c->configs_alt, configs, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_check_pm1(c->stream, c->configs_alt, n, c->cnt));
  int bad = 0;
  HIPCHK(c, hipMemcpyAsync(&bad, c->cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (bad) return fail(c, VMC_ERR_INVALID, "configs must be +-1");
  HIPCHK(c, hipMemcpyAsync(c->configs, c->configs_alt, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  invalidate_configs(c);
  return VMC_OK;
}

int vmc_get_configs(vmc_ctx* c, float* configs) {
  ENTER(c);
  if (!configs) return fail(c, VMC_ERR_INVALID, "null configs");
  HIPCHK(c, hipMemcpyAsync(configs, c->configs, (long long)c->B * c->N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VMC_OK;
}

int vmc_set_shift(vmc_ctx* c, int which, float shift) {
  CHECK_CTX(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  switch (c->path) {
    case PATH_PRODUCT: return fail(c, VMC_ERR_INVALID, "prod: the product has no exponent shift of its own (set the factors')");
    case PATH_SYMMETRIZED: return fail(c, VMC_ERR_INVALID, "symmetrized: the symmetrized ctx has no exponent shift of its own (set the base's)");
    case PATH_NNB: case PATH_EDVEC: break;     // (neural-network backflow, ed_vector: no exponent shift, it stays 0)
    case PATH_FUSED: case PATH_FUSED_LDS: case PATH_DENSE_GENERAL: case PATH_CONV: case PATH_SPLIT_ROWS:
    case PATH_SPLIT_SWEEP: case PATH_CONV_GENERAL: case PATH_PBDG:
      c->ps[which].shift = shift;
      break;
  }
  return VMC_OK;
}

int vmc_get_shift(vmc_ctx* c, int which, float* shift) {
  CHECK_CTX(c);
  if ((which != 0 && which != 1) || !shift) return fail(c, VMC_ERR_INVALID, "bad arguments");
  *shift = c->ps[which].shift;
  return VMC_OK;
}

int vmc_amplitude(vmc_ctx* c, int which, const float* configs, int64_t n_rows, float* logit, float* psi) {
  ENTER(c);
  if (c->prod) return prod_amplitude(c, which, configs, n_rows, logit, psi);
  if (c->symz) return symz_amplitude(c, which, configs, n_rows, logit, psi);
  if (!configs) REFUSE_COMPOSED(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  if (n_rows < 0) return fail(c, VMC_ERR_INVALID, "n_rows < 0");
  std::vector<float> host((size_t)n_rows), hsign(c->sgn ? (size_t)n_rows : 0);
  if (!configs) {
    if (n_rows != c->B) return fail(c, VMC_ERR_INVALID, "n_rows must equal batch_size when configs == NULL");
    PROPAGATE(ensure_cache(c, which));
    HIPCHK(c, hipMemcpyAsync(host.data(), c->ps[which].logit, n_rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (c->sgn)
      HIPCHK(c, hipMemcpyAsync(hsign.data(), c->ps[which].sign, n_rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  } else if (n_rows > 0) {
    PROPAGATE(ensure_packed(c, which));
    PROPAGATE(check_sz0_rows(c, configs, n_rows));
    PROPAGATE(grow_tmp(c, n_rows));
    HIPCHK(c, hipMemcpyAsync(c->tmp_cfg, configs, n_rows * c->N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    PROPAGATE(rows_forward_device(c, which, c->tmp_cfg, n_rows, c->tmp_out, c->tmp_sign));
    HIPCHK(c, hipMemcpyAsync(host.data(), c->tmp_out, n_rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (c->sgn)
      HIPCHK(c, hipMemcpyAsync(hsign.data(), c->tmp_sign, n_rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const float shift = c->ps[which].shift;
  for (int64_t i = 0; i < n_rows; ++i) {
    if (logit) logit[i] = host[i];
    if (!psi) continue;
    switch (c->path) {
      case PATH_EDVEC: psi[i] = hsign[i]; break;                                   // the gathered entry itself
      case PATH_PBDG: case PATH_NNB: psi[i] = hsign[i] * expf(host[i] - shift); break;     // sign(det M) exp(logit - shift)
      case PATH_FUSED: case PATH_FUSED_LDS: case PATH_DENSE_GENERAL: case PATH_CONV: case PATH_SPLIT_ROWS:
      case PATH_SPLIT_SWEEP: case PATH_CONV_GENERAL:
        // wavefunctions.py:350-353: exp(x - shift) (232), or the output activation itself, no shift
        psi[i] = c->oact == VMC_ACT_EXP_ ? expf(host[i] - shift) : host_activation(c->oact, host[i]);
        break;
      case PATH_PRODUCT: case PATH_SYMMETRIZED: break;                             // (prod_amplitude / symz_amplitude, above)
    }
  }
  return VMC_OK;
}

int vmc_local_energy(vmc_ctx* c, int which, float* eloc, double* mean) {
  ENTER(c);
  REFUSE_COMPOSED(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  PROPAGATE(local_energy_device(c, which));
  if (mean) HIPCHK(c, launch_sum(c->stream, c->ps[which].eloc, c->B, c->d_sum));
  if (eloc) HIPCHK(c, hipMemcpyAsync(eloc, c->ps[which].eloc, c->B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  int cnt_total = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt_total, c->off + c->B, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  double s = 0.0;
  if (mean) HIPCHK(c, hipMemcpyAsync(&s, c->d_sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->last_rows = cnt_total;
  if (mean) *mean = s / (double)c->B;
  return VMC_OK;
}

int vmc_local_energy_terms(vmc_ctx* c, int which, float* diag, float* offdiag_over_psi) {
  ENTER(c);
  REFUSE_COMPOSED(c);
  if (which != 0 && which != 1) return fail(c, VMC_ERR_INVALID, "bad which");
  c->fs.want_parts = true;           // (the four-spin fold keeps its two parts for this entry alone)
  const int rc_eloc = local_energy_device(c, which);
  c->fs.want_parts = false;
  PROPAGATE(rc_eloc);
  if (diag) HIPCHK(c, hipMemcpyAsync(diag, c->diag, c->B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (offdiag_over_psi) HIPCHK(c, hipMemcpyAsync(offdiag_over_psi, c->offdiag, c->B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  // four-spin terms: the 1 of every active term's bracket belongs to diag, its three ratio terms to offdiag_over_psi
  std::vector<double> fs_parts(c->fs.n_terms > 0 ? 2 * (size_t)c->B : 0);
  if (c->fs.n_terms > 0) {
    HIPCHK(c, hipMemcpyAsync(fs_parts.data(), c->fs.dsum, c->B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fs_parts.data() + c->B, c->fs.osum, c->B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < fs_parts.size() / 2; ++k) {
    if (diag) diag[k] = (float)((double)diag[k] + fs_parts[k]);
    if (offdiag_over_psi) offdiag_over_psi[k] = (float)((double)offdiag_over_psi[k] + fs_parts[(size_t)c->B + k]);
  }
  return VMC_OK;
}

int vmc_debug_kernel_path(vmc_ctx* c, int32_t* path) {
  CHECK_CTX(c);
  if (!path) return fail(c, VMC_ERR_INVALID, "null");
  *path = c->path;
  return VMC_OK;
}

int vmc_debug_sweep_tile(vmc_ctx* c, int32_t set, int32_t* chains) {
  ENTER(c);
  REFUSE_PRODUCT(c, "vmc_debug_sweep_tile");
  if (set != 0 && set != 8 && set != 16) return fail(c, VMC_ERR_INVALID, "sweep tile: 0 (query), 8 or 16");
  if (set == 8 && !c->sweep8_ok) return fail(c, VMC_ERR_UNSUPPORTED, "no eight-chain sampler for this shape (fully_connected + relu, 128 or 256 padded units, n_sites <= units)");
  if (set) { PROPAGATE(join_sweep(c)); c->sweep_tile = set; }
  if (chains) *chains = c->sweep_tile;
  return VMC_OK;
}

int vmc_last_connected_rows(vmc_ctx* c, int64_t* rows) { CHECK_CTX(c); if (!rows) return fail(c, VMC_ERR_INVALID, "null"); *rows = c->last_rows; return VMC_OK; }

int vmc_timing_enable(vmc_ctx* c, int on) {
  CHECK_CTX(c);
  c->timing = on < 0 || on > 2 ? 1 : on;
  while (c->timing && c->event_pool.size() < 64) {   // enough for a dozen steps in flight
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a)); HIPCHK(c, hipEventCreate(&b));
    c->event_pool.emplace_back(a, b);
  }
  return VMC_OK;
}

int vmc_timing_reset(vmc_ctx* c) {
  CHECK_CTX(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  drain_timings(c);
  c->timings.clear();
  return VMC_OK;
}

int vmc_timing_get(vmc_ctx* c, const char* name, double* ms, int64_t* launches) {
  CHECK_CTX(c);
  if (!name) return fail(c, VMC_ERR_INVALID, "null name");
  drain_timings(c);
  auto it = c->timings.find(name);
  if (ms) *ms = it == c->timings.end() ? 0.0 : it->second.first;
  if (launches) *launches = it == c->timings.end() ? 0 : it->second.second;
  return VMC_OK;
}

int vmc_synchronize(vmc_ctx* c) {
  ENTER(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->sweep_stream));
  return VMC_OK;
}

int vmc_debug_gemm(vmc_ctx* c, int32_t M, int32_t N, int32_t K, const float* A, int64_t sam, int64_t sak,
                   int64_t a_len, const float* B, int64_t sbk, int64_t sbn, int64_t b_len, float* C) {
  ENTER(c);
  DevBuf<float> dA, dB, dC, ws;
  PROPAGATE(dA.alloc(c, a_len, "dA")); PROPAGATE(dB.alloc(c, b_len, "dB")); PROPAGATE(dC.alloc(c, (long long)M * N, "dC"));
  PROPAGATE(ws.alloc(c, 4LL * M * N, "ws"));
  HIPCHK(c, hipMemcpy(dA, A, a_len * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dB, B, b_len * sizeof(float), hipMemcpyHostToDevice));
  GemmArgs g; memset(&g, 0, sizeof(g));
  g.A = dA; g.sam = sam; g.sak = sak; g.B = dB; g.sbk = sbk; g.sbn = sbn;
  g.M = M; g.N = N; g.K = K; g.C = dC; g.ldc = N; g.epilogue = 0;
  g.splitk = K >= 256 ? 4 : 1; g.workspace = ws;
  HIPCHK(c, launch_gemm(c->stream, g));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(C, dC, (long long)M * N * sizeof(float), hipMemcpyDeviceToHost));
  return VMC_OK;
}


}  // extern "C"
