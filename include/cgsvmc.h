/*
 * cgsvmc.h -- C ABI of libcgsvmc_hip.so: the MI355X (gfx950) implementation of the
 * batched VMC inner loop of ClarkResearchGroup/cgs-vmc.
 *
 * The reference has no FFI: its boundary is the Python object API plus
 * tf.Session.run(op) on op handles.  Each entry point below is what a
 * ctypes binding for one of those op handles / object methods calls; the reference
 * interface it replaces is cited as file:line under /root/reference/cgs_vmc.
 *
 * Conventions: every function returns 0 on success or a negative vmc_status; the
 * message is available from vmc_last_error().  The caller owns all host buffers; the
 * library owns all device memory.  Calls are synchronous with respect to the host on
 * return unless stated otherwise (they are stream-ordered internally).  One vmc_ctx per
 * GPU; a ctx is not thread-safe; distinct ctxs are independent.
 *
 * Parameter vector order (wavefunctions.py:167-175, creation order of the snt.Linear
 * variables of FullyConnectedNetwork, wavefunctions.py:345-349):
 *   w_1[N,H] b_1[H] w_2[H,H] b_2[H] ... w_L[H,H] b_L[H] w_out[H,1] b_out[1],
 * every matrix row-major w[in][out]; P = N*H + H + (L-1)*(H*H + H) + H + 1 floats.
 * RestrictedBoltzmannNetwork (wavefunctions.py:391-452; Sonnet creates the variables when the
 * module is first connected, so the onsite layer of _build line 436 comes first):
 *   w_on[N,1] b_on[1] w_1[N,H] b_1[H] w_2[H,H] b_2[H] ... w_{L+1}[H,H] b_{L+1}[H],
 * P = N + 1 + N*H + H + L*(H*H + H) floats (L = num_fc_layers >= 0 relu layers).
 * Conv2DNetwork (wavefunctions.py:531-615) and ResNet2D (wavefunctions.py:710-809): one snt.Conv2D
 * per layers.Conv2dPeriodic in connection order -- conv_2d: num_conv_layers of them; res_net_2d:
 * the initial convolution, then first_conv, second_conv of every ResBlock2d (layers.py:200-201) --
 * each w[k][k][in_channels][F] (row-major) followed by b[F]; in_channels = 1 for the first, F after;
 * P = k*k*F + F + (n_conv - 1)*(k*k*F*F + F).
 * Conv1DNetwork (wavefunctions.py:455-527) and ResNet1D (wavefunctions.py:618-707): the same with
 * snt.Conv1D variables w[k][in_channels][F], b[F] per layers.Conv1dPeriodic;
 * P = k*F + F + (n_conv - 1)*(k*F*F + F).
 * GraphConvNetwork ('gnn', wavefunctions.py:1083-1154; layers.py:415-451): num_layers graph
 * convolutions over an adjacency list adj[N][k] (vmc_set_adjacency), each one snt.Conv2D with a
 * 1 x k kernel: w[1][k][in_channels][F] (row-major) followed by b[F];
 * P = k*F + F + (num_layers - 1)*(k*F*F + F).
 * ProjectedBDG ('pbdg', wavefunctions.py:876-928): the pairing matrix projected_bdg/pairing_matrix
 * [1][N][N], F[i][k] = theta[i*N + k] (i an up site, k a down site); P = N*N.  psi(x) = det M(x),
 * M[r][c] = F[U_r][D_c] over the up sites U and down sites D of x in ascending order: logit =
 * ln|det M|, psi = sign(det M) exp(logit - shift) (psi = 0, logit = -inf where M is singular).
 * n_sites must be even (VMC_ERR_INVALID otherwise) and at most 256 (VMC_ERR_UNSUPPORTED: M^-1 of
 * a chain stays in LDS); every configuration the ctx takes (vmc_set_configs, vmc_amplitude) must
 * have as many up as down spins (VMC_ERR_INVALID).  num_layers, layer_size and the activations are
 * ignored.  Stochastic reconfiguration is not available (vmc_sr_reserve: VMC_ERR_UNSUPPORTED).
 * FullyConnectedNNB ('fully_connected_nnb', VMC_ANSATZ_NNB, wavefunctions.py:931-998): neural-network
 * backflow.  The fully_connected trunk (num_layers = L >= 1 hidden layers of layer_size = H units,
 * always relu) followed by a pairing layer of N*N outputs: w_1 [N][H], b_1 [H], (w_l [H][H], b_l [H])
 * x (L - 1), w_out [H][N*N], b_out [N*N]; P = N*H + H + (L-1)*(H*H + H) + H*N*N + N*N.
 * F(x)[i][k] = out[i*N + k], psi(x) = det M(x), M[r][c] = F(x)[U_r][D_c] (the convention of pbdg):
 * logit = ln|det M|, psi = sign(det M) exp(logit); psi = 0, logit = -inf where M is singular.  There
 * is no exponent shift: vmc_set_shift and vmc_update_norm leave it at 0 and return VMC_OK.  The
 * activations of vmc_desc are ignored.  n_sites must be even (VMC_ERR_INVALID) and at most 256,
 * layer_size at most 512, num_layers at most 16 and batch_size * N*N at most 2^30
 * (VMC_ERR_UNSUPPORTED); configurations must have as many up as down spins (VMC_ERR_INVALID).
 * Stochastic reconfiguration is not available (vmc_sr_reserve: VMC_ERR_UNSUPPORTED).
 * FullVector ('ed_vector', VMC_ANSATZ_ED_VECTOR, wavefunctions.py:1001-1080): one trainable state vector
 * full_vector/ed_vector [len], theta[k] = entry k; vmc_desc.layer_size carries len, P = len; num_layers
 * and the activations are ignored.  The up spins of a configuration set bits: bot = sum_{i < N/2}
 * [s_i > 0] 2^i, top = sum_{i < N/2} [s_{N/2+i} > 0] 2^i, idx = top_table[top] + bot_table[bot] (Lin's
 * two tables, vmc_set_lin_tables), psi = theta[idx]: the gathered entry bit for bit, signed, possibly 0;
 * logit = ln|psi| (-inf at psi = 0).  Two configurations the tables send to one entry share a
 * parameter; O_k(b) = delta(k, idx_b) / psi_b, and chains with psi_b = 0 add nothing to the gradient
 * sums.  There is no exponent shift (vmc_set_shift and vmc_update_norm leave it at 0 and return VMC_OK).
 * n_sites must be even (VMC_ERR_INVALID) and at most 28 (VMC_ERR_UNSUPPORTED: the largest size the
 * kernels are tested at -- C(28,14) = 40,116,600 entries; the 32-bit index itself reaches N = 32),
 * 1 <= len < 2^31; configurations must have as many up as down spins (VMC_ERR_INVALID).  Stochastic
 * reconfiguration is not available (vmc_sr_reserve: VMC_ERR_UNSUPPORTED).
 */
#ifndef CGSVMC_H_
#define CGSVMC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vmc_ctx vmc_ctx;

typedef enum {
  VMC_OK = 0,
  VMC_ERR_INVALID = -1,     /* bad argument (ValueError in the reference API)      */
  VMC_ERR_UNSUPPORTED = -2, /* ansatz shape / activation without a HIP kernel       */
  VMC_ERR_HIP = -3,         /* HIP runtime failure                                  */
  VMC_ERR_STATE = -4        /* call order (e.g. accumulate before set_bonds)        */
} vmc_status;

/* which parameter set: psi is the trained wavefunction, omega its frozen supervisor
 * copy (copy.deepcopy(wavefunction), training.py:660). */
enum { VMC_PSI = 0, VMC_OMEGA = 1 };

/* accumulate / apply modes (training.GROUND_STATE_OPTIMIZERS, training.py:913-917); PENALIZED_ENERGY is an
 * extension (see vmc_overlap) */
enum { VMC_MODE_ENERGY_GRADIENT = 0, VMC_MODE_LOG_OVERLAP_ITSWO = 1 };
#define VMC_MODE_PENALIZED_ENERGY 2

/* wavefunctions.WAVEFUNCTION_TYPES with kernels (wavefunctions.py:1157-1170) */
enum { VMC_ANSATZ_FULLY_CONNECTED = 0, VMC_ANSATZ_RBM = 1, VMC_ANSATZ_CONV_2D = 2,
       VMC_ANSATZ_RES_NET_2D = 3, VMC_ANSATZ_CONV_1D = 4, VMC_ANSATZ_RES_NET_1D = 5,
       VMC_ANSATZ_GNN = 6, VMC_ANSATZ_PBDG = 7, VMC_ANSATZ_NNB = 9 /* 8 is unassigned */, VMC_ANSATZ_ED_VECTOR = 10,
       VMC_ANSATZ_PRODUCT = 11 /* vmc_create_product only: vmc_create refuses it (VMC_ERR_INVALID) */,
       VMC_ANSATZ_SYMMETRIZED = 13 /* vmc_create_symmetrized only: vmc_create refuses it (VMC_ERR_INVALID); 12 is unassigned */ };

/* layers.NONLINEARITIES ids (layers.py:13-21).  Every id is accepted as hidden and as output
 * activation of every ansatz type with kernels. */
enum { VMC_ACT_RELU = 0, VMC_ACT_EXP = 1, VMC_ACT_COS = 2, VMC_ACT_TAN = 3, VMC_ACT_TANH = 4,
       VMC_ACT_SIGMOID = 5, VMC_ACT_IDENTITY = 6 };

typedef struct {
  int32_t n_sites;           /* hparams.num_sites                (utils.py:98)       */
  int32_t batch_size;        /* chains owned by THIS ctx         (utils.py:135)      */
  int32_t num_layers;        /* hparams.num_fc_layers (utils.py:104); conv_2d: num_conv_layers
                                (108); res_net_2d: num_resnet_blocks (114)                     */
  int32_t layer_size;        /* hparams.fc_layer_size (utils.py:105): fully_connected and rbm take up
                                to 4096 units -- the fused kernels up to 512 (any nonlinearity),
                                beyond that the general multi-launch path
                                (materialised rows + GEMMs; two [131072][units] float
                                buffers per ctx: 4 GiB at 4096 units).  Convolutional ansatz types:
                                num_conv_filters (111): the fused kernels up to 64 (four 16-channel MFMA
                                blocks), the general path (feature maps in HBM, a GEMM per convolution) to 1024 */
  int32_t nonlinearity;      /* VMC_ACT_*: hparams.nonlinearity  (utils.py:128)      */
  int32_t output_activation; /* VMC_ACT_*: hparams.output_activation (utils.py:129)  */
  int32_t device;            /* HIP device ordinal                                   */
  int32_t chain_offset;      /* global id of local chain 0 (multi-GPU sharding)      */
  int32_t ansatz;            /* VMC_ANSATZ_*: hparams.wavefunction_type              */
  int32_t reserved;          /* 0                                                    */
  uint64_t seed;             /* Philox key                                           */
  void* stream;              /* hipStream_t to launch on, or NULL for the null stream*/
  /* convolutional ansatz types only (ignored otherwise) */
  int32_t kernel_size;       /* hparams.kernel_size (utils.py:110): fused kernels 1..9, general path to 31;
                                gnn: k, the neighbours per position of the adjacency list (2..64) */
  int32_t size_x, size_y;    /* hparams.size_x, size_y (utils.py:99-100); n_sites = size_x*size_y
                                (ignored by the 1-D types: the chain has n_sites sites; and by gnn) */
  int32_t reserved2;         /* 0                                                    */
} vmc_desc;

/* Number of parameters P for a given shape (no ctx needed). */
int64_t vmc_num_params(int32_t n_sites, int32_t layer_size, int32_t num_layers);
int64_t vmc_num_params_ansatz(int32_t ansatz, int32_t n_sites, int32_t layer_size,
                              int32_t num_layers);
/* convolutional ansatz types: layer_size = num_conv_filters, num_layers as in vmc_desc
 * (gnn: kernel_size = k, the neighbours per position) */
int64_t vmc_num_params_conv(int32_t ansatz, int32_t num_layers, int32_t num_filters,
                            int32_t kernel_size);

/* FullyConnectedNetwork.__init__ + graph_builders.get_configs: allocates everything.
 * wavefunctions.py:331-353, graph_builders.py:92-125. */
int vmc_create(const vmc_desc* desc, vmc_ctx** out);
/* ProductOfWavefunctions ('prod', wavefunctions.py:61-165, 1178-1194): psi(x) = psi_a(x) psi_b(x) over ONE set of chains.
 * a and b are ordinary ctxs that agree in n_sites, batch_size, device, chain_offset and stream (VMC_ERR_INVALID otherwise);
 * the product borrows them -- vmc_destroy on it leaves them alive and free again; destroy the product first.  Factors
 * taken: fully_connected and rbm (every width; exp output only: a positive amplitude with a shift), pbdg, ed_vector.  The
 * convolutional types, gnn, fully_connected_nnb, a dense factor with another output activation and a product of products
 * are refused (VMC_ERR_UNSUPPORTED).  If a factor is signed, every configuration needs Sz = 0, as for that factor alone.
 * theta = a's floats followed by b's, P = P_a + P_b; accumulators [g1_a g1_b | g2_a g2_b | 8 scalars].
 * The product owns the chains, the step counter, the accumulators and the Adam state; the sampler key is a's seed.  While a
 * factor is composed its chain-state entries (vmc_set_configs, vmc_mc_steps, vmc_mc_step_injected, vmc_local_energy*,
 * vmc_accumulate, vmc_apply_adam, vmc_update_norm, vmc_evaluate, the epoch entries, vmc_amplitude on its own chains) return
 * VMC_ERR_STATE; its parameter, shift and host-row vmc_amplitude entries keep working.
 * On the product: vmc_amplitude gives logit = (logit_a - shift_a) + (logit_b - shift_b) and psi = sign_a sign_b exp(logit)
 * (psi = 0, logit = -inf where a factor is zero or singular); vmc_get_shift returns 0, vmc_set_shift VMC_ERR_INVALID,
 * vmc_update_norm changes nothing (the factors' shifts stay where they are: everything runs in the log domain).  The
 * sampler draws the proposals every sampler draws, evaluates both factors in full on the candidates and accepts where
 * dlogit_a + dlogit_b > 0.5 log u; a candidate with psi = 0 is rejected, a chain at psi = 0 accepts any candidate that is
 * not (what the pbdg, fully_connected_nnb and ed_vector samplers do).  Local energies: the off-diagonal row term is the
 * product of the factors' ratios times the bond's coupling, taken once.  The vmc_sr_* entries, the _dist entries, every
 * entry with world_size > 1, the reduce hooks, vmc_debug_sweep_profile, vmc_debug_sweep_tile and vmc_debug_conv_patch
 * return VMC_ERR_UNSUPPORTED.  The vmc_timing_* entries report the product's own regions ("sweep", "eloc_reduce", "grad"). */
int vmc_create_product(vmc_ctx* a, vmc_ctx* b, vmc_ctx** out);
/* The symmetrized ansatz (extension): psi_s(x) = sum_k chi_k psi(g_k x) over ONE set of batch_size chains, sampled from
 * |psi_s|^2 and trained with its own log-derivatives.  g_k: row_k[i] = f_k x[perms[k][i]], f_k = -1 where flips[k] (NULL: no
 * flips), as in vmc_symmetry_expectations; characters [n_ops]: the real characters chi_k of one sector.  The base is an
 * ordinary ctx of batch_size x n_ops rows (VMC_ERR_INVALID otherwise, both numbers named) that the symmetrized ctx borrows
 * as a product borrows its factors: fully_connected and rbm (every width, exp output only), pbdg or ed_vector; everything
 * else, a product and a symmetrized ctx are refused (VMC_ERR_UNSUPPORTED), a base that is already composed with
 * VMC_ERR_STATE.  1 <= n_ops <= 1024, every perm a bijection, every character finite and not all zero (VMC_ERR_INVALID).
 * With flips, or a signed base, every configuration needs Sz = 0.
 * The base holds the permuted rows (row = k batch_size + chain) as its chains and does all network arithmetic; theta IS the
 * base's (vmc_set_params / vmc_get_params / vmc_transfer_params on either ctx reach the same floats), P = the base's; the
 * symmetrized ctx owns the chains, the step counter, the accumulators [2 P + 8] and the Adam state.  While composed the base's
 * chain-state entries return VMC_ERR_STATE; vmc_destroy of the symmetrized ctx frees it again, vmc_destroy of the base first
 * leaves a symmetrized ctx whose every entry returns VMC_ERR_STATE.
 * vmc_amplitude: per row, in fp64 with the ops ascending, m = max_k ln|psi(g_k x)| over the ops with chi_k != 0 and a
 * nonzero amplitude, S = sum_k chi_k s_k exp(l_k - m), A = sum_k |chi_k| exp(l_k - m); logit = (m + ln|S|) - shift_base,
 * psi = sgn(S) exp(logit) (ed_vector base: psi = sum_k chi_k psi_k itself).  Where |S| <= 2^-40 A the row is at a structural
 * zero of the sector: psi = 0, logit = -inf.  vmc_get_shift returns 0, vmc_set_shift VMC_ERR_INVALID, vmc_update_norm
 * changes nothing.  vmc_set_configs refuses a batch with a row at a structural zero (VMC_ERR_INVALID, the row named; if every
 * row is, the message says that the state has no weight in this sector) and leaves the chains untouched; the sampler rejects
 * every candidate at a zero, so no chain is ever at one.  vmc_set_bonds forwards to the base and refuses a bond set the ops
 * do not map onto itself (VMC_ERR_INVALID, op and bond named, as vmc_projected_energy).
 * Local energies: E_s(x) = sum_k c_k E_loc^psi(g_k x) with c_k = chi_k psi(g_k x) / psi_s(x); gradient sums likewise over
 * O(g_k x).  The connected-row count is the base's, over all ops.  Modes 1 and 2 of vmc_accumulate, vmc_epoch_log_overlap,
 * the vmc_sr_* entries, the _dist entries, every entry with world_size > 1, the reduce hooks, the measurement entries,
 * vmc_create_product with a symmetrized factor, vmc_debug_sweep_profile, vmc_debug_sweep_tile and vmc_debug_conv_patch
 * return VMC_ERR_UNSUPPORTED.  vmc_timing_* regions: "sweep", "symz_rows", "symz_fold", "eloc_fold", "grad". */
int vmc_create_symmetrized(vmc_ctx* base, int32_t batch_size, int32_t n_ops, const int32_t* perms /*[n_ops][N]*/,
                           const uint8_t* flips /*[n_ops] or NULL*/, const double* characters /*[n_ops]*/, vmc_ctx** out);
void vmc_destroy(vmc_ctx* ctx);
const char* vmc_last_error(const vmc_ctx* ctx); /* ctx may be NULL: last create error */

/* HeisenbergHamiltonian(bonds, j_x, j_z), operators.py:215-225.  j_x / j_z are
 * per-bond arrays of length n_bonds (constant arrays reproduce the reference). */
int vmc_set_bonds(vmc_ctx* ctx, int32_t n_bonds, const int32_t* ij /*[n_bonds][2]*/,
                  const float* j_x, const float* j_z);

/* The gnn ansatz's graph (GraphConvNetwork, wavefunctions.py:1083-1154): adj[n][t] is the site
 * that tap t of position n reads (np.genfromtxt(adjacency_list_path, dtype=int)); repeated entries
 * are allowed.  n_sites and k must be the ctx's num_sites and kernel_size, every entry in
 * [0, n_sites).  Validates the table, uploads it and its inverse lists (for every site, the
 * (position, tap) pairs that read it, CSR, position-major).  Every forward, sampler, local-energy,
 * gradient or SR entry of a gnn ctx returns VMC_ERR_INVALID until the table is set; other ansatz
 * types refuse the call (VMC_ERR_INVALID). */
int vmc_set_adjacency(vmc_ctx* ctx, int32_t n_sites, int32_t k, const int32_t* adj /*[n_sites][k]*/);
/* The ed_vector ansatz's Lin tables (FullVector, wavefunctions.py:1001-1080): top[t] + bot[b] is the
 * entry of the configuration with upper half-word t and lower half-word b.  n_half must be
 * 2^(num_sites / 2), and every configuration with as many up as down spins must land in [0, len)
 * (VMC_ERR_INVALID otherwise; two configurations may share an entry).  Every forward, sampler,
 * local-energy, gradient or evaluation entry of an ed_vector ctx returns VMC_ERR_INVALID until the
 * tables are set; other ansatz types refuse the call (VMC_ERR_INVALID). */
int vmc_set_lin_tables(vmc_ctx* ctx, int32_t n_half /*2^(N/2)*/, const int32_t* top, const int32_t* bot);
/* Variable assignment / read-back (tf.train.Saver restore/save, run_training.py:134-146;
 * module_transfer_ops, wavefunctions.py:300-325). theta has P floats. */
int vmc_set_params(vmc_ctx* ctx, int which, const float* theta);
int vmc_get_params(vmc_ctx* ctx, int which, float* theta);
int vmc_transfer_params(vmc_ctx* ctx); /* psi -> omega: TrainOpsSWO.update_supervisor */

/* The CONFIGS variable, graph_builders.py:92-125: [batch_size][n_sites] float32 +-1. */
int vmc_set_configs(vmc_ctx* ctx, const float* configs);
int vmc_get_configs(vmc_ctx* ctx, float* configs);

/* exp_norm_shift (wavefunctions.py:206-232), per parameter set. */
int vmc_set_shift(vmc_ctx* ctx, int which, float shift);
int vmc_get_shift(vmc_ctx* ctx, int which, float* shift);

/* Wavefunction.__call__ (wavefunctions.py:355-371) on `configs` ([n_rows][n_sites],
 * host) or, when configs == NULL, on the ctx's chains (n_rows must be batch_size).
 * Writes the pre-exp logit and/or psi = exp(logit - shift); either may be NULL. */
int vmc_amplitude(vmc_ctx* ctx, int which, const float* configs, int64_t n_rows,
                  float* logit, float* psi);

/* n_steps x session.run(mc_step): graph_builders.py:38-89, driven by training.py:608-609
 * and evaluation.py:138-145.  One launch; chain state stays on the GPU.  *accepted (may be
 * NULL) receives the total acceptance_count (graph_builders.py:86). */
int vmc_mc_steps(vmc_ctx* ctx, int64_t n_steps, int64_t* accepted);

/* Test hook: one mc_step with externally supplied proposals: site to lower i_up, site to
 * raise i_dn, acceptance uniform u (all [batch_size]); accept_mask [batch_size] out. */
int vmc_mc_step_injected(vmc_ctx* ctx, const int32_t* i_up, const int32_t* i_dn,
                         const float* u, uint8_t* accept_mask);

/* Test hook: the proposals the sampler would draw at absolute step `step` for the
 * current chains (graph_builders.py:59-65), without moving. */
int vmc_debug_proposals(vmc_ctx* ctx, uint64_t step, int32_t* i_up, int32_t* i_dn, float* u);
/* Diagnostic: runs n_steps mc_steps through the s_memtime-stamped instantiation of the sweep
 * kernel and returns the mean shader cycles per step of up to 16 phases (see
 * engine.debug_sweep_profile for their names).  Never quote its run time. */
int vmc_debug_sweep_profile(vmc_ctx* ctx, int64_t n_steps, double* phase_cycles /*[16]*/);
int vmc_get_step_counter(vmc_ctx* ctx, uint64_t* step);
int vmc_set_step_counter(vmc_ctx* ctx, uint64_t step);

/* HeisenbergHamiltonian.local_value (operators.py:249-259) of parameter set `which` on
 * the ctx's chains: eloc [batch_size] (may be NULL), *mean = mean over the batch
 * (evaluation.py:102).  diag/offdiag_over_psi (may be NULL) are the two terms of
 * HeisenbergHamiltonian.build (operators.py:227-247) with the off-diagonal one already
 * divided by psi. */
int vmc_local_energy(vmc_ctx* ctx, int which, float* eloc, double* mean);
int vmc_local_energy_terms(vmc_ctx* ctx, int which, float* diag, float* offdiag_over_psi);

/* TrainOps.accumulate_gradients: training.py:539-558 (mode ENERGY_GRADIENT) or
 * training.py:661-695 (mode LOG_OVERLAP_ITSWO, beta = hparams.time_evolution_beta). */
/* Mode PENALIZED_ENERGY (extension, no reference counterpart): beta carries the penalty lambda of E[psi] + lambda F(psi,
 * omega) against the frozen set omega; the weights of the second sum are w_c = E_loc(c) + lambda (S1 / S2) r_c (see
 * vmc_overlap), the scalars get e_total += sum E_loc, r_total += sum w and the two counts as mode LOG_OVERLAP_ITSWO fills
 * them, slot 5 += the call's fidelity estimate S1^2 / (alive S2) and slot 6 += 1.  One rank only.  Refusals, before
 * anything is launched: a product ctx or an output activation other than exp on an unsigned type: VMC_ERR_UNSUPPORTED;
 * omega unset, or an SR sample store reserved: VMC_ERR_STATE; lambda < 0 or not finite: VMC_ERR_INVALID. */
int vmc_accumulate(vmc_ctx* ctx, int mode, float beta);
/* TrainOps.reset_gradients: tf.variables_initializer(tf.local_variables()). */
int vmc_reset_accumulators(vmc_ctx* ctx);
/* Accumulator buffer: [g1 (P) | g2 (P) | e_total e_count r_total r_count g_count f_total f_count 0]
 * = 2P+8 floats (f_total / f_count: mode PENALIZED_ENERGY only, 0 otherwise).  The device pointer is
 * exposed so the host can all-reduce it in place (RCCL via torch.distributed); *n_floats = 2P+8. */
int vmc_accumulators_devptr(vmc_ctx* ctx, void** dev_ptr, int64_t* n_floats);
/* The same all-reduce for hosts without torch.distributed: nccl_comm is an existing ncclComm_t of
 * RCCL (NULL or world_size <= 1: no-op); stream-ordered on the ctx's stream, g_count corrected.
 * librccl is resolved with dlopen at the first call. */
int vmc_allreduce_accumulators(vmc_ctx* ctx, void* nccl_comm, int32_t world_size);
int vmc_get_accumulators(vmc_ctx* ctx, float* host /*[2P+8]*/);
int vmc_set_accumulators(vmc_ctx* ctx, const float* host /*[2P+8]*/);

/* TrainOps.apply_gradients: gradient formula (training.py:560-564 or 697-699) + TF1
 * Adam (training.py:84-91).  *energy (may be NULL) = TrainOps.metrics / .energy.
 * Mode PENALIZED_ENERGY: grad = g2 / n - (r_total / r_count) g1 / n, the energy still e_total / e_count. */
int vmc_apply_adam(vmc_ctx* ctx, int mode, float lr, float beta1, float beta2, float eps,
                   double* energy);
int vmc_get_gradient(vmc_ctx* ctx, int mode, float* grad /*[P]*/);
int vmc_mean_energy(vmc_ctx* ctx, double* energy);
int vmc_get_adam_state(vmc_ctx* ctx, float* m, float* v, int64_t* t);
int vmc_set_adam_state(vmc_ctx* ctx, const float* m, const float* v, int64_t t);

/* Whole-epoch entry points: the op sequences of run_optimization_epoch in
 * ONE host call, no Python round trip per op.
 * EnergyGradient (training.py:608-617): n_eq_steps mc_steps, update_norm (skipped when
 * max_value <= 0), reset, n_batches x [accumulate, n_mc_steps mc_steps].  apply_gradients is
 * left to the caller (the multi-GPU all-reduce sits in between).
 * LogOverlapITSWO (training.py:750-763): n_eq_steps mc_steps, update_norm, update_supervisor,
 * n_batches x [n_mc_steps mc_steps, reset, accumulate, Adam]; *energy = mean of the last batch.
 * Single-GPU only (Adam needs the reduced accumulators every batch). */
int vmc_epoch_energy_gradient(vmc_ctx* ctx, int64_t n_eq_steps, int32_t n_batches,
                              int64_t n_mc_steps, float max_value);
int vmc_epoch_log_overlap(vmc_ctx* ctx, float beta, int64_t n_eq_steps, int32_t n_batches,
                          int64_t n_mc_steps, float max_value, float lr, float beta1, float beta2,
                          float eps, double* energy);
/* The EnergyGradient epoch with vmc_accumulate(ctx, VMC_MODE_PENALIZED_ENERGY, lambda) in its accumulate's place
 * (extension; one rank only). */
int vmc_epoch_penalized_energy(vmc_ctx* ctx, float lambda, int64_t n_eq_steps, int32_t n_batches,
                               int64_t n_mc_steps, float max_value);

/* ---- chains sharded over ranks (the reference is single-process) ----------------
 * Rank r owns chains [r B/G, (r+1) B/G) (vmc_desc.chain_offset); the only exchanges are a SUM
 * all-reduce of the accumulator buffer per optimizer step, a MAX all-reduce of one float for
 * update_norm and a SUM all-reduce of P+1 floats per CG iteration of the SR extension.  The
 * entries below issue them IN STREAM, between the kernels of the epoch, so that a multi-rank
 * epoch is one host call per rank exactly like the single-rank one.
 *
 * Transport: an RCCL communicator (`nccl_comm` = ncclComm_t; librccl is resolved with dlopen at
 * first use, the copy torch has already loaded if there is one) or, when nccl_comm == NULL and
 * world_size > 1, the device hook of vmc_set_device_allreduce (below) or the host hook registered
 * with vmc_set_host_allreduce: the library copies the buffer to pinned host memory, calls the hook
 * (which must all-reduce host_buf in place over all ranks: gloo, MPI, ...), and copies it back.  nccl_comm == NULL with world_size <= 1 is the
 * single-rank no-op; a 1-rank communicator still goes through ncclAllReduce. */
enum { VMC_REDUCE_SUM = 0, VMC_REDUCE_MAX = 1,
       VMC_REDUCE_SUM_F64 = 2 /* the buffer holds n DOUBLES (vmc_evaluate's batch means) */ };
typedef int (*vmc_host_allreduce_fn)(void* user, float* host_buf, int64_t n_elements, int32_t op);
int vmc_set_host_allreduce(vmc_ctx* ctx, vmc_host_allreduce_fn hook, void* user);
/* CONTRACT CHANGE (round 4 -> 5): op VMC_REDUCE_SUM_F64 hands the hook n_elements DOUBLES in host_buf
 * (cast the pointer).  A hook written for ops 0 / 1 would silently reduce half of them as floats, so the
 * library only passes op 2 to a host hook that has declared it: vmc_set_host_allreduce_caps(ctx,
 * VMC_HOST_REDUCE_CAP_F64) after registering it (registering a hook clears the caps).  Without the
 * declaration the entries that need it (vmc_evaluate with world_size > 1 on the host hook) return
 * VMC_ERR_UNSUPPORTED.  The device hook always receives op 2 (its contract has had it from the start). */
enum { VMC_HOST_REDUCE_CAP_F64 = 1 };
int vmc_set_host_allreduce_caps(vmc_ctx* ctx, int32_t caps);
/* Third transport, for hosts whose collective library keeps its communicator to itself but reduces
 * device memory in stream order (torch.distributed's ProcessGroupNCCL = RCCL on ROCm): with
 * nccl_comm == NULL and world_size > 1 the library calls this hook -- when one is registered it wins
 * over the host hook -- at the point of the epoch where the all-reduce belongs.  The hook must ENQUEUE
 * an in-place all-reduce of n_elements (float32; float64 for VMC_REDUCE_SUM_F64) at dev_buf that is
 * ordered after the work already on `stream` (the ctx's hipStream_t, NULL = the null stream) and
 * before whatever is enqueued on it afterwards; it need not wait for completion.  No staging copy,
 * no host synchronisation. */
typedef int (*vmc_device_allreduce_fn)(void* user, void* dev_buf, int64_t n_elements, int32_t op,
                                       void* stream);
int vmc_set_device_allreduce(vmc_ctx* ctx, vmc_device_allreduce_fn hook, void* user);
/* Communicator life cycle for hosts whose collective library does not expose its ncclComm_t
 * (torch.distributed): rank 0 draws the 128-byte ncclUniqueId and shares it by any channel, every
 * rank then calls vmc_rccl_comm_create (ncclCommInitRank on `device`). */
int vmc_rccl_unique_id(uint8_t id[128]);
int vmc_rccl_comm_create(const uint8_t id[128], int32_t world_size, int32_t rank, int32_t device,
                         void** nccl_comm);
int vmc_rccl_comm_destroy(void* nccl_comm);
const char* vmc_rccl_last_error(void);
/* File the library's nccl* entry points were resolved from: the librccl next to the libamdhip64 this
 * library is bound to (a process can hold two ROCm stacks -- torch bundles its own -- and streams,
 * buffers and communicators of one must not be handed to the other), else the first librccl.so.1 on
 * the loader path; "" when none was found.  A caller's ncclComm_t must come from THIS instance: a
 * communicator of another librccl in the process is rejected by ncclAllReduce as corrupted. */
const char* vmc_rccl_library_path(void);
/* PCI bus id ("0000:75:00.0") of HIP device `device`, and the file of the libamdhip64 behind this
 * library's hip* symbols -- both answered by THE runtime the library is bound to, so a caller that
 * wants to tell two ranks' devices apart never has to open a HIP runtime of its own by soname (a
 * second runtime in the process: see vmc_rccl_library_path).  Needs no ctx; `len` >= 16. */
int vmc_device_pci_bus_id(int32_t device, char* buf, int32_t len);
const char* vmc_hip_runtime_path(void);
/* Test / diagnostic hook: in-place all-reduce of n_floats of host data through the same transport
 * (staged through the ctx's device scratch for RCCL); op = VMC_REDUCE_*. */
int vmc_debug_allreduce(vmc_ctx* ctx, void* nccl_comm, int32_t world_size, float* host,
                        int64_t n_floats, int32_t op);
/* Wavefunction.update_norm with max_b psi taken over the chains of ALL ranks (logit domain). */
int vmc_update_norm_dist(vmc_ctx* ctx, void* nccl_comm, int32_t world_size, float max_value);
/* vmc_epoch_energy_gradient over sharded chains: update_norm sees the global maximum and the
 * accumulators are all-reduced (g_count corrected) before the call returns, ready for
 * vmc_apply_adam / vmc_sr_solve_dist on every rank. */
int vmc_epoch_energy_gradient_dist(vmc_ctx* ctx, void* nccl_comm, int32_t world_size,
                                   int64_t n_eq_steps, int32_t n_batches, int64_t n_mc_steps,
                                   float max_value);
/* vmc_epoch_log_overlap over sharded chains (training.py:750-763): per batch
 * [n_mc_steps mc_steps, reset, accumulate, all-reduce, Adam] with no host synchronisation;
 * every rank applies the identical Adam step.  With a 1-rank communicator the result is
 * bit-identical to vmc_epoch_log_overlap. */
int vmc_epoch_log_overlap_dist(vmc_ctx* ctx, void* nccl_comm, int32_t world_size, float beta,
                               int64_t n_eq_steps, int32_t n_batches, int64_t n_mc_steps,
                               float max_value, float lr, float beta1, float beta2, float eps,
                               double* energy);

/* MonteCarloOperatorEvaluator.run_evaluation (evaluation.py:113-152) in ONE host call: n_eq_steps
 * mc_steps, then n_samples x [batch mean of the Hamiltonian's local value (evaluation.py:102),
 * n_mc_steps mc_steps].  The batch sums stay on the device; with sharded chains (transport as
 * above) the n_samples per-rank means are SUM-all-reduced in float64 in one collective at the end
 * and divided by world_size, exactly what the op-by-op loop does per sample.  means[n_samples]
 * receives the list run_evaluation returns (as doubles; the Python side rounds to float32 like
 * tf.reduce_mean); *accepted (may be NULL) the acceptance count of THIS rank's chains over the
 * n_samples x n_mc_steps measurement steps (the count the reference computes and drops). */
int vmc_evaluate(vmc_ctx* ctx, void* nccl_comm, int32_t world_size, int64_t n_eq_steps,
                 int32_t n_samples, int64_t n_mc_steps, double* means, int64_t* accepted);

/* Spin correlations -- EXTENSION with no reference counterpart (the reference measures the energy alone).  Over the
 * ctx's current chains, for every pair k = (i, j) of `ij`:
 *   zz_sum[k] = sum_c s_i s_j                                     (integers, exact)
 *   ex_sum[k] = sum_c [s_i s_j < 0] psi(swap_ij x_c) / psi(x_c)   (chains in ascending order, fp64)
 * so that <S_i . S_j> = (zz_sum / 4 + ex_sum / 2) / batch_size; either array may be NULL.  The ratios are the rows of the
 * local energies, evaluated by the kernels of the ctx's ansatz type over a bond set of the pairs (j_x = 2, j_z = 0) that
 * stands in for the Hamiltonian's during a pass and is swapped out again.  The pairs run in passes of at most
 * pairs_per_pass pairs (0: as many as the row budget of a pass takes; a request is clamped to it); the sum of a pair
 * does not depend on the passes or on the other pairs of the list.  A pure measurement: chains, step counter,
 * accumulators, the Hamiltonian's bonds and couplings and the validity of the amplitude caches are as before on return
 * (no vmc_set_bonds is needed before it).  i == j or a site out of range: VMC_ERR_INVALID; a product ctx:
 * VMC_ERR_UNSUPPORTED; a factor of a product ctx: VMC_ERR_STATE. */
int vmc_pair_correlations(vmc_ctx* ctx, int which, int32_t n_pairs, const int32_t* ij /*[n_pairs][2]*/,
                          int32_t pairs_per_pass /*0: planner's choice*/,
                          double* zz_sum /*[n_pairs]*/, double* ex_sum /*[n_pairs]*/);

/* Renyi-2 entanglement entropy by the replica swap estimator -- EXTENSION with no reference counterpart.  The ctx's chains
 * are taken as B / 2 replica pairs (c, c + B / 2) (batch_size must be even).  For every region A of `region_mask` (one 0/1
 * byte per site) a pair MATCHES when both chains hold the same sum of spins on A; x~ is x_c with the sites of A taken from
 * x_{c + B/2}, y~ the other way round.  With l = ln|psi|:
 *   swap_sum[A]    = sum over matching pairs of sigma exp((l(x~) + l(y~)) - (l(x_c) + l(x_{c + B/2})))   (pairs ascending, fp64)
 *   match_count[A] = the number of matching pairs
 * so that Tr rho_A^2 ~ swap_sum / (B / 2) and S2 = -ln of it; either array may be NULL.  sigma is the product of the four
 * signs for the signed types (pbdg, fully_connected_nnb, ed_vector) and 1 otherwise; a pair that does not match would
 * leave the Sz = 0 sector (psi = 0) and contributes 0, and so does a pair with a vanishing amplitude among the four
 * (exactly 0, never NaN).  The swapped rows go through the full forward of the ctx's ansatz type (the device path of
 * vmc_amplitude); the chains' own l and signs are the ctx's cache.  The regions run in passes of at most regions_per_pass
 * regions (0: as many as the row budget of a pass takes; a request is clamped to it); the sums of a region do not depend
 * on the passes or on the other regions of the call.  The empty region and the full set of sites are legal (both give
 * B / 2 and B / 2).  A pure measurement: chains, step counter, accumulators, the Hamiltonian's bonds and the validity of the
 * amplitude and activation caches are as before on return.  Odd batch_size, n_regions < 1, a NULL mask, which outside
 * {0, 1}, regions_per_pass < 0: VMC_ERR_INVALID, before anything touches the device; an output activation other than
 * exp on an unsigned type (the logit is then not ln psi) and a product ctx: VMC_ERR_UNSUPPORTED; a factor of a product
 * ctx: VMC_ERR_STATE, as every chain-state entry. */
int vmc_renyi2_swap(vmc_ctx* ctx, int which, int32_t n_regions, const uint8_t* region_mask /*[n_regions][N], 0/1*/,
                    int32_t regions_per_pass /*0: planner's choice*/,
                    double* swap_sum /*[n_regions]*/, double* match_count /*[n_regions]*/);

/* Dimer-dimer correlations <(S_i . S_j)(S_k . S_l)> -- EXTENSION with no reference counterpart.  `bonds` lists site pairs
 * (any two distinct sites, not only the Hamiltonian's), `pairs` lists ordered pairs (a, b) of indices into `bonds`.  With
 * r(y) = psi(y) / psi(x), [p != q] = 1 when the spins of sites p and q differ, x' = swap_ij x and s' the spins of x':
 *   bond(a; x)  = s_i s_j / 4 + [s_i != s_j] r(swap_ij x) / 2                                  a = (i, j)
 *   dd(a, b; x) = s_i s_j / 4 (s_k s_l / 4 + [s_k != s_l] r(swap_kl x) / 2)                    b = (k, l)
 *               + [s_i != s_j] / 2 (s'_k s'_l r(x') / 4 + [s'_k != s'_l] r(swap_kl x') / 2)
 * which is <x| (S_i . S_j)(S_k . S_l) |psi> / psi(x): the second bond acts on the intermediate configuration x', so bonds
 * that share a site and a == b need no form of their own.  Over the ctx's current chains, ascending, in fp64:
 *   bond_sum[a] = sum_c bond(a; x_c)            dd_sum[p] = sum_c dd(a_p, b_p; x_c)
 * so that <A B> ~ dd_sum / batch_size, <A> ~ bond_sum / batch_size; either array may be NULL, n_pairs = 0 gives the bonds
 * alone.  The ratios are exp of differences of ln|psi| times the signs of the signed types; every exchanged configuration
 * goes through the full forward of the ctx's ansatz type (the device path of vmc_amplitude): n_bonds x B single exchanges
 * in passes of at most pairs_per_pass bonds, kept per (bond, chain) on the device, then B double exchanges per pair in
 * passes of at most pairs_per_pass pairs (0: as many as the row budget of a pass takes, in either phase; a request is
 * clamped to it, for each phase by itself).  A sum depends neither on the passes nor on the
 * other entries of the two lists.  A vanishing amplitude of a row gives the ratio 0 and a chain whose own amplitude
 * vanishes adds 0 to every sum (exactly, never NaN).  A pure measurement: chains, step counter, accumulators, the
 * Hamiltonian's bonds and couplings and the validity of the amplitude and activation caches are as before on return.
 * A bond with i == j, a site or a bond index out of range, n_bonds < 1, n_pairs < 0, pairs_per_pass < 0, a NULL list
 * that is not empty, which outside {0, 1}: VMC_ERR_INVALID, before anything touches the device; an output activation
 * other than exp on an unsigned type and a product ctx: VMC_ERR_UNSUPPORTED; a factor of a product ctx: VMC_ERR_STATE. */
int vmc_dimer_correlations(vmc_ctx* ctx, int which, int32_t n_bonds, const int32_t* bonds /*[n_bonds][2] sites*/,
                           int32_t n_pairs, const int32_t* pairs /*[n_pairs][2] indices into bonds: (a, b)*/,
                           int32_t pairs_per_pass /*0: planner's choice*/,
                           double* bond_sum /*[n_bonds]*/, double* dd_sum /*[n_pairs]*/);

/* Symmetry expectation values -- EXTENSION with no reference counterpart.  An op k is the site permutation perm_k,
 * followed by the global spin flip where flip[k] is 1 (flip NULL: no flips): row_{k,c}[i] = f_k x_c[perm_k[i]] with
 * f_k = -1 where flip[k] and +1 otherwise.  Over the ctx's current chains, with l = ln|psi|:
 *   ratio_sum[k] = sum_c sigma exp(l(row_{k,c}) - l(x_c))                                        (fp64)
 * so that <P_k> ~ ratio_sum[k] / batch_size: the character of the state under a translation, a point-group element or
 * spin inversion.  sigma is the product of the two signs for the signed types (pbdg, fully_connected_nnb, ed_vector)
 * and 1 otherwise; a vanishing amplitude on either side gives exactly 0 (never NaN).  The rows go through the full
 * forward of the ctx's ansatz type (the device path of vmc_amplitude); the chains' own l and signs are the ctx's cache.
 * The ops run in passes of at most ops_per_pass ops (0: as many as the row budget of a pass takes; a request is clamped
 * to it); the sum of an op is added in one fixed order (chains c = l mod 64 ascending per lane l, then a butterfly over
 * the lanes) and does not depend on the passes or on the other ops of the call.  A pure measurement: chains, step counter,
 * accumulators, the Hamiltonian's bonds and the validity of the amplitude and activation caches are as before on return,
 * on a failed call too.  which outside {0, 1}, n_ops < 1, a NULL perm, ops_per_pass < 0, a perm_k that is no bijection
 * of 0 .. N - 1 (the message names the op and the entry; the rows of pbdg, fully_connected_nnb and ed_vector must stay
 * at Sz = 0) or a flip entry above 1: VMC_ERR_INVALID, before anything touches the device; an output activation other
 * than exp on an unsigned type and a product ctx: VMC_ERR_UNSUPPORTED; a factor of a product ctx: VMC_ERR_STATE. */
int vmc_symmetry_expectations(vmc_ctx* ctx, int which, int32_t n_ops, const int32_t* perm /*[n_ops][N]*/,
                              const uint8_t* flip /*[n_ops], 0/1; NULL: no flips*/,
                              int32_t ops_per_pass /*0: the library decides*/, double* ratio_sum /*[n_ops]*/);

/* Symmetry-projected energies -- EXTENSION with no reference counterpart.  The ops are those of
 * vmc_symmetry_expectations (same row convention, same bijection check); chi[s][k] are real characters of n_sectors
 * sectors.  Over the ctx's current chains, with r_{k,c} = sigma exp(l(row_{k,c}) - l(x_c)) formed as there and E_loc(c)
 * the local energy of chain c under the bonds of vmc_set_bonds (what vmc_local_energy gives):
 *   w_s(c)    = sum_k chi[s][k] r_{k,c}
 *   w_sum[s]  = sum_c w_s(c)          we_sum[s] = sum_c w_s(c) E_loc(c)          e_sum = sum_c E_loc(c)       (fp64)
 *   n_alive   = the number of chains whose own amplitude does not vanish
 * so that E_s ~ we_sum[s] / w_sum[s] is the energy of the projected state P_s psi, P_s = sum_k chi[s][k] g_k, its weight
 * in psi is ~ w_sum[s] / n_alive, and e_sum / n_alive is the unprojected energy.  A chain whose own amplitude vanishes
 * contributes exactly 0 to every sum; its E_loc is never read.
 * Validity: every g_k is a symmetry of the Hamiltonian -- CHECKED: each perm_k must map the bonds of
 * vmc_set_bonds onto themselves as a multiset, couplings compared by their bits; the global flip always is one -- the
 * characters are real with chi(g^-1) = chi(g), and P_s is a projector only if the ops form a group (neither is checked).
 * Determinism: w_s(c) is built by sequential fp64 fused multiply-adds in ascending k, carried across the passes, and
 * the chains are folded in vmc_symmetry_expectations' order (lane l the chains l, l + 64, ... ascending, then a butterfly).
 * Every output therefore depends on the chains, the ops and that sector's characters alone: not on ops_per_pass, not on
 * the other sectors of the call, not on how the sectors are tiled over workgroups, not on the grid.
 * A pure measurement like its four siblings: chains, step counter, accumulators, the Hamiltonian's bonds and the validity
 * of the amplitude and activation caches are as before on return, on a failed call too -- with one exception: it runs
 * one local-energy evaluation first, which leaves what vmc_local_energy(ctx, which, ...) leaves (the chains' local
 * energies of `which` on the device, vmc_last_connected_rows).
 * Refusals, all before anything touches the device, vmc_last_error naming the offender: everything
 * vmc_symmetry_expectations refuses, with its codes; n_sectors < 1, a NULL chi or a character that is not finite:
 * VMC_ERR_INVALID; n_sectors x batch_size beyond 2^26 doubles of accumulator: VMC_ERR_UNSUPPORTED; no bonds set:
 * VMC_ERR_STATE; an op that is no symmetry of the Hamiltonian: VMC_ERR_INVALID, the op and the first offending bond
 * named.  Outputs may be NULL. */
int vmc_projected_energy(vmc_ctx* ctx, int which, int32_t n_ops, const int32_t* perm /*[n_ops][N]*/,
                         const uint8_t* flip /*[n_ops], 0/1; NULL: no flips*/, int32_t n_sectors,
                         const double* chi /*[n_sectors][n_ops]*/, int32_t ops_per_pass /*0: the library decides*/,
                         double* w_sum /*[n_sectors]*/, double* we_sum /*[n_sectors]*/, double* e_sum /*[1]*/,
                         int64_t* n_alive /*[1]*/);

/* Lanczos-step energies: the local values of H and H^2 -- EXTENSION with no reference counterpart.  Over the ctx's
 * current chains x_c and the bonds of vmc_set_bonds, H = sum_b j_x[b] (S+S- + S-S+) / 2 + j_z[b] SzSz:
 *   e(c) = (H psi)(x_c) / psi(x_c)      what vmc_local_energy gives (fp32, widened)
 *   g(c) = (H^2 psi)(x_c) / psi(x_c)    = diag(x) e(x) + sum_{a anti on x} hx_a [ r(x^a) diag(x^a) + sum_{b anti on x^a} hx_b r(x^{ab}) ]
 * with hx_b = j_x[b] / 2, diag(y) = sum_b (j_z[b] / 4) y_i y_j, y^a = y with the sites of bond a exchanged and
 * r(y) = psi(y) / psi(x_c), always against the chain's own amplitude.  e(c) and the products hx_a r(x^a) are those of the
 * local-energy call this entry runs first (fp32); everything added on top is fp64.
 *   sums = { sum_c e, sum_c e^2, sum_c g, sum_c e g, sum_c g^2, the number of chains alive }            (fp64)
 * so that under |psi|^2 sampling h1 = <e>, h2 = <e^2> (= <g>), h3 = <e g>, h4 = <g^2> are the moments <H^n> a Lanczos
 * step psi + alpha H psi and the variance extrapolation need.  e_loc / h2_loc [batch_size] (optional) are e and g per
 * chain.  A chain whose own amplitude vanishes has e = g = 0, adds to no sum and is not alive.
 * The rows x^{ab} are a compacted list, chain-major, then a, then b ascending: b naming the site pair of a (a itself, a
 * twin bond) gives the term hx_a hx_b without a row; b disjoint from a gives one row for a < b alone, counted twice; b
 * sharing one site with a gives one row.  *n_rows2 is the length of that list; it goes through the ansatz type's own
 * full forward in passes of at most rows_per_pass rows (0: the library decides).
 * Determinism: every output is the same bits for every rows_per_pass -- a pass may end inside a chain's rows; row p of a
 * chain is added into lane p mod 64 of the chain's accumulator in ascending p, the lanes are folded by a fixed butterfly
 * and the chains are summed in strictly ascending order (csrc/moments.hip states every order).
 * A pure measurement like its siblings: chains, step counter, accumulators, the Hamiltonian's bonds and the validity of
 * the amplitude and activation caches are as before on return -- except what vmc_local_energy(ctx, which, ...) leaves
 * (the chains' local energies of `which` on the device, vmc_last_connected_rows).
 * Refusals, before anything is launched: a bad `which` or rows_per_pass < 0: VMC_ERR_INVALID; no bonds set:
 * VMC_ERR_STATE; an output activation other than exp on an unsigned type, a product ctx, or batch_size x n_bonds^2 beyond
 * the 32-bit row index: VMC_ERR_UNSUPPORTED; a factor of a product ctx: VMC_ERR_STATE.  Outputs may be NULL. */
int vmc_energy_moments(vmc_ctx* ctx, int which, int64_t rows_per_pass /*0: the library decides*/, double sums[6],
                       double* e_loc /*[batch_size] or NULL*/, double* h2_loc /*[batch_size] or NULL*/,
                       int64_t* n_rows2 /*[1]*/);

/* Four-spin (J-Q) terms of the Hamiltonian -- EXTENSION with no reference counterpart.  A term t = (i, j, k, l; q_t) with
 * four distinct sites adds
 *   -q_t (1/4 - S_i . S_j)(1/4 - S_k . S_l)
 * to the Hamiltonian of vmc_set_bonds.  With spins +-1 and r(y) = psi(y) / psi(x) its local value on a configuration x is
 *   e_t(x) = -(q_t / 4) [s_i != s_j][s_k != s_l] (1 - sigma r(swap_ij x) - sigma r(swap_kl x) + r(swap_kl swap_ij x))
 * where sigma = exchange_sign (+-1) is the sign the transverse part carries: +1 in the physical frame, -1 in the
 * sublattice-rotated frame that goes with j_x < 0 (the frame the positive exp-output states are trained in).
 * While terms are set every local energy of the ctx is that of H_J + H_Q: vmc_local_energy, the three modes of
 * vmc_accumulate, the fused epochs, vmc_evaluate (the _dist entries too) and the right-hand side of the SR store; the fold
 * of the local energies is then never deferred into the back-propagation launch, and a sampler launch behind an
 * accumulate waits for all of it.  vmc_local_energy_terms adds the 1 of every active bracket (times -q_t / 4) to diag and
 * the three ratio terms to offdiag_over_psi.
 * ijkl [n_terms][4], q [n_terms].  n_terms = 0 removes the terms: the ctx is then what it was before it took any.
 * Per evaluation: a compacted chain-major list -- per chain one single row for every distinct site pair of the terms
 * that is antiparallel on the chain (pairs ascending by (min, max) site), then one double row for every term with both
 * pairs antiparallel (terms ascending) -- goes through the ansatz type's own full forward in passes of at most
 * rows_per_pass rows (0: the library decides; a pass may end inside a chain's rows), and one fold per chain adds, in
 * fp64, per active term w = -q_t / 4, then fma(-sigma w, r_ij, .), fma(-sigma w, r_kl, .), fma(w, r_ijkl, .) -- lane l the
 * terms l, l + 64, ... ascending, then a fixed butterfly -- and rounds once to fp32 when the sum is added to the chain's
 * local energy: the same bits for every rows_per_pass, batch size and grid (csrc/fourspin.hip states every order).  A
 * chain whose own amplitude vanishes (ed_vector) keeps what the Heisenberg part gives it; a row at a vanishing amplitude
 * gives r = 0.
 * Everything is validated before anything is stored, and a failed call leaves the previous term set in place: a site out
 * of range or named twice in a term, a q that is not finite, an exchange_sign other than +-1, rows_per_pass < 0:
 * VMC_ERR_INVALID; more than 65,536 terms, more than 4,096 distinct site pairs, batch_size x (pairs + terms) beyond
 * 2^31 - 1, an output activation other than exp on an unsigned type, a product ctx, a symmetrized ctx:
 * VMC_ERR_UNSUPPORTED; a factor of a product ctx or the base of a symmetrized ctx: VMC_ERR_STATE.  vmc_create_product and
 * vmc_create_symmetrized refuse a ctx that holds terms, vmc_energy_moments and vmc_projected_energy refuse while terms
 * are set (VMC_ERR_UNSUPPORTED); the other measurements are measurements of the state and stay available. */
int vmc_set_four_spin_terms(vmc_ctx* ctx, int32_t n_terms, const int32_t* ijkl /*[n_terms][4]*/,
                            const float* q /*[n_terms]*/, int32_t exchange_sign /*+1 or -1*/,
                            int64_t rows_per_pass /*0: the library decides*/);
/* The lengths of the list of the last evaluation with terms set: its single rows and its double rows. */
int vmc_last_four_spin_rows(vmc_ctx* ctx, int64_t* single_rows, int64_t* double_rows);

/* Overlap with the frozen parameter set -- EXTENSION with no reference counterpart.  Over the ctx's current chains x_c,
 * drawn from |psi|^2, with r_c = omega(x_c) / psi(x_c):
 *   d_c = (logit_omega(c) - shift_omega) - (logit_psi(c) - shift_psi)      fp64, from the two fp32 amplitude caches
 *   s_c = sgn(omega(x_c)) sgn(psi(x_c))                                    1 on the unsigned types
 *   m   = max of d_c over the chains with s_c != 0 (0 when there is none)
 *   sums = { S1 = sum_c s_c exp(d_c - m), S2 = sum_c exp(2 (d_c - m)), alive, m }
 * so that r_c = s_c exp(d_c), the fidelity |<omega|psi>|^2 / (<psi|psi><omega|omega>) ~ S1^2 / (alive S2) whatever m is,
 * and sum_c r_c = exp(m) S1.  ratio [batch_size] (optional) receives s_c exp(d_c - m).  A chain whose own amplitude
 * vanishes is dead: its ratio is 0, it adds to no sum and is not alive.  A vanishing omega(x_c) gives a ratio of 0
 * exactly (its logarithm is never read); the chain stays alive.
 * Determinism: thread t of one workgroup of 256 adds the chains t, t + 256, ... in ascending order, the 256 partial
 * sums are folded by a fixed butterfly; the max is exact in any order.  The four outputs are the same bits from call to
 * call and for every launch grid (csrc/overlap.hip).
 * A pure measurement: chains, step counter, accumulators, the Hamiltonian's bonds and the validity of the amplitude and
 * activation caches are as before on return.
 * Refusals, before anything is launched: omega unset: VMC_ERR_STATE; an output activation other than exp on an
 * unsigned type, or a product ctx: VMC_ERR_UNSUPPORTED; a factor of a product ctx: VMC_ERR_STATE.  Outputs may be NULL. */
int vmc_overlap(vmc_ctx* ctx, double sums[4], double* ratio /*[batch_size] or NULL*/);

/* Stochastic reconfiguration -- EXTENSION: named by the north star, absent from the reference
 * (training.py has only the plain energy gradient + Adam), so these entries replace no reference
 * interface; they sit where TrainOpsTraditional.apply_gradients (training.py:560-567) sits.
 *   S = <O O^T> - <O><O>^T, f = <E O> - <E><O>, (S + diag_shift I) x = f, theta -= lr x
 * over every sample of the vmc_accumulate(ENERGY_GRADIENT) calls since the last reset.
 * vmc_sr_reserve(n) allocates the sample store for n accumulate calls (chains, activations,
 * back-propagated deltas: 2 L B Hp + B N floats each; convolutional types: the taped inputs and
 * deltas of every convolution, (2 n_conv - 1) B CS floats) and switches recording on; 0 frees it.
 * Covered: fully_connected and rbm (every width the library takes), the convolutional types; exp output.
 * Matrix-free conjugate gradients: vmc_sr_begin (x = 0, r = p = f from the accumulators, which
 * must already be all-reduced), then per iteration vmc_sr_matvec_partial (this rank's
 * sum_b (O_b . p) O_b into the P+1-float buffer of vmc_sr_buffer_devptr, last float =
 * sum_b O_b . p; SUM all-reduce it across ranks) and vmc_sr_cg_update (*rr = |r|^2 after the
 * step).  vmc_sr_solve runs the loop on one GPU until |r| <= tol |f| or max_iter.
 * vmc_sr_apply does theta -= lr x; *energy = TrainOps.metrics as in vmc_apply_adam. */
int vmc_sr_reserve(vmc_ctx* ctx, int32_t n_batches);
int vmc_sr_num_stored(vmc_ctx* ctx, int32_t* n);
int vmc_sr_begin(vmc_ctx* ctx, double* rr0);
int vmc_sr_matvec_partial(vmc_ctx* ctx);
/* The same matvec in two phases, for every path (required on the general convolution path, kernel path 6, whose
 * per-sample weights O_b . p are centred on their mean over ALL ranks; elsewhere phase 1 does nothing and phase 2 is
 * vmc_sr_matvec_partial): phase 1 leaves sum_b O_b . p of this rank's samples in the buffer's last float (the rest
 * zero); SUM all-reduce that float across ranks; phase 2 fills the buffer as vmc_sr_matvec_partial does.  Then the
 * all-reduce of the whole buffer and vmc_sr_cg_update as above.  (An extension like all of SR: no reference line.) */
int vmc_sr_matvec_phase1(vmc_ctx* ctx);
int vmc_sr_matvec_phase2(vmc_ctx* ctx);
int vmc_sr_buffer_devptr(vmc_ctx* ctx, void** dev_ptr, int64_t* n_floats);
int vmc_sr_get_buffer(vmc_ctx* ctx, float* host /*[P+1]*/);   /* host staging (non-RCCL backends) */
int vmc_sr_set_buffer(vmc_ctx* ctx, const float* host /*[P+1]*/);
int vmc_sr_cg_update(vmc_ctx* ctx, float diag_shift, double* rr);
int vmc_sr_solve(vmc_ctx* ctx, float diag_shift, float tol, int32_t max_iter, int32_t* iters,
                 double* rel_residual);
/* vmc_sr_solve with the stored samples sharded over ranks: the P+1-float all-reduce of every CG
 * iteration is issued in stream (transport as above); every rank runs the identical recurrence.
 * The accumulators must already be all-reduced. */
int vmc_sr_solve_dist(vmc_ctx* ctx, void* nccl_comm, int32_t world_size, float diag_shift, float tol,
                      int32_t max_iter, int32_t* iters, double* rel_residual);
/* The same update from the sample space (MinSR): with n stored samples, Obar = O - 1 obar^T and eps_b = E_b - Ebar,
 *   x = Obar^T (Obar Obar^T + n diag_shift I)^-1 eps
 * -- the solution of vmc_sr_solve, from an n x n system.  The Gram matrix T = O O^T is formed once from the dense sample
 * store (per layer two MFMA Gram products joined by a Hadamard product, never O itself); conjugate gradients on
 * C T C + n diag_shift I (C v = v - mean(v)) run until |r| <= tol |eps| or max_iter, each iteration one n x n
 * matrix-vector product whatever the number of parameters; x = sum_b t_b O_b, t = y - ybar, goes where vmc_sr_solve
 * leaves its solution: vmc_sr_get_solution and vmc_sr_apply follow as after vmc_sr_solve.  eps reads the local
 * energies recorded with the store, not the accumulators.  One rank only.  eps = 0 gives *iters = 0 and x = 0.
 * Refusals, before anything is launched: diag_shift <= 0 or not finite (the centred Gram matrix alone is singular),
 * tol < 0 or max_iter < 0: VMC_ERR_INVALID; no store or nothing recorded: VMC_ERR_STATE; a convolutional type (its
 * store has no per-layer Gram form) or more than 16,384 stored samples (T is n^2 floats): VMC_ERR_UNSUPPORTED -- use
 * vmc_sr_solve; a product ctx or a factor of one: as every vmc_sr_* entry. */
int vmc_sr_solve_samples(vmc_ctx* ctx, float diag_shift, float tol, int32_t max_iter, int32_t* iters,
                         double* rel_residual);
/* test hook: the uncentred Gram matrix T = O O^T of the stored samples, *n = their number (T_host NULL: *n alone);
 * refuses what vmc_sr_solve_samples refuses of the store */
int vmc_sr_debug_gram(vmc_ctx* ctx, float* T_host /*[n][n]*/, int32_t* n);
int vmc_sr_get_solution(vmc_ctx* ctx, float* x /*[P]*/);
int vmc_sr_apply(vmc_ctx* ctx, float lr, double* energy);
/* test hook: out = (S + diag_shift I) v over the stored samples (single rank) */
int vmc_sr_debug_matvec(vmc_ctx* ctx, const float* v /*[P]*/, float diag_shift, float* out);

/* Wavefunction.update_norm (wavefunctions.py:261-288) on psi(chains). */
int vmc_update_norm(vmc_ctx* ctx, float max_value);

/* Per-kernel HIP-event timing on the ctx's stream (bench.py's roofline leg).  on = 1 times
 * every region, on = 2 only "sweep" and "tail_eloc" (each recorded event drains the pipeline
 * between two kernels, ~3.5 us: ten of them per step cost 1.8 % of the step they measure).
 * names: "sweep", "tail_eloc", "tail_amp", "z1", "bond_list", "eloc_reduce", "grad",
 * "adam", "sr_matvec".  ms = summed elapsed, launches = number of timed launches. */
int vmc_timing_enable(vmc_ctx* ctx, int on);
int vmc_timing_reset(vmc_ctx* ctx);
int vmc_timing_get(vmc_ctx* ctx, const char* name, double* ms, int64_t* launches);
/* rows the last local-energy call actually evaluated (antiparallel bonds) */
int vmc_last_connected_rows(vmc_ctx* ctx, int64_t* rows);
/* Diagnostic: which kernel family serves this ctx.  0: fused, register-resident rows (<= 256 hidden
 * units); 1: fused, LDS-operand rows (257 .. 512 units); 2: general multi-launch path (> 512 units,
 * or CGS_VMC_WIDE_FAST=0); 3: convolutional kernels; 4: the 3 x bf16 split experiment of the row kernel
 * (CGS_VMC_SPLIT_BF16=1: fully_connected, relu, 193 .. 256 units; fp32 results from the bf16 matrix cores,
 * cgs_vmc_amd/csrc/tail_split.hip -- never the headline configuration); 5: the split sampler as well; 6: the
 * general convolution path; 7: the projected BCS determinant kernels of pbdg (cgs_vmc_amd/csrc/pbdg.hip); 8: neural-network backflow -- the
 * general dense path into the determinant rows of cgs_vmc_amd/csrc/nnb.hip; 9: the Lin-table state vector
 * of ed_vector (cgs_vmc_amd/csrc/edvec.hip); 10: a product ctx (cgs_vmc_amd/csrc/prod.hip over the factors' own kernels). */
int vmc_debug_kernel_path(vmc_ctx* ctx, int32_t* path);
/* Chains per workgroup of the fused dense sampler: 16 (k_sweep16, sweep16.hpp) or 8 (k_sweep8, sweep8.hip: chosen by
 * vmc_create when sixteen-chain tiles would occupy at most half of the CUs -- BASELINE configs 2 and 5 -- or by
 * CGS_VMC_SWEEP_TILE=8|16).  Both kernels implement graph_builders.py:38-89 and produce the same chains bit for bit.
 * set = 0 queries, 8 / 16 switches (test hook; 8 is refused where no k_sweep8 exists for the shape). */
int vmc_debug_sweep_tile(vmc_ctx* ctx, int32_t set, int32_t* chains);
/* Would vmc_mc_steps(n_steps) run the patch sampler of the general convolution path (k_cgen_patch_sweep,
 * cgs_vmc_amd/csrc/conv_patch.hip)?  It recomputes, per step, only the two boxes of every convolution that the exchanged
 * pair of graph_builders.py:67-71 reaches through layers.py:118-160's taps -- the four convolutional ansatz types at <= 16
 * filters on a lattice wider than the last box, launches of >= 8 steps; CGS_VMC_CONV_PATCH=0 never, =2 wherever the shape
 * allows -- and gives the chains of the full-forward sampler bit for bit.  *patch: 1 / 0.
 * The local energies' connected configurations (operators.py:162-169) run through the same kernel's second form.
 * vmc_create sends a convolutional shape that the fused kernels would take to the general path (vmc_debug_kernel_path 6)
 * when these kernels beat them: the boxes of all convolutions at most a fifth of the lattice x convolutions (e.g. 20 x 20
 * sites, 3 x 16 filters 3 x 3).  CGS_VMC_CONV_GENERAL=0 keeps the fused kernels there (their gradient and stochastic-
 * reconfiguration kernels are the faster ones: a solve over many stored samples may prefer them). */
int vmc_debug_conv_patch(vmc_ctx* ctx, int64_t n_steps, int32_t* patch);
int vmc_synchronize(vmc_ctx* ctx);

/* Test hook: C[M,N] = op(A) op(B) through the library's fp32 MFMA GEMM
 * (A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]; host buffers). */
int vmc_debug_gemm(vmc_ctx* ctx, int32_t M, int32_t N, int32_t K, const float* A, int64_t sam,
                   int64_t sak, int64_t a_len, const float* B, int64_t sbk, int64_t sbn,
                   int64_t b_len, float* C);

#ifdef __cplusplus
}
#endif
#endif /* CGSVMC_H_ */
