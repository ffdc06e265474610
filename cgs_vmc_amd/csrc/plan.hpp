// plan.hpp -- every PURE-HOST decision of libcgsvmc_hip.so in one header with no HIP in it: parameter
// layouts, vmc_create's shape / LDS validation and the kernel path of the ctx (enum KernelPath with its
// predicates; plan_desc and plan_split_path decide it), the convolution group / band / slice pickers, the
// sampler's LDS plan and kernel-variant choice, split-K and the XCD-aware block order of the
// weight-gradient GEMM, the stochastic-reconfiguration tile schedules, and the sizes of the buffers
// they index.  The .hip files call these functions (there is no second copy of any formula); the same
// header is compiled by g++ -fsanitize=address,undefined into hostcheck.cpp, which walks a grid of
// shapes on the CPU and asserts that every offset, grid and LDS figure is in range
// (`make -C cgs_vmc_amd/csrc hostcheck`, tests/test_hostcheck.py; SURVEY.md 5 "sanitizers").
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/cgsvmc.h"

#if defined(__HIPCC__)
#define PLAN_HD __host__ __device__
#else
#define PLAN_HD
#endif

#define PLAN_LDS_PER_CU ((size_t)160 * 1024)   // gfx950: 160 KiB of LDS per CU

// ------------------------------------------------------------------------------- dense parameter layout
// offsets of the pieces of the flat parameter vector (both dense ansatz types; include/cgsvmc.h)
struct ParamLayout {
  long long off_w1, off_b1;   // first layer [N,H], [H]
  long long off_h0;           // first H x H layer; layer l at off_h0 + l (H*H + H): w then b
  long long off_wout, off_bout;  // FC: w_out [H], b_out;  RBM: off_wout = -1, off_bout = b_on
  long long off_won;          // RBM: onsite weights [N]; FC: -1
  int n_hh;                   // number of H x H layers (FC: L-1, RBM: L)
};

inline ParamLayout plan_layout(bool rbm, long long N, long long H, long long L) {
  ParamLayout lay;
  if (rbm) {   // w_on[N] b_on | w_1 b_1 | (w b) x L        (see include/cgsvmc.h)
    lay.off_won = 0; lay.off_bout = N; lay.off_wout = -1;
    lay.off_w1 = N + 1; lay.off_b1 = lay.off_w1 + N * H; lay.off_h0 = lay.off_b1 + H;
    lay.n_hh = (int)L;
  } else {     // w_1 b_1 | (w b) x (L-1) | w_out b_out
    lay.off_w1 = 0; lay.off_b1 = N * H; lay.off_h0 = lay.off_b1 + H;
    lay.n_hh = (int)L - 1;
    lay.off_wout = lay.off_h0 + (L - 1) * (H * H + H); lay.off_bout = lay.off_wout + H;
    lay.off_won = -1;
  }
  return lay;
}

// weight matrix / bias of layer l (0 = first layer, 1 .. n_hh = the H x H layers)
inline long long plan_off_w(const ParamLayout& lay, long long H, int l) {
  return l == 0 ? lay.off_w1 : lay.off_h0 + (long long)(l - 1) * (H * H + H);
}
inline long long plan_off_b(const ParamLayout& lay, long long H, int l) {
  return l == 0 ? lay.off_b1 : plan_off_w(lay, H, l) + H * H;
}

inline long long plan_num_params_dense(int ansatz, long long N, long long H, long long L) {
  if (ansatz == VMC_ANSATZ_PBDG) return N * N;        // the pairing matrix F[N][N] (plan_pbdg_*)
  if (ansatz == VMC_ANSATZ_ED_VECTOR) return H;       // the state vector; layer_size carries its length (plan_edvec_*)
  if (ansatz == VMC_ANSATZ_NNB) return N * H + H + (L - 1) * (H * H + H) + H * N * N + N * N;   // trunk + pairing layer
  if (ansatz == VMC_ANSATZ_RBM) return N + 1 + N * H + H + L * (H * H + H);
  return N * H + H + (L - 1) * (H * H + H) + H + 1;
}

inline long long plan_num_params_conv(int n_conv, long long F, long long taps) {
  return taps * F + F + (long long)(n_conv - 1) * (taps * F * F + F);
}

// ------------------------------------------------------------------------------- convolutional geometry
#define CONV_MAX_LAYERS 32
#define CONV_FP 16          // channel tile of the MFMA: filters are zero padded to NCB blocks of 16
#define CONV_MAX_NCB 4      // num_conv_filters <= 64
#define CONV_GENERAL_MAX_K 31   // general path (conv_general.hip): any kernel size the periodic padding allows, bounded for the index arithmetic
#define CONV_GENERAL_MAX_F 1024
#define PLAN_GNN_MAX_K 64       // gnn: neighbours per position
#define PLAN_GNN_MAX_SITES (1023 * 1023)
#define CONV_MAX_K 9        // kernel_size (one instantiation per size; weights of a block pair in register-resident chunks of <= 25 taps)
#define CONV_LDS_PER_WG ((size_t)80 * 1024)   // two 4-wave workgroups share the 160 KiB of a CU

// Geometry of one network.  A feature map of one sample is stored -- in LDS and in the HBM tapes
// alike -- channel-group major: [4 NCB groups][GS dwords], element (site, channel c) at
// (c / 4) * GS + 4 * site + c % 4, with GS >= 4 N a multiple of 64 dwords so that the 16-lane
// groups of ds_read_b128 / ds_write_b128 fall on distinct banks; NCB = ceil(F / 16) channel blocks
// of one MFMA tile each, CS = 4 NCB GS dwords per sample.
struct ConvGeom {
  int K;        // kernel_size
  int D1, D2;   // size_x, size_y: inputs are reshaped to [-1, size_x, size_y, 1] (wavefunctions.py:596)
  int N;        // D1 * D2
  int F;        // num_conv_filters
  int n_conv;   // number of Conv2dPeriodic modules: num_conv_layers, or 1 + 2 num_resnet_blocks
  int resnet;   // 0: Conv2DNetwork, 1: ResNet2D
  int hact;     // hidden activation id of Conv2DNetwork (ResNet2D: selu, layers.py:226)
  int GS;       // dwords per channel group of a feature map (see above)
  int lo, hi;   // periodic padding in front / behind along axis 1: (K-1)/2 and K/2 (layers.py:132-141);
                // the 1-D modules pad K/2 in front and K-1-K/2 behind (layers.py:66-72)
  int KW;       // taps along axis 2: K (Conv2dPeriodic) or 1 (Conv1dPeriodic on an [N, 1] lattice)
  int lo2, hi2; // the same padding for axis 2 (0 for the 1-D modules)
  int NCB;      // channel blocks of 16: (F + 15) / 16
  int CS;       // dwords of one sample's feature map: 4 * NCB * GS
  int graph;    // 1: gnn -- the taps come from an adjacency list adj[N][KW] (K = D1 = 1, D2 = N, no padding), not from
                // the periodic lattice; every route that derives a tap's site from (D1, D2, lo, lo2) must refuse it
};

// LDS of a row / sampler / backward workgroup holding G samples: buf0, buf1, xs, pinfo, row_chain,
// red + the sampler's cur_logit, prop, prop_u + the two wrap tables
// ints per row of the periodic neighbour tables (one entry per tap along an axis)
// general path: row stride (floats) of the im2col matrix = taps x input channels of the widest convolution, 16-byte rows
PLAN_HD inline int plan_cgen_lda(const ConvGeom& g) { return (g.K * g.KW * (g.n_conv > 1 ? g.F : 1) + 3) & ~3; }
PLAN_HD inline int plan_conv_tab(const ConvGeom& g) { return g.K <= 8 ? 8 : 16; }
// general path at <= 16 filters: k_cgen_band (conv_band.hip) stages bands of lattice rows with their periodic halo,
// (rows + K - 1) x (D2 + KW - 1) sites x 16 channels, in LDS; rows per band = as many as keep a band within
// PLAN_CGEN_BAND_LDS bytes (several workgroups per CU); < 1: the lattice is too wide for a band
#define PLAN_CGEN_BAND_LDS (40 * 1024)
#define PLAN_CGEN_BAND_LDS_WIDE (144 * 1024)
#define PLAN_CGEN_BAND_MAX_FRAGS 208      // weight fragments (registers) of one output block: K KW 4 NCB
inline int plan_cgen_band_ncb(const ConvGeom& g) { return (g.F + 15) / 16; }
inline int plan_cgen_band_rows(const ConvGeom& g) {
  const long long per_row = (long long)(g.D2 + g.KW - 1) * 16 * plan_cgen_band_ncb(g) * (long long)sizeof(float);
  // one block: 40 KB (several workgroups per CU); more: one workgroup per CU stages a band for all of its output blocks, up to 144 KB
  long long bh = (plan_cgen_band_ncb(g) > 1 ? PLAN_CGEN_BAND_LDS_WIDE : PLAN_CGEN_BAND_LDS) / per_row - (g.K - 1);
  if (bh > g.D1) bh = g.D1;
  return (int)bh;
}
// rows per band of ONE launch over `rows` row configurations on a chip that holds `capacity` workgroups: few rows (the
// sampler's B candidates at a small batch) take thinner bands, so that every CU has an item -- a launch's latency is an
// item's; many rows (the local energies) take the widest band (least halo re-read)
inline int plan_cgen_band_rows_for(const ConvGeom& g, long long rows, long long capacity) {
  const int bh_max = plan_cgen_band_rows(g);
  if (bh_max < 1 || rows < 1) return bh_max;
  const long long nb_max = (g.D1 + bh_max - 1) / bh_max;
  if (rows * nb_max >= capacity) return bh_max;
  long long nb = (capacity + rows - 1) / rows;
  if (nb > g.D1) nb = g.D1;
  long long bh = (g.D1 + nb - 1) / nb;
  if (bh < 1) bh = 1;
  return (int)(bh < bh_max ? bh : bh_max);
}
// the shapes k_cgen_band takes: up to 64 filters (four channel blocks of 16) as long as one output block's fragments
// against every input block fit the registers (3 x 3: 64 filters; 4 x 4: 48; 5 x 5: 32; 7 x 7: 16), 2 .. 7 taps per
// axis (2-D: K x K; 1-D: K x 1), a band of at least one lattice row within the LDS budget
inline bool plan_cgen_band_ok(const ConvGeom& g) {
  if (g.graph) return false;          // (its bands are stretches of the periodic lattice)
  if (g.F < 1 || g.F > 64 || g.K < 2 || g.K > 7) return false;
  if (!(g.KW == g.K || g.KW == 1)) return false;
  if (g.K * g.KW * 4 * plan_cgen_band_ncb(g) > PLAN_CGEN_BAND_MAX_FRAGS) return false;
  return plan_cgen_band_rows(g) >= 1;
}
// Chain groups of the general convolution sampler (run_sweep_cgen: a step of each group on a stream of its own).  Two
// groups where a launch over the whole batch leaves CUs idle that the next launch of the other group can use: the GEMM
// form with more than one round of 128-position row tiles whose last round is less than 0.9 full (1,024 chains on a
// 10 x 10 lattice: 800 tiles on 256 CUs, 3.125 rounds paid as 4), and the one-workgroup-per-CU band kernel from one
// round of positions on (its tail: measured, 36 x 36 x 64 filters at 32 chains: 161 -> 151 ms per sweep).  One group where
// the launches are latency (36 x 36 x 16 filters at 32 chains: 68 -> 73 ms with two, 214 with four -- the host's launch rate).
inline int plan_cgen_sweep_groups(const ConvGeom& g, long long B, int num_cus) {
  if (B < 2 || num_cus < 1) return 1;
  const long long positions = B * g.N;
  if (plan_cgen_band_ok(g)) return (plan_cgen_band_ncb(g) > 1 && positions >= 128LL * num_cus) ? 2 : 1;
  const long long tiles = ((positions + 127) / 128) * ((g.F + 127) / 128);
  if (tiles <= num_cus) return 1;
  const long long rounds = (tiles + num_cus - 1) / num_cus;
  return tiles * 10 < rounds * num_cus * 9 ? 2 : 1;
}
// The patch sampler of the general convolution path (k_cgen_patch_sweep, conv_patch.hip): an exchange negates two spins,
// and convolution l's output changes only in a box of (l + 1)(K - 1) + 1 sites per axis around each of them (the union of
// the taps' reach: graph_builders.py:67-71 proposes, layers.py:118-160 convolves).  One workgroup per chain keeps the
// chain's maps of every convolution in HBM and recomputes the two boxes per convolution instead of the lattice.
// Shapes: Conv2DNetwork / Conv1DNetwork / ResNet2D / ResNet1D, the band kernel's single-block shapes (<= 16 filters, so that a box
// value has k_cgen_band's bits), at least two convolutions, the last box within the lattice along both axes (it must not
// meet itself around the torus), and the LDS within a CU's.
inline int plan_cgen_patch_side(const ConvGeom& g, int l, int axis) { return (l + 1) * ((axis ? g.KW : g.K) - 1) + 1; }
inline size_t plan_cgen_patch_lds_bytes(const ConvGeom& g) {
  const int L = g.n_conv, T = g.K * g.KW;
  size_t fl = (size_t)((g.N + 3) & ~3);                           // the chain's spins
  fl += (size_t)(L - 1) * T * 256;                                 // weight fragments of the convolutions behind the first
  fl += (size_t)L * 16;                                            // biases
  size_t win = (size_t)(plan_cgen_patch_side(g, 0, 0) + g.K - 1) * (size_t)(plan_cgen_patch_side(g, 0, 1) + g.KW - 1);   // first: 1 channel
  for (int l = 0; l < L; ++l) {
    fl += 2 * (size_t)plan_cgen_patch_side(g, l, 0) * plan_cgen_patch_side(g, l, 1) * 16;          // the two boxes of convolution l
    if (l > 0) {
      const size_t w = (size_t)(plan_cgen_patch_side(g, l, 0) + g.K - 1) * (size_t)(plan_cgen_patch_side(g, l, 1) + g.KW - 1) * 16;
      if (w > win) win = w;
    }
  }
  fl += 2 * win;                                                   // the two staged input windows
  fl += (size_t)((g.N + 7) / 8 * 4);                               // 16-bit marks of the sites inside the last convolution's boxes
  fl += (size_t)((g.N + 3) & ~3);                                  // the next step's site uniforms
  return fl * sizeof(float) + 256;                                 // + the step's scalars
}
#define PLAN_CGEN_PATCH_LDS (156 * 1024)
inline bool plan_cgen_patch_ok(const ConvGeom& g, long long B) {
  if (g.graph) return false;          // (its boxes are rectangles of the periodic lattice)
  if (g.n_conv < 2 || g.n_conv > 9 || g.F > 16 || !plan_cgen_band_ok(g)) return false;       // (residual networks: 1 + 2 blocks convolutions)
  if (plan_cgen_patch_side(g, g.n_conv - 1, 0) > g.D1 || plan_cgen_patch_side(g, g.n_conv - 1, 1) > g.D2) return false;
  if (g.N > 16384 || B < 1) return false;
  if ((long long)g.n_conv * B * g.N * ((g.F + 3) & ~3) * (long long)sizeof(float) > (4LL << 30)) return false;   // the chains' maps
  return plan_cgen_patch_lds_bytes(g) <= PLAN_CGEN_PATCH_LDS;
}
// ... and where it pays: the boxes of the last convolution cover at most half of the lattice
inline bool plan_cgen_patch_pays(const ConvGeom& g) {
  return 4LL * plan_cgen_patch_side(g, g.n_conv - 1, 0) * plan_cgen_patch_side(g, g.n_conv - 1, 1) <= g.N;
}
// ... and where they beat the FUSED kernels (whose maps never leave the LDS): the boxes of all convolutions together at most
// a fifth of the positions a forward computes.  Whole steps at 256 chains, fused -> general path with the patch kernels:
// 24 x 24, 2 x 16 filters 5 x 5 (18 %): 36.2 -> 19.8 ms; 20 x 20, 3 x 16 filters 3 x 3 (14 %): 17.6 -> 13.6 ms.  plan_desc sends
// such a shape to the general path although the fused kernels would take it (CGS_VMC_CONV_GENERAL=0: not by preference).
inline bool plan_cgen_patch_routes(const ConvGeom& g, long long B) {
  if (g.resnet || !plan_cgen_patch_ok(g, B) || !plan_cgen_patch_pays(g)) return false;      // (residual networks: not measured against their fused kernels)
  long long boxes = 0;
  for (int l = 0; l < g.n_conv; ++l) boxes += 2LL * plan_cgen_patch_side(g, l, 0) * plan_cgen_patch_side(g, l, 1);
  return 5 * boxes <= (long long)g.n_conv * g.N;
}
// The routes of the general path whose gathers compute a tap's site from the periodic lattice -- the band kernel and
// its first-convolution form (k_cgen_band, k_cgen_first_direct), the patch kernels, the implicit A-operand gather of
// k_gemm_ring (GemmArgs.conv_a) -- take only these geometries; a graph (gnn) runs the table-driven im2col + GEMM form.
// (With K = D1 = 1 a graph's shape alone would pass some of their checks and give wrong answers.)
PLAN_HD inline bool plan_cgen_periodic(const ConvGeom& g) { return g.graph == 0; }
// k_cgen_first_direct (conv_band.hip): spins [N], weights [taps][Fp], bias [Fp], neighbour table [N][taps]
inline size_t plan_cgen_first_direct_lds_bytes(const ConvGeom& g) {
  const size_t fp = (size_t)((g.F + 3) & ~3), t = (size_t)g.K * g.KW;
  return sizeof(float) * ((size_t)((g.N + 3) & ~3) + t * fp + fp + (size_t)g.N * t);
}
inline size_t plan_cgen_band_lds_bytes(const ConvGeom& g, bool first, int band_rows = 0) {
  const int bh = band_rows > 0 ? band_rows : plan_cgen_band_rows(g);
  return (size_t)(bh + g.K - 1) * (size_t)(g.D2 + g.KW - 1) * (first ? 1 : 16 * (size_t)plan_cgen_band_ncb(g)) * sizeof(float);
}
inline size_t plan_conv_rows_lds(const ConvGeom& g, int G) {
  const size_t xs = (size_t)((g.N + 3) & ~3);
  return ((size_t)G * 2 * g.CS + (size_t)G * xs + (size_t)G * g.N + (size_t)G * 7 + 2 * (size_t)plan_conv_tab(g) * (size_t)(g.D1 + g.D2) + 16) * sizeof(float);
}

// LDS budget of one workgroup: half a CU when a sample's feature maps allow two workgroups per CU
inline size_t plan_conv_lds_cap(const ConvGeom& g, bool one_wg_per_cu = false) {
  if (one_wg_per_cu || g.NCB > 1) return PLAN_LDS_PER_CU;      // one 8-wave workgroup per CU (conv_wide.hpp)
  return plan_conv_rows_lds(g, 1) <= CONV_LDS_PER_WG ? CONV_LDS_PER_WG : PLAN_LDS_PER_CU;
}

inline int plan_conv_waves(const ConvGeom& g) { return g.NCB > 1 ? 8 : 4; }

// samples per pass of the row / backward kernels: the group size (<= 64, LDS within the cap) whose
// position tiles divide most evenly over the waves; ties go to the larger group
inline int plan_conv_pick_group(const ConvGeom& g, int waves, bool one_wg_per_cu = false) {
  int best = 1; double best_eff = -1.0;
  for (int G = 1; G <= 64; ++G) {
    if (plan_conv_rows_lds(g, G) > plan_conv_lds_cap(g, one_wg_per_cu)) break;
    const int tiles = (G * g.N + 15) / 16;
    const int rounds = (tiles + waves - 1) / waves;
    const double eff = (double)G * g.N / 16.0 / ((double)rounds * waves);
    if (eff >= best_eff - 1e-9) { best = G; best_eff = eff; }
  }
  return best;
}

// sampler: chains per workgroup that minimise (workgroups per CU) x (tile rounds of one forward pass) --
// the MFMA time of the busiest CU per mc_step.  The two-channel-block kernels walk their tiles in
// pairs.  Ties go to the group size that fills the last round of workgroups best (4096 chains, 32
// filters on 10 x 10: G = 4 -> 1024 workgroups = 4 per CU measured 84.9 ms per sweep, G = 5 -> 820
// workgroups 87.8 ms), then to the larger group.
inline int plan_conv_pick_sweep_group(const ConvGeom& g, long long B, int num_cus, int waves,
                                      bool one_wg_per_cu = false) {
  long long best_cost = -1;
  double best_fill = 0.0;
  int best = 1;
  for (int G = 1; G <= 64 && plan_conv_rows_lds(g, G) <= plan_conv_lds_cap(g, one_wg_per_cu) && G <= B; ++G) {
    const long long wgs = (B + G - 1) / G, per_cu = (wgs + num_cus - 1) / num_cus;
    long long tiles = ((long long)G * g.N + 15) / 16;
    if (g.NCB > 1) tiles = (tiles + 1) / 2;          // tile pairs
    const long long tile_rounds = (tiles + waves - 1) / waves;
    const long long cost = per_cu * tile_rounds;
    const double fill = (double)wgs / (double)(per_cu * num_cus);
    if (best_cost < 0 || cost < best_cost || (cost == best_cost && fill >= best_fill - 1e-9)) {
      best_cost = cost; best_fill = fill; best = G;
    }
  }
  return best;
}

// persistent grids of the row / backward / SR row-dot kernels: one workgroup per resident slot
inline int plan_conv_grid(const ConvGeom& g, long long n_rows, int G, int num_cus) {
  const long long groups = (n_rows + G - 1) / G;
  const long long slots = (long long)num_cus * ((g.NCB == 1 && plan_conv_rows_lds(g, G) <= CONV_LDS_PER_WG) ? 2 : 1);
  return (int)(groups < slots ? groups : slots);
}

// LDS of the weight-gradient kernel for bands of `rows` lattice rows: delta [NQ][CW] + input
// [NIN][CW] in one padded site numbering, the halo and position maps, ones (+ 8 sites: the operands
// of the quad past the end are read, and dropped)
// k_conv_dw keeps (items per wave) x (input blocks) x (output blocks) accumulator pairs in registers
// (items of a layer: the taps and the bias, over PLAN_DW_WAVES waves): at most PLAN_DW_MAX_ACC of them.
// A workgroup therefore takes NCO of the NCB output channel blocks (all of them when that fits with at most
// two blocks, else one) and one of NTP parts of the items; grid z = (NCB / NCO) * NTP.
#define PLAN_DW_WAVES 8
#define PLAN_DW_MAX_ACC 24
PLAN_HD constexpr int plan_conv_dw_nco(int K, int KW, int NCB) {
  return (NCB <= 2 && ((K * KW + 1 + PLAN_DW_WAVES - 1) / PLAN_DW_WAVES) * NCB * NCB <= PLAN_DW_MAX_ACC) ? NCB : 1;
}
PLAN_HD constexpr int plan_conv_dw_parts(int K, int KW, int NCB) {
  const int nco = plan_conv_dw_nco(K, KW, NCB), ni = K * KW + 1;
  int p = 1;
  while (((ni + PLAN_DW_WAVES * p - 1) / (PLAN_DW_WAVES * p)) * NCB * nco > PLAN_DW_MAX_ACC) ++p;
  return p;
}
inline int plan_conv_dw_nco(const ConvGeom& g) { return plan_conv_dw_nco(g.K, g.KW, g.NCB); }
inline int plan_conv_dw_grid_z(const ConvGeom& g) {
  return (g.NCB / plan_conv_dw_nco(g)) * plan_conv_dw_parts(g.K, g.KW, g.NCB);
}
inline size_t plan_conv_dw_lds(const ConvGeom& g, int rows) {
  const size_t d2p = (size_t)g.D2 + g.KW - 1, npad = (size_t)(g.D1 + g.K - 1) * d2p;
  const size_t nq = ((size_t)rows * d2p + 3) & ~(size_t)3, nin = nq + (size_t)(g.K - 1) * d2p + g.KW;
  const size_t cw = 16 * (size_t)g.NCB, cwd = 16 * (size_t)plan_conv_dw_nco(g);
  return (nq * cwd + nin * cw + npad + g.N + cw + 8 * cw) * sizeof(float);
}

// rows per band: the whole sample when it fits the CU's LDS, else the largest band that does
// (`forced` >= 1: the test knob CGS_VMC_CONV_DW_BAND); 0 when not even one row fits
inline int plan_conv_dw_band(const ConvGeom& g, int forced = 0) {
  int rows = g.D1;
  if (forced >= 1 && forced < rows) rows = forced;
  while (rows > 1 && plan_conv_dw_lds(g, rows) > PLAN_LDS_PER_CU) --rows;
  return plan_conv_dw_lds(g, rows) <= PLAN_LDS_PER_CU ? rows : 0;
}

// sample slices of the weight-gradient kernel: two resident workgroups per CU (NCB = 1) over the
// layers > 0, whose workgroups carry the work
inline int plan_conv_dw_slices(const ConvGeom& g, long long B, int num_cus) {
  const int per_cu = g.NCB == 1 ? 2 : 1;
  const int heavy = (g.n_conv > 1 ? g.n_conv - 1 : 1) * plan_conv_dw_grid_z(g);
  int sl = (per_cu * num_cus + heavy - 1) / heavy;
  sl = sl < 64 ? 64 : (sl > 256 ? 256 : sl);
  return B < sl ? (int)B : sl;
}

// floats of the weight-gradient workspace [slices][n_conv][2][(taps * 16 NCB + 1) * 16 NCB]
inline long long plan_conv_dw_ws_floats(const ConvGeom& g, int slices) {
  const long long KK = (long long)g.K * g.KW, cw = 16LL * g.NCB;
  return (long long)slices * g.n_conv * 2 * (KK * cw + 1) * cw;
}

// floats of the packed images of one parameter set: w0, wf / wb (each), bias
inline long long plan_conv_w0_floats(const ConvGeom& g) { return (long long)g.NCB * (((long long)g.K * g.KW + 3) / 4) * 64; }
inline long long plan_conv_wf_floats(const ConvGeom& g) {
  const long long nl = g.n_conv > 1 ? g.n_conv - 1 : 1;
  return nl * g.NCB * g.NCB * (long long)g.K * g.KW * 256;
}
inline long long plan_conv_bias_floats(const ConvGeom& g) { return (long long)g.n_conv * 16 * g.NCB; }

// ------------------------------------------------------------------------------- fused dense kernels
// LDS of the sampler k_sweep16 (16 chains per workgroup): spins, one or two z1 images, two operand
// buffers, chain scalars, biases, [W1 itself when w1l], [the Philox hand-over area]
// split_operands: the 3 x bf16 split sampler's operand buffers ([8 k-steps][3 terms][64][4] dwords each)
inline size_t plan_sweep_lds_bytes(int N, int Hp, int n_hidden, bool w1l, bool rbm, int uh_floats = 0, bool split_operands = false) {
  const int Nst = (N + 3) & ~3, NT = Hp / 16, ZS = Hp + 4;
  const size_t xb = split_operands ? (size_t)8 * 3 * 256 : (size_t)NT * 256;
  return sizeof(float) * ((size_t)16 * Nst + (size_t)(w1l ? 1 : 2) * 16 * ZS + (size_t)2 * xb + 16 +
                          16 + 7 * 16 + Hp + (size_t)n_hidden * Hp + (rbm ? (w1l ? 0 : Nst) + 16 : 0) +
                          (w1l ? (size_t)N * (Hp + 4) : 0) + uh_floats);
}

// LDS the sampler needs at least (W1 streamed from L2); vmc_create rejects shapes beyond 160 KiB
inline size_t plan_sweep_lds_required(int N, int Hp, int n_hidden, bool rbm) {
  return plan_sweep_lds_bytes(N, Hp, n_hidden, false, rbm);
}

// which instantiation of k_sweep16<NT, NW, ...> a launch takes and with how much LDS
struct SweepPlan {
  int ok;          // 0: the shape does not fit (launch refused)
  int w1l;         // W1 held in LDS
  int fast;        // 0: general variant; 2 / 4: prefetched-Philox variant with UPRE = 2 / 4 draws per lane
  int uh_lds;      // the dedicated hand-over area is part of the LDS
  size_t lds;
};
inline SweepPlan plan_sweep(int N, int NT, int NW, int n_hidden, bool rbm, bool no_w1l, bool plain, bool tuned) {
  SweepPlan p;
  memset(&p, 0, sizeof(p));
  const int Hp = NT * 16;
  const size_t lds_full = plan_sweep_lds_bytes(N, Hp, n_hidden, true, rbm);
  // (more than 256 units: W1 alone would need > 160 KiB; those variants are not instantiated)
  const bool w1l = NT <= 16 && lds_full <= PLAN_LDS_PER_CU && !no_w1l;
  size_t lds = w1l ? lds_full : plan_sweep_lds_bytes(N, Hp, n_hidden, false, rbm);
  if (lds > PLAN_LDS_PER_CU) return p;
  const int nblk = (N + 3) / 4;
  const bool fast2 = nblk <= 32 && plain, fast4 = nblk <= 64 && plain;
  // five-slot hand-over area of the UPRE = 4 variant at 256 units (sweep16_body: UH_IN_X is false)
  if (NT == 16 && NW == 8 && !w1l && !fast2 && fast4) {
    const size_t with_uh = plan_sweep_lds_bytes(N, Hp, n_hidden, false, rbm, 4 * 5 * 256);
    if (with_uh <= PLAN_LDS_PER_CU) { lds = with_uh; p.uh_lds = 1; }
  }
  p.ok = 1; p.w1l = w1l ? 1 : 0; p.lds = lds;
  p.fast = !tuned ? 0 : (fast2 ? 2 : (fast4 ? 4 : 0));
  return p;
}

// k_sweep8 (sweep8.hip): eight chains per workgroup on the 4x4x1 MFMA shape, bit-identical chains to k_sweep16.
// fully_connected + relu, 128 or 256 padded units (one wave per 32 units), at least one H x H layer, one Philox site
// block per lane of a chain's group (8 * Hp / 32 lanes): n_sites <= Hp.  LDS: spins [8][Nst], two operand buffers
// [8][Hp + 16], three [8] int arrays, w_out, the biases of the H x H layers, [W1 when it fits].
struct Sweep8Plan {
  int ok;
  int w1l;
  size_t lds;
};
inline size_t plan_sweep8_lds_bytes(int N, int Hp, int n_hidden, bool w1l) {
  const size_t Nst = (size_t)((N + 3) & ~3);
  return sizeof(float) * (8 * Nst + 2 * 8 * ((size_t)Hp + 16) + 24 + (size_t)Hp + (size_t)n_hidden * Hp +
                          (w1l ? (size_t)N * ((size_t)Hp + 4) : 0));
}
inline Sweep8Plan plan_sweep8(int N, int Hp, int n_hidden, bool no_w1l) {
  Sweep8Plan p;
  memset(&p, 0, sizeof(p));
  if ((Hp != 128 && Hp != 256) || n_hidden < 1 || N < 2 || N > Hp || N > 256) return p;
  const size_t full = plan_sweep8_lds_bytes(N, Hp, n_hidden, true);
  const bool w1l = !no_w1l && full <= PLAN_LDS_PER_CU;
  const size_t lds = w1l ? full : plan_sweep8_lds_bytes(N, Hp, n_hidden, false);
  if (lds > PLAN_LDS_PER_CU) return p;
  p.ok = 1; p.w1l = w1l ? 1 : 0; p.lds = lds;
  return p;
}
// Chains per sampler workgroup: 8 when the shape has a k_sweep8 and sixteen-chain tiles would leave at least half of
// the CUs without one (graph_builders.py:57-88: the batch is the only parallel axis); forced: CGS_VMC_SWEEP_TILE
// (0 = this rule, 8, 16; 8 is honoured where a k_sweep8 exists).
inline int plan_sweep_tile(long long B, int num_cus, bool sweep8_ok, int forced) {
  if (!sweep8_ok || forced == 16) return 16;
  if (forced == 8) return 8;
  return (B + 15) / 16 <= num_cus / 2 ? 8 : 16;
}

// 384 or 512 padded units and at least one H x H layer; LDS of k_tail_lds: two operand buffers
// [2 halves][NT][64][4], partial dots, row meta, biases, w_out
inline size_t plan_tail_lds_bytes(int Hp, int n_hidden) {
  const size_t nt = (size_t)Hp / 16;
  return sizeof(float) * (2 * (2 * nt * 256) + 4 * 32 + 96 + (size_t)n_hidden * nt * 16 + nt * 16);
}
inline bool plan_tail_lds_supported(int Hp, int n_hidden) {
  return (Hp == 384 || Hp == 512) && n_hidden >= 1 && plan_tail_lds_bytes(Hp, n_hidden) <= PLAN_LDS_PER_CU;
}

// ------------------------------------------------------------------------------- projected BCS determinant (pbdg.hip)
// ProjectedBDG: psi(x) = det M(x), M[r][c] = F[U_r][D_c] over the n = N/2 up sites U and down sites D of x (ascending).
// Each chain is one wave that keeps M^-1 (fp32) in LDS with an odd row stride (plan_pbdg_ld: the column walks of the
// matrix-vector products hit distinct banks), the scratch vectors of one exchange ratio and rank-2 update, the slot lists
// and the spins.  N <= 256 (n <= 128): the inverse stays within 64.5 KiB, so two chains still share a CU.
#define PLAN_PBDG_MAX_SITES 256
#define PLAN_PBDG_WG_LDS ((size_t)64 * 1024)   // chains per workgroup are packed up to this much LDS
PLAN_HD inline int plan_pbdg_ld(int n) { return (n & 1) ? n : n + 1; }
// floats: inverse n x ld, six vectors of n (x, y, M^-1 y, x M^-1, column r, row c), N spins; ints: up, dn, perm (n each), pos (N)
PLAN_HD inline size_t plan_pbdg_chain_lds_bytes(int N) {
  const size_t n = (size_t)N / 2, ld = (size_t)plan_pbdg_ld((int)n);
  return 4 * (n * ld + 6 * n + (size_t)N) + 4 * (3 * n + (size_t)N);
}
// chains (waves) per workgroup: 4, 2 or 1, as many as fit PLAN_PBDG_WG_LDS (at least one; one chain at n = 128 takes 72.7 KiB)
inline int plan_pbdg_chains_per_wg(int N) {
  const size_t b = plan_pbdg_chain_lds_bytes(N);
  for (int c = 4; c > 1; c >>= 1)
    if ((size_t)c * b <= PLAN_PBDG_WG_LDS) return c;
  return 1;
}
// The sampler rebuilds M^-1 by a fresh factorisation every R accepted moves of a chain (and after a move whose 2 x 2
// determinant is below PLAN_PBDG_TINY_RATIO in magnitude: the rank-2 update divides by it).  A factorisation costs n^3,
// an update 4 n^2 multiply-adds, so R = n keeps the refreshes at about a fifth of the update work; 16 <= R <= 128.
#define PLAN_PBDG_TINY_RATIO 1e-2f
inline int plan_pbdg_refresh_interval(int N) {
  const int n = N / 2;
  return n < 16 ? 16 : (n > 128 ? 128 : n);
}
// gradient sums: chain slices of the partial-sum launch (partials [slices][2][P] in double, folded in slice order):
// enough threads to fill the chip (about 1024 per CU), at most 256 slices, never more than the chains
inline int plan_pbdg_grad_slices(long long P, long long B, int num_cus) {
  long long s = ((long long)num_cus * 1024 + P - 1) / (P > 0 ? P : 1);
  if (s > 256) s = 256;
  if (s > B) s = B;
  return s < 1 ? 1 : (int)s;
}
inline long long plan_pbdg_grad_ws_doubles(long long P, int slices) { return 2LL * P * slices; }
// vmc_create's shape checks: N even (|U| = |D| = N/2), 2 <= N <= 256
inline int plan_pbdg_check(int N, char* msg, size_t msg_len) {
  if (N < 2 || (N & 1)) {
    snprintf(msg, msg_len, "pbdg: num_sites must be even and >= 2 (got %d): the projected BCS state lives at Sz = 0", N);
    return VMC_ERR_INVALID;
  }
  if (N > PLAN_PBDG_MAX_SITES) {
    snprintf(msg, msg_len, "pbdg: num_sites = %d beyond 256 (n = N/2 > 128: the inverse would exceed 64 KiB of LDS)", N);
    return VMC_ERR_UNSUPPORTED;
  }
  if (msg_len) msg[0] = 0;
  return VMC_OK;
}

// ------------------------------------------------------------------------------- neural-network backflow (nnb.hip)
// FullyConnectedNNB: the fully_connected trunk (L relu layers of H units) with a pairing layer of N^2 outputs,
// psi(x) = det F(x)[U, D].  The trunk and the pairing layer run on the general dense path in blocks of rows whose dense
// pairing layer [rows][N^2] is the only large buffer; the determinant rows reuse pbdg's LDS plan (plan_pbdg_*), hence
// N <= 256.  H <= 512 and L <= 16 are what hostcheck walks; the gradient path holds d ln|psi| / d out of all B chains
// densely ([B][N^2], the A operand of the weight-gradient launch), bounded by PLAN_NNB_MAX_DELTA floats (4 GiB).
#define PLAN_NNB_MAX_SITES PLAN_PBDG_MAX_SITES
#define PLAN_NNB_MAX_UNITS 512
#define PLAN_NNB_MAX_LAYERS 16
#define PLAN_NNB_MAX_DELTA (1LL << 30)
#define PLAN_NNB_BLOCK_MB_DEFAULT 256      // CGS_VMC_NNB_BLOCK_MB
#define PLAN_NNB_BLOCK_MB_MAX 4096
inline int plan_nnb_check(int N, int L, int H, long long B, char* msg, size_t msg_len) {
  if (N < 2 || (N & 1)) {
    snprintf(msg, msg_len, "fully_connected_nnb: num_sites must be even and >= 2 (got %d): psi = det F[up, down] lives at Sz = 0", N);
    return VMC_ERR_INVALID;
  }
  if (B < 1 || H < 1) { snprintf(msg, msg_len, "batch_size, layer_size >= 1 required"); return VMC_ERR_INVALID; }
  if (N > PLAN_NNB_MAX_SITES) {
    snprintf(msg, msg_len, "fully_connected_nnb: num_sites = %d beyond 256 (n = N/2 > 128: the inverse would exceed 64 KiB of LDS)", N);
    return VMC_ERR_UNSUPPORTED;
  }
  if (L < 1 || L > PLAN_NNB_MAX_LAYERS) {
    snprintf(msg, msg_len, "fully_connected_nnb: num_layers = %d outside 1..16", L);
    return VMC_ERR_UNSUPPORTED;
  }
  if (H > PLAN_NNB_MAX_UNITS) {
    snprintf(msg, msg_len, "fully_connected_nnb: layer_size = %d beyond 512", H);
    return VMC_ERR_UNSUPPORTED;
  }
  if (B * (long long)N * N > PLAN_NNB_MAX_DELTA) {
    snprintf(msg, msg_len, "fully_connected_nnb: batch_size x num_sites^2 = %lld beyond 2^30 (the gradient path's dense pairing-layer delta)",
             B * (long long)N * N);
    return VMC_ERR_UNSUPPORTED;
  }
  if (msg_len) msg[0] = 0;
  return VMC_OK;
}
// rows per block of the forward passes: block_mb MiB of dense pairing layer (clamped to 1 .. 4096), at least one row, at
// most 2^20 rows (the trunk's buffers follow) -- the whole workspace of a block is rows x (N^2 + 2 Hp) floats
inline long long plan_nnb_block_rows(int N, long long block_mb) {
  if (block_mb < 1) block_mb = 1;
  if (block_mb > PLAN_NNB_BLOCK_MB_MAX) block_mb = PLAN_NNB_BLOCK_MB_MAX;
  long long rows = (block_mb << 20) / ((long long)N * N * (long long)sizeof(float));
  if (rows < 1) rows = 1;
  if (rows > (1LL << 20)) rows = 1LL << 20;
  return rows;
}
inline long long plan_nnb_block_floats(int N, int Hp, long long rows) { return rows * ((long long)N * N + 2LL * Hp); }
// launches of the determinant rows kernel: cpw rows (waves) per workgroup
inline long long plan_nnb_rows_grid(long long rows, int N) {
  const int cpw = plan_pbdg_chains_per_wg(N);
  return (rows + cpw - 1) / cpw;
}

// ------------------------------------------------------------------------------- Lin-table state vector (edvec.hip)
// FullVector: psi(x) = v[top_t[top(x)] + bot_t[bot(x)]] at Sz = 0; a configuration is one 32-bit word, bot(x) its low
// N/2 bits.  N even and at most 28: the largest size the tests run (C(28,14) = 40,116,600 entries, 160 MB); the index
// arithmetic itself is 32-bit up to N = 32 (C(32,16) < 2^31).  The two tables hold 2^(N/2) int32 each; the persistent
// sampler stages them in LDS (at most 128 KiB at N = 28, one workgroup per CU), every other kernel reads them through L2.
#define PLAN_EDVEC_MAX_SITES 28
#define PLAN_EDVEC_TABLES_LDS_MAX ((size_t)128 * 1024)
PLAN_HD inline size_t plan_edvec_tables_bytes(int N) { return (size_t)2 * sizeof(int32_t) << (N / 2); }
inline bool plan_edvec_tables_in_lds(int N) { return plan_edvec_tables_bytes(N) <= PLAN_EDVEC_TABLES_LDS_MAX; }
// sampler: one thread per chain and a step is one dependent gather, so the time is latency over chains in flight.
// The chains are spread over all CUs in whole waves (a CU's waves interleave their gathers), at most 1024 per workgroup
inline int plan_edvec_sweep_threads(long long B, int num_cus) {
  const long long cus = num_cus > 0 ? num_cus : 1;
  long long waves = (B + 64 * cus - 1) / (64 * cus);
  if (waves < 1) waves = 1;
  if (waves > 16) waves = 16;
  return (int)(64 * waves);
}
inline unsigned plan_edvec_sweep_grid(long long B, int threads) { return (unsigned)((B + threads - 1) / threads); }
// vmc_create's shape checks: N even, 2 <= N <= 28, 1 <= len < 2^31
inline int plan_edvec_check(int N, long long len, char* msg, size_t msg_len) {
  if (N < 2 || (N & 1)) {
    snprintf(msg, msg_len, "ed_vector: num_sites must be even and >= 2 (got %d): the Lin tables address the Sz = 0 sector", N);
    return VMC_ERR_INVALID;
  }
  if (N > PLAN_EDVEC_MAX_SITES) {
    snprintf(msg, msg_len, "ed_vector: num_sites = %d beyond %d (the largest size the kernels are tested at)", N, PLAN_EDVEC_MAX_SITES);
    return VMC_ERR_UNSUPPORTED;
  }
  if (len < 1) {
    snprintf(msg, msg_len, "ed_vector: the vector length (layer_size) must be >= 1 (got %lld)", len);
    return VMC_ERR_INVALID;
  }
  if (len > 0x7fffffffLL) {
    snprintf(msg, msg_len, "ed_vector: a vector of %lld entries is beyond the 32-bit index", len);
    return VMC_ERR_UNSUPPORTED;
  }
  if (msg_len) msg[0] = 0;
  return VMC_OK;
}
// vmc_set_lin_tables: n_half = 2^(N/2), and every Sz = 0 configuration -- a top half-word with N/2 - k set bits and a bot
// half-word with k -- lands in [0, len).  Per popcount class the smallest and the largest entry decide.
inline int plan_edvec_check_tables(int N, int n_half, const int32_t* top, const int32_t* bot, long long len, char* msg,
                                   size_t msg_len) {
  const int h = N / 2;
  if (n_half != (1 << h)) {
    snprintf(msg, msg_len, "ed_vector: the Lin tables must hold 2^(N/2) = %d entries each (got %d)", 1 << h, n_half);
    return VMC_ERR_INVALID;
  }
  if (!top || !bot) { snprintf(msg, msg_len, "ed_vector: null Lin table"); return VMC_ERR_INVALID; }
  long long lo_t[17], hi_t[17], lo_b[17], hi_b[17];
  for (int k = 0; k <= h; ++k) { lo_t[k] = lo_b[k] = 0x7fffffffffffLL; hi_t[k] = hi_b[k] = -0x7fffffffffffLL; }
  for (int wd = 0; wd < n_half; ++wd) {
    int k = 0;
    for (int i = 0; i < h; ++i) k += (wd >> i) & 1;
    if (top[wd] < lo_t[k]) lo_t[k] = top[wd];
    if (top[wd] > hi_t[k]) hi_t[k] = top[wd];
    if (bot[wd] < lo_b[k]) lo_b[k] = bot[wd];
    if (bot[wd] > hi_b[k]) hi_b[k] = bot[wd];
  }
  for (int k = 0; k <= h; ++k)
    if (lo_t[h - k] + lo_b[k] < 0 || hi_t[h - k] + hi_b[k] >= len) {
      const long long bad = lo_t[h - k] + lo_b[k] < 0 ? lo_t[h - k] + lo_b[k] : hi_t[h - k] + hi_b[k];
      snprintf(msg, msg_len, "ed_vector: an Sz = 0 configuration with %d up spins in its lower half has index %lld outside [0, %lld)",
               k, bad, len);
      return VMC_ERR_INVALID;
    }
  if (msg_len) msg[0] = 0;
  return VMC_OK;
}

// ------------------------------------------------------------------------------- product ctx (vmc_api_prod.hip, prod.hip)
// psi = psi_a psi_b over one set of chains: theta = [a | b], accumulators [g1_a g1_b | g2_a g2_b | 8 scalars].
#define PLAN_PROD_CHAINS_PER_WG 4     // one wave per chain (k_prod_accept, the arithmetic of k_wide_propose)
#define PLAN_PROD_FOLD_THREADS 1024   // the single workgroup that folds the chains' acceptance counts in a fixed order
inline long long plan_prod_acc_floats(long long Pa, long long Pb) { return 2 * (Pa + Pb) + 8; }
inline unsigned plan_prod_chain_grid(long long B) { return (unsigned)((B + PLAN_PROD_CHAINS_PER_WG - 1) / PLAN_PROD_CHAINS_PER_WG); }
inline unsigned plan_prod_elem_grid(long long n) { return (unsigned)((n + 255) / 256); }    // 256 threads, one element each
// Which ctx may be a factor: fully_connected / rbm with the exp output (every width), pbdg, ed_vector.  The convolutional
// types, gnn and fully_connected_nnb keep their gradient sums inside block loops of their own and are refused.
inline int plan_prod_child_check(int ansatz, int output_activation, bool is_product, char* msg, size_t msg_len) {
  if (is_product) { snprintf(msg, msg_len, "prod: a product ctx cannot be a factor of another product"); return VMC_ERR_UNSUPPORTED; }
  if (ansatz == VMC_ANSATZ_PBDG || ansatz == VMC_ANSATZ_ED_VECTOR) { if (msg_len) msg[0] = 0; return VMC_OK; }
  if (ansatz == VMC_ANSATZ_FULLY_CONNECTED || ansatz == VMC_ANSATZ_RBM) {
    if (output_activation != 1 /* VMC_ACT_EXP */) {
      snprintf(msg, msg_len, "prod: a dense factor needs the exp output activation (a positive amplitude with a shift)");
      return VMC_ERR_UNSUPPORTED;
    }
    if (msg_len) msg[0] = 0;
    return VMC_OK;
  }
  snprintf(msg, msg_len, "prod: factors are fully_connected, rbm, pbdg or ed_vector ctxs (the convolutional types, gnn and fully_connected_nnb are not taken)");
  return VMC_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------- the measurements (vmc_api_measure.hip; corr.hip, renyi.hip, dimer.hip, symm.hip, proj.hip)
// A measurement runs its items -- pairs of sites, regions, bonds, pairs of bonds -- in passes; a pass is B rows per item
// (row = item x B + chain): for the spin correlations a bond set of its own (bonds, couplings, rowinfo / val) plus the
// dense [B][pairs] scatter target, for the others rows handed to the family's full forward.  Rows of a pass: the budget
// of 2^24 rows (rowinfo 128 MB, val and the dense buffer 64 MB each), never past the 32-bit row index rule of
// vmc_set_bonds (B x items <= 2^31 - 1 - B), and never more than `row_limit` rows where the caller states one (0: none)
// -- what the forward's scratch takes: plan_measure_row_limit below; the spin correlations state none.  At least one
// item whatever the budget says; requested > 0: at most that many items per pass.  Returns 0 when not even one item
// fits the row index (2 B > 2^31 - 1) or an argument is out of range (n_items < 1 included: a dimer call without pairs
// runs no phase 2 and does not ask).
#define PLAN_MEASURE_ROW_BUDGET (1LL << 24)
inline int plan_measure_per_pass(long long B, long long n_items, long long requested, long long row_limit = 0) {
  if (B < 1 || n_items < 1 || requested < 0 || row_limit < 0) return 0;
  const long long limit = (0x7fffffffLL - B) / B;
  if (limit < 1) return 0;
  long long budget = PLAN_MEASURE_ROW_BUDGET;
  if (row_limit > 0 && row_limit < budget) budget = row_limit;
  long long per = budget / B;
  if (per < 1) per = 1;
  if (per > limit) per = limit;
  if (requested > 0 && requested < per) per = requested;
  if (per > n_items) per = n_items;
  return (int)per;
}
// Rows the forward of one pass may take: the scratch per row is the configuration (N floats), the first layer's
// output (Hp floats; the convolutional types and the table types keep the minimal Hp) and five words of row list,
// outputs and signs -- kept within 2^30 floats (4 GiB) -- and every flat index into it (rows x max(N, Hp)) within 32
// bits.  The blocked forwards (general dense, nnb's dense block of nnb_rows rows with its N^2 pairing layer, the general
// convolution) walk any row count in blocks of their own, so they state no further limit.
inline long long plan_measure_row_limit(int N, int Hp) {
  const long long widest = N > Hp ? N : Hp;
  const long long by_index = 0x7fffffffLL / (widest > 0 ? widest : 1);
  const long long by_bytes = (1LL << 30) / ((long long)N + Hp + 5);
  const long long rows = by_index < by_bytes ? by_index : by_bytes;
  return rows < 1 ? 1 : rows;
}
// a buffer [n_items][B] that a fold indexes item x B + chain (the dimers' phase 1): all of its rows stay within the
// 32-bit row index
inline bool plan_measure_rows_ok(long long B, long long n_items) {
  return B >= 1 && n_items >= 1 && n_items <= (0x7fffffffLL - B) / B;
}
inline long long plan_measure_passes(long long n_items, int per) { return per < 1 ? 0 : (n_items + per - 1) / per; }
inline unsigned plan_measure_fold_grid(int items) { return (unsigned)((items + 63) / 64); }    // 64 threads, one item each

// The ops of vmc_symmetry_expectations (symm.hip): perm [n_ops][N] site permutations, flip [n_ops] 0 / 1 (null: no
// flips).  Every perm_k must be a bijection of 0 .. N - 1 -- k_symm_rows gathers x[perm_k[i]], and pbdg, nnb and ed_vector
// index by up / down counts: a bijection and a global flip keep a row at Sz = 0, anything else may not.  VMC_OK, or
// VMC_ERR_INVALID with the op and the entry named in msg.
inline int plan_symm_check_ops(int N, int n_ops, const int32_t* perm, const uint8_t* flip, char* msg, size_t msg_len) {
  if (msg_len) msg[0] = 0;
  if (N < 1 || n_ops < 1 || !perm) {
    snprintf(msg, msg_len, "bad symmetry op arguments");
    return VMC_ERR_INVALID;
  }
  std::vector<unsigned char> seen((size_t)N);
  for (int k = 0; k < n_ops; ++k) {
    if (flip && flip[k] > 1) {
      snprintf(msg, msg_len, "op %d: flip = %d, 0 or 1 required", k, (int)flip[k]);
      return VMC_ERR_INVALID;
    }
    const int32_t* g = perm + (size_t)k * (size_t)N;
    seen.assign((size_t)N, 0);
    for (int i = 0; i < N; ++i) {
      if (g[i] < 0 || g[i] >= N) {
        snprintf(msg, msg_len, "op %d: entry %d = %d is no site in 0 .. %d", k, i, (int)g[i], N - 1);
        return VMC_ERR_INVALID;
      }
      if (seen[(size_t)g[i]]) {
        snprintf(msg, msg_len, "op %d: entry %d names site %d a second time (a permutation of 0 .. %d required)", k, i, (int)g[i], N - 1);
        return VMC_ERR_INVALID;
      }
      seen[(size_t)g[i]] = 1;
    }
  }
  return VMC_OK;
}

// Symmetry-projected energies (vmc_projected_energy; proj.hip).  The per-chain accumulator acc [n_sectors][B] (fp64,
// sector major) is bounded by PLAN_PROJ_MAX_ACC doubles (512 MiB).  k_proj_accum takes the ops of a pass in launches of
// at most PLAN_PROJ_LAUNCH_OPS ops; a workgroup stages the characters of its sector tile for the launch's ops in LDS
// ([ops][tile] doubles) and a thread keeps the tile's accumulators of its chain in registers, hence at most
// PLAN_PROJ_MAX_TILE sectors per tile, fewer where the launch's ops would not fit PLAN_PROJ_LDS_BYTES (several
// workgroups per CU).  0: an argument out of range, or not even one sector fits.
#define PLAN_PROJ_MAX_ACC (1LL << 26)
#define PLAN_PROJ_MAX_TILE 16
#define PLAN_PROJ_LAUNCH_OPS 256
#define PLAN_PROJ_LDS_BYTES ((size_t)32 * 1024)
#define PLAN_PROJ_THREADS 256             // chains per workgroup of k_proj_accum
inline bool plan_proj_acc_ok(long long B, long long n_sectors) {
  return B >= 1 && n_sectors >= 1 && n_sectors <= PLAN_PROJ_MAX_ACC / B;
}
inline int plan_measure_sector_tile(long long n_sectors, long long ops_per_launch) {
  if (n_sectors < 1 || ops_per_launch < 1) return 0;
  long long tile = (long long)(PLAN_PROJ_LDS_BYTES / sizeof(double)) / ops_per_launch;
  if (tile > PLAN_PROJ_MAX_TILE) tile = PLAN_PROJ_MAX_TILE;
  if (tile > n_sectors) tile = n_sectors;
  return (int)tile;
}
inline size_t plan_proj_accum_lds_bytes(int tile, int ops) { return (size_t)tile * (size_t)ops * sizeof(double); }
inline unsigned plan_proj_chain_blocks(long long B) { return (unsigned)((B + PLAN_PROJ_THREADS - 1) / PLAN_PROJ_THREADS); }
inline unsigned plan_proj_sector_tiles(long long n_sectors, int tile) { return tile < 1 ? 0u : (unsigned)((n_sectors + tile - 1) / tile); }

// Are the ops symmetries of the Hamiltonian sum_b j_x[b] (S+S- + S-S+) / 2 + j_z[b] SzSz over the bonds ij [n_bonds][2]?
// Op k maps bond (i, j) to (perm_k[i], perm_k[j]); it is a symmetry when the multiset of (unordered pair, bits of j_x, bits
// of j_z) over the bonds is the one it started as (a multiset: the 2-wide torus names a bond twice).  Invariance under
// perm_k and under its inverse are the same statement, so the row convention of the ops does not matter; the global flip
// is a symmetry of every XXZ bond and is not asked about.  perm: bijections (plan_symm_check_ops first).  VMC_OK, or
// VMC_ERR_INVALID with the op and the first bond whose image is missing named in msg.
struct PlanBondKey {
  int32_t lo, hi; uint32_t jx, jz; int32_t bond;
  bool same(const PlanBondKey& o) const { return lo == o.lo && hi == o.hi && jx == o.jx && jz == o.jz; }
  bool before(const PlanBondKey& o) const {
    if (lo != o.lo) return lo < o.lo;
    if (hi != o.hi) return hi < o.hi;
    if (jx != o.jx) return jx < o.jx;
    if (jz != o.jz) return jz < o.jz;
    return bond < o.bond;
  }
};
inline void plan_bond_key_sort(std::vector<PlanBondKey>& v) {
  std::sort(v.begin(), v.end(), [](const PlanBondKey& a, const PlanBondKey& b) { return a.before(b); });
}
inline int plan_symm_check_hamiltonian(int N, int n_bonds, const int32_t* ij, const float* jx, const float* jz, int n_ops,
                                       const int32_t* perm, char* msg, size_t msg_len) {
  if (msg_len) msg[0] = 0;
  if (N < 1 || n_bonds < 1 || n_ops < 1 || !ij || !jx || !jz || !perm) {
    snprintf(msg, msg_len, "bad Hamiltonian symmetry arguments");
    return VMC_ERR_INVALID;
  }
  auto key = [&](int b, int32_t i, int32_t j) {
    PlanBondKey k;
    k.lo = i < j ? i : j; k.hi = i < j ? j : i; k.bond = b;
    memcpy(&k.jx, jx + b, sizeof(uint32_t)); memcpy(&k.jz, jz + b, sizeof(uint32_t));
    return k;
  };
  std::vector<PlanBondKey> base((size_t)n_bonds), image((size_t)n_bonds);
  for (int b = 0; b < n_bonds; ++b) {
    if (ij[2 * b] < 0 || ij[2 * b] >= N || ij[2 * b + 1] < 0 || ij[2 * b + 1] >= N) {
      snprintf(msg, msg_len, "bond %d = (%d, %d) names no two sites in 0 .. %d", b, (int)ij[2 * b], (int)ij[2 * b + 1], N - 1);
      return VMC_ERR_INVALID;
    }
    base[(size_t)b] = key(b, ij[2 * b], ij[2 * b + 1]);
  }
  plan_bond_key_sort(base);
  for (int k = 0; k < n_ops; ++k) {
    const int32_t* g = perm + (size_t)k * (size_t)N;
    for (int b = 0; b < n_bonds; ++b) image[(size_t)b] = key(b, g[ij[2 * b]], g[ij[2 * b + 1]]);
    plan_bond_key_sort(image);
    int bad = -1;                         // the lowest bond whose image has no partner left in the original multiset
    size_t p = 0;
    for (size_t q = 0; q < image.size(); ++q) {
      while (p < base.size() && !image[q].same(base[p]) && base[p].before(image[q])) ++p;
      if (p < base.size() && image[q].same(base[p])) { ++p; continue; }
      if (bad < 0 || image[q].bond < bad) bad = image[q].bond;
    }
    if (bad >= 0) {
      snprintf(msg, msg_len, "op %d is no symmetry of the Hamiltonian: bond %d = (%d, %d) goes to (%d, %d), which is no bond with its couplings",
               k, bad, (int)ij[2 * bad], (int)ij[2 * bad + 1], (int)g[ij[2 * bad]], (int)g[ij[2 * bad + 1]]);
      return VMC_ERR_INVALID;
    }
  }
  return VMC_OK;
}

// ------------------------------------------------------------------------------- symmetrized ctx (vmc_api_symz.hip, symz.hip)
// psi_s(x) = sum_k chi_k psi(g_k x) over one set of B chains: the base ctx holds the n_ops B permuted rows (row = k B + c)
// as its chains and does all network arithmetic; theta is the base's, the accumulators are [g1 | g2 | 8 scalars] at P.
//
// The structural zero.  Per chain, with l_k = ln|psi(g_k x)|, s_k its sign and m = max_k l_k over the ops that count
// (chi_k != 0, s_k != 0): S = sum_k chi_k s_k exp(l_k - m), A = sum_k |chi_k| exp(l_k - m), both in fp64, ops ascending.
// A row is AT A ZERO of the sector where |S| <= 2^-40 A.  Why 2^-40: the fp64 sum of at most 1,024 terms of magnitude
// <= A is off by at most 1,024 x 2^-53 A = 2^-43 A, so a sum that cancels exactly in real arithmetic lands below
// 2^-40 A with a factor 8 to spare -- but only if the terms that cancel are bit-identical, i.e. the SAME row evaluated
// twice (an op with character -1 that maps the configuration onto itself).  Two different rows of equal amplitude carry
// the fp32 logits' noise, 2^-24 A, sixteen binary orders above the threshold: the rule never fires on a near miss.
#define PLAN_SYMZ_MAX_OPS 1024
#define PLAN_SYMZ_ZERO_LOG2 (-40)
#define PLAN_SYMZ_THREADS 256            // chains per workgroup of the one-thread-per-chain folds
#define PLAN_SYMZ_CHAINS_PER_WG 4        // one wave per chain (k_symz_accept: the arithmetic of k_wide_propose)
#define PLAN_SYMZ_ZERO 0x1p-40           // 2^PLAN_SYMZ_ZERO_LOG2
PLAN_HD inline bool plan_symz_is_zero(double S, double A) { return !(fabs(S) > PLAN_SYMZ_ZERO * A); }
inline unsigned plan_symz_chain_blocks(long long B) { return (unsigned)((B + PLAN_SYMZ_THREADS - 1) / PLAN_SYMZ_THREADS); }
inline unsigned plan_symz_wave_grid(long long B) { return (unsigned)((B + PLAN_SYMZ_CHAINS_PER_WG - 1) / PLAN_SYMZ_CHAINS_PER_WG); }
inline long long plan_symz_acc_floats(long long P) { return 2 * P + 8; }
// What vmc_create_symmetrized decides before anything is allocated.  The base may be what a product takes as a factor
// (fully_connected / rbm with the exp output, pbdg, ed_vector: their gradient sums take an external weight vector);
// base_composite: the base is a product or a symmetrized ctx; base_owned: it already belongs to one.  VMC_OK, or the
// status with the reason in msg.
inline int plan_symz_check(int base_ansatz, int base_output_activation, bool base_composite, bool base_owned,
                           long long base_B, int N, long long batch_size, long long n_ops, const int32_t* perms,
                           const uint8_t* flips, const double* characters, char* msg, size_t msg_len) {
  if (msg_len) msg[0] = 0;
  if (base_composite) {
    snprintf(msg, msg_len, "symmetrized: a product or symmetrized ctx cannot be the base of a symmetrized ctx");
    return VMC_ERR_UNSUPPORTED;
  }
  if (base_ansatz == VMC_ANSATZ_FULLY_CONNECTED || base_ansatz == VMC_ANSATZ_RBM) {
    if (base_output_activation != 1 /* VMC_ACT_EXP */) {
      snprintf(msg, msg_len, "symmetrized: a dense base needs the exp output activation (a positive amplitude with a shift)");
      return VMC_ERR_UNSUPPORTED;
    }
  } else if (base_ansatz != VMC_ANSATZ_PBDG && base_ansatz != VMC_ANSATZ_ED_VECTOR) {
    snprintf(msg, msg_len, "symmetrized: the base is a fully_connected, rbm, pbdg or ed_vector ctx (the convolutional types, gnn and fully_connected_nnb are not taken)");
    return VMC_ERR_UNSUPPORTED;
  }
  if (base_owned) {
    snprintf(msg, msg_len, "symmetrized: the base already belongs to a product or symmetrized ctx");
    return VMC_ERR_STATE;
  }
  if (batch_size < 1) { snprintf(msg, msg_len, "symmetrized: batch_size >= 1 required"); return VMC_ERR_INVALID; }
  if (n_ops < 1 || n_ops > PLAN_SYMZ_MAX_OPS) {
    snprintf(msg, msg_len, "symmetrized: n_ops = %lld, 1 .. %d required", n_ops, PLAN_SYMZ_MAX_OPS);
    return VMC_ERR_INVALID;
  }
  if (base_B != batch_size * n_ops) {
    snprintf(msg, msg_len, "symmetrized: the base holds %lld rows, batch_size x n_ops = %lld x %lld = %lld required", base_B,
             batch_size, n_ops, batch_size * n_ops);
    return VMC_ERR_INVALID;
  }
  if (!perms || !characters) { snprintf(msg, msg_len, "symmetrized: null ops or characters"); return VMC_ERR_INVALID; }
  const int rc = plan_symm_check_ops(N, (int)n_ops, perms, flips, msg, msg_len);
  if (rc != VMC_OK) return rc;
  bool any = false;
  for (long long k = 0; k < n_ops; ++k) {
    if (!std::isfinite(characters[k])) {
      snprintf(msg, msg_len, "symmetrized: character %lld is not finite", k);
      return VMC_ERR_INVALID;
    }
    any = any || characters[k] != 0.0;
  }
  if (!any) { snprintf(msg, msg_len, "symmetrized: every character is zero"); return VMC_ERR_INVALID; }
  return VMC_OK;
}

// Lanczos-step energies (vmc_energy_moments; moments.hip).  The second-order list -- the rows x^{ab} over (chain,
// antiparallel bond a, bond b antiparallel on x^a) -- is indexed with 32-bit integers like the first-order list; a chain
// has at most n_bonds first-order rows of at most n_bonds second-order rows each, so B n_bonds^2 <= 2^31 - 1 keeps every
// index and the prefix off2 in range whatever the configurations are.  A compacted list (this one, the four-spin terms')
// goes through the forward in passes of ROWS (not of items x B as the dense measurements): plan_list_per_pass is the
// budget of 2^24 rows, never more than row_limit (plan_measure_row_limit; 0: none), requested > 0: at most that many; at
// least one row.  0 passes for an empty list; -1: an argument out of range.
// Within a chain the row at place p = q - s (s: the chain's first row) belongs to lane p mod 64 of the chain's
// accumulator: plan_moment_first_row is the first row >= lo that lane `lane` owns, plan_moment_rows_of_lane how many
// of [lo, hi) it owns -- together they state that the lanes' walks partition every pass's slice of a chain.
inline bool plan_moment_index_ok(long long B, long long n_bonds) {
  return B >= 1 && n_bonds >= 1 && n_bonds <= 0x7fffffffLL && n_bonds * n_bonds <= 0x7fffffffLL / B;
}
inline long long plan_list_per_pass(long long n_rows, long long requested, long long row_limit) {
  if (n_rows < 0 || requested < 0 || row_limit < 0) return -1;
  long long per = PLAN_MEASURE_ROW_BUDGET;
  if (row_limit > 0 && row_limit < per) per = row_limit;
  if (requested > 0 && requested < per) per = requested;
  if (per > n_rows) per = n_rows;
  if (per < 1) per = 1;
  return per;
}
PLAN_HD inline long long plan_moment_first_row(long long s, long long lo, int lane) {
  return lo + ((lane - (int)((lo - s) & 63)) & 63);
}
inline long long plan_moment_rows_of_lane(long long s, long long lo, long long hi, int lane) {
  const long long q = plan_moment_first_row(s, lo, lane);
  return q >= hi ? 0 : (hi - q + 63) / 64;
}

// Four-spin (J-Q) terms (vmc_set_four_spin_terms; fourspin.hip).  A term is (i, j, k, l; q) with four distinct sites; the
// host reduces the terms to the table of their distinct unordered site pairs -- pairs[p] = (min, max), ascending by
// (min, max), n_pairs <= 2 n_terms -- and term_pairs[t] = the two indices of (i, j) and (k, l) into it (a term whose two
// pairs are the same unordered pair cannot occur: the sites are distinct).  Per chain the list holds one single row per
// antiparallel pair and one double row per term with both pairs antiparallel, so B (n_pairs + n_terms) <= 2^31 - 1 keeps
// every row index and the prefix over the chains within 32 bits whatever the configurations are.  The fold keeps a chain's
// single ratios in LDS by pair index (fp64): at most PLAN_FOURSPIN_MAX_PAIRS pairs; PLAN_FOURSPIN_MAX_TERMS bounds the
// term table.  plan_fourspin_check validates everything before anything is stored; VMC_OK, or the error with the term
// (or the cap) named in msg.  The list goes through the forward in passes of ROWS (plan_list_per_pass).
#define PLAN_FOURSPIN_MAX_TERMS (1 << 16)
#define PLAN_FOURSPIN_MAX_PAIRS 4096
struct FourSpinTable {
  std::vector<int32_t> pairs;        // [n_pairs][2]
  std::vector<int32_t> term_pairs;   // [n_terms][2]
  int n_pairs() const { return (int)(pairs.size() / 2); }
};
inline FourSpinTable plan_fourspin_pairs(int n_terms, const int32_t* ijkl) {
  FourSpinTable t;
  std::vector<std::pair<int32_t, int32_t>> all;
  all.reserve((size_t)n_terms * 2);
  for (int k = 0; k < 2 * n_terms; ++k) {
    const int32_t a = ijkl[2 * (size_t)k], b = ijkl[2 * (size_t)k + 1];
    all.emplace_back(a < b ? a : b, a < b ? b : a);
  }
  std::vector<std::pair<int32_t, int32_t>> uniq(all);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (const auto& p : uniq) { t.pairs.push_back(p.first); t.pairs.push_back(p.second); }
  for (const auto& p : all)
    t.term_pairs.push_back((int32_t)(std::lower_bound(uniq.begin(), uniq.end(), p) - uniq.begin()));
  return t;
}
inline int plan_fourspin_check(int N, long long B, int n_terms, const int32_t* ijkl, const float* q, int exchange_sign,
                               long long rows_per_pass, char* msg, size_t msg_len) {
  if (msg_len) msg[0] = 0;
  if (N < 1 || B < 1 || n_terms < 1 || !ijkl || !q) {
    snprintf(msg, msg_len, "vmc_set_four_spin_terms: bad term arguments");
    return VMC_ERR_INVALID;
  }
  if (exchange_sign != 1 && exchange_sign != -1) {
    snprintf(msg, msg_len, "vmc_set_four_spin_terms: exchange_sign = %d, +1 or -1 required", exchange_sign);
    return VMC_ERR_INVALID;
  }
  if (rows_per_pass < 0) {
    snprintf(msg, msg_len, "vmc_set_four_spin_terms: bad rows_per_pass (0: the library decides)");
    return VMC_ERR_INVALID;
  }
  if (n_terms > PLAN_FOURSPIN_MAX_TERMS) {
    snprintf(msg, msg_len, "vmc_set_four_spin_terms: %d terms beyond the cap of %d terms", n_terms, PLAN_FOURSPIN_MAX_TERMS);
    return VMC_ERR_UNSUPPORTED;
  }
  for (int t = 0; t < n_terms; ++t) {
    const int32_t* s = ijkl + 4 * (size_t)t;
    bool ok = true;
    for (int a = 0; a < 4; ++a) {
      ok = ok && s[a] >= 0 && s[a] < N;
      for (int b = 0; b < a; ++b) ok = ok && s[a] != s[b];
    }
    if (!ok) {
      snprintf(msg, msg_len, "vmc_set_four_spin_terms: term %d = (%d, %d, %d, %d): four distinct sites in 0 .. %d required", t,
               (int)s[0], (int)s[1], (int)s[2], (int)s[3], N - 1);
      return VMC_ERR_INVALID;
    }
    if (!std::isfinite(q[t])) {
      snprintf(msg, msg_len, "vmc_set_four_spin_terms: the coupling q of term %d is not finite", t);
      return VMC_ERR_INVALID;
    }
  }
  const int n_pairs = plan_fourspin_pairs(n_terms, ijkl).n_pairs();
  if (n_pairs > PLAN_FOURSPIN_MAX_PAIRS) {
    snprintf(msg, msg_len, "vmc_set_four_spin_terms: %d distinct site pairs beyond the cap of %d pairs (the fold's LDS table)",
             n_pairs, PLAN_FOURSPIN_MAX_PAIRS);
    return VMC_ERR_UNSUPPORTED;
  }
  if ((long long)n_pairs + n_terms > 0x7fffffffLL / B) {
    snprintf(msg, msg_len, "vmc_set_four_spin_terms: batch_size x (pairs + terms) = %lld x %lld does not fit the 32-bit row index",
             B, (long long)n_pairs + n_terms);
    return VMC_ERR_UNSUPPORTED;
  }
  return VMC_OK;
}
// The result buffers span the whole list, whose length changes with the chains: they are reserved once for the a-priori
// maximum B (n_pairs + n_terms) rows where that stays within PLAN_FOURSPIN_RESULT_ROWS (2^26 rows, 256 MiB a buffer), so
// that training never reallocates; beyond it geometrically -- at least twice what is held, never past the maximum.
#define PLAN_FOURSPIN_RESULT_ROWS (1LL << 26)
inline long long plan_fourspin_result_rows(long long B, long long n_pairs, long long n_terms, long long total, long long held) {
  const long long most = B * (n_pairs + n_terms);
  if (total <= held) return held;
  if (most <= PLAN_FOURSPIN_RESULT_ROWS) return most;
  long long rows = held * 2 > total ? held * 2 : total;
  if (rows < PLAN_FOURSPIN_RESULT_ROWS) rows = PLAN_FOURSPIN_RESULT_ROWS;
  return rows > most ? most : rows;
}
inline size_t plan_fourspin_fold_lds(int n_pairs) { return (size_t)(n_pairs > 0 ? n_pairs : 1) * sizeof(double); }

// ------------------------------------------------------------------------------- the kernel path of a ctx
// Which family of kernels a ctx runs: decided once (plan_desc, plan_split_path; vmc_create_product sets PATH_PRODUCT),
// kept in vmc_ctx::path, reported by vmc_debug_kernel_path -- the numbers are part of the test suite and of bench.py.
// Code that differs by family is a `switch` over the path that names every enumerator and has no `default`
// (-Werror=switch: a new path fails to compile at every such site until each names it); yes/no questions that more
// than one site asks are the predicates below.
enum KernelPath {
  PATH_FUSED = 0,          // fused dense kernels, <= 256 padded units (k_sweep16 / k_sweep8, k_tail16, k_backprop16)
  PATH_FUSED_LDS = 1,      // fused dense kernels, 257 .. 512 units: operands in LDS (k_sweep16<24|32>, k_tail_lds)
  PATH_DENSE_GENERAL = 2,  // dense layers as GEMMs over row buffers (wide.hip): > 512 units, or CGS_VMC_WIDE_FAST=0
  PATH_CONV = 3,           // fused convolutions (conv.hip)
  PATH_SPLIT_ROWS = 4,     // PATH_FUSED with the row kernel on the bf16 matrix cores (CGS_VMC_SPLIT_BF16=1, EXPERIMENT)
  PATH_SPLIT_SWEEP = 5,    // ... and the sampler's H x H layers too (CGS_VMC_SPLIT_BF16=2)
  PATH_CONV_GENERAL = 6,   // convolutions as im2col + GEMM over maps in HBM (conv_general.hip); every gnn
  PATH_PBDG = 7,           // ProjectedBDG (pbdg.hip): theta is the pairing matrix
  PATH_NNB = 8,            // FullyConnectedNNB (nnb.hip): the general dense trunk into determinant rows
  PATH_EDVEC = 9,          // FullVector (edvec.hip): theta is the state vector
  PATH_PRODUCT = 10,       // a product ctx (vmc_create_product): its factors run their own paths
  PATH_SYMMETRIZED = 11,   // a symmetrized ctx (vmc_create_symmetrized): its base runs its own path over the permuted rows
};
// the fused dense kernels run here: rows, sampler (and its refresh pass) and k_backprop16 with its folds
constexpr bool path_fused_dense(KernelPath p) {
  return p == PATH_FUSED || p == PATH_FUSED_LDS || p == PATH_SPLIT_ROWS || p == PATH_SPLIT_SWEEP;
}
// the dense layers run as GEMMs over the row buffers, the sampler's z1 cache is updated incrementally
constexpr bool path_general_dense(KernelPath p) { return p == PATH_DENSE_GENERAL || p == PATH_NNB; }
// more than 256 units (nnb: any width): the ctx has the general row buffers (wbuf, wide_*)
constexpr bool path_wide(KernelPath p) { return p == PATH_FUSED_LDS || path_general_dense(p); }
constexpr bool path_conv(KernelPath p) { return p == PATH_CONV || p == PATH_CONV_GENERAL; }
// no network: the kernels read theta as it lies, the dense members keep minimal shapes
constexpr bool path_no_network(KernelPath p) { return p == PATH_PBDG || p == PATH_EDVEC; }
constexpr bool path_split(KernelPath p) { return p == PATH_SPLIT_ROWS || p == PATH_SPLIT_SWEEP; }

// ------------------------------------------------------------------------------- vmc_create
struct DescPlan {
  KernelPath path;           // PATH_SPLIT_*, PATH_PRODUCT and PATH_SYMMETRIZED are never planned here (plan_split_path, vmc_create_product / _symmetrized)
  int rbm, resnet, one_d;
  int Hp;                    // padded units of the dense kernels (conv: 64, unused)
  int n_hh;                  // H x H layers
  long long P;               // parameters
  ParamLayout lay;
  ConvGeom cg;
};

// Everything vmc_create decides before it touches the device.  Returns a vmc_status; `msg` receives the
// reason.  wide_fast_allowed = false is CGS_VMC_WIDE_FAST=0.
// conv_general_pref (CGS_VMC_CONV_GENERAL): 1 the general convolution path for every shape, 0 where the fused kernels refuse
// the shape or the patch kernels beat them (plan_cgen_patch_routes), -1 only where the fused kernels refuse it
inline int plan_desc(const vmc_desc* d, bool wide_fast_allowed, DescPlan* out, char* msg, size_t msg_len,
                     int conv_general_pref = 0) {
  memset(out, 0, sizeof(*out));
#define PLAN_FAIL(code, text) do { snprintf(msg, msg_len, "%s", text); return code; } while (0)
  if (d->ansatz == VMC_ANSATZ_PRODUCT)
    PLAN_FAIL(VMC_ERR_INVALID, "a product ctx is made by vmc_create_product from two ctxs, not by vmc_create");
  if (d->ansatz == VMC_ANSATZ_SYMMETRIZED)
    PLAN_FAIL(VMC_ERR_INVALID, "a symmetrized ctx is made by vmc_create_symmetrized from a base ctx, not by vmc_create");
  if (d->ansatz < VMC_ANSATZ_FULLY_CONNECTED ||
      (d->ansatz > VMC_ANSATZ_PBDG && d->ansatz != VMC_ANSATZ_NNB && d->ansatz != VMC_ANSATZ_ED_VECTOR))
    PLAN_FAIL(VMC_ERR_UNSUPPORTED, "only the fully_connected, rbm, conv_1d/2d, res_net_1d/2d, gnn, pbdg, fully_connected_nnb and ed_vector ansatz types have HIP kernels");
  if (d->ansatz == VMC_ANSATZ_ED_VECTOR) {
    // FullVector (wavefunctions.py:1001-1080): layer_size carries the vector length; no layers, no activations
    const int rc = plan_edvec_check(d->n_sites, d->layer_size, msg, msg_len);
    if (rc != VMC_OK) return rc;
    if (d->batch_size < 1) PLAN_FAIL(VMC_ERR_INVALID, "batch_size >= 1 required");
    out->path = PATH_EDVEC;
    out->Hp = 64; out->n_hh = 0;
    out->P = plan_num_params_dense(VMC_ANSATZ_ED_VECTOR, d->n_sites, d->layer_size, 0);
    out->lay = plan_layout(false, d->n_sites, 1, 1);
    if (msg_len) msg[0] = 0;
    return VMC_OK;
  }
  if (d->ansatz == VMC_ANSATZ_NNB) {
    // FullyConnectedNNB (wavefunctions.py:931-998): the fully_connected layout with an output layer N^2 wide; always relu
    const int rc = plan_nnb_check(d->n_sites, d->num_layers, d->layer_size, d->batch_size, msg, msg_len);
    if (rc != VMC_OK) return rc;
    out->path = PATH_NNB;
    out->Hp = (d->layer_size + 63) / 64 * 64; out->n_hh = d->num_layers - 1;
    out->P = plan_num_params_dense(VMC_ANSATZ_NNB, d->n_sites, d->layer_size, d->num_layers);
    out->lay = plan_layout(false, d->n_sites, d->layer_size, d->num_layers);
    out->lay.off_bout = out->lay.off_wout + (long long)d->layer_size * d->n_sites * d->n_sites;
    if (msg_len) msg[0] = 0;
    return VMC_OK;
  }
  if (d->ansatz == VMC_ANSATZ_PBDG) {
    // ProjectedBDG (wavefunctions.py:876-928): no layers, no activations; the dense members keep minimal shapes (unused)
    const int rc = plan_pbdg_check(d->n_sites, msg, msg_len);
    if (rc != VMC_OK) return rc;
    if (d->batch_size < 1) PLAN_FAIL(VMC_ERR_INVALID, "batch_size >= 1 required");
    out->path = PATH_PBDG;
    out->Hp = 64; out->n_hh = 0;
    out->P = plan_num_params_dense(VMC_ANSATZ_PBDG, d->n_sites, 0, 0);
    out->lay = plan_layout(false, d->n_sites, 1, 1);
    if (msg_len) msg[0] = 0;
    return VMC_OK;
  }
  const bool rbm = d->ansatz == VMC_ANSATZ_RBM;
  const bool conv = d->ansatz >= VMC_ANSATZ_CONV_2D && d->ansatz <= VMC_ANSATZ_GNN;
  const bool resnet = d->ansatz == VMC_ANSATZ_RES_NET_2D || d->ansatz == VMC_ANSATZ_RES_NET_1D;
  const bool one_d = d->ansatz == VMC_ANSATZ_CONV_1D || d->ansatz == VMC_ANSATZ_RES_NET_1D;
  out->rbm = rbm; out->resnet = resnet; out->one_d = one_d;
  bool conv_general = false;
  if (d->n_sites < 2 || d->batch_size < 1 || d->num_layers < ((rbm || resnet) ? 0 : 1) || d->layer_size < 1)
    PLAN_FAIL(VMC_ERR_INVALID, "n_sites >= 2, batch_size, layer_size >= 1, num_layers >= 1 (rbm, res_net_2d: >= 0) required");
  ConvGeom& cg = out->cg;
  if (d->ansatz == VMC_ANSATZ_GNN) {
    // GraphConvNetwork (wavefunctions.py:1083-1154): a graph convolution = gather(x, adj) + snt.Conv2D with a 1 x k kernel
    // (layers.py:415-451) = a 1 x k convolution whose taps are read off the table -- the general path's im2col + GEMM
    // form with a table-driven gather (conv_general.hip).  Always the general path: the fused kernels, the band and patch
    // kernels and the implicit gather are periodic (plan_cgen_periodic).
    const int k = d->kernel_size;
    if (k < 2 || k > PLAN_GNN_MAX_K) PLAN_FAIL(VMC_ERR_UNSUPPORTED, "gnn: kernel_size (neighbours per position) must be in 2..64");
    if (d->layer_size > CONV_GENERAL_MAX_F)
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "num_conv_filters > 1024 not supported by the convolution kernels");
    if ((long long)d->num_layers > CONV_MAX_LAYERS) PLAN_FAIL(VMC_ERR_UNSUPPORTED, "too many convolutions");
    if (d->n_sites > PLAN_GNN_MAX_SITES) PLAN_FAIL(VMC_ERR_UNSUPPORTED, "gnn: num_sites beyond the general convolution path's 1023 x 1023");
    cg.K = 1; cg.KW = k; cg.D1 = 1; cg.D2 = d->n_sites; cg.N = d->n_sites; cg.F = d->layer_size;
    cg.n_conv = d->num_layers; cg.resnet = 0; cg.hact = d->nonlinearity;
    cg.GS = (4 * cg.N + 63) / 64 * 64;
    cg.NCB = (cg.F + CONV_FP - 1) / CONV_FP;
    cg.CS = 4 * cg.NCB * cg.GS;
    cg.lo = cg.hi = cg.lo2 = cg.hi2 = 0;
    cg.graph = 1;
    if ((long long)cg.N * plan_cgen_lda(cg) >= (1LL << 28))
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "num_sites x k x filters too large for the general convolution path (one sample's im2col rows beyond 1 GiB)");
    conv_general = true;
  } else if (conv) {
    // Conv2DNetwork reshapes its input to [-1, size_x, size_y, 1] (wavefunctions.py:596-597);
    // Conv1DNetwork expands [B, N] to [B, N, 1] (wavefunctions.py:511): an N x 1 lattice here
    const int sx = one_d ? d->n_sites : d->size_x, sy = one_d ? 1 : d->size_y;
    if (sx < 1 || sy < 1 || (long long)sx * sy != d->n_sites)
      PLAN_FAIL(VMC_ERR_INVALID, "size_x * size_y must equal num_sites");
    // Beyond the limits of the fused kernels (feature maps in LDS: kernel_size <= 9 -- one instantiation per size --,
    // num_conv_filters <= 64 -- four channel blocks of 16 --, a sample's two maps within 160 KiB) the general path
    // of conv_general.hip serves: feature maps in HBM, a convolution = im2col (explicit, or in the A operand's address)
    // + one GEMM (round 5: forward, local energies, sampler, the gradient accumulators of both optimizers and
    // stochastic reconfiguration through the one-call solves)
    bool general = conv_general_pref > 0;
    if (d->kernel_size < 1 || d->kernel_size > CONV_GENERAL_MAX_K)
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "kernel_size 1..31 supported by the convolution kernels");
    if (d->layer_size > CONV_GENERAL_MAX_F)
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "num_conv_filters > 1024 not supported by the convolution kernels");
    if (d->kernel_size > CONV_MAX_K || d->layer_size > CONV_FP * CONV_MAX_NCB) general = true;
    if (sx < d->kernel_size / 2 || (!one_d && sy < d->kernel_size / 2) || sx > 1023 || sy > 1023)
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "lattice sides must be in [kernel_size / 2, 1023]");
    if ((long long)d->num_layers > CONV_MAX_LAYERS)
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "too many convolutions");
    cg.K = d->kernel_size; cg.D1 = sx; cg.D2 = sy; cg.N = d->n_sites; cg.F = d->layer_size;
    cg.n_conv = resnet ? 1 + 2 * d->num_layers : d->num_layers;
    cg.resnet = resnet ? 1 : 0; cg.hact = d->nonlinearity;
    cg.GS = (4 * cg.N + 63) / 64 * 64;
    cg.NCB = (cg.F + CONV_FP - 1) / CONV_FP;
    cg.CS = 4 * cg.NCB * cg.GS;
    if (one_d) {   // layers.py:66-72: k/2 in front, k - 1 - k/2 behind (odd k: (k-1)/2 both)
      cg.KW = 1; cg.lo = cg.K / 2; cg.hi = cg.K - 1 - cg.lo; cg.lo2 = cg.hi2 = 0;
    } else {       // layers.py:132-141: (k-1)/2 in front, k/2 behind, both axes
      cg.KW = cg.K; cg.lo = cg.lo2 = (cg.K - 1) / 2; cg.hi = cg.hi2 = cg.K / 2;
    }
    if (cg.n_conv > CONV_MAX_LAYERS) PLAN_FAIL(VMC_ERR_UNSUPPORTED, "too many convolutions");
    if ((long long)d->batch_size * cg.CS >= (1LL << 31)) general = true;   // 32-bit tape offsets of the fused kernels
    if (plan_conv_rows_lds(cg, 1) > PLAN_LDS_PER_CU) general = true;       // a sample's maps beyond 160 KiB of LDS
    if (!general && conv_general_pref == 0 && plan_cgen_patch_routes(cg, d->batch_size)) general = true;   // a lattice much wider than the network's reach
    if (general && (long long)cg.N * plan_cgen_lda(cg) >= (1LL << 28))
      PLAN_FAIL(VMC_ERR_UNSUPPORTED, "lattice x kernel x filters too large for the general convolution path (one sample's im2col rows beyond 1 GiB)");
    conv_general = general;
  }
  if (d->nonlinearity < 0 || d->nonlinearity > 6 || d->output_activation < 0 || d->output_activation > 6)
    PLAN_FAIL(VMC_ERR_INVALID, "unknown activation id (layers.NONLINEARITIES has 7 entries)");
  if (rbm && d->output_activation != VMC_ACT_EXP)
    PLAN_FAIL(VMC_ERR_INVALID, "the rbm ansatz has no output_activation: it is always exp (wavefunctions.py:419-420)");
  const bool wide = !conv && d->layer_size > 256;
  const int n_hh = conv ? 0 : (rbm ? d->num_layers : d->num_layers - 1);
  // 257 .. 512 units run the fused kernels (every activation); beyond that -- or with the fused path
  // switched off or out of LDS -- the general path (every activation: its back-propagation reads f' off
  // the activation, or off the stored f'(z) for the cosine)
  bool wide_fast = false;
  if (wide && d->layer_size <= 512) {
    const int hp = (d->layer_size + 127) / 128 * 128;     // 8 waves x whole 16-unit tiles
    wide_fast = wide_fast_allowed && (n_hh == 0 || plan_tail_lds_supported(hp, n_hh)) &&
                plan_sweep_lds_required(d->n_sites, hp, n_hh, rbm) <= PLAN_LDS_PER_CU;
  }
  if (wide && d->layer_size > 4096) PLAN_FAIL(VMC_ERR_UNSUPPORTED, "fc_layer_size > 4096 is not supported");
  if (!conv && !wide) {  // the sampler keeps 16 chains' spins, z1 and operands in LDS (160 KiB per CU)
    const int hp = (d->layer_size + 63) / 64 * 64;
    const size_t need = plan_sweep_lds_required(d->n_sites, hp, n_hh, rbm);
    if (need > PLAN_LDS_PER_CU) {
      snprintf(msg, msg_len, "num_sites = %d with %d hidden units needs %zu bytes of LDS for the sampler's "
               "chain state (limit 163840)", d->n_sites, d->layer_size, need);
      return VMC_ERR_UNSUPPORTED;
    }
  }
#undef PLAN_FAIL
  out->path = conv ? (conv_general ? PATH_CONV_GENERAL : PATH_CONV)
                   : wide ? (wide_fast ? PATH_FUSED_LDS : PATH_DENSE_GENERAL) : PATH_FUSED;
  out->n_hh = n_hh;
  out->Hp = conv ? 64 : (wide_fast ? (d->layer_size + 127) / 128 * 128 : (d->layer_size + 63) / 64 * 64);
  if (conv) {
    out->P = plan_num_params_conv(cg.n_conv, cg.F, (long long)cg.K * cg.KW);
    out->lay = plan_layout(false, d->n_sites, d->layer_size, 1);     // minimal dense-side shapes (unused)
    out->n_hh = 0;
  } else {
    out->P = plan_num_params_dense(d->ansatz, d->n_sites, d->layer_size, d->num_layers);
    out->lay = plan_layout(rbm, d->n_sites, d->layer_size, d->num_layers);
  }
  if (msg_len) msg[0] = 0;
  return VMC_OK;
}

// CGS_VMC_SPLIT_BF16 = `level` on a planned ctx (EXPERIMENT: fully_connected, relu, 256 padded units, >= 1 H x H layer):
// 1 the row kernel, 2 the sampler too where sweep16_split_supported (`sweep_ok`) takes the shape; every other ctx keeps
// its path.  hact: the ctx's hidden activation.
inline KernelPath plan_split_path(const DescPlan& p, int hact, int level, bool sweep_ok) {
  if ((level != 1 && level != 2) || p.path != PATH_FUSED || p.rbm || p.Hp != 256 || p.n_hh < 1 || hact != VMC_ACT_RELU)
    return p.path;
  return level == 2 && sweep_ok ? PATH_SPLIT_SWEEP : PATH_SPLIT_ROWS;
}

// ------------------------------------------------------------------------------- gnn adjacency list
// vmc_set_adjacency's validation: the table of a ctx of n_sites sites and k taps, every entry a site
// (wavefunctions.py:1083-1154 gathers with tf.gather, which has no wrap-around: an entry outside [0, N) is an error)
inline int plan_gnn_check_adjacency(int n_sites, int k, int ctx_sites, int ctx_k, const int32_t* adj, char* msg, size_t msg_len) {
  if (!adj) { snprintf(msg, msg_len, "null adjacency list"); return VMC_ERR_INVALID; }
  if (n_sites != ctx_sites || k != ctx_k) {
    snprintf(msg, msg_len, "adjacency list of %d x %d entries, the ctx has num_sites = %d and k = %d", n_sites, k, ctx_sites, ctx_k);
    return VMC_ERR_INVALID;
  }
  for (long long i = 0; i < (long long)n_sites * k; ++i)
    if (adj[i] < 0 || adj[i] >= n_sites) {
      snprintf(msg, msg_len, "adjacency list entry [%lld][%lld] = %d outside [0, %d)", i / k, i % k, (int)adj[i], n_sites);
      return VMC_ERR_INVALID;
    }
  if (msg_len) msg[0] = 0;
  return VMC_OK;
}
// The inverse lists of a valid table, CSR: the pairs (position m, tap t) whose tap reads site n are
// idx[ptr[n] .. ptr[n + 1]), each stored as m k + t (the column block of the im2col matrix), in ascending m k + t --
// the fixed order in which k_gnn_col2im sums them.  ptr [n_sites + 1], idx [n_sites k]; a counting sort.
inline void plan_gnn_inverse(int n_sites, int k, const int32_t* adj, int32_t* ptr, int32_t* idx) {
  for (int n = 0; n <= n_sites; ++n) ptr[n] = 0;
  for (long long i = 0; i < (long long)n_sites * k; ++i) ++ptr[adj[i] + 1];
  for (int n = 0; n < n_sites; ++n) ptr[n + 1] += ptr[n];
  for (long long i = 0; i < (long long)n_sites * k; ++i) idx[ptr[adj[i]]++] = (int32_t)i;   // (ptr[n] ends at ptr[n + 1])
  for (int n = n_sites; n > 0; --n) ptr[n] = ptr[n - 1];
  ptr[0] = 0;
}

// ------------------------------------------------------------------------------- weight-gradient GEMM
#define WG_TM 64           // output tile of the batched weight-gradient kernel (k_wgrad, grad.hip)
#define WG_TN 64
#define WG_TK 32
#define WG_MAX_SPLIT 32    // workspace bound

// One problem of the batched weight-gradient launch: C[m_rows (+ ones row)][n_cols] over K samples
struct WgradShape { int m_rows, n_cols; };

// tiles of one problem (the N = 1 output / onsite problem is a one-column tile row like any other: its
// MFMAs multiply mostly zeros, but it needs no code of its own -- a VALU column sum over all samples in a
// workgroup of its own was latency bound at 190 us)
PLAN_HD inline int plan_wgrad_tiles(int m_rows, int n_cols) {
  return ((m_rows + WG_TM - 1) / WG_TM) * ((n_cols + WG_TN - 1) / WG_TN);
}

// K slices: as many as fill the CUs once (tiles x slices + the other blocks of the launch <= num_cus), each a
// whole number of WG_TK steps, at least 64 samples per slice.  forced > 0: the measurement knob
// CGS_VMC_WGRAD_SLICES
inline int plan_wgrad_slices(long long total_tiles, long long K, int num_cus, int other_blocks = 0, int forced = 0) {
  if (total_tiles <= 0) return 1;
  long long s = (num_cus - other_blocks) / total_tiles;
  if (forced > 0) s = forced;
  const long long by_k = (K + 63) / 64;
  if (s > by_k) s = by_k;
  if (s > WG_MAX_SPLIT) s = WG_MAX_SPLIT;
  if (s < 1) s = 1;
  // whole k-steps per slice; then no more slices than have samples (no slice is ever empty)
  long long kc = (K + s - 1) / s;
  kc = (kc + WG_TK - 1) / WG_TK * WG_TK;
  s = (K + kc - 1) / kc;
  return s < 1 ? 1 : (int)s;
}

// samples per slice, rounded up to whole k-steps
PLAN_HD inline int plan_wgrad_kchunk(int K, int slices) {
  int kc = (K + slices - 1) / slices;
  return (kc + WG_TK - 1) / WG_TK * WG_TK;
}

// XCD-aware block order: workgroups go to the 8 XCDs round robin by linear block id and every XCD has
// its own L2.  The W = tiles x slices work items, slice-major (all tiles of a k-slice share that slice's
// operand rows), are cut into 8 contiguous ranges of G = ceil(W / 8), one per XCD: every XCD gets the
// same number of workgroups (slices per XCD would leave XCDs idle whenever slices % 8 != 0: 5 slices
// ran on 5 of 8 XCDs) and mostly one slice's rows in its L2.  Block b -> item (b % 8) G + b / 8.
struct WgradBlock { int slice, tile; };
PLAN_HD inline WgradBlock plan_wgrad_block(int block, int tiles, int slices) {
  WgradBlock b;
  const int W = tiles * slices, G = (W + 7) / 8;
  const int j = block >> 3, w = (block & 7) * G + j;
  if (j >= G || w >= W) { b.slice = -1; b.tile = 0; return b; }
  b.slice = w / tiles;
  b.tile = w % tiles;
  return b;
}
inline int plan_wgrad_grid(int tiles, int slices) { return tiles <= 0 ? 0 : 8 * ((tiles * slices + 7) / 8); }

// MFMA tiles of the whole dense gradient launch: the output (FC) / onsite (RBM) problem
// [k_in = H or N][1], n_hh hidden problems [H][H], the first layer [N][H]
// out_in_tiles: the N = 1 layer (w_out, b_out / w_on, b_on) is one of the tile problems; false: its sums come
// from the back-propagation kernel's per-workgroup partials and are folded by plan_wgrad_fold_blocks(H)
// workgroups of the same launch (fully_connected on the fused kernels)
// (neural-network backflow: the output problem is the pairing layer [H][N^2])
inline int plan_nnb_wgrad_total_tiles(int N, int H, int n_hh) {
  return plan_wgrad_tiles(H, N * N) + n_hh * plan_wgrad_tiles(H, H) + plan_wgrad_tiles(N, H);
}
inline int plan_wgrad_total_tiles(int N, int H, int n_hh, bool rbm, bool out_in_tiles = true) {
  return (out_in_tiles ? plan_wgrad_tiles(rbm ? N : H, 1) : 0) + n_hh * plan_wgrad_tiles(H, H) + plan_wgrad_tiles(N, H);
}
#define WG_FOLD_OUT 128    // outputs (two sums x (H weights + bias)) per fold workgroup, four row groups each
inline int plan_wgrad_fold_blocks(int H) { return (2 * (H + 1) + WG_FOLD_OUT - 1) / WG_FOLD_OUT; }

// floats of the partial-tile workspace: [tiles][slices][2 x WG_TM x WG_TN + 2 x WG_TN]
inline long long plan_wgrad_ws_floats(long long tiles, int slices) {
  return tiles * slices * 2 * ((long long)WG_TM * WG_TN + WG_TN);
}

// ------------------------------------------------------------------------------- stochastic reconfiguration
#define RD_MAXB 16         // problems per row-dot launch
#define RD_TM 128          // samples per row-dot tile

// dispatch order of the row-dot problems of one launch: largest K first (list scheduling: the light
// tiles fill the end), stable; first_tile[j] = first tile of the j-th dispatched problem
inline int plan_rowdot_schedule(const int* K, const int* M, int n, int* order, int* first_tile) {
  for (int j = 0; j < n; ++j) order[j] = j;
  for (int a = 1; a < n; ++a)
    for (int b = a; b > 0 && K[order[b]] > K[order[b - 1]]; --b) {
      const int tmp = order[b]; order[b] = order[b - 1]; order[b - 1] = tmp;
    }
  int tiles = 0;
  for (int j = 0; j < n; ++j) {
    first_tile[j] = tiles;
    tiles += (M[order[j]] + RD_TM - 1) / RD_TM;
  }
  first_tile[n] = tiles;
  return tiles;
}

inline int plan_sr_wsum_slices(int R, int num_cus) {
  int s = (R + 63) / 64;              // at least 64 samples per slice
  if (s > num_cus) s = num_cus;
  return s < 1 ? 1 : s;
}

// Sample-space solve (srgram.hip): T = O O^T of the n stored samples in SRG_TILE x SRG_TILE tiles, one workgroup of eight
// waves per tile, only the tiles (i, j) with j >= i (the tile is mirrored from the same registers).  The workgroups
// form a linear grid over the upper triangle row by row: row i holds the nt - i tiles (i, i) .. (i, nt - 1).  A
// workgroup stages the row panels of both tile sides through LDS in chunks of SRG_KC columns, rows SRG_LD floats apart
// (16-byte aligned rows for the four-float fragment reads).
#define SRG_TILE 128
#define SRG_KC 32
#define SRG_LD (SRG_KC + 4)
#define SRG_MAX_N 16384     // T is n^2 floats: 1 GiB here; beyond, the parameter-space solver (vmc_sr_solve)
#define SRG_MAX_TERMS 32    // layer terms of one launch (kernel argument table)

struct SrGramPlan {
  int nt;                   // tiles per side
  long long grid;           // workgroups: nt (nt + 1) / 2
  size_t lds_bytes;         // per workgroup: the two row panels of a chunk
};

PLAN_HD inline size_t plan_sr_gram_lds_bytes() { return (size_t)2 * SRG_TILE * SRG_LD * sizeof(float); }

// VMC_OK and the plan, or the refusal (n < 1; n > SRG_MAX_N) with its text
inline int plan_sr_gram(long long n, SrGramPlan* p, char* msg, size_t msg_len) {
  if (n < 1) { snprintf(msg, msg_len, "no stored samples"); return VMC_ERR_STATE; }
  if (n > SRG_MAX_N) {
    snprintf(msg, msg_len, "the sample-space solve holds the n x n Gram matrix of the stored samples: n = %lld > %d "
                           "(use the parameter-space solver, vmc_sr_solve)", n, SRG_MAX_N);
    return VMC_ERR_UNSUPPORTED;
  }
  p->nt = (int)((n + SRG_TILE - 1) / SRG_TILE);
  p->grid = (long long)p->nt * (p->nt + 1) / 2;
  p->lds_bytes = plan_sr_gram_lds_bytes();
  if (p->lds_bytes > PLAN_LDS_PER_CU) { snprintf(msg, msg_len, "Gram tile panels exceed the LDS of a CU"); return VMC_ERR_UNSUPPORTED; }
  return VMC_OK;
}

// workgroup idx of the linear grid -> its tile (i, j), j >= i
PLAN_HD inline void plan_sr_gram_tile(long long idx, int nt, int* i, int* j) {
  int r = 0;
  while (idx >= nt - r) { idx -= nt - r; ++r; }
  *i = r; *j = r + (int)idx;
}
