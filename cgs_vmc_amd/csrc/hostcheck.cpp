// hostcheck.cpp -- the host-side planners of libcgsvmc_hip.so (plan.hpp: parameter layouts, vmc_create's
// shape / LDS validation, convolution group / band / slice pickers, the sampler's LDS plan, split-K and
// XCD block-order maps, SR tile schedules, buffer sizes) driven over a grid of shapes on the CPU under
// AddressSanitizer + UndefinedBehaviourSanitizer (GPU sanitizers are not available on this pool):
//     make -C cgs_vmc_amd/csrc hostcheck        (g++ -fsanitize=address,undefined; tests/test_hostcheck.py)
// Every index a kernel derives from these plans is re-derived here into REAL arrays of the planned
// size, so that an offset one past a buffer is an ASan report and an overflowing product a UBSan one.
// The grid contains all five BASELINE configurations and the limits of include/cgsvmc.h (512 / 4096
// units, 64 filters, kernel 9, 32 x 32 lattices, 1023-site chains).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.hpp"

static long long g_checks = 0, g_shapes = 0, g_rejected = 0, g_general = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    ++g_checks;                                                                          \
    if (!(cond)) { fprintf(stderr, "hostcheck FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
  } while (0)

static const int kCus[] = {256, 304, 64, 1};

static vmc_desc dense_desc(int ansatz, int n, int b, int L, int h, int act, int oact) {
  vmc_desc d;
  memset(&d, 0, sizeof(d));
  d.n_sites = n; d.batch_size = b; d.num_layers = L; d.layer_size = h;
  d.nonlinearity = act; d.output_activation = oact; d.ansatz = ansatz;
  return d;
}

// every piece of the parameter vector lands in [0, P), the pieces are disjoint and cover it
static void check_layout(const DescPlan& p, long long N, long long H) {
  const ParamLayout& lay = p.lay;
  const long long P = p.P;
  CHECK(P > 0);
  if (P > 6000000) {       // too large to mark: the pieces are consecutive, so the ends tell everything
    const long long last = p.rbm ? plan_off_b(lay, H, lay.n_hh) + H : lay.off_bout + 1;
    CHECK(last == P);
    CHECK(lay.off_w1 >= 0 && lay.off_b1 == lay.off_w1 + N * H && lay.off_h0 == lay.off_b1 + H);
    return;
  }
  std::vector<unsigned char> mark((size_t)P, 0);
  auto piece = [&](long long off, long long n) {
    CHECK(off >= 0 && off + n <= P);
    for (long long i = 0; i < n; ++i) { CHECK(mark[(size_t)(off + i)] == 0); mark[(size_t)(off + i)] = 1; }
  };
  piece(lay.off_w1, N * H); piece(lay.off_b1, H);
  for (int l = 1; l <= lay.n_hh; ++l) { piece(plan_off_w(lay, H, l), H * H); piece(plan_off_b(lay, H, l), H); }
  if (p.rbm) { CHECK(lay.off_wout == -1); piece(lay.off_won, N); piece(lay.off_bout, 1); }
  else { CHECK(lay.off_won == -1); piece(lay.off_wout, H); piece(lay.off_bout, 1); }
  for (long long i = 0; i < P; ++i) CHECK(mark[(size_t)i] == 1);
}

// XCD-aware block order: a bijection onto (slice, tile); every XCD gets the same number of work items
// (+- 1 range), contiguous in slice-major order
static void check_block_maps() {
  for (int tiles : {1, 4, 8, 16, 20, 33, 44})
    for (int slices : {1, 5, 7, 8, 9, 12, 32}) {
      const int grid = plan_wgrad_grid(tiles, slices), W = tiles * slices;
      CHECK(grid % 8 == 0 && grid >= W && grid < W + 8 * 8);
      std::vector<int> hit((size_t)W, 0), per_xcd(8, 0), last(8, -1);
      for (int b = 0; b < grid; ++b) {
        const WgradBlock m = plan_wgrad_block(b, tiles, slices);
        if (m.slice < 0) continue;
        CHECK(m.slice < slices && m.tile >= 0 && m.tile < tiles);
        const int w = m.slice * tiles + m.tile;
        hit[(size_t)w] += 1;
        per_xcd[(size_t)(b & 7)] += 1;
        CHECK(w > last[(size_t)(b & 7)]);               // one XCD walks a contiguous, ascending range
        last[(size_t)(b & 7)] = w;
      }
      for (int v : hit) CHECK(v == 1);
      const int G = (W + 7) / 8;
      for (int x = 0; x < 8; ++x) CHECK(per_xcd[(size_t)x] <= G && (per_xcd[(size_t)x] == G || (x + 1) * G > W));
    }
}

// the batched weight-gradient kernel: tiles, K slices and their chunks, the partial-tile workspace and
// the (tile -> problem, m-tile, n-tile) walk of k_wgrad
// (out_in_tiles = false: the output layer's sums come from the back-propagation kernel's partials and are
// folded by extra workgroups of the launch -- fully_connected on the fused kernels)
static void check_wgrad(long long N, long long H, int n_hh, bool rbm, long long B, bool out_in_tiles = true) {
  struct Prob { int k_in, n_out, tile0; };
  std::vector<Prob> probs;
  int tile0 = 0;
  auto add = [&](int k_in, int n_out) { probs.push_back({k_in, n_out, tile0}); tile0 += plan_wgrad_tiles(k_in, n_out); };
  if (out_in_tiles) add(rbm ? (int)N : (int)H, 1);
  for (int l = 0; l < n_hh; ++l) add((int)H, (int)H);
  add((int)N, (int)H);
  const long long tiles = tile0;
  CHECK(tiles == plan_wgrad_total_tiles((int)N, (int)H, n_hh, rbm, out_in_tiles) && tiles >= 1);
  const int other = 1 + (out_in_tiles ? 0 : plan_wgrad_fold_blocks((int)H));
  if (!out_in_tiles) {   // wgrad_fold_out: every output (two sums x (H weights + bias)) in exactly one (block, lane)
    const int nb = plan_wgrad_fold_blocks((int)H), n_out = 2 * ((int)H + 1);
    CHECK(nb >= 1 && nb * WG_FOLD_OUT >= n_out && (nb - 1) * WG_FOLD_OUT < n_out && 4 * WG_FOLD_OUT == 512);
    const int n_wg = (int)((B + 15) / 16), per = (n_wg + 3) >> 2;
    int covered = 0;
    for (int gq = 0; gq < 4; ++gq) { const int i0 = gq * per, i1 = std::min(n_wg, i0 + per); covered += i1 > i0 ? i1 - i0 : 0; }
    CHECK(covered == n_wg);
  }
  // every tile belongs to exactly one problem and lies inside its output; together they cover it
  for (const Prob& p : probs) {
    const int tn = (p.n_out + WG_TN - 1) / WG_TN, nt = plan_wgrad_tiles(p.k_in, p.n_out);
    for (int t = p.tile0; t < p.tile0 + nt; ++t) {
      int pi = 0;
      for (size_t i = 0; i < probs.size(); ++i)
        if (t >= probs[i].tile0) pi = (int)i;
      CHECK(&probs[(size_t)pi] == &p);
      const int lt = t - p.tile0, tm = lt / tn, tnn = lt % tn;
      CHECK(tm * WG_TM < p.k_in && tnn * WG_TN < p.n_out);
    }
    CHECK((long long)((p.k_in + WG_TM - 1) / WG_TM) * tn == nt);
  }
  for (int cus : kCus)
    for (int forced : {0, 1, 3, 12, 100}) {
      const int s = plan_wgrad_slices(tiles, B, cus, other, forced);
      CHECK(s >= 1 && s <= WG_MAX_SPLIT);
      if (!forced) CHECK(s == 1 || tiles * s + other <= cus);
      const int kc = plan_wgrad_kchunk((int)B, s);
      CHECK(kc % WG_TK == 0 && (long long)kc * s >= B);
      CHECK((long long)kc * (s - 1) < B);                 // no slice is empty
      // the last float the last slice of the last tile writes (second product's ones row)
      const long long part = 2 * ((long long)WG_TM * WG_TN + WG_TN);      // WG_PART of grad.hip
      const long long last = ((tiles - 1) * s + (s - 1)) * part + (part - 1);
      CHECK(tiles == 0 || last < plan_wgrad_ws_floats(tiles, WG_MAX_SPLIT));
    }
}

static void check_sweep(const vmc_desc& d, const DescPlan& p) {
  if (path_conv(p.path) || path_general_dense(p.path)) return;
  const int NT = p.Hp / 16;
  CHECK(NT == 4 || NT == 8 || NT == 12 || NT == 16 || NT == 24 || NT == 32);   // the instantiated tile counts
  const int NW = (NT == 16 || NT >= 24) ? 8 : 4;
  const size_t need = plan_sweep_lds_required(d.n_sites, p.Hp, p.n_hh, p.rbm != 0);
  CHECK(need <= PLAN_LDS_PER_CU);
  for (int no_w1l = 0; no_w1l < 2; ++no_w1l)
    for (int plain = 0; plain < 2; ++plain)
      for (int tuned = 0; tuned < 2; ++tuned) {
        const SweepPlan sp = plan_sweep(d.n_sites, NT, NW, p.n_hh, p.rbm != 0, no_w1l != 0, plain != 0, tuned != 0);
        CHECK(sp.ok == 1);
        CHECK(sp.lds <= PLAN_LDS_PER_CU && sp.lds >= (sp.w1l ? (size_t)0 : need));
        CHECK(sp.fast == 0 || sp.fast == 2 || sp.fast == 4);
        CHECK(!(sp.w1l && (NT > 16 || no_w1l)));
        CHECK(!(sp.fast && (!plain || !tuned)));
        if (sp.fast == 2) CHECK((d.n_sites + 3) / 4 <= 32);      // two Philox draws cover 256 sites
        if (sp.fast == 4) CHECK((d.n_sites + 3) / 4 <= 64);
        if (sp.w1l) CHECK(sp.lds == plan_sweep_lds_bytes(d.n_sites, p.Hp, p.n_hh, true, p.rbm != 0));
      }
  if (p.path == PATH_FUSED_LDS && p.n_hh >= 1) {
    CHECK(plan_tail_lds_supported(p.Hp, p.n_hh));
    CHECK(plan_tail_lds_bytes(p.Hp, p.n_hh) <= PLAN_LDS_PER_CU);
  }
  // the eight-chain sampler (sweep8.hip): its shapes, its LDS, and the tile rule
  for (int no_w1l = 0; no_w1l < 2; ++no_w1l) {
    const Sweep8Plan s8 = plan_sweep8(d.n_sites, p.Hp, p.n_hh, no_w1l != 0);
    if (s8.ok) {
      CHECK(p.Hp == 128 || p.Hp == 256);
      CHECK(p.n_hh >= 1 && d.n_sites <= p.Hp && d.n_sites <= 256);        // one Philox site block per lane of a chain's group
      CHECK(s8.lds <= PLAN_LDS_PER_CU && s8.lds == plan_sweep8_lds_bytes(d.n_sites, p.Hp, p.n_hh, s8.w1l != 0));
      CHECK(!(s8.w1l && no_w1l));
      // every array of the kernel's LDS carve-up starts on a 16-byte boundary
      const size_t nst = (size_t)((d.n_sites + 3) & ~3);
      CHECK((8 * nst) % 4 == 0 && (2 * 8 * ((size_t)p.Hp + 16)) % 4 == 0 && ((size_t)p.Hp + 16) % 4 == 0 && ((size_t)p.Hp + 4) % 4 == 0);
    } else {
      CHECK(s8.lds == 0 && s8.w1l == 0);
    }
    for (int forced : {0, 8, 16}) {
      const int tile = plan_sweep_tile(d.batch_size, 256, s8.ok != 0, forced);
      CHECK(tile == 8 || tile == 16);
      if (!s8.ok || forced == 16) CHECK(tile == 16);
      if (s8.ok && forced == 8) CHECK(tile == 8);
      if (s8.ok && forced == 0) CHECK((tile == 8) == ((d.batch_size + 15) / 16 <= 128));
      if (tile == 8 && forced == 0) CHECK((d.batch_size + 7) / 8 <= 256);   // never more eight-chain tiles than CUs by the rule itself
    }
  }
}

// The nine flags (and the product pointer) vmc_ctx held before KernelPath, per path, exactly as the ternary of the old
// vmc_debug_kernel_path related them.  Every predicate of plan.hpp, and every single-path test that replaced a flag, must
// equal the boolean expression over the flags it replaced.
struct OldFlags { int path; bool conv, conv_general, wide, wide_fast, split, split_sweep, pbdg, nnb, edvec, prod; };
static const OldFlags kOldFlags[11] = {
    //    conv cgen wide fast split ssweep pbdg nnb edvec prod
    {0,   0,   0,   0,   0,   0,    0,     0,   0,  0,    0},
    {1,   0,   0,   1,   1,   0,    0,     0,   0,  0,    0},
    {2,   0,   0,   1,   0,   0,    0,     0,   0,  0,    0},
    {3,   1,   0,   0,   0,   0,    0,     0,   0,  0,    0},
    {4,   0,   0,   0,   0,   1,    0,     0,   0,  0,    0},
    {5,   0,   0,   0,   0,   1,    1,     0,   0,  0,    0},
    {6,   1,   1,   0,   0,   0,    0,     0,   0,  0,    0},
    {7,   0,   0,   0,   0,   0,    0,     1,   0,  0,    0},
    {8,   0,   0,   1,   0,   0,    0,     0,   1,  0,    0},      // nnb: the general dense path (wide, never wide_fast)
    {9,   0,   0,   0,   0,   0,    0,     0,   0,  1,    0},
    {10,  0,   0,   0,   0,   0,    0,     0,   0,  0,    1},      // a product starts from a minimal fully_connected ctx
};

static void path_truth_table() {
  for (const OldFlags& f : kOldFlags) {
    // the row is what the old ternary said
    const int old_path = f.prod ? 10 : f.edvec ? 9 : f.nnb ? 8 : f.pbdg ? 7 : f.conv ? (f.conv_general ? 6 : 3)
                       : (f.wide ? (f.wide_fast ? 1 : 2) : (f.split ? (f.split_sweep ? 5 : 4) : 0));
    CHECK(old_path == f.path);
    const KernelPath p = (KernelPath)f.path;
    CHECK(&f == &kOldFlags[p]);
    // the named predicates (the fused-dense one was only ever asked where a product had been sent elsewhere)
    CHECK(path_fused_dense(p) == (!f.prod && !f.conv && !f.pbdg && !f.edvec && !(f.wide && !f.wide_fast)));
    CHECK(path_general_dense(p) == (f.wide && !f.wide_fast));
    CHECK(path_wide(p) == f.wide);
    CHECK(path_conv(p) == f.conv);
    CHECK(path_no_network(p) == (f.pbdg || f.edvec));
    CHECK(path_split(p) == f.split);
    // the single paths that stand where a flag stood
    CHECK((p == PATH_CONV_GENERAL) == f.conv_general && (p == PATH_CONV) == (f.conv && !f.conv_general));
    CHECK((p == PATH_FUSED_LDS) == (f.wide && f.wide_fast) && (p == PATH_DENSE_GENERAL) == (f.wide && !f.wide_fast && !f.nnb));
    CHECK((p == PATH_SPLIT_SWEEP) == f.split_sweep && (p == PATH_SPLIT_ROWS) == (f.split && !f.split_sweep));
    CHECK((p == PATH_PBDG) == f.pbdg && (p == PATH_NNB) == f.nnb && (p == PATH_EDVEC) == f.edvec && (p == PATH_PRODUCT) == f.prod);
    // vmc_create's compounds: the eight-chain sampler's families, the families CGS_VMC_OVERLAP may switch on
    CHECK((p == PATH_FUSED || p == PATH_SPLIT_ROWS) == (!f.prod && !f.conv && !f.wide && !(f.pbdg || f.edvec) && !f.split_sweep));
    CHECK((!path_conv(p) && !path_wide(p) && !path_no_network(p)) == (!f.conv && !f.wide && !(f.pbdg || f.edvec)));
    // the sampler leaves an exact cache
    CHECK(!path_general_dense(p) == (!f.wide || f.wide_fast));
  }
}

// plan_split_path against its condition, written out: CGS_VMC_SPLIT_BF16 = 1 | 2 on fully_connected, relu, 256 padded units,
// at least one H x H layer -- neither convolutional nor wide nor rbm; level 2 reaches the sampler only where it is supported
static void check_split(const DescPlan& p, int ansatz, int h, int act) {
  for (int level : {-1, 0, 1, 2, 3})
    for (int sweep_ok = 0; sweep_ok < 2; ++sweep_ok) {
      const bool split = (level == 1 || level == 2) && ansatz == VMC_ANSATZ_FULLY_CONNECTED && h <= 256 && p.Hp == 256 &&
                         p.n_hh >= 1 && act == VMC_ACT_RELU;
      const KernelPath want = !split ? p.path : (level == 2 && sweep_ok) ? PATH_SPLIT_SWEEP : PATH_SPLIT_ROWS;
      CHECK(plan_split_path(p, act, level, sweep_ok != 0) == want);
    }
}

static void dense_grid() {
  const int sites[] = {2, 4, 10, 16, 36, 100, 144, 256, 400, 1024};
  const int units[] = {1, 7, 32, 64, 80, 128, 200, 256, 257, 300, 384, 400, 512, 513, 1024, 4096, 4097};
  const int layers[] = {0, 1, 2, 3, 6};
  const long long batches[] = {1, 64, 1000, 4096, 32768};
  char msg[256];
  for (int ansatz : {VMC_ANSATZ_FULLY_CONNECTED, VMC_ANSATZ_RBM})
    for (int n : sites)
      for (int h : units)
        for (int L : layers)
          for (int act : {VMC_ACT_RELU, VMC_ACT_COS, VMC_ACT_TANH}) {
            const vmc_desc d = dense_desc(ansatz, n, 4096, L, h, act, VMC_ACT_EXP);
            DescPlan p;
            for (int wf = 0; wf < 2; ++wf) {
              const int rc = plan_desc(&d, wf != 0, &p, msg, sizeof(msg));
              ++g_shapes;
              if (rc != VMC_OK) {
                ++g_rejected;
                CHECK(msg[0] != 0 && (rc == VMC_ERR_INVALID || rc == VMC_ERR_UNSUPPORTED));
                if (ansatz == VMC_ANSATZ_FULLY_CONNECTED && L == 0) CHECK(rc == VMC_ERR_INVALID);
                continue;
              }
              CHECK(h <= 4096 && !(L == 0 && ansatz == VMC_ANSATZ_FULLY_CONNECTED));
              CHECK(p.Hp >= h && p.Hp % 64 == 0 && p.Hp - h < 128);
              CHECK(path_wide(p.path) == (h > 256));
              CHECK(p.path != PATH_FUSED_LDS || (wf && h > 256 && h <= 512 && (p.Hp == 384 || p.Hp == 512)));
              {   // the path decision, written out: <= 256 units fused; 257 .. 512 the LDS-operand kernels where they are
                  // allowed and fit; the general GEMM path otherwise
                const int n_hh = ansatz == VMC_ANSATZ_RBM ? L : L - 1, hp = (h + 127) / 128 * 128;
                const bool fast = wf && h > 256 && h <= 512 && (n_hh == 0 || plan_tail_lds_supported(hp, n_hh)) &&
                                  plan_sweep_lds_required(n, hp, n_hh, ansatz == VMC_ANSATZ_RBM) <= PLAN_LDS_PER_CU;
                CHECK(p.path == (h <= 256 ? PATH_FUSED : fast ? PATH_FUSED_LDS : PATH_DENSE_GENERAL));
                check_split(p, ansatz, h, act);
              }
              CHECK(p.n_hh == (ansatz == VMC_ANSATZ_RBM ? L : L - 1) && p.lay.n_hh == p.n_hh);
              CHECK(p.P == plan_num_params_dense(ansatz, n, h, L));
              check_layout(p, n, h);
              check_sweep(d, p);
              for (long long b : batches) {
                check_wgrad(n, h, p.n_hh, p.rbm != 0, b);
                if (!p.rbm && !path_general_dense(p.path)) check_wgrad(n, h, p.n_hh, false, b, false);
              }
            }
          }
  // the limits of include/cgsvmc.h, and what lies one step beyond them
  DescPlan p;
  vmc_desc d = dense_desc(VMC_ANSATZ_FULLY_CONNECTED, 100, 4096, 3, 4097, VMC_ACT_RELU, VMC_ACT_EXP);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  d = dense_desc(VMC_ANSATZ_FULLY_CONNECTED, 100, 4096, 3, 513, VMC_ACT_COS, VMC_ACT_EXP);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.path == PATH_DENSE_GENERAL);     // the general path has every activation
  d = dense_desc(VMC_ANSATZ_FULLY_CONNECTED, 100, 4096, 3, 512, VMC_ACT_COS, VMC_ACT_EXP);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.path == PATH_FUSED_LDS && p.Hp == 512);
  CHECK(plan_desc(&d, false, &p, msg, sizeof(msg)) == VMC_OK && p.path == PATH_DENSE_GENERAL);
  d = dense_desc(VMC_ANSATZ_RBM, 100, 4096, 2, 256, VMC_ACT_RELU, VMC_ACT_TANH);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_INVALID);
  d = dense_desc(VMC_ANSATZ_FULLY_CONNECTED, 100, 4096, 3, 256, 7, VMC_ACT_EXP);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_INVALID);
  d = dense_desc(8, 100, 4096, 3, 256, 0, VMC_ACT_EXP);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  // BASELINE configs 1 - 5 (config 4 = config 3 per rank)
  const int cfg[4][4] = {{16, 64, 2, 32}, {36, 1024, 3, 128}, {100, 4096, 3, 256}, {256, 1024, 6, 256}};
  for (auto& c : cfg) {
    d = dense_desc(VMC_ANSATZ_FULLY_CONNECTED, c[0], c[1], c[2], c[3], VMC_ACT_RELU, VMC_ACT_EXP);
    CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && !path_wide(p.path));
  }
  d = dense_desc(VMC_ANSATZ_FULLY_CONNECTED, 100, 4096, 3, 256, VMC_ACT_RELU, VMC_ACT_EXP);
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.P == 157697);
  const SweepPlan sp = plan_sweep(100, 16, 8, 2, false, false, true, true);
  CHECK(sp.ok && sp.w1l && sp.fast == 2);                     // config 3: W1 in LDS, two Philox draws per lane
  // BASELINE configs 2 and 5 (1,024 chains per GPU) take eight-chain tiles, config 3 (4,096) sixteen-chain tiles
  const Sweep8Plan c2 = plan_sweep8(36, 128, 2, false), c5 = plan_sweep8(256, 256, 5, false);
  CHECK(c2.ok && c2.w1l && c5.ok && !c5.w1l);                 // 16 x 16 sites: W1 (266 KB) stays in L2
  CHECK(plan_sweep_tile(1024, 256, true, 0) == 8 && plan_sweep_tile(4096, 256, true, 0) == 16 && plan_sweep_tile(2048, 256, true, 0) == 8);
  CHECK(!plan_sweep8(300, 256, 2, false).ok && !plan_sweep8(100, 256, 0, false).ok && !plan_sweep8(100, 192, 2, false).ok);
}

// index of (site, channel) in a feature map; wrap of a periodic coordinate
static long long fmap_index(const ConvGeom& g, int site, int c) { return (long long)(c / 4) * g.GS + 4 * site + c % 4; }
static int wrap(int v, int n) { v %= n; return v < 0 ? v + n : v; }

static void check_conv(const vmc_desc& d, const DescPlan& p) {
  const ConvGeom& g = p.cg;
  const long long B = d.batch_size;
  const int KK = g.K * g.KW, CW = 16 * g.NCB;
  CHECK(g.N == g.D1 * g.D2 && g.GS >= 4 * g.N && g.GS % 64 == 0 && g.CS == 4 * g.NCB * g.GS);
  CHECK(g.NCB >= 1 && g.NCB <= CONV_MAX_NCB && g.F <= CW && g.n_conv >= 1 && g.n_conv <= CONV_MAX_LAYERS);
  CHECK(g.lo + g.hi == g.K - 1 && g.lo2 + g.hi2 == g.KW - 1);
  CHECK(B * g.CS < (1LL << 31));
  {  // the feature-map layout is injective into [0, CS)
    std::vector<unsigned char> mark((size_t)g.CS, 0);
    for (int s = 0; s < g.N; ++s)
      for (int c = 0; c < CW; ++c) {
        const long long i = fmap_index(g, s, c);
        CHECK(i >= 0 && i < g.CS && mark[(size_t)i] == 0);
        mark[(size_t)i] = 1;
      }
  }
  CHECK(p.P == plan_num_params_conv(g.n_conv, g.F, KK));
  {  // k_conv_pack: every theta element it reads is inside the parameter vector, every image element
     // it writes inside the planned image
    const long long p0 = (long long)KK * g.F + g.F, pl = (long long)KK * g.F * g.F + g.F, Q0 = (KK + 3) / 4;
    CHECK(plan_conv_w0_floats(g) == (long long)g.NCB * Q0 * 64);
    long long max_theta = -1;
    for (long long i = 0; i < (long long)g.NCB * Q0 * 64; ++i) {
      const int cb = (int)(i / (Q0 * 64)), q = (int)((i / 64) % Q0), lane = (int)(i % 64), m = lane & 15, gq = lane >> 4;
      const int tap = 4 * q + gq, co = 16 * cb + m;
      if (tap < KK && co < g.F) max_theta = std::max(max_theta, (long long)tap * g.F + co);
    }
    CHECK(max_theta < p0);
    for (int l = 0; l < g.n_conv; ++l) {
      const long long base = l == 0 ? (long long)KK * g.F : p0 + (long long)(l - 1) * pl + (long long)KK * g.F * g.F;
      CHECK(base + g.F <= p.P);
    }
    CHECK(plan_conv_bias_floats(g) == (long long)g.n_conv * 16 * g.NCB);
    const long long per_layer = (long long)KK * 256 * g.NCB * g.NCB;
    CHECK((long long)(g.n_conv - 1) * per_layer <= plan_conv_wf_floats(g));
    if (g.n_conv > 1) {
      const long long wlast = p0 + (long long)(g.n_conv - 2) * pl;     // [tap][cin][cout] of the last convolution
      CHECK(wlast + ((long long)(KK - 1) * g.F + (g.F - 1)) * g.F + (g.F - 1) < p.P);
    }
  }
  const int nw = plan_conv_waves(g);
  CHECK(nw == 4 || nw == 8);
  for (int one = 0; one < 2; ++one) {
    const size_t cap = plan_conv_lds_cap(g, one != 0);
    CHECK(cap == CONV_LDS_PER_WG || cap == PLAN_LDS_PER_CU);
    const int G = plan_conv_pick_group(g, nw, one != 0);
    CHECK(G >= 1 && G <= 64 && plan_conv_rows_lds(g, G) <= cap);
    for (int cus : kCus) {
      const int Gs = plan_conv_pick_sweep_group(g, B, cus, nw, one != 0);
      CHECK(Gs >= 1 && Gs <= 64 && Gs <= B && plan_conv_rows_lds(g, Gs) <= cap);
      const int grid = plan_conv_grid(g, B * 7, G, cus);
      CHECK(grid >= 1 && grid <= 2 * cus && (long long)grid * G <= B * 7 + G);
      const int sl = plan_conv_dw_slices(g, B, cus);
      CHECK(sl >= 1 && sl <= 256 && sl <= B);
      {  // grid z of k_conv_dw: the output block groups x item parts cover every block and every item
         // once, with at most PLAN_DW_MAX_ACC accumulator pairs per wave
        const int nco = plan_conv_dw_nco(g), parts = plan_conv_dw_parts(g.K, g.KW, g.NCB);
        CHECK(nco >= 1 && g.NCB % nco == 0 && parts >= 1 && plan_conv_dw_grid_z(g) == (g.NCB / nco) * parts);
        const int ni = KK + 1, tpw = (ni + PLAN_DW_WAVES * parts - 1) / (PLAN_DW_WAVES * parts);
        CHECK(tpw * g.NCB * nco <= PLAN_DW_MAX_ACC);
        std::vector<int> seen((size_t)ni, 0);
        for (int part = 0; part < parts; ++part)
          for (int i = 0; i < tpw; ++i)
            for (int w = 0; w < PLAN_DW_WAVES; ++w) {
              const int it = w + (part * tpw + i) * PLAN_DW_WAVES;
              if (it < ni) ++seen[(size_t)it];
            }
        for (int it = 0; it < ni; ++it) CHECK(seen[(size_t)it] == 1);
        CHECK((KK + 15) / 16 <= PLAN_DW_WAVES);       // the first layer's tap tiles: one per wave, one part
      }
      // weight-gradient workspace: the last element slice sl-1 / layer n_conv-1 / second sum writes
      const long long rows = (long long)KK * CW + 1, ws = plan_conv_dw_ws_floats(g, sl);
      const long long last = ((((long long)(sl - 1) * g.n_conv + (g.n_conv - 1)) * 2) + 1) * rows * CW + (rows * CW - 1);
      CHECK(last == ws - 1);
      // k_conv_dw_reduce's source index of the last weight and the last bias
      CHECK(((long long)(KK - 1) * CW + (g.F - 1)) * CW + (g.F - 1) < rows * CW);
      CHECK((long long)KK * CW * CW + (g.F - 1) < rows * CW);
    }
  }
  // weight-gradient bands: a band always exists, fits, and its padded numbering stays inside its maps
  for (int forced : {0, 1, 3}) {
    const int rb = plan_conv_dw_band(g, forced);
    CHECK(rb >= 1 && rb <= g.D1 && plan_conv_dw_lds(g, rb) <= PLAN_LDS_PER_CU);
    if (forced >= 1 && forced < g.D1) CHECK(rb <= forced);
    const int D2p = g.D2 + g.KW - 1, NPAD = (g.D1 + g.K - 1) * D2p;
    const int NQ = (rb * D2p + 3) & ~3, NIN = NQ + (g.K - 1) * D2p + g.KW;
    std::vector<int> s_map((size_t)NPAD), s_pos((size_t)g.N);
    for (int i = 0; i < NPAD; ++i) {
      const int p1 = i / D2p, p2 = i - p1 * D2p;
      s_map[(size_t)i] = wrap(p1 - g.lo, g.D1) * g.D2 + wrap(p2 - g.lo2, g.D2);
      CHECK(s_map[(size_t)i] >= 0 && s_map[(size_t)i] < g.N);
    }
    for (int i = 0; i < g.N; ++i) {
      const int a1 = i / g.D2;
      s_pos[(size_t)i] = a1 * D2p + (i - a1 * g.D2);
      CHECK(s_pos[(size_t)i] < NPAD);
    }
    // a band of rb rows starting at row r0: position q of the band + tap offset < NIN
    const int q_last = (rb - 1) * D2p + (g.D2 - 1);
    CHECK(q_last < NQ && q_last + (g.K - 1) * D2p + (g.KW - 1) < NIN);
    const int CWD = 16 * plan_conv_dw_nco(g);
    const size_t floats = ((size_t)NQ * CWD + (size_t)NIN * CW + NPAD + g.N + CW + 8 * CW);
    // the walk reads delta one quad past the end (dropped): NQ + 4 positions of CWD floats stay inside the LDS
    CHECK(((size_t)NQ + 4) * CWD <= floats);
    CHECK(floats * sizeof(float) == plan_conv_dw_lds(g, rb));
  }
}

static void conv_grid() {
  struct Lat { int x, y; };
  const Lat lats[] = {{4, 4}, {3, 5}, {6, 6}, {10, 10}, {16, 16}, {24, 24}, {30, 30}, {32, 32}, {33, 33}, {2, 50}};
  const int chains[] = {8, 40, 100, 1000, 1023, 1024};
  const int filters[] = {1, 4, 8, 16, 17, 32, 33, 48, 49, 64, 65};
  const long long batches[] = {1, 7, 1024, 4096, 100000};
  char msg[256];
  for (int ansatz : {VMC_ANSATZ_CONV_2D, VMC_ANSATZ_RES_NET_2D, VMC_ANSATZ_CONV_1D, VMC_ANSATZ_RES_NET_1D}) {
    const bool one_d = ansatz == VMC_ANSATZ_CONV_1D || ansatz == VMC_ANSATZ_RES_NET_1D;
    const bool resnet = ansatz == VMC_ANSATZ_RES_NET_2D || ansatz == VMC_ANSATZ_RES_NET_1D;
    const int n_lat = one_d ? (int)(sizeof(chains) / sizeof(chains[0])) : (int)(sizeof(lats) / sizeof(lats[0]));
    for (int li = 0; li < n_lat; ++li)
      for (int F : filters)
        for (int K = 1; K <= 10; ++K)
          for (int L : {0, 1, 2, 5, 16})
            for (long long B : batches) {
              vmc_desc d;
              memset(&d, 0, sizeof(d));
              d.ansatz = ansatz; d.batch_size = (int)B; d.num_layers = L; d.layer_size = F; d.kernel_size = K;
              d.nonlinearity = VMC_ACT_RELU; d.output_activation = VMC_ACT_EXP;
              if (one_d) { d.n_sites = chains[li]; }
              else { d.size_x = lats[li].x; d.size_y = lats[li].y; d.n_sites = d.size_x * d.size_y; }
              DescPlan p;
              const int rc = plan_desc(&d, true, &p, msg, sizeof(msg));
              ++g_shapes;
              if (rc != VMC_OK) {
                ++g_rejected;
                CHECK(msg[0] != 0);
                continue;
              }
              CHECK((resnet || L >= 1) && path_conv(p.path));
              {   // the path decision under the three CGS_VMC_CONV_GENERAL preferences, written out
                const bool refused = F > 64 || K > 9 || plan_conv_rows_lds(p.cg, 1) > PLAN_LDS_PER_CU || B * p.cg.CS >= (1LL << 31);
                CHECK(p.path == (refused || plan_cgen_patch_routes(p.cg, B) ? PATH_CONV_GENERAL : PATH_CONV));
                DescPlan q;
                if (plan_desc(&d, true, &q, msg, sizeof(msg), 1) == VMC_OK) CHECK(q.path == PATH_CONV_GENERAL);
                if (plan_desc(&d, true, &q, msg, sizeof(msg), -1) == VMC_OK) CHECK(q.path == (refused ? PATH_CONV_GENERAL : PATH_CONV));
                check_split(p, ansatz, F, VMC_ACT_RELU);      // a convolutional ctx never splits
              }
              if (p.path == PATH_CONV_GENERAL) {       // beyond the fused kernels for one of their four reasons -- or sent here because the patch kernels beat them
                const bool refused = F > 64 || K > 9 || plan_conv_rows_lds(p.cg, 1) > PLAN_LDS_PER_CU || B * p.cg.CS >= (1LL << 31);
                CHECK(refused || plan_cgen_patch_routes(p.cg, B));
                if (!refused) {           // ... by preference only: CGS_VMC_CONV_GENERAL=0 keeps the fused kernels
                  DescPlan pf;
                  CHECK(plan_desc(&d, true, &pf, msg, sizeof(msg), -1) == VMC_OK && pf.path == PATH_CONV);
                }
                if (plan_cgen_patch_ok(p.cg, B)) {      // the patch kernels' LDS plan: within a CU's, every piece inside it
                  const size_t lds = plan_cgen_patch_lds_bytes(p.cg);
                  const int nc = p.cg.n_conv;
                  CHECK(lds <= PLAN_CGEN_PATCH_LDS && F <= 16 && nc >= 2 && nc <= 9);
                  CHECK(plan_cgen_patch_side(p.cg, nc - 1, 0) <= p.cg.D1 && plan_cgen_patch_side(p.cg, nc - 1, 1) <= p.cg.D2);
                  CHECK(2LL * plan_cgen_patch_side(p.cg, nc - 1, 0) * plan_cgen_patch_side(p.cg, nc - 1, 1) <= 32768);   // 16-bit marks: the last index is 2 s1 s2 - 1
                  CHECK(!resnet || !plan_cgen_patch_routes(p.cg, B));      // residual networks come here only when the fused kernels refuse them
                }
                CHECK((long long)p.cg.N * plan_cgen_lda(p.cg) < (1LL << 28));
                // the band kernel of the general path (<= 16 filters, 2 .. 7 taps): a band with its halo fits its LDS
                // budget, the bands cover the lattice, the staged index stays in 32 bits
                if (plan_cgen_band_ok(p.cg)) {
                  const int bh = plan_cgen_band_rows(p.cg);
                  CHECK(F <= 64 && K >= 2 && K <= 7 && bh >= 1 && bh <= p.cg.D1);
                  CHECK(p.cg.K * p.cg.KW * 4 * plan_cgen_band_ncb(p.cg) <= PLAN_CGEN_BAND_MAX_FRAGS && plan_cgen_band_ncb(p.cg) <= 4);
                  CHECK(plan_cgen_band_lds_bytes(p.cg, false) <= (size_t)(plan_cgen_band_ncb(p.cg) > 1 ? PLAN_CGEN_BAND_LDS_WIDE : PLAN_CGEN_BAND_LDS) &&
                        plan_cgen_band_lds_bytes(p.cg, true) <= plan_cgen_band_lds_bytes(p.cg, false));
                  const int nb = (p.cg.D1 + bh - 1) / bh;
                  CHECK((long long)nb * bh >= p.cg.D1 && (long long)(nb - 1) * bh < p.cg.D1);
                  CHECK((long long)(bh + p.cg.K - 1) * (p.cg.D2 + p.cg.KW - 1) * 16 * plan_cgen_band_ncb(p.cg) < (1LL << 24));
                  for (long long rows : {1LL, 7LL, 32LL, 1000LL, 100000LL})       // thinner bands for few rows, never beyond the LDS band
                    for (long long cap : {256LL, 512LL, 1024LL}) {
                      const int b2 = plan_cgen_band_rows_for(p.cg, rows, cap);
                      CHECK(b2 >= 1 && b2 <= bh);
                      CHECK(plan_cgen_band_lds_bytes(p.cg, false, b2) <= plan_cgen_band_lds_bytes(p.cg, false));
                      if (rows * ((p.cg.D1 + bh - 1) / bh) >= cap) CHECK(b2 == bh);
                    }
                } else {
                  CHECK(F > 64 || K > 7 || K < 2 || p.cg.K * p.cg.KW * 4 * plan_cgen_band_ncb(p.cg) > PLAN_CGEN_BAND_MAX_FRAGS ||
                        plan_cgen_band_rows(p.cg) < 1);
                }
                ++g_general;
                continue;
              }
              CHECK(F <= 64 && K <= 9);
              CHECK(plan_conv_rows_lds(p.cg, 1) <= PLAN_LDS_PER_CU);
              check_conv(d, p);
            }
  }
  // named limits: 64 filters and kernel 9 are in, 65 and 10 are out; the bench workloads are in
  vmc_desc d;
  DescPlan p;
  memset(&d, 0, sizeof(d));
  d.ansatz = VMC_ANSATZ_CONV_2D; d.batch_size = 4096; d.num_layers = 5; d.layer_size = 32; d.kernel_size = 7;
  d.size_x = d.size_y = 10; d.n_sites = 100; d.output_activation = VMC_ACT_EXP;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.cg.NCB == 2);
  d.layer_size = 64; d.kernel_size = 9;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.cg.NCB == 4 && plan_conv_tab(p.cg) == 16);
  CHECK(plan_conv_dw_nco(p.cg) == 1 && plan_conv_dw_parts(9, 9, 4) == 2 && plan_conv_dw_grid_z(p.cg) == 8);
  CHECK(plan_conv_dw_nco(5, 5, 2) == 2 && plan_conv_dw_parts(5, 5, 2) == 1);      // the measured 32-filter kernels are unchanged
  CHECK(plan_conv_dw_nco(5, 5, 1) == 1 && plan_conv_dw_parts(5, 5, 1) == 1 && plan_conv_dw_parts(9, 9, 1) == 1);
  CHECK(p.path == PATH_CONV);
  d.layer_size = 65;                                                           // beyond: the general path (conv_general.hip)
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.path == PATH_CONV_GENERAL);
  d.layer_size = 1025;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  d.layer_size = 16; d.kernel_size = 10;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.path == PATH_CONV_GENERAL && p.P == plan_num_params_conv(5, 16, 100));
  d.kernel_size = 32;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  d.kernel_size = 5;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg), true) == VMC_OK && p.path == PATH_CONV_GENERAL);      // forced (CGS_VMC_CONV_GENERAL=1)
  CHECK(plan_cgen_band_ok(p.cg) && plan_cgen_band_rows(p.cg) == 10);           // 16 filters 5 x 5 on 10 x 10: the band kernel, one band
  {  // 36 x 36 x 16 filters, 5 x 5 (bench workload heisenberg36x36_conv3x16k5_b32): three bands of 12 lattice rows
    vmc_desc b = d; DescPlan q;
    b.layer_size = 16; b.num_layers = 3; b.size_x = b.size_y = 36; b.n_sites = 1296; b.batch_size = 32;
    CHECK(plan_desc(&b, true, &q, msg, sizeof(msg)) == VMC_OK && q.path == PATH_CONV_GENERAL && plan_cgen_band_ok(q.cg));
    CHECK(plan_cgen_band_rows(q.cg) == 12 && plan_cgen_band_lds_bytes(q.cg, false) == 16u * 40u * 64u);
    // the patch sampler: boxes of 5, 9, 13 sites per axis; spins 1,296 + fragments 2 x 25 x 256 + biases 48 + boxes
    // 2 x 16 (25 + 81 + 169) + two windows of 17 x 17 x 16 floats + 1,296 16-bit marks + 1,296 uniforms
    CHECK(plan_cgen_patch_ok(q.cg, 32) && plan_cgen_patch_pays(q.cg) && plan_cgen_patch_side(q.cg, 2, 0) == 13);
    CHECK(plan_cgen_patch_lds_bytes(q.cg) == 4u * (1296u + 12800u + 48u + 8800u + 2u * 4624u + 648u + 1296u) + 256u);
    {
      DescPlan t; vmc_desc s = b;
      s.size_x = s.size_y = 12; s.n_sites = 144;                       // the last box (13) would meet itself around the torus
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg), true) == VMC_OK && t.path == PATH_CONV_GENERAL && !plan_cgen_patch_ok(t.cg, 32));
      s.size_x = s.size_y = 13; s.n_sites = 169;                       // fits exactly -- and covers the lattice: does not pay
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg), true) == VMC_OK && plan_cgen_patch_ok(t.cg, 32) && !plan_cgen_patch_pays(t.cg));
      s = b; s.num_layers = 1;                                         // one convolution: nothing to keep
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg)) == VMC_OK && !plan_cgen_patch_ok(t.cg, 32));
      // routing: a shape the fused kernels take goes to the general path where the boxes are at most a fifth of a forward
      s = b; s.size_x = s.size_y = 24; s.n_sites = 576; s.num_layers = 2; s.batch_size = 256;     // 2 (25 + 81) of 2 x 576: 18 %
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg)) == VMC_OK && t.path == PATH_CONV_GENERAL && plan_cgen_patch_routes(t.cg, 256));
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg), -1) == VMC_OK && t.path == PATH_CONV);         // CGS_VMC_CONV_GENERAL=0
      s.size_x = s.size_y = 16; s.n_sites = 256;                                                  // 2 (25 + 81) of 2 x 256: 41 %
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg)) == VMC_OK && t.path == PATH_CONV && plan_cgen_patch_ok(t.cg, 256) && !plan_cgen_patch_routes(t.cg, 256));
      s = b; s.layer_size = 32; s.kernel_size = 3;                     // two channel blocks
      CHECK(plan_desc(&s, true, &t, msg, sizeof(msg)) == VMC_OK && t.path == PATH_CONV_GENERAL && !plan_cgen_patch_ok(t.cg, 32));
    }
    // the sampler's chain groups: one where the launches are latency, two for the one-workgroup-per-CU band kernel
    CHECK(plan_cgen_sweep_groups(q.cg, 32, 256) == 1);
    b.layer_size = 64; b.kernel_size = 3;
    CHECK(plan_desc(&b, true, &q, msg, sizeof(msg)) == VMC_OK && q.path == PATH_CONV_GENERAL && plan_cgen_band_ok(q.cg));
    CHECK(plan_cgen_sweep_groups(q.cg, 32, 256) == 2 && plan_cgen_sweep_groups(q.cg, 1, 256) == 1);
    // ... and for the GEMM form where the last round of row tiles is mostly empty (800 tiles: 3.125 rounds of 256 CUs)
    b.layer_size = 128; b.size_x = b.size_y = 10; b.n_sites = 100; b.batch_size = 1024;
    CHECK(plan_desc(&b, true, &q, msg, sizeof(msg)) == VMC_OK && q.path == PATH_CONV_GENERAL && !plan_cgen_band_ok(q.cg));
    CHECK(plan_cgen_sweep_groups(q.cg, 1024, 256) == 2);       // 800 tiles
    CHECK(plan_cgen_sweep_groups(q.cg, 4096, 256) == 1);       // 3,200 tiles: 12.5 rounds, 0.96 full
    CHECK(plan_cgen_sweep_groups(q.cg, 256, 256) == 1);        // 200 tiles: less than a round
    CHECK(plan_cgen_sweep_groups(q.cg, 1280, 256) == 1);       // 1,000 tiles: 3.9 rounds
  }
  d.kernel_size = 10;
  d.kernel_size = 5; d.size_x = 9;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_INVALID);        // size_x * size_y != num_sites
  d.size_x = 10;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_OK && p.P == plan_num_params_conv(5, 16, 25));
  CHECK(plan_conv_pick_group(p.cg, 4) == 5);                                 // G = 5 on the 10 x 10 lattice
}

static void sr_schedules() {
  unsigned state = 12345u;
  auto rnd = [&](int lo, int hi) { state = state * 1664525u + 1013904223u; return lo + (int)((state >> 8) % (unsigned)(hi - lo + 1)); };
  for (int trial = 0; trial < 2000; ++trial) {
    const int n = rnd(1, RD_MAXB);
    int K[RD_MAXB], M[RD_MAXB], order[RD_MAXB], first[RD_MAXB + 1];
    for (int j = 0; j < n; ++j) { K[j] = rnd(1, 512); M[j] = rnd(1, 300000); }
    const int tiles = plan_rowdot_schedule(K, M, n, order, first);
    std::vector<int> seen((size_t)n, 0);
    long long sum = 0;
    for (int j = 0; j < n; ++j) {
      CHECK(order[j] >= 0 && order[j] < n);
      seen[(size_t)order[j]] += 1;
      if (j > 0) {
        CHECK(K[order[j]] <= K[order[j - 1]]);
        if (K[order[j]] == K[order[j - 1]]) CHECK(order[j] > order[j - 1]);   // stable
      }
      CHECK(first[j] == sum);
      sum += (M[order[j]] + RD_TM - 1) / RD_TM;
    }
    for (int v : seen) CHECK(v == 1);
    CHECK(first[n] == sum && tiles == sum);
  }
  for (int R : {1, 63, 64, 65, 4096, 204800})
    for (int cus : kCus) {
      const int s = plan_sr_wsum_slices(R, cus);
      CHECK(s >= 1 && s <= cus && (s == 1 || (long long)(s - 1) * 64 < R));
    }
}

// gnn (plan_desc's graph geometry, plan_gnn_check_adjacency, plan_gnn_inverse): every periodic-only route refuses the
// geometry, the inverse lists hold every (position, tap) pair exactly once under its site, in ascending order
static void gnn_grid() {
  char msg[256];
  for (int n : {2, 12, 100, 1296})
    for (int k : {1, 2, 5, 9, 64, 65})
      for (int F : {1, 6, 16, 64, 130, 1024, 1025})
        for (int L : {1, 3}) {
          vmc_desc d;
          memset(&d, 0, sizeof(d));
          d.ansatz = VMC_ANSATZ_GNN; d.n_sites = n; d.batch_size = 64; d.num_layers = L; d.layer_size = F;
          d.kernel_size = k; d.output_activation = VMC_ACT_EXP;
          DescPlan p;
          const int rc = plan_desc(&d, true, &p, msg, sizeof(msg));
          ++g_shapes;
          if (k < 2 || k > 64 || F > 1024) { CHECK(rc == VMC_ERR_UNSUPPORTED && msg[0]); ++g_rejected; continue; }
          CHECK(rc == VMC_OK && p.path == PATH_CONV_GENERAL && !p.resnet);
          const ConvGeom& g = p.cg;
          CHECK(g.graph == 1 && g.K == 1 && g.KW == k && g.D1 == 1 && g.D2 == n && g.N == n && g.n_conv == L);
          CHECK(g.lo == 0 && g.lo2 == 0 && !plan_cgen_periodic(g));
          CHECK(!plan_cgen_band_ok(g) && !plan_cgen_patch_ok(g, 64) && !plan_cgen_patch_routes(g, 64));
          CHECK(p.P == plan_num_params_conv(L, F, k) && p.P == (long long)k * F + F + (L - 1) * ((long long)k * F * F + F));
          CHECK(plan_cgen_lda(g) >= k * (L > 1 ? F : 1));
          ++g_general;
        }
  // the table: a random one with repeats, its inverse lists
  for (int n : {2, 7, 144})
    for (int k : {2, 7, 64}) {
      std::vector<int32_t> adj((size_t)n * k), ptr((size_t)n + 1), idx((size_t)n * k);
      unsigned x = 12345u + n * 31u + k;
      for (auto& a : adj) { x = x * 1103515245u + 12345u; a = (int32_t)((x >> 8) % (unsigned)n); }
      CHECK(plan_gnn_check_adjacency(n, k, n, k, adj.data(), msg, sizeof(msg)) == VMC_OK);
      CHECK(plan_gnn_check_adjacency(n, k, n + 1, k, adj.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
      CHECK(plan_gnn_check_adjacency(n, k, n, k - 1, adj.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
      plan_gnn_inverse(n, k, adj.data(), ptr.data(), idx.data());
      CHECK(ptr[0] == 0 && ptr[n] == n * k);
      std::vector<unsigned char> seen((size_t)n * k, 0);
      for (int s = 0; s < n; ++s)
        for (int j = ptr[s]; j < ptr[s + 1]; ++j) {
          CHECK(idx[j] >= 0 && idx[j] < n * k && adj[(size_t)idx[j]] == s && !seen[(size_t)idx[j]]);
          CHECK(j == ptr[s] || idx[j - 1] < idx[j]);
          seen[(size_t)idx[j]] = 1;
        }
      const int32_t keep = adj[0];
      for (int32_t bad : {-1, n}) {
        adj[0] = bad;
        CHECK(plan_gnn_check_adjacency(n, k, n, k, adj.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
      }
      adj[0] = keep;
    }
}

// pbdg (plan_desc's shape checks, plan_pbdg_*): odd / oversized N refused, the LDS plan of every even N re-derived into
// a real array (the carve of pbdg.hip), chains per workgroup within the budget, refresh interval and gradient slices in range
static void pbdg_grid() {
  char msg[256];
  for (int n_sites = 1; n_sites <= 258; ++n_sites) {
    vmc_desc d = dense_desc(VMC_ANSATZ_PBDG, n_sites, 64, 0, 0, VMC_ACT_RELU, VMC_ACT_EXP);
    DescPlan p;
    const int rc = plan_desc(&d, true, &p, msg, sizeof(msg));
    ++g_shapes;
    if (n_sites < 2 || (n_sites & 1)) { CHECK(rc == VMC_ERR_INVALID); ++g_rejected; continue; }
    if (n_sites > PLAN_PBDG_MAX_SITES) { CHECK(rc == VMC_ERR_UNSUPPORTED); ++g_rejected; continue; }
    CHECK(rc == VMC_OK && p.path == PATH_PBDG && p.P == (long long)n_sites * n_sites);
    CHECK(plan_num_params_dense(VMC_ANSATZ_PBDG, n_sites, 0, 0) == p.P);
    const int n = n_sites / 2, ld = plan_pbdg_ld(n);
    CHECK(ld >= n && (ld & 1) == 1);
    const size_t bytes = plan_pbdg_chain_lds_bytes(n_sites);
    CHECK(bytes % 4 == 0);
    const int cpw = plan_pbdg_chains_per_wg(n_sites);
    CHECK(cpw == 1 || cpw == 2 || cpw == 4);
    CHECK((size_t)cpw * bytes <= PLAN_LDS_PER_CU);
    CHECK(cpw == 1 || (size_t)cpw * bytes <= PLAN_PBDG_WG_LDS);
    // the carve: A [n][ld], six vectors [n], spins [N] (floats), up / dn / perm [n], pos [N] (ints); the last element of
    // every piece is touched in a real array of the planned size
    std::vector<float> lds(bytes / 4);
    size_t off = 0;
    auto touch = [&](size_t len) { CHECK(off + len <= lds.size()); lds[off + len - 1] = 1.f; off += len; };
    touch((size_t)n * ld);
    for (int v = 0; v < 6; ++v) touch(n);
    touch(n_sites);
    for (int v = 0; v < 3; ++v) touch(n);
    touch(n_sites);
    CHECK(off == lds.size());
    const int R = plan_pbdg_refresh_interval(n_sites);
    CHECK(R >= 16 && R <= 128);
    for (int cus : kCus)
      for (long long B : {1LL, 7LL, 1024LL, 4096LL}) {
        const int s = plan_pbdg_grad_slices(p.P, B, cus);
        CHECK(s >= 1 && s <= 256 && s <= B);
        CHECK(plan_pbdg_grad_ws_doubles(p.P, s) == 2 * p.P * s);
      }
  }
  CHECK(plan_pbdg_chains_per_wg(256) == 1 && plan_pbdg_chains_per_wg(36) == 4);
  CHECK(plan_pbdg_check(16, msg, sizeof(msg)) == VMC_OK);
  CHECK(plan_pbdg_check(17, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_pbdg_check(258, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
}

// fully_connected_nnb (plan_nnb_*, the NNB branch of plan_desc / plan_num_params_dense): every even N from 4 to 100 (and the
// edges up to 258) with L, H and batch sizes; the parameter layout ends exactly at P; the block of rows stays within the
// planned workspace for every block size; the rows kernel's grid covers the block; the weight-gradient tiles and the
// slices' workspace are in range
static void nnb_grid() {
  char msg[256];
  const int Ns[] = {1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54,
                    56, 58, 60, 62, 64, 66, 68, 70, 72, 74, 76, 78, 80, 82, 84, 86, 88, 90, 92, 94, 96, 98, 99, 100, 128, 200,
                    255, 256, 257, 258};
  for (int n_sites : Ns)
    for (int L : {0, 1, 2, 3, 16, 17})
      for (int H : {1, 7, 32, 64, 100, 256, 300, 512, 513})
        for (long long B : {1LL, 7LL, 64LL, 1024LL, 4096LL, 65536LL}) {
          vmc_desc d = dense_desc(VMC_ANSATZ_NNB, n_sites, (int)B, L, H, VMC_ACT_TANH, VMC_ACT_IDENTITY);   // activations ignored
          DescPlan p;
          const int rc = plan_desc(&d, true, &p, msg, sizeof(msg));
          ++g_shapes;
          CHECK(rc == plan_nnb_check(n_sites, L, H, B, msg, sizeof(msg)));
          if (n_sites < 2 || (n_sites & 1)) { CHECK(rc == VMC_ERR_INVALID); ++g_rejected; continue; }
          const long long NN = (long long)n_sites * n_sites;
          if (n_sites > PLAN_NNB_MAX_SITES || L < 1 || L > PLAN_NNB_MAX_LAYERS || H > PLAN_NNB_MAX_UNITS ||
              B * NN > PLAN_NNB_MAX_DELTA) {
            CHECK(rc == VMC_ERR_UNSUPPORTED); ++g_rejected; continue;
          }
          CHECK(rc == VMC_OK && p.path == PATH_NNB && path_wide(p.path) && path_general_dense(p.path));
          CHECK(p.Hp >= H && p.Hp % 64 == 0 && p.Hp < H + 64 && p.n_hh == L - 1);
          const long long P = (long long)n_sites * H + H + (long long)(L - 1) * ((long long)H * H + H) + H * NN + NN;
          CHECK(p.P == P && plan_num_params_dense(VMC_ANSATZ_NNB, n_sites, H, L) == P);
          // the layout: layers in order, the pairing layer's weights then its biases, ending at P
          CHECK(plan_off_w(p.lay, H, 0) == 0 && plan_off_b(p.lay, H, 0) == (long long)n_sites * H);
          for (int l = 1; l < L; ++l) CHECK(plan_off_b(p.lay, H, l) == plan_off_w(p.lay, H, l) + (long long)H * H);
          CHECK(p.lay.off_wout == (long long)n_sites * H + H + (long long)(L - 1) * ((long long)H * H + H));
          CHECK(p.lay.off_bout == p.lay.off_wout + H * NN && p.lay.off_bout + NN == P);
          // row blocks: bounded by the block size for every knob value, never empty
          for (long long mb : {-5LL, 0LL, 1LL, 16LL, 256LL, 4096LL, 1LL << 40}) {
            const long long rows = plan_nnb_block_rows(n_sites, mb);
            const long long eff = mb < 1 ? 1 : (mb > PLAN_NNB_BLOCK_MB_MAX ? PLAN_NNB_BLOCK_MB_MAX : mb);
            CHECK(rows >= 1 && rows <= (1LL << 20));
            CHECK(rows == 1 || rows * NN * 4 <= (eff << 20));
            CHECK(rows * NN < (1LL << 31) * 4);
            CHECK(plan_nnb_block_floats(n_sites, p.Hp, rows) == rows * (NN + 2 * p.Hp));
            const long long grid = plan_nnb_rows_grid(rows, n_sites);
            CHECK(grid >= 1 && grid * plan_pbdg_chains_per_wg(n_sites) >= rows && grid < (1LL << 31));
          }
          // the default block on the headline lattice: 4 x 10^5 connected rows walk in blocks of a bounded workspace
          if (n_sites == 100) CHECK(plan_nnb_block_rows(100, PLAN_NNB_BLOCK_MB_DEFAULT) == 6710);
          CHECK((size_t)plan_pbdg_chains_per_wg(n_sites) * plan_pbdg_chain_lds_bytes(n_sites) <= PLAN_LDS_PER_CU);
          const int tiles = plan_nnb_wgrad_total_tiles(n_sites, H, L - 1);
          CHECK(tiles == plan_wgrad_tiles(H, (int)NN) + (L - 1) * plan_wgrad_tiles(H, H) + plan_wgrad_tiles(n_sites, H));
          for (int cus : kCus) {
            const int s = plan_wgrad_slices(tiles, B, cus, 1, 0);
            CHECK(s >= 1 && s <= WG_MAX_SPLIT && (long long)plan_wgrad_kchunk((int)B, s) * s >= B);
            CHECK(plan_wgrad_grid(tiles, s) >= tiles * s);
            CHECK(plan_wgrad_ws_floats(tiles, s) < (1LL << 33));
          }
        }
  vmc_desc d = dense_desc(8, 16, 64, 2, 32, VMC_ACT_RELU, VMC_ACT_EXP);        // id 8 stays unassigned
  DescPlan p;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  d = dense_desc(11, 16, 64, 2, 32, VMC_ACT_RELU, VMC_ACT_EXP);                 // the product: vmc_create_product only
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_INVALID);
  d = dense_desc(12, 16, 64, 2, 32, VMC_ACT_RELU, VMC_ACT_EXP);                 // the first id past the product
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
}

// ed_vector (plan_desc's shape checks, plan_edvec_*): odd / oversized N and bad lengths refused, the sampler's grid covers
// every chain in whole waves within a workgroup, the LDS decision keeps the staged tables within a CU, and the table
// check accepts Lin's tables of the Sz = 0 sector (built here) and refuses a short vector, a shifted entry, a wrong size
static void edvec_grid() {
  char msg[256];
  for (int n_sites = 1; n_sites <= 34; ++n_sites) {
    long long len = 1;                                   // C(N, N/2)
    for (int k = 1; k <= n_sites / 2; ++k) len = len * (n_sites / 2 + k) / k;
    vmc_desc d = dense_desc(VMC_ANSATZ_ED_VECTOR, n_sites, 64, 0, (int)len, VMC_ACT_RELU, VMC_ACT_EXP);
    DescPlan p;
    const int rc = plan_desc(&d, true, &p, msg, sizeof(msg));
    ++g_shapes;
    if (n_sites < 2 || (n_sites & 1)) { CHECK(rc == VMC_ERR_INVALID); ++g_rejected; continue; }
    if (n_sites > PLAN_EDVEC_MAX_SITES) { CHECK(rc == VMC_ERR_UNSUPPORTED); ++g_rejected; continue; }
    CHECK(rc == VMC_OK && p.path == PATH_EDVEC && p.P == len);
    CHECK(plan_num_params_dense(VMC_ANSATZ_ED_VECTOR, n_sites, len, 0) == len);
    CHECK(2 * p.P + 8 < 0x7fffffffLL);                    // the accumulator offsets Adam indexes with int
    const size_t tb = plan_edvec_tables_bytes(n_sites);
    CHECK(tb == (size_t)8 << (n_sites / 2));
    CHECK(!plan_edvec_tables_in_lds(n_sites) || tb <= PLAN_LDS_PER_CU);
    CHECK(plan_edvec_tables_in_lds(n_sites));             // (every size under the cap)
    for (int cus : kCus)
      for (long long B : {1LL, 63LL, 64LL, 65LL, 1000LL, 4096LL, 65536LL, 1000000LL}) {
        const int t = plan_edvec_sweep_threads(B, cus);
        CHECK(t >= 64 && t <= 1024 && t % 64 == 0);
        const unsigned g = plan_edvec_sweep_grid(B, t);
        CHECK((long long)g * t >= B && (long long)(g - 1) * t < B);
        CHECK(t == 1024 || g <= (unsigned)cus);           // below the workgroup limit no CU holds two workgroups
      }
    d.layer_size = 0;
    CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_INVALID);
    if (n_sites > 16) continue;
    // Lin's tables: the configurations in ascending order of (top, bot) with popcount(top) + popcount(bot) = N/2
    const int h = n_sites / 2, n_half = 1 << h;
    std::vector<int32_t> top(n_half), bot(n_half), seen(h + 1, 0);
    std::vector<long long> cls(h + 1, 1);               // C(h, k)
    for (int k = 1; k <= h; ++k) cls[k] = cls[k - 1] * (h - k + 1) / k;
    long long base = 0;
    for (int t = 0; t < n_half; ++t) {
      const int k = __builtin_popcount(t);
      top[t] = (int32_t)base; base += cls[h - k];
      bot[t] = seen[k]++;
    }
    CHECK(base == len);
    CHECK(plan_edvec_check_tables(n_sites, n_half, top.data(), bot.data(), len, msg, sizeof(msg)) == VMC_OK);
    CHECK(plan_edvec_check_tables(n_sites, n_half, top.data(), bot.data(), len - 1, msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(plan_edvec_check_tables(n_sites, n_half / 2, top.data(), bot.data(), len, msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(plan_edvec_check_tables(n_sites, n_half, nullptr, bot.data(), len, msg, sizeof(msg)) == VMC_ERR_INVALID);
    bot[0] = -1;                                          // top = all ones, bot = 0: index top[n_half - 1] - 1 = len - 2, still inside
    top[n_half - 1] = 0;                                  // ... now -1
    CHECK(plan_edvec_check_tables(n_sites, n_half, top.data(), bot.data(), len, msg, sizeof(msg)) == VMC_ERR_INVALID);
  }
  CHECK(plan_edvec_check(16, 12870, msg, sizeof(msg)) == VMC_OK);
  CHECK(plan_edvec_check(15, 100, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_edvec_check(30, 100, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  CHECK(plan_edvec_check(16, 0x80000000LL, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
  CHECK(plan_edvec_sweep_threads(4096, 256) == 64 && plan_edvec_sweep_threads(65536, 256) == 256);
}

// product ctx (plan_prod_*): which factors are taken, the accumulator size, grids that cover every chain / element,
// and vmc_create refusing the id
static void prod_grid() {
  char msg[256];
  for (int ansatz = 0; ansatz <= VMC_ANSATZ_PRODUCT; ++ansatz)
    for (int oact = 0; oact <= 6; ++oact) {
      const int rc = plan_prod_child_check(ansatz, oact, false, msg, sizeof(msg));
      const bool dense = ansatz == VMC_ANSATZ_FULLY_CONNECTED || ansatz == VMC_ANSATZ_RBM;
      const bool taken = ansatz == VMC_ANSATZ_PBDG || ansatz == VMC_ANSATZ_ED_VECTOR || (dense && oact == VMC_ACT_EXP);
      CHECK(rc == (taken ? VMC_OK : VMC_ERR_UNSUPPORTED));
      CHECK(plan_prod_child_check(ansatz, oact, true, msg, sizeof(msg)) == VMC_ERR_UNSUPPORTED);
    }
  CHECK(plan_prod_acc_floats(256, 577) == 2 * 833 + 8);
  for (long long B : {1LL, 3LL, 4LL, 40LL, 64LL, 4097LL}) {
    CHECK((long long)plan_prod_chain_grid(B) * PLAN_PROD_CHAINS_PER_WG >= B);
    CHECK(((long long)plan_prod_chain_grid(B) - 1) * PLAN_PROD_CHAINS_PER_WG < B);
    CHECK((long long)plan_prod_elem_grid(B * 16) * 256 >= B * 16);
  }
  vmc_desc d;
  memset(&d, 0, sizeof(d));
  d.n_sites = 16; d.batch_size = 64; d.num_layers = 1; d.layer_size = 32; d.output_activation = VMC_ACT_EXP;
  d.ansatz = VMC_ANSATZ_PRODUCT;
  DescPlan p;
  CHECK(plan_desc(&d, true, &p, msg, sizeof(msg)) == VMC_ERR_INVALID);
}

// the measurements (plan_measure_*): every pass inside the row budget, the 32-bit row index and the caller's row limit
// (one item is always taken), the passes cover the items exactly, a request only ever shrinks a pass, the fold grid
// covers a pass and a whole list, every index into an [n_items][B] buffer and into a pass's rows x sites fits 32 bits,
// and the row limit keeps the forward's scratch and its flat indices in range
static void measure_grid() {
  for (long long B : {1LL, 2LL, 40LL, 64LL, 1000LL, 4096LL, 65536LL, 1LL << 24, (1LL << 24) + 1, (1LL << 24) + 2, 1LL << 30,
                      (1LL << 30) + 1, (1LL << 30) + 2, 0x7ffffffeLL, 0x7fffffffLL})
    for (long long n_items : {1LL, 7LL, 34LL, 50LL, 70LL, 120LL, 200LL, 276LL, 1024LL, 4950LL, 40000LL, 523776LL})
      for (long long req : {0LL, 1LL, 3LL, 7LL, 64LL, 70LL, 276LL, 1LL << 40})
        for (long long lim : {0LL, 1LL, 4096LL, 100000LL, 1LL << 22, 1LL << 40}) {
          const int per = plan_measure_per_pass(B, n_items, req, lim);
          // not even one item fits the row index
          if (2 * B > 0x7fffffffLL) { CHECK(per == 0); CHECK(!plan_measure_rows_ok(B, n_items)); continue; }
          CHECK(per >= 1 && per <= n_items);
          CHECK(B * per <= 0x7fffffffLL - B);                              // vmc_set_bonds' rule
          CHECK(B * per <= PLAN_MEASURE_ROW_BUDGET || per == 1);
          if (lim > 0) CHECK(B * per <= lim || per == 1);
          if (req > 0) CHECK(per <= req);
          CHECK(per <= plan_measure_per_pass(B, n_items, 0, lim));
          CHECK(per <= plan_measure_per_pass(B, n_items, req, 0));
          if (lim == 0) CHECK(per == plan_measure_per_pass(B, n_items, req));   // no row limit is the default
          const long long passes = plan_measure_passes(n_items, per);
          CHECK(passes * per >= n_items && (passes - 1) * per < n_items);
          CHECK((long long)plan_measure_fold_grid(per) * 64 >= per && ((long long)plan_measure_fold_grid(per) - 1) * 64 < per);
          CHECK((long long)plan_measure_fold_grid((int)n_items) * 64 >= n_items);        // the bond fold takes every bond at once
          if (plan_measure_rows_ok(B, n_items)) CHECK(B * n_items + B <= 0x7fffffffLL);
          else CHECK(B * n_items + B > 0x7fffffffLL);
        }
  for (int N : {2, 16, 100, 1024, 4096})
    for (int Hp : {64, 256, 512, 4096}) {
      const long long rows = plan_measure_row_limit(N, Hp);
      CHECK(rows >= 1);
      CHECK(rows * (N > Hp ? N : Hp) <= 0x7fffffffLL);
      CHECK(rows * ((long long)N + Hp + 5) <= (1LL << 30));
    }
  CHECK(plan_measure_per_pass(4096, 4950, 0) == 4096);                // 100 sites, all pairs: two passes
  CHECK(plan_measure_per_pass(40, 120, 0) == 120 && plan_measure_per_pass(40, 120, 7) == 7);
  CHECK(plan_measure_per_pass(0, 1, 0) == 0 && plan_measure_per_pass(1, 0, 0) == 0 && plan_measure_per_pass(1, 1, -1) == 0);
  CHECK(plan_measure_per_pass(4096, 50, 0, plan_measure_row_limit(100, 256)) == 50);      // config 3, the 50 blocks: one pass
  CHECK(plan_measure_per_pass(40, 70, 0) == 70 && plan_measure_per_pass(40, 70, 3) == 3);
  CHECK(plan_measure_per_pass(40, 70, 0, 100) == 2 && plan_measure_per_pass(40, 70, 0, 10) == 1);
  CHECK(plan_measure_per_pass(2, 0, 0) == 0 && plan_measure_per_pass(2, 1, -1) == 0 && plan_measure_per_pass(2, 1, 0, -1) == 0);
  // config 3's shape, one reference bond against the 200 bonds: each phase is one pass of 819,200 rows
  CHECK(plan_measure_per_pass(4096, 200, 0, plan_measure_row_limit(100, 256)) == 200);
  CHECK(plan_measure_per_pass(40, 70, 7) == 7 && plan_measure_per_pass(40, 70, 64) == 64);
  CHECK(plan_measure_per_pass(40, 1024, 0, 100) == 2 && plan_measure_per_pass(40, 1024, 0, 10) == 1);
  CHECK(plan_measure_per_pass(40, 0, 0) == 0 && plan_measure_per_pass(40, 1, -1) == 0 && plan_measure_per_pass(40, 1, 0, -1) == 0);
  CHECK(!plan_measure_rows_ok(40, 0) && !plan_measure_rows_ok(0, 1) && plan_measure_rows_ok(40, 34));
}

// the ops of vmc_symmetry_expectations (plan_symm_check_ops): random bijections with and without flips pass; a
// duplicated, a negative and an == N entry, and a flip above 1, are each refused with the op named
static void symm_ops() {
  char msg[160];
  unsigned long long state = 0x9e3779b97f4a7c15ULL;
  auto next = [&]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(state >> 33); };
  for (int N : {1, 2, 6, 16, 64, 65, 100, 1023})
    for (int n_ops : {1, 3, 8, 70}) {
      std::vector<int32_t> perm((size_t)n_ops * (size_t)N);
      std::vector<uint8_t> flip((size_t)n_ops);
      for (int k = 0; k < n_ops; ++k) {
        int32_t* g = perm.data() + (size_t)k * (size_t)N;
        for (int i = 0; i < N; ++i) g[i] = i;
        for (int i = N - 1; i > 0; --i) std::swap(g[i], g[next() % (unsigned)(i + 1)]);      // Fisher-Yates
        flip[(size_t)k] = (uint8_t)(next() & 1);
      }
      CHECK(plan_symm_check_ops(N, n_ops, perm.data(), flip.data(), msg, sizeof(msg)) == VMC_OK && msg[0] == 0);
      CHECK(plan_symm_check_ops(N, n_ops, perm.data(), nullptr, msg, sizeof(msg)) == VMC_OK);
      const int k = (int)(next() % (unsigned)n_ops), i = (int)(next() % (unsigned)N);
      char want[32];
      snprintf(want, sizeof(want), "op %d:", k);
      int32_t* g = perm.data() + (size_t)k * (size_t)N;
      const int32_t kept = g[i];
      for (int32_t bad : {(int32_t)-1, (int32_t)N, (int32_t)0x7fffffff, (int32_t)(-0x7fffffff - 1)}) {
        g[i] = bad;
        CHECK(plan_symm_check_ops(N, n_ops, perm.data(), flip.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
        CHECK(strstr(msg, want) == msg);
      }
      g[i] = kept;
      if (N > 1) {
        g[i] = g[(i + 1) % N];                                                                // a duplicate
        CHECK(plan_symm_check_ops(N, n_ops, perm.data(), flip.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
        CHECK(strstr(msg, want) == msg && strstr(msg, "second time"));
        g[i] = kept;
      }
      flip[(size_t)k] = 2;
      CHECK(plan_symm_check_ops(N, n_ops, perm.data(), flip.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
      CHECK(strstr(msg, want) == msg && strstr(msg, "flip"));
      flip[(size_t)k] = 1;
      CHECK(plan_symm_check_ops(N, n_ops, perm.data(), flip.data(), msg, sizeof(msg)) == VMC_OK);
    }
  int32_t one = 0;
  CHECK(plan_symm_check_ops(1, 0, &one, nullptr, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_symm_check_ops(0, 1, &one, nullptr, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_symm_check_ops(1, 1, nullptr, nullptr, msg, sizeof(msg)) == VMC_ERR_INVALID);
  CHECK(plan_symm_check_ops(1, 1, &one, nullptr, nullptr, 0) == VMC_OK);
  // config 3's shape, the 100 translations with and without the flip: one pass of 819,200 rows
  CHECK(plan_measure_per_pass(4096, 200, 0, plan_measure_row_limit(100, 256)) == 200);
}

// vmc_projected_energy: plan_symm_check_hamiltonian on tori with and without next-nearest bonds (the 2-wide torus names
// its bonds across the short direction twice), the sector tile and the accumulator budget
static void proj_grid() {
  char msg[256];
  struct Lattice { int sx, sy; bool j2; };
  for (const Lattice& l : {Lattice{4, 4, true}, Lattice{4, 4, false}, Lattice{2, 4, false}, Lattice{8, 1, false}, Lattice{3, 5, true}}) {
    const int sx = l.sx, sy = l.sy, N = sx * sy;
    auto site = [&](int x, int y) { return (int32_t)(((x % sx) + sx) % sx + sx * (((y % sy) + sy) % sy)); };
    std::vector<int32_t> ij;
    std::vector<float> jx, jz;
    auto bond = [&](int a, int b, float x, float z) { ij.push_back(a); ij.push_back(b); jx.push_back(x); jz.push_back(z); };
    for (int y = 0; y < sy; ++y)
      for (int x = 0; x < sx; ++x) {
        bond(site(x, y), site(x + 1, y), 1.f, 1.f);
        if (sy > 1) bond(site(x, y), site(x, y + 1), 1.f, 1.f);
        if (l.j2) { bond(site(x, y), site(x + 1, y + 1), 0.5f, 0.25f); bond(site(x, y), site(x + 1, y - 1), 0.5f, 0.25f); }
      }
    const int nb = (int)jx.size();
    // the translations, the mirror x -> -x, the inversion; on a square also the rotation and the diagonal mirror
    std::vector<int32_t> perm;
    auto op = [&](int a, int b, int c, int d, int tx, int ty) {     // (x, y) -> (a x + b y + tx, c x + d y + ty)
      for (int y = 0; y < sy; ++y) for (int x = 0; x < sx; ++x) perm.push_back(site(a * x + b * y + tx, c * x + d * y + ty));
    };
    for (int ty = 0; ty < sy; ++ty) for (int tx = 0; tx < sx; ++tx) op(1, 0, 0, 1, tx, ty);
    op(-1, 0, 0, 1, 0, 0); op(-1, 0, 0, -1, 1, 2);
    if (sx == sy) { op(0, -1, 1, 0, 0, 0); op(0, 1, 1, 0, 3, 1); }
    const int n_ops = (int)perm.size() / N;
    CHECK(plan_symm_check_ops(N, n_ops, perm.data(), nullptr, msg, sizeof(msg)) == VMC_OK);
    CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), n_ops, perm.data(), msg, sizeof(msg)) == VMC_OK && msg[0] == 0);
    // one bond's j_x changed: the last translation (it moves both coordinates) is no symmetry any more, the identity is
    const int hit = nb / 2;
    const float kept = jx[(size_t)hit];
    jx[(size_t)hit] = 0.75f;
    CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), 1, perm.data(), msg, sizeof(msg)) == VMC_OK);
    CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), n_ops, perm.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), 1, perm.data() + (size_t)(N - 1) * N, msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(strstr(msg, "op 0 ") == msg && strstr(msg, " bond "));
    jx[(size_t)hit] = kept;
    // the exchange of two sites that are no images of each other under the lattice's symmetries
    if (N > 4) {
      std::vector<int32_t> two(perm.begin(), perm.begin() + 2 * N);
      std::swap(two[(size_t)N + 0], two[(size_t)N + 1]);
      CHECK(plan_symm_check_ops(N, 2, two.data(), nullptr, msg, sizeof(msg)) == VMC_OK);
      CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), 2, two.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
      CHECK(strstr(msg, "op 1 ") == msg);
    }
    // the multiset: one of a doubled pair of bonds dropped is noticed where a set would not
    if (sx == 2) {
      std::vector<int32_t> ij1(ij.begin() + 2, ij.end());
      CHECK(plan_symm_check_hamiltonian(N, nb - 1, ij1.data(), jx.data() + 1, jz.data() + 1, n_ops, perm.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    }
    CHECK(plan_symm_check_hamiltonian(N, 0, ij.data(), jx.data(), jz.data(), n_ops, perm.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
    CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), n_ops, nullptr, msg, sizeof(msg)) == VMC_ERR_INVALID);
    ij[1] = N;
    CHECK(plan_symm_check_hamiltonian(N, nb, ij.data(), jx.data(), jz.data(), n_ops, perm.data(), msg, sizeof(msg)) == VMC_ERR_INVALID);
  }
  for (long long n_sectors : {1LL, 2LL, 15LL, 16LL, 17LL, 104LL, 1LL << 20})
    for (long long ops : {1LL, 7LL, 200LL, (long long)PLAN_PROJ_LAUNCH_OPS}) {
      const int tile = plan_measure_sector_tile(n_sectors, ops);
      CHECK(tile >= 1 && tile <= PLAN_PROJ_MAX_TILE && tile <= n_sectors);
      CHECK(plan_proj_accum_lds_bytes(tile, (int)ops) <= PLAN_PROJ_LDS_BYTES);
      const long long tiles = plan_proj_sector_tiles(n_sectors, tile);
      CHECK(tiles * tile >= n_sectors && (tiles - 1) * tile < n_sectors);
      for (long long B : {1LL, 40LL, 200LL, 256LL, 257LL, 4096LL})
        if (plan_proj_acc_ok(B, n_sectors)) {
          const long long blocks = plan_proj_chain_blocks(B);
          CHECK(blocks * PLAN_PROJ_THREADS >= B && (blocks - 1) * PLAN_PROJ_THREADS < B);
          CHECK(blocks * tiles <= 0x7fffffffLL);                         // the one-dimensional grid
          CHECK(n_sectors * B <= PLAN_PROJ_MAX_ACC);
        }
    }
  CHECK(plan_measure_sector_tile(0, 1) == 0 && plan_measure_sector_tile(1, 0) == 0);
  CHECK(plan_measure_sector_tile(104, 200) == 16 && plan_measure_sector_tile(3, 200) == 3);
  CHECK(plan_proj_acc_ok(4096, 104) && plan_proj_acc_ok(1, 1LL << 26) && !plan_proj_acc_ok(2, 1LL << 26) && !plan_proj_acc_ok(4096, 0) && !plan_proj_acc_ok(0, 1));
}

int main() {
  path_truth_table();
  check_block_maps();
  measure_grid();
  symm_ops();
  proj_grid();
  prod_grid();
  edvec_grid();
  nnb_grid();
  pbdg_grid();
  gnn_grid();
  dense_grid();
  conv_grid();
  sr_schedules();
  printf("hostcheck ok: %lld shapes (%lld rejected by plan_desc, %lld convolutional ones on the general path), %lld assertions\n", g_shapes, g_rejected, g_general, g_checks);
  return 0;
}
