"""The inputs of the product tests off the 4 x 4 torus (tests/test_gpu_prod_shapes.py) and the fp64 oracle runs on them.
One place, so that tests/test_prod.py proves on the oracle alone that the committed inputs keep every cap the GPU tests
lean on (banded verdicts, acceptance shares, pbdg logit bounds, group sizes of the injected steps) and the GPU file
runs the same inputs on the kernels.

What each shape reaches in csrc/prod.hip / csrc/vmc_api_prod.hip:
  S1  sign only in slot b (cb_s != nullptr, ca_s == nullptr); N % 4 = 2: a ragged last Philox block; B % 4 = 2
  S2  two signed factors, whose signs multiply
  S3  ed_vector in slot b (length 48620)
  S4  N = 258: Philox block 64 is lane 0's second trip of k_prod_accept's loop and holds two valid sites
  S5  B = 1025: second trip of k_prod_count_fold's stride loop, a chain-grid tail of one wave, many row-combine blocks
  S6  one chain
"""
import functools

import numpy as np

from oracle import vmc_oracle as vo
from tests import edvec_oracle as eo
from tests import pbdg_oracle as po
from tests import prod_oracle as pro

SEED = 2024                                    # the engines' sampler seed
H = 8                                          # dense factors: one layer of 8 units
EPS32 = float(np.finfo(np.float32).eps)
BAND = 1e-4                                    # | |psi'/psi| - sqrt(u) | < 1e-4 |psi'/psi|

# scale: the dense weights of S4 are multiplied by it.  Over the 40 steps of the replay the oracle accepts 0.965 of the
# proposals at 0.3, 0.805 at 1, 0.61 at 2 and 0.565 at 3 (replay('S4').share): 2 puts it inside [0.2, 0.8].
# seed: of the parameters, bonds and rows (default 100 x the case's number).  S2: two determinants accept little --
# of twelve seeds tried on the oracle this one alone gave a share above 0.2 (0.229; the others 0.158 - 0.199).
# start_seed: of the start chains alone.  S5: 1025 chains x 20 verdicts with a band of 1e-4 leave two chains banded on
# average; this start has none (the smallest | |psi'/psi| - sqrt(u) | / |psi'/psi| is 2.0e-4) and keeps the pbdg logit
# bound of all 1025 rows below 0.5 (0.446), so mc_steps' count is compared exactly.  S3: the default start put all six
# chains on entries of one sign; this one has three of each.
CASES = {
    'S1': dict(a='rbm', b='pbdg', n=18, b_chains=6, offset=1000, steps=54, scale=1.0),
    'S2': dict(a='pbdg', b='pbdg', n=22, b_chains=7, offset=0, steps=66, scale=1.0, seed=220, omega_seed=2290),
    'S3': dict(a='fully_connected', b='ed_vector', n=18, b_chains=6, offset=77, steps=54, scale=1.0, start_seed=3001),
    'S4': dict(a='fully_connected', b='rbm', n=258, b_chains=5, offset=123456, steps=40, scale=2.0),
    'S5': dict(a='pbdg', b='fully_connected', n=18, b_chains=1025, offset=0, steps=20, scale=1.0, start_seed=5022),
    'S6': dict(a='fully_connected', b='pbdg', n=18, b_chains=1, offset=3, steps=54, scale=1.0),
}
IDS = sorted(CASES)
EVAL = dict(n_eq=10, n_samples=3, n_mc=6)      # evaluate(None, n_eq, 3, n_mc) on S1
SIGNED = ('pbdg', 'ed_vector')


def _case_seed(cid):
  return CASES[cid].get('seed', 100 * int(cid[1]))


def pbdg_theta(n, seed):
  """tests/test_gpu_prod.py's _pbdg_theta at n sites."""
  lim = np.sqrt(3.0 / n)
  return np.random.default_rng(seed).uniform(-lim, lim, n * n).astype(np.float32)


def spec_of(kind, n):
  if kind == 'pbdg':
    return dict(ansatz='pbdg', num_layers=1, layer_size=1)
  if kind == 'ed_vector':
    top, bot, length = eo.lin_tables(n)
    return dict(ansatz='ed_vector', num_layers=1, layer_size=length, lin_tables=(top, bot))
  return dict(ansatz=kind, num_layers=1, layer_size=H, nonlinearity='relu', output_activation='exp')


def factor_of(kind, n, theta):
  """The fp64 oracle factor of float32 parameters `theta`."""
  theta = np.asarray(theta, np.float32)
  if kind == 'pbdg':
    return pro.pbdg_factor(theta)
  if kind == 'ed_vector':
    top, bot, _ = eo.lin_tables(n)
    return pro.edvec_factor(theta, top, bot)
  return (pro.fc_factor if kind == 'fully_connected' else pro.rbm_factor)(theta, H, 1)


def _theta_of(kind, n, rng, seed, scale):
  if kind == 'pbdg':
    return pbdg_theta(n, seed)
  if kind == 'ed_vector':
    return rng.standard_normal(eo.lin_tables(n)[2]).astype(np.float32)
  init = vo.init_params if kind == 'fully_connected' else vo.rbm_init_params
  return (scale * np.asarray(init(n, H, 1, rng), np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def thetas(cid):
  c = CASES[cid]
  rng = np.random.default_rng(_case_seed(cid))
  ta = _theta_of(c['a'], c['n'], rng, _case_seed(cid) + 1, c['scale'])
  tb = _theta_of(c['b'], c['n'], rng, _case_seed(cid) + 2, c['scale'])
  return ta, tb


def product_of(cid, ta=None, tb=None):
  c = CASES[cid]
  da, db = thetas(cid)
  return pro.Product(factor_of(c['a'], c['n'], da if ta is None else ta), factor_of(c['b'], c['n'], db if tb is None else tb))


def specs(cid):
  c = CASES[cid]
  return [spec_of(c['a'], c['n']), spec_of(c['b'], c['n'])]


def signed(cid):
  return CASES[cid]['a'] in SIGNED or CASES[cid]['b'] in SIGNED


@functools.lru_cache(maxsize=None)
def bonds(cid):
  """(bonds, jx[nb], jz[nb]): N + 5 random site pairs i != j -- repeats, i > j and any range allowed --, jx uniform in
  [0.3, 1.7] with one entry 0 and one -0.8, jz uniform in [-1, 1.5]."""
  n = CASES[cid]['n']
  rng = np.random.default_rng(_case_seed(cid) + 3)
  out = []
  while len(out) < n + 5:
    i, j = (int(x) for x in rng.integers(0, n, 2))
    if i != j:
      out.append((i, j))
  jx = rng.uniform(0.3, 1.7, len(out)).astype(np.float32)
  jx[3], jx[7] = 0.0, -0.8
  jz = rng.uniform(-1.0, 1.5, len(out)).astype(np.float32)
  return out, jx, jz


@functools.lru_cache(maxsize=None)
def start(cid):
  """The chains every test of the case starts from."""
  c = CASES[cid]
  return vo.random_configurations(c['n'], c['b_chains'], np.random.RandomState(c.get('start_seed', _case_seed(cid) + 4)))


@functools.lru_cache(maxsize=None)
def pool(cid):
  """2 B + 3 host rows for the row blocks of amplitude(rows)."""
  c = CASES[cid]
  return vo.random_configurations(c['n'], 2 * c['b_chains'] + 3, np.random.RandomState(_case_seed(cid) + 5))


ROW_BLOCK_CASES = ('S1', 'S4')                  # amplitude(rows) in blocks of B rows runs on these


def compared_rows(cid):
  """Every row whose logit and sign a GPU test compares with the oracle."""
  return np.concatenate([start(cid), pool(cid)]) if cid in ROW_BLOCK_CASES else start(cid)


def chain_ids(cid):
  c = CASES[cid]
  return c['offset'] + np.arange(c['b_chains'])


def proposals(cid, configs, step):
  """(i_up, i_dn, u) of `step` on `configs`: the oracle's Philox with the case's offset chain ids."""
  c = CASES[cid]
  u_sites, u = vo.step_uniforms(SEED, chain_ids(cid), step, c['n'])
  i_up, i_dn = vo.propose_exchange(configs, u_sites)
  return i_up.astype(np.int32), i_dn.astype(np.int32), u


def banded(ratio, u):
  r = np.abs(np.asarray(ratio, np.float64))
  with np.errstate(invalid='ignore'):
    return np.abs(r - np.sqrt(np.asarray(u, np.float64))) < BAND * r


class Replay:
  """mc_steps(n) by the oracle: chains after the last step, accepts per step [n], chains that ever had a banded verdict."""

  def __init__(self, configs, accepts, band):
    self.configs, self.accepts, self.band = configs, accepts, band
    self.accepted = int(accepts.sum())
    self.share = accepts.sum() / float(accepts.size)


def replay_from(cid, prod, configs, step0, n_steps):
  cur, band = np.asarray(configs, np.float32).copy(), np.zeros(len(configs), bool)
  accepts = np.zeros((n_steps, len(configs)), bool)
  for k in range(n_steps):
    i_up, i_dn, u = proposals(cid, cur, step0 + k)
    cur, acc, ratio = pro.mc_step(prod, cur, i_up, i_dn, u)
    band |= banded(ratio, u)
    accepts[k] = acc
  return Replay(cur, accepts, band)


@functools.lru_cache(maxsize=None)
def replay(cid):
  """The replay of mc_steps(steps) from start(cid) at step 0."""
  return replay_from(cid, product_of(cid), start(cid), 0, CASES[cid]['steps'])


@functools.lru_cache(maxsize=None)
def eval_replay():
  """evaluate(None, n_eq, 3, n_mc) on S1 from start('S1') at step 0: (Replay of the equilibration, [Replay per sample])."""
  prod, e = product_of('S1'), EVAL
  eq = replay_from('S1', prod, start('S1'), 0, e['n_eq'])
  cur, step, samples = eq.configs, e['n_eq'], []
  for _ in range(e['n_samples']):
    samples.append(replay_from('S1', prod, cur, step, e['n_mc']))
    cur, step = samples[-1].configs, step + e['n_mc']
  return eq, samples


# ---- tolerances: each factor's own test bound; the product is held to their sum
def _factor_logit(f, configs):
  with np.errstate(divide='ignore'):
    return np.log(np.abs(np.asarray(f.psi(configs), np.float64))) + f.shift


def logit_bound(prod, configs, only=None):
  """Per row: dense 2e-5 max(1, |logit_f|) (tests/test_gpu_random_shapes.py), pbdg 64 (N/2) eps32 kappa(M)
  (tests/test_gpu_pbdg.py), ed_vector 4 eps32 |ln|v|| + eps32 (tests/test_gpu_edvec.py), summed over the factors (only: over the factors of that kind)."""
  n = np.asarray(configs).shape[1]
  out = np.zeros(len(configs))
  for f in (prod.a, prod.b):
    if only is not None and f.kind != only:
      continue
    if f.kind == 'pbdg':
      out += 64 * (n // 2) * EPS32 * po.condition_numbers(f.theta, configs)
    elif f.kind == 'ed_vector':
      out += 4 * EPS32 * np.abs(_factor_logit(f, configs)) + EPS32
    else:
      out += 2e-5 * np.maximum(1.0, np.abs(_factor_logit(f, configs)))
  return out


def pbdg_logit_bound(prod, configs):
  """The pbdg part of logit_bound alone (0 without a pbdg factor)."""
  n = np.asarray(configs).shape[1]
  return sum(64 * (n // 2) * EPS32 * po.condition_numbers(f.theta, configs) for f in (prod.a, prod.b) if f.kind == 'pbdg') + np.zeros(len(configs))


def edvec_eloc_bound(vec, configs, bond_list, jx, jz):
  """tests/test_gpu_prod.py's _edvec_eloc_bound at any size: (n_b + 3) 2^-24 (|diag| + sum|terms|) of the vector's own terms."""
  top, bot, _ = eo.lin_tables(np.asarray(configs).shape[1])
  diag, terms = eo.local_energy_terms(vec, configs, top, bot, bond_list, jx, jz)
  return ((terms != 0).sum(1) + 3) * 2.0 ** -24 * (np.abs(diag) + np.abs(terms).sum(1))


def eloc_bound(prod, configs, ref, bond_list, jx, jz, only=None):
  """Per row: dense 3e-4 max(1, |ref|) (tests/test_gpu_random_shapes.py), pbdg 2e-3 |ref| + 2e-3 mean|ref|
  (tests/test_gpu_pbdg.py), ed_vector edvec_eloc_bound, summed over the factors."""
  ref = np.abs(np.asarray(ref, np.float64))
  out = np.zeros(len(ref))
  for f in (prod.a, prod.b):
    if only is not None and f.kind != only:
      continue
    if f.kind == 'pbdg':
      out += 2e-3 * ref + 2e-3 * ref.mean()
    elif f.kind == 'ed_vector':
      out += edvec_eloc_bound(f.theta, configs, bond_list, jx, jz)
    else:
      out += 3e-4 * np.maximum(1.0, ref)
  return out


def scalar_rtol(prod):
  """The scalar accumulator slots, relative (tests/test_gpu_prod.py's sc_tol): dense 2e-4, pbdg 2e-3; ed_vector adds its
  own absolute term where it is used."""
  return sum({'pbdg': 2e-3, 'ed_vector': 0.0}.get(f.kind, 2e-4) for f in (prod.a, prod.b))


# ---- injected steps with bad and zero moves
def expected_step(prod, configs, i_up, i_dn, u):
  """pro.mc_step on the chains whose proposal names an up site to lower and a down site to raise; a chain whose
  proposal does not stays as it is, mask false.  -> (new configs, mask, psi'/psi (NaN on the bad chains), bad)."""
  cfg = np.asarray(configs, np.float32)
  rows = np.arange(len(cfg))
  bad = ~((cfg[rows, i_up] > 0) & (cfg[rows, i_dn] < 0))
  ok_up = np.array([np.flatnonzero(r > 0)[0] for r in cfg])
  ok_dn = np.array([np.flatnonzero(r < 0)[0] for r in cfg])
  new, acc, ratio = pro.mc_step(prod, cfg, np.where(bad, ok_up, i_up), np.where(bad, ok_dn, i_dn), u)
  new[bad] = cfg[bad]
  acc = acc & ~bad
  ratio = np.where(bad, np.nan, ratio)
  return new, acc, ratio, bad


class Script:
  """A product, its start chains and a list of injected steps (i_up, i_dn, u) with the oracle's verdict on each:
  per step the chains after it, the mask, and the chains of each group."""

  def __init__(self, cid, specs_, prod, configs, steps):
    self.cid, self.specs, self.prod, self.start = cid, specs_, prod, configs
    self.steps, self.after, self.masks, self.bads = steps, [], [], []
    self.zero_start = self.zero_cand = self.bad = 0
    self.first_nonzero_accepts = 0
    self.band = np.zeros(len(configs), bool)
    cur = configs
    for (i_up, i_dn, u) in steps:
      p0 = prod.psi(cur)
      new, acc, ratio, bad = expected_step(prod, cur, i_up, i_dn, u)
      cand = cur.copy()
      rows = np.flatnonzero(~bad)
      cand[rows, i_up[rows]] = -1.0; cand[rows, i_dn[rows]] = 1.0
      p1 = prod.psi(cand)
      self.zero_start += int(((p0 == 0) & ~bad).sum())
      self.first_nonzero_accepts += int(((p0 == 0) & ~bad & (p1 != 0) & acc).sum())
      self.zero_cand += int(((p1 == 0) & ~bad & ~acc).sum())
      self.bad += int(bad.sum())
      live = ~bad & (p0 != 0) & (p1 != 0)
      self.band |= live & banded(np.where(live, ratio, 1.0), np.where(live, u, 0.0))
      self.after.append(new); self.masks.append(acc); self.bads.append(bad)
      cur = new


def _valid_proposals(rng, cur):
  i_up = np.array([rng.choice(np.flatnonzero(r > 0)) for r in cur], np.int32)
  i_dn = np.array([rng.choice(np.flatnonzero(r < 0)) for r in cur], np.int32)
  return i_up, i_dn


def _bad_step(rng, cur):
  """Chains 0, 1: i_up names a down site; 2, 3: i_dn names an up site; 4: both; the others a valid proposal."""
  i_up, i_dn = _valid_proposals(rng, cur)
  for ch in range(min(5, len(cur))):
    up, dn = np.flatnonzero(cur[ch] > 0), np.flatnonzero(cur[ch] < 0)
    if ch in (0, 1, 4):
      i_up[ch] = rng.choice(dn)
    if ch in (2, 3, 4):
      i_dn[ch] = rng.choice(up)
  return i_up, i_dn


@functools.lru_cache(maxsize=None)
def script_edvec():
  """S3 with zeros in the vector: chains 0-2 start on a zero entry (chain 0's first candidate is a zero as well, so it
  leaves on the second step), the first candidates of chains 3 and 4 are zeros; then a step of bad proposals and two
  more ordinary steps."""
  cid = 'S3'
  n = CASES[cid]['n']
  top, bot, _ = eo.lin_tables(n)
  ta, vec = thetas(cid)
  vec = vec.copy()
  cfg = start(cid)
  rng = np.random.default_rng(31)
  first = _valid_proposals(rng, cfg)
  cand = cfg.copy()
  rows = np.arange(len(cfg))
  cand[rows, first[0]] = -1.0; cand[rows, first[1]] = 1.0
  idx0, idx1 = eo.index(cfg, top, bot), eo.index(cand, top, bot)
  vec[idx0[:3]] = 0.0
  vec[idx1[[0, 3, 4]]] = 0.0
  steps = [first + (rng.random(len(cfg)).astype(np.float32),)]
  prod = product_of(cid, ta, vec)
  cur = expected_step(prod, cfg, *steps[0])[0]
  for k in range(4):
    pr = _bad_step(rng, cur) if k == 1 else _valid_proposals(rng, cur)
    steps.append(pr + (rng.random(len(cfg)).astype(np.float32),))
    cur = expected_step(prod, cur, *steps[-1])[0]
  return Script(cid, specs(cid), prod, cfg, steps)


@functools.lru_cache(maxsize=None)
def script_singular_pbdg():
  """A copy of S1 whose pairing matrix has rows 0 and 1 equal: psi_b = 0 wherever sites 0 and 1 are both up.  Chains
  0-2 start there; chain 0's first candidate keeps both twins up (zero to zero: it stays), chains 1 and 2 lower a twin;
  the first candidates of chains 3 and 4 raise the second twin (a zero: rejected); then bad proposals, then two
  ordinary steps."""
  cid = 'S1'
  n, b = CASES[cid]['n'], CASES[cid]['b_chains']
  ta, tb = thetas(cid)
  f = tb.copy().reshape(n, n)
  f[1] = f[0]
  cfg = start(cid).copy()
  rng = np.random.default_rng(32)
  for ch in range(b):
    want = (1.0, 1.0) if ch < 3 else (1.0, -1.0) if ch < 5 else (-1.0, -1.0)
    for site, v in zip((0, 1), want):
      if cfg[ch, site] != v:
        other = rng.choice(np.flatnonzero(cfg[ch, 2:] == v)) + 2
        cfg[ch, site], cfg[ch, other] = v, -v
  assert (cfg.sum(1) == 0).all()
  i_up, i_dn = _valid_proposals(rng, cfg)
  i_up[0] = rng.choice(np.flatnonzero(cfg[0, 2:] > 0)) + 2       # both twins stay up
  i_up[1], i_up[2] = 0, 1
  for ch in (3, 4):
    i_up[ch] = rng.choice(np.flatnonzero(cfg[ch, 2:] > 0)) + 2
    i_dn[ch] = 1
  steps = [(i_up, i_dn, rng.random(b).astype(np.float32))]
  # (numpy's fp64 determinant of a matrix with two equal rows is a rounding residue, 1e-17 of the entries' product, not
  # 0: the oracle's factor is told where the rows coincide, as tests/test_gpu_prod.py tells its assertions)
  twin = pro.pbdg_factor(f.ravel())
  raw = twin.psi
  twin.psi = lambda c: np.where((np.asarray(c)[:, 0] > 0) & (np.asarray(c)[:, 1] > 0), 0.0, raw(c))
  prod = pro.Product(factor_of(CASES[cid]['a'], n, ta), twin)
  cur = expected_step(prod, cfg, *steps[0])[0]
  for k in range(4):
    pr = _bad_step(rng, cur) if k == 1 else _valid_proposals(rng, cur)
    steps.append(pr + (rng.random(b).astype(np.float32),))
    cur = expected_step(prod, cur, *steps[-1])[0]
  return Script(cid, specs(cid), prod, cfg, steps)


SCRIPTS = {'edvec': script_edvec, 'singular_pbdg': script_singular_pbdg}


# ---- the supervisor of the accumulator tests
@functools.lru_cache(maxsize=None)
def omega_thetas(cid):
  """tests/test_gpu_prod.py's perturbed supervisor: theta + 0.3 N(0, 1) mean|theta| over [a | b]."""
  ta, tb = thetas(cid)
  th = np.concatenate([ta, tb]).astype(np.float64)
  rng = np.random.default_rng(CASES[cid].get('omega_seed', _case_seed(cid) + 9))
  tw = (th + 0.3 * rng.standard_normal(th.size) * np.abs(th).mean()).astype(np.float32)
  return tw[:ta.size], tw[ta.size:]


def itswo_reference(cid, beta=0.05):
  """(Accumulators, E_loc of omega, ratio, omega) of LogOverlapITSWO on start(cid) with the supervisor of omega_thetas."""
  prod = product_of(cid)
  omega = product_of(cid, *omega_thetas(cid))
  bond_list, jx, jz = bonds(cid)
  acc = vo.Accumulators(prod.num_params, np.float64)
  e_w, ratio = pro.log_overlap_accumulate(acc, prod, omega, start(cid), bond_list, jx, jz, beta)
  return acc, e_w, ratio, omega
