"""The inputs of the sample-space solve's shape tests (tests/test_gpu_sr_gram_shapes.py).  One place, importable without a
GPU, so that tests/test_sr_gram.py proves on the fp64 references alone what the GPU tests take for granted: the shapes
reach what their rows promise, the rows are nearly all distinct, the truncation points lie inside the solve, and plain
fp32 arithmetic stays within the recorded share of the magnitude sum M (sr_gram_cases.gram_magnitude).

What each case reaches in csrc/srgram.hip (n = stored batches x B samples, row stride = reserved batches x B):
  full128    exactly one full tile, no ragged row or column
  one_over   a second tile row of one sample: a 1 x 1 diagonal tile, 128 x 1 off-diagonal tiles
  big_deep   nt = 9, 45 workgroups, a ragged last tile of 76; stride 1375 != 1100 rows; K = 33, one column past a chunk
             of 32; four layer terms; n % 4 == 0 with n / 4 > 64: a second trip of the float4 matvec; n > 1024: a second
             trip of every single-workgroup loop
  odd1025    the scalar matvec with 17 trips per lane; exactly one element in the second trip of the 1024-thread loops
  rbm1040    the onsite term at nt = 9
  tanh1100   big_deep with the deltas of a smooth activation
  sig516, cos516   the two other derivative shapes on a ragged 5-tile grid
"""
import collections
import functools

import numpy as np

from tests import sr_gram_cases as sg

N = 16                     # 12,870 Sz = 0 configurations: the rows are nearly all distinct
LAM = 1e-2
TILE = 128                 # plan.hpp SRG_TILE
CHUNK = 32                 # plan.hpp SRG_KC
LOOP = 1024                # srgram.hip: the threads of the single-workgroup length-n kernels
ROW_SEED = 10              # sr_gram_cases.draw_rows: one stream per case, cut into the batches

Shape = collections.namedtuple('Shape', 'ansatz h L b stored reserved act')

CASES = {
    'full128': Shape('fully_connected', 16, 2, 64, 2, 2, 'relu'),
    'one_over': Shape('fully_connected', 16, 2, 43, 3, 3, 'relu'),
    'big_deep': Shape('fully_connected', 33, 3, 275, 4, 5, 'relu'),
    'odd1025': Shape('fully_connected', 32, 1, 205, 5, 5, 'relu'),
    'rbm1040': Shape('rbm', 20, 1, 260, 4, 4, 'relu'),
    'tanh1100': Shape('fully_connected', 33, 3, 275, 4, 5, 'tanh'),
    'sig516': Shape('fully_connected', 24, 2, 129, 4, 4, 'sigmoid'),
    'cos516': Shape('fully_connected', 24, 2, 129, 4, 4, 'cos'),
}
IDS = list(CASES)
ROWS = {cid: s.stored * s.b for cid, s in CASES.items()}

STOP_CASES = ('one_over', 'big_deep')          # the exact stop and the truncated solves
EXACT_STOP_CASES = ('full128',) + STOP_CASES   # ... the exact stop also where it falls one iteration short of a group's end
TRUNCATIONS = (0, 1, 3, 8, 9, 13)              # max_iter: none, inside the first group of 8, its end, inside the second
AGREE_CASES = ('big_deep', 'rbm1040', 'tanh1100')
GROW_CASE = 'big_deep'

# Worst |gram_fp32 - gram_ref| / M per case as measured on the CPU (numpy float32, BLAS sgemm).  tests/test_sr_gram.py
# re-measures it and takes a figure within [1 / FP32_ROOM, FP32_ROOM] of the recorded one -- another BLAS sums in another
# order.  The GPU bound is c = GRAM_FACTOR x the recorded figure: the factor covers the MFMA's order of summation, the
# device's own forward and backward rounding and, off relu, its activation functions.
FP32_RATIO = {
    'full128': 2.63e-7,
    'one_over': 2.63e-7,
    'big_deep': 3.59e-7,
    'odd1025': 2.59e-7,
    'rbm1040': 3.43e-7,
    'tanh1100': 2.78e-7,
    'sig516': 2.76e-7,
    'cos516': 3.46e-7,
}
FP32_ROOM = 1.25
GRAM_FACTOR = 16
GRAM_GLOBAL = 2e-4                             # tests/test_gpu_sr_gram.py: |d| <= 2e-4 max|T|, kept; no c may exceed it


def gram_c(cid):
  return GRAM_FACTOR * FP32_RATIO[cid]


@functools.lru_cache(maxsize=None)
def inputs(cid):
  """(theta, the n rows in recording order, rejected draws) of a case; read-only."""
  s = CASES[cid]
  theta = sg.make_theta(s.ansatz, N, s.h, s.L)
  cfgs, rejected = sg.draw_rows(s.ansatz, theta, N, s.h, s.L, ROWS[cid], ROW_SEED, s.act)
  theta.setflags(write=False)
  cfgs.setflags(write=False)
  return theta, cfgs, rejected


def batches(cid):
  """The rows of a case as the engine records them: `stored` batches of B."""
  s = CASES[cid]
  cfgs = inputs(cid)[1]
  return [cfgs[k * s.b:(k + 1) * s.b] for k in range(s.stored)]
