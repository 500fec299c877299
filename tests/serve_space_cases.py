"""The case table of the serving path's argument space and its tie budget: plain CPU code (numpy and tests/serve_reference.py).

Cases of risp_serve_u8, risp_serve_u8_cfa and risp_serve_classical_u8 - shape, white and black level, Bayer phase, demosaic
kind or bilateral form, stage list, channel order - with their inputs, parameter blocks and float64 reference, and the
recorded float32 error E32 that sets TAU of the comparison rule (serve_reference.check):

  * decided pixel (every inner quantisation point - demosaic code, bilateral code, tone-curve code - further than TAU from a
    rounding boundary): each byte whose final truncation is further than TAU from an integer EQUALS the reference;
  * final tie: a byte of a decided pixel within TAU at the final truncation may differ by at most 1;
  * inner tie: a pixel within TAU at an inner point is excused;
  * caps, properties of the input and the reference alone: at most TIE_CAP = 2e-3 of a case's pixels at an inner tie and at
    most 1e-2 of its bytes under the +-1 rule; an input over a cap is drawn again with the next seed, 8 draws at most.

tests/test_gpu_serve_space.py runs every case through the C ABI and the functional wrapper; tests/test_serve_reference_cpu.py
checks the coverage, the caps of every input, E32, and that the rule tells fourteen wrong variants of the reference apart."""
import functools

import numpy as np

import serve_reference as S
from serve_reference import (OP_SKIP, OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3, OP_TONE_CRYSIS,
                             OP_TONE_FILMIC)

# ---------------------------------------------------------------------------------------------------- the axes
# the sizes tests/test_gpu_serve_classical.py and tests/test_gpu_serve_cfa.py give reasons for (a thread owns a 2 x 4 patch, a
# workgroup a 64 x 32 pixel tile): border-only patches, a left and a right border patch, the first interior patch, a tile
# crossed both ways, a grid of eight tiles (XCD-aware order)
SHAPES_CLASSICAL = ['1x4x4', '3x4x4', '1x4x8', '3x6x12', '3x34x68', '8x32x64']
SHAPES_SERVE = ['1x2x4', '3x10x12', '3x34x68', '8x32x64']
DEPTHS = ['1023/0', '1023/64', '16383/512', '65535/0']               # white level / black level
WB, GA, GT, WQ, G3, CR, FI = OP_WB_MANUAL, OP_GAMMA, OP_GTM_MANUAL, OP_WB_QUADRATIC, OP_GAIN3, OP_TONE_CRYSIS, OP_TONE_FILMIC
TAILS = {
    'none': [], 'crysis': [CR], 'filmic-wb-gamma': [FI, WB, GA], 'wb-filmic-gamma': [WB, FI, GA], 'gamma-filmic': [GA, FI],
    'crysis-gtm': [CR, GT], 'wb-crysis-gamma': [WB, CR, GA], 'gain3-crysis': [G3, CR],
    'full8': [WB, CR, GA, GT, FI, G3, GA, WQ], 'skips': [OP_SKIP, FI, OP_SKIP], 'gamma-wbq': [GA, WQ], 'gtm': [GT], 'wb': [WB],
    'gain3': [G3], 'gamma': [GA],
    # serve_u8 only (element-wise)
    'wb-gamma-gtm': [WB, GA, GT], 'wbq5': [WB, GA, GT, WQ, G3], 'skip-gamma': [OP_SKIP, GA],
}
# WbQuadratic stands where its input is bounded by 1 and nothing steep follows it: the polynomial cancels (coefficients
# 10 p - 5 around 0), and behind it a gain of 5, the toe of a gamma or Crysis with lum_adapted 0 (slope 10) multiply its fp32
# error, in the reference's own float32 evaluation, past what the caps below leave room for
WINDOWS = {'none': None, 'w3': (3, 1, 3, 1), 'w1': (1,)}               # per-image windows, cycled; 'w3' runs under max_window 3
SIGMAS = [0.05, 10.0, 100.0]                                          # of tests/test_gpu_serve_cfa.py

# (entry, shape, white/black, phase, demosaic kind | bilateral form, tail, reverse): 'c' risp_serve_classical_u8, 's'
# risp_serve_u8 (RGGB with black level 0) / risp_serve_u8_cfa.  Coverage is checked by tests/test_serve_reference_cpu.py
CASES = [
    ('c', '1x4x4', '1023/0', 'rggb', 'nearest', 'none', 0),
    ('c', '1x4x4', '1023/64', 'rggb', 'bilinear', 'crysis', 0),
    ('c', '1x4x4', '16383/512', 'rggb', 'laplacian', 'filmic-wb-gamma', 0),
    ('c', '1x4x4', '1023/64', 'grbg', 'nearest', 'wb-filmic-gamma', 1),
    ('c', '1x4x4', '16383/512', 'grbg', 'bilinear', 'gamma-filmic', 1),
    ('c', '1x4x4', '65535/0', 'grbg', 'laplacian', 'crysis-gtm', 1),
    ('c', '1x4x4', '16383/512', 'gbrg', 'nearest', 'wb-crysis-gamma', 0),
    ('c', '1x4x4', '65535/0', 'gbrg', 'bilinear', 'gain3-crysis', 0),
    ('c', '1x4x4', '1023/0', 'gbrg', 'laplacian', 'full8', 0),
    ('c', '1x4x4', '65535/0', 'bggr', 'nearest', 'skips', 1),
    ('c', '1x4x4', '1023/0', 'bggr', 'bilinear', 'gamma-wbq', 1),
    ('c', '1x4x4', '1023/64', 'bggr', 'laplacian', 'gtm', 1),
    ('c', '3x4x4', '1023/64', 'rggb', 'nearest', 'wb', 0),
    ('c', '3x4x4', '16383/512', 'rggb', 'bilinear', 'gain3', 0),
    ('c', '3x4x4', '65535/0', 'rggb', 'laplacian', 'gamma', 0),
    ('c', '3x4x4', '16383/512', 'grbg', 'nearest', 'none', 1),
    ('c', '3x4x4', '65535/0', 'grbg', 'bilinear', 'crysis', 1),
    ('c', '3x4x4', '1023/0', 'grbg', 'laplacian', 'filmic-wb-gamma', 1),
    ('c', '3x4x4', '65535/0', 'gbrg', 'nearest', 'wb-filmic-gamma', 0),
    ('c', '3x4x4', '1023/0', 'gbrg', 'bilinear', 'gamma-filmic', 0),
    ('c', '3x4x4', '1023/64', 'gbrg', 'laplacian', 'crysis-gtm', 0),
    ('c', '3x4x4', '1023/0', 'bggr', 'nearest', 'wb-crysis-gamma', 1),
    ('c', '3x4x4', '1023/64', 'bggr', 'bilinear', 'gain3-crysis', 1),
    ('c', '3x4x4', '16383/512', 'bggr', 'laplacian', 'full8', 1),
    ('c', '1x4x8', '16383/512', 'rggb', 'nearest', 'skips', 0),
    ('c', '1x4x8', '65535/0', 'rggb', 'bilinear', 'gamma-wbq', 0),
    ('c', '1x4x8', '1023/0', 'rggb', 'laplacian', 'gtm', 0),
    ('c', '1x4x8', '65535/0', 'grbg', 'nearest', 'wb', 1),
    ('c', '1x4x8', '1023/0', 'grbg', 'bilinear', 'gain3', 1),
    ('c', '1x4x8', '1023/64', 'grbg', 'laplacian', 'gamma', 1),
    ('c', '1x4x8', '1023/0', 'gbrg', 'nearest', 'none', 0),
    ('c', '1x4x8', '1023/64', 'gbrg', 'bilinear', 'crysis', 0),
    ('c', '1x4x8', '16383/512', 'gbrg', 'laplacian', 'filmic-wb-gamma', 0),
    ('c', '1x4x8', '1023/64', 'bggr', 'nearest', 'wb-filmic-gamma', 1),
    ('c', '1x4x8', '16383/512', 'bggr', 'bilinear', 'gamma-filmic', 1),
    ('c', '1x4x8', '65535/0', 'bggr', 'laplacian', 'crysis-gtm', 1),
    ('c', '3x6x12', '65535/0', 'rggb', 'nearest', 'wb-crysis-gamma', 0),
    ('c', '3x6x12', '1023/0', 'rggb', 'bilinear', 'gain3-crysis', 0),
    ('c', '3x6x12', '1023/64', 'rggb', 'laplacian', 'full8', 0),
    ('c', '3x6x12', '1023/0', 'grbg', 'nearest', 'skips', 1),
    ('c', '3x6x12', '1023/64', 'grbg', 'bilinear', 'gamma-wbq', 1),
    ('c', '3x6x12', '16383/512', 'grbg', 'laplacian', 'gtm', 1),
    ('c', '3x6x12', '1023/64', 'gbrg', 'nearest', 'wb', 0),
    ('c', '3x6x12', '16383/512', 'gbrg', 'bilinear', 'gain3', 0),
    ('c', '3x6x12', '65535/0', 'gbrg', 'laplacian', 'gamma', 0),
    ('c', '3x6x12', '16383/512', 'bggr', 'nearest', 'none', 1),
    ('c', '3x6x12', '65535/0', 'bggr', 'bilinear', 'crysis', 1),
    ('c', '3x6x12', '1023/0', 'bggr', 'laplacian', 'filmic-wb-gamma', 1),
    ('c', '3x34x68', '1023/0', 'rggb', 'nearest', 'wb-filmic-gamma', 0),
    ('c', '3x34x68', '1023/64', 'rggb', 'bilinear', 'gamma-filmic', 0),
    ('c', '3x34x68', '16383/512', 'rggb', 'laplacian', 'crysis-gtm', 0),
    ('c', '3x34x68', '1023/64', 'grbg', 'nearest', 'wb-crysis-gamma', 1),
    ('c', '3x34x68', '16383/512', 'grbg', 'bilinear', 'gain3-crysis', 1),
    ('c', '3x34x68', '65535/0', 'grbg', 'laplacian', 'full8', 1),
    ('c', '3x34x68', '16383/512', 'gbrg', 'nearest', 'skips', 0),
    ('c', '3x34x68', '65535/0', 'gbrg', 'bilinear', 'gamma-wbq', 0),
    ('c', '3x34x68', '1023/0', 'gbrg', 'laplacian', 'gtm', 0),
    ('c', '3x34x68', '65535/0', 'bggr', 'nearest', 'wb', 1),
    ('c', '3x34x68', '1023/0', 'bggr', 'bilinear', 'gain3', 1),
    ('c', '3x34x68', '1023/64', 'bggr', 'laplacian', 'gamma', 1),
    ('c', '8x32x64', '1023/64', 'rggb', 'nearest', 'filmic-wb-gamma', 0),
    ('c', '8x32x64', '16383/512', 'rggb', 'bilinear', 'crysis', 0),
    ('c', '8x32x64', '65535/0', 'rggb', 'laplacian', 'none', 0),
    ('c', '8x32x64', '16383/512', 'grbg', 'nearest', 'wb-filmic-gamma', 1),
    ('c', '8x32x64', '65535/0', 'grbg', 'bilinear', 'gamma-filmic', 1),
    ('c', '8x32x64', '1023/0', 'grbg', 'laplacian', 'crysis-gtm', 1),
    ('c', '8x32x64', '65535/0', 'gbrg', 'nearest', 'wb-crysis-gamma', 0),
    ('c', '8x32x64', '1023/0', 'gbrg', 'bilinear', 'gain3-crysis', 0),
    ('c', '8x32x64', '1023/64', 'gbrg', 'laplacian', 'full8', 0),
    ('c', '8x32x64', '1023/0', 'bggr', 'nearest', 'skips', 1),
    ('c', '8x32x64', '1023/64', 'bggr', 'bilinear', 'gamma-wbq', 1),
    ('c', '8x32x64', '16383/512', 'bggr', 'laplacian', 'gtm', 1),
    ('c', '3x6x12', '1023/64', 'rggb', 'nearest', 'gain3-crysis', 1),
    ('c', '3x6x12', '16383/512', 'grbg', 'laplacian', 'full8', 0),
    ('c', '3x4x4', '65535/0', 'gbrg', 'bilinear', 'skips', 1),
    ('c', '3x6x12', '1023/0', 'bggr', 'laplacian', 'gamma-wbq', 0),
    ('c', '3x4x4', '1023/64', 'grbg', 'bilinear', 'gtm', 1),
    ('c', '3x6x12', '16383/512', 'gbrg', 'nearest', 'wb', 0),
    ('c', '3x6x12', '65535/0', 'bggr', 'bilinear', 'gain3', 1),
    ('c', '3x6x12', '1023/0', 'rggb', 'laplacian', 'gamma', 0),
    ('c', '3x4x4', '1023/64', 'gbrg', 'bilinear', 'none', 1),
    ('c', '3x6x12', '16383/512', 'bggr', 'laplacian', 'crysis', 0),
    ('c', '3x4x4', '65535/0', 'rggb', 'nearest', 'filmic-wb-gamma', 1),
    ('c', '3x6x12', '1023/0', 'grbg', 'laplacian', 'wb-filmic-gamma', 0),
    ('c', '3x6x12', '1023/64', 'bggr', 'bilinear', 'gamma-filmic', 1),
    ('c', '3x6x12', '16383/512', 'rggb', 'laplacian', 'crysis-gtm', 0),
    ('c', '3x4x4', '65535/0', 'grbg', 'bilinear', 'wb-crysis-gamma', 1),
    ('c', '3x6x12', '1023/0', 'gbrg', 'nearest', 'gain3-crysis', 0),
    ('c', '3x4x4', '1023/64', 'rggb', 'bilinear', 'full8', 1),
    ('c', '3x6x12', '16383/512', 'grbg', 'laplacian', 'skips', 0),
    ('c', '3x6x12', '65535/0', 'gbrg', 'bilinear', 'gamma-wbq', 1),
    ('c', '3x6x12', '1023/0', 'bggr', 'laplacian', 'gtm', 0),
    ('c', '3x4x4', '1023/64', 'grbg', 'nearest', 'wb', 1),
    ('c', '3x6x12', '16383/512', 'gbrg', 'laplacian', 'gain3', 0),
    ('c', '3x4x4', '65535/0', 'bggr', 'bilinear', 'gamma', 1),
    ('c', '3x6x12', '1023/0', 'rggb', 'laplacian', 'none', 0),
    ('c', '3x6x12', '1023/64', 'gbrg', 'bilinear', 'crysis', 1),
    ('c', '3x6x12', '16383/512', 'bggr', 'nearest', 'filmic-wb-gamma', 0),
    ('c', '3x4x4', '65535/0', 'rggb', 'bilinear', 'wb-filmic-gamma', 1),
    ('c', '3x6x12', '1023/0', 'grbg', 'laplacian', 'gamma-filmic', 0),
    ('c', '3x4x4', '1023/64', 'bggr', 'bilinear', 'crysis-gtm', 1),
    ('c', '3x6x12', '16383/512', 'rggb', 'laplacian', 'wb-crysis-gamma', 0),
    ('s', '1x2x4', '1023/64', 'rggb', 'none', 'none', 0),
    ('s', '1x2x4', '16383/512', 'rggb', 'w3', 'wb-gamma-gtm', 0),
    ('s', '1x2x4', '65535/0', 'rggb', 'w1', 'wbq5', 1),
    ('s', '1x2x4', '16383/512', 'grbg', 'none', 'skip-gamma', 1),
    ('s', '1x2x4', '65535/0', 'grbg', 'w3', 'gain3', 0),
    ('s', '1x2x4', '1023/0', 'grbg', 'w1', 'gtm', 0),
    ('s', '1x2x4', '65535/0', 'gbrg', 'none', 'wb', 1),
    ('s', '1x2x4', '1023/0', 'gbrg', 'w3', 'gamma-wbq', 1),
    ('s', '1x2x4', '1023/64', 'gbrg', 'w1', 'none', 0),
    ('s', '1x2x4', '1023/0', 'bggr', 'none', 'wb-gamma-gtm', 0),
    ('s', '1x2x4', '1023/64', 'bggr', 'w3', 'wbq5', 1),
    ('s', '1x2x4', '16383/512', 'bggr', 'w1', 'skip-gamma', 1),
    ('s', '3x10x12', '16383/512', 'rggb', 'none', 'gain3', 0),
    ('s', '3x10x12', '65535/0', 'rggb', 'w3', 'gtm', 0),
    ('s', '3x10x12', '1023/0', 'rggb', 'w1', 'wb', 1),
    ('s', '3x10x12', '65535/0', 'grbg', 'none', 'gamma-wbq', 1),
    ('s', '3x10x12', '1023/0', 'grbg', 'w3', 'none', 0),
    ('s', '3x10x12', '1023/64', 'grbg', 'w1', 'wb-gamma-gtm', 0),
    ('s', '3x10x12', '1023/0', 'gbrg', 'none', 'wbq5', 1),
    ('s', '3x10x12', '1023/64', 'gbrg', 'w3', 'skip-gamma', 1),
    ('s', '3x10x12', '16383/512', 'gbrg', 'w1', 'gain3', 0),
    ('s', '3x10x12', '1023/64', 'bggr', 'none', 'gtm', 0),
    ('s', '3x10x12', '16383/512', 'bggr', 'w3', 'wb', 1),
    ('s', '3x10x12', '65535/0', 'bggr', 'w1', 'gamma-wbq', 1),
    ('s', '3x34x68', '65535/0', 'rggb', 'none', 'none', 0),
    ('s', '3x34x68', '1023/0', 'rggb', 'w3', 'wb-gamma-gtm', 0),
    ('s', '3x34x68', '1023/64', 'rggb', 'w1', 'wbq5', 1),
    ('s', '3x34x68', '1023/0', 'grbg', 'none', 'skip-gamma', 1),
    ('s', '3x34x68', '1023/64', 'grbg', 'w3', 'gain3', 0),
    ('s', '3x34x68', '16383/512', 'grbg', 'w1', 'gtm', 0),
    ('s', '3x34x68', '1023/64', 'gbrg', 'none', 'wb', 1),
    ('s', '3x34x68', '16383/512', 'gbrg', 'w3', 'gamma-wbq', 1),
    ('s', '3x34x68', '65535/0', 'gbrg', 'w1', 'none', 0),
    ('s', '3x34x68', '16383/512', 'bggr', 'none', 'wb-gamma-gtm', 0),
    ('s', '3x34x68', '65535/0', 'bggr', 'w3', 'wbq5', 1),
    ('s', '3x34x68', '1023/0', 'bggr', 'w1', 'skip-gamma', 1),
    ('s', '8x32x64', '1023/0', 'rggb', 'none', 'gain3', 0),
    ('s', '8x32x64', '1023/64', 'rggb', 'w3', 'gtm', 0),
    ('s', '8x32x64', '16383/512', 'rggb', 'w1', 'wb', 1),
    ('s', '8x32x64', '1023/64', 'grbg', 'none', 'gamma-wbq', 1),
    ('s', '8x32x64', '16383/512', 'grbg', 'w3', 'none', 0),
    ('s', '8x32x64', '65535/0', 'grbg', 'w1', 'wb-gamma-gtm', 0),
    ('s', '8x32x64', '16383/512', 'gbrg', 'none', 'wbq5', 1),
    ('s', '8x32x64', '65535/0', 'gbrg', 'w3', 'skip-gamma', 1),
    ('s', '8x32x64', '1023/0', 'gbrg', 'w1', 'gain3', 0),
    ('s', '8x32x64', '65535/0', 'bggr', 'none', 'gtm', 0),
    ('s', '8x32x64', '1023/0', 'bggr', 'w3', 'wb', 1),
    ('s', '8x32x64', '1023/64', 'bggr', 'w1', 'gamma-wbq', 1),
]
WALK = 16

# ---------------------------------------------------------------------------------------------------- the tie budget
# E32[kind]: the largest |v32 - v64|, in codes, at that kind of quantisation point over every input of CASES and the walk,
# where v32 is the reference's own expression evaluated in float32 on the CPU (exp as exp2(x * log2 e) in float32, the form
# of the kernel's fast exponential; every segment started from the float64 run's codes) and v64 the float64 reference.
# 'final/<op>': at the final truncation, by the last stage that left a float, over the values whose v * 255 lies in
# [0, 256].  TAU = 2 x E32, the factor of conftest.ErrorBudget and of TAU in tests/test_gpu_fused_segment.py: the HIP path
# may cost at most twice the reference's own fp32 arithmetic.  Nothing here is taken from a run of the kernels.  No
# documented error bound of the fast exponential was found in the ROCm documents of this build, so none is added.
# tests/test_serve_reference_cpu.py re-measures E32 and checks that the float32 evaluation itself passes the rule.
E32 = {
    'bilinear': 2.91e-5, 'laplacian': 5.67e-5, 'crysis': 3.19e-5, 'filmic': 1.24e-4, 'bilateral1': 1.76e-5, 'bilateral3': 5.89e-5,
    'final/nearest': 1.47e-5, 'final/wb_manual': 2.44e-5, 'final/gamma': 2.48e-5, 'final/gtm_manual': 1.53e-4,
    'final/wb_quadratic': 3.19e-4, 'final/gain3': 4.66e-4,
}
TAU = {k: 2.0 * v for k, v in E32.items()}


# ---------------------------------------------------------------------------------------------------- builders (CPU)
def _shape(name):
    return tuple(int(v) for v in name.split('x'))


def make_raw(n, h, w, white, black, seed):
    """(N,H,W) int64 samples that fit uint16: uniform up to 10 % above the white level where the type allows, planted samples
    above the white level, below and at the black level; image 1 all zero and image 2 constant (off the tie lattice of the
    2-sample mean: with 10-bit samples (a + b) / 2 * 255 / 1023 is an exact half-integer when a + b is an odd multiple of 341)"""
    rng = np.random.default_rng(seed)
    top = min(int(white * 1.1), 65535)
    raw = rng.integers(0, top + 1, size=(n, h, w), dtype=np.int64)
    raw[0, 0, 0] = top
    raw[0, 0, 1], raw[0, 1, 0], raw[0, -1, -1], raw[0, 1, 1] = max(black - 5, 0), max(black - 1, 0), black, white
    if n > 1:
        raw[1] = 0
    if n > 2:
        raw[2] = black + (white - black) // 3 + 1
    return raw


def make_params(ops, n, rng):
    """per-stage (N,P) float32 blocks as the C ABI takes them; the ranges of tests/test_gpu_serve_cfa.py and, for the tone
    curves, the edges of tests/test_gpu_serve_classical.py (lum_adapted 0 and 1; white_point 0, 0.005 - below the 0.01 floor -
    and 1; exposure_bias 1 and 10), image i taking entry i"""
    u = lambda k, a=0.0, b=1.0: rng.uniform(a, b, size=(n, k)).astype(np.float32)
    pick = lambda vals: np.array([vals[i % len(vals)] for i in range(n)], np.float32)
    out = []
    for op in ops:
        if op == OP_SKIP:
            out.append(None)
        elif op == OP_WB_MANUAL:
            out.append(u(3) * np.float32(5))
        elif op == OP_GAMMA:
            out.append(u(1, 0.2, 0.8))
        elif op == OP_GTM_MANUAL:
            out.append(np.sort(u(3), axis=1))
        elif op == OP_WB_QUADRATIC:
            out.append(u(30, 0.45, 0.55))
        elif op == OP_GAIN3:
            out.append(u(3, 0.5, 2.0))
        elif op == OP_TONE_CRYSIS:
            out.append(pick([rng.uniform(), 0.0, 1.0, rng.uniform()])[:, None])
        elif op == OP_TONE_FILMIC:
            out.append(np.stack([pick([rng.uniform(), 0.0, 0.005, 1.0]), pick([1.0 + 9.0 * rng.uniform(), 1.0, 10.0, 4.0])], axis=1))
        else:
            raise ValueError(op)
    return out


def _build(row, seed0, what):
    entry, shape, depth, phase, form, tail, reverse = row
    n, h, w = _shape(shape)
    white, black = (int(v) for v in depth.split('/'))
    ops = list(TAILS[tail]) if isinstance(tail, str) else list(tail)        # the walk hands its op list over
    case = dict(entry=entry, n=n, h=h, w=w, white=white, black=black, phase=phase, ops=ops, reverse=bool(reverse), what=what,
                params=make_params(ops, n, np.random.default_rng(seed0 + 1)), demosaic='nearest', bilateral=None, max_window=0)
    if entry == 'c':
        case['demosaic'] = form
    elif WINDOWS[form] is not None:
        pat = WINDOWS[form]
        case['bilateral'] = (np.array([pat[i % len(pat)] for i in range(n)], np.int32),
                             np.array([SIGMAS[i % 3] for i in range(n)], np.float32),
                             np.array([SIGMAS[(i + 1) % 3] for i in range(n)], np.float32))
        case['max_window'] = max(pat)
    for attempt in range(8):                                # an input over a cap is drawn again (the input's property alone)
        case['raw'] = make_raw(n, h, w, white, black, seed0 + 100 * attempt)
        case['ref'] = reference(case)
        inner, loose = S.tie_shares(case['ref'], TAU)
        if inner <= S.TIE_CAP and loose <= S.FINAL_CAP:
            case['draws'] = attempt + 1
            return case
    raise AssertionError('%s: no input under the caps in 8 draws (inner %.3e, +-1 bytes %.3e)' % (what, inner, loose))


def reference(case, dtype=np.float64, sync=None, reverse=None):
    return S.serve(case['raw'], case['white'], case['black'], case['phase'], case['demosaic'], case['bilateral'], case['ops'],
                   case['params'], case['reverse'] if reverse is None else reverse, dtype, sync)


@functools.lru_cache(maxsize=None)
def sweep_case(index):
    return _build(CASES[index], 7000 + 13 * index, 'case %d: %s %s %s %s %s %s reverse %d' % ((index,) + CASES[index]))


@functools.lru_cache(maxsize=None)
def walk_case(seed):
    """one step of the seeded walk over the same axes"""
    rng = np.random.default_rng(9100 + seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    entry = 'c' if rng.random() < 0.6 else 's'
    shape = pick(SHAPES_CLASSICAL[:5] if entry == 'c' else SHAPES_SERVE)     # (the eight-tile grid is in the table: at 16384 pixels
    # the exact ties of a 2-sample mean - one value in 514 at 16 bits - alone reach the cap)
    form = pick(list(S.DEMOSAIC)) if entry == 'c' else pick(list(WINDOWS))
    pool = ([WB, GA, GT, G3, OP_SKIP, CR, FI] if entry == 'c' else [WB, GA, GT, G3, OP_SKIP])
    ops, unit = [], form != 'nearest' and form != 'none'     # unit: the running value is known to lie in [0, 1]
    for _ in range(int(rng.integers(0, 9))):
        op = pick(pool + [WQ]) if unit else pick(pool)       # WbQuadratic only where its input is bounded by 1 (it squares it)
        unit = unit if op in (OP_SKIP, GA) else op != WB
        if op == WQ:                                         # nothing steep behind WbQuadratic (see TAILS)
            pool = [GT, G3, OP_SKIP]
        ops.append(op)
    row = (entry, shape, pick(DEPTHS), pick(list(S.SITES)), form, ops, int(rng.integers(0, 2)))
    return _build(row, 9500 + 17 * seed, 'walk %d: %s %s %s %s %s %s reverse %d' % ((seed,) + row))
