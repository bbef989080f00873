"""The cases of tests/test_gpu_conv_dma16.py and their float64 references (conv_ref.Ref), shared with the host check
tests/test_conv_dma16_cases_host.py.  Plain helpers, no fixtures.

The LDS-DMA kernels (csrc/conv_f16x3.hip, conv_igemm_f16x3_dma) build their wave tiles from 16-row / 16-filter blocks in default
arithmetic (v_mfma_f32_16x16x32_f16) and carry the fragments of the next K step across a mid-step barrier.  These are the shapes at
which that form can go wrong where the 32-row form could not; all of them are tiny."""
import functools

import numpy as np

import conv_ref as R

DMA_VARIANTS = (11, 12, 13, 14, 18, 19)      # conv_igemm_f16x3_dma<...>: 128x128 NS2, 256x128 NS3, 128x256 NS3, 128x128 NS3, 128x64 NS2, 64x128 NS2
SPLITK_VARIANTS = (21, 22)                   # ...+splitK on the 64x128 and the 128x128 tile

CASES = [  # n, h, w, cin, cout, k, s, act, res_mode
    # K steps against the ring depth: 1, 2, 3, 4 steps for NS = 2 and NS = 3; nine steps with a tap change every step
    (2, 5, 5, 32, 64, 1, 1, "leaky", 0),
    (2, 5, 5, 64, 64, 1, 1, "leaky", 0),
    (2, 5, 5, 96, 64, 1, 1, "leaky", 0),
    (2, 5, 5, 128, 64, 1, 1, "leaky", 0),
    (1, 8, 8, 32, 64, 3, 2, "leaky", 0),
    # 16-boundaries of the pixel axis: M = 15, 16, 17, 33
    (1, 3, 5, 64, 64, 1, 1, "leaky", 0),
    (1, 4, 4, 64, 64, 1, 1, "leaky", 0),
    (1, 1, 17, 64, 64, 1, 1, "leaky", 0),
    (1, 3, 11, 64, 64, 1, 1, "leaky", 0),
    # ... of the filter axis: Cout = 15, 16, 17, 33, and the head's 255 (all fp32 outputs)
    (1, 4, 5, 64, 15, 1, 1, "linear", 0),
    (1, 4, 5, 64, 16, 1, 1, "linear", 0),
    (1, 4, 5, 64, 17, 1, 1, "linear", 0),
    (1, 4, 5, 64, 33, 1, 1, "linear", 0),
    (1, 4, 5, 64, 255, 1, 1, "linear", 0),
    # strided 3x3 with odd extents: the rows of one 16-block straddle output rows and images
    (3, 7, 5, 32, 64, 3, 2, "leaky", 0),
    (3, 9, 11, 64, 96, 3, 2, "leaky", 0),
    # residual after / before the activation, mish: one 3x3 stride-2 and one 1x1 layer each
    (2, 7, 5, 32, 64, 3, 2, "mish", 1),
    (2, 7, 5, 32, 64, 3, 2, "relu", 2),
    (2, 4, 5, 64, 64, 1, 1, "mish", 1),
    (2, 4, 5, 64, 64, 1, 1, "relu", 2),
]

# forced split-K at the smallest layer its rule takes: nine K steps (3x3 on 32 channels) in two ranges of five and four
SPLITK_CASE = (1, 7, 5, 32, 64, 3, 2, "leaky", 0)

# one merged launch of two convolutions (test_gpu_conv_variants.py's VIEW_CASES layout):
# n, h, w, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off)
MERGED_CASE = (1, 5, 7, (64, 64, 0), (64, 64, 32), 1, 1, "leaky", (0, 0, 0), (32, 32, 0))


def merged_plain_case():
    n, h, wd, (cin, _, _), (cout, _, _), k, s, act, _, _ = MERGED_CASE
    return (n, h, wd, cin, cout, k, s, act, 0)


def all_cases():
    """every case as a plain 9-tuple, in the order of refs()"""
    return list(CASES) + [SPLITK_CASE, merged_plain_case()]


@functools.lru_cache(maxsize=None)
def refs():
    """conv_ref.Ref of every entry of all_cases() (one RandomState(61) stream in list order); computed once per process, read-only"""
    rng = np.random.RandomState(61)
    return tuple(R.Ref(c, *R.make_case(rng, *c[:7], c[8])) for c in all_cases())
