"""The checker of the stacked fused stem (csrc/f110_bitconv2.h bitconv2_forward_kernel<true>; f110_bitconv2_forward_stack's contract in
include/f110_hip.h), NumPy only.  The contract is the composition of two existing ones, and so is the checker: the stacked first layer
of stack_cases.forward_stack (frames j major, then ky, kx; `on`, bias and relu once, after the last frame), then the fma chain of
bitconv2_cases.accumulate2 / finish2.  Nothing is restated here."""
import numpy as np

import bitconv2_cases as b2
import replay_cases as rc
import stack_cases as sc

# the rows of b2.CASES2 the GPU test runs, for what a stacked layer 1 can get wrong
SAL, TALL, ODD, MONO, PIXEL, SEVEN = (b2.CASES2[i] for i in (0, 1, 3, 8, 9, 5))
STACK_CASES = (SAL, TALL, ODD, MONO, PIXEL, SEVEN)
STACKS = (2, 3, 8)
FRAMES = 6                                      # frames an index of the forward cases names


def frames_pool(rows, cols):
    """FRAMES images: the three of b2.images2 (arbitrary, all set, empty) and three seeded ones of half set pixels."""
    return np.concatenate([b2.images2(rows, cols), rc.random_images(rows, cols, n=FRAMES - 3, seed=5)])


def params_stem_stack(k1, c1, k, k2, c2, seed=0):
    """(w1 [C1, k, k1, k1], b1, w2, b2) in fp32 of mixed sign and magnitude: sc.params_stack for layer 1, b2.params2's draw for layer 2."""
    w1, b1 = sc.params_stack(k1, c1, k, seed)
    _, _, w2, bb = b2.params2(k1, c1, k2, c2, seed)
    return w1, b1, w2, bb


def accumulate_stack(imgs, index, w1, b1, s1, on, relu1, w2, s2):
    """Layer 2's fma chain on the stacked layer 1, before b2 and relu2 (the part a test computes once and shares)."""
    return b2.accumulate2(sc.forward_stack(imgs, index, w1, b1, s1, on, relu1), w2, s2)


def forward_stem_stack(imgs, index, w1, b1, s1, on, relu1, w2, bb, s2, relu2):
    """The contract on uint8 images [m, rows, cols] and index [n, k] -> [n, C2, OH2, OW2] float32."""
    return b2.finish2(accumulate_stack(imgs, index, w1, b1, s1, on, relu1, w2, s2), bb, relu2)
