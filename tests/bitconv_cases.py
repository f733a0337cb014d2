"""The checker of the bit convolution (csrc/f110_bitconv.h), NumPy only: the numerics contract of include/f110_hip.h restated tap
by tap in float32 -- acc = 0; taps ky major, kx minor: acc = acc + w[c][ky][kx] where the tap's pixel is set; out = (acc * on) +
bias[c]; out < 0 ? 0 : out with relu -- so that the GPU's output can be compared with `==`, and the gradients in float64."""
import numpy as np

import replay_cases as rc

U = 2.0 ** -24                                 # unit roundoff of fp32

# (rows, cols, kernel, stride, channels): SAL's layer; cols no multiple of 64 with windows across the word boundary at every
# phase and an odd channel count; five words with a tail word and a stride that does not divide; one output; kernel 1 on three words
CASES = [(256, 256, 8, 4, 16), (75, 100, 3, 1, 5), (40, 300, 8, 3, 1), (8, 8, 8, 8, 64), (9, 130, 1, 1, 2)]
ONS = (1.0, 255.0, 1.0 / 255.0)
BACKWARD_CASES = CASES[:3]
BACKWARD_N = (3, 67)                           # 67: a count that no block size divides


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k fp32 roundings."""
    return k * U / (1.0 - k * U)


def out_size(rows, cols, kernel, stride):
    return (rows - kernel) // stride + 1, (cols - kernel) // stride + 1


def images(rows, cols):
    """The three images of a forward case: one of replay_cases.random_images, an all-set one, an empty one."""
    return np.stack([rc.random_images(rows, cols, n=1, seed=11)[0], np.full((rows, cols), 255, np.uint8), np.zeros((rows, cols), np.uint8)])


def many_images(rows, cols, n):
    """n images for the backward cases: random ones, the last all-set and the one before it empty (n >= 3)."""
    a = rc.random_images(rows, cols, n=n, seed=5)
    a[-1] = 255
    a[-2] = 0
    return a


def params(kernel, channels, seed=0):
    """weight [C, 1, k, k] and bias [C] in fp32 of mixed sign and magnitude (cancellation makes the order of the taps matter)."""
    rng = np.random.default_rng([kernel, channels, seed])
    w = (rng.normal(size=(channels, 1, kernel, kernel)) * 10.0 ** rng.integers(-2, 2, (channels, 1, kernel, kernel))).astype(np.float32)
    b = rng.normal(size=channels).astype(np.float32)
    return w, b


def taps(bits, kernel, stride):
    """bits [n, rows, cols] bool -> a list over the taps (ky major, kx minor) of [n, OH, OW] bool views: tap (ky, kx) of every window."""
    n, rows, cols = bits.shape
    oh, ow = out_size(rows, cols, kernel, stride)
    return [bits[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride] for ky in range(kernel) for kx in range(kernel)]


def forward(imgs, weight, bias, stride, on, relu):
    """The contract in float32 on uint8 images [n, rows, cols] (a pixel is set iff it == 255) -> [n, C, OH, OW] float32."""
    bits = np.asarray(imgs) == 255
    w = np.asarray(weight, np.float32)
    ch, _, k, _ = w.shape
    sel = taps(bits, k, stride)
    acc = np.zeros((bits.shape[0], ch) + sel[0].shape[1:], np.float32)
    zero = np.float32(0.0)
    for t, s in enumerate(sel):
        wt = w[:, 0, t // k, t % k]
        acc = acc + np.where(s[:, None], wt[None, :, None, None], zero).astype(np.float32)
        assert acc.dtype == np.float32
    b = np.zeros(ch, np.float32) if bias is None else np.asarray(bias, np.float32)
    out = (acc * np.float32(on)).astype(np.float32) + b[None, :, None, None]
    assert out.dtype == np.float32
    if relu:
        out = np.where(out < 0, zero, out).astype(np.float32)
    return out


def gradients(imgs, grad_out, kernel, stride, on):
    """In float64 with `on` as the fp32 the kernel multiplies by: (grad_weight [C, 1, k, k], grad_bias [C], sum |grad_out * bit|
    per weight, sum |grad_out| per channel) -- the last two scale the bounds of an fp32 sum."""
    bits = np.asarray(imgs) == 255
    g = np.asarray(grad_out, np.float64)
    ch = g.shape[1]
    on = float(np.float32(on))
    gw, aw = np.zeros((ch, 1, kernel, kernel)), np.zeros((ch, 1, kernel, kernel))
    for t, s in enumerate(taps(bits, kernel, stride)):
        gs = g * s[:, None]
        gw[:, 0, t // kernel, t % kernel] = on * gs.sum(axis=(0, 2, 3))
        aw[:, 0, t // kernel, t % kernel] = np.abs(gs).sum(axis=(0, 2, 3))
    return gw, g.sum(axis=(0, 2, 3)), aw, np.abs(g).sum(axis=(0, 2, 3))


def grad_bounds(imgs, grad_out, kernel, stride, on):
    """(bound on |grad_weight error|, bound on |grad_bias error|): M = n * OH * OW terms summed in fp32 in any order, gamma_M times
    the sum of magnitudes; one more rounding for the product with `on`."""
    g = np.asarray(grad_out)
    m = g.shape[0] * g.shape[2] * g.shape[3]
    _, _, aw, ab = gradients(imgs, grad_out, kernel, stride, on)
    return gamma(m + 1) * abs(float(np.float32(on))) * aw, gamma(m) * ab


def bit_patterns(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
