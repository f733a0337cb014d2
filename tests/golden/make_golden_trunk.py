"""Generates tests/golden/g22_trunk.npz and g22_trunk_unit.npz from the reference's own Actor (src/SAL.py:390-411) on the CPU,
seeded, one thread: what conv2 and conv3 with their ReLU compute, forward and backward, on a two-valued block image.  Forward hooks
record conv2's input a1 = relu(conv1(x)), relu(conv2(a1)) and relu(conv3(.)); a seeded fp32 cotangent on the flattened features
that fc1 reads goes through backward(), and per layer the gradient that arrived at the layer's output after its ReLU (grad_out),
its grad_input, weight.grad and bias.grad are recorded, with the weights and biases of both layers.  The fixtures hold data only.
Two rows are recorded, each in a file of its own so that every committed file stays within LIMIT (1 MiB): g22_trunk.npz is the
row fed as the raw 0 / 255 floats (:536, what update() learns from), g22_trunk_unit.npz the row fed as FloatTensor(state) / 255
(:510).  Both come from the same seeded Actor; each row goes through it alone, so weight.grad and bias.grad are that row's.  One
file with both rows is 1.3 MB and does not compress further: the gradients are dense.  What another array already holds is not
stored twice: conv3's grad_out is `cotangent` reshaped to [1, 32, 28, 28], conv2's grad_out is `conv3_grad_input`.
The generator asserts, per recorded array v, |v - fp64| <= gamma(T) * mag: fp64 and mag = sum |terms| from featconv_cases' fp64
sums on the recorded inputs, T the number of terms of the sum, bias included.  torch's default CPU convolution (oneDNN) keeps that
bound here, so it stays enabled.  Run through make_golden.py.
"""
import numpy as np
import torch

import reference
import featconv_cases as fc
from reference import within

LIMIT = 1 << 20
FILES = (('g22_trunk.npz', 255.0), ('g22_trunk_unit.npz', 1.0))     # per file: the one recorded row and what a set pixel is worth in it


def record(sal, name, on, blocks):
    torch.manual_seed(22)
    actor = sal.Actor(action_dim=16)
    R = 1
    x = torch.from_numpy((np.kron(blocks, np.ones((8, 8))) * on).astype(np.float32))
    rec, grads = {}, {}

    def hook(layer):
        def fn(mod, inp, out):
            rec[layer + '_in'] = inp[0].detach().clone()
            rec[layer + '_out'] = torch.relu(out).detach().clone()
            inp[0].register_hook(lambda g: grads.__setitem__(layer + '_grad_input', g.detach().clone()))
        return fn

    feats = []
    handles = [actor.conv2.register_forward_hook(hook('conv2')), actor.conv3.register_forward_hook(hook('conv3')),
               actor.fc1.register_forward_pre_hook(lambda mod, inp: feats.append(inp[0]))]
    actor(x)
    for h in handles:
        h.remove()
    feat = feats[0]
    assert feat.shape == (R, 32 * 28 * 28) and torch.equal(feat.detach().reshape(rec['conv3_out'].shape), rec['conv3_out'])
    assert torch.equal(rec['conv3_in'], rec['conv2_out'])
    cot = torch.from_numpy(fc.tensor(tuple(feat.shape), 22))
    feat.backward(cot)
    out = dict(on=np.array([on], np.float32), a1=rec['conv2_in'].numpy(), cotangent=cot.numpy())
    go = {'conv3': cot.numpy().reshape(R, 32, 28, 28), 'conv2': grads['conv3_grad_input'].numpy()}
    for layer, conv in (('conv2', actor.conv2), ('conv3', actor.conv3)):
        out.update({layer + '_weight': conv.weight.detach().numpy(), layer + '_bias': conv.bias.detach().numpy(),
                    layer + '_out': rec[layer + '_out'].numpy(), layer + '_grad_input': grads[layer + '_grad_input'].numpy(),
                    layer + '_weight_grad': conv.weight.grad.numpy(), layer + '_bias_grad': conv.bias.grad.numpy()})
    assert all(v.dtype == np.float32 for v in out.values())
    # every recorded output against fp64 on the recorded inputs
    for layer, xin in (('conv2', out['a1']), ('conv3', out['conv2_out'])):
        w, b, o = out[layer + '_weight'], out[layer + '_bias'], out[layer + '_out']
        co, ci, k, _ = w.shape
        s = 2 if layer == 'conv2' else 1
        ref, mag = fc.forward_fp64(xin, w, b, s)
        within(layer + '_out', o, np.maximum(ref, 0.0), mag, ci * k * k + 1)
        g = fc.masked(o, go[layer], True)
        assert 0.05 < float((o > 0).mean()) < 0.95 and (g != 0).any()
        ref, mag = fc.grad_x_fp64(g, w, s, xin.shape[2], xin.shape[3])
        within(layer + '_grad_input', out[layer + '_grad_input'], ref, mag, co * (-(-k // s)) ** 2)
        gw, mw, gb, mb = fc.grad_w_fp64(g, xin, k, s)
        pixels = R * o.shape[2] * o.shape[3]
        within(layer + '_weight_grad', out[layer + '_weight_grad'], gw, mw, pixels)
        within(layer + '_bias_grad', out[layer + '_bias_grad'], gb, mb, pixels)
    assert reference.save(name, **out) <= LIMIT


def g22_trunk():
    sal = reference.load_sal()
    torch.set_num_threads(1)
    rng = np.random.default_rng(22)
    for name, on in FILES:
        blocks = rng.random((1, 1, 32, 32)) < rng.uniform(0.3, 0.7, (1, 1, 1, 1))
        record(sal, name, on, blocks)

