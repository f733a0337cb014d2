"""Generates tests/golden/g23_dense.npz from the reference's own Actor (src/SAL.py:390-411) on the CPU, seeded, one thread: what fc1
computes, forward and backward, on the two feature rows the trunk's recordings hold (g22_trunk.npz, the row fed as raw 0 / 255
floats, and g22_trunk_unit.npz, the row fed / 255: `conv3_out`, flattened), as one batch of 2.  The Actor is built under
torch.manual_seed(22), the seed of g22, so its trunk is g22's; the generator asserts that.  Recorded: fc1's pre-activation [2, 512],
a seeded fp32 cotangent on relu(.), fc1's grad_input [2, 25088], bias.grad, bias, and weight.grad and weight on COLS, a fixed set
of 128 columns: the 51 MB weight itself is not committed -- tests/test_dense_cpu.py rebuilds it from the seed, by constructing the
Actor's layers in their order, and checks conv2, conv3 and these columns before it uses it.  The fixture holds data only.
The generator asserts, per recorded array v, |v - fp64| <= gamma(T) * mag: fp64 and mag = sum |terms| from dense_cases' fp64 sums
on the recorded inputs, T the number of terms of the sum, bias included.  Run through make_golden.py.
"""
import numpy as np
import torch

import reference
import dense_cases as dc
import featconv_cases as fc
from reference import within

LIMIT = 1 << 20
SEED = 22
COLS = np.arange(128) * 197         # 0 .. 25019


def g23_dense():
    sal = reference.load_sal()
    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    actor = sal.Actor(action_dim=16)
    rows = [np.load(reference.fixture(name)) for name in fc.GOLDEN]
    for g in rows:
        assert np.array_equal(g['conv2_weight'], actor.conv2.weight.detach().numpy()) and np.array_equal(g['conv3_weight'], actor.conv3.weight.detach().numpy())
    feat = np.stack([g['conv3_out'].reshape(-1) for g in rows]).astype(np.float32)
    x = torch.from_numpy(feat).requires_grad_(True)
    pre = actor.fc1(x)
    cot = torch.from_numpy(fc.tensor(tuple(pre.shape), 23))
    torch.relu(pre).backward(cot)
    w, b = actor.fc1.weight.detach().numpy(), actor.fc1.bias.detach().numpy()
    out = dict(pre=pre.detach().numpy(), cotangent=cot.numpy(), grad_input=x.grad.numpy(), bias=b, bias_grad=actor.fc1.bias.grad.numpy(),
               cols=COLS.astype(np.int64), weight_cols=np.ascontiguousarray(w[:, COLS]),
               weight_grad_cols=np.ascontiguousarray(actor.fc1.weight.grad.numpy()[:, COLS]))
    assert all(v.dtype == np.float32 for k, v in out.items() if k != 'cols')
    n, K = feat.shape
    ref, mag = dc.forward_fp64(feat, w, b)
    within('pre', out['pre'], ref, mag, K + 1)
    g = dc.masked(out['pre'], out['cotangent'], True)
    assert 0.05 < float((out['pre'] > 0).mean()) < 0.95 and (g != 0).any()
    ref, mag = dc.grad_x_fp64(g, w)
    within('grad_input', out['grad_input'], ref, mag, w.shape[0])
    ref, mag = dc.grad_weight_fp64(g, feat[:, COLS])
    within('weight_grad', out['weight_grad_cols'], ref, mag, n)
    ref, mag = dc.grad_bias_fp64(g)
    within('bias_grad', out['bias_grad'], ref, mag, n)
    assert reference.save('g23_dense.npz', **out) <= LIMIT
