#!/usr/bin/env python
"""tests/golden/block_train_vs_reference.npz: the REFERENCE's own ResNet_Block_Pconv2 (models/layers/blocks.py:173-248, opt.pconv =
pconv_pbn_woresbias, no spectral norm) in train() mode and float64 on three small blocks (no resampling, "Down", "Up"): inputs, weights,
the noise its BN layers drew and the gains / biases their linear layers made of it (forward hooks), outputs, the stored statistics after
the step, and the gradients to the input and to every parameter for a fixed output gradient.  Inputs and weights are float32 values (stored
as float32), results float64.  The reference's statistics cast their input with ``x.float()`` ("to float32 if necessary", written for
half precision: normalization.py:321), which would leave a float64 run with float32 sums; Tensor.float is the identity while the block
runs, so every operation of the reference is evaluated in float64.  Nothing of the reference's text is stored.  tests/test_block_train_f64.py reads the file only.
Needs the reference checkout next to the repository (build container only)."""
import argparse
import os
import sys
from unittest import mock

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_train_f64 as C64  # noqa: E402

CASES = (("none", None, 2, 16, 24, 12, 10), ("down", "Down", 2, 8, 16, 12, 10), ("up", "Up", 2, 16, 8, 6, 5))


def main():
    sys.path.insert(0, REF)
    from models.layers.blocks import ResNet_Block_Pconv2
    torch.set_default_dtype(torch.float64)               # (the block draws its noise with torch.randn: float64 like its weights)
    opt = argparse.Namespace(pconv="pconv_pbn_woresbias", norm_G="batch", bn_noise_misc=False)
    out = {}
    for name, kind, N, cin, cout, H, W in CASES:
        torch.manual_seed(100 + cin + cout)
        blk = ResNet_Block_Pconv2(cin, cout, opt, downsample=kind).train()
        f32 = lambda t: t.float().double()                                   # noqa: E731
        with torch.no_grad():
            for prm in blk.parameters():
                prm.copy_(f32(prm))
            for bn in (blk.bn_noise1, blk.bn_noise2):    # noise weights large enough that gains and biases differ per sample
                bn.gain.weight.copy_(f32(torch.randn_like(bn.gain.weight) * 0.1))
                bn.bias.weight.copy_(f32(torch.randn_like(bn.bias.weight) * 0.2))
            blk.conv_aa.bias.copy_(f32(torch.randn(cout) * 0.3))
            blk.conv_ab.bias.copy_(f32(torch.randn(cout) * 0.3))
        mu, sd = 3.0 * (2 * torch.rand(cin) - 1), 0.5 + 1.5 * torch.rand(cin)
        mask = C64.holed_mask(N, H, W, seed=cin + H).double()
        x = torch.randn(N, cin, H, W) * sd[None, :, None, None] + mu[None, :, None, None]
        x = f32(x * mask + 1e-3 * torch.randn(N, cin, H, W) * (1 - mask)).requires_grad_(True)      # (as block_train_f64.holed)
        seen = {}
        hooks = []
        for i, bn in ((1, blk.bn_noise1), (2, blk.bn_noise2)):
            hooks.append(bn.gain.register_forward_hook(lambda m, a, o, i=i: seen.update({f"noise{i}": a[0].detach(), f"gain{i}": 1 + o.detach()})))
            hooks.append(bn.bias.register_forward_hook(lambda m, a, o, i=i: seen.update({f"bias{i}": o.detach()})))
        with mock.patch.object(torch.Tensor, "float", lambda self: self):
            y, um = blk(x, mask.expand(N, cin, H, W).contiguous())
        for h in hooks:
            h.remove()
        assert (um == um[:, :1]).all()
        g = f32(torch.randn_like(y) * (1.0 + torch.arange(y.shape[3]) / y.shape[3]))
        params = dict(blk.named_parameters())
        grads = torch.autograd.grad(y, [x] + list(params.values()), g)
        rec = dict(x=x.detach().float(), mask=mask.float(), g=g.float(), y=y.detach(), um=um[:, :1].float(), dx=grads[0])
        for (k, prm), gr in zip(params.items(), grads[1:]):
            rec["p_" + k] = prm.detach().float()
            rec["d_" + k] = gr
        for k, v in seen.items():
            rec[k] = v
        for i, bn in ((1, blk.bn_noise1), (2, blk.bn_noise2)):
            rec[f"stored_mean{i}"], rec[f"stored_var{i}"] = bn.pbn.stored_mean.clone(), bn.pbn.stored_var.clone()
        rec["dims"] = torch.tensor([N, cin, cout, H, W])
        for k, v in rec.items():
            out[f"{name}/{k}"] = v.numpy()
        print(name, kind, tuple(y.shape), "max|y|", float(y.detach().abs().max()), "holes in um", int((um == 0).sum()))
    path = os.path.join(ROOT, "tests", "golden", "block_train_vs_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    main()
