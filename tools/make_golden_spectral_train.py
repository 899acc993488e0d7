#!/usr/bin/env python
"""tests/golden/spectral_train_vs_reference.npz: the REFERENCE's own ResNet_Block_Pconv2 (models/layers/blocks.py:173-248, opt.pconv =
pconv_pbn_woresbias) and ResNet_Block (:47-87) under norm_G = 'sync:spectral_batch' -- torch.nn.utils.spectral_norm around every
convolution and noise linear -- in train() mode and float64, three small blocks each (no resampling, "Down", "Up"): TWO consecutive
forwards (each moves weight_u / weight_v by one power iteration), then the backward of the sum of both.  Stored: inputs, masks, the noise
the BN layers drew (forward hooks), weight_orig / u / v before and u / v after each forward, biases, outputs, the gradients to both
inputs and to every weight_orig and bias.  Inputs and parameters are float32 values (stored as float32), results float64 in the
packed form of decoder_train_f64.packed.  Data only; nothing of the reference's text.  The statistics' ``x.float()`` cast
(normalization.py:321) is the identity while the blocks run, as in make_golden_block_train.py.  tests/test_spectral_f64.py reads the
file only.  Needs the reference checkout next to the repository (build container only)."""
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
import decoder_train_f64 as D64  # noqa: E402

CASES = (("none", None, 2, 8, 16, 12, 12), ("down", "Down", 2, 8, 16, 12, 12), ("up", "Up", 2, 16, 8, 6, 6))


def layers_of(form, blk):
    """definition name -> the reference's normalised module (and the bias names)."""
    if form == "pconv":
        n1, n2, aa, ab, b = blk.bn_noise1, blk.bn_noise2, blk.conv_aa, blk.conv_ab, blk.conv_b
    else:
        n1, aa, n2, ab = blk.ch_a[0], blk.ch_a[2], blk.ch_a[3], blk.ch_a[5]
        b = blk.ch_b[0] if isinstance(blk.ch_b, torch.nn.Sequential) else None
    return {"w_aa": aa, "w_ab": ab, "w_b": b, "gain1": n1.gain, "bias1": n1.bias, "gain2": n2.gain, "bias2": n2.bias}, (n1, n2)


def main():
    sys.path.insert(0, REF)
    from models.layers.blocks import ResNet_Block, ResNet_Block_Pconv2
    torch.set_default_dtype(torch.float64)
    opt = argparse.Namespace(pconv="pconv_pbn_woresbias", norm_G="sync:spectral_batch", bn_noise_misc=False)
    out = {}
    for form, cls in (("pconv", ResNet_Block_Pconv2), ("res", ResNet_Block)):
        for name, kind, N, cin, cout, H, W in CASES:
            case = f"{form}_{name}"
            torch.manual_seed(200 + cin + 3 * cout + (7 if form == "res" else 0))
            blk = cls(cin, cout, opt, downsample=kind).train()
            layers, noises = layers_of(form, blk)
            layers = {k: m for k, m in layers.items() if m is not None}
            f32 = lambda t: t.float().double()                                   # noqa: E731
            with torch.no_grad():
                for prm in blk.parameters():
                    prm.copy_(f32(prm))
                for k, m in layers.items():
                    if k[:4] in ("gain", "bias"):        # noise weights large enough that gains and biases differ per sample
                        m.weight_orig.copy_(f32(torch.randn_like(m.weight_orig) * 0.2))
                    elif m.bias is not None:
                        m.bias.copy_(f32(torch.randn_like(m.bias) * 0.3))
            rec = {"form": np.array(form), "kind": np.array(kind or "")}
            for k, m in layers.items():
                rec[f"p/{k}"], rec[f"u0/{k}"], rec[f"v0/{k}"] = m.weight_orig.detach().float(), m.weight_u.clone(), m.weight_v.clone()
                if k.startswith("w_") and m.bias is not None:
                    rec[f"p/b_{k[2:]}"] = m.bias.detach().float()
            seen = {}
            hooks = [n.gain.register_forward_hook(lambda m, a, o, i=i: seen.update({f"noise{i}": a[0].detach().clone()}))
                     for i, n in ((1, noises[0]), (2, noises[1]))]
            xs, ys, gys = [], [], []
            for f in range(2):
                mask = C64.holed_mask(N, H, W, seed=cin + H + 5 * f).double()
                mu, sd = 3.0 * (2 * torch.rand(cin) - 1), 0.5 + 1.5 * torch.rand(cin)
                x = torch.randn(N, cin, H, W) * sd[None, :, None, None] + mu[None, :, None, None]
                if form == "pconv":
                    x = x * mask + 1e-3 * torch.randn(N, cin, H, W) * (1 - mask)
                x = f32(x).requires_grad_(True)
                with mock.patch.object(torch.Tensor, "float", lambda self: self):
                    if form == "pconv":
                        y, um = blk(x, mask.expand(N, cin, H, W).contiguous())
                        assert (um == um[:, :1]).all()
                        rec[f"{f}/mask"], rec[f"{f}/um"] = mask.float(), um[:, :1].detach().float()
                    else:
                        y = blk(x)
                gy = f32(torch.randn_like(y) * (1.0 + torch.arange(y.shape[3]) / y.shape[3]))
                rec[f"{f}/x"], rec[f"{f}/y"], rec[f"{f}/gy"] = x.detach().float(), y.detach().clone(), gy.float()
                rec[f"{f}/noise1"], rec[f"{f}/noise2"] = seen["noise1"], seen["noise2"]
                for k, m in layers.items():
                    rec[f"{f}/u/{k}"], rec[f"{f}/v/{k}"] = m.weight_u.clone(), m.weight_v.clone()
                xs.append(x)
                ys.append(y)
                gys.append(gy)
            for h in hooks:
                h.remove()
            params = {k: m.weight_orig for k, m in layers.items()}
            params.update({f"b_{k[2:]}": m.bias for k, m in layers.items() if k.startswith("w_") and m.bias is not None})
            loss = sum((y * g).sum() for y, g in zip(ys, gys))
            grads = torch.autograd.grad(loss, xs + list(params.values()))
            rec["0/dx"], rec["1/dx"] = grads[0], grads[1]
            for k, g in zip(params, grads[2:]):
                rec[f"d/{k}"] = g
            for k, v in rec.items():
                out.update(D64.packed(f"{case}/{k}", v.numpy()) if torch.is_tensor(v) else {f"{case}/{k}": v})
            print(case, kind, tuple(ys[0].shape), "max|y|", float(ys[0].detach().abs().max()), sorted(params))
    path = os.path.join(ROOT, "tests", "golden", "spectral_train_vs_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    main()
