#!/usr/bin/env python
"""tests/golden/decoder_train_vs_reference.npz: the REFERENCE's own generator networks in train() mode and float64, for
tests/test_decoder_train_f64.py (which reads the file only):
  (a) ResNet_Block_Pconv2(8, 16) and (16, 16) (models/layers/blocks.py:173-248) called with the [N,C,H,W] mask (x != 0).float();
  (b) ResNetDecoderPconv2.forward (models/networks/architectures.py:345-375) on a narrow architecture -- get_resnet_arch is patched to
      layers_dec = [8,16,24,24,16,16,16,8,3] with the real resampling pattern;
  (c) a narrow ResNetEncoder_with_Z (:155-197) and one ResNet_Block (blocks.py:47-87) of each resampling kind.
opt.pconv = pconv_pbn_woresbias, norm_G = batch (no spectral norm).  Recorded per case: the input, every parameter, the noise every BN
layer drew and the gains / biases its linear layers made of it (forward hooks), the output, the final mask, the stored statistics after
the step, and the gradients to the input and to every parameter for a fixed output gradient.  Inputs and parameters are float32 values;
the parameters are seeded by their names (decoder_train_f64.fixture_param) and not stored -- the test regenerates them.  Results are
float64, stored as a float32 and an int16 correction with a common scale (decoder_train_f64.packed: 6 bytes, within 1e-12 of the
largest element), so that the file stays under 1 MB.  Tensor.float is the identity on floating tensors while a net runs (the reference's statistics cast
with ``x.float()``, normalization.py:321, which would leave float32 sums in a float64 run); (x != 0).float() becomes float64.  Only data is
stored, nothing of the reference's text.  Needs the reference checkout next to the repository (build container only)."""
import argparse
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import block_train_f64 as B64  # noqa: E402
import decoder_train_f64 as D64  # noqa: E402

NARROW = dict(layers_enc=[3, 4, 4, 4, 4, 8, 8, 4, 4], downsample=[False] * 8, layers_dec=[8, 16, 24, 24, 16, 16, 16, 8, 3],
              upsample=[False, "Down", "Down", False, "Up", "Up", False, False])


def f32(t):
    return t.float().double()


def _float(self):
    return self if self.is_floating_point() else self.double()


def record(out, name, net, x, call):
    """Run ``call(net, x)`` -> (y, mask or None) in train() mode and store everything under ``name/``."""
    net.train()
    with torch.no_grad():
        for k, prm in net.named_parameters():            # float32 values, seeded by name: the test regenerates them
            prm.copy_(D64.fixture_param(name, k, tuple(prm.shape)).double())
    seen, hooks = {}, []
    for k, m in net.named_modules():
        if isinstance(getattr(m, "gain", None), torch.nn.Linear) and isinstance(getattr(m, "bias", None), torch.nn.Linear):
            hooks.append(m.gain.register_forward_hook(lambda mod, a, o, k=k: seen.update({f"noise/{k}": a[0].detach(), f"gain/{k}": 1 + o.detach()})))
            hooks.append(m.bias.register_forward_hook(lambda mod, a, o, k=k: seen.update({f"bias/{k}": o.detach()})))
    x = x.requires_grad_(True)
    with mock.patch.object(torch.Tensor, "float", _float):
        y, mask = call(net, x)
    for h in hooks:
        h.remove()
    g = f32(torch.randn_like(y) * (1.0 + torch.arange(y.shape[3]) / y.shape[3]))
    params = dict(net.named_parameters())
    grads = torch.autograd.grad(y, [x] + list(params.values()), g, allow_unused=True)
    rec = dict(x=x.detach().float(), g=g.float(), y=y.detach(), dx=grads[0])
    if mask is not None:
        assert (mask == mask[:, :1]).all()
        rec["um"] = mask[:, :1].float()
    for (k, prm), gr in zip(params.items(), grads[1:]):
        if gr is not None:                               # (ResNet_Block keeps a conv_b it does not use when its skip is the identity)
            rec["d/" + k] = gr
    for k, b in net.named_buffers():
        if k.endswith("stored_mean") or k.endswith("stored_var"):
            rec["s/" + k] = b.detach().clone()
    rec.update(seen)
    for k, v in rec.items():
        out.update(D64.packed(f"{name}/{k}", v.numpy()))
    print(name, tuple(y.shape), "max|y|", float(y.detach().abs().max()), len(rec), "tensors")


def main():
    sys.path.insert(0, REF)
    if "torchvision" not in sys.modules:                 # architectures.py imports it for its VGG19 only (as tools/make_golden_motion.py)
        tv = sys.modules["torchvision"] = types.ModuleType("torchvision")
        tv.models = sys.modules["torchvision.models"] = types.ModuleType("torchvision.models")
    from models.layers.blocks import ResNet_Block, ResNet_Block_Pconv2
    from models.networks import architectures
    torch.set_default_dtype(torch.float64)               # (the nets draw their noise with torch.randn: float64 like their weights)
    opt = argparse.Namespace(pconv="pconv_pbn_woresbias", norm_G="batch", bn_noise_misc=False, refine_model_type="resnet_256W8UpDown64", ngf=64)
    out = {}

    def holed(N, C, H, W, seed):
        return f32(B64.bn_inputs(N, C, H, W, seed)[0].double() * D64.keep_pattern(N, C, H, W, seed, zero_channel=False).double())

    for cin, cout in ((8, 16), (16, 16)):                # (a)
        torch.manual_seed(100 + cin + cout)
        record(out, f"pblock_{cin}_{cout}", ResNet_Block_Pconv2(cin, cout, opt), holed(2, cin, 12, 10, cin),
               lambda net, x: net(x, (x != 0).float()))
    with mock.patch.object(architectures, "get_resnet_arch", lambda *a, **k: dict(NARROW)):
        torch.manual_seed(200)                           # (b)
        record(out, "decoder", architectures.ResNetDecoderPconv2(opt, channels_in=8, channels_out=3), holed(2, 8, 8, 8, 2), lambda net, x: (net(x), None))
        torch.manual_seed(300)                           # (c)
        record(out, "encoder", architectures.ResNetEncoder_with_Z(opt, channels_in=3, channels_out=4), f32(torch.randn(2, 3, 8, 8)),
               lambda net, x: (torch.cat(net(x), 1), None))
    for kind, cin, cout in ((None, 8, 8), ("Down", 8, 16), ("Up", 16, 8)):          # (the first one's skip is the identity)
        torch.manual_seed(400 + cin + cout)
        H, W = 12, 10
        record(out, f"block_{kind}_{cin}_{cout}", ResNet_Block(cin, cout, opt, downsample=kind), f32(B64.bn_inputs(2, cin, H, W, cin)[0].double()),
               lambda net, x: (net(x), None))
    path = os.path.join(ROOT, "tests", "golden", "decoder_train_vs_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    main()
