#!/usr/bin/env python
"""tests/golden/losses_vs_reference.npz: outputs of the REFERENCE's own SynthesisLoss (models/losses/synthesis.py:61-109, --losses
1.0_l1 10.0_content) on the seeded images of tests/losses_fixture.py, in float64 on the CPU: every value of the returned dict, the five
per-slice L1 distances of its VGG19 (models/networks/architectures.py:82-115) and the gradient of "Total Loss" to the prediction.  Its
torchvision.models.vgg19 is stubbed to return the seeded layer list of losses_fixture.vgg19_features(), and its `.cuda()` calls are
neutralised (get_loss_from_name returns a loss only where torch.cuda.is_available()).  No weights, nothing of the reference's text.
Needs the reference checkout (path: argv[1], default /root/reference)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import losses_fixture as LF  # noqa: E402


def _stubs():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg19 = lambda pretrained=False, **kw: types.SimpleNamespace(features=LF.vgg19_features(dtype=torch.float64))
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tv.models)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    for name in ("cv2", "av", "lz4framed"):
        sys.modules.setdefault(name, types.ModuleType(name))
    torch.cuda.is_available = lambda: True              # get_loss_from_name: `if torch.cuda.is_available(): return loss.cuda()`
    nn.Module.cuda = lambda self, device=None: self


def main():
    sys.path.insert(0, REF)
    _stubs()
    torch.set_num_threads(16)
    from models.losses.synthesis import SynthesisLoss
    loss_fn = SynthesisLoss(types.SimpleNamespace(losses=list(LF.LOSSES)))
    pred, gt = LF.image_pair(*LF.GOLDEN_SHAPE[:1], *LF.GOLDEN_SHAPE[2:])
    pred = pred.double().requires_grad_(True)
    gt = gt.double()
    out = loss_fn(pred, gt)
    out["Total Loss"].backward()
    g = {k.replace(" ", "_"): v.detach().numpy() for k, v in out.items()}
    g["keys"] = np.array(sorted(out.keys()))
    vgg = loss_fn.losses[1].model
    with torch.no_grad():
        g["distances"] = np.array([float(nn.L1Loss()(a, b)) for a, b in zip(vgg(pred), vgg(gt))])
    g["grad"] = pred.grad.numpy()
    for k, v in g.items():
        print(k, v if np.size(v) < 8 else (v.shape, float(np.abs(v).max())))
    path = os.path.join(ROOT, "tests", "golden", "losses_vs_reference.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    main()
