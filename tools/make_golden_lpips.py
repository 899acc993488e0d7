#!/usr/bin/env python
"""tests/golden/lpips_trunk_vs_reference.npz: outputs of the REFERENCE's own PNet("alex", pnet_rand=True, use_gpu=False)
(models/networks/pretrained_networks.py:34-93 on its alexnet, :154-196) in float64 on the CPU, on the seeded image pair of
tests/lpips_fixture.py: `val`, the five per-layer scores, and the sum of each of the five slices of the first image.  Its
torchvision.models.alexnet is stubbed to return the seeded layer list of lpips_fixture.alexnet_features().  That pins the slices, the
pools and the scaling constants of the LPIPS trunk to the reference; the linear heads of LPIPS belong to the lpips package, which the
reference checkout does not contain: they have no counterpart here.  Outputs only: no weights, nothing of the reference's text.
Needs the reference checkout (path: argv[1], default /root/reference)."""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_fixture as LF  # noqa: E402


def _stubs():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.alexnet = lambda pretrained=False, **kw: types.SimpleNamespace(features=LF.alexnet_features(dtype=torch.float64))
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tv.models)


def main():
    sys.path.insert(0, REF)
    _stubs()
    torch.set_num_threads(16)
    from models.networks.pretrained_networks import PNet
    pnet = PNet("alex", pnet_rand=True, use_gpu=False).eval()
    x0, x1 = LF.image_pair(*LF.GOLDEN_SHAPE)
    x0, x1 = x0.double(), x1.double()
    with torch.no_grad():
        val, per = pnet(x0, x1, retPerLayer=True)
        sc = (x0 - pnet.shift.expand_as(x0)) / pnet.scale.expand_as(x0)
        sums = [float(o.sum()) for o in pnet.net.forward(sc)]
    assert val.dtype == torch.float64
    g = {"val": val.numpy(), "layers": torch.stack(per).numpy(), "slice_sums": np.array(sums)}
    for k, v in g.items():
        print(k, v)
    path = os.path.join(ROOT, "tests", "golden", "lpips_trunk_vs_reference.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
