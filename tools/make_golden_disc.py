#!/usr/bin/env python
"""tests/golden/disc_vs_reference.npz: both steps of the reference's own adversarial loss (models/losses/gan_loss.py DiscriminatorLoss with
--discriminator_losses pix2pixHD --gan_mode hinge --norm_D spectralinstance) in float64 on the CPU, for tests/test_disc_f64.py.

Per case (ndf = 8, two images per half, 16 x 16 and 21 x 19): the parameters, u, v and the images are seeded by name
(disc_f64.fixture_param) and not stored.  Stored: the loss dictionaries of run_generator_one_step and then run_discriminator_one_step (two
forwards in train() mode, as the trainer's step), the gradients of their totals to the fake image and to every parameter, u / v after the
first and after the second forward, and the state-dict key list.  float64 results are stored as a float32 part + an int16 correction
(disc_f64.packed); gradients of more than 4096 elements are stored in full for the generator step of the first case and as every 7th
element (key suffix "@7") elsewhere, which keeps the file under 1 MB.  compute_generator_loss accumulates GAN_Feat into self.FloatTensor(1), float32 whatever the model's dtype: the script
sets netD.FloatTensor = torch.DoubleTensor.  Only data is stored, nothing of the reference's text.  Needs the reference checkout (build
container only)."""
import argparse
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import disc_f64 as D64  # noqa: E402

CASES = {"d16": (2, 16, 16), "d21": (2, 21, 19)}
NDF = 8


def main():
    sys.path.insert(0, REF)
    from models.losses.gan_loss import DiscriminatorLoss
    torch.set_default_dtype(torch.float64)
    opt = argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=NDF, output_nc=3,
                             no_ganFeat_loss=False, lambda_feat=10.0, isTrain=True, lr=1e-4, niter=1, niter_decay=1)
    out = {}
    for case, (N, H, W) in CASES.items():
        loss = DiscriminatorLoss(opt).double().train()
        loss.netD.FloatTensor = torch.DoubleTensor
        net = loss.netD.netD
        sd = net.state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == D64.param_shapes(NDF)
        net.load_state_dict({k: D64.fixture_param(case, k, tuple(v.shape)).double() for k, v in sd.items()})
        out[f"{case}/keys"] = np.array(list(loss.state_dict().keys()))
        fake = D64.fixture_param(case, "fake", (N, 3, H, W)).double().requires_grad_(True)
        real = D64.fixture_param(case, "real", (N, 3, H, W)).double()
        params = dict(net.named_parameters())
        rec = {}
        for step, run in (("g", loss.run_generator_one_step), ("d", loss.run_discriminator_one_step)):
            losses = run(fake, real)
            for k, v in losses.items():
                rec[f"{step}/loss/{k}"] = v.detach().reshape(-1)
                assert v.dtype == torch.float64
            wrt = ([fake] if step == "g" else []) + list(params.values())
            grads = torch.autograd.grad(losses["Total Loss"], wrt)
            names = (["fake"] if step == "g" else []) + list(params.keys())
            for k, g in zip(names, grads):               # (the file stays under 1 MB: large gradients in full once, else every 7th element)
                full = g.numel() <= 4096 or (case, step) == ("d16", "g")
                rec[f"{step}/grad/{k}" + ("" if full else "@7")] = g if full else g.reshape(-1)[::7]
            for k, b in net.named_buffers():
                rec[f"{step}/state/{k}"] = b.detach().clone()
        loss.eval()
        before = {k: b.clone() for k, b in net.named_buffers()}
        with torch.no_grad():
            loss.run_discriminator_one_step(fake, real)
        assert all(torch.equal(before[k], b) for k, b in net.named_buffers())
        for k, v in rec.items():
            out.update(D64.packed(f"{case}/{k}", v.numpy()))
        print(case, {k: float(v.sum()) for k, v in rec.items() if "/loss/" in k})
    path = os.path.join(ROOT, "tests", "golden", "disc_vs_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    main()
