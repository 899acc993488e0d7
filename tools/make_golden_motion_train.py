#!/usr/bin/env python
"""tests/golden/motion_train_vs_reference.npz: one training forward + backward of the REFERENCE's own SPADEUnetMaskMotion
(models/unet_motion.py:111-173) built by its option parser with the flag set "spade" of tests/motion_fixture.py plus
--motion_losses 10.0_EndPointError (train_motion_EPE_MotionGAN.sh), its motion_predictor replaced by
SPADEUnet4MaskMotion(num_filters=8, channels_in=6) (the reference's class, 1/4 of the width), train() mode, float64, N = 2, 256 x 256, the
state dict defined by tests/motion_fixture.state_dict.  Build container only: needs the reference checkout (argv[1], default
/root/reference); without CUDA the reference's MotionLoss builds no loss modules (synthesis.py:35-36 returns None), so its own wrapper
classes (MotionEnePointErrorWrapper / MotionL1LossWrapper) are put into ``loss_function.losses`` directly.

Stored (data only, no weights, nothing of the reference's text): the batch seeds' outputs -- every loss entry, PredMotion and each
parameter's gradient at motion_fixture.digest_positions (<= 256 positions per tensor) with each tensor's max|.|, weight_u / weight_v after
the forward, and the sorted state-dict keys with shapes at num_filters = 32."""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_fixture as MF  # noqa: E402
import motion_train_fixture as TF  # noqa: E402


def _stubs():
    def stub(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules.setdefault(name, m)
        return sys.modules[name]
    stub("cupy", memoize=lambda for_each_device=False: (lambda f: f), cuda=types.SimpleNamespace(compile_with_cache=None))
    for n in ("cv2", "av", "lz4framed", "ipdb"):
        stub(n)
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")
    tv.models = stub("torchvision.models", vgg19=None)
    tv.utils = stub("torchvision.utils")


def main():
    sys.path.insert(0, REF)
    _stubs()
    torch.set_num_threads(16)
    from options.train_options import ArgumentParser
    from options.options import get_model
    from models.networks.architectures import SPADEUnet4MaskMotion
    from models.losses import synthesis as RS
    opt, _ = ArgumentParser().parse(MF.FLAGS["spade"] + " --motion_losses " + " ".join(TF.MOTION_LOSSES))
    model = get_model(opt)
    wrappers = {"EndPointError": RS.MotionEnePointErrorWrapper, "MotionL1": RS.MotionL1LossWrapper}
    model.loss_function.losses = torch.nn.ModuleList([wrappers[n]() for n in model.loss_function.loss_names])

    g = {}
    big = model.motion_predictor.state_dict()                    # num_filters = 32: keys and shapes
    keys = sorted(big)
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :big[k].dim()] = list(big[k].shape)
    g["keys_nf32"], g["shapes_nf32"] = np.array(keys), shapes

    model.motion_predictor = SPADEUnet4MaskMotion(num_filters=TF.NF, channels_in=6, channels_out=2, opt=opt)
    net = model.motion_predictor
    ref_sd = net.state_dict()
    sd = TF.state(list(ref_sd.keys()), [tuple(v.shape) for v in ref_sd.values()])
    net.load_state_dict({k: sd[k].to(ref_sd[k].dtype).reshape(ref_sd[k].shape) for k in ref_sd})
    model = model.double().train()
    batch = {k: (v.double() if torch.is_tensor(v) else [t.double() for t in v]) for k, v in TF.batch().items()}
    losses, pred = model(batch)
    losses["Total Loss"].backward()

    def digest(name, t):
        flat = t.detach().double().reshape(-1)
        g[name + "#samples"] = flat[TF.positions(name, flat.numel())].numpy()
        g[name + "#max_abs"] = np.float64(flat.abs().max())
    g["loss_keys"] = np.array(list(losses))
    for k, v in losses.items():
        g["loss/" + k] = np.float64(v.detach())
    digest("PredMotion", pred["PredMotion"])
    g["MovingMask#sum"] = np.float64(pred["MovingMask"].sum())
    for k, p in net.named_parameters():
        digest("grad/" + k, p.grad)
    after = net.state_dict()
    for k in after:
        if k.endswith("weight_u") or k.endswith("weight_v"):
            g["after/" + k] = after[k].detach().numpy().astype(np.float64)
    g["div_flow"] = np.float64(model.div_flow)
    out = os.path.join(ROOT, "tests", "golden", "motion_train_vs_reference.npz")
    np.savez_compressed(out, **g)
    print({k: float(v) for k, v in losses.items()}, "PredMotion max", float(pred["PredMotion"].abs().max()))
    print("wrote", out, os.path.getsize(out) // 1024, "kB")


if __name__ == "__main__":
    main()
