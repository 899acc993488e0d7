#!/usr/bin/env python
"""tests/golden/motion_vs_reference.npz and tests/golden/motion_768.npz: outputs of the REFERENCE's own motion predictors
(models/unet_motion.py:30-191 UnetMotion / SPADEUnetMaskMotion with models/networks/architectures.py:382-493, 602-743) built by its
option parser with the flag sets of tests/motion_fixture.py (the shipped motion training script: norm_G sync:spectral_batch,
motion_norm_G sync:spectral_instance, mask + hint input; and a plain unet_motion set), eval mode, their state dicts replaced by the
deterministic ones of tests/motion_fixture.py.  Stored: key / shape lists and PredMotion of forward_flow at 256 x 256 in full, digests of
one 256 x 512 case; at 768 x 768 digests (4096 sampled positions + plane sums) of the SPADE net run on the CPU in fp32 and in
float64.  No weights, nothing of the reference's text.  Needs the reference checkout (path: argv[1], default /root/reference)."""
import copy
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_fixture as MF  # noqa: E402


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


def build(flagset):
    from options.train_options import ArgumentParser
    from options.options import get_model
    opt, _ = ArgumentParser().parse(MF.FLAGS[flagset])
    model = get_model(opt).eval()
    return model, opt


def main():
    sys.path.insert(0, REF)
    _stubs()
    torch.set_num_threads(16)
    g, big = {}, {}
    models = {}
    for flagset in MF.FLAGS:
        model, opt = build(flagset)
        net = model.motion_predictor
        ref_sd = net.state_dict()
        keys = list(ref_sd.keys())
        shapes = np.full((len(keys), 4), -1, np.int64)
        for i, k in enumerate(keys):
            shapes[i, :ref_sd[k].dim()] = list(ref_sd[k].shape)
        sd = MF.state_dict(flagset, keys, shapes)
        net.load_state_dict({k: sd[k].to(ref_sd[k].dtype).reshape(ref_sd[k].shape) for k in keys})
        g[f"{flagset}_keys"] = np.array(keys)
        g[f"{flagset}_shapes"] = shapes
        g[f"{flagset}_div_flow"] = np.float32(model.div_flow)
        models[flagset] = model
        print(flagset, type(model).__name__, type(net).__name__, len(keys), "keys, div_flow", model.div_flow)

    def predict(model, x):
        with torch.no_grad():
            if x.shape[1] == 3:
                return model.forward_flow(x)["PredMotion"]
            return model.forward_flow(x[:, :3], x[:, 3:4], x[:, 4:6])["PredMotion"]

    for case, (flagset, shape) in MF.CASES.items():
        out = predict(models[flagset], MF.motion_input(case))
        if shape[2] == shape[3]:
            g[f"{case}_out"] = out.numpy().astype(np.float32)
        else:                                        # (within the size limit of a committed file: digests of the rectangular case)
            flat = out.double()[0].reshape(-1)
            g[f"{case}_samples"] = flat[MF.digest_positions(case, flat.numel())].numpy()
            g[f"{case}_plane_sums"] = flat.reshape(2, -1).sum(1).numpy()
            g[f"{case}_max_abs"] = np.float64(flat.abs().max())
        print(case, tuple(out.shape), "max-abs", float(out.abs().max()))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "motion_vs_reference.npz"), **g)

    x = MF.motion_input("spade_768", (1, 6, 768, 768))
    pos = MF.digest_positions("spade_768", 2 * 768 * 768)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        model = copy.deepcopy(models["spade"]).to(dt)
        out = predict(model, x.to(dt)).double()[0].reshape(-1)
        big[f"{tag}_samples"] = out[pos].numpy()
        big[f"{tag}_plane_sums"] = out.reshape(2, -1).sum(1).numpy()
        big[f"{tag}_max_abs"] = np.float64(out.abs().max())
        print("768", tag, "max-abs", float(out.abs().max()))
    big["positions_tag"] = np.array("spade_768")
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "motion_768.npz"), **big)
    for f in ("motion_vs_reference.npz", "motion_768.npz"):
        print("wrote", f, os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) // 1024, "kB")


if __name__ == "__main__":
    main()
