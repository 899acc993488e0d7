#!/usr/bin/env python
"""The fixtures of the tests that once read the reference tree directly (needs the reference checkout: python
tools/make_golden_reference_checks.py REFERENCE_DIR); the tests themselves read only tests/golden/.

  tests/golden/nets_vs_reference.npz  (tests/test_nets_vs_reference.py) -- outputs of the REFERENCE's own network classes
      (models/networks/utilities.py get_encoder / get_decoder / get_net_bg / get_alpha_encoder / get_alpha_decoder) built by its
      option parser with the 2-layer flag set (train_animating_scripts/*.sh), eval mode, bn_noise_misc forced like the test scripts
      do, on the state dicts and inputs tests/nets_fixture.py defines (VS_REFERENCE).  Stored: key / shape lists and outputs.
  tests/golden/reference_io.npz  -- (tests/test_io_formats.py) the bytes of a .flo file slr_sfs_amd.io.write_flo made and the array
      the reference's read_flo (utils/utils.py:252-261) returned for it; (tests/test_dropin_with_reference.py) the names the
      reference's model modules import from models.softsplat / models.projection.euler_integration_manipulator, and what
      AnimatingSoftmaxSplating holds and raises once install_into_reference() is in place.
Nothing of the reference's text is stored: names, shapes and arrays only."""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nets_fixture as NF  # noqa: E402

MODEL_FILES = ("models/animating_softmax_splating.py", "models/animating_softmax_splating_2layers_alpha_seperate.py")
OPS = ("models.softsplat", "models.projection.euler_integration_manipulator")


def _drop_reference_modules():
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.") or k.startswith("options")
              or k in ("cupy", "cv2", "av", "lz4framed") or k.startswith("torchvision")]:
        del sys.modules[k]


def _stub_libraries(with_cupy):
    def stub(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules.setdefault(name, m)
        return sys.modules[name]
    if with_cupy:
        stub("cupy", memoize=lambda for_each_device=False: (lambda f: f), cuda=types.SimpleNamespace(compile_with_cache=None))
    for n in ("cv2", "av", "lz4framed"):
        stub(n)
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")
    tv.models = stub("torchvision.models", vgg19=None)
    tv.utils = stub("torchvision.utils")


def imports_of_ops(ref):
    """'module|imported from|name,name' for every `from X import ...` of the operators in the model files (or `from models import softsplat`)."""
    out = []
    for rel in MODEL_FILES:
        mod = rel[:-3].replace("/", ".")
        for node in ast.walk(ast.parse(open(os.path.join(ref, rel)).read())):
            if isinstance(node, ast.ImportFrom) and node.module and not node.level:
                names = [a.name for a in node.names]
                if node.module in OPS or any(f"{node.module}.{n}" in OPS for n in names):
                    out.append(f"{mod}|{node.module}|{','.join(names)}")
    return out


def dropin(ref, g):
    import slr_sfs_amd as S
    _drop_reference_modules()
    _stub_libraries(with_cupy=False)
    ss, eim = S.install_into_reference()
    import models.animating_softmax_splating as A
    assert A.softsplat is ss and "cupy" not in sys.modules
    from options.train_options import ArgumentParser
    opt, _ = ArgumentParser().parse(
        "--model_type softmax_splating --refine_model_type resnet_256W8UpDown64_de_resnet_pconv2_nonorm "
        "--pconv pconv_pbn_woresbias --norm_G sync:spectral_batch --train_Z --losses 1.0_l1 --W 16")
    model = A.AnimatingSoftmaxSplating(opt).eval()
    assert type(model.softsplater).__module__ == ss.__name__ and type(model.euler_integration).__module__ == eim.__name__
    torch.Tensor.cuda_backup = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        batch = {"features": [(torch.zeros(1, 64, 16, 16), torch.zeros(1, 1, 16, 16))], "images": [torch.zeros(1, 3, 16, 16)],
                 "motions": [torch.zeros(1, 2, 16, 16)], "index": torch.tensor([[0, 1, 4]])}
        try:
            model.forward_flow(batch)
            raised = "nothing"
        except Exception as e:
            raised = f"{type(e).__name__}: {e}"
    finally:
        torch.Tensor.cuda = torch.Tensor.cuda_backup
        del torch.Tensor.cuda_backup
    g["dropin_imports"] = np.array(imports_of_ops(ref))
    g["dropin_softsplater"] = np.array([type(model.softsplater).__name__, model.softsplater.strType])
    g["dropin_euler_integration"] = np.array(type(model.euler_integration).__name__)
    g["dropin_forward_flow_raises"] = np.array(raised)
    _drop_reference_modules()
    print("dropin:", list(g["dropin_imports"]), list(g["dropin_softsplater"]), raised)


def flo(ref, g, tmp):
    from slr_sfs_amd import io
    import re
    src = open(os.path.join(ref, "utils", "utils.py")).read()
    ns = {"np": np}
    exec(re.search(r"def read_flo\(strFile\):.*?reshape\(\[ intHeight, intWidth, 2 \]\)", src, re.S).group(0), ns)
    fl = np.random.default_rng(1).standard_normal((4, 9, 2)).astype(np.float32)
    p = os.path.join(tmp, "b.flo")
    io.write_flo(p, fl)
    g["flo_bytes"] = np.frombuffer(open(p, "rb").read(), np.uint8)
    g["flo_reference_read"] = np.array(ns["read_flo"](p))


def nets_vs_reference(g):
    _drop_reference_modules()
    _stub_libraries(with_cupy=True)
    from models.networks import utilities as U
    from options.train_options import ArgumentParser
    flags = ("--model_type softmax_splating_2layers_alpha_seperate "
             "--refine_model_type resnet_256W8UpDown64_de_resnet_pconv2_nonorm --pconv pconv_pbn_woresbias "
             "--norm_G sync:spectral_batch --train_Z --losses 1.0_l1 --W 32 "
             "--bg_refine_model_type resnet_256W8UpDown64BG_nonorm "
             "--alpha_refine_model_type resnet_256W8UpDown64Layers_de_resnet_pconv2_nonorm "
             "--out_channel 65 --ngf 64 --train_bg --train_alpha --use_alpha0_as_blending_weight")
    opt, _ = ArgumentParser().parse(flags)
    opt.bn_noise_misc = True                       # forced by the test scripts (:127)
    for case, (getter, *_rest) in NF.VS_REFERENCE.items():
        net = getattr(U, getter)(opt).eval()
        ref_sd = net.state_dict()
        keys = list(ref_sd.keys())
        shapes = np.full((len(keys), 4), -1, np.int64)
        for i, k in enumerate(keys):
            shapes[i, :ref_sd[k].dim()] = list(ref_sd[k].shape)
        sd = NF.state_dict("vs_reference/" + case, keys, shapes)
        net.load_state_dict({k: sd[k].to(ref_sd[k].dtype).reshape(ref_sd[k].shape) for k in keys})
        with torch.no_grad():
            out = net(NF.vs_reference_input(case))
        out = out if isinstance(out, tuple) else (out,)
        g[f"{case}_keys"] = np.array(keys)
        g[f"{case}_shapes"] = shapes
        g[f"{case}_nout"] = np.int32(len(out))
        for i, o in enumerate(out):
            g[f"{case}_out{i}"] = o.numpy().astype(np.float32)
            print(case, i, tuple(o.shape), "max-abs", float(o.abs().max()), "finite", bool(torch.isfinite(o).all()))
    _drop_reference_modules()


def main():
    import tempfile
    ref = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ref)
    out = os.path.join(ROOT, "tests", "golden")
    io_g, nets_g = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        flo(ref, io_g, tmp)
    dropin(ref, io_g)
    nets_vs_reference(nets_g)
    for name, g in (("reference_io.npz", io_g), ("nets_vs_reference.npz", nets_g)):
        np.savez_compressed(os.path.join(out, name), **g)
        print("wrote", name, os.path.getsize(os.path.join(out, name)) // 1024, "kB")


if __name__ == "__main__":
    main()
