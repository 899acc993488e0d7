#!/usr/bin/env python
"""SHA-256 of everything the training batch-norm's eight entry points give on seeded inputs, through the public operators
(``bn_relu_mask_train``, ``bn_relu_nonzero_train``): forward, backward with and without ``fork``, batch and stored statistics, no mask /
plane mask / nonzero mask, both layouts -- at the test shapes, at (2, 8, 3, 2751) and at the training shapes [2,64,256,256] and
[2,128,128,128].  Then one training step each of ``TrainablePconvInputBlock``, ``TrainablePconvResBlock`` and ``TrainableResBlock`` with
fixed noise: the output and every gradient.  One line per tensor.  Run once per library (SLR_SFS_AMD_LIB=...) and compare the listings:
a change that reorders no sum leaves every line as it was.  A device is required.

    SLR_SFS_AMD_LIB=slr-sfs_amd/lib/other.so python tools/dev/bn_train_digest.py > other.txt
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = ((1, 8, 5, 7), (2, 24, 33, 20), (2, 64, 37, 51), (2, 130, 4, 4), (2, 8, 3, 2751), (2, 64, 256, 256), (2, 128, 128, 128))


def sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def bn_lines(S, shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H * 31 + W)
    r = lambda *s: torch.randn(*s, generator=g)                               # noqa: E731
    x = r(N, C, H, W) * (torch.rand(N, C, H, W, generator=g) > 0.15).float()  # (single zero elements: the nonzero mask's holes)
    mask = (torch.rand(N, 1, H, W, generator=g) > 0.25).float()
    gain, bias, ga, gskip = 1.0 + 0.3 * r(N, C), 0.3 * r(N, C), r(N, C, H, W), r(N, C, H, W)
    mean, var = 0.2 * r(C), 0.5 + torch.rand(C, generator=g)
    dev = lambda t: t.cuda()                                                  # noqa: E731
    # (a channel-blocked tensor is the same memory read as [N,C/8,H,W,8]: seeded values serve either layout)
    for b8 in (False, True) if C % 8 == 0 else (False,):
        for kind in ("none", "plane", "nonzero"):
            for stored in (False, True):
                for fork in (False, True):
                    xd, gd, bd = dev(x).requires_grad_(True), dev(gain).requires_grad_(True), dev(bias).requires_grad_(True)
                    st = dict(mean=dev(mean), var=dev(var)) if stored else {}
                    if kind == "nonzero":
                        out = S.bn_relu_nonzero_train(xd, gd, bd, b8=b8, fork=fork, **st)
                    else:
                        out = S.bn_relu_mask_train(xd, dev(mask) if kind == "plane" else None, gd, bd, b8=b8, fork=fork, **st)
                    names = ("a", "mean", "var") + (("msum",) if kind == "nonzero" else ())
                    grads = [dev(ga)] + [None] * (len(names) - 1) + ([dev(gskip)] if fork else [])
                    torch.autograd.backward([o for o, gr in zip(out, grads) if gr is not None], [gr for gr in grads if gr is not None])
                    tag = f"bn {'x'.join(map(str, shape))} {'b8' if b8 else 'nchw'} {kind} {'stored' if stored else 'batch'} {'fork' if fork else 'plain'}"
                    for n, t in zip(names, out):
                        yield f"{tag} {n} {sha(t)}"
                    for n, t in (("dx", xd.grad), ("dgain", gd.grad), ("dbias", bd.grad)):
                        yield f"{tag} {n} {sha(t)}"


def block_lines(S):
    N, cin, cout, H, W = 2, 16, 24, 12, 10
    for name, make in (("TrainablePconvInputBlock", lambda: S.TrainablePconvInputBlock(cin, cout)),
                       ("TrainablePconvResBlock", lambda: S.TrainablePconvResBlock(cin, cout, "Down")),
                       ("TrainableResBlock", lambda: S.TrainableResBlock(cin, cout, "Up"))):
        torch.manual_seed(7)
        blk = make()
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for p in blk.parameters():
                p.copy_(0.2 * torch.randn(*p.shape, generator=g))
        blk = blk.cuda().train()
        x = torch.randn(N, cin, H, W, generator=g) * (torch.rand(N, cin, H, W, generator=g) > 0.2).float()
        mask = (torch.rand(N, 1, H, W, generator=g) > 0.25).float()
        noise = (torch.randn(N, 20, generator=g).cuda(), torch.randn(N, 20, generator=g).cuda())
        x = x.cuda().requires_grad_(True)
        out = blk(x, mask.cuda(), noise=noise) if name == "TrainablePconvResBlock" else blk(x, noise=noise)
        y = out[0]
        y.backward(torch.randn(*y.shape, generator=g).cuda())
        yield f"{name} y {sha(y)}"
        if len(out) == 3:
            yield f"{name} update_mask {sha(out[1])}"
        yield f"{name} dx {sha(x.grad)}"
        for n, p in blk.named_parameters():
            yield f"{name} d {n} {sha(p.grad)}"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/dev/bn_train_digest.py: no ROCm device")
    import slr_sfs_amd as S
    S._lib.lib()
    print(f"# library {os.path.basename(os.environ.get('SLR_SFS_AMD_LIB', 'libslrsplat.so'))}")
    for shape in SHAPES:
        for line in bn_lines(S, shape):
            print(line)
    for line in block_lines(S):
        print(line)


if __name__ == "__main__":
    main()
