"""Plain torch definition of the reference's generator loss (models/losses/synthesis.py:61-185 on the VGG19 of
models/networks/architectures.py:82-115): the yardstick of tests/test_losses_f64.py and tests/test_gpu_losses.py.  Every function takes a
``dtype`` (float64: the yardstick; float32: what fp32 costs the same definition, which sizes the GPU tests' bounds) and runs on the CPU.

The gradient of the perceptual loss is DISCONTINUOUS in the features: every ReLU gate [a > 0], every sign(relu(a) - relu(b)) and every
pooling route (which of a window's four elements holds the maximum) is a discrete decision, and an element whose margin is below fp32
rounding may decide differently in fp32 -- after which the gradient differs by far more than rounding over the element's whole
receptive field.  ``gradient_from_decisions`` therefore takes the decisions as ARGUMENTS: with them fixed the gradient is linear in the
seeds, and a float32 implementation can be held to float64 evaluated at the implementation's own decisions.  Test infrastructure only."""
import math

import torch
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)                  # torchvision vgg19().features indices of the convolutions
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
POOLS = (2, 4, 8, 12)                                                     # convolutions with ReLU + MaxPool2d(2, 2) in front
SLICE_ENDS = (0, 2, 4, 8, 12)                                             # relu1_1 ... relu5_1 (architectures.py:93-102)
WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)                     # synthesis.py:173


def _wb(sd, k, dtype):
    return sd[f"features.{CONVS[k]}.weight"].to(dtype), sd[f"features.{CONVS[k]}.bias"].to(dtype)


def activations(x, sd, dtype=torch.float64):
    """The 13 raw (pre-ReLU) convolution outputs of the VGG19 for x [B,3,H,W], NCHW, in ``dtype``."""
    acts, h = [], x.to(dtype)
    for k in range(13):
        if k:
            h = torch.relu(h)
        if k in POOLS:
            h = F.max_pool2d(h, 2, 2)
        w, b = _wb(sd, k, dtype)
        h = F.conv2d(h, w, b, padding=1)
        acts.append(h)
    return acts


def distances(acts_pred, acts_gt):
    """The five mean |relu(a_s(pred)) - relu(a_s(gt))| from the 13 (or the five slice-end) activations of each image."""
    pick = (lambda a: [a[k] for k in SLICE_ENDS]) if len(acts_pred) == 13 else (lambda a: a)      # noqa: E731
    return [(torch.relu(a) - torch.relu(b)).abs().mean() for a, b in zip(pick(acts_pred), pick(acts_gt))]


def perceptual(pred, gt, sd, dtype=torch.float64):
    """(loss, distances, activations of pred): PerceptualLoss.forward, differentiable in ``pred`` by autograd."""
    ap, ag = activations(pred, sd, dtype), activations(gt, sd, dtype)
    d = distances(ap, ag)
    loss = 0
    for s in range(5):
        loss = loss + WEIGHTS[s] * d[s]
    return loss, d, ap


def perceptual_gradient(pred, gt, sd, dtype=torch.float64, scale=1.0):
    """d(scale * loss) / d pred by autograd, with the value, the distances and the (detached) activations of pred and gt."""
    p = pred.detach().to(dtype).requires_grad_(True)
    ap, ag = activations(p, sd, dtype), activations(gt, sd, dtype)
    d = distances(ap, ag)
    loss = 0
    for s in range(5):
        loss = loss + WEIGHTS[s] * d[s]
    (scale * loss).backward()
    return p.grad, loss.detach(), [v.detach() for v in d], [a.detach() for a in ap], [a.detach() for a in ag]


# ---------------------------------------------------------------- the discrete decisions

def _windows(a):
    """[N,C,H,W] -> [N,C,H//2,W//2,4]: each complete 2x2 window's elements in row-major order (floor mode)."""
    OH, OW = a.shape[2] // 2, a.shape[3] // 2
    return torch.stack([a[:, :, dy:2 * OH:2, dx:2 * OW:2] for dy in (0, 1) for dx in (0, 1)], -1)


def decisions(acts_pred, ends_gt):
    """(gates, signs, routes) of 13 raw activations of the prediction and the five slice-end activations of the ground truth:
    13 boolean [a > 0]; 5 sign(relu(a) - relu(b)) in {-1, 0, 1}; 4 route indices (0 .. 3, row-major; the FIRST maximum, torch's choice)
    of the windows of the activations in front of the pools."""
    gates = [a > 0 for a in acts_pred]
    signs = [torch.sign(torch.relu(acts_pred[k]) - torch.relu(b)) for k, b in zip(SLICE_ENDS, ends_gt)]
    routes = [_windows(acts_pred[k - 1]).argmax(-1) for k in POOLS]
    return gates, signs, routes


def margins(acts_pred, ends_gt):
    """The distance of every decision from flipping, same structure as ``decisions``: |a| for gates, |relu(a) - relu(b)| for signs, the
    gap between a window's two largest values for routes.  A sign acts on the gradient only through its element's open gate
    (gate * sign): where a <= 0 -- where relu(a) - relu(b) is 0 for every b <= 0, a third of all elements -- nothing depends on the
    sign unless the gate opens, so the margin there is the gate's, |a| (``sign_matters`` is the mask a > 0)."""
    gates = [a.abs() for a in acts_pred]
    signs = [torch.where(acts_pred[k] > 0, (torch.relu(acts_pred[k]) - torch.relu(b)).abs(), acts_pred[k].abs())
             for k, b in zip(SLICE_ENDS, ends_gt)]
    routes = []
    for k in POOLS:
        top = _windows(acts_pred[k - 1]).topk(2, -1).values
        routes.append(top[..., 0] - top[..., 1])
    return gates, signs, routes


def sign_matters(acts_pred):
    """Where a slice's sign reaches the gradient: the elements whose gate is open."""
    return [acts_pred[k] > 0 for k in SLICE_ENDS]


def gradient_from_decisions(sd, gates, signs, routes, scale=1.0, dtype=torch.float64):
    """d(scale * loss) / d pred with every discrete decision given: LINEAR in the seeds.  With float64's own decisions it is float64
    autograd's gradient (tests/test_losses_f64.py)."""
    g = None
    for k in range(12, -1, -1):
        gate = gates[k].to(dtype)
        if k in SLICE_ENDS:
            s = SLICE_ENDS.index(k)
            seed = signs[s].to(dtype) * (WEIGHTS[s] / gate.numel() * scale)
            ga = gate * (seed if g is None else g + seed)
        elif k + 1 in POOLS:
            r = routes[POOLS.index(k + 1)]
            OH, OW = r.shape[2], r.shape[3]
            up = torch.zeros(gate.shape, dtype=dtype)
            for q in range(4):
                up[:, :, q // 2:2 * OH:2, q % 2:2 * OW:2] = g * (r == q).to(dtype)
            ga = gate * up
        else:
            ga = gate * g
        g = F.conv_transpose2d(ga, sd[f"features.{CONVS[k]}.weight"].to(dtype), padding=1)
    return g


# ---------------------------------------------------------------- the other terms and SynthesisLoss

def l1(pred, gt, dtype=torch.float64):
    return (pred.to(dtype) - gt.to(dtype)).abs().mean()


def psnr(pred, gt, dtype=torch.float64):
    """synthesis.py:113-122."""
    p, g = pred.to(dtype), gt.to(dtype)
    mse_err = (p - g).pow(2).sum(dim=1).view(p.shape[0], -1).mean(dim=1)
    return (10 * (1 / mse_err).log10()).mean()


def ssim(pred, gt, dtype=torch.float64, window_size=11):
    """models/losses/ssim.py:ssim (size_average): the window is built in float32 as there (gaussian -> mm -> .float()), then cast."""
    p, g = pred.to(dtype), gt.to(dtype)
    C, R = p.shape[1], window_size // 2
    g1 = torch.tensor([math.exp(-((x - window_size // 2) ** 2) / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=torch.float32)
    g1 = (g1 / g1.sum()).unsqueeze(1)
    w = g1.mm(g1.t()).float().unsqueeze(0).unsqueeze(0).expand(C, 1, window_size, window_size).contiguous().to(dtype)
    conv = lambda t: F.conv2d(t, w, padding=R, groups=C)                      # noqa: E731
    mu1, mu2 = conv(p), conv(g)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(p * p) - mu1_sq, conv(g * g) - mu2_sq, conv(p * g) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def synthesis_loss(pred, gt, sd, losses=("1.0_l1", "10.0_content"), dtype=torch.float64, subname=""):
    """SynthesisLoss.forward (synthesis.py:93-109): the dict, plus the five distances under "distances" when there is a content term.
    Differentiable in ``pred`` by autograd."""
    out, total, dists = {}, None, None
    for i, item in enumerate(losses):
        lam, name = item.split("_")
        if name == "l1":
            v = l1(pred, gt, dtype)
            out["L1" + subname] = v
        elif name == "content":
            v, dists, _ = perceptual(pred, gt, sd, dtype)
            out["Perceptual" + subname] = v
        else:
            raise ValueError(name)
        total = v if total is None else total + v * float(lam)               # (the first one's lambda is ignored, :105)
    out["Total Loss"] = total
    with torch.no_grad():
        out["psnr" + subname] = psnr(pred, gt, dtype)
        out["ssim" + subname] = ssim(pred, gt, dtype)
    if dists is not None:
        out["distances"] = torch.stack(dists).detach()
    return out
