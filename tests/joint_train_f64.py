"""The joint model's forward (and, for the device tests, its gradients) written out: ``AnimatingSoftmaxSplating`` under ``--train_motion``
(models/animating_softmax_splating.py:189-193, :514-536, :748-766) composed from the definitions that are already pinned to the
reference -- tests/motion_train_f64.py (the motion model: ``model_step`` / ``net_backward``) and tests/train_step_f64.py (encoder twice,
Euler, blend, decoder, tanh; tests/loss_f64.py for the loss) -- plus the glue between them:

  * the motion model is called on {"images": [start], "motions", "hints"};
  * the flow is its PredMotion WITHOUT div_flow (times [W / motionW, W / motionH] = 1);
  * ``Total Loss += motion_loss["Total Loss"]`` in place, which with one entry in ``losses`` is also the tensor under "L1";
  * the named motion losses are copied in; PredMotion and the motion model's GTMotion join the pred_dict.

The Euler paths are discrete, so everything downstream of the flow may be started from a GIVEN flow (``flow=``: the fixture's stored
one, or the device's own): rounding decisions of the integration are then shared between the arithmetics that are compared.
MUTANTS of the glue: "div_flow" (pred * div_flow fed to the integration), "no_motion_loss" (the motion loss left out of Total Loss).
Test infrastructure only."""
import torch

import joint_train_fixture as JF
import loss_f64 as L64
import motion_train_f64 as M64
import train_step_f64 as T

MUTANTS = ("div_flow", "no_motion_loss")


def _inputs(g, batch, flow, dtype):
    return {"images": batch["images"], "motions": flow.to(dtype), "index": batch["index"], "noise": T.noise_lists(g)}


def forward(g, dtype=torch.float64, flow=None, mutants=(), batch=None, with_grads=False, motion_learns=True):
    """-> {"loss": {...}, "PredImg", "PredMotion", "GTMotion", "flow" (what the integration got), "motion_state" (after the forward)}
    and with ``with_grads`` also {"grads_G": reference key -> gradient of Total Loss, "grads_M": motion key -> gradient (the motion loss's
    own plus, through the flow, the synthesis loss's; ``motion_learns`` False: None), "flow_grad"}.

    ``flow``: start everything downstream of the motion model from this tensor [B,2,W,W] instead of from the definition's own PredMotion
    (the mutant "div_flow" multiplies whichever it is by div_flow)."""
    batch = JF.batch() if batch is None else batch
    opts = JF.options()
    P = {k: v.to(dtype) for k, v in JF.motion_state().items()}
    start, gt, hints = (t.to(dtype) for t in (batch["images"][0], batch["motions"], batch["hints"]))
    with torch.no_grad():
        m_loss, m_pred, _, P2 = M64.model_step(P, start, gt, hints, JF.MOTION_LOSSES, JF.DIV_FLOW, True, with_grads=False)
    pred_motion = m_pred["PredMotion"]
    used = (pred_motion if flow is None else flow.to(dtype)).detach().clone()
    if "div_flow" in mutants:
        used = used * JF.DIV_FLOW
    used.requires_grad_(with_grads)
    net = T.generator(JF.generator_fixture(), dtype)
    with torch.set_grad_enabled(with_grads):
        f = T.generator_forward(net, _inputs(g, batch, used, dtype), dtype, opts)
        loss = L64.synthesis_loss(f["PredImg"], f["middle"], None, tuple(JF.LOSSES), dtype)
    loss.pop("distances", None)
    old = loss["Total Loss"]
    if "no_motion_loss" not in mutants:
        new = old + m_loss["Total Loss"]
        for k in list(loss):                                 # the reference's `+=` is in place: "L1" is the same tensor
            if loss[k] is old:
                loss[k] = new
    for name in M64.parse_losses(JF.MOTION_LOSSES)[1]:
        loss[name] = m_loss[name]
    out = {"loss": {k: v.detach() for k, v in loss.items()}, "PredImg": f["PredImg"].detach(), "PredMotion": pred_motion, "GTMotion": gt,
           "flow": used.detach(), "motion_state": P2, "flow_f": f["flow_f"].detach(), "flow_p": f["flow_p"].detach()}
    if with_grads:
        old.backward()                                       # the synthesis part of Total Loss: generator leaves and the flow
        out["grads_G"] = {k: (torch.zeros_like(t) if t.grad is None else t.grad.detach().clone()) for k, t in net["leaves"].items()}
        out["flow_grad"] = used.grad.detach().clone()
    return out


def motion_gradients(dtype, flow_grad, batch=None):
    """The motion network's gradients of the joint Total Loss: ``net_backward`` on the motion loss's own gradient at PredMotion * div_flow
    plus ``flow_grad`` (d synthesis loss / d flow, arriving at PredMotion itself: no div_flow).  -> {motion key: gradient}."""
    batch = JF.batch() if batch is None else batch
    P = {k: v.to(dtype) for k, v in JF.motion_state().items()}
    start, gt, hints = (t.to(dtype) for t in (batch["images"][0], batch["motions"], batch["hints"]))
    with torch.no_grad():
        speed = (gt[:, 0:1] ** 2 + gt[:, 1:2] ** 2).sqrt()
        mask = 1.0 - (speed < speed.mean([1, 2, 3], True) * 0.1).to(dtype)
        pred, cache, P2 = M64.net_forward(P, torch.cat([start, mask, hints], 1), True)
        lam, names = M64.parse_losses(JF.MOTION_LOSSES)
        w_epe = sum(v for v, n in zip(lam, names) if n == "EndPointError")
        w_l1 = sum(v for v, n in zip(lam, names) if n == "MotionL1")
        g_pred = M64.motion_losses_grad(pred * JF.DIV_FLOW, gt, w_epe, w_l1) * JF.DIV_FLOW + flow_grad.to(dtype)
        return M64.net_backward(P2, cache, g_pred)


def rel(got, ref):
    """max|got - ref| / max|ref| (a scalar: its relative error)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
