"""The two-direction blend of the training step in plain torch -- TEST INFRASTRUCTURE ONLY (no tests here).

The definition `slr_sfs_amd.splat_blend` implements, written on tests/splat_f64.py::splat_sum (same position rule, same dropped-pixel
rule), in any dtype, differentiated by torch autograd:

    Zn_d = Z_d - max(Z_d over the whole batch tensor)      (subtract_max; models/animating_softmax_splating.py:601 / :646)
    Zn_d = clamp(Zn_d, lo, hi)                             (clamp_z; :605 / :650)
    w_d  = exp(Zn_d) * a_d,  a_f = alpha, a_p = 1 - alpha  (Z_d None: w_d = a_d)
    out  = (splat([V_f w_f]) + splat([V_p w_p])) / max(splat(w_f) + splat(w_p), eps)

With the same features and logits in both directions this is splat_f64.training_step (tests/test_splat_blend_host.py ties the two).
"""
import torch

import splat_f64 as F64


def weights(z, a, like, dtype, clamp_z, subtract_max):
    if z is None:
        return torch.ones(like.shape[0], 1, like.shape[2], like.shape[3], dtype=dtype) * a
    zn = z.to(dtype)
    if subtract_max:
        zn = zn - zn.max()
    if clamp_z is not None:
        zn = torch.clamp(zn, min=clamp_z[0], max=clamp_z[1])
    return zn.exp() * a


def blend_f64(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, dtype=torch.float64, clamp_z=(-20.0, 20.0), subtract_max=True,
              eps=1e-8, return_norm=False):
    """start_fs / end_fs [N,C,H,W], z_* [N,1,H,W] or None, flow_* [N,2,H,W], alpha [N] (or [N,1,1,1]) -> [N,C,H,W] in `dtype`;
    differentiable in the six tensors."""
    N = start_fs.shape[0]
    a = alpha.to(dtype).reshape(N, 1, 1, 1)
    vf, vp = start_fs.to(dtype), end_fs.to(dtype)
    wf = weights(z_start, a, vf, dtype, clamp_z, subtract_max)
    wp = weights(z_end, 1 - a, vp, dtype, clamp_z, subtract_max)
    Sf = F64.splat_sum(torch.cat([vf * wf, wf], 1), flow_f, dtype)
    Sp = F64.splat_sum(torch.cat([vp * wp, wp], 1), flow_p, dtype)
    norm = Sf[:, -1:] + Sp[:, -1:]
    out = (Sf[:, :-1] + Sp[:, :-1]) / torch.clamp(norm, min=eps)
    return (out, norm) if return_norm else out
