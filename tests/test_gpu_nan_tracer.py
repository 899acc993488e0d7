"""The training kernels on a NaN: same footprint as float64, none lost (tests/nan_tracer.py has the criterion, the plants and the case
table; tests/test_nan_tracer_host.py shows on the CPU that no case of the table is vacuous).

One NaN is planted in one input and the operator runs again: every output must be NaN exactly where the float64 definition of the
planted input is NaN, and have the bits of the clean run everywhere else -- no tolerance.  A NaN that a kernel swallows (fmaxf(NaN, 0)
= 0), a halo that is off by one, a channel tile past a ragged Cin that reads the next sample's planes against zero weights (0 x NaN =
NaN on the matrix cores too), padding by multiplication, a partial sum filed under a neighbour's plane: each of them changes the map.

Cases (N = 2 everywhere; 5 x 7 is the scalar body of the elementwise kernels and 16 x 20 the 16-byte one; both layouts wherever
C % 8 == 0; the convolution shapes are those of tests/test_gpu_conv_train.py, test_gpu_block_train.py and test_gpu_disc.py: one tile,
ragged tiles with Cin 40 / Cout 72, the K split of the 4x4 kernels):
  conv3x3, pconv3x3 (also a plant in the mask plane), scale_bias, conv1x1, conv4x4 (stride 1 and 2, fused LeakyReLU and its gate in the
  backward, odd sizes: all four parity classes), bn (masked / unmasked, batch / stored statistics), bn_nonzero, pconv_epilogue, resample
  (both stages and their adjoints), instnorm, l1, gate (three modes), relu_maxpool (forward and backward, windows with one, two and
  four NaNs), adam (the tensor list of tests/test_gpu_adam.py with its misaligned views) and spectral (sigma and the list-wide weight
  gradient over 130 misaligned tensors).

Left out:
  * the split-f16 rung: its range clamp turns a NaN into a bound by design;
  * the fused BN + ReLU prologue and epilogue of csrc/conv.hip and csrc/pconv.hip, which are on the timed inference path (the update
    mask's clamp in them is covered by the mask plant of pconv3x3);
  * the splat and blend operators, which have non-finite families of their own against the oracle;
  * euler_backward, which uses atomics and so has no clean-run bits;
  * the discriminator step of the iteration: the whole-iteration case runs the generator step.

conv4x4s2 is slr_conv4x4s2_forward of the motion encoder with its LeakyReLU in front and its affine epilogue (plants in x, w, the bias,
the scale and the shift; it has no backward).  The whole iteration (test_whole_iteration_...) runs ``Trainer`` without the discriminator
at the shape of tests/test_gpu_train_step.py with a NaN in one pixel of the start image and, separately, in one decoder weight: every
entry of the returned loss dict and every parameter after the optimiser step is NaN exactly where the float64 iteration's is (it asks
for no clean-run bits, so the forward splat's summation order does not matter).

On the build before DESIGN 3.16 these fail: every bn, bn_nonzero and gate case, relu_maxpool, conv3x3, pconv3x3, conv4x4 at 33 x 20
stride 1, resample-Up, spectral (36 of the table's 59) and both plants of the whole iteration."""
import pytest
import torch

import adam_f64 as A64
import nan_tracer as NT
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda"
X_B8, G_B8 = 1, 2


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def _placed(t, blocked):
    return (to_blocked(t) if blocked else t).to(DEV)


def _back(t, blocked):
    if t is None:
        return None
    t = t.detach().cpu()
    return from_blocked(t) if blocked else t


def _nan(*shape):
    return torch.full(shape, NT.NAN, device=DEV)


# ------------------------------------------------------------------ the device side of every family: inputs (CPU) -> {output: CPU tensor}
# An output "name@variant" is held to the definition's output "name".

def _weight_grad3(S, x, g, cout, layout, splits):
    N, cin, H, W = x.shape
    dw, db = _nan(cout, cin, 3, 3), _nan(cout)
    nbytes = int(S._lib.lib().slr_conv3x3_grad_ws_bytes(N, cin, cout, H, W, splits))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    S._lib.call("slr_conv3x3_weight_grad", x.device, x, g, dw, db, N, cin, cout, H, W, splits, layout, ws, nbytes)
    return dw.cpu(), db.cpu()


def run_conv3x3(S, i):
    cout, cin = i["w"].shape[:2]
    out = {}
    for b8 in ((False, True) if cin % 8 == 0 and cout % 8 == 0 else (False,)):
        x, w, b = _placed(i["x"], b8).requires_grad_(), i["w"].to(DEV).requires_grad_(), i["b"].to(DEV).requires_grad_()
        y = S.conv3x3(x, w, b, in_b8=b8, out_b8=b8)
        y.backward(_placed(i["g"], b8))
        out.update({f"out@b8={b8}": _back(y, b8), f"dx@b8={b8}": _back(x.grad, b8), f"dw@b8={b8}": w.grad.cpu(), f"db@b8={b8}": b.grad.cpu()})
        for splits in NT.SPLITS:
            lay = (X_B8 | G_B8) if b8 else 0
            out[f"dw@b8={b8} splits={splits}"], out[f"db@b8={b8} splits={splits}"] = \
                _weight_grad3(S, _placed(i["x"], b8), _placed(i["g"], b8), cout, lay, splits)
    return out


def run_pconv3x3(S, i):
    cout, cin = i["w"].shape[:2]
    xm, out = i["x"] * i["mask"], {}
    for b8 in ((False, True) if cin % 8 == 0 and cout % 8 == 0 else (False,)):
        x, w, b = _placed(xm, b8).requires_grad_(), i["w"].to(DEV).requires_grad_(), i["b"].to(DEV).requires_grad_()
        y, um = S.partial_conv3x3(x, i["mask"].to(DEV), w, b, in_b8=b8, out_b8=b8)
        y.backward(_placed(i["g"], b8))
        out.update({f"out@b8={b8}": _back(y, b8), f"um@b8={b8}": um.cpu(), f"dx@b8={b8}": _back(x.grad, b8), f"dw@b8={b8}": w.grad.cpu(),
                    f"db@b8={b8}": b.grad.cpu()})
    return out


def run_scale_bias(S, i):
    N, C, H, W = i["g"].shape
    out = {}
    for b8 in ((False, True) if C % 8 == 0 else (False,)):
        gr, db = _nan(N, C, H, W), _nan(C)
        nbytes = int(S._lib.lib().slr_conv3x3_grad_ws_bytes(N, 0, C, H, W, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        S._lib.call("slr_conv_grad_scale_bias", torch.device(DEV), _placed(i["g"], b8), i["r"].to(DEV), i["um"].to(DEV), gr, db, N, C, H, W,
                    G_B8 if b8 else 0, ws, nbytes)
        out.update({f"gr@b8={b8}": _back(gr, b8), f"db@b8={b8}": db.cpu()})
    return out


def run_conv1x1(S, i):
    cout, cin = i["w"].shape[:2]
    out = {}
    for b8 in ((False, True) if cin % 8 == 0 and cout % 8 == 0 else (False,)):
        x, w, b = _placed(i["x"], b8).requires_grad_(), i["w"].to(DEV).requires_grad_(), i["b"].to(DEV).requires_grad_()
        y = S.conv1x1(x, w, b, in_b8=b8, out_b8=b8)
        y.backward(_placed(i["g"], b8))
        out.update({f"out@b8={b8}": _back(y, b8), f"dx@b8={b8}": _back(x.grad, b8), f"dw@b8={b8}": w.grad.cpu(), f"db@b8={b8}": b.grad.cpu()})
    return out


def run_conv4x4(S, i):
    out = {}
    for splits in (0, 3):
        x, w, b = i["x"].to(DEV).requires_grad_(), i["w"].to(DEV).requires_grad_(), i["b"].to(DEV).requires_grad_()
        y = S.conv4x4(x, w, b, stride=i["stride"], leaky=i["leaky"], _splits=splits)
        y.backward(i["g"].to(DEV))
        out.update({f"out@splits={splits}": y.detach().cpu(), f"dx@splits={splits}": x.grad.cpu(), f"dw@splits={splits}": w.grad.cpu(),
                    f"db@splits={splits}": b.grad.cpu()})
    return out


def run_conv4x4s2(S, i):
    """slr_conv4x4s2_forward as nets.Conv4x4s2 calls it, with the affine epilogue's tables given directly."""
    N, cin, H, W = i["x"].shape
    cout = i["w"].shape[0]
    dev = torch.device(DEV)
    w = i["w"].to(DEV)
    frag = torch.empty(S._lib.lib().slr_conv4x4s2_weight_bytes(cout, cin), dtype=torch.uint8, device=DEV)
    S._lib.call("slr_conv4x4s2_f32_weights", dev, w, frag, cout, cin)
    out = _nan(N, cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1)
    sc, sh = (i["scale"].to(DEV), i["shift"].to(DEV)) if "scale" in i else (None, None)
    S._lib.call("slr_conv4x4s2_forward", dev, i["x"].to(DEV), frag, i["b"].to(DEV), sc, sh, out, N, cin, cout, H, W, int(i["leaky"]), 0.2)
    return dict(out=out.cpu())


def _run_bn(S, i, nonzero):
    C = i["x"].shape[1]
    stored = "mean" in i
    out = {}
    for b8 in ((False, True) if C % 8 == 0 else (False,)):
        x, gain, bias = _placed(i["x"], b8).requires_grad_(), i["gain"].to(DEV).requires_grad_(), i["bias"].to(DEV).requires_grad_()
        st = dict(mean=i["mean"].to(DEV), var=i["var"].to(DEV)) if stored else {}
        if nonzero:
            res = S.bn_relu_nonzero_train(x, gain, bias, b8=b8, **st)
            out[f"msum@b8={b8}"] = res[3].cpu()
        else:
            res = S.bn_relu_mask_train(x, None if "mask" not in i else i["mask"].to(DEV), gain, bias, b8=b8, **st)
        res[0].backward(_placed(i["ga"], b8))
        out.update({f"a@b8={b8}": _back(res[0], b8), f"dx@b8={b8}": _back(x.grad, b8), f"dgain@b8={b8}": gain.grad.cpu(),
                    f"dbias@b8={b8}": bias.grad.cpu()})
        if not stored:
            out.update({f"mean@b8={b8}": res[1].cpu(), f"var@b8={b8}": res[2].cpu()})
    return out


def run_bn(S, i):
    return _run_bn(S, i, False)


def run_bn_nonzero(S, i):
    return _run_bn(S, i, True)


def run_pconv_epilogue(S, i):
    N, C, H, W = i["raw"].shape
    out = {}
    for b8 in ((False, True) if C % 8 == 0 else (False,)):
        res = _nan(N, C, H, W)
        S._lib.call("slr_pconv_train_epilogue", torch.device(DEV), _placed(i["raw"], b8), i["ratio"].to(DEV), i["um"].to(DEV), i["bias"].to(DEV),
                    _placed(i["residual"], b8), res, N, C, H, W, int(b8))
        out[f"out@b8={b8}"] = _back(res, b8)
    return out


def run_resample(S, i):
    op = S.avgpool_down if i["kind"] == "Down" else S.upsample_up
    out = {}
    for b8 in (False, True):
        x = _placed(i["x"], b8).requires_grad_()
        y = op(x, b8)
        y.backward(_placed(i["g"], b8))
        out.update({f"y@b8={b8}": _back(y, b8), f"dx@b8={b8}": _back(x.grad, b8)})
    return out


def run_instnorm(S, i):
    x = i["x"].to(DEV).requires_grad_()
    y = S.adversarial.instnorm_lrelu(x)
    y.backward(i["gy"].to(DEV))
    return dict(y=y.detach().cpu(), dx=x.grad.cpu())


def run_l1(S, i):
    out = {}
    n = i["pred"].numel()
    for offset in (0, 1):                                # (offset 1: contiguous tensors that are only 4-byte aligned, the scalar path)
        dev = lambda t: torch.empty(n + offset, device=DEV)[offset:].view(t.shape).copy_(t)      # noqa: E731
        p = dev(i["pred"]).requires_grad_()
        loss = S.losses.l1_loss(p, dev(i["gt"]))
        (NT.L1_SCALE * loss).backward()
        out.update({f"loss@offset={offset}": loss.detach().cpu().reshape(1), f"grad@offset={offset}": p.grad.cpu()})
    return out


def run_gate(S, i):
    mode, a = i["mode"], i["a"]
    with_b, with_g = mode != "relu", mode != "seed"
    dev = lambda t: to_blocked(t).to(DEV)                                 # noqa: E731
    out = _nan(*a.shape)
    total = _nan(1) if with_b else None
    ws = S.losses._sum_ws(out, *a.shape) if with_b else None
    gscale = torch.tensor([NT.GATE_SCALE], dtype=torch.float32, device=DEV)
    S.losses._gate(dev(a), dev(i["b"]) if with_b else None, dev(i["g"]) if with_g else None, total, out, NT.GATE_COEF / a.numel(), gscale, ws)
    res = dict(out=from_blocked(out.cpu()))
    if with_b:
        res["sum"] = total.cpu()
    return res


def run_relu_maxpool(S, i):
    N, C, H, W = i["x"].shape
    x = to_blocked(i["x"]).to(DEV)
    y, dx = _nan(N, C, H // 2, W // 2), _nan(N, C, H, W)
    S._lib.call("slr_relu_maxpool2x2_b8", x.device, x, y, N, C, H, W)
    S._lib.call("slr_relu_maxpool2x2_backward_b8", x.device, x, to_blocked(i["g"]).to(DEV), dx, N, C, H, W)
    return dict(y=from_blocked(y.cpu()), dx=from_blocked(dx.cpu()))


def run_adam(S, i):
    from test_gpu_adam import _offsets, _placed as placed_list, _resumed
    beta1, beta2, lr, _, t0 = A64.SETTINGS[NT.ADAM_SETTING]
    cuts = NT.adam_cuts()
    poff, goff = _offsets()
    params = placed_list(torch.split(i["p"], cuts), poff)
    for p, g in zip(params, placed_list(torch.split(i["g"], cuts), goff)):
        p.grad = g
    opt = S.Adam(params, lr=lr, betas=(beta1, beta2))
    _resumed(opt, params, torch.split(i["m"], cuts), torch.split(i["v"], cuts), t0)
    opt.step()
    cat = lambda ts: torch.cat([t.detach().cpu().reshape(-1) for t in ts])    # noqa: E731
    return dict(p=cat(params), m=cat([opt.state[p]["exp_avg"] for p in params]), v=cat([opt.state[p]["exp_avg_sq"] for p in params]))


def run_spectral(S, i):
    from test_gpu_spectral import _at
    shapes = i["shapes"]
    ws = [_at(w, (k + 1) % 4) for k, w in enumerate(NT.spectral_split(i["w"], shapes, "w"))]
    us = [_at(u, (k + 2) % 4) for k, u in enumerate(NT.spectral_split(i["u"], shapes, "u"))]
    vs = [_at(v, (k + 3) % 4) for k, v in enumerate(NT.spectral_split(i["v"], shapes, "v"))]
    dws = [_at(d, k % 4) for k, d in enumerate(NT.spectral_split(i["dw"], shapes, "w"))]
    inv, su, sv, offs = S.spectral_sigma(ws, us, vs, training=True)
    grads = S.spectral_weight_grad_multi(dws, ws, su, sv, offs, inv)
    cat = lambda ts: torch.cat([t.detach().cpu().reshape(-1) for t in ts])    # noqa: E731
    return {"inv_sigma": inv.cpu(), "u": cat(us), "v": cat(vs), "u@saved": su.cpu(), "v@saved": sv.cpu(), "grad": cat(grads)}


RUNNERS = dict(conv4x4s2=run_conv4x4s2, conv3x3=run_conv3x3, pconv3x3=run_pconv3x3, scale_bias=run_scale_bias, conv1x1=run_conv1x1, conv4x4=run_conv4x4, bn=run_bn,
               bn_nonzero=run_bn_nonzero, pconv_epilogue=run_pconv_epilogue, resample=run_resample, instnorm=run_instnorm, l1=run_l1,
               gate=run_gate, relu_maxpool=run_relu_maxpool, adam=run_adam, spectral=run_spectral)


def test_every_case_of_the_table_has_a_device_side():
    assert {name.split("-")[0] for name in NT.CASES} == set(RUNNERS)


@pytest.mark.parametrize("name", sorted(NT.CASES))
def test_nan_goes_where_float64_sends_it_and_nowhere_else(S, name):
    case = NT.CASES[name]
    run = RUNNERS[name.split("-")[0]]
    clean, ref_clean = run(S, case.inputs()), case.ref_clean()
    assert {k.split("@")[0] for k in clean} == set(ref_clean), (sorted(clean), sorted(ref_clean))
    assert not any(torch.isnan(v).any() for v in clean.values()), "the clean run holds a NaN"
    again = run(S, case.inputs())
    assert all(torch.equal(clean[k], again[k]) for k in clean), "the clean run has no bits to keep: two runs differ"
    failed, runs = [], case.runs()
    for key, pname, index in runs:
        inp = case.with_plant(key, index)
        got, ref, ref32 = run(S, inp), case.ref(inp), None
        for out_key in sorted(got):
            rk = out_key.split("@")[0]
            footprint, bits = NT.mismatches(got[out_key], clean[out_key], ref[rk], ref_clean[rk], rk in case.rederived)
            if rk in case.rederived:
                # the elements whose finite value is formed again from a decision the plant changed have no clean-run bits to keep:
                # they are held to float64 by the criterion of tests/test_gpu_disc.py, E_gpu <= 10 E_plain32 + 1e-6 over the tensor's
                # elements that are not NaN, E_plain32 from the definition's own float32 run of the planted input
                free = NT.expected(clean[out_key], ref[rk], ref_clean[rk], True)[2]
                if bool(free.any()):
                    ref32 = ref32 if ref32 is not None else case.ref(inp, torch.float32)
                    ok = ~torch.isnan(ref[rk])
                    top = float(ref[rk][ok].abs().max())
                    e_gpu = float((got[out_key].double() - ref[rk])[free].abs().max()) / top
                    e_plain = float((ref32[rk].double() - ref[rk])[ok & ~torch.isnan(ref32[rk])].abs().max()) / top
                    if not e_gpu <= 10.0 * e_plain + 1e-6:
                        failed.append(f"{key}[{pname}] -> {out_key}: re-derived elements E_gpu {e_gpu:.3e} > 10 x E_plain32 {e_plain:.3e} + 1e-6")
            if footprint or bits:
                failed.append(f"{key}[{pname}] -> {out_key}: {footprint} elements differ in NaN-ness (float64 {int(torch.isnan(ref[rk]).sum())} NaN, "
                              f"kernel {int(torch.isnan(got[out_key]).sum())} of {ref[rk].numel()}), {bits} lost the clean bits")
    print(f"{name}: {len(runs)} plants x {len(clean)} outputs, {len(failed)} mismatches")
    for line in failed:
        print("   ", line)
    assert not failed, f"{name}: {len(failed)} mismatches, the first: {failed[0]}"


# ------------------------------------------------------------------ 9. one whole iteration, the generator step only

def _iteration(S, g, inputs):
    """One ``Trainer`` iteration without the discriminator from the state in the fixture dict ``g`` on ``inputs`` (host):
    ({loss entry: tensor}, {reference key: the parameter after the optimiser step})."""
    import test_gpu_train_step as TS
    import train_step_f64 as T
    opts = T.options(discriminator_losses="0")
    model = S.TrainingModel(opts, TS._vgg(S), encoder_widths=T.ENC_WIDTHS, decoder_widths=T.DEC_WIDTHS, decoder_updown=T.UPDOWN)
    trainer = S.Trainer(model, opts).to(DEV).train()
    model.load_reference_state_dict(T.state_dict(g))
    model.defer_weight_grad(True)
    losses, _ = trainer(iter([TS._to_device(inputs)]), num_steps=1)
    torch.cuda.synchronize()
    return ({k: v.detach().cpu().reshape(()) for k, v in losses.items()},
            {k: t.detach().cpu() for k, t, learns in model.reference_parameters() if learns})


@pytest.mark.parametrize("plant", sorted(NT.ITERATION_PLANTS))
def test_whole_iteration_is_nan_where_the_float64_iteration_is(S, plant):
    g, inputs = NT.iteration_case(plant)
    ref_losses, ref_after = NT.iteration_ref(g, inputs)
    losses, after = _iteration(S, g, inputs)
    assert sorted(losses) == sorted(ref_losses) and sorted(after) == sorted(ref_after), (sorted(losses), sorted(ref_losses))
    wrong = [k for k in ref_losses if bool(torch.isnan(losses[k])) != bool(torch.isnan(ref_losses[k]))]
    print(f"{plant}: losses {dict((k, float(v)) for k, v in losses.items())}; float64 {dict((k, float(v)) for k, v in ref_losses.items())}")
    params = [k for k in ref_after if not torch.equal(torch.isnan(after[k]), torch.isnan(ref_after[k]))]
    print(f"{plant}: {len(wrong)} of {len(ref_losses)} loss entries and {len(params)} of {len(ref_after)} parameters differ in NaN-ness from float64")
    assert not wrong and not params, (wrong, params[:5])
    if plant == "pixel":                                 # the clean iteration holds no NaN, here and in float64
        g0, in0 = NT.iteration_case(None)
        l0, a0 = _iteration(S, g0, in0)
        assert not any(bool(torch.isnan(v)) for v in l0.values()) and not any(bool(torch.isnan(v).any()) for v in a0.values())
