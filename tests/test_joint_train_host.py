"""Host-side checks of joint training (``slr_sfs_amd.JointTrainingModel``, ``--train_motion``), none of which needs a GPU:

  * the written-out definition of tests/joint_train_f64.py reproduces the reference's own run
    (tests/golden/joint_train_vs_reference.npz, made by tools/make_golden_joint_train.py) within 10 E(def32) + 1e-6 on every loss entry
    and on PredImg, everything downstream of the flow started from the fixture's stored flow, and on PredMotion on its own;
  * two mutants of the glue fall outside that bound (pred * div_flow fed to the integration; the motion loss left out of Total Loss);
  * the checkpoint key set with shapes and the parameter order are the reference's lists; learns follows requires_grad, frozen included;
  * every refusal names its option, and ``TrainingModel`` still refuses ``train_motion``."""
import functools

import numpy as np
import pytest
import torch

import joint_train_f64 as J
import joint_train_fixture as JF
import train_step_f64 as T


@functools.lru_cache(maxsize=None)
def _runs():
    g = JF.load()
    flow = torch.from_numpy(g["flow"])
    return g, flow, J.forward(g, torch.float64, flow), J.forward(g, torch.float32, flow)


def _digest(name, t):
    return t.double().reshape(-1)[JF.positions(name, t.numel())]


def _model(**more):
    import slr_sfs_amd as S
    return S.JointTrainingModel(JF.options(**more), None, nf=JF.NF, encoder_widths=T.ENC_WIDTHS, decoder_widths=T.DEC_WIDTHS,
                                decoder_updown=T.UPDOWN)


def test_the_fixture_is_what_its_module_says(oracle):
    g = JF.load()
    assert g["flow"].shape == (JF.BS, 2, JF.W, JF.W) and g["flow"].dtype == np.float32
    (s, m, e), = JF.INDEX
    valid = (float(oracle.euler_integration(g["flow"], m - s)[1].mean()), float(oracle.euler_integration(-g["flow"], e + 1 - m)[1].mean()))
    print("valid fractions", valid)
    assert min(valid) >= 0.5 and np.allclose(valid, g["valid_fraction"])
    assert list(g["loss_keys"]) == ["ssim", "psnr", "L1", "Total Loss", "EndPointError"]
    assert list(g["pred_keys"]) == ["GTMotion", "OutputImg", "PredImg", "PredMotion", "Z_f"] and bool(g["GTMotion_is_the_batch"])
    assert JF.DIV_FLOW != 1.0 and JF.LOSSES == ["1.0_l1"]


def test_the_definition_reproduces_the_references_run():
    g, flow, r64, r32 = _runs()
    for k in g["loss_keys"]:
        e_ref, e_32 = J.rel(g["loss/" + k], r64["loss"][k]), J.rel(r32["loss"][k], r64["loss"][k])
        print(f"loss {k}: reference {float(g['loss/' + k]):.8g} definition {float(r64['loss'][k]):.8g} E_ref {e_ref:.3e} E_def32 {e_32:.3e}")
        assert e_ref <= 10 * e_32 + 1e-6, k
    assert set(r64["loss"]) == set(g["loss_keys"])
    # the in-place `+=` of :751: with one entry in `losses`, "L1" reads the total
    assert float(g["loss/L1"]) == float(g["loss/Total Loss"]) and float(r64["loss"]["L1"]) == float(r64["loss"]["Total Loss"])
    for name in ("PredImg", "PredMotion"):
        ref = torch.from_numpy(g[name + "#samples"])
        e_ref, e_32 = J.rel(ref, _digest(name, r64[name])), J.rel(_digest(name, r32[name]), _digest(name, r64[name]))
        print(f"{name}: E_ref {e_ref:.3e} E_def32 {e_32:.3e}")
        assert e_ref <= 10 * e_32 + 1e-6, name
        assert abs(float(g[name + "#max_abs"]) - float(r64[name].abs().max())) <= 1e-5 * float(g[name + "#max_abs"])
    # the flow the reference handed to its integration is PredMotion as it is: no div_flow
    e_flow = J.rel(flow, r64["PredMotion"])
    print(f"stored flow against the definition's PredMotion: {e_flow:.3e}")
    assert e_flow <= 10 * J.rel(r32["PredMotion"], r64["PredMotion"]) + 1e-6
    for k, v in r64["motion_state"].items():                                  # u and v of the motion network moved as the definition says
        if k.endswith("weight_u") or k.endswith("weight_v"):
            assert J.rel(torch.from_numpy(g["after/" + k]), v) <= 1e-5, k


@pytest.mark.parametrize("mutant", J.MUTANTS)
def test_mutants_of_the_glue_fall_outside_the_bound(mutant):
    g, flow, r64, r32 = _runs()
    m = J.forward(g, torch.float64, flow, (mutant,))
    out = []
    for k in ("L1", "Total Loss"):
        e_m, e_32 = J.rel(g["loss/" + k], m["loss"][k]), J.rel(r32["loss"][k], r64["loss"][k])
        print(f"{mutant} {k}: E {e_m:.3e} against the bound {10 * e_32 + 1e-6:.3e}")
        out.append(e_m > 10 * e_32 + 1e-6)
    assert all(out)
    if mutant == "div_flow":
        e_m = J.rel(torch.from_numpy(g["PredImg#samples"]), _digest("PredImg", m["PredImg"]))
        e_32 = J.rel(_digest("PredImg", r32["PredImg"]), _digest("PredImg", r64["PredImg"]))
        print(f"{mutant} PredImg: E {e_m:.3e} against the bound {10 * e_32 + 1e-6:.3e}")
        assert e_m > 10 * e_32 + 1e-6


def test_key_set_and_parameter_order_are_the_references():
    import slr_sfs_amd as S
    g = JF.load()
    model = _model()
    trainer = S.Trainer(model, JF.options())
    sd = trainer.reference_state_dict()
    ref = {("model.module." + k[len("model."):] if k.startswith("model.") else k): tuple(int(v) for v in s if v >= 0)
           for k, s in zip(g["state_keys"], g["state_shapes"])}
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert sum(k.startswith("model.module.motion_regressor.motion_predictor.") for k in sd) == 142
    assert not any("motion_regressor" in k and "motion_predictor" not in k for k in sd)
    rows = model.reference_parameters()
    assert [r[0] for r in rows] == list(g["parameter_order"])
    names = [r[0].split(".")[0] for r in rows]
    assert [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n] == ["encoder", "motion_regressor", "projector"]
    motion = [r for r in rows if r[0].startswith("motion_regressor.")]
    assert len(motion) == 110 and all(r[2] for r in motion) and all(r[1].requires_grad for r in motion)
    for r in motion:                                                           # a row's tensor (or its slice) has the reference's shape
        t = r[1] if len(r) == 3 else r[1][r[3]]
        assert tuple(t.shape) == ref["model.module." + r[0]], r[0]
    assert sum(len(r) == 4 for r in rows) == 13 * 4
    # frozen (train_animating_fixmotion.py:448-450): the same rows, none of the motion network's learns, nothing else changes
    before = [(r[0], r[2]) for r in rows]
    model.freeze_motion()
    after = model.reference_parameters()
    assert [r[0] for r in after] == [k for k, _ in before]
    for (k, l0), r in zip(before, after):
        assert r[2] == (l0 and not k.startswith("motion_regressor.")), k
    frozen_ref = dict(zip(g["parameter_order"], g["parameter_learns_frozen"]))
    assert not any(frozen_ref[r[0]] for r in after if r[0].startswith("motion_regressor."))
    assert all(frozen_ref[r[0]] for r in after if r[2])
    # the state dict loads strictly and comes back; a motion checkpoint goes in under the renamed keys
    first = JF.reference_state_dict()
    model.load_reference_state_dict(first)
    back = model.reference_state_dict()
    assert sorted(back) == sorted(first) and all(torch.equal(back[k], first[k]) for k in first)
    ckpt = {"model.module.motion_predictor." + k: v + 0.5 for k, v in JF.motion_state().items()}
    ckpt["model.module.loss_function.something"] = torch.zeros(1)              # (not a motion_predictor key: not used, :441-445)
    model.load_motion_regressor(ckpt)
    back = model.reference_state_dict()
    for k, v in JF.motion_state().items():
        assert torch.equal(back["model.module.motion_regressor.motion_predictor." + k], v + 0.5), k
    assert torch.equal(back["model.module.encoder.gblocks.0.ch_a.2.bias"], first["model.module.encoder.gblocks.0.ch_a.2.bias"])
    short = dict(ckpt)
    del short["model.module.motion_predictor.conv3.weight_u"]
    with pytest.raises(KeyError, match="missing"):
        model.load_motion_regressor(short)
    for bad, err in ((dict(first, **{"model.module.motion_regressor.motion_predictor.conv9.bias": torch.zeros(1)}), "unexpected"),
                     ({k: v for k, v in first.items() if not k.endswith("dconv2.weight_v")}, "missing")):
        with pytest.raises(KeyError, match=err):
            model.load_reference_state_dict(bad)


def test_every_refusal_names_its_option():
    import slr_sfs_amd as S
    with pytest.raises(NotImplementedError, match="train_motion"):
        S.TrainingModel(JF.options())                                          # the plain model goes on refusing it
    with pytest.raises(NotImplementedError, match="train_motion"):
        S.model.check_options(JF.options())
    for more, word in ((dict(train_motion=False), "train_motion"), (dict(motionW=128), "motionW"), (dict(motionH=512), "motionH"),
                       (dict(motion_model_type="SPADE_unet_mask_motion_uvm"), "motion_model_type"),
                       (dict(motion_model_type="unet_motion"), "motion_model_type"),
                       (dict(use_mask_as_motion_input=False), "use_mask_as_motion_input"),
                       (dict(use_hint_as_motion_input=False), "use_hint_as_motion_input"),
                       (dict(motion_norm_G="sync:spectral_batch"), "motion_norm_G"), (dict(motion_losses=["1.0_MotionSmooth"]), "motion_losses"),
                       (dict(use_rgb_features=True), "use_rgb_features"), (dict(use_softmax_splatter_v2=True), "use_softmax_splatter_v2"),
                       (dict(random_ff_mask=True), "random_ff_mask"), (dict(refine_model_type="resnet_256W8UpDown64_skip_warp"), "skip_warp"),
                       (dict(pconv="pconv_other"), "pconv"), (dict(norm_G="sync:batch"), "norm_G")):
        with pytest.raises(NotImplementedError, match=word):
            _model(**more)
        if word not in ("use_mask_as_motion_input", "use_hint_as_motion_input", "motion_norm_G", "motion_losses"):      # (MotionTrainingModel's own)
            with pytest.raises(NotImplementedError, match=word):
                S.check_joint_options(JF.options(**more))
    S.check_joint_options(JF.options())
    model = _model()
    b = JF.batch()
    with pytest.raises(KeyError, match="hints"):
        model({k: v for k, v in b.items() if k != "hints"})
    with pytest.raises(NotImplementedError, match="no CPU path"):
        model(b)                                                               # there is no fallback
    assert isinstance(model, S.TrainingModel) and model.synthesis.euler_pair is True and S.TrainingModel(JF.options(train_motion=False)).synthesis.euler_pair is False
    for bad in (1, None, "yes"):
        with pytest.raises(TypeError, match="deterministic"):
            S.JointTrainingModel(JF.options(), None, nf=JF.NF, deterministic=bad)
