"""The training iteration of the reference for its default configuration (train_animating_scripts/train_baseline2_pconv.sh:
``softmax_splating``, ``resnet_256W8UpDown64_de_resnet_pconv2_nonorm``, ``pconv_pbn_woresbias``, ``--norm_G sync:spectral_batch``,
``--train_Z``, ``--normalize_image``, the pix2pixHD discriminator), put together from this package's pieces.

``TrainingModel`` is ``AnimatingSoftmaxSplating`` (models/animating_softmax_splating.py:176-237, forward :445-775): the encoder on the
start and on the end image, ``TrainingSynthesis``, the decoder, ``tanh``, ``SynthesisLoss``.  ``Trainer`` is ``BaseModel``
(models/base_model.py:8-163): the discriminator, both optimisers and ``__call__`` in the reference's order.  Module names, buffers and
the checkpoint's keys are the reference's, so its checkpoints load strictly and are written back whole.  The generator's group of
spectrally normalised tensors runs with the deferred weight gradient (``spectral.defer_weight_grad``): one list-wide pair of launches
per network forward's backward.  Nothing in a forward or in a whole iteration synchronises the host when the batch is on the device.
There is no fallback: CPU tensors raise.
"""
import copy

import torch
from torch import nn

from . import spectral as _spectral
from .adversarial import DiscriminatorLoss
from .losses import VGG19_CONVS, PerceptualLoss, SynthesisLoss, load_vgg19_state_dict
from .optim import TrainingOptimizers, _value
from .trainable import TrainableDecoderPconv2, TrainableEncoderWithZ
from .training import _UNSUPPORTED, TrainingSynthesis, _flag, _has

REFINE_MODEL_TYPE = "resnet_256W8UpDown64_de_resnet_pconv2_nonorm"
PCONV, NORM_G = "pconv_pbn_woresbias", "sync:spectral_batch"
_VGG_SLICE_STARTS = (0, 2, 7, 12, 21)                    # architectures.py:93-102: features[0:2], [2:7], [7:12], [12:21], [21:30]


def _refuse(name, why=""):
    raise NotImplementedError(f"slr_sfs_amd.TrainingModel: option {name} is not implemented{why}")


def check_options(opts):
    """The option paths of the reference's forward() that this model does not take raise NotImplementedError naming the flag: everything
    ``TrainingSynthesis`` refuses, ``train_motion``, the ``skip_warp`` / ``multires`` refine types (and any other refine type, partial
    convolution or generator norm than the default configuration's), ``use_rgb_features``; depth regression (a batch with ``depth`` under ``use_gt_depth`` = False) is refused by the forward."""
    for name in _UNSUPPORTED + ("train_motion", "use_rgb_features"):
        if _flag(opts, name):
            _refuse(name)
    refine = _value(opts, "refine_model_type", REFINE_MODEL_TYPE)
    for part in ("skip_warp", "multires"):
        if part in refine:
            _refuse(f"refine_model_type={refine} ({part})")
    if refine != REFINE_MODEL_TYPE:
        _refuse(f"refine_model_type={refine}", f" (only {REFINE_MODEL_TYPE})")
    if _value(opts, "pconv", PCONV) != PCONV:
        _refuse(f"pconv={_value(opts, 'pconv', PCONV)}", f" (only {PCONV})")
    if _value(opts, "norm_G", NORM_G) != NORM_G:
        _refuse(f"norm_G={_value(opts, 'norm_G', NORM_G)}", f" (only {NORM_G})")


def _vgg_key(idx):
    k = max(i for i, s in enumerate(_VGG_SLICE_STARTS) if s <= idx)
    return f"slice{k + 1}.{idx}"


def _in_reference_order(net, plain):
    """(reference key, tensor, learns) of every PARAMETER the reference's network has, in the order of its ``parameters()``: per block the
    noise layers' gain and bias, then each convolution's bias before its ``weight_orig`` (spectral_norm re-registers the weight last);
    ResNet_Block keeps the first noise layer and convolution before the second pair (ch_a is one Sequential), ResNet_Block_Pconv2 both
    noise layers before the convolutions, and its never-called ``conv_b`` is a parameter there, too (learns = False: a buffer here)."""
    out = []
    for i, blk in enumerate(net.blocks):
        b = ("gblocks" if plain else "eblocks") + f".{i}."

        def noise(bn, key):
            return [(b + key + ".gain.weight_orig", bn.gain.weight_orig, True), (b + key + ".bias.weight_orig", bn.bias.weight_orig, True)]

        def conv(c, key):
            rows = [] if c.bias is None else [(b + key + ".bias", c.bias, True)]
            return rows + [(b + key + ".weight_orig", c.weight_orig, True)]
        if plain:
            out += noise(blk.bn1, "ch_a.0") + conv(blk.conv_aa, "ch_a.2") + noise(blk.bn2, "ch_a.3") + conv(blk.conv_ab, "ch_a.5")
            if blk.conv_b is not None:
                out += conv(blk.conv_b, "ch_b.0")
        else:
            out += noise(blk.bn1, "bn_noise1") + noise(blk.bn2, "bn_noise2") + conv(blk.conv_aa, "conv_aa") + conv(blk.conv_ab, "conv_ab")
            if blk.conv_b is not None:
                out += conv(blk.conv_b, "conv_b")
            else:
                out.append((b + "conv_b.weight_orig", blk.conv_b_unused.weight_orig, False))
    return out


class TrainingModel(nn.Module):
    """``AnimatingSoftmaxSplating`` for training.  forward(batch) -> (loss_dict, pred_dict), the reference's line by line:

    batch["images"]: [start, middle, end], each [B,3,W,W] in [-1, 1]; batch["motions"] [B,2,W,W], or [B,3,W,W] (``uvm``: the flow is
    ``m[:, :2] * m[:, 2:3]``); batch["index"]: a list of three index tensors [B], a [B,3] tensor, or (a batch of one) a [3] tensor.  Optional
    batch["noise"] = {"start": ..., "end": ..., "projector": ...}: the (noise1, noise2) pairs of every block for the two encoder calls
    and the decoder (drawn from torch.randn in training mode where absent, as the reference's layers do).
    loss_dict: ``SynthesisLoss``'s; pred_dict: OutputImg (the middle image), PredImg, Z_f (the clamped logits the forward splat used,
    detached: for reporting), GTMotion.

    ``vgg``: the ``VGG19Features`` of the content loss.  encoder_widths / decoder_widths / decoder_updown: other widths than the
    reference's (tests).  ``deterministic`` (keyword only, a bool): the run-to-run reproducible forward of ``splat_blend`` -- with it two
    iterations from the same state are bit-equal (``training.splat_blend_fallback_count`` must read 0: DESIGN 3.7.1)."""

    def __init__(self, opts, vgg=None, *, encoder_widths=None, decoder_widths=None, decoder_updown=None, deterministic=False):
        super().__init__()
        self._check_options(opts)
        self.opt = opts
        feat = int(_value(opts, "out_channel", _value(opts, "ngf", 64)))
        self.encoder = TrainableEncoderWithZ(cin=3, feat=feat, widths=encoder_widths, spectral=True)
        self.synthesis = TrainingSynthesis(opts, deterministic=deterministic)
        self.projector = TrainableDecoderPconv2(cin=int(_value(opts, "ngf", feat)), cout=3, widths=decoder_widths, updown=decoder_updown,
                                                spectral=True)
        if self.projector.blocks[0].conv_aa.cin != feat:
            raise ValueError(f"TrainingModel: the decoder reads ngf = {self.projector.blocks[0].conv_aa.cin} channels, the encoder writes {feat}")
        self.loss_function = SynthesisLoss(opts, vgg)
        self.register_buffer("min_z", torch.Tensor([0.1]))                                        # :230-237, literally
        self.register_buffer("max_z", torch.Tensor([_value(opts, "max_z", 10.0)]))
        self.register_buffer("discretized_zs", torch.linspace(_value(opts, "min_z", 0.5), _value(opts, "max_z", 10.0),
                                                              int(_value(opts, "voxel_size", 64))))
        self.relu_z = "relu" in str(_value(opts, "Z_model", "encoder"))
        self.defer_weight_grad(True)

    _check_options = staticmethod(check_options)             # (JointTrainingModel: check_joint_options)

    def defer_weight_grad(self, on=True):
        """One list-wide weight-gradient pair per network forward's backward (default), or the per-layer pairs."""
        _spectral.defer_weight_grad(self.encoder, on)
        _spectral.defer_weight_grad(self.projector, on)
        return self

    # ---- the batch, checked before the device is touched
    def _batch(self, batch):
        images = batch["images"]
        if not isinstance(images, (list, tuple)) or len(images) != 3:
            raise ValueError("TrainingModel: batch['images'] is [start, middle, end]")
        start = images[0]
        for name, t in (("start", images[0]), ("middle", images[1]), ("end", images[2]), ("motions", batch["motions"])):
            if not torch.is_tensor(t):
                raise TypeError(f"TrainingModel: {name}: a tensor is required, got {type(t).__name__}")
            if not t.is_cuda:
                raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
            if t.dtype != torch.float32:
                raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")
        if start.dim() != 4 or start.shape[1] != 3 or start.shape[2] != start.shape[3]:
            raise ValueError(f"TrainingModel: images [B,3,W,W] required, got {tuple(start.shape)}")
        bs, W = start.shape[0], start.shape[3]
        if _has(self.opt, "W") and int(_value(self.opt, "W", W)) != W:
            raise ValueError(f"TrainingModel: images of width {W}, the options say W = {_value(self.opt, 'W', W)}")
        for name, t in (("middle", images[1]), ("end", images[2])):
            if tuple(t.shape) != tuple(start.shape):
                raise ValueError(f"TrainingModel: the {name} image {tuple(t.shape)} does not match the start image {tuple(start.shape)}")
        motions = batch["motions"]
        if motions.dim() != 4 or motions.shape[0] != bs or motions.shape[1] not in (2, 3) or tuple(motions.shape[2:]) != (W, W):
            raise ValueError(f"TrainingModel: motions [B,2,W,W] or [B,3,W,W] required, got {tuple(motions.shape)}")
        if "depth" in batch and _has(self.opt, "use_gt_depth") and not _flag(self.opt, "use_gt_depth"):
            _refuse("use_gt_depth=False (depth regression)")
        index = batch["index"]
        if isinstance(index, (list, tuple)):                                                      # :462-473 (a tuple as a list)
            if len(index) != 3:
                raise ValueError(f"TrainingModel: batch['index'] as a list is [start, middle, end], got {len(index)} entries")
            idx = (index[0], index[1], index[2])
        elif not torch.is_tensor(index):
            raise TypeError(f"TrainingModel: batch['index'] is a list of three index tensors or a tensor, got {type(index).__name__}")
        elif len(index.shape) > 1:
            idx = (index[:, 0], index[:, 1], index[:, 2])
        else:
            idx = (index[0], index[1], index[2])
        return [t.contiguous() for t in images], motions, idx, bs, W

    def forward(self, batch):
        (start_img, middle_img, end_img), motions, (start_index, middle_index, end_index), bs, W = self._batch(batch)
        noise = batch.get("noise") or {}
        start_fs, Z_f = self.encoder(start_img, noise=noise.get("start"))                         # :486-487
        end_fs, Z_p = self.encoder(end_img, noise=noise.get("end"))
        if self.relu_z:                                                                           # :488-490
            Z_f, Z_p = torch.relu(Z_f), torch.relu(Z_p)
        flow, motion_out = self._motion(batch, start_img, motions, bs, W)                          # :514-546
        flow = flow.reshape(bs, 2, W, W).contiguous()                                             # :578
        gen_fs = self.synthesis(start_fs, Z_f, end_fs, Z_p, flow, start_index, middle_index, end_index)   # :579-692
        gen_img = self.projector(gen_fs.contiguous(), noise=noise.get("projector"))               # :742
        gen_img = torch.tanh(gen_img)                                                             # :744
        loss = self.loss_function(gen_img, middle_img)                                            # :746
        pred_dict = {"OutputImg": middle_img, "PredImg": gen_img, "Z_f": self._z_f_norm(Z_f, start_fs), "GTMotion": flow}     # :755-762
        if motion_out is not None:
            self._add_motion(loss, pred_dict, motion_out)                                         # :748-753, :764-766
        return loss, pred_dict

    def _motion(self, batch, start_img, motions, bs, W):
        """The flow the integration gets (:538-546: the batch's motion) and what the subclass's regressor returned (None here)."""
        if motions.shape[1] == 2:
            flow = motions
        else:
            flow = motions[:, :2, ...].clone()
            flow = flow * motions[:, 2:3, ...]
        return flow, None

    @torch.no_grad()
    def _z_f_norm(self, Z_f, start_fs):
        """The reference's Z_f_norm (:588-605), for reporting: the operator computes its own inside the kernel."""
        o = self.synthesis.options
        if not o["train_z"]:
            Z_f = start_fs.new_ones(start_fs.shape[0], 1, *start_fs.shape[2:])
        z = Z_f.detach().reshape(start_fs.shape[0], 1, *start_fs.shape[2:])
        if o["subtract_max"]:
            z = z - z.max()
        return z if o["clamp_z"] is None else torch.clamp(z, min=o["clamp_z"][0], max=o["clamp_z"][1])

    # ---- the reference's state dict
    def _vgg(self):
        for i, loss in enumerate(self.loss_function.losses):
            if isinstance(loss, PerceptualLoss):
                return i, loss.model
        return None, None

    def _reference_entries(self):
        """reference key (under ``model.module.``) -> tensor."""
        out = {"encoder." + k: t for k, t in _spectral._entries(self.encoder).items()}
        out.update({"projector." + k: t for k, t in _spectral._entries(self.projector).items()})
        i, vgg = self._vgg()
        if vgg is not None:                                                                       # the frozen VGG19 is a sub-module there
            for conv, idx in zip(vgg.convs, VGG19_CONVS):
                out[f"loss_function.losses.{i}.model.{_vgg_key(idx)}.weight"] = conv.weight
                out[f"loss_function.losses.{i}.model.{_vgg_key(idx)}.bias"] = conv.bias
        for name in ("min_z", "max_z", "discretized_zs"):
            out[name] = getattr(self, name)
        return out

    def reference_parameters(self):
        """[(reference key, tensor, learns)] in the order of the reference model's ``parameters()`` -- the indices of its ``optimizerG``
        state.  learns = False: frozen there (the VGG19) or never given a gradient (the decoder's unused ``conv_b``)."""
        out = [("encoder." + k, t, l) for k, t, l in _in_reference_order(self.encoder, True)]
        out += [("projector." + k, t, l) for k, t, l in _in_reference_order(self.projector, False)]
        i, vgg = self._vgg()
        if vgg is not None:
            for conv, idx in zip(vgg.convs, VGG19_CONVS):
                out += [(f"loss_function.losses.{i}.model.{_vgg_key(idx)}.weight", conv.weight, False),
                        (f"loss_function.losses.{i}.model.{_vgg_key(idx)}.bias", conv.bias, False)]
        return out

    def reference_state_dict(self, prefix="model.module."):
        """The reference model's complete key set with this model's tensors (detached clones)."""
        return {prefix + k: t.detach().clone() for k, t in self._reference_entries().items()}

    def check_reference_state_dict(self, sd, prefix="model.module."):
        """What ``load_reference_state_dict`` checks before it copies anything; returns the entries under ``prefix`` without it."""
        mine = self._reference_entries()
        theirs = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        missing, extra = sorted(set(mine) - set(theirs)), sorted(set(theirs) - set(mine))
        if missing or extra:
            raise KeyError(f"TrainingModel.load_reference_state_dict({prefix!r}): missing {missing[:4]} ({len(missing)}), "
                           f"unexpected {extra[:4]} ({len(extra)})")
        for k, t in mine.items():
            if tuple(theirs[k].shape) != tuple(t.shape):
                raise ValueError(f"TrainingModel.load_reference_state_dict: {prefix + k}: shape {tuple(theirs[k].shape)}, expected {tuple(t.shape)}")
        return theirs

    @torch.no_grad()
    def load_reference_state_dict(self, sd, prefix="model.module."):
        """Strict in both directions: every key under ``prefix`` is consumed, every tensor found with its shape; else KeyError /
        ValueError and the model is untouched.  The networks go through ``load_spectral_state_dict`` (unfolded: weight_orig, u, v)."""
        theirs = self.check_reference_state_dict(sd, prefix)
        _spectral.load_spectral_state_dict(self.encoder, sd, prefix + "encoder.")
        _spectral.load_spectral_state_dict(self.projector, sd, prefix + "projector.")
        i, vgg = self._vgg()
        if vgg is not None:
            head = f"loss_function.losses.{i}.model."
            load_vgg19_state_dict(vgg, {"features." + k[len(head):].split(".", 1)[1]: v for k, v in theirs.items() if k.startswith(head)})
        for name in ("min_z", "max_z", "discretized_zs"):
            getattr(self, name).copy_(theirs[name])
        return self


MOTION_MODEL_TYPE = "SPADE_unet_mask_motion"
_SPADE_ORDER = ("", "2_0", "2_1", "4_0", "4_1", "8_0", "8_1", "8_2", "8_3", "8_4", "8_5", "8_6", "8_7")      # architectures.py:655-667


def _with(opts, **kw):
    """A shallow copy of the options (a Namespace or a dict) with ``kw`` set."""
    new = copy.copy(opts)
    for k, v in kw.items():
        if isinstance(new, dict):
            new[k] = v
        else:
            setattr(new, k, v)
    return new


def check_joint_options(opts):
    """``JointTrainingModel``'s options: ``train_motion`` with ``motion_model_type SPADE_unet_mask_motion`` (the three-channel ``uvm``
    predictors and every other type raise NotImplementedError naming the option), ``motionW`` = ``motionH`` = ``W`` (the reference's
    ``flow_uvm.view(bs, 2, W, W)`` fails otherwise, animating_softmax_splating.py:526), and everything ``check_options`` refuses.  What
    ``MotionTrainingModel`` refuses it refuses when it is built."""
    if not _flag(opts, "train_motion"):
        raise NotImplementedError("slr_sfs_amd.JointTrainingModel: option train_motion is required (without it: TrainingModel)")
    kind = str(_value(opts, "motion_model_type", MOTION_MODEL_TYPE))
    if kind != MOTION_MODEL_TYPE:
        raise NotImplementedError(f"slr_sfs_amd.JointTrainingModel: option motion_model_type={kind} is not implemented (only {MOTION_MODEL_TYPE}"
                                  f"{'; three-channel uvm predictions are not built' if 'uvm' in kind else ''})")
    W = int(_value(opts, "W", 256))
    for name in ("motionW", "motionH"):
        if int(_value(opts, name, W)) != W:
            raise NotImplementedError(f"slr_sfs_amd.JointTrainingModel: option {name}={_value(opts, name, W)} differs from W={W} (the reference's "
                                      f"view(bs, 2, W, W) of the predicted motion fails there, too)")
    check_options(_with(opts, train_motion=False))


class JointTrainingModel(TrainingModel):
    """``AnimatingSoftmaxSplating`` under ``--train_motion --motion_model_type SPADE_unet_mask_motion``
    (train_animating_fixedMotion_finetuneFluid_IGANonly.sh): the frame synthesis trained on the motion the motion network PREDICTS.
    ``motion_regressor`` is ``MotionTrainingModel(opts with model_type = motion_model_type)`` (:189-193), called on {"images": [start],
    "motions", "hints"} between the encoder and the integration (:514-536); the flow is its ``PredMotion`` WITHOUT ``div_flow``, times
    [W / motionW, W / motionH] (= 1: the sizes are required equal); ``Total Loss`` gains the motion model's, its named losses are copied
    in, and pred_dict gains ``PredMotion`` and takes the motion model's ``GTMotion`` (:748-766).  batch: ``TrainingModel``'s with
    ``motions`` [B,2,W,W] the ground truth and ``hints`` [B,2,W,W].

    Both integrations run through ``euler_integration_pair``: with ``deterministic=True`` the gradient that reaches the motion network is
    the same bits from run to run as well.  ``load_motion_regressor`` takes a motion checkpoint of ``train_motion_unet.py``
    under the renamed keys, ``freeze_motion`` stops its parameters learning (both before the trainer's first step).  ``nf``: another width
    of the motion network than the reference's 32 (tests)."""

    _check_options = staticmethod(check_joint_options)

    def __init__(self, opts, vgg=None, *, nf=32, encoder_widths=None, decoder_widths=None, decoder_updown=None, deterministic=False):
        super().__init__(opts, vgg, encoder_widths=encoder_widths, decoder_widths=decoder_widths, decoder_updown=decoder_updown,
                         deterministic=deterministic)
        from .motion_training import MotionTrainingModel
        self.synthesis = TrainingSynthesis(opts, deterministic=deterministic, euler_pair=True)
        self.motion_regressor = MotionTrainingModel(_with(opts, model_type=_value(opts, "motion_model_type", MOTION_MODEL_TYPE)), nf=nf)

    def _batch(self, batch):
        if "hints" not in batch:                              # (before anything else: no device is needed to say so)
            raise KeyError("slr_sfs_amd.JointTrainingModel: batch['hints'] is required (option use_hint_as_motion_input)")
        out = super()._batch(batch)
        if out[1].shape[1] != 2:
            raise NotImplementedError("slr_sfs_amd.JointTrainingModel: three-channel uvm motions (motion_model_type) are not built")
        return out

    def _motion(self, batch, start_img, motions, bs, W):
        motion_loss, out = self.motion_regressor({"images": [start_img], "motions": motions, "hints": batch["hints"]})   # :516-523
        pred = out["PredMotion"]
        if pred.shape[1] != 2:
            raise NotImplementedError("slr_sfs_amd.JointTrainingModel: three-channel uvm predictions (motion_model_type) are not built")
        # :524-535: PredMotion as it is (no div_flow), times [W / motionW, W / motionH] = [1, 1] (check_joint_options): the same bits
        return pred.view(bs, 2, W, W), (motion_loss, out)

    def _add_motion(self, loss, pred_dict, motion_out):
        motion_loss, out = motion_out
        # :751 is an in-place `+=` on the tensor under "Total Loss" -- which IS the first named loss's tensor when `losses` has one entry
        # (SynthesisLoss leaves its first term unscaled), so that entry reads the new total as well.  Out of place here, same values.
        old = loss["Total Loss"]
        new = old + motion_loss["Total Loss"]
        for k in list(loss):
            if loss[k] is old:
                loss[k] = new
        for name in self.motion_regressor.loss_function.loss_names:                               # :752-753
            loss[name] = motion_loss[name]
        pred_dict["PredMotion"], pred_dict["GTMotion"] = out["PredMotion"], out["GTMotion"]       # :764-766

    # ---- parameters and checkpoints
    _MOTION = "motion_regressor.motion_predictor."

    def load_motion_regressor(self, state_dict, prefix="model.module."):
        """train_animating_fixmotion.py:438-446: the keys of a motion checkpoint that hold ``motion_predictor`` go under
        ``motion_regressor.motion_predictor``; the others are not used.  Strict on the network: every tensor found, every key consumed."""
        renamed = {k.replace("motion_predictor", self._MOTION[:-1]): v for k, v in state_dict.items() if "motion_predictor" in k}
        self.motion_regressor.motion_predictor.load_reference_state_dict(renamed, prefix + self._MOTION)
        return self

    def freeze_motion(self):
        """:448-450: the motion network's parameters stop learning (its u / v still move in train() mode, as the reference's do)."""
        for name, p in self.motion_regressor.named_parameters():
            if "motion_predictor" in name:
                p.requires_grad = False
        return self

    def _reference_entries(self):
        out = super()._reference_entries()
        for k, t, sl in self.motion_regressor.motion_predictor._reference_entries():
            out[self._MOTION + k] = t if sl is None else t[sl]
        return out

    def reference_parameters(self):
        """The parent's rows with the motion network's between encoder and projector, in the reference's registration order; the rows
        of ``mlp_gamma`` / ``mlp_beta`` carry the slice of ``mlp_gb`` they are.  learns: the parameter's ``requires_grad``."""
        rows = super().reference_parameters()
        net, mine = self.motion_regressor.motion_predictor, []
        for name in [f"conv{i}" for i in range(1, 9)] + [f"dconv{i}" for i in range(1, 9)]:
            m = getattr(net, name)
            mine += [(f"{name}.bias", m.bias, m.bias.requires_grad), (f"{name}.weight_orig", m.weight_orig, m.weight_orig.requires_grad)]
        for s in _SPADE_ORDER:
            sp = getattr(net, f"spade_layer{s}")
            sh, gb, C = sp.mlp_shared, sp.mlp_gb, sp.C
            mine += [(f"spade_layer{s}.mlp_shared.0.weight", sh.weight, sh.weight.requires_grad),
                     (f"spade_layer{s}.mlp_shared.0.bias", sh.bias, sh.bias.requires_grad)]
            for half, sl in (("mlp_gamma", slice(0, C)), ("mlp_beta", slice(C, 2 * C))):
                mine += [(f"spade_layer{s}.{half}.weight", gb.weight, gb.weight.requires_grad, sl),
                         (f"spade_layer{s}.{half}.bias", gb.bias, gb.bias.requires_grad, sl)]
        mine = [(self._MOTION + r[0],) + tuple(r[1:]) for r in mine]
        cut = max(k for k, r in enumerate(rows) if r[0].startswith("encoder.")) + 1
        return rows[:cut] + mine + rows[cut:]

    @torch.no_grad()
    def load_reference_state_dict(self, sd, prefix="model.module."):
        super().load_reference_state_dict(sd, prefix)                      # (checks every key and shape, the motion network's included)
        self.motion_regressor.motion_predictor.load_reference_state_dict(sd, prefix + self._MOTION)
        return self


class Trainer(nn.Module):
    """``BaseModel`` (models/base_model.py): ``model``, with ``opts.discriminator_losses != '0'`` the discriminator ``netD``
    (``DiscriminatorLoss``: gan_mode, lambda_feat, no_ganFeat_loss, ndf, output_nc read from ``opts``), and the optimisers of
    ``TrainingOptimizers`` with the reference's betas rule.  The optimisers are made at first use, when the parameters are on the device.

    ``trainer(dataloader, isval=False, num_steps=1, return_batch=False)`` is the reference's ``__call__``: ``dataloader`` an iterator of
    batches; returns (losses, images) (``return_batch`` with ``isval``: also the batch)."""

    def __init__(self, model, opts):
        super().__init__()
        self.model = model
        self.opt = opts
        self.use_discriminator = str(_value(opts, "discriminator_losses", "0")) != "0"
        if self.use_discriminator:
            name = str(_value(opts, "discriminator_losses", "pix2pixHD"))
            if name != "pix2pixHD":
                raise NotImplementedError(f"slr_sfs_amd.Trainer: option discriminator_losses={name} is not implemented (only pix2pixHD)")
            self.netD = DiscriminatorLoss(gan_mode=_value(opts, "gan_mode", "hinge"), lambda_feat=float(_value(opts, "lambda_feat", 10.0)),
                                          no_ganFeat_loss=bool(_flag(opts, "no_ganFeat_loss")), ndf=int(_value(opts, "ndf", 64)),
                                          output_nc=int(_value(opts, "output_nc", 3)))
        self.normalize_image = _flag(opts, "normalize_image")
        self._optimizers, self._rows = None, None

    # ---- optimisers (base_model.py:15-46, 80-93)
    @property
    def optimizers(self):
        if self._optimizers is None:
            params, self._rows = [], self._reference_rows()                                       # (learns is read ONCE, here)
            for _, t, learns, _ in self._rows:
                if learns and all(t is not q for q in params):                                    # (a tensor the reference holds in pieces: once)
                    params.append(t)
            listed = {id(t) for t in params}
            left = [n for n, p in self.model.named_parameters() if p.requires_grad and id(p) not in listed]
            if left:
                raise RuntimeError(f"Trainer: parameters outside the reference's order: {left[:4]}")
            self._optimizers = TrainingOptimizers(params, list(self.netD.parameters()) if self.use_discriminator else None, self.opt)
        return self._optimizers

    @property
    def optimizer_G(self):
        return self.optimizers.optimizer_G

    @property
    def optimizer_D(self):
        return self.optimizers.optimizer_D

    def update_learning_rate(self):
        self.optimizers.update_learning_rate()

    def _to_unit(self, images):
        if self.normalize_image:                                                                  # [-1, 1] to [0, 1]
            for k in images.keys():
                if "Img" in k:
                    images[k] = 0.5 * images[k] + 0.5
        return images

    def forward(self, dataloader, isval=False, num_steps=1, return_batch=False):                  # base_model.py:95-163
        weight = 1.0 / float(num_steps)
        if isval:
            batch = next(dataloader)
            t_losses, output_images = self.model(batch)
            self._to_unit(output_images)
            if return_batch:
                return t_losses, output_images, batch
            return t_losses, output_images
        opt = self.optimizers
        opt.optimizer_G.zero_grad()
        if self.use_discriminator:
            all_output_images = []
            for _ in range(num_steps):
                batch = next(dataloader)
                t_losses, output_images = self.model(batch)
                g_losses = self.netD.run_generator_one_step(output_images["PredImg"], output_images["OutputImg"])
                (g_losses["Total Loss"] / weight + t_losses["Total Loss"] / weight).mean().backward()
                all_output_images += [output_images]
            opt.optimizer_G.step()
            opt.optimizer_D.zero_grad()
            for step in range(num_steps):
                d_losses = self.netD.run_discriminator_one_step(all_output_images[step]["PredImg"], all_output_images[step]["OutputImg"])
                (d_losses["Total Loss"] / weight).mean().backward()
            opt.optimizer_D.step()
            g_losses.pop("Total Loss")
            d_losses.pop("Total Loss")
            t_losses.update(g_losses)
            t_losses.update(d_losses)
        else:
            for _ in range(num_steps):
                t_losses, output_images = self.model(next(dataloader))
                (t_losses["Total Loss"] / weight).mean().backward()
            opt.optimizer_G.step()
        self._to_unit(output_images)
        return t_losses, output_images

    # ---- checkpoints in the reference's scheme: state_dict (model.module.*, netD.*), optimizerG, optimizerD
    def reference_state_dict(self):
        sd = self.model.reference_state_dict("model.module.")
        if self.use_discriminator:
            sd.update({"netD." + k: v.detach().clone() for k, v in self.netD.state_dict().items()})
        return sd

    def _reference_rows(self):
        """``model.reference_parameters()`` as (key, tensor, learns, rows): a fourth entry is the slice of ``tensor`` (along dimension 0)
        that the reference holds as a parameter of its own -- the motion network's mlp_gamma / mlp_beta are the halves of one tensor."""
        return [(r[0], r[1], r[2], r[3] if len(r) > 3 else None) for r in self.model.reference_parameters()]

    def _slots(self):
        """[(reference ``optimizerG`` index, index in this optimiser, slice or None)] of the rows that learn, and the reference's
        parameter count.  Once the optimiser exists the rows are those it was made from: a parameter frozen then keeps its index and
        has no state."""
        rows = self._rows if self._optimizers is not None else self._reference_rows()
        own, slots = [], []
        for k, (_, t, learns, sl) in enumerate(rows):
            if learns:
                j = next((j for j, q in enumerate(own) if q is t), None)
                if j is None:
                    j = len(own)
                    own.append(t)
                slots.append((k, j, sl))
        return slots, len(rows)

    def reference_checkpoint(self):
        """{"state_dict", "optimizerG", ["optimizerD"]}: the tensors under the reference's keys and the optimiser states under the
        reference's parameter indices (its ``parameters()`` also lists the frozen VGG19 and the decoder's unused ``conv_b``, which
        have no state)."""
        ckpt = {"state_dict": self.reference_state_dict()}
        own = self.optimizers.state_dict()
        slots, n = self._slots()
        g = own["optimizerG"]
        state = {}
        for ref, j, sl in slots:
            if j in g["state"]:
                st = g["state"][j]
                state[ref] = st if sl is None else dict(st, exp_avg=st["exp_avg"][sl].clone(), exp_avg_sq=st["exp_avg_sq"][sl].clone())
        ckpt["optimizerG"] = {"state": state, "param_groups": [dict(g["param_groups"][0], params=list(range(n)))]}
        if self.use_discriminator:
            ckpt["optimizerD"] = own["optimizerD"]
        return ckpt

    def load_reference_checkpoint(self, ckpt):
        """A checkpoint of the reference (or of ``reference_checkpoint``).  Strict in both directions: every key of ``state_dict`` is
        consumed and every tensor found; the optimiser states are taken where the checkpoint has them (``optimizerG``, and with a
        discriminator ``optimizerD`` with it).  Everything is checked before anything is copied -- keys and shapes of the model and of
        netD, the optimisers' parameter counts, indices and moment shapes: a refused checkpoint leaves the trainer untouched."""
        sd = ckpt["state_dict"]
        known = ("model.module.", "netD.")
        extra = sorted(k for k in sd if not k.startswith(known) or (k.startswith("netD.") and not self.use_discriminator))
        if extra:
            raise KeyError(f"Trainer.load_reference_checkpoint: unexpected keys {extra[:4]} ({len(extra)})")
        self.model.check_reference_state_dict(sd, "model.module.")
        netd = None
        if self.use_discriminator:
            netd = {k[len("netD."):]: v for k, v in sd.items() if k.startswith("netD.")}
            mine = self.netD.state_dict()
            if set(netd) != set(mine):
                raise KeyError(f"Trainer.load_reference_checkpoint: netD: missing {sorted(set(mine) - set(netd))[:4]}, "
                               f"unexpected {sorted(set(netd) - set(mine))[:4]}")
            for k, t in mine.items():
                if tuple(netd[k].shape) != tuple(t.shape):
                    raise ValueError(f"Trainer.load_reference_checkpoint: netD.{k}: shape {tuple(netd[k].shape)}, expected {tuple(t.shape)}")
        own = None
        if "optimizerG" in ckpt:
            slots, n = self._slots()
            rows = self._rows if self._optimizers is not None else self._reference_rows()
            g = ckpt["optimizerG"]
            if len(g["param_groups"]) != 1 or len(g["param_groups"][0]["params"]) != n:
                raise ValueError(f"Trainer.load_reference_checkpoint: optimizerG lists {sum(len(q['params']) for q in g['param_groups'])} parameters "
                                 f"in {len(g['param_groups'])} group(s), the reference's model has {n} in one")
            back = {ref: (j, sl) for ref, j, sl in slots}
            stray = sorted(k for k in g["state"] if k not in back)
            if stray:
                raise ValueError(f"Trainer.load_reference_checkpoint: optimizerG has state for frozen parameters {stray[:4]}")
            self._check_moments("optimizerG", g["state"], {k: rows[k][1] if back[k][1] is None else rows[k][1][back[k][1]] for k in back})
            merged, pieces = {}, {}
            for ref, j, sl in slots:
                if sl is None:
                    if ref in g["state"]:
                        merged[j] = g["state"][ref]
                else:
                    pieces.setdefault(j, []).append((sl.start, ref))
            for j, parts in pieces.items():                                                       # the pieces of one tensor: all or none, one step
                have = [ref for _, ref in sorted(parts) if ref in g["state"]]
                if not have:
                    continue
                if len(have) != len(parts) or any(float(g["state"][r]["step"]) != float(g["state"][have[0]]["step"]) for r in have):
                    raise ValueError(f"Trainer.load_reference_checkpoint: optimizerG states {[r for _, r in sorted(parts)]} are the pieces of one "
                                     f"tensor here: all of them are needed, at one step count")
                merged[j] = dict(g["state"][have[0]], exp_avg=torch.cat([g["state"][r]["exp_avg"] for r in have]),
                                 exp_avg_sq=torch.cat([g["state"][r]["exp_avg_sq"] for r in have]))
            own = {"optimizerG": {"state": merged,
                                  "param_groups": [dict(g["param_groups"][0], params=list(range(1 + max((j for _, j, _ in slots), default=-1))))]}}
            if self.use_discriminator:
                if "optimizerD" not in ckpt:
                    raise KeyError("Trainer.load_reference_checkpoint: optimizerG without optimizerD (this trainer has a discriminator)")
                d, params_d = ckpt["optimizerD"], list(self.netD.parameters())
                if len(d["param_groups"]) != 1 or len(d["param_groups"][0]["params"]) != len(params_d):
                    raise ValueError(f"Trainer.load_reference_checkpoint: optimizerD lists {sum(len(q['params']) for q in d['param_groups'])} "
                                     f"parameters in {len(d['param_groups'])} group(s), netD has {len(params_d)} in one")
                stray = sorted(k for k in d["state"] if not 0 <= k < len(params_d))
                if stray:
                    raise ValueError(f"Trainer.load_reference_checkpoint: optimizerD has state for parameters it does not list {stray[:4]}")
                self._check_moments("optimizerD", d["state"], dict(enumerate(params_d)))
                own["optimizerD"] = d
        self.model.load_reference_state_dict(sd, "model.module.")
        if netd is not None:
            self.netD.load_state_dict(netd, strict=True)
        if own is not None:
            self.optimizers.load_state_dict(own)
        return self

    @staticmethod
    def _check_moments(name, state, params):
        for k, st in state.items():
            for moment in ("exp_avg", "exp_avg_sq"):
                if moment not in st or "step" not in st:
                    raise KeyError(f"Trainer.load_reference_checkpoint: {name} state {k} lacks {moment} / step")
                if tuple(st[moment].shape) != tuple(params[k].shape):
                    raise ValueError(f"Trainer.load_reference_checkpoint: {name} state {k}: {moment} {tuple(st[moment].shape)}, "
                                     f"the parameter is {tuple(params[k].shape)}")
