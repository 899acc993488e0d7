"""Host-side checks of the list-wide spectral weight gradient (no GPU): ABI 21, the plan of ``slr_spectral_weight_grad_multi`` decoded from
the layout include/slr_splat.h documents -- work items, offsets, scratch -- for lists of 1 and 130 tensors over the shapes of the sigma
list, the refusals of the three entry points, and the Python side's refusals and opt-in switch, none of which touches a device.  Then the model
and the trainer: options, keys, the float64 definition of tests/train_step_f64.py pinned to the reference's run, and that definition's
gradients -- autograd against the written-out backward, the pinned gate-clean case of the tight level, and the deliberately wrong
compositions that the criterion must tell from float32 rounding at each level."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_spectral_f64 import SIGMA_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x7F0000100000
ENTRIES = ("slr_spectral_grad_plan_bytes", "slr_spectral_grad_plan_fill", "slr_spectral_weight_grad_multi")


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def _refused(L, rc, *words):
    msg = L.slr_last_error()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def _header():
    return open(os.path.join(ROOT, "include", "slr_splat.h")).read()


def test_entry_points_are_declared_and_abi_is_21(L):
    from slr_sfs_amd import _lib
    hdr = _header()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION >= 21 and L.slr_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION


def _list(n):
    """n tensors cycling through SIGMA_SHAPES, with addresses, offsets and slots that are NOT the running sums (a subset of a forward's
    list, in another order, is a legal list): the filler must copy them, not derive them."""
    rows = np.array([SIGMA_SHAPES[i % len(SIGMA_SHAPES)][0] for i in range(n)], dtype=np.int32)
    cols = np.array([SIGMA_SHAPES[i % len(SIGMA_SHAPES)][1] for i in range(n)], dtype=np.int32)
    addr = np.empty((3, n), dtype=np.uint64)
    for k in range(3):
        addr[k] = P + (k << 36) + 4 * np.arange(n, dtype=np.uint64) * 4099
    u_off = (7 + 3 * np.cumsum(rows[::-1])[::-1]).astype(np.int64)
    v_off = (11 + 5 * np.cumsum(cols[::-1])[::-1]).astype(np.int64)
    slot = ((np.arange(n) * 37) % (2 * n)).astype(np.int32)
    return rows, cols, addr, u_off, v_off, slot


def _fill(L, buffer, need, count, rows_, cols_, addr, u_off_, v_off_, slot_, **kw):
    arg = dict(buf=buffer.ctypes.data, bytes=need, n=count, a0=addr[0].ctypes.data, a1=addr[1].ctypes.data, a2=addr[2].ctypes.data,
               rows=rows_.ctypes.data, cols=cols_.ctypes.data, u_off=u_off_.ctypes.data, v_off=v_off_.ctypes.data, slot=slot_.ctypes.data)
    arg.update(kw)
    return L.slr_spectral_grad_plan_fill(*(arg[k] for k in ("buf", "bytes", "n", "a0", "a1", "a2", "rows", "cols", "u_off", "v_off", "slot")))


@pytest.mark.parametrize("n", [1, 130])
def test_grad_plan_layout_is_the_documented_one(L, n):
    hdr = _header()
    chunk = int(re.search(r"SLR_SPECTRAL_GRAD_CHUNK\s+(\d+)", hdr).group(1))
    al = lambda v, a: (v + a - 1) // a * a                                    # noqa: E731
    for first_shape in range(len(SIGMA_SHAPES) if n == 1 else 1):
        rows, cols, addr, u_off, v_off, slot = _list(n + first_shape)
        rows, cols, addr, u_off, v_off, slot = (a[..., first_shape:] for a in (rows, cols, addr, u_off, v_off, slot))
        rows, cols, u_off, v_off, slot = (np.ascontiguousarray(a) for a in (rows, cols, u_off, v_off, slot))
        addr = np.ascontiguousarray(addr)
        chunks = [-(-int(r) * int(c) // chunk) for r, c in zip(rows, cols)]
        n_work = sum(chunks)
        work_off = al(64 + 64 * n, 16)
        scratch_off = al(work_off + 8 * n_work, 256)
        need = L.slr_spectral_grad_plan_bytes(n, rows.ctypes.data, cols.ctypes.data)
        assert need == scratch_off + al(8 * n_work, 256)
        buf = np.full(need + 64, 0xAB, dtype=np.uint8)
        assert _fill(L, buf, need, n, rows, cols, addr, u_off, v_off, slot) == 0, L.slr_last_error()
        assert (buf[need:] == 0xAB).all(), "written behind the plan"
        assert (buf[scratch_off:need] == 0xAB).all(), "the scratch is the device's: the filler leaves it alone"
        magic, ck, nn_, nw = (int(x) for x in buf[:16].view(np.uint32))
        assert magic == int(re.search(r"SLR_SPECTRAL_GRAD_PLAN_MAGIC\s+0x([0-9a-f]+)u", hdr).group(1), 16) == 0x44475053
        assert (ck, nn_, nw) == (chunk, n, n_work)
        assert [int(x) for x in buf[16:48].view(np.uint64)] == [64, need, work_off, scratch_off] and not buf[48:64].any()
        rec = buf[64:64 + 64 * n]
        r64, r32 = rec.view(np.int64).reshape(n, 8), rec.view(np.int32).reshape(n, 16)
        first = 0
        for t in range(n):
            assert [int(x) for x in r64[t, :3]] == [int(addr[k, t]) for k in range(3)]
            assert list(r32[t, 6:10]) == [rows[t], cols[t], slot[t], chunks[t]]
            assert (int(r64[t, 5]), int(r64[t, 6]), int(r64[t, 7])) == (u_off[t], v_off[t], first)
            first += chunks[t]
        assert not buf[64 + 64 * n:work_off].any()
        work = buf[work_off:work_off + 8 * n_work].view(np.int32).reshape(n_work, 2)
        assert [tuple(int(x) for x in w) for w in work] == [(t, c) for t in range(n) for c in range(chunks[t])]
        assert not buf[work_off + 8 * n_work:scratch_off].any()
        # every tensor's partial sums lie inside the scratch, one double per work item, nobody else's
        assert first == n_work and scratch_off + 8 * n_work <= need


def test_grad_plan_refusals(L):
    n = 9
    rows, cols, addr, u_off, v_off, slot = _list(n)
    need = L.slr_spectral_grad_plan_bytes(n, rows.ctypes.data, cols.ctypes.data)
    buf = np.zeros(need, dtype=np.uint8)
    fill = lambda **kw: _fill(L, buf, need, n, rows, cols, addr, u_off, v_off, slot, **kw)          # noqa: E731
    assert fill() == 0
    assert L.slr_spectral_grad_plan_bytes(0, rows.ctypes.data, cols.ctypes.data) == 0
    assert L.slr_spectral_grad_plan_bytes(-3, rows.ctypes.data, cols.ctypes.data) == 0
    assert L.slr_spectral_grad_plan_bytes(n, None, cols.ctypes.data) == 0 and L.slr_spectral_grad_plan_bytes(n, rows.ctypes.data, None) == 0
    _refused(L, fill(bytes=need - 1), b"slr_spectral_grad_plan_fill", b"bytes")
    _refused(L, fill(n=0), b"slr_spectral_grad_plan_fill", b"n ")
    _refused(L, fill(n=-1), b"slr_spectral_grad_plan_fill", b"n ")
    for k in ("buf", "a0", "a1", "a2", "rows", "cols", "u_off", "v_off", "slot"):
        _refused(L, fill(**{k: None}), b"slr_spectral_grad_plan_fill", b"null")
    for which, value in (("rows", 3073), ("rows", 0), ("cols", 3073), ("cols", -1)):
        bad = (rows if which == "rows" else cols).copy()
        bad[4] = value
        _refused(L, fill(**{which: bad.ctypes.data}), b"slr_spectral_grad_plan_fill", b"rows, cols")
        pair = (bad, cols) if which == "rows" else (rows, bad)
        assert L.slr_spectral_grad_plan_bytes(n, pair[0].ctypes.data, pair[1].ctypes.data) == 0
    edge = rows.copy()
    edge[4] = 3072                                                             # (the limit itself is a legal size)
    assert L.slr_spectral_grad_plan_bytes(n, edge.ctypes.data, cols.ctypes.data) >= need and fill(rows=edge.ctypes.data) == 0
    for k in range(3):
        odd = addr[k].copy()
        odd[2] += 2
        _refused(L, fill(**{f"a{k}": odd.ctypes.data}), b"slr_spectral_grad_plan_fill", b"aligned")
        zero = addr[k].copy()
        zero[n - 1] = 0
        _refused(L, fill(**{f"a{k}": zero.ctypes.data}), b"slr_spectral_grad_plan_fill", b"null tensor")
    for k, a in (("u_off", u_off), ("v_off", v_off), ("slot", slot)):
        neg = a.copy()
        neg[1] = -1
        _refused(L, fill(**{k: neg.ctypes.data}), b"slr_spectral_grad_plan_fill", b"negative")
    same = addr[0].ctypes.data                                                 # out may be dw
    assert fill(a2=same) == 0


def test_device_entry_refuses_bad_arguments_before_anything_is_launched(L):
    f = L.slr_spectral_weight_grad_multi
    _refused(L, f(None, 1, 1, P, P, P, None), b"slr_spectral_weight_grad_multi", b"null")
    for k in range(3):
        args = [P, P, P]
        args[k] = None
        _refused(L, f(P, 1, 1, *args, None), b"slr_spectral_weight_grad_multi", b"null")
    _refused(L, f(P, 0, 1, P, P, P, None), b"slr_spectral_weight_grad_multi", b"n_tensors")
    _refused(L, f(P, 3, 2, P, P, P, None), b"slr_spectral_weight_grad_multi", b"n_work")        # (every tensor has at least one chunk)
    _refused(L, f(P + 8, 1, 1, P, P, P, None), b"slr_spectral_weight_grad_multi", b"aligned")
    _refused(L, f(P, 1, 1, P + 2, P, P, None), b"slr_spectral_weight_grad_multi", b"aligned")


def test_python_side_refuses_before_the_device_is_touched():
    import slr_sfs_amd as S
    w, dw = torch.zeros(4, 6), torch.zeros(4, 6)
    su, sv, inv = torch.zeros(4), torch.zeros(6), torch.zeros(1)
    with pytest.raises(NotImplementedError, match="ROCm device tensors only"):
        S.spectral_weight_grad_multi([dw], [w], su, sv, [(0, 0)], inv)
    with pytest.raises(ValueError, match="one dw"):
        S.spectral_weight_grad_multi([], [], su, sv, [], inv)
    with pytest.raises(ValueError, match="one dw"):
        S.spectral_weight_grad_multi([dw], [w], su, sv, [(0, 0), (0, 0)], inv)
    with pytest.raises(TypeError, match="a tensor is required"):
        S.spectral_weight_grad_multi([dw], [w], None, sv, [(0, 0)], inv)


def test_deferred_gradient_is_opt_in():
    import slr_sfs_amd as S
    from slr_sfs_amd import spectral
    net = S.TrainableDecoderPconv2(cin=8, cout=3, widths=[8, 8, 8, 8, 8, 8, 8], spectral=True)
    keys = list(net.state_dict())
    g = spectral.group_of(net)
    assert g.deferred is False
    assert S.defer_weight_grad(net) is net and g.deferred is True and spectral.group_of(net) is g
    S.defer_weight_grad(net, False)
    assert g.deferred is False
    assert list(net.state_dict()) == keys                                      # the switch is no state: the keys stay
    assert spectral.Normalised(None).weight is None                            # without a group's alias a layer computes with weight_orig


# ------------------------------------------------------------------ the model and the trainer: options, keys, the float64 definition

def _model(opts=None, vgg=True):
    import slr_sfs_amd as S
    import losses_fixture as LF
    import train_step_f64 as T
    v = S.losses.load_vgg19_state_dict(S.losses.VGG19Features(), LF.vgg19_state_dict()) if vgg else None
    return S.TrainingModel(T.options() if opts is None else opts, v, encoder_widths=T.ENC_WIDTHS, decoder_widths=T.DEC_WIDTHS,
                           decoder_updown=T.UPDOWN)


@pytest.mark.parametrize("flag", ["use_softmax_splatter_v2", "use_softmax_splatter_v3", "use_3d_splatter", "use_mesh_splatter", "random_ff_mask",
                                  "train_motion", "use_rgb_features"])
def test_unsupported_flags_raise_naming_the_flag(flag):
    import train_step_f64 as T
    from slr_sfs_amd import training
    assert set(training._UNSUPPORTED) <= {"use_softmax_splatter_v2", "use_softmax_splatter_v3", "use_3d_splatter", "use_mesh_splatter",
                                          "random_ff_mask"}                   # (every one of them is a case here)
    with pytest.raises(NotImplementedError, match=flag):
        _model(T.options(**{flag: True}), vgg=False)
    _model(T.options(**{flag: False}))                                        # (present and off: the reference's `in opt and opt.x`)


@pytest.mark.parametrize("name,value,word", [
    ("refine_model_type", "resnet_256W8UpDown64_skip_warp111_de_resnet_pconv2_nonorm", "skip_warp"),
    ("refine_model_type", "resnet_256W8UpDown64_multires_de_resnet_pconv2_nonorm", "multires"),
    ("refine_model_type", "resnet_256W8UpDown64", "refine_model_type"),
    ("pconv", "pconv_bn", "pconv"), ("norm_G", "batch", "norm_G")])
def test_unsupported_configurations_raise_naming_the_option(name, value, word):
    import train_step_f64 as T
    with pytest.raises(NotImplementedError, match=word):
        _model(T.options(**{name: value}), vgg=False)


def test_other_refusals_of_model_and_trainer():
    import slr_sfs_amd as S
    import train_step_f64 as T
    with pytest.raises(NotImplementedError, match="style"):
        _model(T.options(losses=["1.0_l1", "10.0_style"]))
    with pytest.raises(ValueError, match="VGG19Features"):
        _model(vgg=False)                                                     # the content loss needs its network
    m = _model()
    with pytest.raises(NotImplementedError, match="discriminator_losses"):
        S.Trainer(m, T.options(discriminator_losses="pix2pix"))
    assert not S.Trainer(m, T.options(discriminator_losses="0")).use_discriminator
    g = T.load()
    batch = {"images": [torch.from_numpy(g["images"][k]) for k in range(3)], "motions": torch.from_numpy(g["motions"]),
             "index": torch.from_numpy(g["index"])}
    with pytest.raises(NotImplementedError, match="ROCm device tensors only"):
        m(batch)                                                              # CPU tensors: no CPU path, nothing was run
    assert m.relu_z is False and _model(T.options(Z_model="encoder_relu")).relu_z is True


def _reference_keys(g):
    """The reference's BaseModel(model).state_dict() keys with shapes; training wraps ``model`` in DataParallel, which makes its
    ``model.`` keys ``model.module.`` (SURVEY, "State-dict key scheme")."""
    keys = [("model.module." + k[len("model."):]) if k.startswith("model.") else k for k in g["state_keys"]]
    return {k: tuple(int(x) for x in s if x >= 0) for k, s in zip(keys, g["state_shapes"])}


def test_checkpoint_key_set_is_the_references():
    import slr_sfs_amd as S
    import train_step_f64 as T
    g = T.load()
    ref = _reference_keys(g)
    trainer = S.Trainer(_model(), T.options())
    sd = trainer.reference_state_dict()
    assert sorted(sd) == sorted(ref)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert sum(k.startswith("netD.") for k in sd) > 0 and sum("loss_function" in k for k in sd) == 26
    # the parameter order of the reference's optimizerG, frozen ones included
    order = ["model.module." + k for k in g["parameter_order"]]
    mine = trainer.model.reference_parameters()
    assert [("model.module." + k) for k, _, _ in mine] == order
    learns = {("model.module." + k): bool(v) for k, v in zip(g["parameter_order"], g["parameter_learns"])}
    for k, t, l in mine:
        assert sd["model.module." + k].shape == t.shape
        if not l:                                        # frozen there, or (the decoder's unused conv_b) never given a gradient
            assert not learns["model.module." + k] or k.endswith("conv_b.weight_orig"), k
        else:
            assert learns["model.module." + k] and t.requires_grad, k
    assert [("netD." + k) for k, _ in trainer.netD.named_parameters()] == ["netD." + k for k in g["netD_parameter_order"]]


def test_state_dict_round_trip_is_the_identity_and_strict():
    import slr_sfs_amd as S
    import train_step_f64 as T
    g = T.load()
    trainer = S.Trainer(_model(), T.options())
    first = T.state_dict(g)
    first.update({k: v for k, v in trainer.reference_state_dict().items() if k.startswith("netD.")})
    first = {k: (v + 0.25 if k.startswith("netD.") and v.is_floating_point() else v) for k, v in first.items()}
    trainer.load_reference_checkpoint({"state_dict": first})
    back = trainer.reference_state_dict()
    assert sorted(back) == sorted(first) and all(torch.equal(back[k], first[k]) for k in first)
    assert not any(k.endswith("weight") and "encoder" in k for k in back)      # unfolded: weight_orig, u and v, no folded weight
    missing = dict(first)
    gone = next(k for k in missing if k.endswith("conv_b.weight_u"))
    del missing[gone]
    with pytest.raises(KeyError, match="missing"):
        trainer.load_reference_checkpoint({"state_dict": missing})
    for extra in ("model.module.encoder.gblocks.0.ch_a.2.weight", "netD.netD.netD.discriminator_2.model0.0.weight", "epoch_state"):
        with pytest.raises(KeyError, match="unexpected"):
            trainer.load_reference_checkpoint({"state_dict": dict(first, **{extra: torch.zeros(1)})})
    wrong = dict(first)
    wrong["model.module.max_z"] = torch.zeros(2)
    with pytest.raises(ValueError, match="shape"):
        trainer.load_reference_checkpoint({"state_dict": wrong})
    bad_d = dict(first)
    k_d = next(k for k in bad_d if k.startswith("netD.") and bad_d[k].dim() == 4)
    bad_d[k_d] = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError, match="netD"):
        trainer.load_reference_checkpoint({"state_dict": bad_d})
    # the optimiser entries are checked before the first copy, too
    other = {k: v + 1.0 if v.is_floating_point() else v for k, v in first.items()}
    n = len(trainer.model.reference_parameters())
    group = dict(lr=5e-4, betas=(0.0, 0.9), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False)
    ok_g = {"state": {}, "param_groups": [dict(group, params=list(range(n)))]}
    ok_d = {"state": {}, "param_groups": [dict(group, params=list(range(len(list(trainer.netD.parameters())))))]}
    frozen = next(k for k, (_, _, learns) in enumerate(trainer.model.reference_parameters()) if not learns)
    moments = lambda shape: {"step": torch.zeros(()), "exp_avg": torch.zeros(shape), "exp_avg_sq": torch.zeros(shape)}          # noqa: E731
    for what, ckpt, err in (("count", {"optimizerG": dict(ok_g, param_groups=[dict(group, params=list(range(n - 1)))]), "optimizerD": ok_d}, ValueError),
                            ("frozen", {"optimizerG": dict(ok_g, state={frozen: moments((1,))}), "optimizerD": ok_d}, ValueError),
                            ("moment shape", {"optimizerG": dict(ok_g, state={0: moments((3, 3))}), "optimizerD": ok_d}, ValueError),
                            ("no optimizerD", {"optimizerG": ok_g}, KeyError),
                            ("optimizerD count", {"optimizerG": ok_g, "optimizerD": dict(ok_d, param_groups=[dict(group, params=[0])])}, ValueError)):
        with pytest.raises(err):
            trainer.load_reference_checkpoint(dict(ckpt, state_dict=other))
    after = trainer.reference_state_dict()
    assert all(torch.equal(after[k], first[k]) for k in first), "a refused checkpoint leaves the trainer untouched"
    assert trainer._optimizers is None                                         # (nothing was even built)


def test_float64_definition_is_pinned_to_the_reference():
    """Every value the reference's own float32 forward recorded against the definition of tests/train_step_f64.py in float64:
    E(reference float32, def64) <= 10 E(def32, def64) + 1e-6, the project's criterion with the reference's float32 run in the device's
    place.  Every loss entry, PSNR and ssim included, is compared as it is (relative error of the scalar): none needed another quantity."""
    import conv_train_f64 as C64
    import train_step_f64 as T
    g = T.load()
    assert list(g["loss_keys"]) == ["L1", "Perceptual", "Total Loss", "psnr", "ssim"]
    assert list(g["pred_keys"]) == ["GTMotion", "OutputImg", "PredImg", "Z_f"]
    assert len({tuple(r[1:] - r[:-1]) for r in g["index"]}) == 2              # two different time pairs
    r64, r32 = T.forward(g, torch.float64), T.forward(g, torch.float32)
    rows = [("loss " + k, torch.from_numpy(np.asarray(g["loss/" + k])).reshape(1), r64["loss"][k].reshape(1), r32["loss"][k].reshape(1))
            for k in g["loss_keys"]]
    rows += [(k, torch.from_numpy(g[k]), r64[k], r32[k]) for k in ("PredImg", "Z_f")]
    for name, ref, d64, d32 in rows:
        e_ref, e_def = C64.E(ref.double(), d64), C64.E(d32.double(), d64)
        print(f"{name}: E(reference32, def64) {e_ref:.3e}  E(def32, def64) {e_def:.3e}  bound {10 * e_def + 1e-6:.3e}")
        assert e_ref <= 10 * e_def + 1e-6, name


# ------------------------------------------------------------------ the float64 definition of the iteration's gradients

@functools.lru_cache(maxsize=None)
def _g():
    import train_step_f64 as T
    return T.load()


@functools.lru_cache(maxsize=None)
def _tight(train_z=True, n=1, mutant=None, dtype=torch.float64):
    import train_step_f64 as T
    inputs, gpred = T.clean_batches(_g(), train_z, n)
    return T.chain_gradients(inputs, gpred, dtype, T.options(W=8, train_Z=train_z), (mutant,) if mutant else (), _g())


def _disc_state(seed):
    """The discriminator's initialisation as tests/test_gpu_train_step.py::_trainer makes it, under disc_f64's keys."""
    import slr_sfs_amd as S
    import train_step_f64 as T
    torch.manual_seed(seed)
    d = S.DiscriminatorLoss(gan_mode="hinge", lambda_feat=10.0, no_ganFeat_loss=False, ndf=T.NDF, output_nc=3)
    return {k[len("netD.netD."):]: v.detach().clone() for k, v in d.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _loose(use_d=True, n=1, mutant=None, dtype=torch.float64):
    import train_step_f64 as T
    one = T.fixture_inputs(_g())
    return T.iteration_gradients([one, T.second_batch(one)][:n], _disc_state(T.DISC_SEED) if use_d else None, dtype, use_d,
                                 mutants=(mutant,) if mutant else (), g=_g())


def _outside(figs):
    """(tensors outside their bound, the largest e / bound) of train_step_f64.figures' result."""
    over = [e / b for e, _, b in figs.values()]
    return sum(r > 1.0 for r in over), max(over)


def test_autograd_is_the_written_out_gradient():
    """The leaves' gradients that autograd gives the differentiable definition are ``spectral_f64.network_grads``' -- the written-out
    backward every piece is tested against -- fed with autograd's own gradient at that network's output: the decoder, and the encoder
    as the sum of its two calls (each with the u, v and sigma of ITS forward), in float64 to 1e-12 of the largest element.  The 16
    cancelling biases are held against the magnitude of their terms, as everywhere."""
    import block_train_f64 as B64
    import conv_train_f64 as C64
    import spectral_f64 as S64
    import train_step_f64 as T
    (inp,), (gpred,) = T.clean_batches(_g())
    net = T.generator(_g(), torch.float64)
    f = T.generator_forward(net, inp, torch.float64, T.options(W=8))
    outs = [call[0][-1]["y"] for call in f["encoder_calls"]] + [f["decoder"][0][-1]["y"]]
    for y in outs:
        y.retain_grad()
    f["PredImg"].backward(gpred.double())
    assert all(y.grad is not None and bool(y.grad.abs().max() > 0) for y in outs)
    written = {}
    with torch.no_grad():
        runs = [("encoder.gblocks", T.ENC_FORMS, T.ENC_NAMES, net["enc"], [None] * 8, call, y.grad) for call, y in zip(f["encoder_calls"], outs)]
        runs.append(("projector.eblocks", T.DEC_FORMS, T.DEC_NAMES, net["dec"], T.UPDOWN, f["decoder"], outs[2].grad))
        for head, forms, names, ps, kinds, (fs, uns, ctxs, noise), gy in runs:
            ds = S64.network_grads(forms, fs, ps, uns, kinds, noise, gy, ctxs)
            for i, d in enumerate(ds):
                for name, key in names.items():
                    if ps[i].get(name) is None:
                        continue
                    rows = [(f"{head}.{i}.{key}.weight_orig", d["d_" + name], None)]
                    b = T.BIASES.get(name)
                    if b is not None and ps[i].get(b) is not None:
                        rows.append((f"{head}.{i}.{key}.bias", d["d" + b], d["db_aa_terms"].max() if b == "b_aa" else None))
                    for k, t, terms in rows:
                        old = written.get(k, (0.0, None))
                        written[k] = (old[0] + t, terms if old[1] is None else old[1] + terms)
    assert sorted(written) == sorted(net["leaves"]) and len(written) == 141
    worst = 0.0
    for k, (t, terms) in written.items():
        e = C64.E(net["leaves"][k].grad, t) if terms is None else B64.E_terms(net["leaves"][k].grad, t, terms)
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print(f"autograd against the written-out gradient: {len(written)} leaves, largest E {worst:.3e}")


def test_the_gate_clean_case_is_pinned():
    """The small case of the tight level (train_step_f64.clean_case) at its pinned seeds: the margins, that the first seed IS the first,
    that the Euler integration gives float32 and float64 the same flows, and that the case exercises what it is there for -- pixels
    leaving the frame in both directions and holes in the blended features, so that the per-element mask of the decoder's first block
    has something to do."""
    import train_step_f64 as T
    assert T.CLEAN_SEEDS[True][0] == 14 and T.MARGIN == 1e-4
    assert T.first_clean_seed(_g(), T.options(W=8), limit=T.CLEAN_SEEDS[True][0] + 1)[0] == T.CLEAN_SEEDS[True][0]
    off = T.options(W=8, train_Z=False)                  # train_Z off: both seeds are the first of their searches, below the limit of 200
    assert T.CLEAN_SEEDS[False] == (52, 82) and max(T.CLEAN_SEEDS[False]) < 200
    assert T.first_clean_seed(_g(), off, limit=53)[0] == 52
    assert T.first_clean_seed(_g(), off, before=(T.clean_case(_g(), 52)[0],), limit=83)[0] == 82
    for train_z in (True, False):
        r64, r32 = _tight(train_z, 2), _tight(train_z, 2, None, torch.float32)
        for n, pre in enumerate(r64["pre"]):
            m = T.margin(pre)
            print(f"train_Z {train_z} batch {n} seed {T.CLEAN_SEEDS[train_z][n]}: margin {m:.4e} over {len(pre)} batch-norm evaluations, "
                  f"{r64['holes'][n]} zeros in gen_fs")
            assert len(pre) == 48 and m > T.MARGIN
            assert r64["holes"][n] > 0
            for d in range(2):
                flow = r64["flows"][n][d]
                assert torch.equal(flow.float(), r32["flows"][n][d]) and torch.equal(flow.float().double(), flow)
                gone = flow[:, 0] == 9.0                                      # max(H, W) + 1: the pixel left the frame
                assert bool(gone.any()) and not bool(gone.all())
    assert _tight(True, 1)["margin"] == T.margin(_tight(True, 2)["pre"][0])   # (the first batch of two is the single batch)


TIGHT_MUTANTS = (("end_dropped", 1), ("through_power", 1), ("first_uv", 1), ("overwrite", 2))
LOOSE_MUTANTS = (("end_dropped", 1), ("through_power", 1), ("no_gan", 1), ("no_weight", 2), ("stale_d_uv", 1))
LOOSE_MEASURED_ONLY = (("first_uv", 1), ("overwrite", 2))
LOOSE_MUTANTS_WITHOUT_D = (("no_weight", 2), ("overwrite", 2))               # the accumulation of the trainer's branch without a discriminator


def test_the_tight_criterion_separates_mutants_from_rounding():
    """At the 8 x 8 case every wrong composition of train_step_f64.MUTANTS' first four leaves 10 E_plain32 + 1e-6 on at least one
    tensor; the definition's own float32 run, by construction, on none."""
    import train_step_f64 as T
    for mutant, n in TIGHT_MUTANTS:
        r64, r32, bad = _tight(True, n), _tight(True, n, None, torch.float32), _tight(True, n, mutant)
        figs = T.figures(bad["grads"], r64["grads"], r32["grads"])
        count, ratio = _outside(figs)
        print(f"tight, {mutant} ({n} batch): {count} of {len(figs)} tensors outside the bound, by up to {ratio:.1f} x")
        assert len(figs) == 141 and count >= 1, mutant
    plain = [e for e, _, _ in T.figures(r32["grads"], r64["grads"], r32["grads"]).values()]
    print(f"tight: E_plain32 {min(plain):.3e} .. {max(plain):.3e}")


def test_the_loose_level_stays_meaningful_and_separates_its_mutants():
    """At the fixture shape through L1 + VGG and the discriminator: E_plain32 <= 0.03 on every compared tensor (no bound above 0.3) in
    the four cases the device test runs, and every mutant of the lists out of bound on at least one tensor."""
    import train_step_f64 as T
    assert T.SECOND_OFFSETS == (2, 4)
    for use_d, n in ((True, 1), (False, 1), (True, 2), (False, 2)):
        r64, r32 = _loose(use_d, n), _loose(use_d, n, None, torch.float32)
        figs = T.figures(r32["grads_G"], r64["grads_G"], r32["grads_G"])
        if use_d:
            figs.update(T.figures(r32["grads_D"], r64["grads_D"], r32["grads_D"], T.final_bias_terms(r64["grads_D"], n)))
        plain = sorted(e for e, _, _ in figs.values())
        print(f"loose, D {use_d}, {n} batch: E_plain32 {plain[0]:.3e} .. median {plain[len(plain) // 2]:.3e} .. {plain[-1]:.3e} "
              f"over {len(figs)} tensors")
        assert len(figs) == 141 + (14 if use_d else 0) and plain[-1] <= 0.03, (use_d, n, plain[-1])
    for mutant, n in LOOSE_MUTANTS + LOOSE_MEASURED_ONLY:
        r64, r32, bad = _loose(True, n), _loose(True, n, None, torch.float32), _loose(True, n, mutant)
        figs_g = T.figures(bad["grads_G"], r64["grads_G"], r32["grads_G"])
        figs_d = T.figures(bad["grads_D"], r64["grads_D"], r32["grads_D"], T.final_bias_terms(r64["grads_D"], n))
        (cg, rg), (cd, rd) = _outside(figs_g), _outside(figs_d)
        print(f"loose, {mutant} ({n} batch): generator {cg} of {len(figs_g)} outside the bound, by up to {rg:.1f} x; "
              f"discriminator {cd} of {len(figs_d)}, by up to {rd:.1f} x")
        if (mutant, n) in LOOSE_MUTANTS:
            assert cg + cd >= 1, mutant
    for mutant, n in LOOSE_MUTANTS_WITHOUT_D:
        r64, r32, bad = _loose(False, n), _loose(False, n, None, torch.float32), _loose(False, n, mutant)
        count, ratio = _outside(T.figures(bad["grads_G"], r64["grads_G"], r32["grads_G"]))
        print(f"loose without the discriminator, {mutant} ({n} batch): generator {count} of 141 outside the bound, by up to {ratio:.1f} x")
        assert count >= 1, mutant
