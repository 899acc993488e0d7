"""The size limits of the launching entry points, probed on the host ("Size limits of the entry points"): for every limit an
entry point documents, the smallest size past it -- or the nearest one its factors can form -- must be refused with SLR_E_BADARG before
anything touches a device, and the message must name the entry point.

Every call here passes sizes that no buffer backs (the pointers are a dummy 16-byte aligned integer), and every call is EXPECTED TO BE
REFUSED.  On a machine without a device a probe that is wrongly accepted reaches the launch and comes back with HIP's "no device"
error: the test fails cleanly.  On a machine with a device it would launch on the dummy pointer -- so the module skips there."""
import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("the probes pass sizes that no buffer backs and a dummy pointer: a probe the library wrongly accepts would launch on it, "
                "so they run only where torch.cuda.is_available() is false (there it fails cleanly with HIP's no-device error)",
                allow_module_level=True)

P = 0x10000                                                # a 16-byte aligned non-null "pointer"
IN_B8, OUT_B8, SKIP_B8, POOL_OUT, UP_OUT = 1, 2, 32, 64, 128


@pytest.fixture(scope="module")
def L():
    import os
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


# entry point -> (arguments in the header's order without the stream: a string names a size of the probe, anything else is passed as it
#                 is; the sizes of a call every check accepts).  A probe changes some of the sizes.
SMALL = dict(N=1, C=8, Cin=8, Cout=8, H=8, W=8, b8=0, layout=0, k=0, Ca=2, Cb=2, B=1, steps=1, mc=1, skip_cin=8, ws_bytes=1 << 40)
OWN = {"slr_conv1x1_small": dict(Cout=3), "slr_pconv3x3_forward_tail": dict(Cin=128, Cout=128)}      # what an entry point needs to differ
CONV3 = ["N", "Cin", "Cout", "H", "W"]
ENTRY = {
    # ---- the memory-bound stages of the decoder (csrc/resample.hip, csrc/pconv.hip)
    "slr_conv1x1_small": [P, P, P, P, "N", "Cin", "Cout", "H", "W", "b8"],
    "slr_avgpool3x3s2": [P, P, "N", "C", "H", "W", "b8"],
    "slr_upsample_bilinear2x": [P, P, "N", "C", "H", "W", "b8"],
    "slr_bn_relu_mask": [P, P, P, P, "mc", P, "N", "C", "H", "W"],
    "slr_pconv_epilogue": [P, P, P, 1.0, None, None, None, P, None, 72.0, "N", "C", "H", "W"],
    # ---- the convolutions (csrc/conv.hip)
    "slr_conv3x3_forward": [P, P, None, None, P, *CONV3, 1.0, 64.0, None, None, "layout"],
    "slr_pconv3x3_forward": [P, None, None, P, P, 1.0, 64.0, P, None, None, None, P, None, *CONV3, "layout"],
    "slr_conv3x3_forward_skip": [P, P, None, P, *CONV3, 1.0, 64.0, None, None, P, P, None, "skip_cin", 1.0, P, "ws_bytes", "layout"],
    "slr_pconv3x3_forward_skip": [P, None, None, P, P, 1.0, 64.0, P, P, None, *CONV3, P, P, "skip_cin", 1.0, P, "ws_bytes", "layout"],
    "slr_conv3x3_forward_skipout": [P, P, None, None, P, *CONV3, 1.0, 64.0, None, None, P, None, P, "layout"],
    "slr_pconv3x3_forward_skipout": [P, None, None, P, P, 1.0, 64.0, P, None, None, None, P, None, *CONV3, P, P, "layout"],
    "slr_pconv3x3_forward_tail": [P, P, P, 1.0, 64.0, P, None, P, P, P, P, None, *CONV3],
    "slr_narrow_gather": [P, P, P, None, None, None, P, P, P, "N", "Cin", "H", "W", 1.0, 1.0, 64.0],
    "slr_conv1x1_forward": [P, P, None, P, *CONV3, 1.0, 64.0, "layout"],
    "slr_conv3x3_split_weights": [P, P, "Cout", "Cin", 1.0],
    "slr_conv3x3_f32_weights": [P, P, "Cout", "Cin"],
    "slr_conv3x3_wino_weights": [P, P, "Cout", "Cin"],
    "slr_conv1x1_split_weights": [P, P, "Cout", "Cin", 1.0],
    "slr_conv1x1_f32_weights": [P, P, "Cout", "Cin"],
    # ---- the motion U-Nets (csrc/motion.hip, csrc/motion_grad.hip, csrc/conv4x4.hip)
    "slr_resize_segmap": [P, P, "N", "C", "H", "W", "k", -1],
    "slr_upsample2x_concat": [P, "Ca", P, "Cb", P, "N", "H", "W", -1, 0],
    "slr_upsample2x_concat_backward": [P, None, None, "Ca", None, "Cb", P, P, "N", "H", "W", -1, 0],
    "slr_instnorm_spade": [P, P, P, "N", "C", "H", "W", 1e-5],
    "slr_instnorm_spade_train_forward": [P, P, P, P, P, "N", "C", "H", "W", 1e-5],
    "slr_instnorm_spade_backward": [P, P, P, P, P, P, P, "N", "C", "H", "W"],
    "slr_conv4x4s2_forward": [P, P, None, None, None, P, *CONV3, 0, 0.2],
    "slr_conv4x4s2_backward_data": [P, None, P, P, *CONV3, 0.2],
    "slr_motion_loss": [P, P, P, "N", "H", "W", P, "ws_bytes"],
    "slr_motion_loss_grad": [P, P, None, None, P, "N", "H", "W"],
    # ---- the Euler integration (csrc/euler.hip)
    "slr_euler_integrate": [P, "H", "W", "steps", 1.0, P, None],
    "slr_euler_integrate_all": [P, "H", "W", "steps", 1.0, P, None],
    "slr_euler_backward": [P, "H", "W", "steps", 1.0, P, P],
    "slr_euler_integrate_batch": [P, P, "B", "H", "W", 1.0, P, None],
    "slr_euler_backward_batch": [P, P, "B", "H", "W", 1.0, P, P],
    "slr_euler_pair_forward": [P, P, P, "B", "H", "W", P, P, None, None],
    "slr_euler_pair_backward": [P, P, P, "B", "H", "W", P, P, P, P, "ws_bytes"],
    # ---- the clip metrics (csrc/metrics.hip, csrc/lpips.hip)
    "slr_ssim_mse": [P, P, 0, None, P, "N", "C", "H", "W", 11, P, "ws_bytes"],
    "slr_vgg_prep": [P, 0, 1, P, "N", "H", "W"],
    "slr_lpips_prep": [P, 0, 1, P, "N", "H", "W"],
    "slr_feature_cos_distance": [P, P, P, "N", "C", "H", "W", P, "ws_bytes"],
    "slr_lpips_distance": [P, P, P, P, "N", "C", "H", "W", P, "ws_bytes"],
    # ---- the training kernels: they refuse N * C * H * W >= 2^31 - 1024 outright (csrc/conv_grad.hip, csrc/block_grad.hip, csrc/decoder_grad.hip)
    "slr_conv3x3_weight_grad": [P, P, P, None, *CONV3, 0, 0, P, "ws_bytes"],
    "slr_conv_grad_scale_bias": [P, P, None, P, None, "N", "C", "H", "W", 0, P, "ws_bytes"],
    "slr_conv1x1_weight_grad": [P, P, P, *CONV3, 0, 0, P, "ws_bytes"],
    "slr_bn_batch_stats": [P, None, 1e-5, P, P, P, "N", "C", "H", "W", "b8", P, "ws_bytes"],
    "slr_bn_relu_mask_train": [P, P, P, None, P, "N", "C", "H", "W", "b8"],
    "slr_pconv_train_epilogue": [P, P, P, P, None, P, "N", "C", "H", "W", "b8"],
    "slr_avgpool3x3s2_backward": [P, P, "N", "C", "H", "W", "b8"],
    "slr_upsample_bilinear2x_backward": [P, P, "N", "C", "H", "W", "b8"],
}

M31 = 1 << 31
# (entry point, what is probed, the sizes that differ from SMALL).  A product limit is reached with the smallest factors that form it:
# 2^31 - 256 = 256 * (2^23 - 1), 2^31 - 2^18 = 8191 * 2^18, 2^29 - 64 = 64 * (2^23 - 1), 2^31 - 1024 = 1024 * (2^21 - 1), 2^31 - 128 = 128 * (2^24 - 1).
PROBES = [
    # the five holes this table was written for, at the sizes they were found with (H * W, 4 * H * W or the grid round-up past an int)
    ("slr_conv1x1_small", "H*W = 2^31 + 65536", dict(H=65536, W=32769)),
    ("slr_conv1x1_small", "H*W = 2^31 - 1", dict(H=1, W=M31 - 1, b8=1)),
    ("slr_bn_relu_mask", "H*W = 2^31 + 65536", dict(H=65536, W=32769)),
    ("slr_bn_relu_mask", "H*W = 2^31 - 1", dict(H=1, W=M31 - 1)),
    ("slr_pconv_epilogue", "H*W = 2^31 + 65536", dict(H=65536, W=32769)),
    ("slr_pconv_epilogue", "H*W = 2^31 - 1", dict(H=1, W=M31 - 1)),
    ("slr_upsample2x_concat", "4*H*W = 2^31 - 4", dict(H=1, W=536870911)),
    ("slr_resize_segmap", "H*W = 2^31 - 1", dict(H=1, W=M31 - 1)),
    # ---- every limit, at the smallest size past it
    ("slr_conv1x1_small", "H*W = 2^31 - 256", dict(H=256, W=8388607)),
    ("slr_conv1x1_small", "H*W = 2^31 - 256, channel-blocked", dict(H=256, W=8388607, b8=1)),
    ("slr_conv1x1_small", "N = 65536", dict(N=65536)),
    ("slr_conv1x1_small", "Cout*Cin = 2^31", dict(Cout=4, Cin=1 << 29)),
    ("slr_avgpool3x3s2", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_avgpool3x3s2", "N*C = 65536", dict(N=8192)),
    ("slr_upsample_bilinear2x", "H*W = 2^28", dict(H=16384, W=16384)),
    ("slr_upsample_bilinear2x", "N*C = 65536", dict(N=8192, b8=1)),
    ("slr_bn_relu_mask", "H*W = 2^31 - 2^18", dict(H=8191, W=262144)),
    ("slr_bn_relu_mask", "H*W = 2^31 - 2^18, no mask", dict(H=8191, W=262144, mc=-1)),
    ("slr_bn_relu_mask", "N = 65536", dict(N=65536)),
    ("slr_bn_relu_mask", "C = 65536", dict(C=65536, mc=0)),
    ("slr_pconv_epilogue", "H*W = 2^31 - 2^18", dict(H=8191, W=262144)),
    ("slr_pconv_epilogue", "N = 65536", dict(N=65536)),
    ("slr_pconv_epilogue", "C = 65536", dict(C=65536)),
    ("slr_conv3x3_forward", "N = 65536", dict(N=65536)),
    ("slr_conv3x3_forward", "Cout = 2^20", dict(Cout=1 << 20)),
    ("slr_conv3x3_forward", "Cin*H*W = 2^31", dict(Cin=128, H=4096, W=4096)),
    ("slr_conv3x3_forward", "H*W = 2^31 - 1024", dict(Cin=1, H=1024, W=2097151)),
    ("slr_conv3x3_forward", "N*Cout*H*W = 2^40", dict(N=1024, Cin=1, Cout=1024, H=1024, W=1024)),
    ("slr_conv3x3_forward", "Cin*H*W = 2^31, channel-blocked", dict(Cin=128, Cout=128, H=4096, W=4096, layout=IN_B8 | OUT_B8)),
    ("slr_pconv3x3_forward", "Cin*H*W = 2^31", dict(Cin=128, H=4096, W=4096)),
    ("slr_pconv3x3_forward", "N = 65536", dict(N=65536)),
    ("slr_conv3x3_forward_skip", "Cin*H*W = 2^31", dict(Cin=128, Cout=128, H=4096, W=4096, layout=IN_B8 | OUT_B8 | SKIP_B8)),
    ("slr_conv3x3_forward_skip", "skip_cin*H*W = 2^31", dict(Cin=8, Cout=128, H=4096, W=4096, skip_cin=128, layout=IN_B8 | OUT_B8 | SKIP_B8)),
    ("slr_conv3x3_forward_skip", "pooled: N*Cout/8 = 65536", dict(N=4096, Cout=128, layout=IN_B8 | OUT_B8 | SKIP_B8 | POOL_OUT)),
    ("slr_conv3x3_forward_skip", "up-sampled: N*Cout/8 = 65536", dict(N=4096, Cout=128, layout=IN_B8 | OUT_B8 | SKIP_B8 | UP_OUT)),
    ("slr_conv3x3_forward_skip", "up-sampled: N*Cout*H*W = 2^38", dict(N=2048, Cout=128, H=1024, W=1024, layout=IN_B8 | OUT_B8 | SKIP_B8 | UP_OUT)),
    ("slr_pconv3x3_forward_skip", "Cin*H*W = 2^31", dict(Cin=128, Cout=128, H=4096, W=4096, layout=IN_B8 | OUT_B8 | SKIP_B8)),
    ("slr_pconv3x3_forward_skip", "pooled: N*Cout/8 = 65536", dict(N=4096, Cout=128, layout=IN_B8 | OUT_B8 | SKIP_B8 | POOL_OUT)),
    ("slr_conv3x3_forward_skipout", "Cin*H*W = 2^31", dict(Cin=128, Cout=3, H=4096, W=4096, layout=IN_B8)),
    ("slr_pconv3x3_forward_skipout", "Cin*H*W = 2^31", dict(Cin=128, Cout=3, H=4096, W=4096, layout=IN_B8)),
    ("slr_pconv3x3_forward_tail", "Cin*H*W = 2^31", dict(H=4096, W=4096)),
    ("slr_pconv3x3_forward_tail", "N = 65536", dict(N=65536)),
    ("slr_narrow_gather", "H*W = 2^31 - 64", dict(H=64, W=33554431)),
    ("slr_narrow_gather", "ceil(H/4) = 65536", dict(H=262141, W=1)),
    ("slr_narrow_gather", "N = 65536", dict(N=65536)),
    ("slr_conv1x1_forward", "H*W = 2^31 - 128", dict(H=128, W=16777215)),
    ("slr_conv1x1_forward", "Cin*H*W = 2^40", dict(Cin=1024, H=32768, W=32768)),
    ("slr_conv1x1_forward", "N = 65536", dict(N=65536)),
    ("slr_conv1x1_forward", "Cout = 2^20", dict(Cout=1 << 20)),
    ("slr_conv3x3_split_weights", "padded Cout*Cin*9 = 2^30 * 9/8", dict(Cout=8192, Cin=16384)),
    ("slr_conv3x3_f32_weights", "padded Cout*Cin*9 = 2^30 * 9/8", dict(Cout=8192, Cin=16384)),
    ("slr_conv3x3_wino_weights", "padded Cout*Cin*16 = 2^30", dict(Cout=8192, Cin=8192)),
    ("slr_conv1x1_split_weights", "padded Cout*Cin = 2^30", dict(Cout=32768, Cin=32768)),
    ("slr_conv1x1_f32_weights", "padded Cout*Cin = 2^30", dict(Cout=32768, Cin=32768)),
    ("slr_resize_segmap", "H*W = 2^31 - 256", dict(H=256, W=8388607)),
    ("slr_resize_segmap", "N*C = 65536", dict(N=8192)),
    ("slr_resize_segmap", "k = 16", dict(k=16, H=65536, W=65536)),
    ("slr_upsample2x_concat", "4*H*W = 2^31 - 256", dict(H=64, W=8388607)),
    ("slr_upsample2x_concat", "N*(Ca+Cb) = 65536", dict(N=16384)),
    ("slr_upsample2x_concat_backward", "4*H*W = 2^31", dict(H=16384, W=32768)),
    ("slr_upsample2x_concat_backward", "N*(Ca+Cb) = 65536", dict(N=16384)),
    ("slr_instnorm_spade", "H*W = 2^31 - 1024", dict(H=1024, W=2097151)),
    ("slr_instnorm_spade", "N*C = 2^31", dict(N=1 << 28)),
    ("slr_instnorm_spade_train_forward", "H*W = 2^31 - 1024", dict(H=1024, W=2097151)),
    ("slr_instnorm_spade_backward", "H*W = 2^31 - 256", dict(H=256, W=8388607)),
    ("slr_conv4x4s2_forward", "H*W = 2^31", dict(H=65536, W=32768)),
    ("slr_conv4x4s2_forward", "N = 65536", dict(N=65536)),
    ("slr_conv4x4s2_forward", "Cin = 65536", dict(Cin=65536)),
    ("slr_conv4x4s2_backward_data", "N*H*W = 2^31", dict(N=2048, H=1024, W=1024)),
    ("slr_conv4x4s2_backward_data", "H = 2^20", dict(H=1 << 20, W=2)),
    ("slr_motion_loss", "ceil(H*W/4096) = 65536", dict(H=1, W=65535 * 4096 + 1)),
    ("slr_motion_loss", "N = 65536", dict(N=65536)),
    ("slr_motion_loss_grad", "ceil(H*W/4096) = 65536", dict(H=1, W=65535 * 4096 + 1)),
    ("slr_motion_loss_grad", "N = 65536", dict(N=65536)),
    ("slr_euler_integrate", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_integrate_all", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_backward", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_integrate_batch", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_integrate_batch", "B = 65536", dict(B=65536)),
    ("slr_euler_backward_batch", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_backward_batch", "B = 65536", dict(B=65536)),
    ("slr_euler_backward_batch", "B*H*W = 2^38", dict(B=512, H=16384, W=32768)),
    ("slr_euler_pair_forward", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_pair_forward", "B = 65536", dict(B=65536)),
    ("slr_euler_pair_backward", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_euler_pair_backward", "B = 65536", dict(B=65536)),
    ("slr_ssim_mse", "H*W = 2^31 - 128", dict(C=3, H=128, W=16777215)),
    ("slr_ssim_mse", "N*C*H*W = 2^40", dict(N=1024, C=64, H=4096, W=4096)),
    ("slr_vgg_prep", "H*W = 2^31", dict(H=65536, W=32768)),
    ("slr_vgg_prep", "N*H*W = 2^40", dict(N=1024, H=32768, W=32768)),
    ("slr_lpips_prep", "H*W = 2^31", dict(H=65536, W=32768)),
    ("slr_lpips_prep", "N*H*W = 2^40", dict(N=1024, H=32768, W=32768)),
    ("slr_feature_cos_distance", "H*W = 2^31 - 256", dict(H=256, W=8388607)),
    ("slr_lpips_distance", "H*W = 2^31 - 256", dict(H=256, W=8388607)),
    ("slr_lpips_distance", "N = 65536", dict(N=65536)),
    ("slr_conv3x3_weight_grad", "N*max(Cin,Cout)*H*W = 2^31 - 1024", dict(Cin=1, Cout=1, H=1024, W=2097151)),
    ("slr_conv3x3_weight_grad", "N*Cout = 65536", dict(N=8192, H=1, W=1)),
    ("slr_conv3x3_weight_grad", "9*Cout*Cin >= 2^31 - 64", dict(Cin=15447, Cout=15447, H=1, W=1)),
    ("slr_conv_grad_scale_bias", "N*C*H*W = 2^31 - 1024", dict(C=1, H=1024, W=2097151)),
    ("slr_conv_grad_scale_bias", "N*C = 65536", dict(N=8192, H=1, W=1)),
    ("slr_conv1x1_weight_grad", "N*max(Cin,Cout)*H*W = 2^31 - 1024", dict(Cin=1, Cout=1, H=1024, W=2097151)),
    ("slr_conv1x1_weight_grad", "Cin*Cout = 2^28", dict(Cin=16384, Cout=16384, H=1, W=1)),
    ("slr_bn_batch_stats", "N*C*H*W = 2^31 - 1024", dict(C=1, H=1024, W=2097151)),
    ("slr_bn_batch_stats", "N*C = 65536", dict(N=8192, H=1, W=1)),
    ("slr_bn_relu_mask_train", "N*C*H*W = 2^31 - 1024", dict(C=1, H=1024, W=2097151)),
    ("slr_pconv_train_epilogue", "N*C*H*W = 2^31 - 1024", dict(C=1, H=1024, W=2097151)),
    ("slr_avgpool3x3s2_backward", "H*W = 2^30", dict(H=32768, W=32768)),
    ("slr_avgpool3x3s2_backward", "N*C = 65536", dict(N=8192)),
    ("slr_upsample_bilinear2x_backward", "H*W = 2^28", dict(H=16384, W=16384)),
]
# the words of a size refusal; the Euler entry points say what is too large
WORDS = {"slr_euler": (b"size", b"too large")}


def test_every_probed_entry_point_is_an_export_and_every_table_row_is_probed():
    from slr_sfs_amd._lib import SIGNATURES
    for name, args in ENTRY.items():
        assert len(args) + 1 == len(SIGNATURES[name][1]), name          # (+ the stream)
        assert all(a in SMALL for a in args if isinstance(a, str)), name
    assert {p[0] for p in PROBES} == set(ENTRY)
    assert len({(p[0], p[1]) for p in PROBES}) == len(PROBES)


@pytest.mark.parametrize("name,what,sizes", PROBES, ids=[f"{p[0]}-{p[1]}".replace(" ", "") for p in PROBES])
def test_size_past_the_limit_is_refused(L, name, what, sizes):
    dims = dict(SMALL, **OWN.get(name, {}))
    dims.update(sizes)
    args = [dims[a] if isinstance(a, str) else a for a in ENTRY[name]]
    rc = getattr(L, name)(*args, None)
    msg = L.slr_last_error()
    words = next((w for prefix, w in WORDS.items() if name.startswith(prefix)), (b"size",))
    assert rc == -1 and name.encode() in msg and any(w in msg for w in words), (name, what, rc, msg)
