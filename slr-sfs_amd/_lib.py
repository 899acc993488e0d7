"""ctypes binding of libslrsplat.so (C ABI: include/slr_splat.h).  No fallback of any kind."""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SLR_SFS_AMD_LIB") or os.path.join(_HERE, "lib", "libslrsplat.so")   # env: dev only
ABI_VERSION = 28
WS_PREBINNED, WS_CLEAN = 1, 2       # include/slr_splat.h: flags of the `prebinned` argument
BLEND_DETERMINISTIC = 1             # ... of slr_splat_blend_forward_ex's `flags`

# The C ABI of include/slr_splat.h, once: entry point -> (return type, argument types).  lib() applies it; SYMBOLS is its keys.
_vp, _fp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
SIGNATURES = {
    "slr_abi_version": (_i, []),
    "slr_last_error": (ctypes.c_char_p, []),
    "slr_splat_time_next": (None, [_vp, _vp]),
    "slr_euler_integrate": (_i, [_fp, _i, _i, _i, _f, _fp, _fp, _vp]),
    "slr_euler_integrate_all": (_i, [_fp, _i, _i, _i, _f, _fp, _fp, _vp]),
    "slr_euler_backward": (_i, [_fp, _i, _i, _i, _f, _fp, _fp, _vp]),
    "slr_euler_integrate_batch": (_i, [_fp, _vp, _i, _i, _i, _f, _fp, _fp, _vp]),
    "slr_euler_backward_batch": (_i, [_fp, _vp, _i, _i, _i, _f, _fp, _fp, _vp]),
    "slr_euler_pair_forward": (_i, [_fp, _vp, _vp, _i, _i, _i, _fp, _fp, _fp, _fp, _vp]),
    "slr_euler_pair_workspace_bytes": (_sz, [_i, _i, _i]),
    "slr_euler_pair_backward": (_i, [_fp, _vp, _vp, _i, _i, _i, _fp, _fp, _fp, _vp, _sz, _vp]),
    "slr_splat_workspace_bytes": (_sz, [_i, _i, _i]),
    "slr_splat_workspace_init": (_i, [_vp, _sz, _i, _i, _i, _vp]),
    "slr_splat_bin": (_i, [_fp, _i, _i, _i, _vp, _sz, _vp]),
    "slr_splat_bin_pair": (_i, [_fp, _fp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "slr_splat_set_scan_max_tiles": (_i, [_i]),
    "slr_splat_set_front_end": (_i, [_i]),
    "slr_splat_set_scan_shape": (None, [_i, _i, _i, _i]),
    "slr_softsplat_forward": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _i, _vp]),
    "slr_softsplat_mode_forward": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp]),
    "slr_splat_normalize": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _f, _vp]),
    "slr_synth_group": (_i, [_fp, _fp, _fp, _i, _fp, _fp, _f, _fp, _fp, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "slr_clip_plan_bytes": (_sz, [_i, _i, _i]),
    "slr_clip_plan_totals": (_i, [_i, _i, _i, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    "slr_clip_plan_build": (_i, [_fp, _vp, _fp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "slr_pack_planes4": (_i, [_fp, _fp, _i, _i, _i, _i, _vp]),
    "slr_synth_group_clip_batch": (_i, [_fp, _fp, _fp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _sz, _i, _vp, _i, _vp, _vp]),
    "slr_synth_two_groups_clip_batch": (_i, [_fp, _fp, _fp, _i, _fp, _fp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _sz, _i, _vp, _i, _vp, _vp]),
    "slr_synth_group_clip": (_i, [_fp, _fp, _fp, _i, _fp, _fp, _f, _fp, _fp, _i, _i, _i, _f, _vp, _sz, _i, _i, _i, _vp]),
    "slr_global_max": (_i, [_fp, _sz, _fp, _fp, _vp]),
    "slr_softsplat_backward": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "slr_softsplat_backward_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_softsplat_backward_ws": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_splat_blend_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_splat_blend_forward": (_i, [_fp] * 9 + [_f, _f, _f, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _i, _vp, _sz, _vp]),
    "slr_splat_blend_forward_ex": (_i, [_fp] * 9 + [_f, _f, _f, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _i, _i, _vp, _sz, _vp]),
    "slr_splat_fallback_count_offset": (_sz, [_i, _i, _i]),
    "slr_splat_blend_backward": (_i, [_fp] * 9 + [_f, _f, _f] + [_fp] * 9 + [_i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_maxsplat_forward": (_i, [_fp, _fp, _fp, _f, _i, _i, _i, _i, _vp, _sz, _i, _vp]),
    "slr_max_warp_norm": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _i, _vp]),
    "slr_bn_relu_mask": (_i, [_fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _vp]),
    "slr_pconv_epilogue": (_i, [_fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _f, _i, _i, _i, _i, _vp]),
    "slr_conv_saturation_count": (_i, [ctypes.POINTER(ctypes.c_ulonglong), _i, _vp]),
    "slr_conv_saturation_record": (_i, [_vp, _vp]),
    "slr_conv3x3_weight_bytes": (_sz, [_i, _i]),
    "slr_conv3x3_split_weights": (_i, [_fp, _vp, _i, _i, _f, _vp]),
    "slr_conv3x3_f32_weights": (_i, [_fp, _vp, _i, _i, _vp]),
    "slr_conv3x3_wino_weight_bytes": (_sz, [_i, _i]),
    "slr_conv3x3_wino_weights": (_i, [_fp, _vp, _i, _i, _vp]),
    "slr_conv3x3_forward": (_i, [_fp, _vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _f, _fp, _fp, _i, _vp]),
    "slr_pconv3x3_forward": (_i, [_fp, _fp, _fp, _fp, _vp, _f, _f, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "slr_conv_pool_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_conv_up_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_conv3x3_forward_skip": (_i, [_fp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _f, _f, _fp, _fp, _fp, _vp, _fp, _i, _f, _vp, _sz, _i, _vp]),
    "slr_pconv3x3_forward_skip": (_i, [_fp, _fp, _fp, _fp, _vp, _f, _f, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _vp, _i, _f, _vp, _sz, _i, _vp]),
    "slr_conv3x3_forward_skipout": (_i, [_fp, _vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _f, _fp, _fp, _fp, _fp, _fp, _i, _vp]),
    "slr_pconv3x3_forward_skipout": (_i, [_fp, _fp, _fp, _fp, _vp, _f, _f, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _i, _vp]),
    "slr_conv_tail_weight_bytes": (_sz, [_i]),
    "slr_conv_tail_weight_source": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "slr_conv_tail_weights": (_i, [_fp, _fp, _vp, _i, _f, _f, _vp]),
    "slr_pconv3x3_forward_tail": (_i, [_fp, _fp, _vp, _f, _f, _fp, _fp, _fp, _fp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_narrow_gather": (_i, [_fp] * 9 + [_i, _i, _i, _i, _f, _f, _f, _vp]),
    "slr_conv1x1_weight_bytes": (_sz, [_i, _i]),
    "slr_conv1x1_split_weights": (_i, [_fp, _vp, _i, _i, _f, _vp]),
    "slr_conv1x1_f32_weights": (_i, [_fp, _vp, _i, _i, _vp]),
    "slr_conv1x1_forward": (_i, [_fp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _f, _f, _i, _vp]),
    "slr_avgpool3x3s2": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_upsample_bilinear2x": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_conv1x1_small": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "slr_conv4x4s2_weight_bytes": (_sz, [_i, _i]),
    "slr_conv4x4s2_f32_weights": (_i, [_fp, _vp, _i, _i, _vp]),
    "slr_conv4x4s2_forward": (_i, [_fp, _vp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "slr_instnorm_spade": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _f, _vp]),
    "slr_resize_segmap": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "slr_upsample2x_concat": (_i, [_fp, _i, _fp, _i, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_ssim_ws_bytes": (_sz, [_i, _i, _i]),
    "slr_ssim_mse": (_i, [_vp, _vp, _i, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_vgg_prep": (_i, [_vp, _i, _i, _fp, _i, _i, _i, _vp]),
    "slr_relu_maxpool2x2_b8": (_i, [_fp, _fp, _i, _i, _i, _i, _vp]),
    "slr_feature_cos_ws_bytes": (_sz, [_i, _i, _i]),
    "slr_feature_cos_distance": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_loss_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_l1_loss_grad": (_i, [_fp, _fp, _fp, _fp, _f, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_feature_l1_gate_b8": (_i, [_fp, _fp, _fp, _fp, _fp, _f, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_relu_maxpool2x2_backward_b8": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "slr_conv3x3_grad_ws_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "slr_conv3x3_weight_grad": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_conv_grad_scale_bias": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_bn_train_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_bn_batch_stats": (_i, [_fp, _fp, _f, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_bn_train_tables": (_i, [_fp, _fp, _fp, _fp, _f, _fp, _fp, _i, _i, _vp]),
    "slr_bn_relu_mask_train": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_bn_relu_mask_backward": (_i, [_fp] * 9 + [_f] + [_fp] * 4 + [_i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_conv1x1_grad_ws_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "slr_conv1x1_weight_grad": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_avgpool3x3s2_backward": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_upsample_bilinear2x_backward": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_bn_nonzero_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "slr_bn_nonzero_stats": (_i, [_fp, _f, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_nonzero_count_plane": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_bn_relu_nonzero_train": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_bn_relu_nonzero_backward": (_i, [_fp] * 8 + [_f] + [_fp] * 4 + [_i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_pconv_train_epilogue": (_i, [_fp] * 6 + [_i, _i, _i, _i, _i, _vp]),
    "slr_conv4x4_weight_bytes": (_sz, [_i, _i, _i]),
    "slr_conv4x4_f32_weights": (_i, [_fp, _fp, _vp, _i, _i, _i, _i, _vp]),
    "slr_conv4x4_forward": (_i, [_fp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "slr_conv4x4_backward_data": (_i, [_fp, _fp, _vp, _fp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "slr_conv4x4_grad_ws_bytes": (_sz, [_i] * 7),
    "slr_conv4x4_weight_grad": (_i, [_fp] * 5 + [_i, _i, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp]),
    "slr_instnorm_lrelu_forward": (_i, [_fp] * 4 + [_i, _i, _i, _i, _f, _f, _vp]),
    "slr_instnorm_lrelu_backward": (_i, [_fp] * 5 + [_i, _i, _i, _i, _f, _vp]),
    "slr_adam_plan_bytes": (_sz, [_i, _vp]),
    "slr_adam_plan_fill": (_i, [_vp, _sz, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slr_adam_step": (_i, [_vp, _i, _i, _fp, _vp, _f, _i, _vp]),
    "slr_spectral_plan_bytes": (_sz, [_i, _vp, _vp]),
    "slr_spectral_plan_fill": (_i, [_vp, _sz, _i, _vp, _vp, _vp, _vp, _vp]),
    "slr_spectral_sigma": (_i, [_vp, _i, _i, _fp, _fp, _fp, _i, _vp]),
    "slr_conv3x3_f32_weights_scaled": (_i, [_fp, _fp, _vp, _i, _i, _i, _vp]),
    "slr_conv1x1_f32_weights_scaled": (_i, [_fp, _fp, _vp, _i, _i, _i, _vp]),
    "slr_conv_prep_plan_bytes": (_sz, [_i, _vp, _vp, _vp, _vp]),
    "slr_conv_prep_plan_fill": (_i, [_vp, _sz, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slr_conv_prep_scaled_multi": (_i, [_vp, _i, _i, _fp, _vp]),
    "slr_spectral_grad_ws_bytes": (_sz, [_i, _i]),
    "slr_spectral_weight_grad": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _vp, _sz, _vp]),
    "slr_spectral_grad_plan_bytes": (_sz, [_i, _vp, _vp]),
    "slr_spectral_grad_plan_fill": (_i, [_vp, _sz, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slr_spectral_weight_grad_multi": (_i, [_vp, _i, _i, _fp, _fp, _fp, _vp]),
    "slr_conv4x4s2_backward_data": (_i, [_fp, _fp, _vp, _fp, _i, _i, _i, _i, _i, _f, _vp]),
    "slr_conv4x4s2_grad_ws_bytes": (_sz, [_i] * 6),
    "slr_conv4x4s2_weight_grad": (_i, [_fp] * 4 + [_i, _i, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp]),
    "slr_instnorm_spade_train_forward": (_i, [_fp] * 5 + [_i, _i, _i, _i, _f, _vp]),
    "slr_instnorm_spade_backward": (_i, [_fp] * 7 + [_i, _i, _i, _i, _vp]),
    "slr_upsample2x_concat_backward": (_i, [_fp, _fp, _fp, _i, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "slr_motion_loss_ws_bytes": (_sz, [_i, _i, _i]),
    "slr_motion_loss": (_i, [_fp, _fp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "slr_motion_loss_grad": (_i, [_fp] * 5 + [_i, _i, _i, _vp]),
    "slr_layer_composite_forward": (_i, [_fp] * 8 + [_i, _i, _i, _vp]),
    "slr_layer_composite_backward": (_i, [_fp] * 11 + [_i, _i, _i, _vp]),
    "slr_alpha_losses_ws_bytes": (_sz, [_i, _i, _i]),
    "slr_alpha_losses_forward": (_i, [_fp] * 9 + [_i, _i, _i, _i, _vp, _sz, _vp]),
    "slr_alpha_losses_backward": (_i, [_fp] * 10 + [_i, _i, _i, _i, _vp]),
    "slr_blend_alpha0_ws_bytes": (_sz, [_i, _i, _i]),
    "slr_blend_alpha0_forward": (_i, [_fp] * 5 + [_f, _i, _i, _i, _vp, _sz, _vp]),
    "slr_blend_alpha0_backward": (_i, [_fp] * 6 + [_f, _i, _i, _i, _vp]),
    "slr_lpips_prep": (_i, [_vp, _i, _i, _fp, _i, _i, _i, _vp]),
    "slr_convkxk_weight_bytes": (_sz, [_i, _i, _i]),
    "slr_convkxk_f32_weights": (_i, [_fp, _vp, _i, _i, _i, _vp]),
    "slr_convkxk_forward": (_i, [_fp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "slr_relu_maxpool3x3s2_b8": (_i, [_fp, _fp, _i, _i, _i, _i, _vp]),
    "slr_lpips_distance_ws_bytes": (_sz, [_i, _i, _i]),
    "slr_lpips_distance": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
}
SYMBOLS = tuple(SIGNATURES)

_lib = None
_lock = threading.Lock()


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of the library (cross-compiles without a GPU)."""
    import subprocess
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc")], stdout=out)
    return LIB_PATH


def lib():
    """The loaded library; raises RuntimeError (loudly) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"slr_sfs_amd: HIP library {LIB_PATH} is missing -- build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C slr-sfs_amd/csrc`). "
                f"There is no CPU/PyTorch fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.slr_abi_version() != ABI_VERSION:
            raise RuntimeError(f"slr_sfs_amd: {LIB_PATH} has ABI {L.slr_abi_version()}, expected {ABI_VERSION}")
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().slr_last_error()
        # A failed call may have left the counters of its workspace dirty (a launch error in flight): the calls that follow say
        # SLR_WS_CLEAN and would trust them.  Drop every cached workspace -- the next call gets a freshly initialised one.
        if rc > 0:                                       # (a hipError_t; argument errors, rc < 0, launch nothing)
            clear_workspaces()
        raise RuntimeError(f"slr_sfs_amd: {what} failed (rc={rc}): {msg.decode() if msg else ''}")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call(name, device, *args):
    """Entry point ``name`` of the library, looked up at every call, with ``args`` (tensors as their device pointers) and torch's
    current stream on ``device``, run with ``device`` current; raises naming the entry point if it fails."""
    args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]   # (isinstance: ~1.5 us less per call than torch.is_tensor)
    with torch.cuda.device(device):
        check(getattr(lib(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)), name)


def stream_of(t):
    """HIP stream handle torch is currently using on the tensor's device."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_device(*tensors):
    """The reference raises NotImplementedError for CPU tensors (models/softsplat.py:418-419)
    and asserts contiguity (:401-402); same here -- there is no CPU path."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")
        assert t.is_contiguous() is True


# ---- scratch: caller-owned workspaces, cached per (device, stream, role, shape), least-recently-used eviction ----
# A workspace is tied to the stream it was first used on (two streams must never share one), so the stream handle is
# part of the key; the cache is bounded -- a service that animates many resolutions or creates and destroys streams
# would otherwise pin ~300 MB of HBM per (stream, shape) for ever.  Evicted tensors go back to torch's stream-ordered
# caching allocator (safe: they were only ever used on the stream they were allocated on).
# HIP graphs: a workspace that was handed out while its stream was CAPTURING has its address baked into the captured
# graph, whose replays nobody can see from here -- such workspaces are pinned: never evicted (clear_workspaces(
# include_captured=True) drops them once the graphs that use them are gone), and nothing is evicted during a capture.
import collections

WS_CACHE_MAX = max(1, int(os.environ.get("SLR_SFS_AMD_WS_CACHE", "8")))
_ws_cache = collections.OrderedDict()
_ws_captured = {}


def workspace(t, role, N, C, H, W, nbytes=None):
    """A torch-allocated (stream-ordered) workspace for splatting [N,<=C,H,W] on t's device."""
    stream = torch.cuda.current_stream(t.device)
    key = (t.device.index, stream.cuda_stream, role, N, C, H, W, nbytes)
    ws = _ws_captured.get(key)
    if ws is not None:
        return ws
    with torch.cuda.device(t.device):                    # (the capture status of t's device, not of the current one)
        capturing = torch.cuda.is_current_stream_capturing()
    ws = _ws_cache.get(key)
    if ws is None:
        if nbytes is None:
            nbytes = int(lib().slr_splat_workspace_bytes(N, H, W))
        while not capturing and len(_ws_cache) >= WS_CACHE_MAX:
            _ws_cache.popitem(last=False)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
        # a splat workspace starts zeroed; the kernels leave its counters zero again, so the calls may say WS_CLEAN (no zero kernel)
        call("slr_splat_workspace_init", t.device, ws, ws.numel(), N, H, W)
        _ws_cache[key] = ws
    else:
        _ws_cache.move_to_end(key)
    if capturing:                                       # its address is now part of a graph: keep it for good
        _ws_captured[key] = _ws_cache.pop(key)
    return ws


def clear_workspaces(include_captured=False):
    _ws_cache.clear()
    if include_captured:
        _ws_captured.clear()
