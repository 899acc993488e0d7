"""slr_sfs_amd -- MI355X-native Euler-warp + softmax-splat frame synthesis.

Drop-in replacement for the hot path of simon3dv/SLR-SFS:
  models/softsplat.py                                  -> slr_sfs_amd.softsplat
  models/projection/euler_integration_manipulator.py   -> slr_sfs_amd.euler_integration_manipulator
  forward_flow data-flow of models/animating_softmax_splating*.py -> slr_sfs_amd.synthesis

All compute runs in hand-written HIP kernels (slr-sfs_amd/csrc, C ABI in include/slr_splat.h)
loaded from slr-sfs_amd/lib/libslrsplat.so.  There is NO fallback: importing works without a
GPU (so the build can be checked), but every operator raises if the library is missing or the
tensors are not on a ROCm device.
"""
from . import _lib  # noqa: F401
from . import softsplat, euler_integration_manipulator, synthesis, nets, pipeline, parallel, io, motion, metrics, evaluation, training, losses, trainable, adversarial, optim, spectral  # noqa: F401
from .training import splat_blend, TrainingSynthesis  # noqa: F401
from .losses import SynthesisLoss, PerceptualLoss, L1LossWrapper, VGG19Features, load_vgg19_state_dict  # noqa: F401
from .trainable import conv3x3, partial_conv3x3, TrainableConv3x3, TrainablePartialConv3x3  # noqa: F401
from .trainable import (bn_relu_mask_train, conv1x1, avgpool_down, upsample_up, TrainableConv1x1, TrainableNoiseBN,  # noqa: F401
                        TrainablePconvResBlock)
from .trainable import (bn_relu_nonzero_train, partial_conv_factors_counts, partial_conv3x3_counts, TrainablePconvInputBlock,  # noqa: F401
                        TrainableResBlock, TrainableDecoderPconv2, TrainableEncoderWithZ, TrainableEncoder, TrainableBGDecoder)
from .adversarial import (conv4x4, instnorm_lrelu, spectral_weight, TrainableNLayerDiscriminator,  # noqa: F401
                          TrainableMultiscaleDiscriminator, GANLoss, DiscriminatorLoss)
from .optim import Adam, TrainingOptimizers  # noqa: F401
from .spectral import SpectralGroup, SpectralLinear, spectral_sigma, prepare_scaled, spectral_weight_grad, load_spectral_state_dict, reference_state_dict  # noqa: F401
from .spectral import spectral_weight_grad_multi, defer_weight_grad  # noqa: F401
from . import motion_training  # noqa: F401
from .motion_training import (conv4x4s2, instnorm_spade_train, upsample2x_concat_train, motion_losses, MotionLoss,  # noqa: F401
                              TrainableSPADEIN, TrainableSPADEUnet4MaskMotion, MotionTrainingModel)
from . import model  # noqa: F401
from .model import TrainingModel, Trainer, JointTrainingModel, check_joint_options  # noqa: F401
from . import layers  # noqa: F401
from .layers import layer_composite, alpha_losses, blend_alpha0, TwoLayerTrainingModel, TwoLayerAlpha0TrainingModel  # noqa: F401
from .softsplat import FunctionSoftsplat, ModuleSoftsplat, ModuleMaximumsplat, ModuleMaximumWarpNormsplat  # noqa: F401
from .euler_integration_manipulator import euler_integration, EulerIntegration, euler_integration_all, euler_integration_pair  # noqa: F401
from .dropin import install_into_reference  # noqa: F401

__version__ = "0.1.0"
