"""sggan_amd -- MI355X-native SG-GAN train-step hot path.

The directory is called ``sg-gan-tf2_amd`` (not an importable name); import it as
``sggan_amd`` via the shim at the repository root.
"""
from . import _abi  # noqa: F401
from ._abi import SggError, lib  # noqa: F401
from .model import default_args, sggan  # noqa: F401
from .module import D_NORMS, UPSAMPLES, Discriminator, Generator, GeneratorUNet, discriminator, discriminator_param_specs, generator_resnet, generator_unet  # noqa: F401
from .ops import conv2d, deconv2d, diff_augment, feature_match, instance_norm, lrelu, relu, ssim_loss, tanh, upsample2x  # noqa: F401

__all__ = ["sggan", "default_args", "generator_resnet", "generator_unet", "discriminator", "Generator", "GeneratorUNet", "Discriminator",
           "conv2d", "deconv2d", "instance_norm", "lrelu", "relu", "tanh", "diff_augment", "ssim_loss", "feature_match", "upsample2x", "D_NORMS", "UPSAMPLES", "discriminator_param_specs", "lib", "SggError", "LIB_PATH"]


def __getattr__(name):
    if name == "LIB_PATH":              # the library actually bound (tools/ may select another build before first use)
        return _abi.LIB_PATH
    raise AttributeError(name)
