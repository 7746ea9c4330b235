from .autoencoder_asym_kl import AsymmetricAutoencoderKL
from .autoencoder_kl import AutoencoderKL
from .autoencoder_tiny import AutoencoderTiny
from .BrushNet_CA import BrushNetModel
from .clip_text import CLIPTextModel
from .clip_vision import CLIPVisionModelWithProjection
from .controlnet import ControlNetModel, MultiControlNetModel
from .unet_2d_condition import UNet2DConditionModel

__all__ = ["BrushNetModel", "UNet2DConditionModel", "ControlNetModel", "MultiControlNetModel", "AutoencoderKL",
           "AsymmetricAutoencoderKL", "AutoencoderTiny", "CLIPTextModel", "CLIPVisionModelWithProjection"]
