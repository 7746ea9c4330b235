"""VaeImageProcessor: the PIL / NumPy <-> tensor conversions at the two ends of the pipelines.

Host-side mirror of the diffusers class the reference pipelines instantiate
(/root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:284 `VaeImageProcessor(vae_scale_factor=...)`, :1058
`image_processor.postprocess(image, output_type=..., do_denormalize=...)`; pipeline_PowerPaint_Brushnet_CA.py:1305-1311
`image_processor.preprocess(image / mask, height, width)`; pipeline_PowerPaint_ControlNet.py:281-283
`VaeImageProcessor(do_convert_rgb=True, do_normalize=False)` for the control image).  diffusers itself is not
installable here: these are the documented conversions (uint8 / 255, 2x - 1, Lanczos resize to multiples of the VAE
factor, x / 2 + 0.5 clamped, round to uint8), restated; plain data-format glue, no tensor math of the hot path.
"""
from typing import List, Optional

import numpy as np
import torch


OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class CLIPImageProcessor:
    """transformers' `CLIPImageProcessor` as the `feature_extractor` of an IP-Adapter pipeline uses it (host code, PIL for the
    resize): RGB -> shortest edge to `size` (bicubic, the long edge truncated: int(size * long / short)) -> centre crop to
    `crop_size` -> * 1/255 -> (x - mean) / std -> NCHW float32.  Images are PIL images or HWC uint8 arrays, or lists of either;
    `processor(images, return_tensors="pt").pixel_values` is [B, 3, crop, crop]."""

    def __init__(self, size=224, crop_size=224, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD,
                 rescale_factor: float = 1 / 255, do_resize: bool = True, do_center_crop: bool = True, do_rescale: bool = True,
                 do_normalize: bool = True, do_convert_rgb: bool = True, resample=3, **unused):
        if isinstance(size, dict):
            if "shortest_edge" not in size:
                raise ValueError(f"CLIPImageProcessor: size must name `shortest_edge`, got {size}")
            size = size["shortest_edge"]
        if isinstance(crop_size, dict):
            crop_size = (crop_size["height"], crop_size["width"])
        elif isinstance(crop_size, int):
            crop_size = (crop_size, crop_size)
        if int(resample) != 3:
            raise ValueError(f"CLIPImageProcessor: only bicubic resampling (PIL code 3) is implemented, got {resample}")
        self.size, self.crop_size = int(size), tuple(int(c) for c in crop_size)
        self.image_mean, self.image_std, self.rescale_factor = tuple(image_mean), tuple(image_std), float(rescale_factor)
        self.do_resize, self.do_center_crop, self.do_rescale = bool(do_resize), bool(do_center_crop), bool(do_rescale)
        self.do_normalize, self.do_convert_rgb = bool(do_normalize), bool(do_convert_rgb)

    @classmethod
    def from_pretrained(cls, folder: str, **kw):
        """`<folder>/preprocessor_config.json` (a local folder; nothing is downloaded)."""
        import json
        import os
        f = os.path.join(str(folder), "preprocessor_config.json")
        if not os.path.isfile(f):
            raise FileNotFoundError(f"{f} not found")
        with open(f) as fh:
            cfg = json.load(fh)
        cfg.update(kw)
        return cls(**cfg)

    def _one(self, image) -> np.ndarray:
        import PIL.Image
        if isinstance(image, np.ndarray):
            if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (1, 3, 4):
                raise ValueError(f"CLIPImageProcessor: arrays must be HWC uint8, got {image.dtype} {image.shape}")
            image = PIL.Image.fromarray(image[:, :, 0] if image.shape[2] == 1 else image)
        if not isinstance(image, PIL.Image.Image):
            raise ValueError(f"CLIPImageProcessor: unsupported image type {type(image)}")
        if self.do_convert_rgb or image.mode != "RGB":
            image = image.convert("RGB")
        if self.do_resize:
            w, h = image.size
            short, long = (w, h) if w <= h else (h, w)
            new_long = int(self.size * long / short)
            image = image.resize((self.size, new_long) if w <= h else (new_long, self.size), resample=PIL.Image.BICUBIC)
        x = np.asarray(image)                                               # HWC uint8
        if self.do_center_crop:
            ch, cw = self.crop_size
            h, w = x.shape[:2]
            if h < ch or w < cw:
                raise ValueError(f"CLIPImageProcessor: a {h}x{w} image is smaller than the crop {ch}x{cw} (padding is not implemented)")
            top, left = (h - ch) // 2, (w - cw) // 2
            x = x[top:top + ch, left:left + cw]
        x = x.transpose(2, 0, 1)
        if self.do_rescale:
            x = (x.astype(np.float64) * self.rescale_factor).astype(np.float32)
        else:
            x = x.astype(np.float32)
        if self.do_normalize:
            mean = np.array(self.image_mean, dtype=np.float32)[:, None, None]
            std = np.array(self.image_std, dtype=np.float32)[:, None, None]
            x = (x - mean) / std
        return x

    def __call__(self, images, return_tensors: Optional[str] = "pt", **unused):
        from types import SimpleNamespace
        if not isinstance(images, (list, tuple)):
            images = [images]
        if not images:
            raise ValueError("CLIPImageProcessor: no image given")
        arr = np.stack([self._one(i) for i in images], axis=0)
        if return_tensors not in ("pt", "np", None):
            raise ValueError(f"CLIPImageProcessor: return_tensors={return_tensors!r} (\"pt\" or \"np\")")
        return SimpleNamespace(pixel_values=torch.from_numpy(arr) if return_tensors == "pt" else arr)


class VaeImageProcessor:
    def __init__(self, do_resize: bool = True, vae_scale_factor: int = 8, resample: str = "lanczos",
                 do_normalize: bool = True, do_binarize: bool = False, do_convert_rgb: bool = False,
                 do_convert_grayscale: bool = False):
        from types import SimpleNamespace
        self.config = SimpleNamespace(do_resize=do_resize, vae_scale_factor=vae_scale_factor, resample=resample,
                                      do_normalize=do_normalize, do_binarize=do_binarize,
                                      do_convert_rgb=do_convert_rgb, do_convert_grayscale=do_convert_grayscale)

    # ---- elementary conversions
    @staticmethod
    def numpy_to_pil(images: np.ndarray) -> list:
        import PIL.Image
        if images.ndim == 3:
            images = images[None, ...]
        images = (images * 255).round().astype("uint8")
        if images.shape[-1] == 1:
            return [PIL.Image.fromarray(i.squeeze(), mode="L") for i in images]
        return [PIL.Image.fromarray(i) for i in images]

    @staticmethod
    def pil_to_numpy(images) -> np.ndarray:
        if not isinstance(images, list):
            images = [images]
        return np.stack([np.array(i).astype(np.float32) / 255.0 for i in images], axis=0)

    @staticmethod
    def numpy_to_pt(images: np.ndarray) -> torch.Tensor:
        if images.ndim == 3:
            images = images[..., None]
        return torch.from_numpy(images.transpose(0, 3, 1, 2))

    @staticmethod
    def pt_to_numpy(images: torch.Tensor) -> np.ndarray:
        return images.cpu().permute(0, 2, 3, 1).float().numpy()

    @staticmethod
    def normalize(images):
        return 2.0 * images - 1.0

    @staticmethod
    def denormalize(images):
        return (images / 2 + 0.5).clamp(0, 1)

    def get_default_height_width(self, image, height: Optional[int] = None, width: Optional[int] = None):
        import PIL.Image
        if height is None:
            height = image.height if isinstance(image, PIL.Image.Image) else image.shape[2 if torch.is_tensor(image) else 1]
        if width is None:
            width = image.width if isinstance(image, PIL.Image.Image) else image.shape[3 if torch.is_tensor(image) else 2]
        f = self.config.vae_scale_factor
        return height - height % f, width - width % f

    def resize(self, image, height: int, width: int):
        import PIL.Image
        if isinstance(image, PIL.Image.Image):
            res = {"lanczos": PIL.Image.LANCZOS, "bilinear": PIL.Image.BILINEAR, "bicubic": PIL.Image.BICUBIC,
                   "nearest": PIL.Image.NEAREST}[self.config.resample]
            return image.resize((width, height), resample=res)
        if torch.is_tensor(image):
            return torch.nn.functional.interpolate(image, size=(height, width))
        return self.pt_to_numpy(torch.nn.functional.interpolate(self.numpy_to_pt(image), size=(height, width)))

    # ---- the two entry points the pipelines use
    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        import PIL.Image
        if isinstance(image, (PIL.Image.Image, np.ndarray, torch.Tensor)):
            image = [image]
        if not isinstance(image, list) or not image:
            raise ValueError("image must be a PIL image, an ndarray, a tensor or a list of those")
        first = image[0]
        if isinstance(first, PIL.Image.Image):
            if self.config.do_convert_rgb:
                image = [i.convert("RGB") for i in image]
            elif self.config.do_convert_grayscale:
                image = [i.convert("L") for i in image]
            if self.config.do_resize:
                height, width = self.get_default_height_width(image[0], height, width)
                image = [self.resize(i, height, width) for i in image]
            t = self.numpy_to_pt(self.pil_to_numpy(image))
        elif isinstance(first, np.ndarray):
            arr = np.concatenate(image, axis=0) if first.ndim == 4 else np.stack(image, axis=0)
            t = self.numpy_to_pt(arr.astype(np.float32))
            if self.config.do_resize:
                height, width = self.get_default_height_width(t, height, width)
                t = self.resize(t, height, width)
        elif torch.is_tensor(first):
            t = torch.cat(image, dim=0) if first.ndim == 4 else torch.stack(image, dim=0)
            if t.ndim == 3:                                   # [B, H, W] masks
                t = t.unsqueeze(1)
            if self.config.do_resize:
                height, width = self.get_default_height_width(t, height, width)
                t = self.resize(t.float(), height, width)
        else:
            raise ValueError(f"unsupported image type {type(first)}")
        if self.config.do_normalize and not (torch.is_tensor(first) and t.min() < 0):
            t = self.normalize(t)                             # tensors already in [-1, 1] are left alone
        if self.config.do_binarize:
            t = (t >= 0.5).to(t.dtype)
        return t

    def postprocess(self, image: torch.Tensor, output_type: str = "pil",
                    do_denormalize: Optional[List[bool]] = None):
        if not torch.is_tensor(image):
            raise ValueError("postprocess expects the decoded image tensor [B, C, H, W]")
        if output_type == "latent":
            return image
        if output_type not in ("pt", "np", "pil"):
            output_type = "np"
        if do_denormalize is None:
            do_denormalize = [self.config.do_normalize] * image.shape[0]
        image = torch.stack([self.denormalize(image[i]) if do_denormalize[i] else image[i]
                             for i in range(image.shape[0])])
        if output_type == "pt":
            return image
        arr = self.pt_to_numpy(image)
        return arr if output_type == "np" else self.numpy_to_pil(arr)


class IPAdapterMaskProcessor(VaeImageProcessor):
    """diffusers-0.27 `IPAdapterMaskProcessor`: `preprocess(masks, height=, width=)` turns PIL images / arrays / tensors into
    the binary [n, 1, H, W] tensor that `cross_attention_kwargs={"ip_adapter_masks": ...}` takes (grey, Lanczos resize,
    >= 0.5 -> 1), and the static `downsample` is the rule by which one adapter's mask becomes one weight per query row of a
    cross-attention level -- the ONE implementation of it: NetRuntime.set_ip_masks fills the kernels' weight buffers with it."""

    def __init__(self, do_resize: bool = True, vae_scale_factor: int = 8, resample: str = "lanczos",
                 do_normalize: bool = False, do_binarize: bool = True, do_convert_grayscale: bool = True):
        super().__init__(do_resize=do_resize, vae_scale_factor=vae_scale_factor, resample=resample,
                         do_normalize=do_normalize, do_binarize=do_binarize, do_convert_grayscale=do_convert_grayscale)

    @staticmethod
    def downsample(mask: torch.Tensor, batch_size: int, num_queries: int, value_embed_dim: int) -> torch.Tensor:
        """mask [1, H, W] -> [batch_size, num_queries, value_embed_dim]: a bicubic resize (unclamped: a binary mask rings to
        about -0.094 and 1.094) to the grid of the mask's OWN aspect ratio that holds num_queries positions, flattened in row
        order; a grid with fewer positions is padded with zeros at the end, one with more is cut (a warning each)."""
        import math
        import warnings
        o_h, o_w = mask.shape[1], mask.shape[2]
        ratio = o_w / o_h
        mask_h = int(math.sqrt(num_queries / ratio))
        if mask_h < 1:
            raise ValueError(f"a {o_h}x{o_w} mask has no grid of {num_queries} positions (its aspect ratio leaves no row)")
        mask_h = int(mask_h) + int((num_queries % int(mask_h)) != 0)
        mask_w = num_queries // mask_h
        m = torch.nn.functional.interpolate(mask.unsqueeze(0), size=(mask_h, mask_w), mode="bicubic").squeeze(0)
        if batch_size < m.shape[0]:
            m = m[:batch_size]
        elif batch_size > m.shape[0]:
            m = m.repeat(batch_size, 1, 1)
        m = m.view(m.shape[0], -1)
        area = mask_h * mask_w
        if area < num_queries:
            warnings.warn("The aspect ratio of the mask does not match the aspect ratio of the output image. "
                          "Please update your masks or adjust the output size for optimal performance.", UserWarning)
            m = torch.nn.functional.pad(m, (0, num_queries - m.shape[1]), value=0.0)
        if area > num_queries:
            warnings.warn("The aspect ratio of the mask does not match the aspect ratio of the output image. "
                          "Please update your masks or adjust the output size for optimal performance.", UserWarning)
            m = m[:, :num_queries]
        return m.reshape(m.shape[0], m.shape[1], 1).repeat(1, 1, value_embed_dim)
