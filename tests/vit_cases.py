"""Shared cases of tests/test_clip_vision.py and tests/test_vit_kernels_gpu.py: the CLIP vision tower on the HIP path.

The pin of the tower is `transformers.CLIPVisionModelWithProjection` itself on the CPU in fp32, on weights whose matrices are
rounded to bf16 (what the HIP path stores), initialised as tests/test_clip.py::hf_model initialises the text tower: the default
init is tiny, so matrices are scaled and biases / norms perturbed.

Bounds of the kernel tests (nothing fitted):

  pp_vit_patchify   a copy with one rounding: integer pixels in [-256, 256] are representable in bf16 and fp16, so the rows
                    EQUAL F.unfold's bit for bit, the pad columns are exact zeros, everything else keeps its sentinel.
  pp_vit_embed_ln   the kernel forms e = a + b in fp32 from the stored 16-bit operands (one rounding, |de| <= 2^-24 |e|) and
                    then runs pp_layernorm's arithmetic on e.  The gate is norm_cases.gate_layernorm evaluated ON the fp64 sum
                    (two passes, no magnification) plus that one u32 term pushed through the norm: a perturbation de of the
                    input moves (e - mean) rstd gamma by at most |gamma| rstd (|de| + mean|de| + |e - mean| rstd^2
                    mean(|e - mean| |de|)) -- the three places e enters (the element, the mean, the variance).
  PP_ACT_GELU       gemm_cases' gate for the pre-activation, d = (K + splits + 5) 2^-24 A, pushed through the GELU, whose slope
                    is at most 1.13: 1.13 d; + 1.5e-7 for the Abramowitz-Stegun erf (|erf error| <= 1.5e-7, so x Phi(x) errs by
                    0.75e-7 |x| where the tail has not vanished; the fp32 evaluation of the polynomial, the exponential and the
                    reciprocal costs a few u32 |x|, which d covers: A >= |pre| and K + splits + 5 >= 70); + one 16-bit rounding,
                    u |ref| (+ half the subnormal quantum 2^-25 in fp16, as norm_cases._finish has it).
                    The integer probe (pre-activation an exact small integer, output within ONE unit in the last place of fp64
                    x Phi(x)) takes integers from PROBE_MIN = -3 up: the store rounds by half a unit, so the evaluation may err
                    by half a unit, and it errs by up to 0.75e-7 |x| (above).  At x = -3, x Phi(x) = -4.05e-3, whose fp16 unit
                    is 2^-18 = 3.8e-6: 2.25e-7 is 6 % of it.  At x = -4, x Phi(x) = -1.27e-4 with an fp16 unit of 1.2e-7, below
                    the formula's own 3e-7: no probe can ask that of an erf good to 1.5e-7.  Upwards x Phi(x) -> x and the unit
                    grows with it.
"""
import math

import torch

U32 = 2.0 ** -24
PATCHIFY_SHAPES = ((1, 14, 14, 14), (2, 42, 28, 14), (3, 45, 31, 14), (1, 224, 224, 14))         # (B, H, W, P)
EMBED_SHAPES = ((1, 1, 64), (2, 9, 320), (3, 256, 1280))                                          # (B, np, C)
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
SPLITS = (1, 2, 3, 4, 8)              # gemm_cases.SPLITS
ERF_ERR = 1.5e-7                      # Abramowitz-Stegun 7.1.26
PROBE_MIN = -3                        # smallest pre-activation of the exact GELU probe (module docstring)

# the tower against transformers: (hidden, heads, intermediate, layers, image, projection, batch)
TOWER_CASES = {"a": (320, 4, 640, 2, 42, 64, 2), "b": (320, 4, 640, 2, 224, 64, 1), "c": (1280, 16, 5120, 2, 224, 1024, 3)}
TINY = dict(hidden_size=320, num_attention_heads=4, intermediate_size=640, num_hidden_layers=2, image_size=42, patch_size=14,
            projection_dim=64)


def hf_vision(seed=0, **cfg):
    """transformers.CLIPVisionModelWithProjection (eval, CPU fp32) with scaled weights, perturbed biases / norms and matrices
    rounded to bf16 -- tests/test_clip.py::hf_model for the vision tower."""
    import transformers
    kw = dict(hidden_act="gelu", patch_size=14)
    kw.update(cfg)
    torch.manual_seed(seed)
    m = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**kw)).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)
            elif "embedding" not in n:
                p.mul_(2.0)
            p.copy_(p.to(torch.bfloat16).float() if p.dim() >= 2 else p)
    return m


def tower_cfg(name: str) -> dict:
    c, h, f, layers, img, proj, _ = TOWER_CASES[name]
    return dict(hidden_size=c, num_attention_heads=h, intermediate_size=f, num_hidden_layers=layers, image_size=img,
                patch_size=14, projection_dim=proj)


def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gate_gelu(pre: torch.Tensor, A: torch.Tensor, K: int, splits: int, u: float):
    """-> (ref, gate) fp64 for out = round16(gelu(pre)), pre off by at most (K + splits + 5) 2^-24 A."""
    ref = gelu64(pre)
    d = (K + max(1, splits) + 5) * U32 * A.double()
    return ref, 1.13 * d + ERF_ERR + u * ref.abs() + (2.0 ** -25 if u < 2.0 ** -9 else 0.0)


def gate_embed_ln(e64: torch.Tensor, gamma, beta, eps: float, dtype):
    """-> (ref, gate) fp64 for pp_vit_embed_ln on the exact sums e64 [rows, C] (see the module docstring)."""
    import norm_cases as NC
    ref, g = NC.gate_layernorm(e64, gamma, beta, eps, dtype)
    de = U32 * e64.abs()
    mean = e64.mean(-1, keepdim=True)
    var = ((e64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dev = (e64 - mean).abs()
    extra = gamma.double().abs() * rstd * (de + de.mean(-1, keepdim=True) + dev * rstd * rstd * (dev * de).mean(-1, keepdim=True))
    return ref, g + (1.0 + NC.unit_roundoff(dtype)) * extra


def save_tiny_checkpoint(folder, hf) -> None:
    """config.json + model.safetensors of `hf` in `folder` (the layout `from_pretrained(local_dir)` reads)."""
    import json
    import os
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    cfg = {k: v for k, v in hf.config.to_dict().items() if isinstance(v, (int, float, str, bool, type(None)))}
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in hf.state_dict().items()}, os.path.join(folder, "model.safetensors"))
