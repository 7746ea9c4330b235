"""CLIP vision tower (transformers.CLIPVisionModelWithProjection, the `image_encoder` of an IP-Adapter pipeline) compiled to a
HIP launch plan -- the sibling of `clip.py`.  ViT-H/14 is the tower every SD-1.5 IP-Adapter ships with: 1280 hidden, 16 heads of
80, 257 tokens at 224 x 224.

Front (csrc/vit.hip around one GEMM):
    rows = patchify(pixels)                    pp_vit_patchify: the im2col rows of the stride-P patch conv, K = 3 P P zero-padded
                                               to a multiple of 64 (588 -> 640 for P = 14)
    e    = rows @ W_patch^T                    pp_gemm_bf16 (no bias; the conv weight flattened, zero-padded along K)
    x0   = pre_layrnorm([class | e] + pos)     pp_vit_embed_ln (the fp32 sum is not rounded before the norm) = hidden state 0
Per layer (pre-LN transformer, no mask, exact GELU), eight launches:
    h  = x + out_proj(attn(LN1(x)))            pp_layernorm, pp_gemm_bf16 (fused q|k|v, N = 3C), pp_transpose_v,
                                               pp_attention_fwd (d = 80, ldvt = tokens rounded up to 8),
                                               pp_gemm_bf16 (+ residual in the epilogue)
    x' = h + fc2(gelu(fc1(LN2(h))))            pp_layernorm, pp_gemm_bf16 (PP_ACT_GELU epilogue), pp_gemm_bf16 (+ residual)
V^T comes from pp_transpose_v, not from the QKV GEMM's out_vt epilogue.  The epilogue accepts rows_per_batch = 257, but only on
its element-wise branch (2-byte stores a V^T row apart instead of 16-byte ones), and it leaves columns [257, 264) of V^T
unwritten, which pp_attention_fwd wants finite; pp_transpose_v writes them as zeros and is the documented fallback for token
counts off the 8 grid (the rule engine.py's self-attention follows).  A square grid's k^2 + 1 tokens are never on it (squares
are 0, 1 or 4 mod 8), so the tower has this one form.
Back:
    pooled = post_layernorm(x_L[:, 0])         pp_layernorm on the class-token row of each image (one launch per image)
    image_embeds = pooled @ W_proj^T           pp_gemm_bf16 (no bias)
"""
from typing import Dict, Optional

import torch

from . import _lib as L
from .engine import Arena, Builder, ParamPack, Plan, _align

HEAD_DIMS = (40, 80, 160)          # pp_attention_fwd


class CLIPVisionNet:
    def __init__(self, hidden_size: int = 1280, intermediate_size: int = 5120, num_hidden_layers: int = 32,
                 num_attention_heads: int = 16, image_size: int = 224, patch_size: int = 14, projection_dim: int = 1024,
                 layer_norm_eps: float = 1e-5):
        self.C, self.F, self.n_layers, self.heads = hidden_size, intermediate_size, num_hidden_layers, num_attention_heads
        self.image_size, self.patch, self.proj, self.eps = image_size, patch_size, projection_dim, layer_norm_eps
        d = hidden_size // num_attention_heads
        if hidden_size % num_attention_heads or d not in HEAD_DIMS:
            raise L.PPError(f"CLIPVisionModelWithProjection: head_dim {hidden_size}/{num_attention_heads} is not implemented on the "
                            f"HIP path (pp_attention_fwd takes {', '.join(map(str, HEAD_DIMS))}: ViT-H/14 runs; ViT-L/14 with "
                            f"head_dim 64 and ViT-bigG/14 with head_dim 104 do not)")
        if hidden_size % 64 or intermediate_size % 64:
            raise L.PPError(f"CLIPVisionModelWithProjection: hidden_size {hidden_size} / intermediate_size {intermediate_size} "
                            f"must be multiples of 64 (the GEMM's K)")
        if hidden_size > 2048:
            raise L.PPError(f"CLIPVisionModelWithProjection: hidden_size {hidden_size} > 2048 (pp_layernorm)")
        if projection_dim % 8 or patch_size <= 0 or image_size < patch_size:
            raise L.PPError(f"CLIPVisionModelWithProjection: projection_dim {projection_dim} must be a multiple of 8 and "
                            f"patch_size {patch_size} must fit image_size {image_size}")
        self.d = d
        self.Kp = _align(3 * patch_size * patch_size, 64)           # K of the patch GEMM
        self.n_pos = (image_size // patch_size) ** 2 + 1
        self.params: Optional[ParamPack] = None
        self.P: Dict[str, int] = {}

    def pack(self, sd: Dict[str, torch.Tensor], device):
        """sd: `embeddings.*`, `pre_layrnorm.*`, `encoder.layers.{i}.*`, `post_layernorm.*` (the keys below `vision_model.`)
        and `visual_projection.weight`."""
        pk = ParamPack()
        bf, f32 = torch.bfloat16, torch.float32

        def W(k):
            return sd[k].detach().float()

        wp = W("embeddings.patch_embedding.weight").reshape(self.C, -1)               # [C][3 P P]: c, ky, kx
        pk.add("patch.weight", torch.nn.functional.pad(wp, (0, self.Kp - wp.shape[1])), bf)
        pk.add("cls", W("embeddings.class_embedding").reshape(self.C), bf)
        pk.add("pos", W("embeddings.position_embedding.weight"), bf)
        for n in ("pre_layrnorm", "post_layernorm"):
            pk.add(f"{n}.weight", W(f"{n}.weight"), f32)
            pk.add(f"{n}.bias", W(f"{n}.bias"), f32)
        for i in range(self.n_layers):
            p = f"encoder.layers.{i}"
            for n in ("layer_norm1", "layer_norm2"):
                pk.add(f"{p}.{n}.weight", W(f"{p}.{n}.weight"), f32)
                pk.add(f"{p}.{n}.bias", W(f"{p}.{n}.bias"), f32)
            pk.add(f"{p}.qkv.weight", torch.cat([W(f"{p}.self_attn.{n}_proj.weight") for n in "qkv"], 0), bf)
            pk.add(f"{p}.qkv.bias", torch.cat([W(f"{p}.self_attn.{n}_proj.bias") for n in "qkv"], 0), f32)
            pk.add(f"{p}.out.weight", W(f"{p}.self_attn.out_proj.weight"), bf)
            pk.add(f"{p}.out.bias", W(f"{p}.self_attn.out_proj.bias"), f32)
            for n in ("fc1", "fc2"):
                pk.add(f"{p}.{n}.weight", W(f"{p}.mlp.{n}.weight"), bf)
                pk.add(f"{p}.{n}.bias", W(f"{p}.mlp.{n}.bias"), f32)
        pk.add("visual_projection.weight", W("visual_projection.weight"), bf)
        pk.to_device(device)
        self.params, self.P = pk, pk.ptr
        return self

    def tokens(self, H: int, W: int) -> int:
        n = (H // self.patch) * (W // self.patch) + 1
        if H < self.patch or W < self.patch or n != self.n_pos:
            raise L.PPError(f"CLIPVisionModelWithProjection: a {H}x{W} image makes {n} tokens, the position table has "
                            f"{self.n_pos} (image_size {self.image_size}, patch_size {self.patch}); position embeddings are not "
                            f"interpolated")
        return n

    def build(self, pb: Builder, pix: int, B: int, H: int, W: int) -> int:
        """pix: fp32 pixels NCHW [B][3][H][W]; returns the pointer of image_embeds [B][projection_dim] (bf16).  Leaves
        `self.hidden` (transformers' `hidden_states`: pre_layrnorm's output and every layer's) and `self.pooled`."""
        P, Cc, d = self.P, self.C, self.d
        n = self.tokens(H, W)
        rows, npatch = B * n, n - 1
        x = pb.alloc(rows * Cc * 2)                          # (persistent: the hidden states are allocated before any scratch)
        m = pb.mark()
        col = pb.alloc(B * npatch * self.Kp * 2)
        pb.plan.add("vit_patchify", pb.lib.pp_vit_patchify, pix, L.PP_DT_F32, B, H, W, self.patch, col, self.Kp, self.Kp, pb.dt)
        e = pb.linear(col, B * npatch, self.Kp, P["patch.weight"], Cc, name="linear")
        pb.plan.add("vit_embed_ln", pb.lib.pp_vit_embed_ln, e, Cc, P["cls"], P["pos"], B, npatch, Cc, P["pre_layrnorm.weight"],
                    P["pre_layrnorm.bias"], self.eps, x, pb.dt)
        pb.release(m)
        self.hidden = [x]
        ldvt = _align(n, 8)
        for i in range(self.n_layers):
            p = f"encoder.layers.{i}"
            nxt = pb.alloc(rows * Cc * 2)                    # (persistent, like x: `output_hidden_states=True` is free)
            m = pb.mark()
            mid = pb.alloc(rows * Cc * 2)
            h = pb.layernorm(x, rows, Cc, P[f"{p}.layer_norm1.weight"], P[f"{p}.layer_norm1.bias"], self.eps)
            vt = pb.alloc(B * Cc * ldvt * 2)
            qkv = pb.linear(h, rows, Cc, P[f"{p}.qkv.weight"], 3 * Cc, P[f"{p}.qkv.bias"], name="linear")
            pb.plan.add("transpose_v", pb.lib.pp_transpose_v, qkv + 4 * Cc, 3 * Cc, B, n, Cc, vt, ldvt)
            a = pb.attention(qkv, 3 * Cc, qkv + 2 * Cc, 3 * Cc, vt, ldvt, B, self.heads, n, n, d)
            pb.linear(a, rows, Cc, P[f"{p}.out.weight"], Cc, P[f"{p}.out.bias"], res1=x, out=mid, name="linear")
            h = pb.layernorm(mid, rows, Cc, P[f"{p}.layer_norm2.weight"], P[f"{p}.layer_norm2.bias"], self.eps)
            f = pb.linear(h, rows, Cc, P[f"{p}.fc1.weight"], self.F, P[f"{p}.fc1.bias"], act=L.PP_ACT_GELU, name="linear")
            pb.linear(f, rows, self.F, P[f"{p}.fc2.weight"], Cc, P[f"{p}.fc2.bias"], res1=mid, out=nxt, name="linear")
            pb.release(m)
            x = nxt
            self.hidden.append(x)
        # post_layernorm on the class-token row of each image only (pp_layernorm takes contiguous rows: one launch per image)
        self.pooled = pb.alloc(B * Cc * 2)
        for b in range(B):
            pb.plan.add("layernorm", pb.lib.pp_layernorm, x + b * n * Cc * 2, 1, Cc, P["post_layernorm.weight"],
                        P["post_layernorm.bias"], self.eps, self.pooled + b * Cc * 2, pb.dt)
        return pb.linear(self.pooled, B, Cc, P["visual_projection.weight"], self.proj, name="linear")


class CLIPVisionRuntime:
    def __init__(self, net: CLIPVisionNet, device):
        self.net, self.device = net, torch.device(device)
        self.key = None
        self.plan: Optional[Plan] = None
        self.arena: Optional[Arena] = None

    def _build(self, arena: Arena, B: int, H: int, W: int):
        pb = Builder(arena)
        pix = arena.alloc(B * 3 * H * W * 4)
        out = self.net.build(pb, pix, B, H, W)
        return pix, out, pb.plan

    def ensure(self, B: int, H: int, W: int):
        if (B, H, W) == self.key:
            return
        dry = Arena()
        self._build(dry, B, H, W)
        self.arena = Arena(_align(dry.peak, 4096), self.device)
        self.pix, self.out, self.plan = self._build(self.arena, B, H, W)
        self.hidden, self.pooled = list(self.net.hidden), self.net.pooled
        self.n = self.net.tokens(H, W)
        self.key = (B, H, W)

    def hidden_states(self, last_only: bool = False):
        """transformers' `hidden_states` of the last `run` (pre_layrnorm's output + one tensor per layer), as copies (the
        arena is overwritten by the next call); last_only: the last layer's alone."""
        B = self.key[0]
        return tuple(self.arena.view(p, (B, self.n, self.net.C), torch.bfloat16).clone()
                     for p in (self.hidden[-1:] if last_only else self.hidden))

    def pooled_output(self):
        return self.arena.view(self.pooled, (self.key[0], self.net.C), torch.bfloat16).clone()

    def run(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values [B, 3, H, W] (any float dtype, on the device) -> image_embeds [B, projection_dim] bf16 (arena view)."""
        B, ch, H, W = pixel_values.shape
        if ch != 3:
            raise ValueError(f"pixel_values must be [B, 3, H, W], got {tuple(pixel_values.shape)}")
        self.ensure(B, H, W)
        self.arena.view(self.pix, (B, 3, H, W), torch.float32).copy_(pixel_values)
        self.plan.run(torch.cuda.current_stream().cuda_stream)
        return self.arena.view(self.out, (B, self.net.proj), torch.bfloat16)
