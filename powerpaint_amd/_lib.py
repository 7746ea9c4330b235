"""ctypes binding of libpp_hip.so (the C ABI declared in include/pp_hip.h).

The product path has NO fallback: if the shared library is missing this module raises at import of the symbols
(`lib()`), and every op raises on a non-zero return code.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpp_hip.so")
if os.environ.get("PP_LAB") == "1" and os.environ.get("PP_LIB"):      # lab: A/B against a variant build (csrc/Makefile)
    LIB_PATH = os.path.abspath(os.environ["PP_LIB"])

PP_X_PLAIN, PP_X_CONV3X3 = 0, 1
PP_ACT_NONE, PP_ACT_GEGLU, PP_ACT_SILU, PP_ACT_SOFTMAX80, PP_ACT_GELU = 0, 1, 2, 3, 4
PP_TILE_AUTO, PP_TILE_128x160, PP_TILE_64x160, PP_TILE_256x160 = 0, 1, 2, 3
PP_DT_F32, PP_DT_BF16, PP_DT_F16 = 0, 1, 2      # dtype codes of the C ABI (include/pp_hip.h)
PP_ATTN_AUTO, PP_ATTN_PHASED, PP_ATTN_PIPE_Q32, PP_ATTN_PIPE_Q64, PP_ATTN_PIPE_LOG2 = 0, 1, 2, 3, 4   # pp_attention_fwd_variant
ABI_VERSION = 29                                  # PP_ABI_VERSION of include/pp_hip.h this binding was written against
PP_ERR = {0: "PP_OK", -1: "PP_ERR_BAD_ARG", -2: "PP_ERR_UNSUPPORTED", -3: "PP_ERR_LAUNCH", -4: "PP_ERR_WORKSPACE"}

vp, i32, f32, sz = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


class PPGemmArgs(C.Structure):
    _fields_ = [
        ("M", i32), ("N", i32), ("K", i32), ("x_mode", i32),
        ("x1", vp), ("x2", vp),
        ("c1", i32), ("c2", i32), ("ldx1", i32), ("ldx2", i32),
        ("batch", i32), ("hin", i32), ("win", i32), ("hout", i32), ("wout", i32), ("stride", i32), ("up", i32),
        ("w", vp), ("bias", vp), ("rowvec", vp),
        ("ld_rowvec", i32), ("rows_per_batch", i32),
        ("res1", vp), ("ldres1", i32),
        ("res2", vp), ("ldres2", i32),
        ("scale", f32), ("act", i32),
        ("out", vp), ("ldo", i32), ("out_f32", i32),
        ("out_vt", vp), ("vt_col0", i32), ("vt_ld", i32),
        ("splitk", i32), ("tile", i32),
        ("workspace", vp),
        ("dbg", i32), ("dtype", i32), ("out_dup_rows", i32), ("res1_wrap_rows", i32),
        ("row_stats_out", vp), ("ln_stats", vp), ("ln_colsum", vp),
        ("ln_tiles", i32), ("ln_dim", i32), ("ln_eps", f32), ("w_batch_stride", i32),
        ("gn_acc", vp * 2), ("gn_cg", i32 * 2), ("gn_c0", i32 * 2), ("gn_groups", i32 * 2),
        ("x3", vp), ("x4", vp), ("c3", i32), ("c4", i32),
        ("gn_in_acc", vp), ("gn_in_gb", vp), ("gn_in_groups", i32), ("gn_in_silu", i32), ("gn_in_eps", f32),
        ("gn_dup_batch", i32),
        ("gn_next_out", vp), ("gn_next_gamma", vp), ("gn_next_beta", vp), ("gn_next_eps", f32), ("gn_next_silu", i32),
        ("gn_next_sub", i32), ("gn_dup_mask", i32), ("vec_batch_stride", i32),
        ("tile_ctr", vp), ("combine_fault", vp),
        ("subpix", i32),
        ("tile_group_m", i32),
    ]


def gemm_args(dtype: int, M: int, N: int, K: int, x, w, out, x2=None, K2: int = 0, ldx=None, ldx2: int = 0, ldo: int = 0,
              ldres1: int = 0, ldres2: int = 0, rows_per_batch: int = 0, scale: float = 1.0) -> PPGemmArgs:
    """The geometry of a PP_X_PLAIN request, out[M][N] = epilogue(concat(x[M][K], x2[M][K2]) @ w[N][K + K2]^T), from raw
    pointers and integers; leading dimensions default to dense rows.  The caller adds what is its own: epilogue operands,
    tile / split wishes, subscriptions, workspace."""
    a = PPGemmArgs()
    a.dtype = dtype
    a.M, a.N, a.K, a.x_mode = M, N, K + K2, PP_X_PLAIN
    a.x1, a.x2, a.c1, a.c2 = x, x2 or None, K, K2
    a.ldx1, a.ldx2 = (K if ldx is None else ldx), (ldx2 or K2)
    a.w, a.out = w, out
    a.ldo, a.ldres1, a.ldres2 = ldo or N, ldres1 or N, ldres2 or N
    a.rows_per_batch, a.scale = rows_per_batch, scale
    return a


def conv3x3_args(dtype: int, B: int, H: int, W: int, c1: int, cout: int, x, x2=None, c2: int = 0, x3=None, c3: int = 0,
                 x4=None, c4: int = 0, stride: int = 1, up: bool = False, w=None, out=None, scale: float = 1.0,
                 up_size=None) -> PPGemmArgs:
    """The geometry of a PP_X_CONV3X3 request: conv3x3 (padding 1) over concat(x, x2) NHWC [B][H][W][c1 + c2], after a nearest
    2x upsample if `up`, + a 1x1 tail over concat(x3, x4) at the output pixel -> NHWC [B][hout][wout][cout] (a.hout / a.wout:
    a caller that sizes `out` from them sets a.out afterwards).  up_size = (h, w) with `up`: the nearest resize goes to that
    size instead, 2 H - 1 or 2 H rows and 2 W - 1 or 2 W columns (F.interpolate(size=...) of Upsample2D)."""
    hv, wv = (2 * H, 2 * W) if up else (H, W)
    if up_size is not None:
        if not up or stride != 1 or up_size[0] not in (2 * H - 1, 2 * H) or up_size[1] not in (2 * W - 1, 2 * W):
            raise ValueError(f"up_size {tuple(up_size)} is no nearest-resize target of a {H}x{W} source")
        hv, wv = up_size
    ho, wo = (hv - 1) // stride + 1, (wv - 1) // stride + 1
    a = PPGemmArgs()
    a.dtype = dtype
    a.M, a.N, a.K, a.x_mode = B * ho * wo, cout, 9 * (c1 + c2) + c3 + c4, PP_X_CONV3X3
    a.x1, a.x2, a.c1, a.c2 = x, x2 or None, c1, c2
    a.x3, a.x4, a.c3, a.c4 = x3 or None, x4 or None, c3, c4
    a.batch, a.hin, a.win, a.hout, a.wout, a.stride, a.up = B, H, W, ho, wo, stride, int(up)
    a.w, a.out = w, out
    a.ldo, a.ldres1, a.ldres2 = cout, cout, cout
    a.rows_per_batch, a.scale = ho * wo, scale
    return a


PP_LORA_MAX_ADAPTERS, PP_LORA_MAX_RANK = 8, 128
PP_LORA_ROWS_PLAIN, PP_LORA_ROWS_GEGLU = 0, 1
PP_TOME_MAX_TOKENS = 16384            # tokens per batch item the pp_tome_* entries take (include/pp_hip.h)
PP_IP_MAX_TOKENS = 64                 # image tokens per adapter pp_ip_attn_add takes (include/pp_hip.h)
PP_LORA_COLS_PLAIN, PP_LORA_COLS_IGEMM, PP_LORA_COLS_KPERM, PP_LORA_COLS_KPERM_GEGLU = 0, 1, 2, 3


class PPLoraMergeArgs(C.Structure):
    _fields_ = [
        ("N", i32), ("K", i32), ("w", vp), ("ldw", C.c_int64), ("n_adapters", i32),
        ("rank", i32 * PP_LORA_MAX_ADAPTERS), ("coef", f32 * PP_LORA_MAX_ADAPTERS),
        ("up", vp * PP_LORA_MAX_ADAPTERS), ("down", vp * PP_LORA_MAX_ADAPTERS),
        ("gamma", vp), ("beta", vp), ("badd", vp),
        ("out", vp), ("ldo", C.c_int64), ("out_rows", i32), ("out_cols", i32), ("out_dtype", i32),
        ("row_mode", i32), ("row_off", i32), ("col_mode", i32), ("col_off", i32), ("taps", i32), ("cin_pad", i32),
        ("colsum", vp), ("bias", vp),
    ]


# name -> (restype, argtypes); must list every symbol of include/pp_hip.h (tests/test_abi.py checks the header)
SIGNATURES = {
    "pp_abi_version": (C.c_int, []),
    "pp_last_error": (C.c_char_p, []),
    "pp_build_id": (C.c_char_p, []),
    "pp_gemm_bf16": (C.c_int, [C.POINTER(PPGemmArgs), vp]),
    "pp_gemm_workspace_bytes": (sz, [C.POINTER(PPGemmArgs)]),
    "pp_linear_skinny": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "pp_timestep_embedding": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "pp_groupnorm_workspace_bytes": (sz, [C.c_int, C.c_int, C.c_int]),
    "pp_gemm_gn_stats_ok": (C.c_int, [C.POINTER(PPGemmArgs)]),
    "pp_conv_gn_supported": (C.c_int, [C.POINTER(PPGemmArgs)]),
    "pp_conv_gn_preferred": (C.c_int, [C.POINTER(PPGemmArgs)]),
    "pp_gemm_gn_next_ok": (C.c_int, [C.POINTER(PPGemmArgs), C.c_int]),
    "pp_upconv_subpix_supported": (C.c_int, [C.c_int] * 6),
    "pp_upconv_subpix_supported_to": (C.c_int, [C.c_int] * 8),
    "pp_upconv_fold": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "pp_gemm_combine_ctr_bytes": (sz, [C.POINTER(PPGemmArgs)]),
    "pp_gemm_combine_fused": (C.c_int, [C.POINTER(PPGemmArgs)]),
    "pp_gemm_tile_group_m": (C.c_int, [C.POINTER(PPGemmArgs)]),
    "pp_xcd_placement_ok": (C.c_int, []),
    "pp_groupnorm_apply_acc": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp, vp, vp, C.c_int, vp,
                                         C.c_int, vp]),
    "pp_zero_u64": (C.c_int, [vp, C.c_longlong, vp]),
    "pp_embed_splice": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_longlong, vp]),
    "pp_attention_small": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, f32, C.c_int, C.c_int, vp]),
    "pp_softmax_rows": (C.c_int, [vp, C.c_longlong, C.c_int, C.c_int, f32, vp, C.c_longlong, C.c_int, vp]),
    "pp_groupnorm_stats": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_groupnorm_apply": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp, vp, vp, C.c_int, vp,
                                     C.c_int, vp]),
    "pp_layernorm": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, f32, vp, C.c_int, vp]),
    "pp_attention_fwd": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, f32, C.c_int, vp]),
    "pp_attention_fwd_variant": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, f32, C.c_int, C.c_int, vp]),
    "pp_attention_tiled_ok": (C.c_int, [C.c_int] * 5),
    "pp_attention_fwd_tiled": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, f32, C.c_int, C.c_int, vp]),
    "pp_transpose_v": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_conv3x3_direct": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp,
                                    vp, C.c_int, vp]),
    "pp_conv3x3_smallcout": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]),
    "pp_nchw_to_nhwc": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "pp_nhwc_to_nchw": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
    "pp_vit_patchify": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "pp_vit_embed_ln": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, f32, vp, C.c_int, vp]),
    "pp_add_bf16": (C.c_int, [vp, vp, vp, C.c_longlong, C.c_int, vp]),
    "pp_cfg_sched_step": (C.c_int, [vp, C.c_int, f32, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "pp_step_select_t": (C.c_int, [vp, vp, vp, vp]),
    "pp_ddim_variance_noise": (C.c_int, [vp, vp, C.c_int, vp, vp, vp]),
    "pp_cfg_lcm_step": (C.c_int, [vp, C.c_int, f32, vp, vp, C.c_int, vp, vp, vp, vp]),
    "pp_cfg_sigma_step": (C.c_int, [vp, C.c_int, f32, vp, vp, C.c_int, vp, vp, vp, vp]),
    "pp_cfg_ksampler_step": (C.c_int, [vp, C.c_int, f32, vp, vp, vp, C.c_int, vp, vp, vp, vp]),
    "pp_latent_blend": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "pp_gn_conv3x3_smallcout_supported": (C.c_int, [C.c_int] * 3),
    "pp_gn_conv3x3_smallcout": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp,
                                          C.c_int, vp, C.c_int, vp]),
    "pp_tfront_supported": (C.c_int, [C.c_int] * 4),
    "pp_tfront": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_float, C.c_int, vp, vp, vp, vp, vp, C.c_float, vp, C.c_int, vp, C.c_int,
                            vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp]),
    "pp_attention_log2_ok": (C.c_int, [C.c_int] * 3),
    "pp_xattn_block_supported": (C.c_int, [C.c_int] * 5),
    "pp_xattn_fold": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_float,
                                vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "pp_xattn_block": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp, C.c_int, vp,
                                 C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "pp_ff_fused_supported": (C.c_int, [C.c_int] * 3),
    "pp_ff_fused": (C.c_int, [C.POINTER(PPGemmArgs), vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp]),
    "pp_step_head": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp,
                              C.c_longlong, vp]),
    "pp_step_head_scaled": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                     vp, C.c_longlong, vp, vp]),
    "pp_step_advance": (C.c_int, [vp, vp]),
    "pp_lora_merge": (C.c_int, [C.POINTER(PPLoraMergeArgs), vp]),
    "pp_freeu": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "pp_mask_prep": (C.c_int, [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "pp_ip_attn_add": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32, f32,
                                 C.c_int, vp]),
    "pp_ip_attn_add_masked": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32, f32,
                                        vp, C.c_int, vp]),
    "pp_perceiver_attn": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, f32, C.c_int, vp]),
    "pp_tome_supported": (C.c_int, [C.c_int] * 5),
    "pp_tome_match": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp,
                                vp, C.c_int, vp]),
    "pp_tome_select": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "pp_tome_merge": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int,
                                vp, C.c_int, C.c_int, vp]),
    "pp_tome_unmerge": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_attn_identity_v": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_pag_combine": (C.c_int, [vp, C.c_int, f32, vp, vp, C.c_int, vp]),
    "pp_cfg_rescale": (C.c_int, [vp, C.c_int, f32, vp, vp, vp, C.c_int, C.c_int, vp]),
    "pp_conv4x4s2": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_relu": (C.c_int, [vp, vp, C.c_longlong, C.c_int, vp]),
    "pp_masked_image_pack": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_mask_blend": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
    "pp_conv3x3_c64": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "pp_taesd_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
}

_lib = None


class PPError(RuntimeError):
    pass


def lib():
    """Load libpp_hip.so (once).  Raises loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PPError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (or `make -C powerpaint_amd/csrc`). There is no CPU/PyTorch fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        if l.pp_abi_version() != ABI_VERSION:
            raise PPError("libpp_hip.so ABI version mismatch")
        _lib = l
    return _lib


def dtype_code(dtype) -> int:
    """torch 16-bit dtype -> PP_DT_* (the HIP path stores activations and matrix weights in bf16 or fp16)."""
    import torch
    if dtype == torch.bfloat16:
        return PP_DT_BF16
    if dtype == torch.float16:
        return PP_DT_F16
    raise PPError(f"the HIP path computes in bf16 or fp16 (fp32 accumulate), not {dtype}")


def build_id() -> str:
    """What the loaded library was built from (pp_build_id: digest of sources + headers + extra flags)."""
    return lib().pp_build_id().decode()


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().pp_last_error().decode() if rc == -3 else ""
        raise PPError(f"{what} failed: {PP_ERR.get(rc, rc)} {msg}")
