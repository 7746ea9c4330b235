"""Tensor-level convenience wrappers over the C ABI (one call = one kernel launch family).

These take/return torch CUDA tensors (bf16 NHWC / row-major activations) and exist for tests, micro-benchmarks and
users who want a single op; the networks themselves go through `engine.Builder`, which bakes raw pointers into plans.
Every wrapper raises `PPError` on a non-zero return code -- there is no fallback.
"""
import ctypes as C
from typing import Optional

import torch

from . import _lib as L

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _set_gn(a, gn, rows_per_batch):
    """gn: up to two (acc int64 [B][groups][2] (zeroed by the caller), channels_per_group, channel_offset, groups)."""
    if not gn:
        return
    a.rows_per_batch = rows_per_batch
    for k, (acc, cg, c0, groups) in enumerate(gn):
        a.gn_acc[k], a.gn_cg[k], a.gn_c0[k], a.gn_groups[k] = acc.data_ptr(), cg, c0, groups


# (ABI v21) the in-kernel split-K combine: `fuse_combine=True` on gemm / conv3x3 hands the launch zeroed tile counters where
# pp_gemm_combine_ctr_bytes() asks for them.  `last_combine` describes the most recent such call: fused (did pp_gemm_bf16
# combine in-kernel), ctr (the counters: all zero again after the launch), and combine_faults() reads the fault counter.
last_combine = {"fused": False, "ctr": None}
_fault_words = {}


def _fault_word(device) -> torch.Tensor:
    key = torch.device(device)
    if key not in _fault_words:
        _fault_words[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _fault_words[key]


def combine_faults(device) -> int:
    """Split-K tiles whose splits did NOT share an XCD since the process started (synchronises; must stay 0)."""
    return int(_fault_word(device).item())


def _attach_combine(a, device, enable):
    """enable: False / None -- no counters; True -- where pp_gemm_combine_ctr_bytes() advises them; "force" -- also where the
    library advises the separate combine (large tiles); a tensor -- the caller's own (zeroed or re-armed) counters."""
    last_combine["fused"], last_combine["ctr"] = False, None
    if enable is None or enable is False:
        return
    bound = ((a.M + 127) // 128) * ((a.N + 159) // 160) * 16      # 16 bytes per 128 x 160 tile always suffice
    if torch.is_tensor(enable):
        ctr = enable
        assert ctr.dtype == torch.int64 and ctr.numel() * 8 >= bound
    else:
        n = L.lib().pp_gemm_combine_ctr_bytes(C.byref(a))
        if enable == "force":
            n = max(n, bound)
        if not n:
            return
        ctr = torch.zeros(n // 8, dtype=torch.int64, device=device)
    a.tile_ctr, a.combine_fault = ctr.data_ptr(), _fault_word(device).data_ptr()
    last_combine["ctr"] = ctr
    last_combine["fused"] = bool(L.lib().pp_gemm_combine_fused(C.byref(a)))


def _norm_out(out, shape, like: torch.Tensor, what: str) -> torch.Tensor:
    """The output of the norm wrappers: a new tensor, or `out` -- a contiguous tensor (or view into a larger buffer) of the
    result's shape and the inputs' format; the kernels take no row stride.  Elements outside it are the caller's."""
    if out is None:
        return torch.empty(*shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.dtype != like.dtype or out.device != like.device:
        raise L.PPError(f"{what}: `out` must be a contiguous {list(shape)} tensor of the inputs' format")
    return out


def _view2d(t, rows: int, cols: int, dtype, like: torch.Tensor, what: str) -> torch.Tensor:
    """A caller-owned [rows, cols] output: any 2-D view with unit column stride (a window of a larger buffer); its row stride
    is the leading dimension the kernel gets.  Elements outside the view are the caller's."""
    if (t.dim() != 2 or tuple(t.shape) != (rows, cols) or t.stride(1) != 1 or t.stride(0) < cols or t.dtype != dtype
            or t.device != like.device):
        raise L.PPError(f"{what}: must be a [{rows}, {cols}] row-major view (unit column stride) of the output format")
    return t


def _rows_in(t, cols: int, like: torch.Tensor, what: str) -> int:
    """Row stride of a strided 2-D input [rows, cols] (a window of a larger buffer): unit column stride, rows that do not
    overlap, the format and device of `like`.  What lies in the pad columns is never read."""
    if t.dim() != 2 or t.shape[1] != cols or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < cols) or t.dtype != like.dtype \
            or t.device != like.device:
        raise L.PPError(f"{what}: must be a [rows, {cols}] row-major view (unit column stride) of the inputs' format")
    return t.stride(0) if t.shape[0] > 1 else cols


def _exact(t, shape, dtype, like: torch.Tensor, what: str) -> torch.Tensor:
    """A caller-owned output the ABI has no stride for: contiguous, of exactly this shape and format."""
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.dtype != dtype or t.device != like.device:
        raise L.PPError(f"{what}: must be a contiguous {list(shape)} tensor of {dtype}")
    return t


def _vt_window(t, nb: int, cols: int, rows: int, like: torch.Tensor, what: str) -> torch.Tensor:
    """A caller-owned V^T output: a [nb, cols, rows] window of a contiguous [nb, cols, ld] buffer (ld = the view's stride(1))."""
    if (t.dim() != 3 or tuple(t.shape) != (nb, cols, rows) or t.stride(2) != 1 or t.dtype != like.dtype or t.device != like.device
            or t.stride(1) < rows or (nb > 1 and t.stride(0) != cols * t.stride(1))):
        raise L.PPError(f"{what}: must be a [{nb}, {cols}, {rows}] window of a contiguous [nb, cols, ld] buffer of the inputs' format")
    return t


def _nhwc_view(t, shape, like: torch.Tensor, what: str) -> torch.Tensor:
    """A caller-owned NHWC conv output [B, H, W, C]: dense pixels whose channel stride (the kernel's ldo) is the view's pixel
    stride, i.e. a column window of a [B*H*W, ldo] buffer."""
    B, H, W, Cc = shape
    bad = t.dim() != 4 or tuple(t.shape) != tuple(shape) or t.stride(3) != 1 or t.dtype != like.dtype or t.device != like.device
    if not bad:                      # (the stride of a dimension of size 1 is arbitrary: the pixel stride comes from the first that counts)
        ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else Cc))
        bad = (ld < Cc or (W > 1 and H > 1 and t.stride(1) != W * ld) or (B > 1 and H * W > 1 and t.stride(0) != H * W * ld))
    if bad:
        raise L.PPError(f"{what}: must be a {list(shape)} NHWC view of the inputs' format with dense pixels (channel stride = ld)")
    return t


def _nhwc_ld(t, shape) -> int:
    B, H, W, Cc = shape
    return t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else Cc))


def _res_ld(t, shape, like: torch.Tensor, what: str, rows_only: bool = False) -> int:
    """Pixel stride (ldres) of a conv residual: an NHWC tensor of `shape` (the request's output; rows_only: any number of
    leading rows, as res1 with res1_wrap holds) of the inputs' format with dense pixels, checked as `out` is."""
    if t is None:
        return shape[3]
    if t.dim() == 2:                 # rows x channels: the same tensor, flattened
        if t.shape[1] != shape[3] or t.stride(1) != 1 or t.dtype != like.dtype or t.device != like.device or \
                (not rows_only and t.shape[0] != shape[0] * shape[1] * shape[2]):
            raise L.PPError(f"{what}: must be [{shape[0] * shape[1] * shape[2]}, {shape[3]}] rows of the inputs' format")
        return t.stride(0) if t.shape[0] > 1 else shape[3]
    if rows_only:
        shape = tuple(t.shape[:3]) + (shape[3],) if t.dim() == 4 else shape
    _nhwc_view(t, shape, like, what)
    return _nhwc_ld(t, shape)


last_workspace = {"bytes": 0}     # what pp_gemm_workspace_bytes() asked for the most recent gemm / conv call


def _workspace(lib, a, device, workspace):
    """The split-K workspace of request `a`: a new buffer, or the caller's fp32 tensor (contiguous, large enough)."""
    ws = lib.pp_gemm_workspace_bytes(C.byref(a))
    last_workspace["bytes"] = ws
    if workspace is None:
        return torch.empty(max(ws, 4) // 4, dtype=torch.float32, device=device) if ws else None
    if (workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != device
            or workspace.numel() * 4 < ws):
        raise L.PPError(f"`workspace` must be a contiguous fp32 tensor of at least {ws} bytes on the inputs' device")
    return workspace if ws else None


def groupnorm_apply_acc(x: torch.Tensor, acc: torch.Tensor, gamma, beta, eps: float, silu: bool, groups: int = 32,
                        x2=None, out: Optional[torch.Tensor] = None):
    """GroupNorm(+SiLU) of concat(x, x2) from statistics accumulated by the producers (PPGemmArgs.gn_acc).
    out: see _norm_out."""
    B, H, W, C1 = x.shape
    C2 = x2.shape[3] if x2 is not None else 0
    y = _norm_out(out, (B, H, W, C1 + C2), x, "groupnorm_apply_acc")
    L.check(L.lib().pp_groupnorm_apply_acc(_p(x), C1, _p(x2), C2, B, H * W, groups, eps, _p(gamma), _p(beta), _p(acc),
                                           int(silu), _p(y), L.dtype_code(x.dtype), _s()), "pp_groupnorm_apply_acc")
    return y


def gemm(x: torch.Tensor, w: torch.Tensor, bias=None, x2=None, res1=None, res2=None, scale: float = 1.0, act: int = 0,
         rowvec=None, rows_per_batch: int = 0, out_f32: bool = False, vt_col0: int = 0, tile: int = 0,
         splitk: int = 0, tile_group_m: int = 0, row_stats: bool = False, ln_stats=None, ln_colsum=None, ln_dim: int = 0,
         ln_eps: float = 1e-5, gn=None, res1_wrap: int = 0, fuse_combine: bool = False, out=None, vt=None, stats=None,
         workspace=None):
    """x [M,K1] (+ x2 [M,K2]) bf16, w [N,K1+K2] bf16 -> out [M,N] (or [M,N/2] for GEGLU; (out, vt) when vt_col0).
    out: write into this tensor instead of a new one -- any [M, n_out] view with unit column stride, its row stride is the
    ldo of the launch (a window of a larger buffer; what lies outside it is the caller's); it may BE res1 (in place,
    include/pp_hip.h "Aliasing").  vt: the caller's V^T output, a [nb, N - vt_col0, rows_per_batch] window of a contiguous
    [nb, N - vt_col0, vt_ld] buffer; stats: the caller's row moments, contiguous [M, ceil(N/160), 2] fp32 (the ABI has no
    stride for them); workspace: the caller's fp32 split-K workspace.  A mismatch of shape, format or device raises PPError.
    w [nb, N, K]: one matrix per batch item of rows_per_batch rows (PPGemmArgs.w_batch_stride); with act =
    L.PP_ACT_SOFTMAX80 bias / ln_colsum may then be [nb, N] as well (vec_batch_stride).
    res1_wrap: res1 holds that many rows only, row m adds res1[m mod res1_wrap] (PPGemmArgs.res1_wrap_rows).
    tile / splitk / tile_group_m: the tuning wishes of PPGemmArgs (0 = automatic); the result is the same bit for bit.
    row_stats=True additionally returns the per-row (sum, sumsq) partials [M, ceil(N/160), 2] fp32;
    ln_stats (that layout) + ln_colsum [N] fp32 apply the folded-LayerNorm correction (see include/pp_hip.h)."""
    lib = L.lib()
    M, K1 = x.shape
    K2 = x2.shape[1] if x2 is not None else 0
    N = w.shape[-2]
    n_out = N // 2 if act == L.PP_ACT_GEGLU else (vt_col0 if vt_col0 else N)
    odt = torch.float32 if out_f32 else x.dtype
    if out is None:
        out = torch.empty(M, n_out, dtype=odt, device=x.device)
    else:
        _view2d(out, M, n_out, odt, x, "gemm: `out`")
    a = L.gemm_args(L.dtype_code(x.dtype), M, N, K1, _p(x), _p(w), _p(out), x2=_p(x2), K2=K2, ldx=x.stride(0),
                    ldx2=x2.stride(0) if x2 is not None else 0, ldo=out.stride(0) if M > 1 else n_out,
                    ldres1=res1.stride(0) if res1 is not None else 0,
                    ldres2=res2.stride(0) if res2 is not None else 0, rows_per_batch=rows_per_batch, scale=scale)
    if w.dim() == 3:
        a.w_batch_stride = w.stride(0)
        if bias is not None and bias.dim() == 2:
            a.vec_batch_stride = bias.stride(0)
    a.bias, a.rowvec, a.res1, a.res2 = _p(bias), _p(rowvec), _p(res1), _p(res2)
    a.ld_rowvec = rowvec.stride(0) if (rowvec is not None and rowvec.dim() == 2 and rowvec.shape[0] > 1) else 0
    a.res1_wrap_rows, a.act, a.out_f32 = res1_wrap, act, int(out_f32)
    if vt_col0:
        nb, ncols = M // rows_per_batch, N - vt_col0
        if vt is None:
            vt = torch.zeros(nb, ncols, rows_per_batch, dtype=x.dtype, device=x.device)
        elif (vt.dim() != 3 or tuple(vt.shape) != (nb, ncols, rows_per_batch) or vt.stride(2) != 1 or vt.dtype != x.dtype
              or vt.device != x.device or vt.stride(1) < rows_per_batch or vt.stride(0) != ncols * vt.stride(1)):
            raise L.PPError(f"gemm: `vt` must be a [{nb}, {ncols}, {rows_per_batch}] window of a contiguous [nb, cols, vt_ld] "
                            "buffer of the inputs' format")
        a.out_vt, a.vt_col0, a.vt_ld = _p(vt), vt_col0, vt.stride(1)
    elif vt is not None:
        raise L.PPError("gemm: `vt` without vt_col0")
    a.tile, a.splitk, a.tile_group_m = tile, splitk, tile_group_m
    _set_gn(a, gn, rows_per_batch)
    if row_stats:
        tn = (N + 159) // 160
        if stats is None:
            stats = torch.zeros(M, tn, 2, dtype=torch.float32, device=x.device)
        elif (tuple(stats.shape) != (M, tn, 2) or not stats.is_contiguous() or stats.dtype != torch.float32
              or stats.device != x.device):
            raise L.PPError(f"gemm: `stats` must be a contiguous [{M}, {tn}, 2] fp32 tensor")
        a.row_stats_out = _p(stats)
    elif stats is not None:
        raise L.PPError("gemm: `stats` without row_stats")
    if ln_stats is not None:
        a.ln_stats, a.ln_colsum, a.ln_tiles, a.ln_dim, a.ln_eps = _p(ln_stats), _p(ln_colsum), ln_stats.shape[1], ln_dim, ln_eps
    wsb = _workspace(lib, a, x.device, workspace)
    a.workspace = _p(wsb)
    _attach_combine(a, x.device, fuse_combine)
    L.check(lib.pp_gemm_bf16(C.byref(a), _s()), "pp_gemm_bf16")
    if row_stats:
        return out, stats
    return (out, vt) if vt_col0 else out


def gn_gamma_beta(gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """(gamma, beta) interleaved per channel, fp32 [C][2]: PPGemmArgs.gn_in_gb."""
    return torch.stack([gamma.float(), beta.float()], 1).contiguous()


def conv_gn_supported(x: torch.Tensor, cout: int, x2=None, x3=None, x4=None, groups: int = 32) -> bool:
    """Would conv3x3(..., gn_in=...) run as the fused GroupNorm + SiLU + conv launch for these shapes?"""
    a = _conv_request(x, cout, 1, False, x2, x3, x4)
    a.gn_in_acc, a.gn_in_gb, a.gn_in_groups, a.gn_in_silu, a.gn_in_eps = 1, 1, groups, 1, 1e-5   # (non-null placeholders)
    return bool(L.lib().pp_conv_gn_supported(C.byref(a)))


def conv_halo_routed(x: torch.Tensor, cout: int, x2=None, x3=None, x4=None, stride: int = 1, up: bool = False,
                     tile: int = 0, up_size=None) -> bool:
    """Does a PLAIN conv3x3 of these shapes run on the halo-tile loop (pp_conv_gn_supported() == 2) rather than the tap-major
    implicit GEMM?"""
    a = _conv_request(x, cout, stride, up, x2, x3, x4, up_size)
    a.tile = tile
    return L.lib().pp_conv_gn_supported(C.byref(a)) == 2


def _conv_request(x, cout, stride, up, x2, x3, x4, up_size=None) -> L.PPGemmArgs:
    """L.conv3x3_args of NHWC tensors (x2 rides beside x; x3 / x4: the 1x1 tail over concat(x3, x4) at the output pixel)"""
    B, H, W, C1 = x.shape
    ch = lambda t: t.shape[3] if t is not None else 0      # noqa: E731
    return L.conv3x3_args(L.dtype_code(x.dtype), B, H, W, C1, cout, _p(x), _p(x2), ch(x2), _p(x3), ch(x3), _p(x4), ch(x4),
                          stride, up, up_size=up_size)


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias=None, stride: int = 1, up: bool = False, x2=None, rowvec=None,
            res1=None, res2=None, scale: float = 1.0, tile: int = 0, splitk: int = 0, gn=None, x3=None, x4=None,
            gn_in=None, gn_next=None, dup: bool = False, gn_dup_mask: int = 0, res1_wrap: int = 0,
            fuse_combine: bool = False, out=None, workspace=None, ynext=None, up_size=None, tile_group_m: int = 0):
    """x NHWC bf16 [B,H,W,C1] (+x2 [B,H,W,C2]); w bf16 [Cout, 9*(C1+C2)] (k = (ky*3+kx)*C + c) -> NHWC bf16.
    up_size (with up): F.interpolate(size=up_size, mode="nearest") in front of the conv instead of the 2x upsample, 2 H - 1 or
    2 H rows and 2 W - 1 or 2 W columns (Upsample2D with `output_size`).
    dup: every output row is stored twice -> out [2B, ...] (PPGemmArgs.out_dup_rows: the CFG twin prefix); gn_dup_mask:
    which of the `gn` subscriptions hold [2B][groups][2] accumulators that receive both halves' sums.
    gn_in = (acc int64 [B][groups][2], gamma_beta fp32 [C1+C2][2], groups, eps): GroupNorm + SiLU of concat(x, x2) fused
    into the loader (x, x2 are then the RAW tensors); raises PPError(PP_ERR_UNSUPPORTED) where conv_gn_supported() is
    False.  gn_next = (gamma, beta, eps, silu, sub): the GroupNorm that consumes the OUTPUT (its statistics subscription
    is gn[sub]) applied by the split-K combine (PPGemmArgs.gn_next_*) -> returns (out, normalised).
    out: the caller's NHWC output, dense pixels with the channel stride taken from the view (ldo; see _nhwc_view); res1 / res2
    likewise carry their own pixel stride and are checked the same way.  workspace: the caller's fp32 split-K workspace.
    ynext: the caller's gn_next output, a contiguous tensor of the output's shape (the ABI has no stride for it; _norm_out)."""
    lib = L.lib()
    B, C1, C2, cout = x.shape[0], x.shape[3], (x2.shape[3] if x2 is not None else 0), w.shape[0]
    a = _conv_request(x, cout, stride, up, x2, x3, x4, up_size)
    ho, wo = a.hout, a.wout
    oshape = (2 * B if dup else B, ho, wo, cout)
    if out is None:
        out = torch.empty(*oshape, dtype=x.dtype, device=x.device)
    else:
        a.ldo = _nhwc_ld(_nhwc_view(out, oshape, x, "conv3x3: `out`"), oshape)
    a.w, a.out, a.scale = _p(w), _p(out), scale
    a.bias, a.rowvec, a.res1, a.res2 = _p(bias), _p(rowvec), _p(res1), _p(res2)
    rshape = (B, ho, wo, cout)
    a.ldres1 = _res_ld(res1, rshape, x, "conv3x3: `res1`", rows_only=res1_wrap > 0)
    a.ldres2 = _res_ld(res2, rshape, x, "conv3x3: `res2`")
    if rowvec is not None and rowvec.dim() == 2 and rowvec.shape[0] > 1:
        a.ld_rowvec = rowvec.stride(0)
    a.res1_wrap_rows = res1_wrap
    if dup:
        a.out_dup_rows = a.M
        if gn_dup_mask:
            a.gn_dup_batch, a.gn_dup_mask = B, gn_dup_mask
    a.tile, a.splitk, a.tile_group_m = tile, splitk, tile_group_m
    _set_gn(a, gn, ho * wo)
    if gn_next is None and ynext is not None:
        raise L.PPError("conv3x3: `ynext` without gn_next")
    if gn_next is not None:
        g_, b_, eps_, silu_, sub_ = gn_next
        ynext = _norm_out(ynext, oshape, x, "conv3x3: `ynext`")
        a.gn_next_out, a.gn_next_gamma, a.gn_next_beta = _p(ynext), _p(g_), _p(b_)
        a.gn_next_eps, a.gn_next_silu, a.gn_next_sub = eps_, int(silu_), sub_
    if gn_in is not None:
        acc, gb, groups, eps = gn_in
        assert gb.dtype == torch.float32 and gb.shape == (C1 + C2, 2) and gb.is_contiguous()
        a.gn_in_acc, a.gn_in_gb, a.gn_in_groups, a.gn_in_silu, a.gn_in_eps = _p(acc), _p(gb), groups, 1, eps
    wsb = _workspace(lib, a, x.device, workspace)
    a.workspace = _p(wsb)
    if gn_next is not None and not lib.pp_gemm_gn_next_ok(C.byref(a), a.gn_next_sub):
        raise L.PPError("pp_gemm_gn_next_ok() = 0 for this launch (PP_ERR_UNSUPPORTED)")
    _attach_combine(a, x.device, fuse_combine)
    L.check(lib.pp_gemm_bf16(C.byref(a), _s()), "pp_gemm_bf16(conv)")
    return (out, ynext) if gn_next is not None else out


def upconv_fold(w: torch.Tensor) -> torch.Tensor:
    """The folded weights of the sub-pixel upsampling conv (pp_upconv_fold): w 16-bit [Cout, 9*C] (k = (ky*3+kx)*C + c) ->
    [4, Cout, 4*C], parity p = 2a + b, k = (dy*2+dx)*C + c."""
    cout, cin = w.shape[0], w.shape[1] // 9
    assert w.is_contiguous() and w.shape[1] == 9 * cin
    out = torch.empty(4, cout, 4 * cin, dtype=w.dtype, device=w.device)
    L.check(L.lib().pp_upconv_fold(_p(w), cout, cin, L.dtype_code(w.dtype), _p(out), _s()), "pp_upconv_fold")
    return out


def upconv_subpix_supported(x: torch.Tensor, cout: int) -> int:
    """pp_upconv_subpix_supported for a source tensor x NHWC [B,H,W,C]: 0 refused, 1 runs, 2 runs and the plans route it."""
    B, H, W, C1 = x.shape
    return int(L.lib().pp_upconv_subpix_supported(B, H, W, C1, cout, L.dtype_code(x.dtype)))


def conv3x3_up_subpix(x: torch.Tensor, wfold: torch.Tensor, bias=None, rowvec=None, res1=None, res2=None, scale: float = 1.0,
                      tile: int = 0, splitk: int = 0, gn=None, out=None, workspace=None, tile_group_m: int = 0):
    """`nearest 2x -> conv3x3` of x NHWC [B,H,W,C] in its sub-pixel form (PPGemmArgs.subpix) on wfold = upconv_fold(w)
    -> NHWC [B,2H,2W,Cout]; res1 / res2 have the output's shape, `gn` subscriptions describe the output tensor.  Raises
    PPError(PP_ERR_UNSUPPORTED) where upconv_subpix_supported() is 0 or a split is forced; conv3x3(up=True) is the other,
    nine-tap request and is not routed here.  out / workspace: as conv3x3 takes them (the form runs in one pass: a
    workspace is checked and never used)."""
    B, H, W, C1 = x.shape
    cout = wfold.shape[1]
    assert tuple(wfold.shape) == (4, cout, 4 * C1) and wfold.is_contiguous()
    a = L.conv3x3_args(L.dtype_code(x.dtype), B, H, W, C1, cout, _p(x))
    a.K, a.subpix = 4 * C1, 1
    if out is None:
        out = torch.empty(B, 2 * H, 2 * W, cout, dtype=x.dtype, device=x.device)
    else:
        a.ldo = _nhwc_ld(_nhwc_view(out, (B, 2 * H, 2 * W, cout), x, "conv3x3_up_subpix: `out`"), (B, 2 * H, 2 * W, cout))
    a.w, a.out, a.scale = _p(wfold), _p(out), scale
    a.bias, a.rowvec, a.res1, a.res2 = _p(bias), _p(rowvec), _p(res1), _p(res2)
    a.ldres1 = _res_ld(res1, (B, 2 * H, 2 * W, cout), x, "conv3x3_up_subpix: `res1`")
    a.ldres2 = _res_ld(res2, (B, 2 * H, 2 * W, cout), x, "conv3x3_up_subpix: `res2`")
    if rowvec is not None and rowvec.dim() == 2 and rowvec.shape[0] > 1:
        a.ld_rowvec = rowvec.stride(0)
    a.tile, a.splitk, a.tile_group_m = tile, splitk, tile_group_m
    _set_gn(a, gn, H * W)
    a.workspace = _p(_workspace(L.lib(), a, x.device, workspace))
    L.check(L.lib().pp_gemm_bf16(C.byref(a), _s()), "pp_gemm_bf16(sub-pixel upsampling conv)")
    return out


def groupnorm(x: torch.Tensor, gamma, beta, eps: float, silu: bool, groups: int = 32, x2=None,
              out: Optional[torch.Tensor] = None):
    """x NHWC bf16 [B,H,W,C1] (+x2) -> NHWC bf16 [B,H,W,C1+C2]; gamma/beta fp32.  out: see _norm_out."""
    lib = L.lib()
    B, H, W, C1 = x.shape
    C2 = x2.shape[3] if x2 is not None else 0
    Ct = C1 + C2
    ws = torch.empty(lib.pp_groupnorm_workspace_bytes(B, H * W, Ct) // 4, dtype=torch.float32, device=x.device)
    y = _norm_out(out, (B, H, W, Ct), x, "groupnorm")
    dt = L.dtype_code(x.dtype)
    L.check(lib.pp_groupnorm_stats(_p(x), C1, _p(x2), C2, B, H * W, groups, _p(ws), dt, _s()), "pp_groupnorm_stats")
    L.check(lib.pp_groupnorm_apply(_p(x), C1, _p(x2), C2, B, H * W, groups, eps, _p(gamma), _p(beta), _p(ws),
                                   int(silu), _p(y), dt, _s()), "pp_groupnorm_apply")
    return y


def layernorm(x: torch.Tensor, gamma, beta, eps: float = 1e-5, out: Optional[torch.Tensor] = None):
    """x [rows, C] 16-bit contiguous -> LayerNorm over C; gamma / beta fp32.  out: see _norm_out."""
    rows, Cc = x.shape
    y = _norm_out(out, (rows, Cc), x, "layernorm")
    L.check(L.lib().pp_layernorm(_p(x), rows, Cc, _p(gamma), _p(beta), eps, _p(y), L.dtype_code(x.dtype), _s()),
            "pp_layernorm")
    return y


def transpose_v(v: torch.Tensor, batch: int, nk: int, ldvt: Optional[int] = None):
    """v [batch*nk, cols] (row stride v.stride(0)) -> vt [batch, cols, ldvt]."""
    cols = v.shape[1]
    ldvt = ldvt or (nk + 7) // 8 * 8
    vt = torch.empty(batch, cols, ldvt, dtype=v.dtype, device=v.device)
    L.check(L.lib().pp_transpose_v(_p(v), v.stride(0), batch, nk, cols, _p(vt), ldvt, _s()), "pp_transpose_v")
    return vt


def _attn_out(out, ldo, rows: int, cols: int, like: torch.Tensor) -> torch.Tensor:
    """The [rows, cols] output view of the attention wrappers: `out` (a caller's view, its row stride is the ldo the kernel
    gets; elements outside the view are the caller's) or a new buffer with row stride `ldo` (default: tight)."""
    if out is None:
        return torch.empty(rows, ldo or cols, dtype=like.dtype, device=like.device)[:, :cols]
    if (tuple(out.shape) != (rows, cols) or out.stride(1) != 1 or out.dtype != like.dtype or out.device != like.device
            or (ldo is not None and ldo != out.stride(0))):
        raise L.PPError(f"attention: `out` must be a [{rows}, {cols}] row-major view of the inputs' format (row stride = ldo)")
    return out


def attention_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, nq: int, nk: int,
                    causal: bool = False, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                    ldo: Optional[int] = None):
    """q [batch*nq, >=heads*64], k / v [batch*nk, ...] row-major bf16 (row strides from the tensors) -> o [batch*nq, heads*64]
    (out / ldo: see _attn_out)."""
    d = 64
    o = _attn_out(out, ldo, batch * nq, heads * d, q)
    L.check(L.lib().pp_attention_small(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                       batch, heads, nq, nk, d, scale if scale is not None else d ** -0.5, int(causal),
                                       L.dtype_code(q.dtype), _s()), "pp_attention_small")
    return o


def perceiver_attention(q: torch.Tensor, kv_x: torch.Tensor, kv_l: Optional[torch.Tensor], batch: int, heads: int, nq: int,
                        scale: Optional[float] = None, out: Optional[torch.Tensor] = None, ldo: Optional[int] = None):
    """The Resampler's attention (pp_perceiver_attn): q [batch*nq, >=heads*64]; kv_x [batch*nx, >=2*heads*64] and kv_l
    [batch*nl, ...] (or None) rows of [K | V], row strides from the tensors -> o [batch*nq, heads*64] over the nx + nl keys
    (out / ldo: see _attn_out)."""
    d = 64
    o = _attn_out(out, ldo, batch * nq, heads * d, q)
    nx, nl = kv_x.shape[0] // batch, (kv_l.shape[0] // batch if kv_l is not None else 0)
    L.check(L.lib().pp_perceiver_attn(_p(q), q.stride(0), _p(kv_x), kv_x.stride(0), nx, _p(kv_l),
                                      kv_l.stride(0) if kv_l is not None else 0, nl, _p(o), o.stride(0), batch, heads, nq, d,
                                      scale if scale is not None else d ** -0.5, L.dtype_code(q.dtype), _s()),
            "pp_perceiver_attn")
    return o


def softmax_rows(s: torch.Tensor, scale: float = 1.0, dtype=torch.bfloat16):
    """fp32 logits [rows, n] (row stride s.stride(0)) -> 16-bit softmax(scale * s) [rows, n]."""
    rows, n = s.shape
    p = torch.empty(rows, n, dtype=dtype, device=s.device)
    L.check(L.lib().pp_softmax_rows(_p(s), s.stride(0), rows, n, float(scale), _p(p), n, L.dtype_code(dtype), _s()),
            "pp_softmax_rows")
    return p


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, batch: int, heads: int, nq: int, nk: int, d: int,
              scale: Optional[float] = None, variant: int = L.PP_ATTN_AUTO, out: Optional[torch.Tensor] = None,
              ldo: Optional[int] = None):
    """q [batch*nq, >=heads*d] / k [batch*nk, ...] row-major bf16 (row strides taken from the tensors);
    vt [batch, heads*d, ldvt].  Returns o [batch*nq, heads*d] (out / ldo: see _attn_out).  `variant` names the kernel
    (L.PP_ATTN_*): AUTO is what the pipelines run; a named kernel raises PP_ERR_UNSUPPORTED on a shape it does not cover."""
    o = _attn_out(out, ldo, batch * nq, heads * d, q)
    L.check(L.lib().pp_attention_fwd_variant(_p(q), q.stride(0), _p(k), k.stride(0), _p(vt), vt.stride(1), _p(o),
                                             o.stride(0), batch, heads, nq, nk, d,
                                             scale if scale is not None else d ** -0.5, L.dtype_code(q.dtype),
                                             int(variant), _s()), "pp_attention_fwd")
    return o


def attention_tiled(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, batch: int, heads: int, h: int, w: int, nh: int,
                    nw: int, d: int, scale: Optional[float] = None, variant: int = L.PP_ATTN_AUTO,
                    out: Optional[torch.Tensor] = None, ldo: Optional[int] = None):
    """Self-attention inside the nh x nw tiles of an h x w token grid (pp_attention_fwd_tiled): operands as `attention` with
    nq = nk = h * w.  Shapes: pp_attention_tiled_ok(h, w, nh, nw, d); anything else raises."""
    o = _attn_out(out, ldo, batch * h * w, heads * d, q)
    L.check(L.lib().pp_attention_fwd_tiled(_p(q), q.stride(0), _p(k), k.stride(0), _p(vt), vt.stride(1), _p(o), o.stride(0),
                                           batch, heads, h, w, nh, nw, d, scale if scale is not None else d ** -0.5,
                                           int(variant), L.dtype_code(q.dtype), _s()), "pp_attention_fwd_tiled")
    return o


def xattn_fold(k: torch.Tensor, vt: torch.Tensor, batch: int, nctx: int, heads: int, wq: torch.Tensor, wo: torch.Tensor,
               q_colsum=None, q_bias=None, scale: Optional[float] = None, kperm=False, gt=None, gcs=None, gbias=None,
               ht=None):
    """Once per prompt (pp_xattn_fold): k [batch*nctx, >=c], vt [batch, c, ldvt], wq / wo [c, c] ([out][in]) ->
    (gt [batch, heads*80, c], gcs [batch, heads*80] fp32, gbias [batch, heads*80] fp32, ht [batch, c, heads*80]).
    k may be a column window of wider rows (its row stride is ldk), vt a [batch, c, nctx] window of a contiguous
    [batch, c, ldvt] buffer; what lies behind column c / nctx is not read.  kperm: False / True / 2 (include/pp_hip.h).
    gt / gcs / gbias / ht: the caller's outputs, contiguous and of exactly those shapes (the ABI has no stride for them)."""
    c = wq.shape[0]
    dev, dt = k.device, k.dtype
    if k.dim() != 2 or k.shape[0] != batch * nctx or k.shape[1] < c or k.stride(1) != 1 or (k.shape[0] > 1 and k.stride(0) < c):
        raise L.PPError(f"xattn_fold: `k` must be [{batch * nctx}, >= {c}] rows with unit column stride")
    if (vt.dim() != 3 or vt.shape[0] != batch or vt.shape[1] != c or vt.shape[2] < nctx or vt.stride(2) != 1 or vt.dtype != dt
            or vt.stride(1) < nctx or (batch > 1 and vt.stride(0) != c * vt.stride(1))):
        raise L.PPError(f"xattn_fold: `vt` must be a [{batch}, {c}, >= {nctx}] window of a contiguous [batch, c, ldvt] buffer")
    for w_, nm in ((wq, "wq"), (wo, "wo")):
        if tuple(w_.shape) != (c, c) or not w_.is_contiguous() or w_.dtype != dt:
            raise L.PPError(f"xattn_fold: `{nm}` must be a contiguous [{c}, {c}] matrix of the inputs' format")
    n = heads * 80
    gt = torch.empty(batch, n, c, dtype=dt, device=dev) if gt is None else _exact(gt, (batch, n, c), dt, k, "xattn_fold: `gt`")
    ht = torch.empty(batch, c, n, dtype=dt, device=dev) if ht is None else _exact(ht, (batch, c, n), dt, k, "xattn_fold: `ht`")
    gcs = torch.empty(batch, n, dtype=torch.float32, device=dev) if gcs is None else \
        _exact(gcs, (batch, n), torch.float32, k, "xattn_fold: `gcs`")
    gb = torch.empty(batch, n, dtype=torch.float32, device=dev) if gbias is None else \
        _exact(gbias, (batch, n), torch.float32, k, "xattn_fold: `gbias`")
    L.check(L.lib().pp_xattn_fold(_p(k), k.stride(0) if k.shape[0] > 1 else k.shape[1], _p(vt), vt.stride(1), batch, nctx, heads, c, _p(wq), _p(q_colsum),
                                  _p(q_bias), _p(wo), scale if scale is not None else (c // heads) ** -0.5, _p(gt),
                                  _p(gcs), _p(gb), _p(ht), int(kperm), L.dtype_code(dt), _s()), "pp_xattn_fold")
    return gt, gcs, gb, ht


def xattn_block(x: torch.Tensor, folded, bias_o=None, res=None, ln_stats=None, ln_eps: float = 1e-5,
                rows_per_batch: int = 0, row_stats=False, twin: bool = False, pre_w=None, pre_b=None,
                ln_fold: bool = False, out=None):
    """out = softmax_per_head(LNfold(x) gt^T) ht^T + bias_o + res  (pp_xattn_block); x [M, c], folded = xattn_fold(...).
    twin: x / res / ln_stats hold ONE half of a CFG pair (M rows) whose other half is identical; the output has 2 M rows
    (src_wrap_rows = M) and `folded` is per batch item of the full batch.
    x / res may be windows of wider rows (unit column stride; the pad columns are not read).  out: the caller's [M, c] view
    with unit column stride (its row stride is ldo; what lies outside it is the caller's); row_stats: True, or the caller's
    contiguous [M, c / 160, 2] fp32 tensor."""
    gt, gcs, gb, ht = folded
    wrap = x.shape[0] if twin else 0
    M, c = x.shape[0] * (2 if twin else 1), x.shape[1]
    ldx = _rows_in(x, c, x, "xattn_block: `x`")
    ldres = _rows_in(res, c, x, "xattn_block: `res`") if res is not None else 0
    if res is not None and res.shape[0] != x.shape[0]:
        raise L.PPError("xattn_block: `res` must have the rows of `x`")
    nb = M // (rows_per_batch or M)
    _exact(gt, (nb, 640, c), x.dtype, x, "xattn_block: folded gt")
    _exact(ht, (nb, c, 640), x.dtype, x, "xattn_block: folded ht")
    _exact(gcs, (nb, 640), torch.float32, x, "xattn_block: folded gcs")
    _exact(gb, (nb, 640), torch.float32, x, "xattn_block: folded gbias")
    out = torch.empty(M, c, dtype=x.dtype, device=x.device) if out is None else _view2d(out, M, c, x.dtype, x, "xattn_block: `out`")
    if torch.is_tensor(row_stats):
        st = _exact(row_stats, (M, c // 160, 2), torch.float32, x, "xattn_block: `row_stats`")
        row_stats = True
    else:
        st = torch.zeros(M, c // 160, 2, dtype=torch.float32, device=x.device) if row_stats else None
    # pre_w / pre_b: the Linear in front (h = x pre_w^T + pre_b + res) in the same launch; `folded` must come from
    # xattn_fold(kperm=True); ln_fold = a LayerNorm of h is folded into `folded` (row moments are computed in the kernel)
    tiles = ln_stats.shape[1] if ln_stats is not None else (c // 160 if (pre_w is not None and ln_fold) else 0)
    L.check(L.lib().pp_xattn_block(_p(x), ldx, _p(res), ldres, _p(ln_stats),
                                   tiles, ln_eps, _p(gt), _p(gcs), _p(gb), _p(ht),
                                   _p(bias_o), _p(out), out.stride(0) if M > 1 else c, _p(st), M, c, rows_per_batch or M, wrap, _p(pre_w), _p(pre_b),
                                   L.dtype_code(x.dtype), _s()), "pp_xattn_block")
    return (out, st) if row_stats else out


def ff_fused(hs: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2kp: torch.Tensor, bias2=None, cs1=None, ln_stats=None,
             ln_eps: float = 1e-5, res1=None, res2=None, res1_wrap: int = 0, rows_per_batch: int = 0, gn=None,
             w2_kperm: bool = True, scale: float = 1.0, out=None):
    """pp_ff_fused: out = ([h (.) gelu(g) | hs] w2kp^T + bias2) * scale + res1 + res2 with h | g = FF1(LayerNorm-folded hs), one
    launch.  hs / res1 / res2 may be windows of wider rows (unit column stride; the pad columns are not read; res1 holds
    res1_wrap rows when that is set); out: the caller's [M, 320] view with unit column stride (its row stride is ldo).
    hs [M, 320]; w1 [2560, 320] (GEGLU-interleaved rows, gamma folded); w2kp [320, 1600]: w2_kperm=True -> hidden index
    permuted (engine._kperm_geglu; the 4-wave kernel that chains the GEGLU in registers), False -> natural order (the 8-wave
    kernel, activations exchanged through LDS); ln_stats [M, 2, 2] row moments of hs or None; gn: as ops.gemm takes them."""
    M, Cc = hs.shape
    ldx = _rows_in(hs, Cc, hs, "ff_fused: `hs`")
    ld1 = _rows_in(res1, Cc, hs, "ff_fused: `res1`") if res1 is not None else 0
    ld2 = _rows_in(res2, Cc, hs, "ff_fused: `res2`") if res2 is not None else 0
    if res1 is not None and res1.shape[0] != (res1_wrap or M):
        raise L.PPError(f"ff_fused: `res1` must have {res1_wrap or M} rows")
    if res2 is not None and res2.shape[0] != M:
        raise L.PPError(f"ff_fused: `res2` must have {M} rows")
    if tuple(w1.shape) != (8 * Cc, Cc) or not w1.is_contiguous() or tuple(w2kp.shape) != (Cc, 5 * Cc) or not w2kp.is_contiguous():
        raise L.PPError("ff_fused: `w1` / `w2kp` must be contiguous [2560, 320] / [320, 1600] matrices")
    out = torch.empty(M, Cc, dtype=hs.dtype, device=hs.device) if out is None else _view2d(out, M, Cc, hs.dtype, hs, "ff_fused: `out`")
    a = L.gemm_args(L.dtype_code(hs.dtype), M, Cc, 4 * Cc, _p(hs), _p(w2kp), _p(out), x2=_p(hs), K2=Cc, ldx2=ldx,
                    ldo=out.stride(0) if M > 1 else Cc, ldres1=ld1, ldres2=ld2, rows_per_batch=rows_per_batch, scale=scale)
    a.bias, a.res1, a.res2, a.res1_wrap_rows = _p(bias2), _p(res1), _p(res2), res1_wrap
    _set_gn(a, gn, rows_per_batch)
    L.check(L.lib().pp_ff_fused(C.byref(a), _p(w1), _p(b1), _p(cs1), _p(ln_stats),
                                ln_stats.shape[1] if ln_stats is not None else 0, ln_eps, int(w2_kperm), _s()), "pp_ff_fused")
    return out


def gn_conv3x3_smallcout(x, acc, gamma, beta, eps: float, w, bias, groups: int = 32):
    """conv_norm_out + SiLU + conv_out in one launch: x NHWC 16-bit [B,H,W,Cin], acc int64 [B,groups,2] (the producers'
    GroupNorm accumulators), w [4, 9*Cin] -> fp32 NCHW [B,4,H,W]."""
    B, H, W, Cin = x.shape
    out = torch.empty(B, w.shape[0], H, W, dtype=torch.float32, device=x.device)
    L.check(L.lib().pp_gn_conv3x3_smallcout(_p(x), B, H, W, Cin, groups, eps, _p(gamma), _p(beta), _p(acc), _p(w), _p(bias),
                                            w.shape[0], _p(out), L.dtype_code(x.dtype), _s()), "pp_gn_conv3x3_smallcout")
    return out


def conv3x3_direct(x, w, bias, stride: int = 1, silu: bool = False, add=None):
    """x NHWC bf16 [B,H,W,Cin]; w bf16 [3,3,Cin,Cout]."""
    B, H, W, Cin = x.shape
    cout = w.shape[3]
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty(B, ho, wo, cout, dtype=x.dtype, device=x.device)
    L.check(L.lib().pp_conv3x3_direct(_p(x), B, H, W, Cin, _p(w), _p(bias), cout, stride, int(silu), _p(add), _p(out),
                                      L.dtype_code(x.dtype), _s()), "pp_conv3x3_direct")
    return out


def conv3x3_smallcout(x, w, bias):
    """x NHWC bf16 [B,H,W,Cin]; w bf16 [4, 9*Cin] -> fp32 NCHW [B,4,H,W]."""
    B, H, W, Cin = x.shape
    out = torch.empty(B, w.shape[0], H, W, dtype=torch.float32, device=x.device)
    L.check(L.lib().pp_conv3x3_smallcout(_p(x), B, H, W, Cin, _p(w), _p(bias), w.shape[0], _p(out),
                                         L.dtype_code(x.dtype), _s()), "pp_conv3x3_smallcout")
    return out


def nchw_to_nhwc(src: torch.Tensor, batch: Optional[int] = None, ldc: Optional[int] = None, c0: int = 0, dst=None,
                 dtype=torch.bfloat16):
    B, Cc, H, W = src.shape
    nb = batch or B
    ldc = ldc or Cc
    if dst is None:
        dst = torch.zeros(nb, H, W, ldc, dtype=dtype, device=src.device)
    src = src.contiguous()
    L.check(L.lib().pp_nchw_to_nhwc(_p(src), _DT[src.dtype], nb, Cc, H * W, B if nb != B else 0, _p(dst), ldc, c0,
                                    L.dtype_code(dst.dtype), _s()), "pp_nchw_to_nhwc")
    return dst


def nhwc_to_nchw(src: torch.Tensor, dtype=torch.float32):
    B, H, W, Cc = src.shape
    dst = torch.empty(B, Cc, H, W, dtype=dtype, device=src.device)
    L.check(L.lib().pp_nhwc_to_nchw(_p(src), B, Cc, H * W, _p(dst), _DT[dtype], L.dtype_code(src.dtype), _s()),
            "pp_nhwc_to_nchw")
    return dst


def vit_patchify(src: torch.Tensor, patch: int, out: Optional[torch.Tensor] = None, dtype=torch.bfloat16):
    """src [B, 3, H, W] fp32 | bf16 | fp16 -> the im2col rows of the stride-`patch` patch conv, [B * (H // patch) * (W // patch),
    cols] 16-bit with columns [3 patch^2, cols) written as zeros (pp_vit_patchify).  out: any [rows, cols] view with unit column
    stride (a window of a larger buffer; its row stride is the ldo of the launch, what lies outside it is the caller's).
    Default: cols = 3 patch^2 rounded up to 64."""
    B, Cc, H, W = src.shape
    if Cc != 3:
        raise L.PPError("vit_patchify: src must be [B, 3, H, W]")
    rows = B * (H // patch) * (W // patch)
    if out is None:
        out = torch.empty(rows, (3 * patch * patch + 63) // 64 * 64, dtype=dtype, device=src.device)
    elif out.dim() != 2 or out.shape[0] != rows or out.stride(1) != 1 or out.stride(0) < out.shape[1] or out.device != src.device:
        raise L.PPError(f"vit_patchify: `out` must be a [{rows}, cols] row-major 16-bit view on the source's device")
    src = src.contiguous()
    L.check(L.lib().pp_vit_patchify(_p(src), _DT[src.dtype], B, H, W, patch, _p(out), out.shape[1], out.stride(0), L.dtype_code(out.dtype),
                                    _s()), "pp_vit_patchify")
    return out


def vit_embed_ln(patches: torch.Tensor, class_embedding: torch.Tensor, pos: torch.Tensor, batch: int, gamma, beta,
                 eps: float = 1e-5, out: Optional[torch.Tensor] = None):
    """LayerNorm([class | patches] + pos) as one launch (pp_vit_embed_ln): patches [batch * np, C] (any row stride >= C), class
    embedding [C], pos [np + 1, C], all of one 16-bit format; gamma / beta fp32 -> [batch * (np + 1), C].  out: see _norm_out."""
    Cc = patches.shape[1]
    npatch = patches.shape[0] // batch
    ldp = _rows_in(patches, Cc, patches, "vit_embed_ln: `patches`")
    if patches.shape[0] != batch * npatch or tuple(pos.shape) != (npatch + 1, Cc) or class_embedding.numel() != Cc or \
            pos.dtype != patches.dtype or class_embedding.dtype != patches.dtype:
        raise L.PPError("vit_embed_ln: patches [batch * np, C], class_embedding [C], pos [np + 1, C] of one 16-bit format")
    y = _norm_out(out, (batch * (npatch + 1), Cc), patches, "vit_embed_ln")
    L.check(L.lib().pp_vit_embed_ln(_p(patches), ldp, _p(class_embedding.contiguous()), _p(pos.contiguous()), batch, npatch, Cc,
                                    _p(gamma), _p(beta), eps, _p(y), L.dtype_code(patches.dtype), _s()), "pp_vit_embed_ln")
    return y


def add(a: torch.Tensor, b: torch.Tensor):
    out = torch.empty_like(a)
    L.check(L.lib().pp_add_bf16(_p(a), _p(b), _p(out), a.numel(), L.dtype_code(a.dtype), _s()), "pp_add_bf16")
    return out


def freeu(hidden: torch.Tensor, skip: torch.Tensor, b: float, s: float, acc: Optional[torch.Tensor] = None,
          groups: int = 32, inplace: bool = False):
    """FreeU in front of an up-block resnet (pp_freeu): hidden [B,H,W,Ch] with its first Ch/2 channels times b, skip
    [B,H,W,Cs] through the four-bin Fourier filter with scale s.  acc: int64 [B][groups][2] (zeroed by the caller) receives
    the GroupNorm statistics of concat(hidden', skip').  inplace: both tensors are rewritten (what the launch plans do).
    Returns (hidden', skip')."""
    B, H, W, Ch = hidden.shape
    ho, so = (hidden, skip) if inplace else (torch.empty_like(hidden), torch.empty_like(skip))
    bs = torch.tensor([b, s], dtype=torch.float32, device=hidden.device)
    L.check(L.lib().pp_freeu(_p(hidden), _p(ho), Ch, _p(skip), _p(so), skip.shape[3], B, H, W, _p(bs), _p(acc), groups,
                             L.dtype_code(hidden.dtype), _s()), "pp_freeu")
    return ho, so


def timestep_embedding(t: torch.Tensor, rows: int, dim: int):
    out = torch.empty(rows, dim, dtype=torch.float32, device=t.device)
    L.check(L.lib().pp_timestep_embedding(_p(t), rows, dim, _p(out), _s()), "pp_timestep_embedding")
    return out


def linear_skinny(x: torch.Tensor, w: torch.Tensor, bias=None, act_in: int = 0, act_out: int = 0):
    rows, K = x.shape
    N = w.shape[0]
    out = torch.empty(rows, N, dtype=torch.float32, device=x.device)
    L.check(L.lib().pp_linear_skinny(_p(x), rows, K, _p(w), _p(bias), N, _p(out), N, act_in, act_out,
                                     L.dtype_code(w.dtype), _s()), "pp_linear_skinny")
    return out


def tfront(x: torch.Tensor, acc: torch.Tensor, gamma, beta, w1: torch.Tensor, b1, w2p: torch.Tensor, cs2, b2, rows_per_batch: int,
           gn_eps: float = 1e-6, ln_eps: float = 1e-5, groups: int = 32, q_scale: float = 1.0, hs=None, qk=None, vt=None):
    """pp_tfront: hs = proj_in(GroupNorm(x)); q | k | v = QKV(LayerNorm1(hs)), V transposed.  x [M, 320] raw rows, acc the
    int64 GroupNorm accumulators of x, w2p the gamma-folded QKV weight with engine._kperm applied.  -> (hs, qk [M, 640], vt).
    q_scale multiplies the Q third before its rounding (head_dim^-0.5 * log2 e for L.PP_ATTN_PIPE_LOG2).
    x may be a window of wider rows (unit column stride; the pad columns are not read).  hs / qk: the caller's [M, 320] /
    [M, 640] views with unit column stride (their row strides are ldhs / ldqk); vt: the caller's [nb, 320, rows_per_batch]
    window of a contiguous [nb, 320, ldvt] buffer.  What lies outside the views is the caller's."""
    M, c = x.shape
    if rows_per_batch <= 0 or M % rows_per_batch:
        raise L.PPError("tfront: M must be a multiple of rows_per_batch")
    nb = M // rows_per_batch
    ldx = _rows_in(x, c, x, "tfront: `x`")
    if tuple(acc.shape) != (nb, groups, 2) or acc.dtype != torch.int64 or not acc.is_contiguous():
        raise L.PPError(f"tfront: `acc` must be a contiguous int64 [{nb}, {groups}, 2] tensor")
    hs = torch.empty(M, c, dtype=x.dtype, device=x.device) if hs is None else _view2d(hs, M, c, x.dtype, x, "tfront: `hs`")
    qk = torch.empty(M, 2 * c, dtype=x.dtype, device=x.device) if qk is None else _view2d(qk, M, 2 * c, x.dtype, x, "tfront: `qk`")
    vt = torch.empty(nb, c, rows_per_batch, dtype=x.dtype, device=x.device) if vt is None else \
        _vt_window(vt, nb, c, rows_per_batch, x, "tfront: `vt`")
    L.check(L.lib().pp_tfront(_p(x), ldx, _p(acc), _p(gamma), _p(beta), gn_eps, groups, _p(w1), _p(b1), _p(w2p), _p(cs2),
                              _p(b2), ln_eps, _p(hs), hs.stride(0) if M > 1 else c, _p(qk), qk.stride(0) if M > 1 else 2 * c, _p(vt),
                              vt.stride(1), M, c, rows_per_batch,
                              float(q_scale), L.dtype_code(x.dtype), _s()), "pp_tfront")
    return hs, qk, vt


# ---- token merging (csrc/tome.hip; include/pp_hip.h, "Token merging") --------------------------------------------------------
def tome_supported(h: int, w: int, C: int, sx: int = 2, sy: int = 2) -> bool:
    return bool(L.lib().pp_tome_supported(h, w, C, sx, sy))


def tome_match(x: torch.Tensor, batch: int, h: int, w: int, table: torch.Tensor, sx: int = 2, sy: int = 2, row_idx=None,
               best=None, score=None):
    """pp_tome_match: x 16-bit [batch*h*w, C] (row stride free); table uint8 [rows, >= hsy*wsx] on the device; row_idx: int32
    device tensor with the table row to use, or None (row 0).  -> (best_dst int32 [batch, h*w], score fp32 [batch, h*w])."""
    n, Cc = h * w, x.shape[1]
    best = torch.empty(batch, n, dtype=torch.int32, device=x.device) if best is None else best
    score = torch.empty(batch, n, dtype=torch.float32, device=x.device) if score is None else score
    L.check(L.lib().pp_tome_match(_p(x), x.stride(0), batch, h, w, Cc, sx, sy, _p(table), table.stride(0), table.shape[0],
                                  _p(row_idx), _p(best), _p(score), L.dtype_code(x.dtype), _s()), "pp_tome_match")
    return best, score


def tome_select(best: torch.Tensor, score: torch.Tensor, nd: int, r: int, out=None):
    """pp_tome_select -> (pos [batch, n], rowtok [batch, n - r], seg [batch, nd + 1], lst [batch, r]), int32."""
    batch, n = best.shape
    if out is None:
        out = tuple(torch.empty(batch, max(m, 1), dtype=torch.int32, device=best.device) for m in (n, n - r, nd + 1, r))
    pos, rowtok, seg, lst = out
    L.check(L.lib().pp_tome_select(_p(best), _p(score), batch, n, nd, r, _p(pos), _p(rowtok), _p(seg), _p(lst), _s()),
            "pp_tome_select")
    return pos, rowtok, seg, lst


def tome_merge(qk: torch.Tensor, vt: torch.Tensor, batch: int, n: int, nd: int, r: int, rowtok, seg, lst, qk_out=None,
               vt_out=None):
    """pp_tome_merge: qk 16-bit [batch*n, 2C] (row stride free), vt 16-bit [batch, C, ldvt] -> (qk_out [batch*(n - r), 2C],
    vt_out [batch, C, round8(n - r)]), or into the given views."""
    Cc, nm = qk.shape[1] // 2, n - r
    qk_out = torch.empty(batch * nm, 2 * Cc, dtype=qk.dtype, device=qk.device) if qk_out is None else qk_out
    vt_out = torch.empty(batch, Cc, (nm + 7) // 8 * 8, dtype=qk.dtype, device=qk.device) if vt_out is None else vt_out
    L.check(L.lib().pp_tome_merge(_p(qk), qk.stride(0), _p(vt), vt.stride(1), batch, n, Cc, nd, r, _p(rowtok), _p(seg), _p(lst),
                                  _p(qk_out), qk_out.stride(0), _p(vt_out), vt_out.stride(1), L.dtype_code(qk.dtype), _s()),
            "pp_tome_merge")
    return qk_out, vt_out


def tome_unmerge(a: torch.Tensor, pos: torch.Tensor, out=None):
    """pp_tome_unmerge: a 16-bit [batch*nm, C] (row stride free), pos int32 [batch, n] -> out [batch*n, C]."""
    batch, n = pos.shape
    nm, Cc = a.shape[0] // batch, a.shape[1]
    out = torch.empty(batch * n, Cc, dtype=a.dtype, device=a.device) if out is None else out
    L.check(L.lib().pp_tome_unmerge(_p(a), a.stride(0), _p(pos), batch, n, nm, Cc, _p(out), out.stride(0), _s()),
            "pp_tome_unmerge")
    return out


def attn_identity_v(vt: torch.Tensor, n: int, out: torch.Tensor, batch0: int = 0, batch: Optional[int] = None):
    """pp_attn_identity_v: vt 16-bit [items, C, ldvt] (V transposed) -> rows [b*n, b*n + n) x columns [0, C) of `out` ([items*n,
    >= C], row stride free) for b in [batch0, batch0 + batch): the attention output of PAG's perturbed batch items, V itself."""
    items, Cc, ldvt = vt.shape
    batch = items - batch0 if batch is None else batch
    if vt.stride(2) != 1 or vt.stride(1) != ldvt or vt.stride(0) != Cc * ldvt or out.stride(1) != 1 or out.dtype != vt.dtype:
        raise L.PPError("attn_identity_v: vt must be dense [items, C, ldvt], out row-major of the same 16-bit format")
    if batch0 < 0 or batch < 1 or batch0 + batch > items or out.shape[0] < items * n or out.shape[1] < Cc:
        raise L.PPError(f"attn_identity_v: items [{batch0}, {batch0 + batch}) of {items}, n = {n}: out {tuple(out.shape)} is too small")
    L.check(L.lib().pp_attn_identity_v(_p(vt), ldvt, batch0, batch, n, Cc, _p(out), out.stride(0), _s()), "pp_attn_identity_v")
    return out


def pag_combine(eps: torch.Tensor, cfg: bool, guidance: float, pag_table: torch.Tensor, step: torch.Tensor):
    """pp_pag_combine, in place: eps fp32 [3 or 2 segments, ...] contiguous; pag_table fp32 [rows]; step int32 [1] on the device."""
    segs = 3 if cfg else 2
    if eps.dtype != torch.float32 or not eps.is_contiguous() or eps.shape[0] != segs or pag_table.dtype != torch.float32 or \
            step.dtype != torch.int32:
        raise L.PPError(f"pag_combine: eps must be contiguous fp32 [{segs}, ...], pag_table fp32, step int32")
    L.check(L.lib().pp_pag_combine(_p(eps), int(bool(cfg)), float(guidance), _p(pag_table), _p(step), eps[0].numel(), _s()),
            "pp_pag_combine")
    return eps


def cfg_rescale(eps: torch.Tensor, guidance: float, phi_cell: torch.Tensor, pag_table: Optional[torch.Tensor] = None,
                step: Optional[torch.Tensor] = None):
    """pp_cfg_rescale, in place: eps fp32 [2 or 3 segments, batch, ...] contiguous, (e_u, e_c) or with `pag_table` (fp32 [rows],
    `step` int32 [1] on the device) (e_u, e_c, e_p); phi_cell fp32 [1] on the device, read by the launch.  Segment 0 becomes
    the guided prediction rescaled per sample (diffusers' rescale_noise_cfg)."""
    segs = 3 if pag_table is not None else 2
    if eps.dtype != torch.float32 or not eps.is_contiguous() or eps.dim() < 3 or eps.shape[0] != segs or \
            phi_cell.dtype != torch.float32 or phi_cell.numel() != 1:
        raise L.PPError(f"cfg_rescale: eps must be contiguous fp32 [{segs}, batch, ...], phi_cell one fp32")
    if pag_table is not None and (pag_table.dtype != torch.float32 or step is None or step.dtype != torch.int32):
        raise L.PPError("cfg_rescale: pag_table must be fp32 and come with the int32 step counter")
    L.check(L.lib().pp_cfg_rescale(_p(eps), segs, float(guidance), _p(pag_table) if pag_table is not None else None,
                                   _p(phi_cell), _p(step) if step is not None else None, eps.shape[1], eps[0, 0].numel(), _s()),
            "pp_cfg_rescale")
    return eps
