"""The small and step kernels of csrc/small.hip held to exact probes, capped-grid shapes and guarded outputs: the shared case
matrix, the fp64 references, the derived gates and a torch restatement of every kernel's index walk.  Plain torch, no HIP:
tests/test_small_probes.py proves on the CPU that the faithful walk meets every case and that every named defect fails one;
tests/test_small_exact_gpu.py runs the same matrix through the C ABI.

THE OPERATIONS (as include/pp_hip.h and the kernels define them)
  conv_direct   pp_conv3x3_direct: out[b][oy][ox][co] = to16(silu?(bias[co] + sum_{ky,kx,ci} x[b][oy s+ky-1][ox s+kx-1][ci]
                w[ky][kx][ci][co] + add[b][oy][ox][co])), pad 1, stride s in {1, 2}, hout = (hin - 1) / s + 1.  One work item =
                (pixel, 8 output channels), i = pixel * (cout / 8) + slice; the grid is capped at 4096 blocks of 256 and strides.
  conv_out      pp_conv3x3_smallcout: out[b][co][y][x] (fp32 NCHW, co < 4) = bias[co] + sum w[co][ky][kx][ci] x[b][y+ky-1][x+kx-1][ci].
                cin % 32 == 0 and cin <= 384: the MFMA kernel -- a workgroup owns 32 consecutive pixels (two 16-pixel groups, flat
                over batch, rows and columns); step st = wave + 4 j (j < 3) of cin / 32 is live if st < cin / 32; a tap outside
                the image or a pixel slot past the end reads a clamped address and is masked to zero.  Otherwise the scalar
                kernel: one wave per pixel, four pixels per block.
  to_nhwc       pp_nchw_to_nhwc: dst[i][c0 + j] = to16(src[(b % bmod or b)][j][p]), i = b hw + p, row stride ldc; capped grid.
  to_nchw       pp_nhwc_to_nchw: dst[b][ch][p] = src[b][p][ch] as fp32 or unchanged 16 bits; capped grid over b c hw.
  add           pp_add_bf16: out = to16(a + b), one fp32 add, 8 elements per work item; capped grid over n / 8.
  skinny        pp_linear_skinny: out[r][n] = act_out(bias[n] + sum_k act_in(x[r][k]) w[n][k]); rows are padded with zero rows
                to the template R in {1, 4, 8, 16}, only r < rows is stored; a block has 4 columns, at most 2048 blocks, the
                column loop strides; R K floats of LDS (above 64 KB: opted in; above 160 KB: PP_ERR_UNSUPPORTED).
  temb          pp_timestep_embedding: out[r][k] = cos(t f_k), out[r][half + k] = sin(t f_k), f_k = exp(-ln(1e4) k / half),
                i = r half + k.
  softmax       pp_softmax_rows: p[r][c] = to16(exp2(s l - M) / S), l = fp32(scale) * fp32(log2 e) in fp32; float4 body over
                n / 4 groups, scalar tail, columns [n, ldp) written as zeros.  CONTRACT: scale log2e s must be finite.  The
                product s l is rounded to fp32 once and every pass uses that value (no fused multiply-subtract: the row maximum
                must give exp2(0); found by the `largest` regime, defect softmax_product_fused_into_subtraction).
  splice        pp_embed_splice: out[r] = src_row[r] >= 0 ? table[src_row[r]] : ext[-src_row[r] - 1], row_bytes raw bytes; the
                copy width (16 / 4 / 1 bytes) is the common alignment of the three bases and row_bytes.
  step_head     pp_step_head[_scaled]: temb_out = table[step]; x_in[i][c0 + j] = to16(lat[b % bmod][j][p] (/ in_div[step]));
                zero_dst[0 .. nz) = 0.  The latent branch runs on at most 256 blocks, the zero branch too, the row copy on 64.
  zero_u64      pp_zero_u64: dst[0 .. n) = 0 on at most 1024 blocks.
  step kernels  pp_cfg_sched_step (kinds 0..3), pp_cfg_lcm_step, pp_cfg_sigma_step, pp_cfg_ksampler_step,
                pp_ddim_variance_noise: fp32 elementwise on row step_dev[0] of a device table, the formulas of `step_formula`
                (the kernels' own); grid capped at 4096 blocks.  With a ticket the block that draws the last one does
                step += 1 and returns the ticket to 0; without, the counter is not touched.
  blend         pp_latent_blend: x[i] = (1 - m[e % hw]) (b == 0 ? x0[e] : a x0[e] + b z[i]) + m[e % hw] x[i], e = i % chw.
  mask_prep     pp_mask_prep modes 0..3 (threshold, image * (mask < 0.5), torch-nearest resize, sum over channels < 0).
  gn_conv       pp_gn_conv3x3_smallcout (csrc/norm.hip) = pp_groupnorm_apply_acc (SiLU) -> pp_conv3x3_smallcout, bit for bit on
                exact data (GN_CONV_CASES below); what pp_gn_conv3x3_smallcout_supported refuses is refused.

PROBE E (bit equality).  x in {-1, 0, 1}, sparse so that a sum stays representable; w in {+-1, +-2}; integer bias and `add`;
the skinny x is fp32 small integers; step kernels: small integers, integer guidance, coefficients that are integers or powers
of two (so the divisions by c1 / al are exact).  The builder asserts |sum| < 2^24 and that every result survives the cast to
the output format.  Softmax: one-hot rows (one logit ahead by more than 160 in the exp2 domain: every other exponential is
exactly 0 in fp32, the sum 1, the answer 1 and 0 in any order), n = 1, and the largest finite logits the contract allows
(two equal maxima -> 0.5, 0.5, 0...).  Copies, layout, splice, zero, mask_prep and add are bit-exact on ANY data: ties of the
16-bit rounding, +-0, subnormals, the largest finite values and, in fp16, sums / casts that overflow to inf; reference = the
fp64 value cast once (a 16-bit pair differs by > 13 binades only when the small operand is below a quarter ulp of the large
one: the fp32 add in between cannot move the result).

PROBE R (fp64 reference, derived gate  |out - ref| <= u |ref| + n_r 2^-24 A;  u = 2^-8 bf16, 2^-11 fp16, 0 for fp32 outputs;
A = the sum of the absolute values of every term of the element).  n_r per kernel, from its operation sequence:
  conv_direct   9 cin fmas in one chain + the add + 1: n_r = 9 cin + 2.
  conv_out      MFMA: at most 9 cin roundings inside the chain of MFMAs of a wave, 3 adds of the four partials, bias; scalar:
                at most 9 cin / 8 fmas x 8 per lane, 6 shuffle adds, bias: n_r = 9 cin + 8 for both.
  skinny        K fmas per lane at most, 6 shuffle adds, bias: n_r = K + 7.  act_in = SiLU: every x carries the SiLU term below,
                propagated through |w|.
  SiLU          norm_cases, "SiLU": slope <= 1.1; x / (1 + exp(-x)) with the argument product (u32 |pre|), exp, add, division:
                d' = 1.1 d + (7 + |pre|) 2^-24 |ref|.
  step kernels  every fp32 operation of the formula rounds once; an operation's error is at most 2^-24 times the absolute-value
                evaluation of the formula (every operand and coefficient replaced by its magnitude, every subtraction by an
                addition, the division by |c1| / |al| kept), which is A.  n_r = the number of operations of the longest
                formula of the kernel + 1 (second order): N_R below.
  blend         7 operations: n_r = 8.
  softmax       norm_cases' pp_xattn_block model with the row length in place of 80: the logit x = s l and x - M carry
                D = 2 2^-24 (|x| + |M|) in the exp2 domain and move p by p (2^(2 D) - 1); the sum: ceil(n / 256) + 16 adds along
                the longest chain (thread, 6 shuffles, 4 waves), each term with exp2 (2 ulp budget = 4 u32) and a rescale
                (exp2, product): n_S = 3 (ceil(n / 256) + 16) + 3; exp2, the reciprocal and the product of the second pass: 4.
                gate = u p + p (2^(2 D) - 1) + (n_S + 4) 2^-24 p + half a subnormal of the format.
  temb          exponent e = -c k / half: the constant (u32), one product, one division: |de| <= 3 u32 |e|; expf, cosf, sinf: the
                ROCm tree this suite is built against ships no ulp table for the device math library, so EACH CALL IS BOUNDED BY
                2 ulp = 4 u32 (an assumption, stated here, not tuned: profiles/small_exact_achieved.txt shows the slack);
                f carries (3 |e| + 4) u32, a = t f one more: da = (3 |e| + 5) u32 |a|;
                gate = da (|sin'|, |cos'| <= 1) + 4 u32 |ref| + 2^-149.  t = 0 is probe E: exactly (1, 0).

MEMORY.  Every output is a window of a sentinel-filled buffer (0x5A..., GUARD elements in front and behind, pad columns
where the ABI has a stride: ldo, ldc / c0; the softmax's [n, ldp) belongs to the window); every byte outside must be unchanged.
In-place outputs (latents, state) start from their data inside the window.  Inputs have finite POISON in pads, in rows past the
end and behind bias and weights; the logits' pads [n, lds) are NaN; the noise z is NaN on rows that must not read it.

THE WALK (`walk`) restates each kernel's indexing in torch on fp64 copies of the same flat buffers (NaN = never stored), with
the named DEFECTS; `failures` applies the checks of the GPU test to its result.
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

import gemm_cases as GC
import norm_cases as NC

DTYPES, POISON, U32 = GC.DTYPES, GC.POISON, GC.U32
Buf, unit_roundoff, worst_ratio = GC.Buf, GC.unit_roundoff, GC.worst_ratio
GUARD = 64
PP_ERR_BAD_ARG, PP_ERR_UNSUPPORTED = -1, -2
LOG2E32 = 1.4426950216293335          # fp32(1.44269504088896340736), the constant of pp_softmax_rows' host side
SENT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
INTS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

DEFECTS = ("stride_loop_second_pass_dropped", "hin_win_swapped", "stride2_odd_last_row_dropped", "clamped_pixel_not_masked",
           "group_crosses_batch_item", "third_load_round_dropped", "scalar_last_block_dropped", "skinny_padded_row_written",
           "skinny_columns_past_grid_dropped", "skinny_rows_past_8_dropped", "softmax_tail_skipped", "softmax_pad_not_zeroed",
           "softmax_reads_logit_pad", "softmax_product_fused_into_subtraction",
           "splice_ext_off_by_one", "splice_tail_bytes_dropped", "blend_mask_per_channel",
           "blend_x0_per_batch_item", "mask_nearest_h_w_swapped", "mask_broadcast_over_batch_dropped", "ticket_not_rearmed",
           "counter_moved_without_ticket", "bmod_ignored", "c0_ignored", "temb_row_ignored", "ksampler_push_before_read",
           "pndm_save_after_update", "z_read_on_quiet_row", "zero_tail_dropped", "nchw_channel_stride_from_ldc",
           "direct_padding_not_zero", "nchw_batch_item_ignored", "pack_halves_swapped", "skinny_last_k_piece_dropped",
           "temb_sin_cos_swapped", "splice_src_row_ignored", "mask_threshold_strict", "mask_sum_le_zero")


class Case(NamedTuple):
    kernel: str
    id: str
    probe: str                     # "E" bit equality, "R" derived gate, "X" refused
    p: dict
    only: Optional[str] = None     # one format only; kernels without a 16-bit side run once ("fp32")
    expect: int = 0                # the error code of a refusal


# ------------------------------------------------------------------------------------------------ memory helpers
def bits(x: torch.Tensor) -> torch.Tensor:
    return x.view(INTS[x.element_size()])


def flat_in(data: torch.Tensor, fill=POISON, guard: int = GUARD) -> Buf:
    """a dense input of any shape as one row of a flat buffer with `guard` poisoned elements in front and behind"""
    n = data.numel()
    full = torch.full((n + 2 * guard,), fill, dtype=data.dtype)
    full[guard:guard + n] = data.reshape(-1)
    return Buf(full, guard, 1, n, n)


def padded_in(data: torch.Tensor, pad: int, fill=POISON, guard: int = GUARD) -> Buf:
    """[rows, cols] with row stride cols + pad, pads and guards filled"""
    rows, cols = data.shape
    ld = cols + pad
    full = torch.full((rows * ld + 2 * guard,), fill, dtype=data.dtype)
    b = Buf(full, guard, rows, cols, ld)
    b.view.copy_(data)
    return b


def window(rows: int, cols: int, pad: int, dtype, init: Optional[torch.Tensor] = None, guard: int = GUARD) -> Buf:
    """an output window [rows, cols] (row stride cols + pad) in a sentinel-filled buffer; `init`: an in-place output's data"""
    ld = cols + pad
    esz = torch.empty(0, dtype=dtype).element_size()
    full = torch.full((rows * ld + 2 * guard,), SENT[esz] if esz < 8 else SENT[8], dtype=INTS[esz]).view(dtype)
    b = Buf(full, guard, rows, cols, ld)
    if init is not None:
        b.view.copy_(init.reshape(rows, cols))
    return b


def outside_clean(b: Buf) -> bool:
    return bool((bits(b.full)[b.outside()] == SENT[b.full.element_size()]).all())


def _emu(b: Buf, keep: bool = False) -> Buf:
    """the fp64 twin of an output window for the walk: NaN everywhere (never stored), the data of an in-place output kept"""
    full = torch.full((b.full.numel(),), math.nan, dtype=torch.float64)
    e = Buf(full, b.base, b.rows, b.cols, b.ld)
    if keep:
        e.view.copy_(b.view.double())
    return e


def _rd(full64: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """a read at flat indices; a defective walk may leave the buffer: it gets the nearest end (poison)"""
    return full64[idx.clamp(0, full64.numel() - 1)]


def _r16(v: torch.Tensor, dtype) -> torch.Tensor:
    return v.to(dtype).double()


def passes(total: int, cap: int, defect=None, per_block: int = 256):
    """the work items of a capped grid: min(cap, ceil(total / per_block)) blocks; pass k covers [k span, (k + 1) span)"""
    grid = min(cap, max(1, -(-total // per_block)))
    span = grid * per_block
    out, k = [], 0
    while k * span < total:
        out.append(torch.arange(k * span, min(total, (k + 1) * span)))
        k += 1
        if defect == "stride_loop_second_pass_dropped":
            break
    return out


def grid_blocks(total: int, cap: int = 4096, per_block: int = 256) -> int:
    return min(cap, max(1, -(-total // per_block)))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _sparse_pm1(g, shape, p):
    return (torch.rand(shape, generator=g) < p).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def _w_exact(g, shape):
    return (torch.randint(0, 2, shape, generator=g).double() + 1) * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def _randn16(g, shape, dtype, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype).double()


def silu_gate(d, pre, ref):
    return 1.1 * d + (7 + pre.abs()) * U32 * ref.abs()


def specials(dtype, n: int, g) -> torch.Tensor:
    """n values of `dtype` (16-bit or fp32) that a copy / add / cast must get bit-right: +-0, subnormals, the largest finite
    values, rounding ties of both 16-bit formats, values whose fp16 cast or sum overflows; no inf, no NaN"""
    fi = torch.finfo(dtype)
    base = [0.0, -0.0, fi.tiny, -fi.tiny, fi.tiny / 4, -fi.tiny / 2, fi.max, -fi.max, fi.max, 1.0, -1.0, 0.5, 65504.0, 65504.0,
            -65504.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0, 65519.996, 2.0 ** -25,
            3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -134, 1e-40, 255.5, 256.5, 2049.0, 2051.0, 33000.0, 40000.0]
    v = torch.tensor(base, dtype=torch.float64).clamp(-fi.max, fi.max).to(dtype)
    r = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 12, (n,), generator=g).float())).to(dtype)
    k = torch.randperm(n, generator=g)[:min(n, v.numel())]
    r[k] = v[:k.numel()]
    return r


# ------------------------------------------------------------------------------------------------ conv_direct
def _conv_direct_ref(x, w, bias, add, s):
    pre = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), None, stride=s, padding=1).permute(0, 2, 3, 1)
    if bias is not None:
        pre = pre + bias
    if add is not None:
        pre = pre + add
    return pre


def build_conv_direct(c, dtype):
    p = c.p
    B, H, W, cin, cout, s = p["B"], p["H"], p["W"], p["cin"], p["cout"], p["stride"]
    ho, wo = (H - 1) // s + 1, (W - 1) // s + 1
    g = GC._gen(11, B, H, W, cin, cout, s, c.probe == "E")
    if c.probe == "E":
        x, w = _sparse_pm1(g, (B, H, W, cin), min(0.5, 24.0 / (9 * cin))), _w_exact(g, (3, 3, cin, cout))
        bias, add = _ints(g, (cout,), -4, 4), _ints(g, (B, ho, wo, cout), -4, 4)
    else:
        x, w = _randn16(g, (B, H, W, cin), dtype), _randn16(g, (3, 3, cin, cout), dtype, (9 * cin) ** -0.5)
        bias, add = torch.randn(cout, generator=g).double(), _randn16(g, (B, ho, wo, cout), dtype)
    bias, add = (bias if p.get("bias", True) else None), (add if p.get("add") else None)
    pre = _conv_direct_ref(x, w, bias, add, s)
    A = _conv_direct_ref(x.abs(), w.abs(), None if bias is None else bias.abs(), None if add is None else add.abs(), s)
    ref = NC.silu64(pre) if p.get("silu") else pre
    t = dict(inp=dict(x=flat_in(x.to(dtype)), w=flat_in(w.to(dtype)), bias=None if bias is None else flat_in(bias.float()),
                      add=None if add is None else flat_in(add.to(dtype))),
             out=dict(out=window(B * ho * wo, cout, 0, dtype)), ref=dict(out=ref.reshape(-1, cout)), gate={})
    if c.probe == "E":
        assert float(A.max()) < 2 ** 24 and bool((ref.to(dtype).double() == ref).all()), (c.id, "probe E is not exact")
    else:
        d = (9 * cin + 2) * U32 * A
        if p.get("silu"):
            d = silu_gate(d, pre, ref)
        t["gate"]["out"] = (unit_roundoff(dtype) * ref.abs() + d).reshape(-1, cout)
    return t


def walk_conv_direct(c, t, dtype, defect=None):
    p = c.p
    B, H, W, cin, cout, s = p["B"], p["H"], p["W"], p["cin"], p["cout"], p["stride"]
    i_ = t["inp"]
    xf, wf = i_["x"].full.double(), i_["w"].full.double()
    o = _emu(t["out"]["out"])
    hout, wout = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    if defect == "stride2_odd_last_row_dropped" and s == 2:
        hout = H // 2 if H > 1 else 1
    S = cout >> 3
    j8, ci = torch.arange(8), torch.arange(cin)
    for i in passes(B * hout * wout * S, 4096, defect):
        sl, pix = i % S, i // S
        ox, oy, b = pix % wout, (pix // wout) % hout, pix // (wout * hout)
        acc = torch.zeros(i.numel(), 8, dtype=torch.float64)
        if i_["bias"] is not None:
            acc += _rd(i_["bias"].full.double(), i_["bias"].base + sl[:, None] * 8 + j8)
        for ky in range(3):
            for kx in range(3):
                iy, ix = oy * s + ky - 1, ox * s + kx - 1
                ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                row = (b * W + iy) * H + ix if defect == "hin_win_swapped" else (b * H + iy) * W + ix
                xv = _rd(xf, i_["x"].base + row[:, None] * cin + ci)
                if defect != "direct_padding_not_zero":
                    xv = xv * ok[:, None]
                wi = i_["w"].base + ((ky * 3 + kx) * cin + ci)[None, :, None] * cout + (sl[:, None, None] * 8 + j8)
                acc += torch.einsum("nc,ncj->nj", xv, _rd(wf, wi))
        oi = pix[:, None] * cout + sl[:, None] * 8 + j8
        if i_["add"] is not None:
            acc += _rd(i_["add"].full.double(), i_["add"].base + oi)
        if p.get("silu"):
            acc = NC.silu64(acc)
        o.full[o.base + oi] = _r16(acc, dtype)
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ conv_out (cout 4)
def conv_out_mfma(cin: int) -> bool:
    return cin % 32 == 0 and cin <= 384


def build_conv_out(c, dtype):
    p = c.p
    B, H, W, cin = p["B"], p["H"], p["W"], p["cin"]
    g = GC._gen(12, B, H, W, cin, c.probe == "E")
    K = 9 * cin
    if c.probe == "E":
        x, w, bias = _sparse_pm1(g, (B, H, W, cin), min(0.5, 256.0 / K)), _w_exact(g, (4, 9, cin)), _ints(g, (4,), -4, 4)
    else:
        x, w = _randn16(g, (B, H, W, cin), dtype), _randn16(g, (4, 9, cin), dtype, K ** -0.5)
        bias = torch.randn(4, generator=g).double()
    if not p.get("bias", True):
        bias = None
    conv = lambda a, b_: F.conv2d(a.permute(0, 3, 1, 2), b_.reshape(4, 3, 3, cin).permute(0, 3, 1, 2), padding=1)   # noqa: E731
    ref = conv(x, w) + (0 if bias is None else bias.view(1, 4, 1, 1))
    A = conv(x.abs(), w.abs()) + (0 if bias is None else bias.abs().view(1, 4, 1, 1))
    t = dict(inp=dict(x=flat_in(x.to(dtype)), w=flat_in(w.to(dtype)), bias=None if bias is None else flat_in(bias.float())),
             out=dict(out=window(B * 4 * H, W, 0, torch.float32)), ref=dict(out=ref.reshape(-1, W)), gate={})
    if c.probe == "E":
        assert float(A.max()) < 2 ** 24, (c.id, "probe E is not exact")
    else:
        t["gate"]["out"] = ((K + 8) * U32 * A).reshape(-1, W)
    return t


def walk_conv_out(c, t, dtype, defect=None):
    p = c.p
    B, H, W, cin = p["B"], p["H"], p["W"], p["cin"]
    i_ = t["inp"]
    xf, wf = i_["x"].full.double(), i_["w"].full.double()
    o = _emu(t["out"]["out"])
    npix = B * H * W
    ci = torch.arange(cin)
    wmat = _rd(wf, i_["w"].base + torch.arange(4 * 9 * cin)).reshape(4, 9, cin)
    bias = _rd(i_["bias"].full.double(), i_["bias"].base + torch.arange(4)) if i_["bias"] is not None else torch.zeros(4, dtype=torch.float64)
    if conv_out_mfma(cin):
        slot = torch.arange(-(-npix // 32) * 32)
        pv = slot < npix
        pc = torch.where(pv, slot, torch.tensor(npix - 1))
        ox, oy = pc % W, (pc // W) % H
        own = pc if defect != "group_crosses_batch_item" else torch.clamp((slot // 16) * 16, max=npix - 1)
        img = (own // (W * H)) * H * W
        steps = cin >> 5
        live = sorted({wv + 4 * j for wv in range(4) for j in range(2 if defect == "third_load_round_dropped" else 3) if wv + 4 * j < steps})
        lc = torch.cat([torch.arange(32 * s_, 32 * s_ + 32) for s_ in live])
        acc = torch.zeros(slot.numel(), 4, dtype=torch.float64)
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            iy, ix = oy + ky - 1, ox + kx - 1
            ok = pv & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            addr = (img + torch.where(ok, iy, oy) * W + torch.where(ok, ix, ox)) * cin
            xv = _rd(xf, i_["x"].base + addr[:, None] + ci)
            if defect != "clamped_pixel_not_masked":
                xv = xv * ok[:, None]
            acc += xv[:, lc] @ wmat[:, tap, lc].t()
        q = slot[pv]
        acc = acc[pv]
    else:
        nblk = -(-npix // 4) if defect != "scalar_last_block_dropped" else npix // 4
        q = torch.arange(min(npix, nblk * 4))
        ox, oy, b = q % W, (q // W) % H, q // (W * H)
        acc = torch.zeros(q.numel(), 4, dtype=torch.float64)
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            iy, ix = oy + ky - 1, ox + kx - 1
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            xv = _rd(xf, i_["x"].base + (((b * H + iy) * W + ix) * cin)[:, None] + ci) * ok[:, None]
            acc += xv @ wmat[:, tap, :].t()
    qx, qy, qb = q % W, (q // W) % H, q // (W * H)
    r = torch.arange(4)
    o.full[o.base + ((qb[:, None] * 4 + r) * H + qy[:, None]) * W + qx[:, None]] = (acc + bias).float().double()
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ layout, add
SRC_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def build_to_nhwc(c, dtype):
    p = c.p
    B, ch, hw, bmod, ldc, c0 = p["B"], p["c"], p["hw"], p["bmod"], p["ldc"], p["c0"]
    sdt = SRC_DT[p["src"]]
    nb = bmod if bmod > 0 else B
    src = specials(sdt, nb * ch * hw, GC._gen(13, B, ch, hw, bmod)).reshape(nb, ch, hw)
    full = src[torch.arange(B) % nb]
    ref = full.float().to(dtype).permute(0, 2, 1).reshape(B * hw, ch)
    return dict(inp=dict(src=flat_in(src)), out=dict(dst=window(B * hw, ldc, 0, dtype)), ref=dict(dst=ref), gate={},
                cols=dict(dst=(c0, ch)))


def walk_to_nhwc(c, t, dtype, defect=None):
    p = c.p
    B, ch, hw, bmod, ldc, c0 = p["B"], p["c"], p["hw"], p["bmod"], p["ldc"], p["c0"]
    s = t["inp"]["src"]
    sf = s.full.double()
    o = _emu(t["out"]["dst"])
    if defect == "c0_ignored":
        c0 = 0
    j = torch.arange(ch)
    for i in passes(B * hw, 4096, defect):
        b, pp = i // hw, i % hw
        sb = b % bmod if bmod > 0 and defect != "bmod_ignored" else b
        cs = ldc if defect == "nchw_channel_stride_from_ldc" else ch
        v = _rd(sf, s.base + (sb[:, None] * cs + j) * hw + pp[:, None])
        o.full[o.base + i[:, None] * ldc + c0 + j] = v.float().to(dtype).double()
    return dict(dst=o)


def build_to_nchw(c, dtype):
    p = c.p
    B, ch, hw = p["B"], p["c"], p["hw"]
    src = specials(dtype, B * hw * ch, GC._gen(14, B, ch, hw)).reshape(B, hw, ch)
    odt = torch.float32 if p["dst"] == "f32" else dtype
    return dict(inp=dict(src=flat_in(src)), out=dict(dst=window(B * ch, hw, 0, odt)),
                ref=dict(dst=src.permute(0, 2, 1).reshape(B * ch, hw).to(odt)), gate={})


def walk_to_nchw(c, t, dtype, defect=None):
    p = c.p
    B, ch, hw = p["B"], p["c"], p["hw"]
    s = t["inp"]["src"]
    o = _emu(t["out"]["dst"])
    for i in passes(B * ch * hw, 4096, defect):
        pp, cc, b = i % hw, (i // hw) % ch, i // (hw * ch)
        if defect == "nchw_batch_item_ignored":
            b = torch.zeros_like(b)
        o.full[o.base + i] = _rd(s.full.double(), s.base + (b * hw + pp) * ch + cc)
    return dict(dst=o)


def build_add(c, dtype):
    n = c.p["n"]
    g = GC._gen(15, n)
    a, b = specials(dtype, n, g), specials(dtype, n, g)
    if dtype == torch.float16 and n >= 8:
        a[:2], b[:2] = torch.tensor([65504.0, -65504.0], dtype=dtype), torch.tensor([65504.0, -40000.0], dtype=dtype)   # -> inf
    return dict(inp=dict(a=flat_in(a), b=flat_in(b)), out=dict(out=window(1, n, 0, dtype)),
                ref=dict(out=(a.double() + b.double()).to(dtype).reshape(1, n)), gate={})


def walk_add(c, t, dtype, defect=None):
    n = c.p["n"]
    a, b = t["inp"]["a"], t["inp"]["b"]
    o = _emu(t["out"]["out"])
    j = torch.arange(8)
    for i in passes(n // 8, 4096, defect):
        k = (i[:, None] * 8 + j).reshape(-1)
        ko = k ^ 1 if defect == "pack_halves_swapped" else k
        o.full[o.base + ko] = (_rd(a.full.double(), a.base + k) + _rd(b.full.double(), b.base + k)).to(dtype).double()
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ skinny linear
def skinny_template(rows: int) -> int:
    return 1 if rows == 1 else 4 if rows <= 4 else 8 if rows <= 8 else 16


def refuses_skinny(p) -> int:
    if p["rows"] <= 0 or p["rows"] > 16 or p["K"] <= 0 or p["K"] % 8 or p["N"] <= 0:
        return PP_ERR_BAD_ARG
    return PP_ERR_UNSUPPORTED if skinny_template(p["rows"]) * p["K"] * 4 > 160 * 1024 else 0


def build_skinny(c, dtype):
    p = c.p
    rows, K, N, pad = p["rows"], p["K"], p["N"], p.get("pad", 8)
    g = GC._gen(16, rows, K, N, c.probe == "E")
    if c.probe == "X":
        z = torch.zeros
        return dict(inp=dict(x=flat_in(z(max(1, rows * K))), w=flat_in(z(max(1, N * K)).to(dtype)), bias=flat_in(z(N))),
                    out=dict(out=window(min(max(rows, 1), 16), N, pad, torch.float32)), ref={}, gate={})
    if c.probe == "E":
        x = _sparse_pm1(g, (rows, K), min(0.5, 256.0 / K)) * _ints(g, (rows, K), 1, 2)
        w, bias = _w_exact(g, (N, K)), _ints(g, (N,), -4, 4)
    else:
        x, w = torch.randn(rows, K, generator=g).double(), _randn16(g, (N, K), dtype, K ** -0.5)
        bias = torch.randn(N, generator=g).double()
    if not p.get("bias", True):
        bias = None
    xa = NC.silu64(x) if p.get("act_in") else x
    pre = xa @ w.t() + (0 if bias is None else bias)
    A = xa.abs() @ w.abs().t() + (0 if bias is None else bias.abs())
    ref = NC.silu64(pre) if p.get("act_out") else pre
    t = dict(inp=dict(x=flat_in(x.float()), w=flat_in(w.to(dtype)), bias=None if bias is None else flat_in(bias.float())),
             out=dict(out=window(rows, N, pad, torch.float32, guard=16 * (N + pad))), ref=dict(out=ref), gate={})
    if c.probe == "E":
        assert float(A.max()) < 2 ** 24, (c.id, "probe E is not exact")
    else:
        d = (K + 7) * U32 * A
        if p.get("act_in"):
            d = d + (((7 + x.abs()) * U32 * xa.abs()) @ w.abs().t())
        if p.get("act_out"):
            d = silu_gate(d, pre, ref)
        t["gate"]["out"] = d
    return t


def walk_skinny(c, t, dtype, defect=None):
    p = c.p
    rows, K, N = p["rows"], p["K"], p["N"]
    i_ = t["inp"]
    o = _emu(t["out"]["out"])
    R = skinny_template(rows)
    if defect == "skinny_rows_past_8_dropped":
        R = min(R, 8)
    xs = torch.zeros(R, K, dtype=torch.float64)                      # the LDS copy: rows past `rows` are zero
    live = min(rows, R)
    xs[:live] = _rd(i_["x"].full.double(), i_["x"].base + torch.arange(live * K)).reshape(live, K)
    if p.get("act_in"):
        xs = NC.silu64(xs)
    if defect == "skinny_last_k_piece_dropped":
        xs[:, K - 8:] = 0.0
    nb = min(2048, (N + 3) // 4)
    n = torch.arange(nb * 4)
    cols = []
    while n[0] < N:
        cols.append(n[n < N])
        n = n + nb * 4
        if defect == "skinny_columns_past_grid_dropped":
            break
    for n in cols:
        wv = _rd(i_["w"].full.double(), i_["w"].base + n[:, None] * K + torch.arange(K))
        v = xs @ wv.t()
        if i_["bias"] is not None:
            v = v + _rd(i_["bias"].full.double(), i_["bias"].base + n)
        if p.get("act_out"):
            v = NC.silu64(v)
        nr = R if defect == "skinny_padded_row_written" else min(rows, R)
        r = torch.arange(nr)
        o.full[o.base + r[:, None] * o.ld + n] = v[:nr].float().double()
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ timestep embedding
LN1E4_32 = 9.210340499877930          # fp32(9.210340371976184): the constant as the kernel holds it


def build_temb(c, dtype):
    p = c.p
    tv, rows, dim = p["t"], p["rows"], p["dim"]
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    e = -math.log(10000.0) * k / half
    a = tv * torch.exp(e)
    ref = torch.cat([torch.cos(a), torch.sin(a)]).expand(rows, dim).clone()
    t = dict(inp=dict(t=flat_in(torch.tensor([tv], dtype=torch.float32))), out=dict(out=window(rows, dim, 0, torch.float32)),
             ref=dict(out=ref), gate={})
    if c.probe == "R":
        da = ((3 * e.abs() + 5) * U32 * a.abs()).repeat(2).expand(rows, dim)
        t["gate"]["out"] = da + 4 * U32 * ref.abs() + 2.0 ** -149
    return t


def walk_temb(c, t, dtype, defect=None):
    p = c.p
    rows, dim = p["rows"], p["dim"]
    half = dim >> 1
    o = _emu(t["out"]["out"])
    tv = float(t["inp"]["t"].view[0, 0])
    i = torch.arange(rows * half)
    r = i // half
    k = i - r * half
    if defect == "temb_row_ignored":
        r = torch.zeros_like(r)
    a = tv * torch.exp(-math.log(10000.0) * k.double() / half)
    first, second = (torch.sin(a), torch.cos(a)) if defect == "temb_sin_cos_swapped" else (torch.cos(a), torch.sin(a))
    o.full[o.base + r * dim + k] = first.float().double()
    o.full[o.base + r * dim + half + k] = second.float().double()
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ softmax rows
def refuses_softmax(p) -> int:
    n, lds, ldp = p["n"], p["lds"], p["ldp"]
    if p["rows"] <= 0 or n <= 0 or lds < n or ldp < n or lds & 3 or ldp & 3 or p.get("s_off", 0) & 15 or p.get("p_off", 0) & 7:
        return PP_ERR_BAD_ARG
    return 0


def build_softmax(c, dtype):
    p = c.p
    rows, n, lds, ldp, scale, regime = p["rows"], p["n"], p["lds"], p["ldp"], p["scale"], p["regime"]
    g = GC._gen(17, rows, n, lds, ldp, len(regime))
    if c.probe == "X":
        return dict(inp=dict(s=flat_in(torch.zeros(rows * max(lds, n) + 8))), out=dict(p=window(rows, max(ldp, n, 4), 0, dtype)), ref={}, gate={})
    l32 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32))
    if regime == "normal":
        s = torch.randn(rows, n, generator=g) * 30
    elif regime == "equal":
        s = torch.full((rows, n), 3.25)
    elif regime == "spike":
        s = torch.randn(rows, n, generator=g)
        s[torch.arange(rows), torch.randint(0, n, (rows,), generator=g)] += 60.0
    elif regime == "onehot":                            # ahead by > 160 in the exp2 domain: the hot index walks body, tail, ends
        s = torch.randn(rows, n, generator=g)
        hot = torch.tensor([n - 1, 0, n // 2])[:rows]
        s[torch.arange(rows), hot] += 170.0 / l32
    else:                                               # "largest": +-FLT_MAX / 2 at scale such that scale log2e s stays finite
        big = torch.finfo(torch.float32).max / 2
        s = torch.full((rows, n), -big)
        s[:, 0] = big
        s[:, n - 1] = big
    s = s.float()
    x = s.double() * l32
    M = x.max(1, keepdim=True).values
    pr = torch.exp2(x - M)
    ref = torch.zeros(rows, ldp, dtype=torch.float64)
    ref[:, :n] = pr / pr.sum(1, keepdim=True)
    t = dict(inp=dict(s=padded_in(s, lds - n, fill=math.nan)), out=dict(p=window(rows, ldp, 0, dtype)), ref=dict(p=ref), gate={})
    if c.probe == "E":
        e = ref.to(dtype).double()                       # (2^-170 is not 0 in fp64; it is in fp32 and after the one cast)
        assert bool(((e == 0) | (e == 1) | (e == 0.5)).all()) and float((ref - e).abs().max()) < 2.0 ** -140, c.id
        if regime == "onehot":
            assert n == 1 or bool((x - M)[e[:, :n] == 0].max() < -160), c.id
    else:
        D = 2 * U32 * (x.abs() + M.abs())
        n_s = 3 * (-(-n // 256) + 16) + 3
        sub = 2.0 ** -25 if dtype == torch.float16 else 2.0 ** -134
        gt = torch.zeros_like(ref)
        pp = ref[:, :n]
        gt[:, :n] = unit_roundoff(dtype) * pp + pp * (torch.exp2(2 * D) - 1) + (n_s + 4) * U32 * pp + sub
        t["gate"]["p"] = gt
    return t


def walk_softmax(c, t, dtype, defect=None):
    p = c.p
    rows, n, lds, ldp, scale = p["rows"], p["n"], p["lds"], p["ldp"], p["scale"]
    s = t["inp"]["s"]
    o = _emu(t["out"]["p"])
    l32 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32))
    n4 = n >> 2
    body, tail = torch.arange(n4 * 4), torch.arange(n4 * 4, n)
    if defect == "softmax_reads_logit_pad":
        body = torch.arange(-(-n // 4) * 4)
        tail = tail[:0]
    for r in range(rows):
        xb = _rd(s.full.double(), s.base + r * lds + body) * l32
        xt = _rd(s.full.double(), s.base + r * lds + tail) * l32
        if defect == "softmax_tail_skipped":
            xt = xt[:0]
        allx = torch.cat([xb, xt])
        # the maximum is taken from the fp32-ROUNDED products; so is every exponent, unless the product rides an fma
        M = allx.float().double().max() if allx.numel() else torch.tensor(-math.inf, dtype=torch.float64)
        if defect != "softmax_product_fused_into_subtraction":
            xb, xt, allx = xb.float().double(), xt.float().double(), allx.float().double()
        S = torch.exp2(allx - M).sum()
        o.full[o.base + r * ldp + body[body < ldp]] = _r16(torch.exp2(xb - M) / S, dtype)[body < ldp]
        if xt.numel():
            o.full[o.base + r * ldp + tail] = _r16(torch.exp2(xt - M) / S, dtype)
        if defect != "softmax_pad_not_zeroed":
            o.full[o.base + r * ldp + torch.arange(n, ldp)] = 0.0
    return dict(p=o)


# ------------------------------------------------------------------------------------------------ embedding splice
def splice_width(t_off: int, e_off: int, o_off: int, row_bytes: int) -> int:
    al = t_off | e_off | o_off | row_bytes
    return 16 if al & 15 == 0 else 4 if al & 3 == 0 else 1


def build_splice(c, dtype):
    p = c.p
    nr, rb, nt, ne = p["n_rows"], p["row_bytes"], p["n_table"], p["n_ext"]
    g = GC._gen(18, nr, rb, nt, ne)
    table = torch.randint(0, 256, (nt, rb), generator=g, dtype=torch.uint8)
    ext = torch.randint(0, 256, (max(ne, 1), rb), generator=g, dtype=torch.uint8)
    src = torch.randint(0, nt, (nr,), generator=g, dtype=torch.int32)
    if ne:
        k = torch.arange(nr) % 3 == 1
        src[k] = -1 - (torch.arange(nr, dtype=torch.int32)[k] % ne)
        src[nr // 2] = -ne                              # the last ext row
    src[0], src[-1] = (nt - 1, 0) if nr > 1 else (nt - 1, nt - 1)
    ref = torch.where((src >= 0)[:, None], table[src.clamp(min=0).long()], ext[(-src - 1).clamp(min=0).long()])
    # a misaligned base: `off` bytes into a buffer whose guard keeps 16-byte alignment otherwise
    return dict(inp=dict(table=flat_in(table, fill=0xEE, guard=GUARD + p.get("t_off", 0)),
                         ext=flat_in(ext, fill=0xEE, guard=GUARD + p.get("t_off", 0)) if ne else None,
                         src=flat_in(src, fill=0)),
                out=dict(out=window(nr, rb, 0, torch.uint8, guard=GUARD + p.get("o_off", 0))), ref=dict(out=ref), gate={})


def walk_splice(c, t, dtype, defect=None):
    p = c.p
    nr, rb = p["n_rows"], p["row_bytes"]
    i_ = t["inp"]
    o = _emu(t["out"]["out"])
    tab = i_["table"]
    ext = i_["ext"] if i_["ext"] is not None else tab
    width = splice_width(p.get("t_off", 0), p.get("t_off", 0), p.get("o_off", 0), rb)
    if defect == "splice_tail_bytes_dropped":           # the width from the bases alone: row_bytes / width truncates
        width = splice_width(p.get("t_off", 0), p.get("t_off", 0), p.get("o_off", 0), 0)
    nbytes = rb // width * width
    j = torch.arange(nbytes)
    for r in range(nr):
        s = r if defect == "splice_src_row_ignored" else int(i_["src"].view[0, r])
        if s >= 0:
            v = _rd(tab.full.double(), tab.base + s * rb + j)
        else:
            v = _rd(ext.full.double(), ext.base + ((-s) if defect == "splice_ext_off_by_one" else (-s - 1)) * rb + j)
        o.full[o.base + r * rb + j] = v
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ step head, zero
def build_step_head(c, dtype):
    p = c.p
    B, ch, hw, bmod, ldc, c0, rf, nz, scaled = p["B"], p["c"], p["hw"], p["bmod"], p["ldc"], p["c0"], p["row_floats"], p["nz"], p["scaled"]
    g = GC._gen(19, B, ch, hw, bmod, rf, nz)
    steps, step = 4, 2
    table = torch.randn(steps, rf, generator=g)
    nb = bmod if bmod > 0 else B
    lat = specials(torch.float32, nb * ch * hw, g).reshape(nb, ch, hw)
    div = torch.tensor([3.0, 0.25, 2.0, 8.0])            # powers of two on the row that is read: the division is exact
    v = lat[torch.arange(B) % nb].double() / (div[step].double() if scaled else 1.0)
    ref = v.float().to(dtype).permute(0, 2, 1).reshape(B * hw, ch)
    return dict(inp=dict(table=flat_in(table), lat=flat_in(lat), step=flat_in(torch.tensor([step], dtype=torch.int32), fill=0),
                         div=flat_in(div) if scaled else None),
                out=dict(temb=window(1, rf, 0, torch.float32), x=window(B * hw, ldc, 0, dtype), z=window(1, nz, 0, torch.int64)),
                ref=dict(temb=table[step].reshape(1, rf), x=ref, z=torch.zeros(1, nz, dtype=torch.int64)), gate={}, cols=dict(x=(c0, ch)))


def walk_step_head(c, t, dtype, defect=None):
    p = c.p
    B, ch, hw, bmod, ldc, c0, rf, nz, scaled = p["B"], p["c"], p["hw"], p["bmod"], p["ldc"], p["c0"], p["row_floats"], p["nz"], p["scaled"]
    i_ = t["inp"]
    o = {k: _emu(b) for k, b in t["out"].items()}
    step = int(i_["step"].view[0, 0])
    for i in passes(rf, 64, defect):
        o["temb"].full[o["temb"].base + i] = _rd(i_["table"].full.double(), i_["table"].base + step * rf + i)
    d = float(_rd(i_["div"].full.double(), torch.tensor(i_["div"].base + step))) if scaled else 1.0
    if defect == "c0_ignored":
        c0 = 0
    j = torch.arange(ch)
    for i in passes(B * hw, 256, defect):
        b, pp = i // hw, i % hw
        sb = b % bmod if bmod > 0 and defect != "bmod_ignored" else b
        v = _rd(i_["lat"].full.double(), i_["lat"].base + (sb[:, None] * ch + j) * hw + pp[:, None]) / d
        o["x"].full[o["x"].base + i[:, None] * ldc + c0 + j] = v.float().to(dtype).double()
    for i in passes(nz if defect != "zero_tail_dropped" else nz // 256 * 256, 256, defect):
        o["z"].full[o["z"].base + i] = 0.0
    return o


def build_zero(c, dtype):
    n = c.p["n"]
    return dict(inp={}, out=dict(z=window(1, n, 0, torch.int64)), ref=dict(z=torch.zeros(1, n, dtype=torch.int64)), gate={})


def walk_zero(c, t, dtype, defect=None):
    n = c.p["n"]
    o = _emu(t["out"]["z"])
    for i in passes(n if defect != "zero_tail_dropped" else n // 256 * 256, 1024, defect):
        o.full[o.base + i] = 0.0
    return dict(z=o)


# ------------------------------------------------------------------------------------------------ step kernels
# operations of the longest formula of each kernel (cfg combine: 3) + 1
N_R = {"ddim": 3 + 3 + 3 + 1, "dpm": 3 + 3 + 2 + 5 + 1, "pndm": 3 + 7 + 3 + 1, "unipc": 3 + 3 + 9 + 7 + 1, "lcm": 3 + 3 + 3 + 3 + 1,
       "sigma": 3 + 2 + 2 + 1, "ksampler": 3 + 8 + 2 + 1, "noise": 2 + 1}
STEP_STATE = {"ddim": 0, "dpm": 1, "pndm": 5, "unipc": 4, "lcm": 0, "sigma": 0, "ksampler": 4, "noise": 0}
STEP_ROW = {"ddim": 8, "dpm": 8, "pndm": 16, "unipc": 16, "lcm": 8, "sigma": 8, "ksampler": 16, "noise": 8}
STEP_NOISE = ("lcm", "sigma", "ksampler", "noise")


def step_formula(kernel, row, e, x, st, z, ab=False, defect=None):
    """one element-wise application of a table row (fp64 tensors; st [slots, n] or None) -> (x', st').  ab: the absolute-value
    evaluation that is the A of the gate (operands and coefficients are magnitudes already, subtractions add)."""
    sub = (lambda a, b: a + b) if ab else (lambda a, b: a - b)
    c = row
    st2 = st.clone() if st is not None else None
    if kernel == "ddim":
        x0 = sub(x, c[0] * e) / c[1]
        return c[2] * x0 + c[3] * e, st2
    if kernel == "dpm":
        x0 = sub(x, c[0] * e) / c[1]
        d1 = c[5] * sub(x0, st[0])
        st2[0] = x0
        return sub(sub(c[2] * x, c[3] * x0), c[4] * d1), st2
    if kernel == "pndm":
        h1, h2, h3, push = st[int(c[6])], st[int(c[7])], st[int(c[8])], int(c[9])
        mo = c[0] * e + c[1] * h1 + c[2] * h2 + c[3] * h3
        src = st[4] if c[10] != 0 else x
        xn = c[4] * src + c[5] * mo
        if c[11] != 0:
            st2[4] = xn if defect == "pndm_save_after_update" else x
        if push >= 0:
            st2[push] = e
        return xn, st2
    if kernel == "unipc":
        x0 = sub(x, c[0] * e) / c[1]
        a1, a2 = st[1], st[2]
        xc = x
        if c[2] != 0:
            xc = c[3] * st[0] + c[4] * a1 + c[5] * a2 + c[6] * st[3] + c[7] * x0
        st2[0], st2[3], st2[2], st2[1] = xc, a2, a1, x0
        return c[8] * xc + c[9] * x0 + c[10] * a1 + c[11] * a2, st2
    if kernel == "lcm":
        x0 = sub(x, c[0] * e) / c[1]
        den = c[2] * x0 + c[3] * x
        quiet = c[5] == 0 and defect != "z_read_on_quiet_row"
        return (den if quiet else c[4] * den + c[5] * z), st2
    if kernel == "sigma":
        xn = x + c[1] * e
        quiet = c[2] == 0 and defect != "z_read_on_quiet_row"
        return (xn if quiet else xn + c[2] * z), st2
    if kernel == "ksampler":
        clampi = lambda v: min(max(int(v), 0), 2)      # noqa: E731
        s1, s2, s3, push = clampi(c[6]), clampi(c[7]), clampi(c[8]), min(int(c[9]), 2)
        hist = st
        if defect == "ksampler_push_before_read" and push >= 0:
            hist = st.clone()
            hist[push] = e
        xn = (st[3] if c[10] != 0 else x) + c[0] * e + c[1] * hist[s1] + c[2] * hist[s2] + c[3] * hist[s3]
        if c[4] != 0 or defect == "z_read_on_quiet_row":
            xn = xn + c[4] * z
        if c[11] != 0:
            st2[3] = x
        if push >= 0:
            st2[push] = e
        return xn, st2
    if kernel == "noise":
        return x + c[4] * z, st2
    raise KeyError(kernel)


# hand-written table rows: (exact rows for probe E: integers / powers of two; c1, al = 0.5 or 2), two consecutive rows each
STEP_ROWS = {
    "ddim": {"E": [[2, 0.5, 3, -2, 0, 0, 0, 0], [1, 2, 0.5, 4, 0, 0, 0, 0]], "R": [[0.6, 0.8, 0.9, 0.43, 0, 0, 0, 0], [0.5, 0.86, 0.95, 0.3, 0, 0, 0, 0]]},
    "dpm": {"E": [[2, 0.5, 3, -2, -1, 2, 0, 0], [1, 2, 0.5, 4, 2, 0.5, 0, 0]], "R": [[0.6, 0.8, 0.83, -0.21, -0.105, 1.3, 0, 0], [0.5, 0.86, 0.7, -0.3, 0, 0.8, 0, 0]]},
    "pndm": {"E": [[2, -1, 3, 0.5, 2, -3, 0, 1, 2, 3, 0, 1, 0, 0, 0, 0], [1, 2, -0.5, 1, 0.5, 2, 3, 0, 1, -1, 1, 0, 0, 0, 0, 0]],
             "R": [[2.29, -2.46, 1.54, -0.375, 1.02, -0.11, 0, 1, 2, 3, 0, 1, 0, 0, 0, 0], [0.5, 0.5, 0, 0, 1.03, -0.13, 3, 0, 1, -1, 1, 0, 0, 0, 0, 0]]},
    "unipc": {"E": [[2, 0.5, 0, 9, 9, 9, 9, 9, 2, -1, 3, 0.5, 0, 0, 0, 0], [1, 2, 1, 2, -1, 0.5, 3, -2, 0.5, 2, -1, 1, 0, 0, 0, 0]],
              "R": [[0.6, 0.8, 0, 9, 9, 9, 9, 9, 0.83, 0.21, 0.11, -0.04, 0, 0, 0, 0], [0.5, 0.86, 1, 0.8, 0.1, -0.07, 0.02, 0.12, 0.7, 0.33, 0.09, -0.03, 0, 0, 0, 0]]},
    "lcm": {"E": [[2, 0.5, 3, -1, 2, 0.5, 0, 0], [1, 2, 0.5, 2, 1, 0, 0, 0]], "R": [[0.6, 0.8, 0.98, 0.02, 0.9, 0.43, 0, 0], [0.5, 0.86, 0.9, 0.1, 1, 0, 0, 0]]},
    "sigma": {"E": [[7, -2, 0.5, 0, 0, 0, 0, 0], [5, 3, 0, 0, 0, 0, 0, 0]], "R": [[7.1, -2.3, 1.7, 0, 0, 0, 0, 0], [4.8, -1.9, 0, 0, 0, 0, 0, 0]]},
    # row 1 pushes into slot 1, which it reads as h2; row 2 uses the saved sample, reads what row 1 pushed, no noise
    "ksampler": {"E": [[2, -1, 3, 0.5, 2, 7, 0, 1, 2, 1, 0, 1, 0, 0, 0, 0], [1, 2, -0.5, 1, 0, 5, 1, 2, 0, -1, 1, 0, 0, 0, 0, 0]],
                 "R": [[-2.3, 0.7, -0.4, 0.1, 1.7, 7.1, 0, 1, 2, 1, 0, 1, 0, 0, 0, 0], [-0.95, -0.95, 0.2, 0.05, 0, 4.8, 1, 2, 0, -1, 1, 0, 0, 0, 0, 0]]},
    "noise": {"E": [[9, 9, 9, 9, 2, 0, 0, 0], [9, 9, 9, 9, -0.5, 0, 0, 0]], "R": [[9, 9, 9, 9, 0.37, 0, 0, 0], [9, 9, 9, 9, 0.21, 0, 0, 0]]},
}
STEP_FIRST = 1                       # the counter's value before the first launch: row 0 and the row behind are poison


def step_quiet(kernel, row) -> bool:
    """a row on which the noise must not be read"""
    return (kernel == "lcm" and row[5] == 0) or (kernel in ("sigma",) and row[2] == 0) or (kernel == "ksampler" and row[4] == 0)


def build_step(c, dtype):
    p = c.p
    k, n, cfg, ticket = p["kind"], p["n"], p["cfg"], p["ticket"]
    g = GC._gen(20, n, cfg, ticket, len(k), c.probe == "E")
    rows = torch.tensor(STEP_ROWS[k][c.probe], dtype=torch.float64)
    W = STEP_ROW[k]
    table = torch.full((4, W), POISON, dtype=torch.float64)
    table[STEP_FIRST:STEP_FIRST + 2] = rows
    ns = STEP_STATE[k]
    launches = 2 if ticket else 1
    if c.probe == "E":
        gs = 3.0
        draw = lambda *s: _ints(g, s, -3, 3)           # noqa: E731
    else:
        gs = 7.5
        draw = lambda *s: torch.randn(*s, generator=g).float().double()   # noqa: E731
    eps = [draw(2 if cfg else 1, n) for _ in range(launches)]
    zs = [draw(n) for _ in range(launches)]
    x, st = draw(n), (draw(ns, n) if ns else None)
    xr, sr = x.clone(), (st.clone() if ns else None)
    Ax, As = x.abs(), (st.abs() if ns else None)
    for j in range(launches):
        row = rows[j]
        e = eps[j][0] + gs * (eps[j][1] - eps[j][0]) if cfg else eps[j][0]
        ea = eps[j][0].abs() + gs * (eps[j][1].abs() + eps[j][0].abs()) if cfg else eps[j][0].abs()
        ra = row.abs()
        if k in ("pndm", "ksampler"):
            ra[6:] = row[6:]                            # slots and flags keep their values
        if step_quiet(k, row):
            zs[j] = torch.full((n,), math.nan, dtype=torch.float64)
        za = torch.nan_to_num(zs[j].abs(), nan=0.0)
        # A is accumulated over the launches: the second launch's inputs carry the first one's bound
        Ax, As = step_formula(k, ra, ea, Ax, As, za, ab=True)
        xr, sr = step_formula(k, row, e, xr, sr, zs[j])
    t = dict(inp=dict(eps=[flat_in(e.float()) for e in eps], z=[flat_in(z.float()) for z in zs], table=flat_in(table.float()),
                      step=None, gs=gs),
             out=dict(x=window(1, n, 0, torch.float32, init=x.float()), step=window(1, 1, 0, torch.int32, init=torch.tensor([STEP_FIRST], dtype=torch.int32)),
                      ticket=window(1, 1, 0, torch.int32, init=torch.zeros(1, dtype=torch.int32))),
             ref=dict(x=xr.reshape(1, n)), gate={}, launches=launches)
    if ns:
        t["out"]["state"] = window(ns, n, 0, torch.float32, init=st.float())
        t["ref"]["state"] = sr
    if c.probe == "E":
        for name, r in t["ref"].items():
            assert bool((r.float().double() == r).all()) and float(r.abs().max()) < 2 ** 24, (c.id, name, "probe E is not exact")
    else:
        t["gate"]["x"] = (launches * N_R[k] * U32 * Ax).reshape(1, n)
        if ns:
            t["gate"]["state"] = launches * N_R[k] * U32 * As
    return t


def walk_step(c, t, dtype, defect=None):
    p = c.p
    k, n, cfg, ticket = p["kind"], p["n"], p["cfg"], p["ticket"]
    i_ = t["inp"]
    o = {name: _emu(b, keep=True) for name, b in t["out"].items()}
    tab = i_["table"]
    W = STEP_ROW[k]
    grid = grid_blocks(n)
    for j in range(t["launches"]):
        step = int(o["step"].view[0, 0])
        row = _rd(tab.full.double(), tab.base + step * W + torch.arange(W))
        ef, zf = i_["eps"][j], i_["z"][j]
        for i in passes(n, 4096, defect):
            e = _rd(ef.full.double(), ef.base + i)
            if cfg:
                e = e + i_["gs"] * (_rd(ef.full.double(), ef.base + n + i) - e)
            x = o["x"].full[o["x"].base + i]
            st = None
            if "state" in o:
                sb = o["state"]
                st = sb.full[sb.base + torch.arange(sb.rows)[:, None] * n + i]
            xn, st2 = step_formula(k, row, e, x, st, _rd(zf.full.double(), zf.base + i), defect=defect)
            o["x"].full[o["x"].base + i] = xn.float().double()
            if st is not None:
                sb.full[sb.base + torch.arange(sb.rows)[:, None] * n + i] = st2.float().double()
        if ticket:                                       # every block draws one ticket; the last one re-arms and advances
            tk = o["ticket"].view
            tk[0, 0] += grid
            if tk[0, 0] == grid:
                if defect != "ticket_not_rearmed":
                    tk[0, 0] = 0
                o["step"].view[0, 0] += 1
        elif defect == "counter_moved_without_ticket":
            o["step"].view[0, 0] += 1
    return o


# ------------------------------------------------------------------------------------------------ latent blend
BLEND_ROWS = {"E": [[0.5, 2.0], [2.0, -0.5], [1.0, 0.0]], "R": [[0.3, 0.95], [0.8, 0.6], [1.0, 0.0]]}


def build_blend(c, dtype):
    p = c.p
    B, C, hw, r = p["B"], p["C"], p["hw"], p["row"]
    g = GC._gen(21, B, C, hw, r, c.probe == "E")
    n = B * C * hw
    tab = torch.tensor(BLEND_ROWS[c.probe], dtype=torch.float64)
    a, b = tab[r]
    if c.probe == "E":
        x, x0, z = _ints(g, (B, C, hw), -4, 4), _ints(g, (C, hw), -4, 4), _ints(g, (B, C, hw), -4, 4)
        m = torch.randint(0, 3, (hw,), generator=g).double() / 2          # 0, 0.5, 1: differs between pixels
    else:
        x, x0, z = (torch.randn(s, generator=g).float().double() for s in ((B, C, hw), (C, hw), (B, C, hw)))
        m = torch.rand(hw, generator=g).float().double()
    x0 = x0 + torch.arange(C, dtype=torch.float64)[:, None] * (8 if c.probe == "E" else 0.0)   # differs between channels
    if b == 0:
        z = torch.full_like(z, math.nan)
    proper = x0.expand(B, C, hw) if b == 0 else a * x0 + b * z
    ref = (1 - m) * proper + m * x
    A = (1 + m) * (x0.abs().expand(B, C, hw) if b == 0 else a.abs() * x0.abs() + b.abs() * z.abs()) + m * x.abs()
    t = dict(inp=dict(x0=flat_in(x0.float()), m=flat_in(m.float()), z=flat_in(z.float()), tab=flat_in(tab.float()),
                      step=flat_in(torch.tensor([r], dtype=torch.int32), fill=0)),
             out=dict(x=window(1, n, 0, torch.float32, init=x.float())), ref=dict(x=ref.reshape(1, n)), gate={})
    if c.probe == "E":
        assert bool((ref.float().double() == ref).all()), c.id
    else:
        t["gate"]["x"] = (8 * U32 * A).reshape(1, n)
    return t


def walk_blend(c, t, dtype, defect=None):
    p = c.p
    B, C, hw = p["B"], p["C"], p["hw"]
    i_ = t["inp"]
    o = _emu(t["out"]["x"], keep=True)
    n, chw = B * C * hw, C * hw
    r = int(i_["step"].view[0, 0])
    a, b = (float(v) for v in _rd(i_["tab"].full.double(), i_["tab"].base + 2 * r + torch.arange(2)))
    for i in passes(n, 4096, defect):
        e = i if defect == "blend_x0_per_batch_item" else i % chw
        mk = _rd(i_["m"].full.double(), i_["m"].base + (e // hw if defect == "blend_mask_per_channel" else e % hw))
        x0 = _rd(i_["x0"].full.double(), i_["x0"].base + e)
        proper = x0 if b == 0 else a * x0 + b * _rd(i_["z"].full.double(), i_["z"].base + i)
        o.full[o.base + i] = ((1 - mk) * proper + mk * o.full[o.base + i]).float().double()
    return dict(x=o)


# ------------------------------------------------------------------------------------------------ mask prep
def build_mask(c, dtype):
    p = c.p
    mode, B, ch, h, w, ho, wo = p["mode"], p["B"], p["c"], p["h"], p["w"], p.get("ho", 0), p.get("wo", 0)
    g = GC._gen(22, mode, B, ch, h, w, ho, wo)
    b = None
    if mode == 0:
        a = torch.rand(B, ch, h, w, generator=g)
        a.view(-1)[:8] = torch.tensor([0.5, 0.49999997, 0.50000006, 0.0, 1.0, -0.0, 1e-40, 0.5])
        ref = (a >= 0.5).float()
    elif mode == 1:
        a = specials(torch.float32, B * ch * h * w, g).reshape(B, ch, h, w)
        b = (torch.rand(B, 1, h, w, generator=g) * 4).round() / 4     # 0, 0.25, 0.5, 0.75, 1: ties at the threshold
        ref = a * (b < 0.5)
    elif mode == 2:
        a = torch.rand(B, 1, h, w, generator=g)
        ref = F.interpolate(a, size=(ho, wo), mode="nearest")
    else:
        a = torch.randint(-4, 5, (B, ch, h, w), generator=g).float() / 4
        a[0, :, 0, 0] = torch.tensor([0.0, -0.0, 0.0])[:ch]
        ref = (a.double().sum(1, keepdim=True) < 0).float()
    return dict(inp=dict(a=flat_in(a), b=None if b is None else flat_in(b)), out=dict(out=window(1, ref.numel(), 0, torch.float32)),
                ref=dict(out=ref.reshape(1, -1)), gate={})


def walk_mask(c, t, dtype, defect=None):
    p = c.p
    mode, B, ch, h, w, ho, wo = p["mode"], p["B"], p["c"], p["h"], p["w"], p.get("ho", 0), p.get("wo", 0)
    a = t["inp"]["a"]
    af = a.full.double()
    o = _emu(t["out"]["out"])
    hw = h * w
    total = B * ho * wo if mode == 2 else B * hw if mode == 3 else B * ch * hw
    for i in passes(total, 4096, defect):
        if mode == 0:
            av = _rd(af, a.base + i)
            v = (av > 0.5 if defect == "mask_threshold_strict" else av >= 0.5).double()
        elif mode == 1:
            bi, pp = i // (ch * hw), i % hw
            if defect == "mask_broadcast_over_batch_dropped":
                bi = torch.zeros_like(bi)
            bb = t["inp"]["b"]
            av = _rd(af, a.base + i)
            v = torch.where(_rd(bb.full.double(), bb.base + bi * hw + pp) < 0.5, av, av * 0.0)
        elif mode == 2:
            x, y, bi = i % wo, (i // wo) % ho, i // (wo * ho)
            f32 = torch.float32
            sy = torch.floor(y.to(f32) * (torch.tensor(h, dtype=f32) / torch.tensor(ho, dtype=f32))).long().clamp(max=h - 1)
            sx = torch.floor(x.to(f32) * (torch.tensor(w, dtype=f32) / torch.tensor(wo, dtype=f32))).long().clamp(max=w - 1)
            v = _rd(af, a.base + bi * hw + (sy * h + sx if defect == "mask_nearest_h_w_swapped" else sy * w + sx))
        else:
            bi, pp = i // hw, i % hw
            s = torch.zeros(i.numel(), dtype=torch.float32)
            for j in range(ch):
                s = s + _rd(af, a.base + (bi * ch + j) * hw + pp).float()
            v = (s <= 0 if defect == "mask_sum_le_zero" else s < 0).double()
        o.full[o.base + i] = v
    return dict(out=o)


# ------------------------------------------------------------------------------------------------ fused conv_norm_out + conv_out
# pp_gn_conv3x3_smallcout against the two launches it replaces, BIT FOR BIT (GPU only: the 8 x 8 patch walk of csrc/norm.hip is
# not restated here).  The statistics are norm_cases' `constant` regime (every element of a population equal: the int64
# accumulators and the mean are exact, v = 0); beta in [1, 2) puts the normalised, SiLU'd, 16-bit activation into [0.5, 2), a
# multiple of 2^-12 in either format, whatever the scale / shift cancellation leaves; the weights are sparse +-1, +-2 with
# sum |w| <= 512 per output, the bias an integer: every partial sum is a multiple of 2^-12 below 2^12 and exact in fp32 in ANY
# order, so the patch kernel (MFMA per tap, then a 9-tap gather) and pp_conv3x3_smallcout (taps inside the MFMA chain, four
# partials) must agree to the bit.  The GPU test asserts the precondition on the activation the apply launch stored.
GN_CONV_CASES = [dict(B=2, H=H, W=W, cin=cin, groups=32) for (H, W) in ((13, 9), (8, 8), (1, 1), (9, 17)) for cin in (32, 64, 320, 384)]
GN_CONV_REFUSED = [dict(B=1, H=8, W=8, cin=416, groups=32, cout=4), dict(B=1, H=8, W=8, cin=24, groups=8, cout=4),
                   dict(B=1, H=8, W=8, cin=64, groups=32, cout=3), dict(B=1, H=8, W=8, cin=64, groups=0, cout=4),
                   dict(B=1, H=8, W=8, cin=64, groups=24, cout=4)]


def gn_conv_supported(cin: int, cout: int, groups: int) -> bool:
    return cout == 4 and cin > 0 and cin % 32 == 0 and cin <= 384 and 0 < groups <= 32 and cin % groups == 0


def build_gn_conv(p, dtype):
    B, H, W, cin, groups = p["B"], p["H"], p["W"], p["cin"], p["groups"]
    g = GC._gen(23, B, H, W, cin)
    x = NC.build_x("constant", dtype, B, H * W, cin, groups, key=23)
    K = 9 * cin
    w = _sparse_pm1(g, (4, K), min(0.5, 256.0 / K)) * _ints(g, (4, K), 1, 2)
    assert float(w.abs().sum(1).max()) <= 512
    return dict(x=flat_in(x), acc=NC.build_acc(x, None, groups), gamma=(torch.randn(cin, generator=g) * 0.3 + 1.0),
                beta=1.0 + torch.rand(cin, generator=g) * 0.999, w=flat_in(w.to(dtype)), w64=w, bias=flat_in(_ints(g, (4,), -4, 4).float()),
                out=window(B * 4 * H, W, 0, torch.float32))


# ------------------------------------------------------------------------------------------------ the matrix
BUILD = dict(conv_direct=build_conv_direct, conv_out=build_conv_out, to_nhwc=build_to_nhwc, to_nchw=build_to_nchw, add=build_add,
             skinny=build_skinny, temb=build_temb, softmax=build_softmax, splice=build_splice, step_head=build_step_head,
             zero=build_zero, step=build_step, blend=build_blend, mask=build_mask)
WALK = dict(conv_direct=walk_conv_direct, conv_out=walk_conv_out, to_nhwc=walk_to_nhwc, to_nchw=walk_to_nchw, add=walk_add,
            skinny=walk_skinny, temb=walk_temb, softmax=walk_softmax, splice=walk_splice, step_head=walk_step_head,
            zero=walk_zero, step=walk_step, blend=walk_blend, mask=walk_mask)
FORMATLESS = ("temb", "splice", "zero", "step", "blend", "mask")      # no 16-bit side: run once


def _cases():
    cs = []

    def add(kernel, probe, only=None, expect=0, **p):
        ident = f"{kernel}-{probe}-" + "-".join(f"{k}{v}" for k, v in p.items() if v is not None and v is not False)
        if all(k.id != ident for k in cs):               # (the explicit lists below may name a case the sweeps already hold)
            cs.append(Case(kernel, ident, probe, p, only, expect))
    # ---- pp_conv3x3_direct
    shapes = ((1, 1), (1, 7), (5, 1), (6, 11), (13, 9))
    for k, (H, W) in enumerate(shapes):
        for m, cin in enumerate((1, 3, 4, 5, 9, 16)):
            cout = (8, 24, 320)[(k + m) % 3]
            s = 1 + (k + m) % 2
            add("conv_direct", "E", B=2, H=H, W=W, cin=cin, cout=cout, stride=s, bias=(m % 2 == 0), add=(m % 3 != 0))
            if (k + m) % 2 == 0:
                add("conv_direct", "R", B=2, H=H, W=W, cin=cin, cout=cout, stride=s, bias=True, add=(m % 3 == 0), silu=(m % 3 != 2))
    for H, W in ((6, 11), (13, 9), (5, 1), (1, 7)):       # stride 2 on odd and even sizes, explicitly
        add("conv_direct", "E", B=2, H=H, W=W, cin=4, cout=8, stride=2, bias=True, add=True)
    add("conv_direct", "E", B=2, H=13, W=9, cin=9, cout=320, stride=1, bias=True, add=True)
    add("conv_direct", "R", B=2, H=13, W=9, cin=4, cout=320, stride=1, bias=True, add=True, silu=True)
    add("conv_direct", "E", B=1, H=91, W=91, cin=1, cout=1032, stride=1, bias=True, add=True)       # 1 068 249 work items
    # ---- pp_conv3x3_smallcout
    mf = ((3, 5, 7), (2, 1, 9), (2, 9, 1), (1, 3, 5), (1, 4, 4), (1, 1, 17), (1, 7, 9), (2, 4, 4), (1, 1, 1))  # npix % 32: 9, 18, 18, 15, 16, 17, 31, 0, 1
    for k, (B, H, W) in enumerate(mf):
        for m, cin in enumerate((32, 64, 320, 384)):
            if (k + m) % 2 == 0 or cin == 384 and k < 3:
                add("conv_out", "E", B=B, H=H, W=W, cin=cin, bias=(k + m) % 3 != 0)
    for cin in (32, 320, 384):
        add("conv_out", "R", B=3, H=5, W=7, cin=cin, bias=True)
    for cin, (B, H, W) in ((8, (1, 3, 3)), (24, (2, 3, 5)), (416, (1, 2, 3)), (24, (1, 1, 1))):
        add("conv_out", "E", B=B, H=H, W=W, cin=cin, bias=cin != 24)
        add("conv_out", "R", B=B, H=H, W=W, cin=cin, bias=True)
    # ---- layout
    for src in ("f32", "bf16", "fp16"):
        for ch, ldc, c0 in ((1, 2, 1), (4, 9, 0), (9, 16, 5), (4, 4, 0)):
            add("to_nhwc", "E", src=src, B=4, c=ch, hw=35, bmod=(2 if ch != 9 else 0), ldc=ldc, c0=c0)
    add("to_nhwc", "E", src="f32", B=2, c=1, hw=524300, bmod=0, ldc=2, c0=0)
    for dst in ("f32", "same"):
        for ch in (1, 4, 9):
            add("to_nchw", "E", B=3, c=ch, hw=35, dst=dst)
    add("to_nchw", "E", B=1, c=8, hw=131100, dst="same")
    for n in (8, 4096, 8 * (1048576 + 300)):
        add("add", "E", n=n)
    add("add", "X", expect=PP_ERR_BAD_ARG, n=12)
    # ---- pp_linear_skinny
    for rows in (1, 2, 4, 5, 8, 9, 16):
        add("skinny", "E", rows=rows, K=520, N=333, bias=rows % 2 == 1)
    for rows, K, N in ((1, 8, 1), (5, 8, 3), (16, 8, 3), (2, 1280, 3), (9, 1280, 1), (16, 1280, 333), (1, 8, 8197), (9, 8, 8197), (4, 1280, 333)):
        add("skinny", "E", rows=rows, K=K, N=N, bias=True)
    for rows, K, N, ai, ao in ((1, 520, 333, 1, 0), (2, 1280, 333, 0, 1), (5, 520, 3, 1, 1), (9, 520, 333, 1, 1), (16, 1280, 333, 1, 0),
                               (8, 8, 8197, 0, 1), (4, 520, 1, 0, 0)):
        add("skinny", "R", rows=rows, K=K, N=N, bias=True, act_in=ai, act_out=ao)
    add("skinny", "X", expect=PP_ERR_UNSUPPORTED, rows=16, K=2816, N=8)
    add("skinny", "X", expect=PP_ERR_BAD_ARG, rows=17, K=8, N=8)
    add("skinny", "X", expect=PP_ERR_BAD_ARG, rows=2, K=12, N=8)
    # ---- pp_timestep_embedding
    for tv in (0.0, 1.0, 500.5, 999.0):
        for rows, dim in ((1, 2), (3, 320), (3, 2), (1, 320)):
            add("temb", "E" if tv == 0 else "R", t=tv, rows=rows, dim=dim)
    # ---- pp_softmax_rows
    for n in (1, 3, 4, 5, 255, 257, 1023, 1030):
        lds, ldp = -(-n // 4) * 4 + (4 if n % 2 else 0), -(-n // 4) * 4 + (64 if n % 3 == 0 else 4 if n % 4 == 0 else 0)
        if n > 1:
            add("softmax", "R", rows=3, n=n, lds=lds, ldp=ldp, scale=1.0, regime="normal")
            add("softmax", "R", rows=3, n=n, lds=lds, ldp=ldp, scale=512 ** -0.5, regime="equal")
            add("softmax", "R", rows=3, n=n, lds=lds, ldp=ldp, scale=512 ** -0.5, regime="spike")
            add("softmax", "E", rows=3, n=n, lds=lds, ldp=ldp, scale=0.5, regime="largest")
        add("softmax", "E", rows=3, n=n, lds=lds, ldp=ldp, scale=512 ** -0.5, regime="onehot")
    for bad in (dict(lds=4, ldp=8), dict(lds=8, ldp=4), dict(lds=6, ldp=8), dict(lds=8, ldp=6), dict(lds=8, ldp=8, s_off=4),
                dict(lds=8, ldp=8, p_off=4)):
        add("softmax", "X", expect=PP_ERR_BAD_ARG, rows=2, n=5, scale=1.0, regime="normal", **bad)
    # ---- pp_embed_splice
    for nr in (1, 77, 300):
        for rb, t_off, o_off in ((1536, 0, 0), (1540, 0, 0), (1537, 0, 0), (1536, 4, 0), (1536, 0, 1), (1540, 0, 2)):
            for ne in (0, 5):
                if ne or (rb, t_off, o_off) == (1536, 0, 0):
                    add("splice", "E", n_rows=nr, row_bytes=rb, n_table=40, n_ext=ne, t_off=t_off, o_off=o_off)
    add("splice", "E", n_rows=1, row_bytes=113 * 1024, n_table=3, n_ext=0, t_off=0, o_off=0)
    # ---- step head, zero
    for scaled in (False, True):
        add("step_head", "E", B=2, c=4, hw=32900, bmod=1, ldc=8, c0=0, row_floats=20160, nz=65536 + 3, scaled=scaled)
        add("step_head", "E", B=4, c=4, hw=35, bmod=2, ldc=9, c0=4, row_floats=1280, nz=5, scaled=scaled)
    add("zero", "E", n=262144 + 5)
    add("zero", "E", n=3)
    # ---- step kernels
    for k in STEP_ROWS:
        for n in (1, 255, 257):
            for cfg in ((0,) if k == "noise" else (0, 1)):
                for ticket in ((False,) if k == "noise" else (False, True)):
                    add("step", "E", kind=k, n=n, cfg=cfg, ticket=ticket)
        for n, cfg, ticket in ((257, 1, True), (255, 0, False), (1048576 + 257, 1, True)):
            add("step", "R" if n < 1000 else "E", kind=k, n=n, cfg=cfg if k != "noise" else 0, ticket=ticket and k != "noise")
    # ---- latent blend, mask prep
    for hw in (1, 35, 87403):
        for r in range(3):
            add("blend", "E", B=3, C=4, hw=hw, row=r)
            if hw == 35:
                add("blend", "R", B=3, C=4, hw=hw, row=r)
    for mode, ch in ((0, 1), (1, 3), (3, 3), (1, 1), (3, 1)):
        add("mask", "E", mode=mode, B=2, c=ch, h=5, w=9)
    add("mask", "E", mode=0, B=2, c=1, h=1025, w=1024)
    add("mask", "E", mode=1, B=1, c=3, h=1025, w=1024)
    add("mask", "E", mode=2, B=2, c=1, h=1025, w=1024, ho=129, wo=128)
    for ho, wo in ((4, 7), (18, 11), (9, 5)):
        add("mask", "E", mode=2, B=2, c=1, h=9, w=5, ho=ho, wo=wo)
    return cs


CASES = _cases()


def case_dtypes(c: Case):
    if c.kernel in FORMATLESS:
        return [(torch.float32, "fp32")]
    return [(d, f) for d, f in DTYPES if c.only in (None, f)]


def refuses(c: Case) -> int:
    """the host checks, restated: the code a request is refused with before any launch (0: it runs)"""
    if c.kernel == "skinny":
        return refuses_skinny(c.p)
    if c.kernel == "softmax":
        return refuses_softmax(c.p)
    if c.kernel == "add":
        return PP_ERR_BAD_ARG if c.p["n"] <= 0 or c.p["n"] % 8 else 0
    return 0


def build(c: Case, dtype):
    return BUILD[c.kernel](c, dtype)


def walk(c: Case, t, dtype, defect=None):
    return WALK[c.kernel](c, t, dtype, defect)


def compare(c: Case, t, name: str, got: torch.Tensor):
    """the value check of one output window (`got` in its own format, [rows, cols]) -> (message or None, error / gate or None)"""
    ref = t["ref"][name]
    if name in t.get("cols", {}):                      # a channel window inside the row stride: the other columns are guards
        c0, n = t["cols"][name]
        got = got[:, c0:c0 + n]
    if name in t["gate"]:
        gt = t["gate"][name].to(got.device)
        r = worst_ratio(got, ref.to(got.device), gt)
        if not r <= 1.0:
            bad = ((got.double() - ref.to(got.device)).abs() > gt) | ~torch.isfinite(got.double())
            return f"{name}: error / gate {r:.3f}, first bad index {bad.nonzero()[0].tolist()}", r
        return None, r
    exp = ref.to(got.dtype).to(got.device) if ref.dtype != got.dtype else ref.to(got.device)
    ne = bits(got.contiguous()) != bits(exp.contiguous())
    if bool(ne.any()):
        i = ne.nonzero()[0]
        return (f"{name}: not bit-equal at {int(ne.sum())} elements, first bad index {i.tolist()}: got {got[tuple(i)].item()!r}, "
                f"expected {exp[tuple(i)].item()!r}"), None
    return None, None


def where(c: Case, name: str, idx) -> str:
    """the borders a failing element (row, column of its window) lies on"""
    p, tags = c.p, []
    r, col = int(idx[0]), int(idx[1])
    if c.kernel == "conv_direct":
        s = p["stride"]
        ho, wo = (p["H"] - 1) // s + 1, (p["W"] - 1) // s + 1
        y, x = (r // wo) % ho, r % wo
        if y in (0, ho - 1) or x in (0, wo - 1):
            tags.append("image edge")
        if r * (p["cout"] // 8) + col // 8 >= 4096 * 256:
            tags.append("second stride pass")
    elif c.kernel == "conv_out":
        H, W = p["H"], p["W"]
        y, pix = r % H, (r // (4 * H) * H + r % H) * W + col
        if y in (0, H - 1) or col in (0, W - 1):
            tags.append("image edge")
        if pix % 16 in (0, 15):
            tags.append("group edge")
        tags.append(f"workgroup {pix // 32}")
    elif c.kernel == "skinny":
        if col >= 2048 * 4:
            tags.append("second column pass")
        if r >= p["rows"] - 1:
            tags.append("last live row")
    elif c.kernel in ("step", "add", "blend", "zero") and name != "state":
        if col >= 4096 * 256 * (8 if c.kernel == "add" else 1) or c.kernel == "zero" and col >= 1024 * 256:
            tags.append("second stride pass")
    elif c.kernel == "softmax":
        n = p["n"]
        tags.append("pad column" if col >= n else "scalar tail" if col >= n // 4 * 4 else "vector body")
    return ", ".join(tags)


def failures(c: Case, t, dtype, defect=None):
    """the walk (faithful or defective) under the checks of the GPU test: values, guards, counters"""
    if c.probe == "X":
        return [] if refuses(c) == c.expect else [f"refusal: expected {c.expect}, the host check gives {refuses(c)}"]
    o = walk(c, t, dtype, defect)
    out = []
    for name, e in o.items():
        b = t["out"][name]
        if name in ("step", "ticket"):
            want = (STEP_FIRST + (t["launches"] if c.p["ticket"] else 0)) if name == "step" else 0
            if int(e.view[0, 0]) != want:
                out.append(f"{name}: {int(e.view[0, 0])}, expected {want}")
            continue
        if not bool(torch.isnan(e.full[e.outside()]).all()):
            out.append(f"{name}: bytes outside the window were written")
        win = e.view
        cols = t.get("cols", {}).get(name)
        if cols is not None:
            keep = torch.zeros(win.shape[1], dtype=torch.bool)
            keep[cols[0]:cols[0] + cols[1]] = True
            if not bool(torch.isnan(win[:, ~keep]).all()):
                out.append(f"{name}: pad columns were written")
        sel = win if cols is None else win[:, cols[0]:cols[0] + cols[1]]
        if bool(torch.isnan(sel).any()) and not bool(torch.isnan(t["ref"][name].double()).any()):
            out.append(f"{name}: elements of the window were never stored, first {torch.isnan(sel).nonzero()[0].tolist()}")
            continue
        msg, _ = compare(c, t, name, win.to(b.full.dtype))
        if msg:
            out.append(msg)
    return out
