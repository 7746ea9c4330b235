/*
 * pp_hip.h -- C ABI of libpp_hip.so: the MI355X (gfx950) kernels of the PowerPaint denoising hot path.
 *
 * The reference (open-mmlab/PowerPaint) has NO FFI / plugin / custom-op interface for this path: it reaches the
 * GPU only through torch/diffusers module calls.  Each entry point below therefore cites the
 * reference *call site / module* whose device work it replaces.  Conventions for every entry:
 *   - `extern "C"`, plain pointers + sizes, no torch types;
 *   - all pointers are DEVICE pointers unless named `host_*`;
 *   - activations are 16-bit (raw uint16 storage; bf16 or fp16, selected per call by the `dtype` argument / field --
 *     where a comment below says "bf16" read "the call's 16-bit format") in NHWC / [rows][channels] layout,
 *     parameters as documented;
 *   - the last argument is a `hipStream_t` (passed as void*; torch.cuda.current_stream().cuda_stream);
 *   - returns PP_OK (0) or a negative PP_ERR_*; never throws, never allocates, never synchronises, keeps no
 *     pointer after return, is re-entrant per stream; workspaces are caller-provided and sized by *_workspace_bytes.
 */
#ifndef PP_HIP_H_
#define PP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_ERR_BAD_ARG (-1)      /* shape / alignment / enum outside the supported set            */
#define PP_ERR_UNSUPPORTED (-2)  /* valid request the kernels do not implement (e.g. head_dim 24) */
#define PP_ERR_LAUNCH (-3)       /* hipLaunchKernel / hipFuncSetAttribute failed                  */
#define PP_ERR_WORKSPACE (-4)    /* workspace pointer null or too small                           */

#define PP_ABI_VERSION 29
/* 16-bit storage format of activations and matrix weights ("dtype" arguments; the same codes pp_nchw_to_nhwc uses for
 * its source): bf16 or fp16 -- the reference's default is fp16 (/root/reference/app.py:548,559).  MFMA accumulation,
 * norm statistics, softmax, biases and latents are fp32 with either. */
#define PP_DT_F32 0
#define PP_DT_BF16 1
#define PP_DT_F16 2
int pp_abi_version(void);
/* Digest (hex) of the sources, headers and extra flags this library was built from -- what a committed profile or bench
 * record names as "the build it was taken from" (stable across rebuilds and checkout paths). */
const char* pp_build_id(void);
/* hipGetLastError() text of the last PP_ERR_LAUNCH on this thread (host pointer, static storage). */
const char* pp_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM 3x3 convolution on bf16 MFMA tiles.
 *   out[m][n] = epilogue( sum_k X[m][k] * W[n][k] )
 * Replaces: every nn.Conv2d(3x3) / nn.Conv2d(1x1) / nn.Linear on the path --
 *   ResnetBlock2D.conv1/conv2/conv_shortcut, Downsample2D.conv, Upsample2D.conv (ctor sites
 *   /root/reference/powerpaint/models/unet_2d_blocks.py:1274-1285,1319-1321,2542), Transformer2DModel.proj_in/out,
 *   Attention.to_q/k/v/to_out, FeedForward GEGLU proj + out (unet_2d_blocks.py:1289-1300), BrushNet zero-convs
 *   (/root/reference/powerpaint/models/BrushNet_CA.py:842-845,861,899-902) incl. `* conditioning_scale` (:930-934),
 *   and the residual adds `hidden_states + *_add_samples.pop(0)` (unet_2d_blocks.py:1388-1398,2629-2638).
 *
 * X operand modes:
 *   PP_X_PLAIN   : X[m][k] row-major; k <  c1 read from x1 (row stride ldx1), k >= c1 from x2 (row stride ldx2)
 *                  -> channel-concat of two tensors without materialising it (up-block skip concat,
 *                  unet_2d_blocks.py:2589,2732).  K = c1 + c2.
 *   PP_X_CONV3X3 : X is the im2col view of an NHWC tensor [batch][hin][win][c1(+c2)]; pad 1; k = (ky*3+kx)*C + c;
 *                  `stride` 1|2 (Downsample2D: hout = (hin - 1) / stride + 1, odd hin included); `up`=1 fuses the nearest
 *                  upsample of the input (Upsample2D).  (ABI v29) With up = 1 and stride 1 the virtual input is
 *                  F.interpolate(x, size=(hout, wout), mode="nearest") for hout in {2 hin - 1, 2 hin} and wout in
 *                  {2 win - 1, 2 win}, the axes independent: virtual pixel (y, x) is source pixel (y >> 1, x >> 1) --
 *                  floor(i hin / (2 hin - 1)) = i >> 1 for every i <= 2 hin - 2 -- and the conv's zero padding begins at
 *                  hout x wout, not at 2 hin x 2 win (the upsamplers of a UNet whose latent is no multiple of
 *                  2^levels resize to the next skip tensor's size).  Any other hout / wout: PP_ERR_BAD_ARG.  The
 *                  tap-major kernels take every such request; the halo-tile loop (pp_conv_gn_supported) and the sub-pixel
 *                  form (pp_upconv_subpix_supported_to) take the exact 2x target only.
 *                  M = batch*hout*wout, K = 9*(c1+c2).  c1, c2 multiples of 64.
 * W operand: bf16 [N][K] row-major (conv weights pre-permuted to [Cout][ky][kx][Cin] by the host).
 * Epilogue:  v = (acc + bias[n] + rowvec[m / rows_per_batch][n]) * scale + res1[m][n] + res2[m][n]
 *            act = PP_ACT_GEGLU: columns come in interleaved groups of four (h0,h1,g0,g1); out[m][n/2+j] = h_j*gelu_erf(g_j)
 *            (weights/bias pre-interleaved by the host), out has N/2 columns.
 *            out_vt != NULL: columns >= vt_col0 are written TRANSPOSED per batch item to out_vt[b][n - vt_col0][row in batch]
 *            (V^T for attention), the others to `out`.
 * Aliasing:  res1 MAY be the same tensor as `out` (same pointer, ldres1 == ldo: `out += (acc + bias) * scale`, in place) on a
 *            launch with the plain 16-bit epilogue: act = PP_ACT_NONE, no out_f32 / out_vt / row_stats_out / ln_stats /
 *            gn_next_out, out_dup_rows == 0 and res1_wrap_rows == 0.  On every path such a launch can take -- the staged
 *            single-pass epilogue, the register-staged one, split-K with the separate combine launch (the GEMM kernel then
 *            touches only the fp32 slabs), split-K with the in-kernel share combine -- element [m][n] is read as res1 and
 *            then written as `out` by ONE thread, each exactly once, and no workgroup reads `out` as an operand, so no
 *            other thread can observe the element in between.  out_dup_rows stores rows a second thread's res1 read may
 *            cover and res1_wrap_rows reads rows another thread writes: not in place.  Any other overlap of res1 / res2 /
 *            x* / w with `out` (offset pointers, different row strides, res2 -- kept for the skip tensors, which never
 *            alias) is undefined.  Several ControlNets use it: the zero convs of every net but the first accumulate into the
 *            first net's residual buffers (MultiControlNetModel, /root/reference/powerpaint/pipelines/
 *            pipeline_PowerPaint_ControlNet.py:306,1686-1694 -- diffusers sums the nets' residuals in separate adds).
 */
#define PP_X_PLAIN 0
#define PP_X_CONV3X3 1
#define PP_ACT_NONE 0
#define PP_ACT_GEGLU 1
#define PP_ACT_SILU 2
/* (ABI v20) softmax over every group of 80 consecutive output columns, in the exp2 domain (the weights carry log2 e); a
 * -inf bias entry masks its column.  16-bit output [M][N], N % 80 == 0.  With the folded LayerNorm on the input side and
 * per-item weights (w_batch_stride / vec_batch_stride) this is the FIRST of the two GEMMs the cross-attention sub-block
 * becomes once K and V are folded into its projections (pp_xattn_fold): probabilities = softmax_h(LN2(h) G_h); the second,
 * plain GEMM multiplies them with H = V Wo^T.  No residuals / row vector / statistics / split-K on this launch. */
#define PP_ACT_SOFTMAX80 3
/* (added under ABI 29) exact-erf GELU, v = v Phi(v), applied where PP_ACT_SILU is: after the residuals, before the one
 * rounding of the store, on every path that honours PP_ACT_SILU (the staged and the register-staged epilogue, the full
 * split-K combine), under every tile form and split count.  PP_X_PLAIN requests without ln_stats / row_stats_out only
 * (PP_ERR_UNSUPPORTED otherwise: the staged kernel carries the GELU as instantiations of its own, so that the others keep
 * their register budgets, and the conv and folded-LayerNorm ones have none).  Phi through the Abramowitz-Stegun 7.1.26 erfc of the GEGLU epilogue (|erf error| <= 1.5e-7).  fc1 of
 * the CLIP vision tower (hidden_act = "gelu").  Any `act` outside 0 .. 4 is PP_ERR_BAD_ARG. */
#define PP_ACT_GELU 4

typedef struct PPGemmArgs {
  int32_t M, N, K;
  int32_t x_mode;
  const void* x1;
  const void* x2;
  int32_t c1, c2;
  int32_t ldx1, ldx2;
  int32_t batch, hin, win, hout, wout, stride, up;
  const void* w;
  const float* bias;
  const float* rowvec;
  int32_t ld_rowvec, rows_per_batch;
  const void* res1;
  int32_t ldres1;
  const void* res2;
  int32_t ldres2;
  float scale;
  int32_t act;
  void* out;
  int32_t ldo;
  int32_t out_f32;
  void* out_vt;
  int32_t vt_col0;
  int32_t vt_ld;      /* row stride of out_vt (>= rows_per_batch) */
  int32_t splitk;     /* 0 = auto */
  int32_t tile;       /* 0 = auto; else PP_TILE_* */
  float* workspace;   /* split-K partials, pp_gemm_workspace_bytes() */
  int32_t dbg;        /* 0.  (Phase-ablation switches of the measurement scripts under tools/: honoured by -DPP_LAB builds
                       * only, libpp_hip.so ignores the field.) */
  int32_t dtype;      /* PP_DT_BF16 | PP_DT_F16: format of x*, w, res*, out (unless out_f32), out_vt */
  /* (ABI v19) The two halves of a classifier-free-guidance batch are bit-identical from `torch.cat([latents] * 2)`
   * (/root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:990-996) down to the first cross-attention
   * (/root/reference/powerpaint/models/unet_2d_condition.py:1183-1236): the launches in front of it run on ONE half.
   *   out_dup_rows   > 0: every output row m is ALSO stored at row m + out_dup_rows of `out` (the tensor has 2 M rows; its
   *                  consumers behind the prefix -- the up-block skip concat -- see the full batch).  Single-pass 16-bit
   *                  epilogue only (no split-K, GEGLU, V^T, fp32 output, row moments): PP_ERR_UNSUPPORTED otherwise.
   *   res1_wrap_rows > 0: res1 has only res1_wrap_rows rows; output row m adds res1 row (m mod res1_wrap_rows)
   *                  (requires M <= 2 * res1_wrap_rows): the first full-batch launch reads the half-batch residual. */
  int32_t out_dup_rows;
  int32_t res1_wrap_rows;
  /* LayerNorm folded into the GEMM (BasicTransformerBlock.norm1/2/3 -> the Linear that follows):
   *   LN(x) W^T = rstd * (x (gamma.W)^T - mean * colsum) + beta W^T, so the host packs W' = gamma (.) W, passes
   *   ln_colsum[n] = sum_k W'[n][k] and adds beta W^T to the bias; mean / rstd come from per-row moments.
   * Producer side: row_stats_out != NULL makes the epilogue write, for every output row m and N-tile t (160 columns),
   *   (sum, sum of squares) of the stored bf16 values to row_stats_out[(m * tiles_n + t) * 2].
   * Consumer side: ln_stats != NULL (layout above, ln_tiles tiles per row, ln_dim = row length) switches the epilogue to
   *   v = rstd[m] * (acc - mean[m] * ln_colsum[n]) + bias[n] ... (then residuals / activation as usual). */
  float* row_stats_out;
  const float* ln_stats;
  const float* ln_colsum;
  int32_t ln_tiles;
  int32_t ln_dim;
  float ln_eps;
  /* (ABI v20; the slot of ABI v12-v14's experiment of the same name) > 0: PP_X_PLAIN only -- batch item b = m / rows_per_batch
   * multiplies with the [N][K] matrix at w + b * w_batch_stride elements (rows_per_batch % 64 == 0: 64-row tiles inside
   * one item).  The encoder hidden states are step-invariant, so pp_xattn_fold leaves one G^T / H^T per prompt. */
  int32_t w_batch_stride;
  /* GroupNorm statistics of the OUTPUT, accumulated by the epilogue (the stats launch of the consuming GroupNorm
   * disappears).  Up to two consumers per tensor (a UNet skip tensor feeds the next layer's norm and, concatenated,
   * an up-block norm):  gn_acc[k] -> int64 [batch][gn_groups[k]][2] = (sum, sum of squares) of the stored bf16 values
   * in fixed point (PP_GN_SUM_SCALE / PP_GN_SQ_SCALE), added with 64-bit integer atomics => order-independent,
   * bit-reproducible.  Column n of this GEMM is channel gn_c0[k] + n of the consumer's (possibly concatenated)
   * input, whose groups are gn_cg[k] channels wide.  Requires rows_per_batch % 64 == 0 (set rows_per_batch), a v2
   * tile, no GEGLU / V^T / fp32 output; pp_gemm_gn_stats_ok() tells.  The caller zeroes gn_acc before the launch. */
  int64_t* gn_acc[2];
  int32_t gn_cg[2];
  int32_t gn_c0[2];
  int32_t gn_groups[2];
  /* PP_X_CONV3X3 only: the contraction continues after the nine taps with c3 + c4 channels read at the OUTPUT pixel
   * (a 1x1 convolution of concat(x3, x4), NHWC bf16 at the output resolution) -- ResnetBlock2D.conv_shortcut(input)
   * summed into conv2:  K = 9 (c1 + c2) + c3 + c4, weight columns in that order.  Requires stride 1, no upsample,
   * c3 % 64 == 0, c4 % 64 == 0, a v2 tile. */
  const void* x3;
  const void* x4;
  int32_t c3;
  int32_t c4;
  /* PP_X_CONV3X3, stride 1, no upsample (ABI v14): `GroupNorm(gn_in_groups) -> SiLU` of the conv INPUT concat(x1, x2)
   * applied by the loader, i.e. ResnetBlock2D's `norm1 -> nonlinearity -> conv1` / `norm2 -> nonlinearity -> dropout
   * -> conv2` (diffusers 0.27 ResnetBlock2D.forward; ctor sites /root/reference/powerpaint/models/unet_2d_blocks.py:
   * 1274-1285) as ONE launch: the normalised activation is never written to memory.  x1 / x2 then hold the RAW
   * (un-normalised) tensors; gn_in_acc -> int64 [batch][gn_in_groups][2] = the (sum, sum of squares) accumulators of
   * concat(x1, x2) in the fixed-point format of gn_acc above, COMPLETE before this launch (written by the producers'
   * epilogues); gn_in_gb -> fp32 [c1 + c2][2] = (gamma, beta) interleaved per channel.  The optional 1x1 tail (x3, x4)
   * is NOT normalised.  Zero padding applies to the normalised tensor, as in the reference.  Supported shapes:
   * pp_conv_gn_supported(); the arithmetic of the normalisation is that of pp_groupnorm_apply_acc -- values rounded to
   * the 16-bit format before the convolution where the two-launch path stores them -- up to 1-ulp differences of the SiLU
   * (the loader evaluates it with v_exp / v_rcp: a few per cent of the normalised values differ from the apply launch's by
   * one unit of the 16-bit format; only the gn_next_* combine path below is bit-identical to the apply launch).  gn_in_*
   * on a PP_X_PLAIN launch is PP_ERR_UNSUPPORTED, gn_in_acc without gn_in_gb (or the reverse) PP_ERR_BAD_ARG. */
  const int64_t* gn_in_acc;
  const float* gn_in_gb;
  int32_t gn_in_groups;
  int32_t gn_in_silu;   /* must be 1 (every GroupNorm in front of a 3x3 conv of the path is followed by SiLU) */
  float gn_in_eps;
  /* (ABI v19) with out_dup_rows: the statistics subscriptions k whose bit is set in gn_dup_mask belong to a consumer of the
   * FULL (duplicated) tensor -- the epilogue adds every (batch item b, group) contribution to batch item b + gn_dup_batch of
   * gn_acc[k] as well.  A subscription without its bit is a consumer of the half batch (the next layer of the prefix). */
  int32_t gn_dup_batch;
  /* (ABI v17) The GroupNorm (+ SiLU) that CONSUMES this launch's output, applied by the split-K combine itself: where one
   * workgroup of the combine owns a whole (batch item, 160-column tile) -- rows_per_batch <= 256, i.e. the 16 x 16 and 8 x 8
   * levels -- and the consumer's groups lie whole inside the tile, the tile's fixed-point (sum, sum of squares) ARE the
   * groups' statistics, so the combine writes `out` (the raw tensor: residual / skip consumers) AND
   * gn_next_out = [SiLU](GroupNorm(out)) with the arithmetic of pp_groupnorm_apply_acc (bit-identical), and the separate
   * apply launch (6.5 .. 12 us each at those levels) disappears.  gn_next_sub = which of gn_acc[0 / 1] carries the
   * consumer's grouping (its accumulator is still updated).  Honoured only where pp_gemm_gn_next_ok() = 1; ignored
   * (never silently: the caller asks first) otherwise.  Reference: the norm1 / norm2 / Transformer2DModel.norm modules
   * behind a ResnetBlock2D conv, /root/reference/powerpaint/models/unet_2d_blocks.py:1274-1300. */
  void* gn_next_out;
  const float* gn_next_gamma;
  const float* gn_next_beta;
  float gn_next_eps;
  int32_t gn_next_silu;
  int32_t gn_next_sub;
  int32_t gn_dup_mask;   /* see gn_dup_batch */
  /* (ABI v20) with w_batch_stride and act = PP_ACT_SOFTMAX80: bias and ln_colsum advance by this many floats per batch item */
  int32_t vec_batch_stride;
  /* (ABI v21; v22: every split combines its own share) The split-K combine INSIDE the producing kernel.  tile_ctr != NULL
   * permits it: pp_gemm_combine_ctr_bytes() bytes of device memory (two 64-bit words per tile), ZERO before the first launch
   * that uses them, private to this launch within a step.  The words are monotonic arrival counts: a launch adds its split
   * count to bits 40.. of each and leaves bits 0..39 (the round's bookkeeping) zero; they may be re-zeroed between launches
   * (a step's accumulator-pool zeroing does) but never while one runs.  Where pp_gemm_bf16 finds the launch eligible -- lean
   * epilogue, an 8-wave ping-pong or halo-tile kernel, 2 / 4 / 8 splits of a tile of >= 16 x splits rows, tiles % 8 == 0 so
   * that the splits of a tile share an XCD (csrc/gemm_combine.h) -- the splits of a tile wait for each other at the tile's
   * counter (XCD-local atomics; BOUNDED: a split that gives up marks its share abandoned and the last arriver combines it)
   * and each sums ITS 1 / S of the tile's rows over the fp32 slabs, in slab order, and runs the combine's epilogue on them
   * (incl. gn_acc; gn_next_* behind a second arrival, the shares' integer sums exchanged through per-tile scratch that
   * pp_gemm_workspace_bytes() already counts behind the slabs): same bits as the separate combine launch, which then does
   * not happen.  Not eligible => the separate combine as before; tile_ctr is a permission, never a request that can fail.
   * combine_fault (optional): a device counter that stays non-zero if an abandoned share was never taken back (splits of a
   * tile on different XCDs count in different L2s and never reach S) or a second-arrival wait hit its bound: the caller
   * checks it at its synchronisation points and refuses the results (pp_* never synchronises).  Replaces the combine
   * behind the split-K convs / Linears of the 32x32 and 16x16 levels
   * (/root/reference/powerpaint/models/unet_2d_blocks.py:1457-1500, 850-899, 2696-2770). */
  uint64_t* tile_ctr;
  uint32_t* combine_fault;
  /* (ABI v28) PP_X_CONV3X3: 1 = the SUB-PIXEL form of Upsample2D's `nearest 2x -> conv3x3` (ctor site
   * /root/reference/powerpaint/models/unet_2d_blocks.py:2542).  Output pixel (2i + a, 2j + b) of that conv reads only the 2x2
   * source pixels (i + a - 1 + dy, j + b - 1 + dx), dy, dx in {0, 1}: the nine taps collapse onto four, with the weights of the
   * taps that share a source pixel summed (pp_upconv_fold).  The request describes the SOURCE geometry -- hin = hout, win =
   * wout, stride 1, up = 0, M = batch * hin * win, rows_per_batch = hin * win -- with `w` = the folded buffer of
   * pp_upconv_fold, [4 parities 2a + b][N][2][2][c1], and K = 4 * c1; `out`, res1 and res2 are [batch][2 hout][2 wout][N]
   * tensors (source row m of parity (a, b) is their row of pixel (2i + a, 2j + b)); gn_acc subscriptions describe that output
   * tensor (its batch items are the source's).  4/9 of the MACs of the `up` = 1 request; the folded weights are rounded to
   * the 16-bit format once more, so the result differs from the `up` = 1 request's by up to one rounding of an activation
   *  -- a request of its own, never a route the library takes for `up` = 1.  Runs on the halo-tile loop
   * only, one pass (splitk <= 1), one source tensor, no 1x1 tail, no gn_in_* / gn_next_* / out_dup_rows / res1_wrap_rows:
   * PP_ERR_UNSUPPORTED otherwise (pp_upconv_subpix_supported() tells).  0: every request of ABI v27 as before. */
  int32_t subpix;
  /* (added under ABI 29 as the LAST field; 0 = every request as before -- a caller built against an older header of this
   * version must be rebuilt: tests/test_abi.py compares the struct sizes)  The tile order of the launch.  The kernels give every XCD a contiguous range of tile ids; the ids walk groups of
   * `tile_group_m` M panels -- inside a group the M tile runs fastest, then the N tile, the last group may be shorter -- so the
   * workgroups resident on an XCD share tile_group_m activation panels and resident / tile_group_m weight strips in its L2.
   * 0 = automatic (the library models the fabric reads of the launch and picks the group height: DESIGN.md section 4);
   * > 0 forces that height, clamped to the M tiles of the form (1 = M-major, a large value = N-major); < 0: PP_ERR_BAD_ARG.
   * Like `tile` / `splitk` a tuning wish: the result is bit for bit the same in every order. */
  int32_t tile_group_m;
} PPGemmArgs;
#define PP_GN_SUM_SCALE 16777216.0f /* 2^24 */
#define PP_GN_SQ_SCALE 1048576.0f   /* 2^20 */
/* Accuracy envelope of the statistics behind ln_stats and gn_acc (and of the two-launch GroupNorm / LayerNorm).  Every
 * path but pp_layernorm forms the variance as E[x^2] - mean^2, which magnifies a relative error e of the sums by
 *     kappa = (mean^2 + var) / (var + eps)          (eps in the denominator on purpose: rstd is 1 / sqrt(var + eps), and a
 *                                                    constant population, var = 0, then has a finite kappa = mean^2 / eps)
 * into a relative error e kappa / 2 of rstd.  With eS / eQ the guaranteed relative error of the sum / the sum of squares
 * (u32 = 2^-24 per fp32 rounding of a running sum; derivation and the tests that hold the kernels to it:
 * tests/norm_cases.py), the statistics term stays below the rounding of the 16-bit output (u = 2^-8 bf16, 2^-11 fp16) for
 *     kappa <= 2 u / (eQ + 2 eS).
 * These are worst-case figures, linear in the number of roundings; a typical tensor errs like its square root and the
 * error beyond the envelope grows gradually (tests/test_norm_exact_gpu.py gates it there as well).
 *                                                 eS ~ eQ                              kappa (mean / std)   bf16         fp16
 *   pp_groupnorm_stats -> pp_groupnorm_apply      (L - 1 + Pe cg - 1) u32: 82 .. 126 u32 at the
 *     (fp32 chunk partials, fp64 fold)            UNet's shapes (L pixels per thread, Pe cg partials)       350 (18)     43 (6.5)
 *   gn_acc, filled by an epilogue                 R u32 for the column sums of a row block of R <= 256
 *     (int64 fixed point, fp64 fold)              rows, + half a quantum (2^-25 / 2^-21) per add:  R = 64   680 (26)     85 (9)
 *                                                                                                   R = 256  170 (13)     21 (4.6)
 *   gn_acc as a contract (exact sums rounded once to the quanta)                    limited by the format:  mean / std 64, 512
 *   row_stats_out -> ln_stats, fp32 one pass      (28 + tiles + 2) u32, tiles = C / 160:           C = 320  1300 (36)    165 (13)
 *     (gemm / xattn_fused / ff_fused consumers)   (+)                                              C = 1280 1100 (33)    140 (12)
 *   moments formed inside pp_tfront / the chained 84 u32 (80 roundings per lane, two shuffle adds, 1 / C and the product) (+)
 *     pp_xattn_block from the stored row                                                           C = 320  510 (23)     64 (8)
 *   ln_stats given exactly (rounded once to fp32) (tiles + 3) u32                                  C = 320  7700 (64*)   960 (31)
 *   (+) these rows follow from the same model but no `edge` case sits at them: the tests pin the producer (row moments
 *       against exact sums) and the consumers (moments given exactly, at their edge; pp_tfront at mean / std 16) separately.
 *   pp_layernorm (two passes)                     no magnification: the mean errs by (8 NP + 6) u32 |mean|, below u std up to
 *                                                 the format's limit (*: a standard deviation of two quanta is mean / std = 64
 *                                                 in bf16, 512 in fp16)
 * Inside the envelope the output is within u |y| + the fp32 terms of tests/norm_cases.py of the fp64 result.  var is
 * clamped at 0 everywhere, so rstd never exceeds 1 / sqrt(eps): a constant population yields beta. */

/* Order and rounding of the GEMM / conv epilogue -- the same on every path a request can take (the single-pass staged and
 * register-staged epilogues, the lean, full and statistics split-K combines, the in-kernel combine, the halo-tile kernel):
 *     acc = sum_k X[m][k] W[n][k]                                     fp32 (MFMA); split-K: fp32 slabs added in slab order
 *     v   = (acc [folded-LayerNorm correction] + bias[n] + rowvec[m / rows_per_batch][n]) * scale
 *     v   = v + res1[m or m - res1_wrap_rows][n] + res2[m][n]         (the residuals are NOT scaled)
 *     v   = act(v)                                                    PP_ACT_SILU | PP_ACT_GELU | the GEGLU product | the group softmax
 *     out = v rounded ONCE to the 16-bit format, to nearest even      (no rounding with out_f32)
 * every operation in fp32; nothing is rounded to 16 bits before the store (the row moments and GroupNorm accumulators are
 * formed from the values AS STORED).  With integer data whose partial sums stay below 2^24 the result is therefore exact
 * under any tile form, K order or split count, and a sum that lies halfway between two 16-bit values goes to the even one:
 * tests/test_gemm_exact_gpu.py holds every tile form to bit equality on such data, on sentinel-guarded outputs with row
 * strides ldo > N, and to |out - ref| <= u |ref| + (K + splits + 5) 2^-24 sum|terms| on random data (tests/gemm_cases.py).
 * Nothing outside rows [0, M) x columns [0, N) of `out` (ldo may exceed N; likewise out_vt / vt_ld), and nothing behind
 * pp_gemm_workspace_bytes() of the workspace, is written; pads of x* / res* / w may hold any finite values. */
#define PP_TILE_AUTO 0
#define PP_TILE_128x160 1
#define PP_TILE_64x160 2
#define PP_TILE_256x160 3

int pp_gemm_bf16(const PPGemmArgs* args, void* stream);   /* (historic name: bf16 or fp16 per args->dtype) */
/* bytes of PPGemmArgs.workspace this request needs: the fp32 slabs of a split-K launch + (ABI v22) behind them 6 KB per tile
 * of statistics scratch where the launch could combine in-kernel (tile_ctr); 0 = single pass */
size_t pp_gemm_workspace_bytes(const PPGemmArgs* args);
/* 1 if this launch (as pp_gemm_bf16 would configure it) can accumulate GroupNorm statistics (gn_acc), else 0 */
int pp_gemm_gn_stats_ok(const PPGemmArgs* args);
/* 1 if pp_gemm_bf16 runs this PP_X_CONV3X3 request with the GroupNorm + SiLU of its input fused into the loader
 * (gn_in_acc / gn_in_gb set), else 0 -- the caller then keeps pp_groupnorm_apply_acc + a plain conv.
 * 2 (round 6) for a PLAIN request (no gn_in_*) that pp_gemm_bf16 routes to the same halo-tile loop WITHOUT the
 * normalisation instead of the tap-major implicit GEMM: stride 1 (Upsample2D's nearest-2x conv included), tile = PP_TILE_AUTO, output images at least 16 wide
 * (every input pixel crosses the global -> LDS path once per tile instead of once per tap: 52 against 58 us at 64x64,
 * K = 2880; profiles/r06_conv_raw.txt).  Same request, same result contract; a routing fact for tests and planners. */
int pp_conv_gn_supported(const PPGemmArgs* args);
/* (ABI v16) 1 if the fused launch is supported AND, by the per-shape measurements on MI355X (profiles/
 * r04_conv_gn_variants.txt), at least as fast as pp_groupnorm_apply_acc + the plain conv it replaces; the engine asks this
 * one when it lays out a ResnetBlock2D.  The normalisation costs ~600 wave cycles per 8-pixel x 64-channel strip and is
 * repeated per 160-column tile and per halo row.  Round 6 (ABI v22): since plain convs run on the same loop WITHOUT the
 * normalisation (pp_conv_gn_supported() == 2) and the apply kernels' SiLU uses the hardware reciprocal, apply + plain conv
 * wins at every level (step -2.0 % same-box, profiles/r06_conv_raw.txt): this returns 0 for every shape of the SD-1.5 plans;
 * the fused launch remains an operator for a caller that sets gn_in_* . */
int pp_conv_gn_preferred(const PPGemmArgs* args);
/* (ABI v28) The sub-pixel form of an upsampling conv (PPGemmArgs.subpix), asked by SOURCE shape: 0 = pp_gemm_bf16 answers
 * such a request PP_ERR_UNSUPPORTED (source rows narrower than 8 pixels or not a multiple of 8, channels off the 64 grid,
 * no tile of whole source rows); 1 = it runs; 2 = it runs and is where the plans use it -- source images at least 16 wide,
 * the widths from which plain convs run on the halo-tile loop at all (below, the 9-tap request stays on the tap-major
 * weight stream at 16/9 fewer weight bytes). */
int pp_upconv_subpix_supported(int batch, int h, int w, int cin, int cout, int dtype);
/* (ABI v29) The same question for an upsampler that resizes the h x w source to hout x wout (PP_X_CONV3X3, up = 1): the
 * sub-pixel form writes whole 2x2 output quads, so a cropped target (2 h - 1 rows or 2 w - 1 columns) answers 0 and the
 * caller keeps the nine-tap `up` request; the exact target answers what pp_upconv_subpix_supported does. */
int pp_upconv_subpix_supported_to(int batch, int h, int w, int hout, int wout, int cin, int cout, int dtype);
/* (ABI v28) The folded weights of the sub-pixel form: w = the packed conv weight [cout][3][3][cin] (16-bit `dtype`) ->
 * out [4][cout][2][2][cin], out[2a + b][n][dy][dx][c] = sum over ky in R[a][dy], kx in R[b][dx] of w[n][ky][kx][c] with
 * R[0] = ({0}, {1, 2}), R[1] = ({0, 1}, {2}); summed in fp32 in the order ky outer, kx inner, rounded once (to nearest even).
 * cin % 8 == 0.  A cache derived from the weights: the plans run it outside the step, again whenever the weights change. */
int pp_upconv_fold(const void* w, int cout, int cin, int dtype, void* out, void* stream);
/* (ABI v17) 1 if this launch, as pp_gemm_bf16 would configure it, ends in the split-K combine that can apply the consumer
 * GroupNorm of subscription `sub` (PPGemmArgs.gn_next_*), else 0. */
int pp_gemm_gn_next_ok(const PPGemmArgs* args, int sub);
/* (ABI v21 / v22) Bytes of PPGemmArgs.tile_ctr the library ADVISES for this launch (16 per tile): 0 = the launch does not run
 * split-K, can never combine in-kernel (tile form, tiles % 8 != 0, epilogue not lean, placement check failed), or is one where
 * the separate combine launch measured faster on MI355X.  Measured inside the headline step's hipGraph (profiles/
 * r06_fused_combine.txt): launches of 2 and 4 splits whose workgroups are all resident at once (tiles x splits <= CUs) are a
 * draw to 8 us better per launch and a draw on the step with 18 kernels fewer -- advised; 8 splits (shares of 16 / 32 rows at
 * the 8x8 level and the 32 -> 16 downsample: the tail is a chain of ~1 us memory round trips against one 11 us kernel) lose
 * 2 .. 3 us per launch, 0.4 % on the step -- not advised.  (The first form, ONE workgroup combining the whole tile, lost
 * everywhere: +3 %.)  A caller that sets tile_ctr anyway (16 bytes per 128-row x 160-column tile always suffice) gets the
 * in-kernel combine wherever it is correct, bit for bit the separate one.  Asked at plan-build time, never inside a stream
 * capture: the first call per process may run pp_xcd_placement_ok(). */
size_t pp_gemm_combine_ctr_bytes(const PPGemmArgs* args);
/* (ABI v21) 1 if pp_gemm_bf16 will combine this launch in-kernel (tile_ctr set and every condition met, incl. the
 * gn_next_* apply where requested), else 0: how many kernels the launch is. */
int pp_gemm_combine_fused(const PPGemmArgs* args);
/* (added under ABI 29) The tile order pp_gemm_bf16 runs this request in: the group height (see PPGemmArgs.tile_group_m) of the form the
 * request resolves to, >= 1; 0 if the request does not run.  Pure host logic. */
int pp_gemm_tile_group_m(const PPGemmArgs* args);
/* (ABI v21) Launches a probe grid on the current device and SYNCHRONISES it (the one entry point that does): 1 if the
 * workgroups of dim3(tiles, splits) grids are placed on the XCDs round-robin by their linear id (what the in-kernel
 * combine's co-location rests on), else 0.  Cached per device. */
int pp_xcd_placement_ok(void);

/* Small-M ("skinny") linear in fp32 accumulate: out[b][n] = act_in(x[b][:]) . W[n][:] + bias[n], b < rows <= 16.
 * Replaces TimestepEmbedding.linear_1/linear_2 and the 22 ResnetBlock2D.time_emb_proj (batched into one call by
 * concatenating their weights along N) -- [diffusers-0.27.0]; reference call site unet_2d_condition.py:1155-1156.
 * x fp32 [rows][K]; W bf16 [N][K]; bias fp32; out fp32 [rows][ldo]. act_in: 0 none, 2 silu. act_out likewise. */
int pp_linear_skinny(const float* x, int rows, int K, const void* w, const float* bias, int N, float* out, int ldo,
                     int act_in, int act_out, int dtype, void* stream);

/* Sinusoidal timestep embedding (Timesteps(dim, flip_sin_to_cos=True, freq_shift=0)), unet_2d_condition.py:914-938.
 * out fp32 [rows][dim] = [cos(t f_k), sin(t f_k)], t read from device pointer (one value broadcast to all rows). */
int pp_timestep_embedding(const float* t_dev, int rows, int dim, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU) on NHWC bf16, two launches: statistics, then apply.
 * Replaces ResnetBlock2D.norm1/norm2 + nonlinearity, Transformer2DModel.norm, conv_norm_out + conv_act
 * (unet_2d_condition.py:1351-1353) -- nn.GroupNorm(32, C, eps).
 *   stats : x = concat(x1[c1], x2[c2]) per pixel; per-chunk partial (sum, sum of squares) per group -> workspace
 *           (pp_groupnorm_workspace_bytes()).
 *   apply : folds the partials (fp64, fixed order), then y[b][p][c] = act((x - mean) * rstd * gamma + beta) as bf16,
 *           y row stride = c1 + c2.  `workspace` is the buffer the stats call wrote (same batch / hw / channels).
 */
size_t pp_groupnorm_workspace_bytes(int batch, int hw, int C);
int pp_groupnorm_stats(const void* x1, int c1, const void* x2, int c2, int batch, int hw, int groups,
                       float* workspace, int dtype, void* stream);
int pp_groupnorm_apply(const void* x1, int c1, const void* x2, int c2, int batch, int hw, int groups, float eps,
                       const float* gamma, const float* beta, const float* workspace, int silu, void* y,
                       int dtype, void* stream);

/* GroupNorm apply from accumulated statistics: acc = int64 [batch][groups][2] filled by the producers' epilogues
 * (PPGemmArgs.gn_acc); otherwise identical to pp_groupnorm_apply. */
int pp_groupnorm_apply_acc(const void* x1, int c1, const void* x2, int c2, int batch, int hw, int groups, float eps,
                           const float* gamma, const float* beta, const int64_t* acc, int silu, void* y, int dtype,
                           void* stream);
/* dst[0..n) = 0 (64-bit words): one launch zeroes the statistics accumulators of a whole forward pass */
int pp_zero_u64(void* dst, long long n, void* stream);

/* LayerNorm over the last dim, bf16 [rows][C] -> bf16 [rows][C]; BasicTransformerBlock.norm1/2/3 (eps 1e-5). */
int pp_layernorm(const void* x, int rows, int C, const float* gamma, const float* beta, float eps, void* y,
                 int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused attention forward  O = softmax(Q K^T * scale) V, non-causal, no mask (AttnProcessor2_0 /
 * F.scaled_dot_product_attention) -- [diffusers-0.27.0] Attention used by Transformer2DModel.
 *   q  : bf16, element (b, i, h, j) at q[(b*nq + i)*ldq + h*d + j]
 *   k  : bf16, element (b, t, h, j) at k[(b*nk + t)*ldk + h*d + j]
 *   vt : bf16 V TRANSPOSED, element (b, t, h, j) at vt[((b*heads + h)*d + j)*ldvt + t]   (ldvt >= nk, mult of 8)
 *   o  : bf16, same indexing as q with ldo.
 * head_dim d in {40, 80, 160}; nk arbitrary (keys >= nk masked).
 * Padding: columns [nk, ldvt) of vt, and whatever follows the last row of K (item batch-1, key nk-1) in its buffer, may
 * hold any FINITE values -- a kernel may load them but they never reach the result; non-finite padding is not supported
 * (a masked probability is an exact 0, and 0 * NaN is NaN).  Nothing outside rows [0, batch*nq) x columns [0, heads*d)
 * of o is written.  (tests/test_attention_exact_gpu.py runs every kernel on poisoned pads and a sentinel-filled o.)
 */
int pp_attention_fwd(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo,
                     int batch, int heads, int nq, int nk, int d, float scale, int dtype, void* stream);
/* The same op with the kernel named explicitly (since ABI v8; op-level parity tests address every shipping kernel,
 * the pipelines use PP_ATTN_AUTO = what pp_attention_fwd picks):
 *   PP_ATTN_PHASED   attn_fwd_kernel   (three-phase, every head dim / key count)
 *   PP_ATTN_PIPE_Q32 attn_pipe_kernel  (software-pipelined, 32 queries per wave, 64-key tiles; d = 40, nk % 64 == 0, nk >= 256)
 *   PP_ATTN_PIPE_Q64 attn_pipe_kernel  (64 queries per wave on 32-key tiles; same shapes; AUTO takes it when
 *                                       batch * heads * ceil(nq / 256) >= 512, i.e. the 64x64 and 128x128 latents)
 *   PP_ATTN_PIPE_LOG2 (ABI v20) the pipelined kernel AUTO would take, for a q that already holds Q * scale * log2(e) (the
 *                                       producing GEMM's epilogue multiplies: pp_tfront q_scale): the running softmax
 *                                       reference enters as the initial accumulator of the QK^T MFMAs, a score leaves the
 *                                       matrix pipe as the exp2 argument (no VALU multiply-add per score); `scale` is NOT
 *                                       applied.  Shapes: pp_attention_log2_ok(); never chosen by AUTO.
 * A named kernel that does not cover the shape returns PP_ERR_UNSUPPORTED. */
#define PP_ATTN_AUTO 0
#define PP_ATTN_PHASED 1
#define PP_ATTN_PIPE_Q32 2
#define PP_ATTN_PIPE_Q64 3
#define PP_ATTN_PIPE_LOG2 4
int pp_attention_log2_ok(int nq, int nk, int d);
int pp_attention_fwd_variant(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo,
                             int batch, int heads, int nq, int nk, int d, float scale, int dtype, int variant,
                             void* stream);
/* Tiled self-attention (HyperTile; entries added under ABI v29): the tokens of a batch item are an h x w grid in row-major
 * order, cut into nh x nw tiles of th x tw = (h / nh) x (w / nw) tokens, and a query attends only to the keys of its own
 * tile -- block-diagonal attention, one launch of the tiled form of attn_pipe_kernel.  Token r of tile (ty, tx) is row
 * (ty*th + r / tw) * w + tx*tw + r % tw of its batch item.  Layouts exactly as pp_attention_fwd with nq = nk = h*w and
 * ldvt >= h*w; `variant` takes the PP_ATTN_* codes: AUTO picks by the occupancy rule of pp_attention_fwd_variant computed on
 * the tiled grid (batch * heads * nh * nw * ceil(th*tw / 256) >= 512 -> 64 queries per wave), PP_ATTN_PIPE_LOG2 expects the
 * pre-multiplied q as above, PP_ATTN_PHASED has no tiled form (PP_ERR_UNSUPPORTED).
 * pp_attention_tiled_ok(h, w, nh, nw, d) == 1 exactly where h % nh == 0, w % nw == 0, nh * nw > 1, the pipelined kernel
 * takes (nq, nk, d) = (th*tw, th*tw, d) (pp_attention_log2_ok), and nw == 1 or tw % 32 == 0 (a 32-key half of an LDS tile
 * then lies inside one run of tw contiguous rows); everywhere else pp_attention_fwd_tiled returns PP_ERR_UNSUPPORTED.
 * Padding as pp_attention_fwd: columns [h*w, ldvt) of vt may hold any finite values.  Keys outside a query's tile are never
 * loaded (so they may hold anything at all), nothing outside rows [0, batch*h*w) x columns [0, heads*d) of o is written, and
 * every element inside is.  A bad argument (null or misaligned pointer strides, h % nh != 0, w % nw != 0, ldvt < h*w, an
 * unknown variant or dtype) returns PP_ERR_BAD_ARG without a launch. */
int pp_attention_tiled_ok(int h, int w, int nh, int nw, int d);
int pp_attention_fwd_tiled(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo,
                           int batch, int heads, int h, int w, int nh, int nw, int d, float scale, int variant,
                           int dtype, void* stream);
/* [rows = b*nk + t][cols] bf16 (row stride ld) -> vt[b][col][t] (row stride ldvt).  Used for the cross-attention V
 * (computed once per call: encoder_hidden_states are step-invariant) and as the unfused fallback for self-attention. */
int pp_transpose_v(const void* v, int ld, int batch, int nk, int cols, void* vt, int ldvt, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Direct 3x3 convolutions (pad 1) for MFMA-unfriendly channel counts:
 *   pp_conv3x3_direct    : cout % 8 == 0, any cin, stride 1|2 -- conv_in (Cin 4/9 -> 320; BrushNet conv_in_condition,
 *                          /root/reference/powerpaint/models/BrushNet_CA.py:223-228,822-823) and the
 *                          ControlNetConditioningEmbedding convs (3->16->...->320, SiLU between).
 *                          x: bf16 NHWC [batch][hin][win][cin]; w: bf16 [3][3][cin][cout] (cout contiguous);
 *                          bias fp32; add: optional bf16 NHWC tensor added before the optional SiLU; out: bf16 NHWC.
 *   pp_conv3x3_smallcout : cout == 4, cin % 8 == 0, stride 1 -- conv_out (unet_2d_condition.py:1354).
 *                          x: bf16 NHWC; w: bf16 [cout][3][3][cin]; out: fp32 NCHW [batch][cout][h][w] (the UNet
 *                          boundary layout, consumed directly by pp_cfg_sched_step).
 */
int pp_conv3x3_direct(const void* x, int batch, int hin, int win, int cin, const void* w, const float* bias,
                      int cout, int stride, int silu_out, const void* add, void* out, int dtype, void* stream);
int pp_conv3x3_smallcout(const void* x, int batch, int h, int w_, int cin, const void* w, const float* bias, int cout,
                         float* out_nchw, int dtype, void* stream);
/* conv_norm_out + SiLU + conv_out in one launch (unet_2d_condition.py:1351-1354): GroupNorm statistics from the
 * producers' accumulators (`acc`, as pp_groupnorm_apply_acc), the normalised activation rounded to the 16-bit format
 * where the two-launch path stores it, 3x3 / pad 1 conv to `cout` = 4 channels, fp32 NCHW out.  x NHWC [batch][h][w][cin];
 * w [4][9][cin] (pp_conv3x3_smallcout's layout).  pp_gn_conv3x3_smallcout_supported(): cout == 4, cin % 32 == 0, cin <= 384. */
int pp_gn_conv3x3_smallcout_supported(int cin, int cout, int groups);
int pp_gn_conv3x3_smallcout(const void* x, int batch, int h, int w, int cin, int groups, float eps, const float* gamma,
                            const float* beta, const int64_t* acc, const void* wgt, const float* bias, int cout,
                            float* out_nchw, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Layout / assembly kernels at the module boundary (NCHW torch tensors <-> internal NHWC bf16).
 * pp_nchw_to_nhwc : src fp32|bf16|f16 NCHW [batch][c][hw] -> dst bf16 [batch][hw][ldc] at channel offset c0.
 *                   src_batch_mod > 0 reads batch item (b % src_batch_mod)  -> `torch.cat([latents]*2)`
 *                   (pipeline_PowerPaint.py:990) without a copy.
 * pp_nhwc_to_nchw : 16-bit [batch][hw][c] -> fp32 | the same 16-bit format, NCHW.
 * dtype codes: PP_DT_F32 0, PP_DT_BF16 1, PP_DT_F16 2; the trailing `dtype` is the format of the NHWC side.
 */
int pp_nchw_to_nhwc(const void* src, int src_dtype, int batch, int c, int hw, int src_batch_mod, void* dst, int ldc,
                    int c0, int dtype, void* stream);
int pp_nhwc_to_nchw(const void* src, int batch, int c, int hw, void* dst, int dst_dtype, int dtype, void* stream);
/* (added under ABI 29) The front of the CLIP vision tower (transformers CLIPVisionEmbeddings + pre_layrnorm; the
 * `image_encoder` of an IP-Adapter pipeline), two launches around the patch GEMM.
 * pp_vit_patchify : src fp32|bf16|f16 NCHW [batch][3][h][w] (src_dtype: PP_DT_*) -> dst 16-bit [batch*gh*gw][cols] with row
 *                   stride ldo >= cols, the im2col rows of a stride-`patch` convolution: gh = h / patch, gw = w / patch
 *                   (remainder pixels dropped, as the conv drops them); row (b*gh + gy)*gw + gx, column
 *                   c*patch*patch + ky*patch + kx holds pixel (b, c, gy*patch + ky, gx*patch + kx) -- the flattened order of
 *                   patch_embedding.weight [N][3][P][P], so the patch embedding is pp_gemm_bf16 against that weight
 *                   zero-padded along K to cols.  Columns [3*patch*patch, cols) of every row are WRITTEN as zeros (cols and
 *                   ldo multiples of 8, dst 16-byte aligned; the GEMM wants K = cols % 64 == 0: 588 -> 640 for patch 14).  A
 *                   copy with one rounding to the 16-bit format: bit-exact on representable values.  Nothing outside rows
 *                   [0, batch*gh*gw) x columns [0, cols) of dst is written.
 * pp_vit_embed_ln : y[b*(np+1) + t][C] = LayerNorm(e) * gamma + beta with e = class_embedding + pos[0] for t = 0 and
 *                   patches[(b*np + t - 1)*ldp ..] + pos[t] for t >= 1; patches (row stride ldp >= C, ldp % 8 == 0),
 *                   class_embedding [C] and pos [np+1][C] are 16-bit, gamma / beta fp32.  The sum is formed in fp32 from the
 *                   stored operands and is NOT rounded before the norm; the norm is pp_layernorm's (two passes, same
 *                   arithmetic); one rounding at the store.  C % 8 == 0, C <= 2048 (PP_ERR_UNSUPPORTED above), any np >= 1,
 *                   any batch; every pointer 16-byte aligned.  Nothing outside the batch*(np+1) rows x C columns of y is written.  This is hidden state 0
 *                   of transformers' encoder (after pre_layrnorm). */
int pp_vit_patchify(const void* src, int src_dtype, int batch, int h, int w, int patch, void* dst, int cols, int ldo,
                    int dtype, void* stream);
int pp_vit_embed_ln(const void* patches, int ldp, const void* class_embedding, const void* pos, int batch, int np, int C,
                    const float* gamma, const float* beta, float eps, void* y, int dtype, void* stream);
/* out = a + b on bf16 tensors of n elements (n % 8 == 0).  The residual adds that cannot ride a GEMM epilogue:
 * ControlNet `down_block_res_sample + down_block_additional_residual` on the already-consumed skip tensors
 * (/root/reference/powerpaint/models/unet_2d_condition.py:1263-1272,1296-1297). */
int pp_add_bf16(const void* a, const void* b, void* out, long long n, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused classifier-free guidance + scheduler step on fp32 NCHW latents.
 * Replaces pipeline_PowerPaint.py:1018-1023 / pipeline_PowerPaint_Brushnet_CA.py:1444-1449:
 *     eps = eps_u + g * (eps_c - eps_u);  latents = scheduler.step(eps, t, latents)
 * eps2 : fp32 [2*n] (uncond half first, pipeline_PowerPaint.py:516) when cfg != 0, else [n].
 * Per-step coefficients are read from a DEVICE table coef[step][8] = {c0 .. c5, _, _} and a device step counter:
 *     x0   = (x - c0 * eps) / c1                  (c0 = sqrt(1 - a_t), c1 = sqrt(a_t): the data prediction)
 *     kind 0 (DDIM): x_next = c2 * x0 + c3 * eps   (c2 = sqrt(a_prev), c3 = sqrt(1 - a_prev - std_dev_t^2); c4 = std_dev_t is
 *             read by pp_ddim_variance_noise only)
 *     kind 1 (DPM-Solver++ 2M): d1 = c5 * (x0 - m_prev);  x_next = c2 * x - c3 * x0 - c4 * d1;  m_prev <- x0
 *             (c2 = sigma_next / sigma_t, c3 = alpha_next (exp(-h) - 1), c4 = c3 / 2 or 0 on first-order steps, c5 = 1 / r0)
 *     kind 2 (PNDM / PLMS, PNDMScheduler(skip_prk_steps=True) -- the scheduler the SD-1.5 checkpoint config names):
 *             table rows are 16 floats {w0..w3, a, b, slot(h1), slot(h2), slot(h3), push_slot | -1, use_saved, save};
 *             m = w0 eps + w1 h1 + w2 h2 + w3 h3;  x_next = a * (use_saved ? saved : x) + b * m;  `m_prev` is the state
 *             [5][n] fp32 (4 history slots + the saved sample), zero before the first step.  N steps = N + 1 rows.
 *     kind 3 (UniPC, predict_x0 / bh1|bh2 / order <= 3 -- what app.py:197 installs on the ppt-v2 pipeline):
 *             rows are 16 floats {sigma_t, alpha_t, use_corr, k_last, k_m1, k_m2, k_m3, k_x0, p_xc, p_x0, p_m1, p_m2};
 *             x0 = (x - sigma_t eps) / alpha_t;  xc = use_corr ? k . (last, m1, m2, m3, x0) : x;
 *             x_next = p . (xc, x0, m1, m2);  state [4][n] fp32 <- (xc, x0, m1, m2), zero before the first step.
 * `step_dev` (int32 on device) selects the row.  advance_ticket == NULL: it is NOT incremented here (pp_step_advance
 * does).  advance_ticket != NULL (ABI v20; a zero-initialised device word that belongs to this call site): this launch is
 * the step's last reader of the counter and moves it on itself -- the block that finishes last does step_dev[0] += 1
 * and returns the ticket to zero; no pp_step_advance launch behind it.
 */
int pp_cfg_sched_step(const float* eps2, int cfg, float guidance, float* latents, float* m_prev, int n, int kind,
                      const float* coef_table, int32_t* step_dev, uint32_t* advance_ticket, void* stream);
/* Stochastic DDIM, `eta > 0` (the pipelines' `eta` argument, pipeline_PowerPaint.py:736-745 / 1023: it reaches
 * `DDIMScheduler.step` only): after pp_cfg_sched_step of the same step,  latents += std_dev_t * noise  with
 * std_dev_t = coef[step][4] of the kind-0 table (eta * sqrt((1-a_prev)/(1-a_t) * (1-a_t/a_prev)); column 3 then holds
 * sqrt(1-a_prev-std_dev_t^2)) and `noise` fp32 [n] drawn by the host from the caller's generator, once per step. */
int pp_ddim_variance_noise(float* latents, const float* noise, int n, const float* coef_table, const int32_t* step_dev,
                           void* stream);
/* (ABI v25) Fused classifier-free guidance + LCMScheduler.step (diffusers 0.27 `LCMScheduler`, few-step latent
 * consistency sampling) on fp32 NCHW latents; replaces the guidance combine and `self.scheduler.step(...)` of
 * pipeline_PowerPaint_Brushnet_CA.py:1449 (and the same line of the other two loops) when the scheduler is an LCMScheduler.
 * Table row coef[step][8] = {sqrt(1-a_t), sqrt(a_t), c_out, c_skip, sqrt(a_prev), sqrt(1-a_prev), 0, 0}:
 *     x0  = (x - sqrt(1-a_t) eps) / sqrt(a_t)
 *     den = c_out x0 + c_skip x                       (boundary condition, s = t * timestep_scaling:
 *                                                      c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25))
 *     x'  = sqrt(a_prev) den + sqrt(1-a_prev) noise   (every row but the last of the full schedule)
 *     x'  = den                                       (last row: columns 4, 5 = (1, 0); `noise` is NOT read there)
 * eps2 / cfg / guidance / step_dev / advance_ticket as pp_cfg_sched_step; `noise` fp32 [n], drawn by the host from the
 * caller's generator before every step but the last.  n need not be a multiple of 4. */
int pp_cfg_lcm_step(const float* eps2, int cfg, float guidance, float* latents, const float* noise, int n,
                    const float* coef_table, int32_t* step_dev, uint32_t* advance_ticket, void* stream);
/* (ABI v26) Fused classifier-free guidance + the step of a sigma-space sampler (EulerDiscreteScheduler at s_churn = 0,
 * EulerAncestralDiscreteScheduler; Karras et al., arXiv:2206.00364, k-diffusion sample_euler / sample_euler_ancestral) on
 * fp32 NCHW latents held in sigma space (x = x0 + sigma eps).  Table row coef[step][8] = {sigma, dt, s_up, 0, 0, 0, 0, 0}:
 *     e  = cfg ? eps_u + guidance (eps_c - eps_u) : eps        (the derivative (x - x0) / sigma of epsilon prediction)
 *     x' = x + dt e                                            (Euler: dt = sigma_next - sigma;  ancestral: s_down - sigma)
 *     x' = x' + s_up noise                                     (rows with s_up != 0 only; `noise` is NOT read otherwise)
 * eps2 / cfg / guidance / step_dev / advance_ticket as pp_cfg_sched_step; `noise` fp32 [n] drawn by the host.  n need not
 * be a multiple of 4. */
int pp_cfg_sigma_step(const float* eps2, int cfg, float guidance, float* latents, const float* noise, int n,
                      const float* coef_table, int32_t* step_dev, uint32_t* advance_ticket, void* stream);
/* (ABI v27) Fused classifier-free guidance + one table row of a sigma-space sampler that keeps state between network
 * evaluations (HeunDiscreteScheduler, KDPM2DiscreteScheduler, KDPM2AncestralDiscreteScheduler, LMSDiscreteScheduler;
 * Karras et al., arXiv:2206.00364, k-diffusion sample_heun / sample_dpm_2 / sample_dpm_2_ancestral / sample_lms at
 * s_churn = 0) on fp32 NCHW latents held in sigma space.  Table row coef[step][16] =
 *     {c_e, c_h1, c_h2, c_h3, s_up, sigma_eval, slot1, slot2, slot3, push_slot, use_saved, save, 0, 0, 0, 0}
 * (slots and flags stored as floats; sigma_eval, the noise level of the row's evaluation, is host bookkeeping):
 *     e   = cfg ? eps_u + guidance (eps_c - eps_u) : eps       (the derivative (x - x0) / sigma of epsilon prediction)
 *     x'  = (use_saved ? saved : x) + c_e e + c_h1 H[slot1] + c_h2 H[slot2] + c_h3 H[slot3]
 *     x'  = x' + s_up noise                                    (rows with s_up != 0 only; `noise` is NOT read otherwise)
 *     if (save)           saved        = x                     (the value BEFORE this row's update)
 *     if (push_slot >= 0) H[push_slot] = e                     (after the reads: a row may push into a slot it read)
 * `state` fp32 [4][n] = H[0], H[1], H[2], saved; zero before the first row.  Every element touches only its own index of
 * latents / state / noise.  Rows per sampler (sigma_k the base grid, sigma_N = 0):
 *     Heun   A_k: save, push 0, c_e = sigma_{k+1} - sigma_k;  B_k: use_saved, c_e = c_h1 = (sigma_{k+1} - sigma_k) / 2 over
 *            slot 0;  last row: Euler to 0.  2N - 1 rows, no noise drawn.
 *     DPM2   A_k: save, c_e = sigma_mid - sigma_k;  B_k (evaluated at sigma_mid): use_saved, c_e = sigma_{k+1} - sigma_k.
 *     DPM2 a as DPM2 towards sigma_down of the ancestral split; B_k: c_e = sigma_down - sigma_k, s_up = sigma_up.  The host
 *            draws one noise tensor per row, A rows included (used by the B rows only), as the library's step() does.
 *     LMS    N rows; c_e, c_h1..3 = the integrals of the Lagrange basis over [sigma_i, sigma_{i+1}]; the history is a ring
 *            over the 3 slots, each row pushing e into the slot of the oldest entry it read.
 * eps2 / cfg / guidance / step_dev / advance_ticket as pp_cfg_sched_step.  n need not be a multiple of 4. */
int pp_cfg_ksampler_step(const float* eps2, int cfg, float guidance, float* latents, float* state, const float* noise, int n,
                         const float* coef_table, int32_t* step_dev, uint32_t* advance_ticket, void* stream);

/* (ABI v18) Front end of Transformer2DModel at C = 320 in one launch (csrc/tfront.hip):
 *     hs = proj_in(GroupNorm(x)),   q | k | v = to_q / to_k / to_v(LayerNorm1(hs))
 * i.e. `hidden_states = self.norm(hidden_states); hidden_states = self.proj_in(hidden_states)` of diffusers 0.27
 * Transformer2DModel.forward plus `norm_hidden_states = self.norm1(hidden_states)` and the attn1 projections of
 * BasicTransformerBlock.forward (ctor site /root/reference/powerpaint/models/unet_2d_blocks.py:1289-1300).  x: raw rows
 * [M][c]; gn_acc: the (sum, sum of squares) accumulators of x in the format of PPGemmArgs.gn_acc, complete before the launch;
 * w1 / b1: proj_in [c][c] ([out][in]) and bias; w2p: the QKV weight [3c][c] with LayerNorm1's gamma folded in AND its input
 * index permuted inside every group of 32 (position 8 kg + j holds index 16 (j >> 2) + 4 kg + (j & 3): the MFMA
 * accumulator layout of the first GEMM is then the B-operand layout of the second); cs2 / b2: its column sums and W beta.
 * Outputs: hs [M][c] (the residual of attn1.to_out), qk [M][>= 2c] = Q | K, vt [batch][c][ldvt] = V transposed -- what
 * pp_attention_fwd reads.  Arithmetic = pp_groupnorm_apply_acc -> pp_gemm_bf16(row_stats_out) -> pp_gemm_bf16(ln_stats)
 * up to the fp32 summation order.  pp_tfront_supported() = 1 for c = 320, 128-row tiles inside one batch item.
 * q_scale (ABI v20): the Q third is multiplied by it in fp32 before its one rounding to 16 bits -- 1.0 for
 * pp_attention_fwd, head_dim^-0.5 * log2(e) for PP_ATTN_PIPE_LOG2.  hs and qk: 16-byte aligned, ldhs % 8 == ldqk % 8 == 0
 * (round 6: the rows leave as whole 128-byte lines).
 * Pinned by tests/test_tblock_exact_gpu.py:
 *   - gn_acc is TRUSTED as given: mean = sum / n, var = max(q / n - mean^2, 0) in fp64 with n = rows_per_batch * (c / gn_groups),
 *     rstd = (float)(1 / sqrt(var + gn_eps)); the kernel never looks at whether x has those moments.  One table per batch item
 *     b = (first row of the 128-row tile) / rows_per_batch; gn_groups: every divisor of 320 up to 32.
 *   - rounding points: the normalised row x * (rstd gamma) + (beta - mean rstd gamma) once to 16 bits; hs = that . w1^T + b1 once to
 *     16 bits; the LayerNorm1 moments from the STORED hs; each of Q * q_scale, K, V once.  q_scale touches the Q third only:
 *     two calls that differ in q_scale alone leave hs, K and V^T bit-identical.
 *   - V^T of tile rows [m0, m0 + 128) goes to vt[b][channel][m0 - b * rows_per_batch ..]; ldvt >= rows_per_batch, ldvt % 8 == 0,
 *     ldx >= c, ldhs >= c, ldqk >= 2 c (PP_ERR_BAD_ARG otherwise).  x may carry anything (NaN included) in the columns behind c;
 *     nothing is written outside the [M][c], [M][2 c] and [batch][c][rows_per_batch] windows. */
int pp_tfront_supported(int M, int c, int rows_per_batch, int gn_groups);
int pp_tfront(const void* x, int ldx, const void* gn_acc, const float* gn_gamma, const float* gn_beta, float gn_eps, int gn_groups,
              const void* w1, const float* b1, const void* w2p, const float* cs2, const float* b2, float ln_eps, void* hs,
              int ldhs, void* qk, int ldqk, void* vt, int ldvt, int M, int c, int rows_per_batch, float q_scale, int dtype,
              void* stream);
/* Fused cross-attention sub-block of BasicTransformerBlock (norm2 -> attn2 -> residual) for C = 320, 8 heads, <= 80
 * context tokens -- the three launches `to_q` (pp_gemm_bf16, LayerNorm folded) -> pp_attention_fwd -> `to_out`
 * (pp_gemm_bf16 + residual + row moments) of the 64x64 level as ONE (ctor site /root/reference/powerpaint/models/
 * unet_2d_blocks.py:1289-1300; diffusers 0.27 `BasicTransformerBlock.forward`: `attn2(norm2(h), encoder_hidden_states) + h`).
 * The encoder hidden states do not change during a call, so pp_xattn_fold contracts K into the query projection and V
 * into the output projection once per prompt:
 *     gt   [batch][heads*80][c]   G^T[b][h*80+key][:] = scale*log2(e) * sum_d K[b][key][h*d'+d] * wq[h*d'+d][:]   (16-bit)
 *     gcs, gbias [batch][heads*80] fp32: the same contraction of q_colsum / q_bias (the folded-LayerNorm terms of
 *          to_q; NULL = 0); gbias = -inf on the padded keys (key >= nctx), which masks them
 *     ht   [batch][c][heads*80]   H^T[b][n][h*80+key] = sum_d wo[n][h*d'+d] * V^T[b][h*d'+d][key], the contraction
 *          index permuted inside every group of 32 (position 8*kg + j holds index 16*(j>>2) + 4*kg + (j&3)) so that the
 *          accumulator registers of the logits are the B fragments of the second GEMM without any data movement
 * with k [batch*nctx][ldk] and vt [batch][c][ldvt] as pp_attention_fwd takes them, wq / wo [c][c] row-major
 * ([out][in]).  pp_xattn_block then computes, per 128-row tile (rows_per_batch % 128 == 0),
 *     p   = softmax_per_head( rstd*(x gt^T - mean*gcs) + gbias )          (exp2 domain; mean / rstd from ln_stats as in
 *                                                                           PPGemmArgs, NULL = no LayerNorm folded)
 *     out = p ht^T + bias_o + res ,   row_stats_out[m][c/160][2] = (sum, sum of squares) of the stored values.
 * (ABI v19) pre_w != NULL (C = 320): the Linear in FRONT of the sub-block rides in the same launch --
 *     h = x pre_w^T + pre_b + res     (BasicTransformerBlock: `attn1(norm1(h0)) + h0`, i.e. attn1.to_out applied to the
 *     self-attention output x, residual res = h0; pre_w [c][c] 16-bit ([out][in]), pre_b fp32 or NULL),
 * then the sub-block on h (rounded to 16 bits where the separate launch stored it): h is the logits' input, the source of
 * the LayerNorm row moments (computed in the kernel; ln_stats is ignored, ln_tiles > 0 = "a LayerNorm is folded into gt")
 * and the residual of the output.  The logits' B operand then comes out of the first GEMM's accumulators, so gt must be
 * packed with its channel index permuted inside every group of 32: pp_xattn_fold(kperm = 1) (position 8 kg + j holds
 * channel 16 (j >> 2) + 4 kg + (j & 3), the permutation pp_tfront uses).
 * (ABI v19) src_wrap_rows > 0: x, res and ln_stats hold only src_wrap_rows rows and output row m reads row
 * (m mod src_wrap_rows), M <= 2 * src_wrap_rows -- the two halves of a CFG batch are identical up to this sub-block (the
 * first place the prompt enters, unet_2d_condition.py:1183-1236), so everything in front of it ran on one half; the folded
 * operands (gt, gcs, gbias, ht) are per batch item of the FULL batch.  C = 320 only (PP_ERR_UNSUPPORTED otherwise).
 * pp_xattn_block_supported() = 1 when the shape is one this kernel takes (the caller keeps the three-launch chain
 * otherwise); both entry points return PP_ERR_UNSUPPORTED for other shapes.
 * (ABI v20) pp_xattn_fold(kperm = 2) stores ht with its contraction index in NATURAL order (column h * 80 + key): the
 * operands of the two-GEMM form of the same sub-block, where the row-local kernels lose (C = 1280: M <= 2048 rows) --
 *     P   = pp_gemm_bf16(x, w = gt, w_batch_stride = 640 c, bias = gbias, ln_colsum = gcs, vec_batch_stride = 640,
 *                        ln_stats, act = PP_ACT_SOFTMAX80)                          [M][640] probabilities
 *     out = pp_gemm_bf16(P, w = ht, w_batch_stride = 640 c, bias = bias_o, res1 = h, row_stats_out)
 * with half the multiplications of the chain at C = 1280 (2 x 640 c per row instead of 2 c^2 + 4 * 77 c).
 * Pinned by tests/test_tblock_exact_gpu.py:
 *   - pp_xattn_fold: gt = round16(fl32(fl32(sum) * fl32(scale * log2 e))), one rounding to 16 bits; gbias the same product kept in
 *     fp32; ht = round16(sum); gcs = 0 without q_colsum, else the fp32 sum of the STORED gt row (q_colsum itself is only a
 *     flag: its values are not read); padded keys (key >= nctx): gt row 0, gbias -inf, ht column 0.  kperm: bit 0 permutes the
 *     channel index of gt (C = 320 only), bit 1 leaves the contraction index of ht in natural order; 3 is PP_ERR_BAD_ARG.
 *     k may carry anything behind column c (ldk >= c), vt behind column nctx (ldvt >= nctx); gt / gcs / gbias / ht are dense.
 *   - pp_xattn_block: the probabilities are rounded once to 16 bits, the output once; the tables of batch item
 *     b = (first row of the tile) / rows_per_batch (of the FULL batch under src_wrap_rows); row_stats_out splits a row at every
 *     160 columns.  pre_w: h is rounded once, parked in the tile's own rows of `out` (never wrapped) and read back as the
 *     residual; x, res and ln_stats are wrapped, `out`, row_stats_out and the folded operands are not.  C = 640 / 1280
 *     (64-row tiles, one 320-column group per workgroup): no pre_w, no src_wrap_rows (PP_ERR_UNSUPPORTED).
 *     x / res may carry anything behind column c; out and res 16-byte aligned, ldx, ldo, ldres >= c and multiples of 8,
 *     src_wrap_rows a multiple of rows_per_batch with M <= 2 src_wrap_rows, pre_b only with pre_w (PP_ERR_BAD_ARG otherwise). */
int pp_xattn_block_supported(int M, int c, int rows_per_batch, int nctx, int heads);
int pp_xattn_fold(const void* k, int ldk, const void* vt, int ldvt, int batch, int nctx, int heads, int c, const void* wq,
                  const float* q_colsum, const float* q_bias, const void* wo, float scale, void* gt, float* gcs,
                  float* gbias, void* ht, int kperm, int dtype, void* stream);
int pp_xattn_block(const void* x, int ldx, const void* res, int ldres, const float* ln_stats, int ln_tiles, float ln_eps,
                   const void* gt, const float* gcs, const float* gbias, const void* ht, const float* bias_o, void* out,
                   int ldo, float* row_stats_out, int M, int c, int rows_per_batch, int src_wrap_rows, const void* pre_w,
                   const float* pre_b, int dtype, void* stream);

/* (ABI v19) FeedForward + proj_out of a C = 320 transformer in ONE launch (csrc/ff_fused.hip):
 *     out = epilogue2( [ h (.) gelu_erf(g) | hs ] W2'^T ),    h | g = rstd (hs W1^T - mean colsum1) + bias1   (interleaved)
 * i.e. `ff(norm3(hidden_states)) + hidden_states` of diffusers 0.27 BasicTransformerBlock.forward (FeedForward with GEGLU)
 * followed by Transformer2DModel.proj_out + the block residual (ctor site /root/reference/powerpaint/models/
 * unet_2d_blocks.py:1289-1300): the two launches pp_gemm_bf16(act = PP_ACT_GEGLU, folded LayerNorm) -> pp_gemm_bf16 over the
 * K-concatenation [g | hs] -- without the [M][1280] GEGLU tensor ever being written: the hidden dimension is streamed in
 * chunks of 64 units against persistent fp32 accumulators of the second GEMM.
 *   g2 : the SECOND GEMM exactly as pp_gemm_bf16 would take it (x_mode PLAIN, N = 320, c1 = 1280, c2 = 320, K = 1600):
 *        x2 / ldx2 = hs (raw rows: LayerNorm3 is folded), w = [W_po W_ff2 | W_po] ([320][1600], 16-bit) with the HIDDEN index
 *        (the first 1280 columns) permuted inside every group of 32 -- storage position 8 kg + 2 q + e holds unit
 *        8 q + 2 kg + e -- so that the GEGLU values in the first GEMM's accumulator registers are the second GEMM's B
 *        fragments; bias, scale, res1 (+ res1_wrap_rows), res2, out / ldo, dtype and the gn_acc subscriptions are honoured as
 *        in pp_gemm_bf16; x1 is NOT read (the tensor it would name does not exist).  rowvec, GEGLU / V^T / fp32 outputs, row
 *        moments, gn_next_*, out_dup_rows: PP_ERR_UNSUPPORTED.
 *   w1 : [2560][320] 16-bit, rows interleaved (h0, h1, g0, g1) as PP_ACT_GEGLU takes them, LayerNorm gamma folded in;
 *   b1 / cs1 : [2560] fp32 bias (incl. W beta) and column sums of w1 (cs1 may be NULL when ln_stats is NULL);
 *   ln_stats : row moments of hs in the layout of PPGemmArgs.ln_stats (ln_tiles partials per row) or NULL (no LayerNorm folded).
 * Arithmetic = the two-launch chain up to the fp32 summation order of the second GEMM (the GEGLU values are rounded to the
 * 16-bit format exactly where the chain stores them).  pp_ff_fused_supported(): c == 320, M and rows_per_batch multiples of 128.
 * w2_kperm: 1 = W2' with the hidden index permuted as above (four waves, the GEGLU chained in registers); 0 = W2' in NATURAL
 * hidden order (eight waves, the activations exchanged through LDS).  Both forms compute the same thing.
 * Pinned by tests/test_tblock_exact_gpu.py:
 *   - rounding points: h (.) gelu(g) once to 16 bits (gelu_fast_f: the gate +-16 gives exactly 16 / 0), the output once;
 *   - epilogue order: out = (acc + bias) * scale + (res1 + res2) -- the scale does NOT touch the residuals;
 *   - res1_wrap_rows > 0: res1 holds that many rows, M <= 2 res1_wrap_rows; the wrap is decided per 64-row PASS of the epilogue
 *     (rows [m0, m0 + 64) read res1 rows m0 - wrap when m0 >= wrap), so res1_wrap_rows % 64 == 0 is all that is needed: a wrap
 *     of 64 in the middle of a 128-row tile is honoured;
 *   - gn_acc: the moments of the values AS STORED, per batch item (first row of the tile) / rows_per_batch, one slot set per
 *     160-column half; gn_cg >= 8; the caller sizes gn_groups so that (gn_c0 + 319) / gn_cg < gn_groups (not checked);
 *     integer accumulation: a repeated call gives equal bits;
 *   - x2 / res1 / res2 may carry anything (NaN included) behind column 320; ldx2, ldo, ldres1, ldres2 >= 320 and multiples of
 *     8; x2, out, res1 and res2 16-byte aligned (PP_ERR_BAD_ARG otherwise; the last two conditions are refused since these
 *     tests: a short ldres or a misaligned base used to be launched). */
int pp_ff_fused_supported(int M, int c, int rows_per_batch);
int pp_ff_fused(const PPGemmArgs* g2, const void* w1, const float* b1, const float* cs1, const float* ln_stats, int ln_tiles,
                float ln_eps, int w2_kperm, void* stream);

/* ppt-v1 with a 4-channel (non-inpainting) UNet -- the `num_channels_unet == 4` branch of the loop body,
 * pipeline_PowerPaint.py:1025-1039: after pp_cfg_sched_step of the same step
 *     latents[b] = (1 - mask) * (a * image_latents + b * noise[b]) + mask * latents[b]
 * with (a, b) = renoise_table[step] = (sqrt(abar), sqrt(1 - abar)) of the NEXT timestep (`scheduler.add_noise(
 * init_latents_proper, noise, timesteps[i + 1])`), (1, 0) on the last step (the clean image latents are put back).
 * fp32; latents / noise [batch][channels][hw], image_latents [channels][hw] and mask [hw] = the FIRST image's
 * (`image_latents[:1]`, `mask[:1]` broadcast, as the reference does); renoise_table [steps][2]. */
int pp_latent_blend(float* latents, const float* image_latents, const float* mask, const float* noise,
                    const float* renoise_table, const int32_t* step_dev, int batch, int channels, int hw, void* stream);

/* (ABI v19) The head of a captured denoising step as ONE launch -- what pp_embed_splice (one row), pp_nchw_to_nhwc and
 * pp_zero_u64 did in three (each a launch floor of 5-6 us): temb_out[0 .. row_floats) = temb_table[step][:] (the per-schedule
 * table of the time-embedding chain's output, unet_2d_condition.py:1155-1156: it depends on the timestep alone);
 * x_in[b][p][c0 + j] = latents[b mod src_batch_mod][j][p] for j < c (fp32 NCHW -> 16-bit NHWC: `torch.cat([latents] * 2)`,
 * pipeline_PowerPaint.py:990, without the copy); zero_dst[0 .. n_zero) = 0 (64-bit words: the GroupNorm accumulators). */
int pp_step_head(const float* temb_table, const int32_t* step_dev, float* temb_out, int row_floats, const float* latents,
                 int batch, int c, int hw, int src_batch_mod, void* x_in, int ldc, int c0, int dtype, void* zero_dst,
                 long long n_zero, void* stream);
/* (ABI v26) pp_step_head for a sigma-space scheduler (Euler, Euler ancestral): the same launch, the latents branch writing
 * x_in[b][p][c0 + j] = to16(latents[b mod src_batch_mod][j][p] / in_div[step]) -- `scheduler.scale_model_input`
 * (pipeline_PowerPaint.py:993, pipeline_PowerPaint_Brushnet_CA.py:1391) with in_div[i] = sqrt(sigma_i^2 + 1), a device table
 * of one fp32 per schedule row indexed by step_dev[0].  The division is in fp32, the value is converted to 16 bits once.
 * Time-embedding row and zeroing exactly as pp_step_head. */
int pp_step_head_scaled(const float* temb_table, const int32_t* step_dev, float* temb_out, int row_floats, const float* latents,
                        int batch, int c, int hw, int src_batch_mod, void* x_in, int ldc, int c0, int dtype, void* zero_dst,
                        long long n_zero, const float* in_div, void* stream);
/* t_out[0] = timesteps[step]; used at the top of a captured step.  advance: ++step. */
int pp_step_select_t(const float* timesteps, const int32_t* step_dev, float* t_out, void* stream);
int pp_step_advance(int32_t* step_dev, void* stream);

/* Bit-exact mask prep (pipeline_PowerPaint.py:143-147,677-679; pipeline_PowerPaint_Brushnet_CA.py:1312,1342-1344):
 *   mode 0: out = (mask >= 0.5) ? 1 : 0                                  fp32 [n]
 *   mode 1: out = image * (mask < 0.5), mask broadcast over `c` channels  fp32 [batch][c][hw]
 *   mode 2: nearest downsample of a [batch][1][h][w] mask to [batch][1][ho][wo]  (F.interpolate default)
 *   mode 3: out = (sum_c rgb[b][c][p] < 0) ? 1 : 0                        (BrushNet original_mask)
 */
int pp_mask_prep(int mode, const float* a, const float* b, float* out, int batch, int c, int h, int w, int ho, int wo,
                 void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Task-prompt embedding splice -- the gather half of EmbeddingLayerWithFixes.forward
 * (/root/reference/powerpaint/utils/utils.py:378-483: ids >= num_embeddings -> row 0 of the base table, then the
 * learned [n_vec][dim] block of each placeholder is spliced over every occurrence of its id run).
 * The host walks the ids exactly as the reference does and hands over one source row per output row:
 *   src_row[i] >= 0 : out[i] = table[src_row[i]]            (base nn.Embedding weight)
 *   src_row[i] <  0 : out[i] = ext[-src_row[i] - 1]         (all external embeddings, concatenated along rows)
 * Rows are copied as `row_bytes` raw bytes (any dtype; bit-exact).  `ext` may be NULL when no src_row is negative.
 */
int pp_embed_splice(const void* table, const void* ext, const int32_t* src_row, void* out, int n_rows,
                    long long row_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Row softmax  p[r][c] = softmax_c(scale * s[r][c]),  fp32 logits -> bf16 probabilities.
 * The VAE mid-block attention (diffusers AutoencoderKL: one head of dim 512 over H*W tokens -- the call sites are
 * /root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:657-669,1051) is two pp_gemm_bf16 launches around this
 * kernel; pp_attention_fwd covers the UNet's head dims only.  lds / ldp: row strides in elements (multiples of 4).
 * (ABI v29) Columns [n, ldp) of every row of p are WRITTEN as zeros: a caller whose second GEMM needs K % 64 == 0 pads ldp
 * to it and multiplies the pad columns with zero-padded V^T columns (pp_transpose_v), whatever the buffer held before.
 * CONTRACT: every logit times scale * log2(e) must be FINITE in fp32.  The running maximum starts at -inf, so a thread whose
 * first four logits are all -inf (or overflow to it) forms exp2(-inf - -inf) = NaN and the whole row is NaN; a masked logit
 * is a large finite negative number, not -inf.  +-FLT_MAX / 2 at scale 0.5 is inside the contract (tests/small_cases.py).
 */
int pp_softmax_rows(const float* s, long long lds, int rows, int n, float scale, void* p, long long ldp, int dtype,
                    void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Attention for short sequences: the CLIP text tower the pipelines call through `self.text_encoder(ids)[0]`
 * (/root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:378-423; transformers CLIPTextModel: 77 tokens, 12 heads
 * of 64, causal mask).  q / k / v / o: bf16, element (b, t, h, j) at x[(b*n + t)*ld + h*d + j] (v NOT transposed).
 * d == 64, nk <= 128; causal: key j visible to query i iff j <= i (needs nq == nk).
 */
int pp_attention_small(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                       int batch, int heads, int nq, int nk, int d, float scale, int causal, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (ABI v23) LoRA merge: one block of a packed parameter tensor rebuilt in place from its fp32 source weight and up to
 * PP_LORA_MAX_ADAPTERS low-rank adapters.  The reference keeps adapters as side branches: its pipelines inherit
 * LoraLoaderMixin (/root/reference/powerpaint/pipelines/pipeline_PowerPaint_Brushnet_CA.py:147-148), forward
 * cross_attention_kwargs["scale"] to the UNet (/root/reference/powerpaint/models/unet_2d_condition.py:1192-1195,1357-1358)
 * and to the text encoder (pipeline_PowerPaint_Brushnet_CA.py:451-493,1248), two small GEMMs per adapted layer per step.
 * Here the step is a fixed launch plan over one parameter buffer, so the adapters are folded INTO that buffer:
 *     W_eff[n][k] = W[n][k] + sum_a coef[a] * sum_r up[a][n][r] * down[a][r][k]         (fp32, fmaf chains)
 *     out[row_off + rowmap(n)][col_off + colmap(k)] = round(W_eff[n][k] * gamma[k])     (one rounding to out_dtype)
 *   w     : fp32 [N][K] in SOURCE (diffusers) order, row stride ldw; a conv [Cout][Cin][kh][kw] is K = Cin*kh*kw
 *   up[a] : fp32 [N][rank[a]], down[a] : fp32 [rank[a]][K], coef[a] = adapter weight * call scale * alpha / rank
 *   gamma : NULL or fp32 [K] per-column factor (the LayerNorm weight of a folded entry), indexed by SOURCE column
 *   rowmap: PP_LORA_ROWS_PLAIN n | PP_LORA_ROWS_GEGLU [h ; g] halves -> quads (h_2q, h_2q+1, g_2q, g_2q+1), N % 4 == 0
 *   colmap: PLAIN k | IGEMM (c, t) -> t * cin_pad + c with taps = kh*kw (channels cin..cin_pad-1 are written as zero) |
 *           KPERM / KPERM_GEGLU the permutations inside groups of 32 of the chained-GEMM kernels (K % 32 == 0)
 *   out   : out_dtype PP_DT_BF16 / PP_DT_F16 / PP_DT_F32 (unrounded), a matrix of out_rows x out_cols elements with
 *           row stride ldo; a block that does not lie inside it is PP_ERR_BAD_ARG
 *   colsum: NULL or fp32, colsum[row] = sum over the block's columns of the values AS STORED (rounded), by destination row
 *   bias  : NULL or fp32, bias[row] = sum_k W_eff[n][k] * beta[k] + badd[n]  (beta [K] and badd [N] each optional)
 * Zero adapters is a plain re-pack.  More than 8 adapters or a rank outside 1..128 is PP_ERR_BAD_ARG (the caller refuses,
 * calls are not chained).  Side vectors make the launch walk all columns of a 64-row block in one workgroup.
 */
#define PP_LORA_MAX_ADAPTERS 8
#define PP_LORA_MAX_RANK 128
#define PP_LORA_ROWS_PLAIN 0
#define PP_LORA_ROWS_GEGLU 1
#define PP_LORA_COLS_PLAIN 0
#define PP_LORA_COLS_IGEMM 1
#define PP_LORA_COLS_KPERM 2
#define PP_LORA_COLS_KPERM_GEGLU 3
typedef struct PPLoraMergeArgs {
  int32_t N, K;
  const float* w;
  int64_t ldw;
  int32_t n_adapters;
  int32_t rank[PP_LORA_MAX_ADAPTERS];
  float coef[PP_LORA_MAX_ADAPTERS];
  const float* up[PP_LORA_MAX_ADAPTERS];
  const float* down[PP_LORA_MAX_ADAPTERS];
  const float* gamma;
  const float* beta;
  const float* badd;
  void* out;
  int64_t ldo;
  int32_t out_rows, out_cols, out_dtype;
  int32_t row_mode, row_off;
  int32_t col_mode, col_off, taps, cin_pad;
  float* colsum;
  float* bias;
} PPLoraMergeArgs;
int pp_lora_merge(const PPLoraMergeArgs* args, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (ABI v24) FreeU in front of an up-block resnet (diffusers-0.27 apply_freeu / fourier_filter with threshold = 1, called
 * per resnet by the reference's first two up blocks, powerpaint/models/unet_2d_blocks.py:2563-2587, 2706-2730), ONE launch:
 *     hidden_out[b][p][c] = hidden[b][p][c] * (c < ch / 2 ? bs[0] : 1)
 *     skip_out = fourier_filter(skip, scale = bs[1]): per channel plane, with X(u,v) = sum_{h,w} x[h,w] e^{-2 pi i (uh/H + vw/W)},
 *         y[h,w] = x[h,w] + (bs[1] - 1) / (H W) * Re sum_{(u,v) in {-1,0}^2} X(u,v) e^{+2 pi i (uh/H + vw/W)}
 *     (the four bins the mask of the shifted spectrum scales; the set is not Hermitian-symmetric, Re is part of the definition)
 *   hidden / skip : 16-bit NHWC [batch][h][w][ch] / [batch][h][w][cs], 4-byte aligned; ch % 4 == 0 (ch / 2 even), cs % 2 == 0,
 *                   h, w >= 2 (h + w <= 512, else PP_ERR_UNSUPPORTED)
 *   hidden_out    : may BE hidden (only the scaled half is then written); skip_out may BE skip; the two tensors must not
 *                   alias each other
 *   bs            : DEVICE pointer to (b, s), fp32 -- read by the kernel, so a captured graph follows new values
 *   acc           : NULL, or int64 [batch][groups][2], 8-byte aligned, (ch + cs) % groups == 0, groups <= 64: the launch ADDS the
 *                   (sum, sum of squares) of concat(hidden_out, skip_out) per group, of the values as stored, in the fixed point
 *                   of PPGemmArgs.gn_acc -- what pp_groupnorm_apply_acc / gn_in_acc of the resnet's norm1 read (the sums the
 *                   producers' epilogues took describe the tensors before FreeU)
 * Arithmetic fp32, one rounding to `dtype` (bf16 / fp16). */
int pp_freeu(const void* hidden, void* hidden_out, int ch, const void* skip, void* skip_out, int cs, int batch, int h, int w,
             const float* bs, int64_t* acc, int groups, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (added under ABI 29; purely additive) IP-Adapter: the image-prompt term of the decoupled cross-attention of diffusers-0.27
 * IPAdapterAttnProcessor2_0, added IN PLACE to the output of the text cross-attention, ONE launch per adapter:
 *     o[b][r][h*d .. (h+1)*d) += ip_scale * sum_j softmax_j(qk_scale * q[b][r][h] . k_ip[b][j][h]) * v_ip[b][j][h]
 *   q, o       : 16-bit [batch * nq][heads * d] with row strides ldq / ldo (elements, multiples of 8, >= heads * d), 16-byte
 *                aligned, not overlapping; q is only read
 *   k_ip, v_ip : 16-bit [batch][nk][heads * d], contiguous, 16-byte aligned: to_k_ip / to_v_ip of the adapter's image tokens
 *   d          : 40, 80 or 160 (else PP_ERR_UNSUPPORTED; d % 8 != 0 is PP_ERR_BAD_ARG); 1 <= nk <= PP_IP_MAX_TOKENS (4 tokens
 *                per image of a base adapter: 16 images); heads <= 64, batch <= 65535
 *   ip_scale   : by value.  0 is "no term": the call returns PP_OK without a launch and o keeps its bits
 * Scores, softmax (maximum subtracted), the weighted sum and the add are fp32, one rounding to `dtype` (bf16 / fp16) at the
 * store; every element of o is read once and written once by the same lane, nothing outside [batch * nq) x [heads * d) is
 * touched (the gaps of ldo > heads * d included). */
#define PP_IP_MAX_TOKENS 64
int pp_ip_attn_add(const void* q, int ldq, const void* k_ip, const void* v_ip, void* o, int ldo, int batch, int heads, int nq,
                   int nk, int d, float qk_scale, float ip_scale, int dtype, void* stream);

/* (added under ABI 29; purely additive) pp_ip_attn_add under diffusers-0.27 `ip_adapter_masks`: the term of query row r is
 * multiplied by row_w[r] (IPAdapterMaskProcessor.downsample of the adapter's mask: one value per query row, in flat row
 * order, the same for every batch item and channel):
 *     o[b][r][:] += ip_scale * row_w[r] * sum_j softmax_j(qk_scale * q[b][r][h] . k_ip[b][j][h]) * v_ip[b][j][h]
 *   row_w      : DEVICE pointer to fp32 [nq], 4-byte aligned -- read by the kernel, so a captured graph follows new values.
 *                NULL or unaligned is PP_ERR_BAD_ARG.  Any finite value: a bicubic resize of a binary mask rings below 0
 *                and above 1.
 *   everything else as pp_ip_attn_add: the same limits and return codes, ip_scale == 0 launches nothing
 * Arithmetic as pp_ip_attn_add, ip_scale * row_w[r] formed in fp32, still ONE rounding to `dtype` at the store.  With
 * row_w[r] == 1.0f the row is pp_ip_attn_add's bit for bit.  A row with row_w[r] == 0.0f keeps its bits in o (signed zeros
 * included): it is neither read (q, o) nor written, and a group of rows that are all 0 costs no arithmetic either. */
int pp_ip_attn_add_masked(const void* q, int ldq, const void* k_ip, const void* v_ip, void* o, int ldo, int batch, int heads,
                          int nq, int nk, int d, float qk_scale, float ip_scale, const float* row_w, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * IP-Adapter Plus (added under ABI 29: purely additive).  The attention of the adapter's Resampler -- a few latent queries
 * over the image rows AND the latent rows, which the two to_kv GEMMs of a layer leave in two buffers:
 *     o[b,i,h*d:(h+1)*d] = sum_t softmax_t(scale * q[b,i,h] . K[b,t,h]) V[b,t,h],   t over nx + nl keys
 *   q, o  : 16-bit, element (b, i, h, j) at [(b*nq + i)*ld + h*d + j]; ldq, ldo >= heads*d; q is only read, q != o
 *   kv_x  : 16-bit rows of [K | V]: key t < nx of item b is row b*nx + t (row stride ldkx >= 2*heads*d), K at column
 *           h*d + j, V at column heads*d + h*d + j -- what a to_kv GEMM writes
 *   kv_l  : likewise with nl rows per item: keys nx .. nx + nl - 1.  nl = 0 with kv_l = NULL is plain cross-attention
 *           (nl > 0 without kv_l, or the reverse, is PP_ERR_BAD_ARG)
 *   d     : 64 (else PP_ERR_UNSUPPORTED); nq >= 1, nx >= 1, nl >= 0, any number of keys (they are walked in tiles with a
 *           running maximum and sum); every leading dimension a multiple of 8, every pointer 16-byte aligned
 *           (PP_ERR_BAD_ARG otherwise); batch, heads <= 65535
 * Scores, softmax (maximum subtracted; the denominator sums the unrounded probabilities) and accumulation are fp32; the
 * probabilities are rounded once to `dtype` for the P V matrix product; one rounding to `dtype` (bf16 / fp16) at the store.
 * Nothing outside rows [0, batch*nq) x columns [0, heads*64) of o is written; nothing behind the last key row of either
 * segment, and no column behind 2*heads*64, reaches the result (they may hold anything finite or not). */
int pp_perceiver_attn(const void* q, int ldq, const void* kv_x, int ldkx, int nx, const void* kv_l, int ldkl, int nl, void* o,
                      int ldo, int batch, int heads, int nq, int d, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Token merging (added under ABI 29: purely additive).  ToMe for Stable Diffusion (Bolya & Hoffman 2023; tomesd's
 * bipartite_soft_matching_random2d) in front of a self-attention: the r most redundant tokens of an h x w grid are averaged
 * into their most similar DESTINATION token, attention runs on n - r rows, and its output is copied back out to all n.
 *   geometry   : n = h*w tokens per batch item in row-major order; one token of every sy x sx window (hsy = h / sy rows of
 *                wsx = w / sx windows, integer division) is a destination, nd = hsy*wsx of them; every other token -- the
 *                leftover rows and columns of sizes that are no multiple of the window included -- is a source.
 *   table      : uint8 rows of >= nd entries (row stride table_row_stride bytes, table_rows rows): entry i*wsx + j of a row is
 *                the in-window index k of the destination of window (i, j), token (i*sy + k / sx, j*sx + k % sx).  A value
 *                >= sx*sy is read as sx*sy - 1.
 *   row_idx    : DEVICE pointer to one int32, the table row to use, clamped to [0, table_rows) -- read by the kernel, so a
 *                captured graph follows a device-side step counter with no re-capture.  NULL: row 0.
 *   merged sequence (n - r rows): the kept sources in ascending token order, then the destinations in ascending token order.
 * pp_tome_supported: 1 where the four entries run the geometry (h, w >= 2, at least one window, sx*sy <= 256,
 * n <= PP_TOME_MAX_TOKENS, C a positive multiple of 8), else 0; they return PP_ERR_UNSUPPORTED there and launch nothing.
 *
 * pp_tome_match: x 16-bit [batch*n][C] (row stride ldx >= C, a multiple of 8; 16-byte aligned), the hidden state the matching
 *   is computed from.  best_dst int32 [batch][n], score fp32 [batch][n]: per SOURCE token the destination token with the
 *   highest cosine and that cosine; an equal maximum goes to the lower destination token.  Destination tokens get
 *   best_dst = -1 and score = -2.  The dot products are accumulated in fp32 on the matrix cores from the 16-bit values; the
 *   inverse norms are fp32 (1 / sqrt of the fp32 sum of squares of the same values; a zero row has inverse norm 0, cosine 0).
 * pp_tome_select: the r sources with the highest score are merged (an equal score goes to the lower token), 0 <= r <= n - nd.
 *   pos    int32 [batch][n]      merged-sequence row of every token (a merged source: the row of its destination)
 *   rowtok int32 [batch][n - r]  the token a merged-sequence row starts from (the kept source, or the destination)
 *   seg    int32 [batch][nd + 1] list bounds: the sources merged into the destination of rank d are lst[seg[d] .. seg[d+1])
 *   lst    int32 [batch][r]      merged source tokens, grouped by destination rank, ascending token order inside a group
 * pp_tome_merge: qk 16-bit rows [batch*n][2C] (row stride ldqk) and vt 16-bit [batch][C][ldvt] (V transposed, ldvt >= n) ->
 *   qk_out [batch*(n - r)][2C] (row stride ldqk_out) and vt_out [batch][C][ldvt_out], ldvt_out >= round8(n - r) a multiple of 8, the
 *   columns [n - r, round8(n - r)) written as zeros (what pp_attention_fwd may read), none behind them.  A destination row is the mean of itself and its list (fp32 sum in list order,
 *   one division, ONE rounding to `dtype`); every other row is copied.  Outputs must not alias inputs.
 * pp_tome_unmerge: out[b][t][0:C] = a[b][pos[b][t]][0:C], 16-bit rows (a: nm = n - r rows per item, row stride lda; out: n rows,
 *   row stride ldo); a pos outside [0, nm) is clamped.
 * Leading dimensions of row buffers are multiples of 8 and their pointers 16-byte aligned; int32 / fp32 buffers 4-byte
 * aligned (PP_ERR_BAD_ARG otherwise).  Nothing outside the stated outputs is written (the gaps of a padded leading dimension
 * included).  No floating-point atomics: the same inputs give the same bits on every run. */
#define PP_TOME_MAX_TOKENS 16384
int pp_tome_supported(int h, int w, int C, int sx, int sy);
int pp_tome_match(const void* x, int ldx, int batch, int h, int w, int C, int sx, int sy, const void* table,
                  int table_row_stride, int table_rows, const void* row_idx, void* best_dst, void* score, int dtype,
                  void* stream);
int pp_tome_select(const void* best_dst, const void* score, int batch, int n, int nd, int r, void* pos, void* rowtok, void* seg,
                   void* lst, void* stream);
int pp_tome_merge(const void* qk, int ldqk, const void* vt, int ldvt, int batch, int n, int C, int nd, int r, const void* rowtok,
                  const void* seg, const void* lst, void* qk_out, int ldqk_out, void* vt_out, int ldvt_out, int dtype,
                  void* stream);
int pp_tome_unmerge(const void* a, int lda, const void* pos, int batch, int n, int nm, int C, void* out, int ldo, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Perturbed-attention guidance (added under ABI 29: purely additive).  PAG (diffusers' PAGMixin) runs one more segment of
 * the batch whose selected self-attentions are replaced by the identity -- their output is V -- and guides away from it.
 *
 * pp_attn_identity_v: out[b][p][c] = vt[b][c][p] for b in [batch0, batch0 + batch), p < n, c < C: the attention output of
 *   the perturbed batch items, copied out of V^T (16-bit [all items][C][ldvt], what pp_transpose_v, the QKV GEMM's out_vt
 *   epilogue and pp_tfront leave) into the attention output rows (16-bit, item b's rows are b*n .. b*n + n - 1, row stride
 *   ldo).  A bit copy: bf16 and fp16 alike.  The inverse of pp_transpose_v.
 *   C % 8 == 0, ldvt >= n, ldvt % 8 == 0, ldo >= C, ldo % 8 == 0, any n >= 1; batch0 >= 0, 1 <= batch <= 65535; pointers
 *   2-byte aligned (16-byte aligned pointers get 16-byte accesses on both sides).  PP_ERR_BAD_ARG otherwise, without a launch.
 *   Columns [n, ldvt) of V^T may hold anything: they may be read and never reach `out`.  Rows of `out` of other batch items
 *   and the bytes behind column C of a row are never written.  out must not alias vt.
 *
 * pp_pag_combine: eps fp32 [3][n] (cfg = 1: e_u, e_c, e_p) or [2][n] (cfg = 0: e_c, e_p), the last segment the perturbed one.
 *   With s = pag_table[step_dev[0]] (fp32 table on the device, one scale per schedule row; step_dev the loop's int32 step
 *   counter, read and NOT moved) segment 0 becomes, in place,
 *       cfg = 1:  e_u + guidance * (e_c - e_u) + s * (e_c - e_p)          cfg = 0:  e_c + s * (e_c - e_p)
 *   every element from its own index only; the other segments are not written.  The scheduler's step launch behind it runs
 *   with cfg = 0 on segment 0.  n >= 1 need not be a multiple of 4; eps 4-byte aligned; cfg is 0 or 1 (PP_ERR_BAD_ARG). */
int pp_attn_identity_v(const void* vt, int ldvt, int batch0, int batch, int n, int C, void* out, int ldo, void* stream);
int pp_pag_combine(float* eps, int cfg, float guidance, const float* pag_table, const int32_t* step_dev, int n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * guidance_rescale (added under ABI 29: purely additive).  diffusers' `rescale_noise_cfg` (Lin et al., "Common Diffusion
 * Noise Schedules and Sample Steps are Flawed", section 3.4): the guided prediction of every sample is pulled back to the
 * standard deviation of that sample's conditional prediction.  No counterpart in the reference.
 *
 * pp_cfg_rescale: eps fp32 [segs][batch][per], the `per` = C*H*W values of one sample contiguous.  segs = 2: (e_u, e_c),
 *   pag_table NULL (step_dev is not read and may be NULL).  segs = 3: (e_u, e_c, e_p), pag_table non-NULL and
 *   s = pag_table[step_dev[0]] as pp_pag_combine reads it (step_dev read and NOT moved).  phi = phi_dev[0]: one fp32 in
 *   device memory, read by the launch (a captured graph sees the value the cell holds when it is replayed).  With
 *       m = e_u + guidance * (e_c - e_u)  [+ s * (e_c - e_p)]            (the step kernels' / pp_pag_combine's expression)
 *       SSD(x[b]) = sum_i (x[b][i] - mean(x[b]))^2                        (two passes: the mean first; never sum x^2)
 *   segment 0 of sample b becomes, in place,   m * (phi * sqrt(SSD(e_c[b]) / SSD(m[b])) + (1 - phi)).
 *   Only the ratio of the two deviations enters, so torch.std's n - 1 cancels.  A sample whose m has no variance divides by
 *   0, as the library does.  The other segments, the table, the cell and the counter are not written.  The scheduler's step
 *   launch behind it runs with cfg = 0 on segment 0.
 *   One launch, one workgroup per sample, no atomics: a sample's result depends on its own values, on `per` and on whether
 *   the 16-byte path is taken (per % 4 == 0 and eps 16-byte aligned) -- not on batch, on its index in the batch or on the run.
 *   batch >= 1, per >= 2 (need not be a multiple of 4), eps 4-byte aligned; PP_ERR_BAD_ARG otherwise, and for segs outside
 *   {2, 3}, segs = 3 without a table or step counter, segs = 2 with a table, NULL eps or phi_dev -- all without a launch. */
int pp_cfg_rescale(float* eps, int segs, float guidance, const float* pag_table, const float* phi_dev, const int32_t* step_dev,
                   int batch, int per, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (added under ABI 29; purely additive) AsymmetricAutoencoderKL -- the mask-conditioned VAE decoder of diffusers-0.27
 * (autoencoder_asym_kl.py; vae.py: MaskConditionEncoder / MaskConditionDecoder; Zhu et al., arXiv:2306.04632).
 *
 * pp_conv4x4s2: nn.Conv2d(cin, cout, kernel_size=4, stride=2, padding=1) (layers 2..4 of the condition encoder) as an implicit
 *   GEMM on the matrix cores over all sixteen taps: 16 cin cout MACs per output pixel (+ the padding of the 128 x 128 tiles).
 *     x    : 16-bit NHWC [batch][hin][win][cin], 16-byte aligned, cin % 64 == 0, hin, win >= 2
 *     w    : 16-bit [cout][16 cin], column (4 ky + kx) cin + c; 16-byte aligned; cout % 4 == 0
 *     bias : fp32 [cout] or NULL, added to the fp32 accumulator before the one rounding
 *     out  : 16-bit NHWC [batch][(hin - 2) / 2 + 1][(win - 2) / 2 + 1][cout], 8-byte aligned
 *     relu_in != 0: the convolution reads max(x, 0) -- applied as the operand is loaded, x itself is not written (the
 *       decoder's blends read the pre-ReLU tensor).  A NaN with the sign bit set is read as 0.
 * pp_relu: out[i] = max(x[i], 0) over n 16-bit values (n % 8 == 0, 16-byte aligned, out may be x); the same sign-bit rule.
 * pp_masked_image_pack: out[b][p][k] = (1 - mask[b][p]) * image[b][k][p] for k < c, 0 for c <= k < 8: fp32 NCHW image
 *   [batch][c][h w] and fp32 mask [batch][h w] -> the 8-channel 16-bit NHWC image pp_conv3x3_direct reads (16-byte aligned).
 *   c <= 8.  fp32 arithmetic, one rounding.
 * pp_mask_blend: the blend in front of every up block of MaskConditionDecoder and behind the last,
 *       out[b][y][x][k] = sample * m + cond * (1 - m),   m = mask[b][y * mask_h / h][x * mask_w / w]
 *   (F.interpolate(mode="nearest") of the full-resolution mask; mask_h % h == 0 and mask_w % w == 0), computed as
 *   fma(sample, m, cond * (1 - m)) in fp32 -- three roundings -- and rounded once to `dtype`.  Linear in m: any float mask.
 *     sample, cond, out : 16-bit NHWC [batch][h][w][c], 16-byte aligned, c % 64 == 0; out may be sample
 *     mask              : fp32 [batch][mask_h][mask_w], one plane per batch item
 *     acc               : NULL, or int64 [batch][groups][2], c % groups == 0: the launch ADDS (sum, sum of squares) of the
 *                         values it stored, per group, in the fixed point of PPGemmArgs.gn_acc (what pp_groupnorm_apply_acc
 *                         reads): fp32 partial sums of 8 values per thread in a fixed order, then 64-bit integer atomics, so
 *                         the result does not depend on the order of the workgroups.  No floating-point atomics.
 *     cond == NULL      : nothing is blended or written; the launch only adds the statistics of `sample` to acc (the
 *                         unconditioned decode takes its statistics on the same route, so that a mask of ones reproduces it
 *                         bit for bit). */
int pp_conv4x4s2(const void* x, int batch, int hin, int win, int cin, const void* w, const float* bias, int cout, int relu_in,
                 void* out, int dtype, void* stream);
int pp_relu(const void* x, void* out, long long n, int dtype, void* stream);
int pp_masked_image_pack(const float* image, const float* mask, int batch, int c, int h, int w, void* out, int dtype,
                         void* stream);
int pp_mask_blend(const void* sample, const void* cond, const float* mask, void* out, int batch, int h, int w, int c,
                  int mask_h, int mask_w, int64_t* acc, int groups, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (added under ABI 29; purely additive) AutoencoderTiny -- TAESD, diffusers' autoencoder_tiny.py (vae.py: EncoderTiny /
 * DecoderTiny / AutoencoderTinyBlock): a 64-channel conv net without norms or attention on the SD latent space.
 *
 * pp_conv3x3_c64: nn.Conv2d(64, 64, 3, padding=1) with bias, residual and ReLU in the epilogue,
 *       out = [relu](acc + bias + res),   fp32 accumulator over the 576 products, ONE rounding to `dtype`.
 *     x    : 16-bit NHWC [batch][hin][win][64], 16-byte aligned
 *     w    : 16-bit [64][3][3][64] = [cout][(3 ky + kx) 64 + cin], 16-byte aligned
 *     bias : fp32 [64], 16-byte aligned, or NULL
 *     res  : NULL, or a 16-bit NHWC tensor of the output's shape, 8-byte aligned; must not alias out
 *     out  : 16-bit NHWC [batch][hout][wout][64], 8-byte aligned
 *     mode : 0  stride 1, hout = hin
 *            1  stride 2, symmetric padding 1, hout = (hin - 1) / 2 + 1 (odd sides included)
 *            2  nn.Upsample(scale_factor=2, mode="nearest") in front of the stride-1 conv: the conv reads source pixel
 *               (output pixel >> 1), its padding 1 lies at the output resolution, hout = 2 hin
 *   The whole weight matrix is kept in LDS by persistent workgroups that walk the output tiles; the input tile with its
 *   one-pixel halo is staged in LDS, so an input element is fetched once per tile.  No atomics, no workspace.  A value is one
 *   fixed-order sum: it does not depend on `batch` or on the item's place in the batch.  PP_ERR_BAD_ARG for a dtype that is
 *   not bf16 / fp16, a NULL x / w / out, mode outside 0..2, non-positive sizes or a misaligned pointer -- without a launch.
 * pp_taesd_pack: the two maps at the module boundary.  src fp32 | bf16 | fp16 (src_dtype: PP_DT_*) NCHW [batch][c][h w], c <= 8
 *   -> out 16-bit NHWC [batch][h w][8] (16-byte aligned; what pp_conv3x3_direct reads), channels [c, 8) WRITTEN as zeros.
 *     mode 0 (image)  : (x + 1) / 2            mode 1 (latents): 3 tanh(x / 3)   (+-inf -> +-3)
 *   fp32 arithmetic, one rounding to `dtype`. */
int pp_conv3x3_c64(const void* x, int batch, int hin, int win, const void* w, const float* bias, const void* res, int mode,
                   int relu, void* out, int dtype, void* stream);
int pp_taesd_pack(const void* src, int src_dtype, int batch, int c, int h, int w, int mode, void* out, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PP_HIP_H_ */
