"""Shared by tests/test_gemm_probes.py (CPU) and tests/test_gemm_exact_gpu.py (-m gpu): probes, fp64 references, derived
gates, the memory layout and a CPU restatement of the tile / K walk of powerpaint_amd/csrc/gemm.hip and of the halo-tile loop
of csrc/conv_gn.hip.  Plain torch; touches no HIP.

THE OP (include/pp_hip.h "Epilogue", read off epilogue4 / the staged epilogue / the three combines of gemm.hip, the halo-tile
epilogue of conv_gn.hip and gemm_combine.h -- all six agree):

    acc  = sum_k X[m][k] W[n][k]                                    fp32, MFMA
    v    = (acc + bias[n] + rowvec[m / rows_per_batch][n]) * scale   fp32
    v    = v + (res1[row1(m)][n] + res2[m][n])                       fp32; row1(m) = m - wrap if wrap > 0 and m >= wrap
    v    = act(v)                                                    NONE | SiLU | GEGLU (h * gelu(g) of interleaved quads)
    out  = round_to_nearest_even_16(v)                               the ONE rounding to the 16-bit format (none if out_f32)

(the two residuals are added to each other first in the staged epilogue and the combines, one after the other in epilogue4:
the same real number, at most one fp32 rounding apart).  `epilogue64` below is that order in fp64; every reference uses it.

PROBE E (integer-exact, compared for BIT EQUALITY).  x in {-1, 0, +1} with density p = min(1/2, 256/K), w in {+-1, +-2},
bias / rowvec / res1 / res2 integers in [-8, 8], scale in {1, 0.5}.  Every product and every partial sum, in any order, is
an integer of magnitude <= S = sum |x||w|, and the builder asserts S < 2^24: fp32 accumulation is then exact under any
tiling, order, K split and whatever the MFMA does inside.  The epilogue adds integers (exact) and multiplies by a power of
two (exact), so fp32 v = the fp64 v; the builder asserts that v is representable in the output format, so the stored value
is the fp64 result cast once.  Any dropped, doubled or mis-sourced element moves an exact value by >= 0.5.  The builder also
asserts that every 64-row x 64-deep block of X holds a non-zero (no K tile of any M tile is invisible).  The side outputs are
exact on the same data: the fp32 output, the V^T store, out_dup_rows, res1_wrap_rows, the per-row moments of row_stats (sums
of <= 160 integers |v| <= 256 and of their squares: < 2^24) and the int64 GroupNorm accumulators.  For the latter the
epilogues (gemm.hip: gcs / gcq per thread over its rows of <= 256-row tiles, folded over <= 16 row-threads; the gn combine:
16-row column sums; gn_column: sm * 2^24 and sq * 2^20 are power-of-two scalings, exact, then __float2ll_rn) form fp32
partials over at most 256 rows of one column; they stay integers below 2^24 iff 256 max v^2 < 2^24, which the builder asserts
(`gn_partials_exact`).  No path breaks it, so norm_cases.gate_epilogue_acc is not needed here.  The sub-pixel upsampling
form folds sums of <= 4 weights in [-2, 2] (|.| <= 8, exact in 16 bits): pp_upconv_fold and the four-tap launch are both
bit-exact against the nine-tap fp64 reference.

PROBE T (ties and single rounding, BIT EQUALITY).  acc[m][n] = BASE + (m mod 16) + (n mod 16) from three non-zero K columns
(x[m][0] = BASE/2, w[n][0] = 2; x[m][1] = m mod 16, w[n][1] = 1; x[m][2] = 1, w[n][2] = n mod 16); BASE = 256 (bf16: ulp 2 on
[256, 512)) or 2048 (fp16: ulp 2 on [2048, 4096)), so odd sums are exact ties.  Variants: `rne` (no epilogue: a truncating
store fails on every odd sum), `res` (res1 = +-1 makes odd sums even: a 16-bit rounding of the accumulator before the residual
is off by 2 where RNE went the other way), `bias` (bias 0.5, scale 2: (acc + 0.5) * 2 = 2 acc + 1 against 2 acc + 0.5, BASE
halved so that the result lies in the same binade), `b256` (fp16 only, BASE 256: every value exact in fp16, odd ones are not
bf16 values: an epilogue that passes through bf16 fails).

PROBE R (random, fp64 reference, derived gate).  R+: x, w uniform in [0.5, 1), w times 2^-e, no bias / residual, so
A = sum |x||w| = ref and the gate is purely relative.  R-: N(0,1) rounded to the format, w times K^-1/2, all epilogue
operands; SiLU / GEGLU run here only.  Gate per element:

    |out - ref| <= u |ref| + n_r 2^-24 A,   u = 2^-8 (bf16) | 2^-11 (fp16)   (the convention of attention_cases.py)

A = the sum of the absolute values of everything added into the element (|x||w| products, |bias|, |rowvec|, all times
|scale|, |res1|, |res2|); n_r = the number of fp32 roundings on the path, worst case: how an MFMA rounds inside one
instruction is not documented, so each is bounded by its K depth, one rounding per product added => K for the accumulation
under any tiling; + (splits - 1) adds of the combine; + the epilogue operations: bias, rowvec, scale, res1 + res2, + v: 5.
n_r = K + splits + 5 (`n_roundings`), never tuned to what the hardware achieves.  For K = 2944 the R+ gate is 1.045 u
(bf16) / 1.36 u (fp16).  SiLU / GELU add the terms of norm_cases (its docstring, "SiLU" and "GEGLU"): the derivative bound
propagates the pre-activation error d: SiLU (slope <= 1.1) 1.1 d + (7 + |v|) 2^-24 |y|, GEGLU h gelu(g)
d_h |gelu(g)| + (|h| + d_h) (1.13 d_g + 2^-20 |g|) + 2 2^-24 |y| (gelu_fast_f is within 2^-20 |g|), as `gate` writes them.

MEMORY (`build`, `lay`, `sentinel_out`).  Every output (out, out_vt, out_f32, row_stats) is a window of a larger sentinel-filled buffer: 64 rows in
front, 64 behind, 8 pad columns (ldo = N + 8; vt_ld = rows_per_batch + 8); row_stats, for which the ABI has no stride, gets
the rows only.  After the launch every byte outside the window must be unchanged.  The split-K workspace gets a sentinel
tail.  x, x2, res1 are windows with ld = cols + 8, res2 with ld = cols + 16 (a stride different from ldo: with three equal
strides `res_uses_ldo` could not be seen), pad columns and 64 rows behind the last row filled with a finite poison (1000: a
kernel may read it, it may not reach a result: one poisoned element moves an exact value by >= 500); w is followed by 8
poisoned rows, bias by 8 poisoned entries.  Conv inputs are dense NHWC (the ABI has no pixel stride) with 64 poison rows in
front of image 0 and behind the last image; B >= 2 makes a halo read across an image border land on real, different data.
`ld4` cases use pads of 4 columns: rows are then 8-byte aligned only, v2_ok() is false, the register-staged kernel and the full
(non-lean) combine run.

THE MATRIX (`CASES`).  PLAIN: M in {40, 261, 264, 512} x N in {36, 160, 200, 328} x K in {64, 192, 704}, concat (128, 192) and
(64, 64), all fifteen tile ids + AUTO, splitk in {1, 2, 3, 4, 8} on K = 704.  Thinning rule (pairwise over tile x shape x
splitk; both formats run for every case): tile t meets M[j], N[(j + t) mod 4], K[(j + t) mod 3] for j = 0..3 -- every tile
meets every M and every N, N = 36 included (v2 ids: refused with PP_ERR_BAD_ARG as v2_ok says) --, two split counts on
K = 704, one concat, one T variant, one R regime; the side outputs, all T variants through every epilogue (single pass,
lean / full / in-kernel combine), both R regimes and the activations on one tile per family (v1 / v2 lock-step / ping-pong).
out_dup_rows is a conv3x3 argument of the wrappers and runs as a conv case.  The folded LayerNorm (ln_stats / ln_colsum:
plain on every family, with a split -- the full combine --, GEGLU and V^T on the v2 families) and the group softmax
(PP_ACT_SOFTMAX80, with and without the folded LayerNorm, three masked logits) are R- cases in this layout; their gates are
norm_cases.folded_pre's error of the logits (moments given in fp32, `folded_ln_eps`) finished as norm_cases._finish does, and
for the softmax the terms of norm_cases' pp_xattn_block model: p (2^(2 D) - 1) for logits off by D, 88 2^-24 p for the 80
exponentials, v_exp and v_rcp, u p for the rounding, 2^-25 for fp16 subnormals.  gn_next_* (the consumer GroupNorm applied by
the split-K combine, tap-major and halo-tile) runs on probe E data: raw output and accumulators exact, the normalised output
-- dense by the ABI (ldo == N), so guarded by rows only, like the row moments -- bit for bit the pp_groupnorm_apply_acc launch
on them, which tests/test_norm_exact_gpu.py holds to its gate.
ceil(11 / 8) = 2 K tiles per slice leave slices 6 and 7 of the 8-split cases EMPTY (kt_begin >= kt_total): read off the
loops, an empty slice issues only zero-sized descriptors, runs no K step, keeps every barrier and vmcnt wait uniform (v1: one
__syncthreads and no loop; lock-step: NS - 1 dead issues, the drain; ping-pong: `tiles_left <= 0` -> dead descriptors, the
two group barriers) and stores a zero slab, which the combines add.  CONV: the shapes, channel pairs, tails, strides and
Cout of `CONV_*` below; split counts chosen so that slices start in x2 of a tap (C2 = 64 is one K tile: the restart
`k >= n1 -> second source` of the walks), at a tap boundary, inside the tail and
(halo-tile loop: its tail is split on its own) at x3|x4 -- `slice_start_kinds` computes them and the CPU file asserts each
occurs (on the tap-major walk x4 starts at K tile 9 ctiles + 2 = 11 or 29, both prime: no slice can start there).  The
halo-tile loop takes plain (tile AUTO, images >= 16 wide), `up` and the sub-pixel form; BM 128 by the library's choice, 256
with a forced split, 64 at the 4 x 16 image, which is added to the shapes for that.
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

import norm_cases as NC
import upconv_cases as UC

DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
U32 = 2.0 ** -24
POISON = 1000.0
LN_EPS = 1e-5
GUARD_ROWS, PAD_COLS = 64, 8
# PP_TILE_FORMS of gemm.hip: id -> (rows, ping-pong, v2)
TILES = {1: (128, False, False), 2: (64, False, False), 3: (256, False, False), 21: (128, False, True),
         31: (128, False, True), 22: (64, False, True), 32: (64, False, True), 42: (64, False, True),
         62: (64, False, True), 23: (256, False, True), 33: (256, False, True), 24: (128, False, True),
         53: (256, True, True), 44: (128, True, True), 54: (128, True, True)}
TILE_IDS = [0] + list(TILES)
PP_ERR_BAD_ARG, PP_ERR_UNSUPPORTED = -1, -2

DEFECTS = ("drop_last_k_tile_of_slice", "slice_restart_in_x2_reads_x1", "slice_restart_in_tail_reads_x3_for_x4",
           "tail_uses_tap_geometry", "ky_kx_swapped", "halo_crosses_batch_item", "stride2_odd_last_row_dropped",
           "up_rounds_half_up", "rows_past_M_written", "cols_past_N_written", "pad_columns_of_ldo_written",
           "n_major_tile_swap", "xcd_remap_drops_tile_when_grid_not_mult_of_8", "x2_offset_uses_ldx1", "res_uses_ldo",
           "rowvec_batch_from_tile_start", "res1_wrap_off_by_rows", "scale_after_residual", "bias_after_scale",
           "store_truncates", "acc_rounded_before_residual", "fp16_through_bf16", "combine_drops_last_slab",
           "vt_transposed_within_batch_only", "row_stats_count_pad_columns", "gn_acc_counts_rows_past_M",
           "subpix_parity_swapped")


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def _gen(*key) -> torch.Generator:
    seed = 0
    for x in key:
        seed = (seed * 1000003 + int(x) + 17) % (2 ** 31 - 1)
    return torch.Generator("cpu").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ cases
class Case(NamedTuple):
    kind: str                    # plain | conv | subpix
    probe: str                   # E | T:rne | T:res | T:bias | T:b256 | R+ | R-
    M: int = 0                   # plain
    N: int = 0                   # columns / Cout
    K1: int = 0                  # plain: K of x (conv: C1)
    K2: int = 0                  # plain: K of x2 (conv: C2)
    tile: int = 0
    splitk: int = 0
    epi: tuple = ()              # of: bias rowvec res1 res2 half (scale 0.5) silu geglu
    side: Optional[str] = None   # f32 | vt | dup | wrap | stats | gn | fuse | ld4
    B: int = 0                   # conv
    H: int = 0
    W: int = 0
    C3: int = 0
    C4: int = 0
    stride: int = 1
    up: bool = False
    expect: int = 0              # the error code the library must answer with (0: it runs)
    only: Optional[str] = None   # a case of one format only ("fp16")

    @property
    def id(self) -> str:
        if self.kind == "plain":
            s = f"plain-{self.probe}-M{self.M}-N{self.N}-K{self.K1}" + (f"+{self.K2}" if self.K2 else "")
        else:
            s = (f"{self.kind}-{self.probe}-{self.B}x{self.H}x{self.W}-c{self.K1}+{self.K2}-t{self.C3}+{self.C4}-n{self.N}"
                 + ("-s2" if self.stride == 2 else "") + ("-up" if self.up else ""))
        s += f"-t{self.tile}-sk{self.splitk}"
        if self.epi:
            s += "-" + "+".join(self.epi)
        return s + (f"-{self.side}" if self.side else "")

    # ---- geometry
    @property
    def hw_out(self):
        if self.kind == "subpix":
            return self.H, self.W                      # the request describes the SOURCE image
        hv, wv = (2 * self.H, 2 * self.W) if self.up else (self.H, self.W)
        return (hv - 1) // self.stride + 1, (wv - 1) // self.stride + 1

    @property
    def rows(self) -> int:                             # M of the request
        if self.kind == "plain":
            return self.M
        ho, wo = self.hw_out
        return self.B * ho * wo

    @property
    def K(self) -> int:
        if self.kind == "plain":
            return self.K1 + self.K2
        return (4 if self.kind == "subpix" else 9) * (self.K1 + self.K2) + self.C3 + self.C4

    @property
    def rows_per_batch(self) -> int:
        if self.kind != "plain":
            ho, wo = self.hw_out
            return ho * wo
        return 64 if (self.side in ("vt", "gn") or "rowvec" in self.epi or "softmax" in self.epi) else 0

    @property
    def halo(self) -> bool:
        """does the request run on the halo-tile loop (cg_raw_ok / cg_subpix_ok of conv_gn.hip)?"""
        if self.kind == "subpix":
            return True
        if self.kind != "conv" or self.tile != 0 or self.stride != 1 or self.side in ("ld4", "dup"):
            return False
        ho, wo = self.hw_out
        return wo >= 16 and wo % 8 == 0 and any(halo_shape_ok(self, bm) for bm in (256, 128, 64))

    @property
    def scale(self) -> float:
        return 0.5 if "half" in self.epi else (2.0 if self.probe == "T:bias" else 1.0)


def halo_shape_ok(c: Case, bm: int) -> bool:
    ho, wo = c.hw_out
    return bm % wo == 0 and (ho * wo) % bm == 0 and bm + 2 * wo <= 384       # cg_shape_ok (CG_HALO_PX = 384)


def halo_form(c: Case):
    """(bm, splitk) of a halo-tile launch: cg_choose / cg_choose_subpix of conv_gn.hip at these (small) shapes, where no
    tile count reaches the chip-filling thresholds."""
    tn = (c.N + 159) // 160
    ok = {bm: halo_shape_ok(c, bm) for bm in (256, 128, 64)}
    if c.kind == "subpix":
        want = {3: 256, 1: 128, 2: 64}.get(c.tile, 0)
        if want and ok[want]:
            return want, 1
        return (256 if ok[256] else 128 if ok[128] else 64), 1
    nch = (c.K1 + c.K2) // 64
    tiles = lambda bm: (c.rows // bm) * tn      # noqa: E731
    if ok[256] and ok[128] and tiles(256) * 4 <= 256 and nch <= 10 and c.splitk <= 0:
        bm = 128
    else:
        bm = 256 if ok[256] else 128 if ok[128] else 64
    sk = 1
    while tiles(bm) * sk * 2 <= 256 and nch // (sk * 2) >= 2 and sk < 8:
        sk *= 2
    sk = c.splitk if c.splitk > 0 else sk
    return bm, min(sk, 8, nch)


def launch_form(c: Case):
    """(family, bm, splitk, pp) the emulation walks: halo | v1 | v2.  AUTO on the tap-major / plain kernels: the result of
    an exact probe does not depend on the tile, so the emulation takes 64 x 160 x 3 stages and the forced split count."""
    if c.halo:
        bm, sk = halo_form(c)
        return "halo", bm, sk, True
    bm, pp, v2 = TILES[c.tile or 32]
    if c.side == "ld4" or c.N % 8:
        v2, bm, pp = False, TILES[c.tile if c.tile in (1, 2, 3) else 2][0], False
    sk = max(1, c.splitk)
    if c.N % 8 or c.side == "stats":
        sk = 1
    return ("v2" if v2 else "v1"), bm, sk, pp


def slice_start_kinds(c: Case):
    """Where the K slices s > 0 of a split launch begin: tap (a tap boundary) | in_x1 | in_x2 (in the second source of a tap)
    | tail (its first tile) | in_tail (inside x3) | x3x4 (the first tile of x4) | in_x4 | empty (no K tile left)."""
    fam, bm, sk, _ = launch_form(c)
    kinds = []
    if c.kind == "plain" or sk <= 1:
        return kinds
    c1, c2, c3, c4 = c.K1, c.K2, c.C3, c.C4
    if fam == "halo":                                   # chunks and tail tiles are split separately
        nch, nt = (c1 + c2) // 64, (c3 + c4) // 64
        for s in range(1, sk):
            ch = s * nch // sk * 64
            kinds.append("tap" if ch == 0 else "in_x2" if ch >= c1 else "in_x1")
            if nt:
                tk = s * nt // sk * 64
                kinds.append("tail" if tk == 0 else "x3x4" if tk == c3 else "in_x4" if tk > c3 else "in_tail")
        return kinds
    ct, total = (c1 + c2) // 64, c.K // 64
    per = -(-total // sk)
    for s in range(1, sk):
        kt = s * per
        if kt >= total:
            kinds.append("empty")
        elif kt < 9 * ct:
            cc = kt % ct * 64
            kinds.append("tap" if cc == 0 else "in_x2" if cc >= c1 else "in_x1")
        else:
            cc = (kt - 9 * ct) * 64
            kinds.append("tail" if cc == 0 else "x3x4" if cc == c3 else "in_x4" if cc > c3 else "in_tail")
    return kinds


PLAIN_M, PLAIN_N, PLAIN_K = (40, 261, 264, 512), (36, 160, 200, 328), (64, 192, 704)
SPLITS = (1, 2, 3, 4, 8)
EPIS = ((), ("bias",), ("res1",), ("bias", "rowvec", "res1", "res2", "half"), ("bias", "res2"), ("rowvec", "half"))
T_VARIANTS = ("T:rne", "T:res", "T:bias", "T:b256")
FAMILY_TILES = (1, 32, 54)                   # register-staged, v2 lock-step, ping-pong
CONV_SHAPES = ((3, 8, 8), (2, 16, 16), (2, 8, 24), (2, 24, 8), (1, 5, 7), (2, 9, 9), (2, 4, 16))
CONV_CH = ((64, 0), (192, 0), (128, 64))
CONV_TAILS = ((0, 0), (64, 0), (128, 64))
CONV_COUT = (160, 200, 328)
V2_TILES = [t for t in TILES if TILES[t][2]]


def _expect_plain(tile: int, N: int, side=None) -> int:
    """a v2 tile id on a tensor the 16-byte staged epilogue cannot address: pp_gemm_bf16 answers PP_ERR_BAD_ARG"""
    return PP_ERR_BAD_ARG if (tile and TILES[tile][2] and (N % 8 or side == "ld4")) else 0


def _plain_cases():
    out = []
    for t, tile in enumerate(TILE_IDS):
        for j in range(4):                                           # every tile meets every M and every N
            M, N, K = PLAIN_M[j], PLAIN_N[(j + t) % 4], PLAIN_K[(j + t) % 3]
            epi = EPIS[(t + j) % len(EPIS)]
            out.append(Case("plain", "E", M, N, K, 0, tile, 1, epi, expect=_expect_plain(tile, N)))
        for sk in (SPLITS[t % 5], SPLITS[(t + 2) % 5]):              # ragged slices; 8: slices of 2, 1 and 0 K tiles
            out.append(Case("plain", "E", PLAIN_M[(t + sk) % 4], PLAIN_N[1 + (t + sk) % 3], 704, 0, tile, sk,
                            EPIS[(t + sk) % len(EPIS)]))
        k1, k2 = ((128, 192), (64, 64))[t % 2]                        # concat: slices start at and inside x2
        out.append(Case("plain", "E", PLAIN_M[(t + 1) % 4], PLAIN_N[1 + t % 3], k1, k2, tile, (1, 2, 3)[t % 3], EPIS[t % 6]))
        v = T_VARIANTS[t % 4]
        out.append(Case("plain", v, 264, 200, 64, 0, tile, 1, only="fp16" if v == "T:b256" else None))
        full = ("bias", "rowvec", "res1", "res2", "half")                # every tile meets a random regime on ragged edges
        out.append(Case("plain", ("R+", "R-")[t % 2], 261, 200, 192, 0, tile, 1, () if t % 2 == 0 else full))
    for tile in FAMILY_TILES:
        v2 = TILES[tile][2]
        for v in T_VARIANTS:                                          # single pass, lean combine, in-kernel combine, full combine
            only = "fp16" if v == "T:b256" else None
            out.append(Case("plain", v, 261, 200, 64, 0, tile, 1, only=only))
            out.append(Case("plain", v, 264, 200, 128, 0, tile, 2, only=only))
            if tile == 54:
                out.append(Case("plain", v, 512, 320, 256, 0, tile, 2, side="fuse", only=only))
            if tile == 1:
                out.append(Case("plain", v, 264, 200, 128, 0, tile, 2, side="ld4", only=only))
                out.append(Case("plain", v, 40, 36, 64, 0, tile, 1, only=only))
        full = ("bias", "rowvec", "res1", "res2", "half")
        out.append(Case("plain", "E", 261, 200, 192, 0, tile, 1, ("bias",), side="f32"))
        out.append(Case("plain", "E", 264, 328, 704, 0, tile, 3, ("bias", "res1"), side="f32"))
        out.append(Case("plain", "E", 264, 200, 192, 0, tile, 1, full, side="ld4", expect=_expect_plain(tile, 200, "ld4")))
        out.append(Case("plain", "E", 264, 200, 704, 0, tile, 4, full, side="ld4", expect=_expect_plain(tile, 200, "ld4")))
        if v2:
            out.append(Case("plain", "E", 256, 480, 192, 0, tile, 1, ("bias", "half"), side="vt"))
            out.append(Case("plain", "E", 256, 200, 192, 0, tile, 1, ("bias", "res1", "half"), side="wrap"))
            out.append(Case("plain", "E", 256, 200, 704, 0, tile, 2, ("bias", "res1", "half"), side="wrap"))
            out.append(Case("plain", "E", 261, 328, 192, 0, tile, 1, ("bias", "res1"), side="stats"))
            out.append(Case("plain", "E", 192, 320, 192, 0, tile, 1, full, side="gn"))
            out.append(Case("plain", "E", 192, 320, 704, 0, tile, 2, full, side="gn"))
        for sk in (2, 4):
            if tile == 54:                                            # tiles % 8 == 0, M % 128 == 0: the in-kernel combine
                out.append(Case("plain", "E", 512, 320, 704, 0, tile, sk, full, side="fuse"))
        for probe in ("R+", "R-"):
            epi = () if probe == "R+" else ("bias", "rowvec", "res1", "res2", "half")
            out.append(Case("plain", probe, 261, 200, 704, 0, tile, 1, epi))
            out.append(Case("plain", probe, 512, 328, 704, 0, tile, 3, epi))
            out.append(Case("plain", probe, 40, 36, 192, 0, tile, 1, epi, expect=_expect_plain(tile, 36)))
        out.append(Case("plain", "R-", 264, 200, 192, 0, tile, 1, ("bias", "res1", "silu")))
        if v2:
            out.append(Case("plain", "R-", 264, 320, 192, 0, tile, 1, ("bias", "geglu")))
    # the folded LayerNorm (plain, + split, GEGLU, V^T) and the group softmax: R- only, gate terms of norm_cases
    for tile in FAMILY_TILES:
        out.append(Case("plain", "R-", 261, 200, 320, 0, tile, 1, ("ln", "bias")))
        out.append(Case("plain", "R-", 264, 328, 320, 0, tile, 2, ("ln", "bias")))
        if TILES[tile][2]:
            out.append(Case("plain", "R-", 261, 320, 320, 0, tile, 1, ("ln", "bias", "geglu")))
            out.append(Case("plain", "R-", 256, 480, 320, 0, tile, 1, ("ln", "bias"), side="vt"))
    out.append(Case("plain", "R-", 192, 240, 320, 0, 0, 1, ("ln", "bias", "softmax")))
    out.append(Case("plain", "R-", 128, 160, 192, 0, 0, 1, ("bias", "softmax")))
    for tile in (0, 62):
        out.append(Case("plain", "R+", 264, 200, 704, 0, tile, 1))
        out.append(Case("plain", "R-", 264, 200, 704, 0, tile, 2, ("bias", "rowvec", "res1", "res2", "half")))
    return out


def _conv_cases():
    out = []
    full = ("bias", "rowvec", "res1", "res2", "half")
    # tap-major: every v2 tile meets the conv walk, a tail and a split; shapes / channels / Cout rotate
    for t, tile in enumerate(V2_TILES):
        B, H, W = CONV_SHAPES[t % 4]
        c1, c2 = CONV_CH[t % 3]
        out.append(Case("conv", "E", 0, CONV_COUT[t % 3], c1, c2, tile, 1, EPIS[t % 6], B=B, H=H, W=W))
        B, H, W = CONV_SHAPES[(t + 1) % 4]
        c1, c2 = CONV_CH[(t + 2) % 3]
        c3, c4 = CONV_TAILS[1 + t % 2]
        out.append(Case("conv", "E", 0, CONV_COUT[(t + 1) % 3], c1, c2, tile, (2, 4, 8, 3)[t % 4], EPIS[(t + 3) % 6],
                        B=B, H=H, W=W, C3=c3, C4=c4))
    for tile in (1, 2, 3):                                            # the register-staged kernel: no tail
        B, H, W = CONV_SHAPES[tile]
        out.append(Case("conv", "E", 0, CONV_COUT[tile % 3], *CONV_CH[tile % 3], tile, tile, EPIS[tile], B=B, H=H, W=W))
        out.append(Case("conv", "E", 0, 160, 64, 0, tile, 1, ("bias",), B=2, H=8, W=8, C3=64, expect=PP_ERR_UNSUPPORTED))
    # slice starts inside x2, at a tap, inside the tail: (128, 64) + tail (128, 64) = 30 K tiles
    for tile, sk in ((54, 8), (32, 4), (53, 2), (44, 8)):
        out.append(Case("conv", "E", 0, 200, 128, 64, tile, sk, full, B=3, H=8, W=8, C3=128, C4=64))
    # stride 2 (odd sizes included) and nearest-2x `up` on the tap-major walk
    for t, (shape, tile) in enumerate((((1, 5, 7), 32), ((2, 9, 9), 54), ((3, 8, 8), 31), ((2, 24, 8), 1), ((2, 9, 9), 2))):
        B, H, W = shape
        out.append(Case("conv", "E", 0, CONV_COUT[t % 3], *CONV_CH[t % 3], tile, 1 + t % 2, EPIS[(t + 1) % 6], B=B, H=H, W=W,
                        stride=2))
    for t, (shape, tile) in enumerate((((1, 5, 7), 32), ((3, 8, 8), 54), ((2, 8, 24), 33), ((1, 5, 7), 2))):
        B, H, W = shape
        out.append(Case("conv", "E", 0, CONV_COUT[(t + 1) % 3], *CONV_CH[(t + 1) % 3], tile, 1 + t % 2, EPIS[(t + 2) % 6],
                        B=B, H=H, W=W, up=True))
    # the halo-tile loop (tile AUTO): plain BM 128 / 256 (forced split) / 64, tails, `up`, split over chunks and tail
    out.append(Case("conv", "E", 0, 200, 64, 0, 0, 0, ("bias", "res1"), B=2, H=16, W=16))
    out.append(Case("conv", "E", 0, 328, 128, 64, 0, 0, full, B=2, H=16, W=16))
    out.append(Case("conv", "E", 0, 160, 128, 64, 0, 3, full, B=2, H=16, W=16, C3=128, C4=64))
    out.append(Case("conv", "E", 0, 200, 192, 0, 0, 2, ("bias",), B=2, H=16, W=16, C3=64))
    out.append(Case("conv", "E", 0, 160, 192, 0, 0, 0, ("res2",), B=2, H=4, W=16))
    out.append(Case("conv", "E", 0, 200, 128, 64, 0, 2, full, B=2, H=4, W=16))
    out.append(Case("conv", "E", 0, 200, 128, 64, 0, 0, full, B=3, H=8, W=8, up=True))
    out.append(Case("conv", "E", 0, 160, 192, 0, 0, 3, ("bias",), B=3, H=8, W=8, up=True))
    out.append(Case("conv", "E", 0, 320, 128, 64, 0, 0, full, B=2, H=16, W=16, side="gn"))
    out.append(Case("conv", "E", 0, 320, 128, 64, 0, 2, full, B=2, H=16, W=16, side="gn"))
    out.append(Case("conv", "E", 0, 320, 128, 64, 54, 2, full, B=3, H=8, W=8, side="gn"))
    out.append(Case("conv", "E", 0, 320, 192, 0, 54, 2, full, B=4, H=16, W=16, side="fuse"))
    out.append(Case("conv", "E", 0, 320, 128, 64, 54, 2, full, B=3, H=8, W=8, side="gnnext"))     # the combine applies the next norm
    out.append(Case("conv", "E", 0, 320, 192, 0, 0, 2, ("bias", "res1"), B=2, H=16, W=16, side="gnnext"))   # halo-tile loop
    for tile in (32, 54, 0):                                          # out_dup_rows: the single-pass staged epilogue
        out.append(Case("conv", "E", 0, 328, 64, 0, tile, 1, ("bias", "res1"), B=3, H=8, W=8, side="dup"))
    for tile in (3, 1, 2, 0):                                         # the sub-pixel form: BM 256 / 128 / 64 / its choice
        B, H, W = (3, 8, 8) if tile == 2 else (2, 16, 16)
        out.append(Case("subpix", "E", 0, CONV_COUT[tile % 3], 64 if tile else 192, 0, tile, 1,
                        EPIS[(3, 1, 4, 0)[tile % 4]], B=B, H=H, W=W))
    # T through the tap-major and the halo-tile epilogues (the three K columns sit in the centre tap), R in both regimes
    for v in T_VARIANTS:
        only = "fp16" if v == "T:b256" else None
        out.append(Case("conv", v, 0, 200, 64, 0, 0, 0, B=2, H=16, W=16, only=only))
        out.append(Case("conv", v, 0, 200, 64, 0, 0, 3, B=2, H=16, W=16, C3=128, C4=64, only=only))
        out.append(Case("conv", v, 0, 200, 64, 0, 54, 1, B=3, H=8, W=8, only=only))
    for probe in ("R+", "R-"):
        epi = () if probe == "R+" else full
        out.append(Case("conv", probe, 0, 200, 128, 64, 0, 0, epi, B=2, H=16, W=16))
        out.append(Case("conv", probe, 0, 328, 192, 0, 54, 2, epi, B=2, H=9, W=9, stride=2))
        out.append(Case("conv", probe, 0, 160, 128, 64, 32, 4, epi, B=3, H=8, W=8, C3=128, C4=64))
    return out


CASES = _plain_cases() + _conv_cases()
assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"


def case_dtypes(c: Case):
    return [(d, f) for d, f in DTYPES if c.only in (None, f)]


# ------------------------------------------------------------------------------------------------ memory
class Buf:
    """A [rows, cols] window of a flat buffer: element (r, c) at base + r * ld + c."""

    def __init__(self, full, base, rows, cols, ld):
        self.full, self.base, self.rows, self.cols, self.ld = full, base, rows, cols, ld

    @property
    def view(self) -> torch.Tensor:
        return self.full.as_strided((self.rows, self.cols), (self.ld, 1), self.base)

    def to(self, dev):
        return Buf(self.full.to(dev), self.base, self.rows, self.cols, self.ld)

    def outside(self) -> torch.Tensor:
        """mask over the flat buffer: True where the element does not belong to the window"""
        m = torch.ones(self.full.numel(), dtype=torch.bool, device=self.full.device)
        m.as_strided((self.rows, self.cols), (self.ld, 1), self.base).fill_(False)
        return m


def lay(data: torch.Tensor, pad: int, front: int, back: int, fill: float) -> Buf:
    """`data` [rows, cols] as a window with ld = cols + pad, `front` / `back` rows of `fill` around it, pads filled too."""
    rows, cols = data.shape
    ld = cols + pad
    full = torch.full(((front + rows + back) * ld,), fill, dtype=data.dtype)
    b = Buf(full, front * ld, rows, cols, ld)
    b.view.copy_(data)
    return b


SENTINEL16, SENTINEL32 = 0x5A5A, 0x5A5A5A5A


def sentinel_out(rows: int, cols: int, pad: int, dtype, guard: int = GUARD_ROWS) -> Buf:
    """an output window in a sentinel-filled buffer (bit pattern 0x5A5A..., finite in every format)"""
    ld = cols + pad
    n = (rows + 2 * guard) * ld
    if dtype == torch.float64:                         # (the emulation's buffers: NaN marks what was never stored)
        full = torch.full((n,), math.nan, dtype=dtype)
    elif dtype in (torch.float32, torch.int32):
        full = torch.full((n,), SENTINEL32, dtype=torch.int32).view(dtype)
    else:
        full = torch.full((n,), SENTINEL16, dtype=torch.int16).view(dtype)
    return Buf(full, guard * ld, rows, cols, ld)


# ------------------------------------------------------------------------------------------------ data
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _x_exact(g, M, K):
    p = min(0.5, 256.0 / K)
    x = (torch.rand(M, K, generator=g) < p).double() * (torch.randint(0, 2, (M, K), generator=g).double() * 2 - 1)
    return _ensure_blocks(x)


def _ensure_blocks(x):
    """no 64-row x 64-deep block may be invisible"""
    for i in range(0, x.shape[0], 64):
        for j in range(0, x.shape[1], 64):
            if not bool(x[i:i + 64, j:j + 64].any()):
                x[i, j] = 1.0
    return x


def build(c: Case, dtype, device="cpu"):
    """The tensors of a case in the layout of `Setup` (drawn on the CPU, in `dtype`, then moved to `device`) and the fp64
    reference, computed on `device`.  -> dict."""
    g = _gen(*[ord(ch) for ch in c.id[:48]], len(c.id))
    M, N, K = c.rows, c.N, c.K
    conv = c.kind != "plain"
    Mo = M * (4 if c.kind == "subpix" else 1)          # rows of the output tensor (res1 / res2 have its shape)
    ctot = c.K1 + c.K2
    t = {"case": c, "dtype": dtype}
    kx = (9 * ctot + c.C3 + c.C4) if c.kind == "subpix" else K         # the sub-pixel request is built from the 9-tap weights
    # ---- operands as real numbers (fp64), logical shapes: sources [rows_of_source, channels], w [N, kx]
    if conv:
        npx = c.B * c.H * c.W
        src_rows = {"x1": npx, "x2": npx, "x3": M, "x4": M}
    chans = {"x1": c.K1, "x2": c.K2, "x3": c.C3, "x4": c.C4}
    names = [n for n in ("x1", "x2", "x3", "x4") if chans[n]]
    if c.probe == "E":
        xs = {n: _x_exact(g, src_rows[n] if conv else M, chans[n]) for n in names}
        if conv:                                       # density by the K of the whole contraction
            p = min(0.5, 256.0 / K)
            for n in names:
                keep = (torch.rand(xs[n].shape, generator=g) < p / min(0.5, 256.0 / chans[n])).double()
                xs[n] = _ensure_blocks(xs[n] * keep)
        w = (torch.randint(1, 3, (N, kx), generator=g) * (torch.randint(0, 2, (N, kx), generator=g) * 2 - 1)).double()
    elif c.probe.startswith("T"):
        base = 256.0 if (dtype == torch.bfloat16 or c.probe == "T:b256") else 2048.0
        if c.probe == "T:bias":
            base /= 2
        xs = {n: torch.zeros(src_rows[n] if conv else M, chans[n], dtype=torch.float64) for n in names}
        w = torch.zeros(N, kx, dtype=torch.float64)
        k0 = 4 * ctot if conv else 0                   # conv: the centre tap, so that acc depends on the output pixel only
        rows = torch.arange(xs["x1"].shape[0], dtype=torch.float64)
        xs["x1"][:, 0], xs["x1"][:, 1], xs["x1"][:, 2] = base / 2, rows % 16, 1.0
        w[:, k0], w[:, k0 + 1], w[:, k0 + 2] = 2.0, 1.0, torch.arange(N, dtype=torch.float64) % 16
    else:
        if c.probe == "R+":
            xs = {n: (torch.rand(src_rows[n] if conv else M, chans[n], generator=g) * 0.5 + 0.5) for n in names}
            w = (torch.rand(N, kx, generator=g) * 0.5 + 0.5) * 2.0 ** -math.ceil(math.log2(K))
        else:
            xs = {n: torch.randn(src_rows[n] if conv else M, chans[n], generator=g) for n in names}
            w = torch.randn(N, kx, generator=g) * K ** -0.5
        xs = {n: v.to(dtype).double() for n, v in xs.items()}
        w = w.to(dtype).double()
    exact = not c.probe.startswith("R")
    rnd = (lambda *s: _ints(g, s, -8, 8)) if exact else (lambda *s: torch.randn(*s, generator=g))
    rpb = c.rows_per_batch
    nb = -(-M // rpb) if rpb else 1
    wrap = 128 if c.side == "wrap" else 0
    e = {"bias": None, "rowvec": None, "res1": None, "res2": None}
    if "bias" in c.epi:
        e["bias"] = rnd(N).float().double()
    if c.probe == "T:bias":
        e["bias"] = torch.full((N,), 0.5, dtype=torch.float64)
    if "rowvec" in c.epi:
        e["rowvec"] = rnd(nb, N).float().double()
    if "res1" in c.epi:
        e["res1"] = rnd(wrap or Mo, N).to(dtype).double()
    if c.probe == "T:res":                             # odd sums become even: exactly representable
        odd = ((torch.arange(M)[:, None] % 16 + torch.arange(N)[None, :] % 16) % 2 == 1).double()
        e["res1"] = odd * torch.where(torch.arange(M)[:, None] % 2 == 0, 1.0, -1.0)
    if "res2" in c.epi:
        e["res2"] = rnd(Mo, N).to(dtype).double()
    # ---- layout
    pad = 4 if c.side == "ld4" else PAD_COLS
    for n in names:
        t[n] = lay(xs[n].to(dtype), 0 if conv else PAD_COLS, GUARD_ROWS if conv else 0, GUARD_ROWS, POISON)
    t["w9"] = w.to(dtype) if c.kind == "subpix" else None
    wk = UC.fold(w.float()).double() if c.kind == "subpix" else w      # [4, N, 4 C] folded, exact for the E probe
    t["w"] = torch.cat([wk.reshape(-1, wk.shape[-1]), torch.full((8, wk.shape[-1]), POISON, dtype=torch.float64)]).to(dtype)
    t["bias"] = torch.cat([e["bias"], torch.full((8,), POISON, dtype=torch.float64)]).float() if e["bias"] is not None else None
    t["rowvec"] = e["rowvec"].float() if e["rowvec"] is not None else None
    t["res1"] = lay(e["res1"].to(dtype), pad, 0, GUARD_ROWS, POISON) if e["res1"] is not None else None
    t["res2"] = lay(e["res2"].to(dtype), pad + 8, 0, GUARD_ROWS, POISON) if e["res2"] is not None else None
    t["wrap"], t["nb"] = wrap, nb
    if "softmax" in c.epi:                             # a masked logit: the last three columns of the last group
        t["bias"][N - 3:N] = -math.inf
    if "ln" in c.epi:                                  # w is gamma (.) W rounded; moments rounded once from the exact tile sums
        S, Q, _ = NC.row_tile_sums(xs["x1"])
        t["ln_stats"] = torch.stack([S, Q], -1).float().contiguous()
        t["ln_colsum"] = torch.cat([w.sum(1), torch.full((8,), POISON, dtype=torch.float64)]).float()
    for k_, v_ in t.items():
        if isinstance(v_, (Buf, torch.Tensor)):
            t[k_] = v_.to(device)
    # ---- the reference (fp64): the op as torch states it, the epilogue in the order of the header
    wd = t["w9"].double() if c.kind == "subpix" else t["w"][:wk.reshape(-1, wk.shape[-1]).shape[0]].double()
    if conv:
        acc, A = _conv_ref(c, {n: t[n].view.double() for n in names}, wd)
    else:
        X = torch.cat([t[n].view.double() for n in names], 1)
        acc, A = X @ wd.T, X.abs() @ wd.abs().T
        if "ln" in c.epi:                              # acc := LN(x) w'^T with its error terms (norm_cases.folded_pre)
            tiles = K // 160
            tb = t["bias"][:N].double()
            acc, dz = NC.folded_pre(X, wd, t["ln_colsum"][:N], torch.zeros(N, device=device), LN_EPS, NC.folded_ln_eps(tiles))
            t["d_pre"] = dz + 3 * U32 * torch.where(torch.isfinite(tb), tb.abs(), torch.zeros_like(tb))
    op = {k: (t[k].view.double() if isinstance(t[k], Buf) else (t[k][:N].double() if k == "bias" else t[k].double()))
          if t[k] is not None else None for k in e}
    t["ref"], t["A"], t["pre"] = epilogue64(c, acc, A, op, wrap)
    t["acc"] = acc
    if exact:
        _assert_exact(c, t, dtype)
    return t


def _conv_ref(c: Case, xs, w):
    """conv3x3 (padding 1) in fp64 over concat(x1, x2) -- after a nearest 2x upsample (repeat_interleave) for `up` and the
    sub-pixel request -- as nine shifted slices of the zero-padded image times the weight's (ky, kx, c) columns, + the 1x1
    tail at the output pixel; -> (acc [M, N], A = the same over absolute values).  Plain slicing and one matmul: no index
    arithmetic shared with the emulation, and nothing a device lacks in fp64."""
    ctot = c.K1 + c.K2
    up = c.up or c.kind == "subpix"
    s_ = c.stride

    def run(xm, wm):
        x = torch.cat([xm[n] for n in ("x1", "x2") if n in xm], 1).reshape(c.B, c.H, c.W, ctot)
        if up:
            x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
        hv, wv = x.shape[1], x.shape[2]
        ho, wo = (hv - 1) // s_ + 1, (wv - 1) // s_ + 1
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        cols = [xp[:, ky:ky + s_ * (ho - 1) + 1:s_, kx:kx + s_ * (wo - 1) + 1:s_, :] for ky in range(3) for kx in range(3)]
        X = torch.cat(cols, 3).reshape(c.B * ho * wo, 9 * ctot)
        if c.C3:
            X = torch.cat([X] + [xm[n] for n in ("x3", "x4") if n in xm], 1)
        return X @ wm.T
    return run(xs, w), run({n: v.abs() for n, v in xs.items()}, w.abs())


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def epilogue64(c: Case, acc, A, op, wrap: int = 0):
    """(acc + bias + rowvec) * scale + res1 + res2, the activation; -> (ref, A, the value in front of the activation) in fp64,
    BEFORE the one rounding.
    Rows follow the request's row order; for the sub-pixel request that is the OUTPUT tensor's (the reference computes the
    up-conv directly)."""
    M = acc.shape[0]
    v, a = acc.clone(), A.clone()
    if op["bias"] is not None:
        v, a = v + op["bias"], a + op["bias"].abs()
    if op["rowvec"] is not None:
        rpb = c.rows_per_batch * (4 if c.kind == "subpix" else 1)
        idx = torch.arange(M, device=acc.device) // rpb
        v, a = v + op["rowvec"][idx], a + op["rowvec"][idx].abs()
    v, a = v * c.scale, a * abs(c.scale)
    if op["res1"] is not None:
        r = op["res1"][torch.arange(M, device=acc.device) % wrap] if wrap else op["res1"]
        v, a = v + r, a + r.abs()
    if op["res2"] is not None:
        v, a = v + op["res2"], a + op["res2"].abs()
    pre = v
    if "softmax" in c.epi:                             # per group of 80 columns, in the exp2 domain
        q = v.reshape(M, -1, 80)
        v = torch.softmax(q * math.log(2.0), -1).reshape(M, -1)
    if "silu" in c.epi:
        v = v * torch.sigmoid(v)
    if "geglu" in c.epi:
        q = v.reshape(M, -1, 4)
        v = (q[:, :, :2] * gelu64(q[:, :, 2:])).reshape(M, -1)
    return v, a, pre


def _assert_exact(c: Case, t, dtype):
    """the preconditions of probes E and T, from the reference"""
    assert float(t["A"].max()) < 2.0 ** 24, (c.id, "sum |x||w| must stay below 2^24")
    ref = t["ref"]
    odt = torch.float32 if c.side == "f32" else dtype
    if c.probe in ("E", "T:res", "T:b256"):
        assert bool((ref.to(odt).double() == ref).all()), (c.id, "every expected value must be representable", float(ref.abs().max()))
    if c.probe == "E":
        assert float(ref.abs().max()) <= 256.0 and gn_partials_exact(ref), c.id


def gn_partials_exact(ref) -> bool:
    """every fp32 partial an epilogue forms for the GroupNorm accumulators / row moments is an integer multiple of 1/4 below
    2^24: <= 256 rows (160 columns) of |v| <= 256 in steps of 1/2"""
    return 256.0 * float((ref * ref).max()) < 2.0 ** 24


def expected_out(c: Case, t, dtype) -> torch.Tensor:
    """the reference cast ONCE to the output format"""
    return t["ref"].to(torch.float32 if c.side == "f32" else dtype)


def n_roundings(c: Case) -> int:
    _, _, sk, _ = launch_form(c)
    return c.K + sk + 5


def gate(c: Case, t, dtype) -> torch.Tensor:
    """u |ref| + n_r 2^-24 A (+ the activation's terms); fp64 [M, n_out]"""
    u = 0.0 if c.side == "f32" else unit_roundoff(dtype)
    d = t["d_pre"] if "ln" in c.epi else n_roundings(c) * U32 * t["A"]
    ref = t["ref"]
    pre = t["pre"]
    if "silu" in c.epi:                                # norm_cases, "SiLU": slope <= 1.1; exp, the division, the argument
        d = 1.1 * d + (7 + pre.abs()) * U32 * ref.abs()
    if "geglu" in c.epi:                               # norm_cases, "GEGLU": |gelu'| <= 1.13, gelu_fast_f within 2^-20 |g|
        q, dq = pre.reshape(pre.shape[0], -1, 4), d.reshape(d.shape[0], -1, 4)
        a_, g_, da, dg = q[:, :, :2], q[:, :, 2:], dq[:, :, :2], dq[:, :, 2:]
        d = (da * gelu64(g_).abs() + (a_.abs() + da) * (1.13 * dg + 2.0 ** -20 * g_.abs())).reshape(ref.shape) \
            + 2 * U32 * ref.abs()
    if "softmax" in c.epi:                             # norm_cases, pp_xattn_block: logits off by D move p by p (2^(2 D) - 1);
        D = d.reshape(d.shape[0], -1, 80).max(-1, keepdim=True).values.expand(-1, -1, 80).reshape(d.shape)
        return u * ref + ref * (torch.exp2(2 * D) - 1) + 88 * U32 * ref + 2.0 ** -25     # 80 exponentials, v_exp, v_rcp: 88
    if "ln" in c.epi:                                  # norm_cases._finish: the propagated terms are themselves rounded
        return u * ref.abs() + (1 + u) * d + (2.0 ** -25 if dtype == torch.float16 else 0.0)
    return u * ref.abs() + d


def worst_ratio(out, expected, g) -> float:
    err = (out.double() - expected).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    r = torch.where(g > 0, err / g.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def gate_rpm(ref, A, K: int, splits: int, dtype) -> torch.Tensor:
    """the R gate for a test that holds (ref, A) itself: u |ref| + (K + splits + 5) 2^-24 A"""
    u = unit_roundoff(dtype)
    return u * ref.abs() + (K + max(1, splits) + 5) * U32 * A


# ------------------------------------------------------------------------------------------------ side outputs (exact)
def expected_sides(c: Case, t, dtype):
    """what the side outputs of an E case must hold, from the reference: dict name -> tensor"""
    M, N = c.rows, c.N
    stored = expected_out(c, t, dtype).double()
    s = {}
    if c.side == "stats":                              # per-row (sum, sumsq) of the stored values per 160-column tile
        tn = (N + 159) // 160
        st = torch.zeros(M, tn, 2, dtype=torch.float64, device=stored.device)
        for j in range(tn):
            blk = stored[:, j * 160:(j + 1) * 160]
            st[:, j, 0], st[:, j, 1] = blk.sum(1), (blk * blk).sum(1)
        s["stats"] = st.float()
    if c.side in ("gn", "gnnext"):                                 # two subscriptions: groups of 10 from channel 0, of 40 from channel 40
        s["gn"] = [gn_expected(stored, c.rows_per_batch, cg, c0, groups) for cg, c0, groups in gn_subs(c)]
    return s


def gn_subs(c: Case):
    return [(10, 0, c.N // 10), (40, 40, c.N // 40 + 1)]


def gn_expected(stored, rpb: int, cg: int, c0: int, groups: int) -> torch.Tensor:
    M, N = stored.shape
    nb = M // rpb
    acc = torch.zeros(nb, groups, 2, dtype=torch.int64, device=stored.device)
    grp = (torch.arange(N, device=stored.device) + c0) // cg
    v = stored.reshape(nb, rpb, N)
    for gi in range(groups):
        sel = v[:, :, grp == gi]
        acc[:, gi, 0] = (sel.sum((1, 2)) * 2.0 ** 24).round().long()
        acc[:, gi, 1] = ((sel * sel).sum((1, 2)) * 2.0 ** 20).round().long()
    return acc


# ------------------------------------------------------------------------------------------------ the emulation
def _rd(b: Buf, full64, r, cidx, ld=None):
    """flat read of rows r [n] x columns cidx [k] of a window (whatever lies there: pads, poison rows), fp64 [n, k]"""
    addr = b.base + r[:, None] * (ld or b.ld) + cidx[None, :]
    return full64[addr.clamp(0, full64.numel() - 1)]


def _round16(v, dtype, defect):
    """the one rounding of the epilogue (fp64 -> the 16-bit format, as fp64)"""
    v32 = v.float()
    if defect == "fp16_through_bf16" and dtype == torch.float16:
        v32 = v32.to(torch.bfloat16).float()
    if defect == "store_truncates":
        r = v32.to(dtype)
        over = r.float().abs() > v32.abs()
        bits = r.view(torch.int16) - over.to(torch.int16)              # one step towards zero
        return bits.view(dtype).double()
    return v32.to(dtype).double()


def tile_walk_emulate(c: Case, t, dtype, defect=None):
    """What the kernels do, structurally, on the flat buffers of `t` (fp64 accumulation: the probes are exact):
    BM x 160 tiles under the XCD remap in either tile order; the K walk in 64-deep tiles -- tap-major over (x1, x2), then the
    1x1 tail over (x3, x4); chunk-major with all taps per chunk on the halo-tile loop --; split-K slices, their slabs and the
    combine; the conv geometry for stride / up / the four sub-pixel parities; the epilogue in the header's order with one
    round-to-nearest-even; stores through (ldo, vt_ld) into sentinel (NaN) buffers.  `defect`: one of DEFECTS.
    -> dict: out (Buf, fp64, NaN outside what was written), vt, stats, gn."""
    assert defect is None or defect in DEFECTS
    fam, bm, sk, _ = launch_form(c)
    M, N, K = c.rows, c.N, c.K
    conv, subpix = c.kind != "plain", c.kind == "subpix"
    f64 = {n: t[n].full.double() for n in ("x1", "x2", "x3", "x4", "res1", "res2") if t.get(n) is not None}
    wrows = t["w"].shape[0] - 8
    w64 = t["w"].double()
    ho, wo = c.hw_out
    ctot, ct = c.K1 + c.K2, (c.K1 + c.K2) // 64
    ntaps = 4 if subpix else 9
    f32o = c.side == "f32"
    n_out = N // 2 if "geglu" in c.epi else (160 if c.side == "vt" else N)
    orows = M * (4 if subpix else 1) * (2 if c.side == "dup" else 1)
    pad = 4 if c.side == "ld4" else 0 if c.side == "gnnext" else PAD_COLS
    out = sentinel_out(orows, n_out, pad, torch.float64)
    out.full.fill_(math.nan)
    res = {"out": out}
    rpb = c.rows_per_batch
    if c.side == "vt":
        res["vt"] = vt = sentinel_out(t["nb"] * (N - 160), rpb, PAD_COLS, torch.float64)
        vt.full.fill_(math.nan)
    tn = (N + 159) // 160
    stats = torch.zeros(M, tn, 2, dtype=torch.float64) if c.side == "stats" else None
    gn = [torch.zeros(t["nb"], g, 2, dtype=torch.float64) for _, _, g in gn_subs(c)] if c.side in ("gn", "gnnext") else None
    tiles_m = M // bm if fam == "halo" else -(-M // bm)
    n_major = tiles_m < tn and tiles_m <= 8
    grid = tiles_m * tn
    ar64 = torch.arange(64)

    def pixel(m):                                       # request row -> (image, oy, ox)
        b = m // (ho * wo)
        rem = m - b * ho * wo
        return b, rem // wo, rem % wo

    def gather(m, valid, src, tap, cc, par=(0, 0)):
        """the [bm, 64] X tile of rows m: source tensor `src` at channel offset cc (inside the source), tap geometry"""
        b_ = t[src]
        if not conv:
            ld = t["x1"].ld if (src == "x2" and defect == "x2_offset_uses_ldx1") else b_.ld
            return torch.where(valid[:, None], _rd(b_, f64[src], m, cc + ar64, ld), 0.0)
        bi, oy, ox = pixel(m)
        if src in ("x3", "x4") and tap is None:        # the 1x1 tail: the output pixel itself
            return torch.where(valid[:, None], _rd(b_, f64[src], m, cc + ar64), 0.0)
        if subpix:
            dy, dx = divmod(tap, 2)
            iy, ix = oy + par[0] - 1 + dy, ox + par[1] - 1 + dx
            hv, wv = c.H, c.W
            sy, sx = iy, ix
        else:
            ky, kx = divmod(tap, 3)
            if defect == "ky_kx_swapped":
                ky, kx = kx, ky
            iy, ix = oy * c.stride - 1 + ky, ox * c.stride - 1 + kx
            hv, wv = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
            if defect == "up_rounds_half_up" and c.up:
                sy, sx = ((iy + 1) >> 1).clamp(max=c.H - 1), ((ix + 1) >> 1).clamp(max=c.W - 1)
            else:
                sy, sx = (iy >> 1, ix >> 1) if c.up else (iy, ix)
        hlim = hv - 1 if (defect == "stride2_odd_last_row_dropped" and c.stride == 2 and c.H % 2) else hv
        ok = valid & (ix >= 0) & (ix < wv)
        if defect != "halo_crosses_batch_item":
            ok = ok & (iy >= 0) & (iy < hlim)
        elif hlim != hv:
            ok = ok & (iy < hlim)
        px = (bi * c.H + sy) * c.W + sx
        return torch.where(ok[:, None], _rd(b_, f64[src], px, cc + ar64), 0.0)

    def k_steps(split):
        """the K tiles of one slice as (weight column k0, source, tap | None, channel offset inside the source)"""
        steps = []

        def src_of(cc, tail):
            a_, b2, ca = ("x3", "x4", c.C3) if tail else ("x1", "x2", c.K1)
            return (a_, cc) if cc < ca else (b2, cc - ca)
        if fam == "halo":
            nch, nt = ct, (c.C3 + c.C4) // 64
            for ch in range(split * nch // sk, (split + 1) * nch // sk):
                for tap in range(ntaps):
                    s_, off = src_of(ch * 64, False)
                    steps.append((tap * ctot + ch * 64, s_, tap, off))
            for tk in range(split * nt // sk, (split + 1) * nt // sk):
                s_, off = src_of(tk * 64, True)
                steps.append((ntaps * ctot + tk * 64, s_, None, off))
        else:
            total = K // 64
            per = -(-total // sk)
            kb, ke = split * per, min(total, (split + 1) * per)
            for kt in range(kb, ke):
                if not conv:
                    s_, off = src_of(kt * 64, False)
                    steps.append((kt * 64, s_, None, off))
                elif kt < 9 * ct:
                    s_, off = src_of(kt % ct * 64, False)
                    steps.append((kt * 64, s_, kt // ct, off))
                else:
                    s_, off = src_of((kt - 9 * ct) * 64, True)
                    steps.append((kt * 64, s_, None, off))
        # ---- defects of the walk
        if defect == "drop_last_k_tile_of_slice" and sk > 1 and steps:
            steps = steps[:-1]
        if split > 0 and steps and defect in ("slice_restart_in_x2_reads_x1", "slice_restart_in_tail_reads_x3_for_x4"):
            want, repl = ("x2", "x1") if defect == "slice_restart_in_x2_reads_x1" else ("x4", "x3")
            starts = [0]                               # where the walk (re)positions itself: the slice's first K tile, and on
            if fam == "halo":                          # the halo-tile loop the first tail tile (split on its own) as well
                starts += [i for i, st_ in enumerate(steps) if st_[2] is None and st_[1] in ("x3", "x4")][:1]
            for i0 in starts:                          # the restart forgets the second source until the segment ends
                i = i0
                while i < len(steps) and steps[i][1] == want and steps[i][2] == steps[i0][2]:
                    k0, _, tap, off = steps[i]
                    steps[i] = (k0, repl, tap, off % max(64, t[repl].cols))
                    i += 1
        if defect == "tail_uses_tap_geometry":
            steps = [(k0, s_, 0 if (tap is None and s_ in ("x3", "x4")) else tap, off) for k0, s_, tap, off in steps]
        return steps

    def tail_gather(m, valid, s_, tap, off, par):
        if s_ in ("x3", "x4") and tap is not None:      # (defect) the tail read with the geometry of tap 0
            bi, oy, ox = pixel(m)
            ok = valid & (oy >= 1) & (ox >= 1)
            return torch.where(ok[:, None], _rd(t[s_], f64[s_], m - wo - 1, off + ar64), 0.0)
        return gather(m, valid, s_, tap, off, par)

    npar = 4 if subpix else 1
    slabs = torch.zeros(sk, M * npar, N, dtype=torch.float64) if sk > 1 else None

    def out_row(m, par):                                # the row of `out` request row m is stored at
        if not subpix:
            return m
        a_, b2 = (par[1], par[0]) if defect == "subpix_parity_swapped" else par
        bi, oy, ox = pixel(m)
        return (bi * 2 * c.H + 2 * oy + a_) * 2 * c.W + 2 * ox + b2

    def epilogue(m, n, acc, single_pass, par=(0, 0), m_blk=0):
        """rows m [r] x columns n [k] (tile-shaped in a single pass; all valid elements behind a combine)"""
        vm, vn = m < M, n < N
        orow = out_row(m, par)
        v = acc.clone()
        bias = torch.zeros(len(n), dtype=torch.float64)
        if t["bias"] is not None:
            bias = t["bias"].double()[n.clamp(max=t["bias"].numel() - 1)]
        rv = torch.zeros_like(v)
        if t["rowvec"] is not None:
            bidx = (torch.full_like(m, m_blk) if (defect == "rowvec_batch_from_tile_start" and single_pass) else m) // rpb
            rv = t["rowvec"].double()[bidx.clamp(max=t["nb"] - 1)][:, n.clamp(max=N - 1)]
        r12 = torch.zeros_like(v)
        for name in ("res1", "res2"):
            if t[name] is not None:
                rr = orow.clone()
                if name == "res1" and t["wrap"]:
                    lim = t["wrap"] + (1 if defect == "res1_wrap_off_by_rows" else 0)
                    rr = torch.where(rr >= lim, rr - t["wrap"], rr)
                ld = out.ld if defect == "res_uses_ldo" else None
                r12 = r12 + _rd(t[name], f64[name], rr, n, ld)
        if "ln" in c.epi:                              # the folded-LayerNorm correction, from the row moments
            st_ = t["ln_stats"].double()[m.clamp(max=M - 1)]
            mean = st_[:, :, 0].sum(1) / K
            rstd = 1.0 / torch.sqrt((st_[:, :, 1].sum(1) / K - mean * mean).clamp_min(0.0) + LN_EPS)
            cs_ = t["ln_colsum"].double()[n.clamp(max=t["ln_colsum"].numel() - 1)]
            v = (v - cs_[None, :] * mean[:, None]) * rstd[:, None]
        if defect == "acc_rounded_before_residual":
            v = _round16(v, dtype, None)
        if defect == "bias_after_scale":
            v = v * c.scale + bias + rv + r12
        elif defect == "scale_after_residual":
            v = (v + bias + rv + r12) * c.scale
        else:
            v = (v + bias + rv) * c.scale + r12
        if "softmax" in c.epi:
            v = torch.softmax(v.reshape(len(m), -1, 80) * math.log(2.0), -1).reshape(len(m), -1)
        if "silu" in c.epi:
            v = v * torch.sigmoid(v)
        cols = n
        if "geglu" in c.epi:
            q = v.reshape(len(m), -1, 4)
            v = (q[:, :, :2] * gelu64(q[:, :, 2:])).reshape(len(m), -1)
            cols = (n.reshape(-1, 4)[:, :1] // 2 + torch.arange(2)[None, :]).reshape(-1)     # out[m][n / 2 + j]
            vn = vn.reshape(-1, 4)[:, :2].reshape(-1)
        st = v if f32o else _round16(v, dtype, defect)
        # ---- stores
        wm = vm | (defect == "rows_past_M_written" and single_pass)
        wn = vn.clone()
        if single_pass and defect == "cols_past_N_written":
            wn = torch.ones_like(vn)
        if single_pass and defect == "pad_columns_of_ldo_written":
            wn = wn | (cols < out.ld)
        if c.side == "vt":
            isvt = cols >= 160
            bidx, rin = m // rpb, m % rpb
            if defect == "vt_transposed_within_batch_only":
                bidx = torch.zeros_like(bidx)
            vrow = bidx[:, None] * (N - 160) + (cols[None, :] - 160)
            addr = vt.base + vrow * vt.ld + rin[:, None]
            sel = wm[:, None] & (wn & isvt)[None, :]
            vt.full[addr[sel]] = st[sel]
            wn = wn & ~isvt
        sel = wm[:, None] & wn[None, :]
        addr = out.base + orow[:, None] * out.ld + cols[None, :]
        ok = (addr >= 0) & (addr < out.full.numel())
        out.full[addr[sel & ok]] = st[sel & ok]
        if c.side == "dup":
            out.full[(addr + M * out.ld)[sel & ok]] = st[sel & ok]
        if stats is not None and single_pass:
            cn = torch.ones_like(vn) if defect == "row_stats_count_pad_columns" else vn
            blk = torch.where(cn[None, :], st, 0.0)
            tj = int(n[0]) // 160
            stats[m[vm], tj, 0] = blk.sum(1)[vm]
            stats[m[vm], tj, 1] = (blk * blk).sum(1)[vm]
        if gn is not None:
            rows_in = torch.ones_like(vm) if (defect == "gn_acc_counts_rows_past_M" and single_pass) else vm
            blk = torch.where(rows_in[:, None] & vn[None, :], st, 0.0)
            bidx = (m // rpb).clamp(max=t["nb"] - 1)
            for k, (cg, c0, groups) in enumerate(gn_subs(c)):
                grp = ((n + c0) // cg).clamp(max=groups - 1)
                for b_ in bidx.unique().tolist():
                    rb = blk[bidx == b_]
                    gn[k][b_, :, 0].index_add_(0, grp, rb.sum(0))
                    gn[k][b_, :, 1].index_add_(0, grp, (rb * rb).sum(0))

    for bid in range(grid * npar):
        par_i, bid_t = (bid % 4, bid // 4) if subpix else (0, bid)    # the four parities of a tile are neighbouring blocks
        par = divmod(par_i, 2)
        nwg = grid
        q, r, xcd, idx = nwg >> 3, nwg & 7, bid_t & 7, bid_t >> 3
        if defect == "xcd_remap_drops_tile_when_grid_not_mult_of_8":
            lid = xcd * q + idx
        else:
            lid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
        if n_major and defect == "n_major_tile_swap":   # the N-major split of the id with the M-major divisor
            tile_n, tile_m = divmod(lid, tn)
        elif n_major:
            tile_n, tile_m = divmod(lid, tiles_m)
        else:
            tile_m, tile_n = divmod(lid, tn)
        if tile_m >= tiles_m or tile_n >= tn or lid >= grid:
            continue                                    # (a defective map can point outside the grid: nothing is computed)
        m = torch.arange(tile_m * bm, tile_m * bm + bm)
        n = torch.arange(tile_n * 160, tile_n * 160 + 160)
        valid = m < M
        wsel = (par_i * wrows // npar + n).clamp(max=t["w"].shape[0] - 1)
        for split in range(sk):
            acc = torch.zeros(bm, 160, dtype=torch.float64)
            for k0, s_, tap, off in k_steps(split):
                xt = tail_gather(m, valid, s_, tap, off, par)
                wt = torch.where((n < N)[:, None], w64[wsel][:, k0:k0 + 64], 0.0)
                acc += xt @ wt.T
            if sk > 1:
                mm, nn = m[valid], n[n < N]
                slabs[split][(out_row(mm, par) if subpix else mm)[:, None], nn[None, :]] = acc[valid][:, n < N]
            else:
                epilogue(m, n, acc, True, par, tile_m * bm)
    if sk > 1:
        total = slabs[:-1].sum(0) if defect == "combine_drops_last_slab" else slabs.sum(0)
        for m0 in range(0, M, 16):                      # the combines work on (row block, 160-column tile) pieces
            m = torch.arange(m0, min(M, m0 + 16))
            for j in range(tn):
                n = torch.arange(j * 160, min(N, (j + 1) * 160))
                epilogue(m, n, total[m][:, n], False)
    res["stats"] = stats.float() if stats is not None else None
    if gn is not None:
        res["gn"] = [torch.stack([(a_[..., 0] * 2.0 ** 24).round(), (a_[..., 1] * 2.0 ** 20).round()], -1).long() for a_ in gn]
    return res


def emu_result(c: Case, t, dtype, defect=None):
    """-> (out window as `dtype` / fp32 values in fp64 with NaN where nothing was stored, the emulation's dict)"""
    r = tile_walk_emulate(c, t, dtype, defect)
    return r["out"].view.clone(), r


def untouched(b: Buf) -> bool:
    """an emulated output buffer: everything outside the window is still the (NaN) sentinel"""
    return bool(torch.isnan(b.full[b.outside()]).all())


def windows_of(c: Case, t, full):
    """a [M, N] tensor of the op cut into the output windows of the case: dict name -> tensor (vt [nb * cols, rows_per_batch])"""
    w = {"out": full}
    if c.side == "vt":
        rpb = c.rows_per_batch
        w["out"] = full[:, :160]
        w["vt"] = full[:, 160:].reshape(t["nb"], rpb, -1).permute(0, 2, 1).reshape(-1, rpb)
    if c.side == "dup":
        w["out"] = torch.cat([full, full])
    return w


def expected_windows(c: Case, t, dtype):
    """every output window of an E / T case as the reference says it, cast once: dict name -> fp64 tensor"""
    return windows_of(c, t, expected_out(c, t, dtype).double())


def gated_windows(c: Case, t, dtype):
    """every output window of an R case: dict name -> (fp64 reference, gate)"""
    r, g = windows_of(c, t, t["ref"]), windows_of(c, t, gate(c, t, dtype))
    return {k: (r[k], g[k]) for k in r}


def emulation_failures(c: Case, t, dtype, defect=None):
    """Run the emulation and judge it as the GPU file judges the library: E / T for equality (side outputs included), R under
    its gate, nothing stored outside a window.  -> list of what failed (empty: the case passes)."""
    r = tile_walk_emulate(c, t, dtype, defect)
    bad = []
    rand = c.probe.startswith("R")
    for name, exp in (gated_windows(c, t, dtype) if rand else expected_windows(c, t, dtype)).items():
        got = r[name].view
        if rand:
            if not worst_ratio(got, exp[0], exp[1]) <= 1.0:
                bad.append(name + ": gate")
        elif not bool((got == exp).all()):
            bad.append(name + ": value")
        if not untouched(r[name]):
            bad.append(name + ": stored outside the window")
    sides = expected_sides(c, t, dtype) if not c.probe.startswith("R") else {}
    if "stats" in sides and not bool((r["stats"] == sides["stats"]).all()):
        bad.append("row_stats")
    if "gn" in sides and not all(bool((a == b).all()) for a, b in zip(r["gn"], sides["gn"])):
        bad.append("gn_acc")
    return bad


# ------------------------------------------------------------------------------------------------ for the older random tests
def conv64(x, w, stride: int = 1, up: bool = False):
    """conv3x3 (padding 1; after a nearest 2x upsample if `up`) in fp64 by slicing: x NHWC [B,H,W,C], w [Cout, 9 C]
    (k = (ky*3+kx)*C + c) -> [B, ho, wo, Cout]"""
    x = x.double()
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, hv, wv, C = x.shape
    ho, wo = (hv - 1) // stride + 1, (wv - 1) // stride + 1
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = [xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :] for ky in range(3) for kx in range(3)]
    return (torch.cat(cols, 3).reshape(B * ho * wo, 9 * C) @ w.double().T).reshape(B, ho, wo, -1)


def derived_check(out, ref, A, K: int, splits: int, what=""):
    """out against the fp64 `ref` under the R gate (A: the absolute sums, same shape); -> the worst error / gate"""
    g = gate_rpm(ref, A, K, splits, out.dtype)
    r = worst_ratio(out.reshape(ref.shape), ref, g)
    print(f"[gemm derived gate] {what}: error / gate {r:.3f}")
    assert r <= 1.0, (what, "error / derived gate", r)
    return r
