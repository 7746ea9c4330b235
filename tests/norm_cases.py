"""Shared by the normalisation probe tests (not a test file): data regimes, fp64 references, derived error bounds, the GPU
case matrix and a NumPy restatement of every path's arithmetic with named defects.  Nothing here touches the HIP library.

Notation.  u = unit roundoff of the 16-bit format (2^-8 bf16, 2^-11 fp16), u32 = 2^-24.  A statistic population (a
(batch item, group) of GroupNorm, a row of LayerNorm) has n elements, mean m, variance v, sum S, sum of squares Q and
    kappa = (m^2 + v) / (v + eps),
the factor by which a relative error of Q (or S) grows in  v = Q / n - m^2.

The output model, common to every path.  With dm the error of the mean and dr the relative error of rstd,
    pre  = (x - m) rstd gamma + beta            (the value before SiLU / rounding),   nrm = (x - m) rstd gamma
    |d pre| <= dm rstd (1 + dr) |gamma| + dr |nrm| + c32 u32 T
T the magnitudes before cancellation, (|x| + |m|) rstd |gamma| + |beta|, c32 the count of fp32 roundings on the way (6 for
the scale / shift form  x * sc + sh  of the GroupNorm kernels: m and rstd to fp32, sc = rstd * gamma, m * sc, beta - m * sc,
x * sc, the last add; 4 for LayerNorm's (x - m) * rstd * gamma + beta).  SiLU has slope <= 1.1 and is evaluated as
x * rcp(1 + exp2(-x log2 e)): exp2 and rcp are 1 ulp (2^-23) each, the argument product carries u32 |pre|, the add and the
final product u32 each:  (7 + |pre|) u32 |y|.  The stored value is rounded once:  gate = u |ref| + (1 + u) (the above)
[+ 2^-25 in fp16: outputs below 2^-14 are subnormal].

The statistics model.  |dS| <= eS sum|x| + aS,  |dQ| <= eQ Q + aQ  (relative fp32 accumulation terms, absolute fixed-point
terms) give  dm = dS / n,  dv = dQ / n + 2 |m| dm + dm^2,  d = dv / (v + eps)  and, exactly (no linearisation),
    dr = 1 / sqrt(1 - d) - 1,  capped by  sqrt((v + eps) / eps) - 1:  every kernel clamps v at 0, rstd <= 1 / sqrt(eps).
Since sum|x| / n <= sqrt(Q / n) and |m| <= sqrt(Q / n):  d <= (eQ + 2 eS) kappa, so dr ~ (eQ + 2 eS) kappa / 2.
A sum of k fp32 terms rounds k - 1 times, each by <= u32 of the running sum; squares of 16-bit values are exact in fp32
(16 or 22 significant bits), adding a zero is exact.  Per path:

  gn_stats_kernel -> gn_fold (`stats_eps`): a thread adds L = ceil(per / P) pixels per channel, the group fold adds
      Pe cg partials (Pe = min(P, per) pixel lanes hold data), the fp64 fold over <= 128 chunks adds 128 * 2^-53:
      eS = eQ = (L - 1 + Pe cg - 1) u32 + 2^-46.
  accumulators built by `build_acc` (pp_groupnorm_apply_acc against its contract): aS = 2^-25, aQ = 2^-21 (half a quantum),
      eS = eQ = 2^-50 (the fp64 fold).
  epilogue accumulators against the exact sums of the stored output (`gate_epilogue_acc`): every (row block, column) pair
      is one add of a rounded fp32 column sum: ceil(rows_per_batch / R) * columns of the group adds of half a quantum, and
      the column sums carry R u32 (R + 1 for the squares: v * v rounds) of the group's sum|x| (Q).  R, the rows of a block,
      is 16 in the split-K combine, 64 in a per-pass fold (always so at rows_per_batch = 64), the tile height otherwise;
      where the caller cannot know it, 16 for the adds and min(256, rows_per_batch) for the column sums.
  row moments (`gate_row_stats`): 8 values per thread (4 pair sums, 4 adds) then <= 20 pieces in sequence: 28 u32 sum|x|,
      29 u32 Q per (row, 160-column tile).
  folded LayerNorm (`gate_folded_ln`, moments given in fp32): one rounding of each partial, `tiles` adds, 1 / C and the
      product:  eS = eQ = (tiles + 3) u32;  v = q / C - m * m in fp32 adds 2 u32 Q / n;  rsqrtf 4 u32.  The GEMM itself:
      acc = sum_k x_k w'_k in fp32, any order: K u32 A with A = sum_k |x_k w'_k|;  cs to fp32, cs * m, the subtraction:
      3 u32 |cs m|;  all scaled by rstd.  GEGLU a * gelu(g): |gelu'| <= 1.13, gelu_fast_f is within 2^-20 |g|
      (Abramowitz-Stegun 7.1.26: 1.5e-7 on erf; v_rcp, v_exp and eight fp32 operations).
  pp_tfront (`gate_tfront_hs`, `gate_tfront_qkv`): the GroupNorm gate (accumulator path, rounding included) carried through
      |w1|, C u32 of proj_in's absolute products, one rounding of hs; then, from the hs the kernel stored, the folded
      LayerNorm with moments formed in the kernel: 80 roundings per lane, two shuffle adds, 1 / C and the product: 84 u32.
  pp_xattn_block (`gate_xattn_block`): the folded-LayerNorm logits (exp2 domain) with error D move a probability by
      p (2^(2 D) - 1); the fp32 sum of 80 exponentials, v_exp, v_rcp: 88 u32 p; p rounded to 16 bits: u p; 640 u32 of the
      second GEMM's absolute products.
  layernorm_kernel (two passes, `gate_layernorm`): lane sums of 8 NP values, six butterfly adds:  E = 8 NP + 5 roundings,
      dm = (E + 1) u32 sum|x| / C;  the second pass sums (x - m')^2 -- positive terms, no cancellation --
      dv = (E + 3) u32 (v + dm^2) + dm^2;  rsqrtf 4 u32.  kappa does not amplify dv here, only dm / std = (E + 1) u32
      sqrt(kappa).

Envelope (`kappa_envelope`): the largest kappa at which the statistics term stays below the output rounding,
(eQ + 2 eS) kappa / 2 <= u, i.e. kappa <= 2 u / (eQ + 2 eS); include/pp_hip.h states it per path and format.  These are
guaranteed (worst-case, linear in the number of roundings) figures: a typical input errs like the square root of the count.
The `edge` regime sits at min(envelope, what the format can hold with a standard deviation of two quanta: mean / std = 64
in bf16, 512 in fp16).

Regimes (`build_x`): values are rounded to the format first, every reference sees the kernel's bits.
  zero      N(0, 1)
  offset16  N(16 s, 1), s = +-1 per population
  edge      N(r s, 1), r = sqrt(kappa_edge - 1)
  constant  every element of a population equal to k / 2, |k| = 1 .. 15: sums and squares (multiples of 1/4 below 2^22
            for n <= 2^16) are exact in fp32 and in fixed point, so v = 0 exactly and the statistics terms vanish
            (`stats_exact`); the output is beta up to the scale / shift cancellation; eps 1e-5 and 1e-6
  outlier   N(0, 1), one channel multiplied by 100
  tiny      N(0, 2^-12): the 2^-20 quantum of the squared-sum accumulator matters

The emulations (`emu_*`) restate each path in NumPy float32 in the kernel's accumulation order and carry the defects of
DEFECTS by name; tests/test_norm_probes.py proves on the CPU that the faithful form meets every gate of the GPU matrix and
that each defect fails one.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
SUM_SCALE, SQ_SCALE = 2.0 ** 24, 2.0 ** 20
REGIMES = ("zero", "offset16", "edge", "constant", "outlier", "tiny")
DEFECTS = ("last_chunk_dropped", "per_floor", "n_counts_c1_only", "x2_read_with_c1_stride",
           "slot_group_from_first_channel", "tail_loop_rows_skipped", "fourth_prefetched_row_dropped",
           "batch_from_tile_start", "acc_scales_swapped", "ragged_column_tile_dropped", "ln_last_block_skipped",
           "np_one_too_small", "folded_cs_mean_dropped", "folded_ln_dim_is_one_tile")
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]

# ------------------------------------------------------------------------------------------------ the GPU matrix
# (c1, c2, groups, hw, batch)
GN_SHAPES = [
    (32, 0, 32, 1, 2),          # one pixel, one channel per group: n = 1
    (8, 0, 1, 5, 2),            # one slot, one group, hw < 16
    (64, 0, 8, 15, 2),          # groups < 32, one chunk one pixel short of two
    (320, 0, 32, 17, 2),        # one chunk of 17 pixels: three pixels per stats lane, the last one ragged
    (320, 0, 32, 47, 2),        # two chunks (24 + 23)
    (320, 0, 32, 2065, 1),      # nchunk capped at 128: per = 17, chunk 121 short, 122 .. 127 empty
    (1280, 0, 32, 2065, 1),     # one row per pass, the apply grid capped at 512 blocks: rows >= 2048 in the tail loop
    (2048, 0, 32, 9, 2),        # S = 256 exactly, one row per pass, fewer than four rows per thread
    (1280, 1280, 32, 9, 2),     # S = 320: the flat path; gn_fold_acc's loop past channel 2048
    (2056, 0, 8, 5, 2),         # cg = 257: every slot boundary straddled, flat path
    (8, 56, 32, 5, 2),          # cg = 2; the two sources have different strides
    (640, 320, 32, 17, 2),      # cg = 30: a group straddles the two sources
]
GN_ALL_REGIMES_AT = (320, 0, 32, 47, 2)
LN_C = (8, 320, 512, 520, 1024, 1032, 1536, 1544, 2048)
LN_ROWS = (1, 5, 7)
LN_ALL_REGIMES_AT = 520
ROWSTAT_N, ROWSTAT_M = (200, 320, 1280), (5, 192)
FOLD_KINDS = ("plain", "geglu", "vt")
FOLD_C = (320, 1280)
FOLD_REGIMES = ("zero", "offset16", "edge", "outlier")
FOLD_B, FOLD_HW = 2, 136
FOLD_N = {"plain": 320, "geglu": 640, "vt": 960}
# epilogue accumulators through ops.gemm: (name, batch, rows_per_batch, N, K, [(cg, c0, groups)], splitk)
EPI_CASES = [
    ("b3", 3, 64, 320, 320, [(10, 0, 32)], 1),
    ("b5", 5, 64, 320, 320, [(10, 0, 32)], 1),
    ("n200", 3, 64, 200, 320, [(10, 0, 20)], 1),
    ("cg8_c0_4", 3, 64, 160, 320, [(8, 4, 21)], 1),
    ("two_subs", 3, 64, 320, 320, [(10, 0, 32), (20, 320, 32)], 1),
    ("b3_splitk2", 3, 64, 320, 1280, [(10, 0, 32)], 2),
    ("two_subs_splitk2", 5, 64, 320, 1280, [(10, 0, 32), (20, 320, 32)], 2),
]
EPI_TILES = (53, 44, 22, 0)      # one 256-row, one 128-row, one 64-row tile, and the library's choice


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def max_ratio_of_format(dtype) -> float:
    """largest mean / std (std = 1) at which the standard deviation is still two quanta of the format"""
    return {torch.bfloat16: 64.0, torch.float16: 512.0}[dtype]


def quantum(x: float, dtype) -> float:
    bits = {torch.bfloat16: 7, torch.float16: 10}[dtype]
    return 2.0 ** (math.floor(math.log2(abs(x))) - bits)


def _gen(*key) -> torch.Generator:
    seed = 0
    for x in key:
        seed = (seed * 1000003 + int(x) + 17) % (2 ** 31 - 1)
    return torch.Generator("cpu").manual_seed(seed)


def gn_nchunk(hw: int) -> int:
    return max(1, min(128, hw // 16))


def gn_launch(hw: int, C: int):
    """(S, P of the stats kernel, nchunk, per, R rows per apply pass (0: flat path), apply blocks)"""
    S = C // 8
    P = min(8, 512 // S)
    nchunk = gn_nchunk(hw)
    per = (hw + nchunk - 1) // nchunk
    if S <= 256:
        R = 256 // S
        nb = (hw + R * 4 - 1) // (R * 4)
    else:
        R = 0
        nb = (hw * S + 2047) // 2048
    return S, P, nchunk, per, R, max(1, min(512, nb))


# ------------------------------------------------------------------------------------------------ statistics error terms
def stats_eps(hw: int, C: int, groups: int):
    """(eS, eQ, aS, aQ) of gn_stats_kernel -> gn_fold"""
    S, P, nchunk, per, _, _ = gn_launch(hw, C)
    L = (per + P - 1) // P
    e = (L - 1 + min(P, per) * (C // groups) - 1) * U32 + 2.0 ** -46
    return e, e, 0.0, 0.0


def acc_eps():
    """(eS, eQ, aS, aQ) of accumulators rounded once from the exact sums (build_acc)"""
    return 2.0 ** -50, 2.0 ** -50, 0.5 / SUM_SCALE, 0.5 / SQ_SCALE


def folded_ln_eps(tiles: int):
    e = (tiles + 3) * U32
    return e, e + 2 * U32, 0.0, 0.0


def kappa_envelope(eS: float, eQ: float, dtype) -> float:
    return 2.0 * unit_roundoff(dtype) / (eQ + 2.0 * eS)


def edge_ratio(eS: float, eQ: float, dtype) -> float:
    """mean / std of the `edge` regime: at the envelope, or at what the format can hold"""
    k = kappa_envelope(eS, eQ, dtype)
    return min(math.sqrt(max(k - 1.0, 0.0)), max_ratio_of_format(dtype))


# ------------------------------------------------------------------------------------------------ regimes
def build_x(regime: str, dtype, B: int, hw: int, C: int, groups: int, ratio: float = 0.0, key=0) -> torch.Tensor:
    """[B, hw, C] in `dtype` (CPU); a population is (batch item, group of C / groups channels) x hw.  ratio: mean / std of
    `edge`."""
    assert regime in REGIMES, regime
    g = _gen(REGIMES.index(regime), B, hw, C, groups, key)
    x = torch.randn(B, hw, C, generator=g, dtype=torch.float64)
    cg = C // groups
    sign = (torch.randint(0, 2, (B, 1, groups), generator=g).double() * 2 - 1).repeat_interleave(cg, 2)
    if regime == "offset16":
        x = x + 16.0 * sign
    elif regime == "edge":
        x = x + ratio * sign
    elif regime == "constant":
        k = torch.randint(1, 16, (B, 1, groups), generator=g).double().repeat_interleave(cg, 2)
        assert hw * cg <= 2 ** 16                                      # (see the module docstring: sums stay exact)
        x = (0.5 * k * sign).expand(B, hw, C).clone()
    elif regime == "outlier":
        x[:, :, (C // 2 + 3) % C] *= 100.0
    elif regime == "tiny":
        x = x * 2.0 ** -6
    return x.to(dtype)


# ------------------------------------------------------------------------------------------------ fp64 references
def _pop(x: torch.Tensor, groups: int):
    """x [B, hw, C] fp64 -> (n, sum|x|, Q, mean, var) per population [B, groups] and the channel -> group map"""
    B, hw, C = x.shape
    cg = C // groups
    xg = x.reshape(B, hw, groups, cg)
    n = hw * cg
    S1 = xg.abs().sum((1, 3))
    Q = (xg * xg).sum((1, 3))
    mean = xg.sum((1, 3)) / n
    var = ((xg - mean[:, None, :, None]) ** 2).sum((1, 3)) / n
    return n, S1, Q, mean, var


def _per_channel(t: torch.Tensor, cg: int) -> torch.Tensor:
    return t.repeat_interleave(cg, 1)[:, None, :]                       # [B, groups] -> [B, 1, C]


def silu64(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(x)


def ref_groupnorm(x1, x2, groups: int, gamma, beta, eps: float, silu: bool):
    """GroupNorm(+SiLU) of concat(x1, x2) [B, hw, c] in fp64 -> ref [B, hw, C]"""
    x = (torch.cat([x1, x2], -1) if x2 is not None else x1).double()
    cg = x.shape[2] // groups
    _, _, _, mean, var = _pop(x, groups)
    pre = (x - _per_channel(mean, cg)) * _per_channel(1.0 / torch.sqrt(var + eps), cg) * gamma.double() + beta.double()
    return silu64(pre) if silu else pre


def ref_layernorm(x, gamma, beta, eps: float):
    x = x.double()
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * gamma.double() + beta.double()


def ref_ln_linear(x, w16, t, eps: float):
    """LayerNorm (no affine: gamma sits in w16, beta in t) -> Linear with the 16-bit weights the kernel multiplies"""
    one = torch.ones(x.shape[1], dtype=torch.float64, device=x.device)
    return ref_layernorm(x, one, 0 * one, eps) @ w16.double().t() + t.double()


def gelu64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def group_sums(t: torch.Tensor, cg: int, c0: int, groups: int):
    """t [B, rows, N] (the stored output) at channel offset c0 of a norm with `groups` groups of cg channels ->
    exact (sum, sum of squares, sum|x|, columns) per (batch item, group), fp64 [B, groups] each"""
    B, rows, N = t.shape
    td = t.double()
    gi = (c0 + torch.arange(N, device=t.device)) // cg
    onehot = torch.zeros(N, groups, dtype=torch.float64, device=t.device)
    onehot[torch.arange(N, device=t.device), gi] = 1.0
    return td.sum(1) @ onehot, (td * td).sum(1) @ onehot, td.abs().sum(1) @ onehot, onehot.sum(0)


def row_tile_sums(t: torch.Tensor, bn: int = 160):
    """t [M, N] -> exact (sum, sum of squares, sum|x|) per (row, 160-column tile), fp64 [M, ceil(N / bn)] each"""
    M, N = t.shape
    tiles = (N + bn - 1) // bn
    td = torch.zeros(M, tiles * bn, dtype=torch.float64, device=t.device)
    td[:, :N] = t.double()
    td = td.reshape(M, tiles, bn)
    return td.sum(-1), (td * td).sum(-1), td.abs().sum(-1)


def build_acc(x1, x2, groups: int) -> torch.Tensor:
    """The int64 [B][groups][2] accumulators of concat(x1, x2), straight from the fp64 sums"""
    x = (torch.cat([x1, x2], -1) if x2 is not None else x1).double()
    B, hw, C = x.shape
    xg = x.reshape(B, hw, groups, C // groups)
    return torch.stack([torch.round(xg.sum((1, 3)) * SUM_SCALE), torch.round((xg * xg).sum((1, 3)) * SQ_SCALE)], -1).to(torch.int64)


# ------------------------------------------------------------------------------------------------ gates
def _dr(d: torch.Tensor, v_eps: torch.Tensor, eps: float) -> torch.Tensor:
    """relative error of rstd for |dv| <= d (v + eps).  Upwards 1 / sqrt(1 - d) - 1, but every kernel clamps v at 0, so rstd
    never exceeds 1 / sqrt(eps); downwards 1 - 1 / sqrt(1 + d)."""
    up = torch.where(d < 1.0, 1.0 / torch.sqrt((1.0 - d).clamp_min(1e-300)) - 1.0, torch.full_like(d, math.inf))
    up = torch.minimum(up, torch.sqrt(v_eps / eps) - 1.0)
    return torch.maximum(up, 1.0 - 1.0 / torch.sqrt(1.0 + d))


def _finish(ref, dpre, pre, silu: bool, dtype):
    u = unit_roundoff(dtype)
    if silu:
        dpre = 1.1 * dpre + (7.0 + pre.abs()) * U32 * ref.abs()
    g = u * ref.abs() + (1.0 + u) * dpre
    return g + 2.0 ** -25 if dtype == torch.float16 else g


def gate_groupnorm(x1, x2, groups: int, gamma, beta, eps: float, silu: bool, dtype, terms, stats_exact: bool = False):
    """-> (ref, gate) fp64 [B, hw, C]; terms = (eS, eQ, aS, aQ) of the path, stats_exact: the `constant` regime"""
    x = (torch.cat([x1, x2], -1) if x2 is not None else x1).double()
    cg = x.shape[2] // groups
    eS, eQ, aS, aQ = (0.0, 0.0, 0.0, 0.0) if stats_exact else terms
    n, S1, Q, mean, var = _pop(x, groups)
    dm = (eS * S1 + aS) / n
    dv = (eQ * Q + aQ) / n + 2.0 * mean.abs() * dm + dm * dm
    dr = _dr(dv / (var + eps), var + eps, eps)
    rstd = 1.0 / torch.sqrt(var + eps)
    ga, be = gamma.double().abs(), beta.double()
    m_c, r_c, dm_c, dr_c = (_per_channel(t, cg) for t in (mean, rstd, dm, dr))
    nrm = (x - m_c) * r_c * gamma.double()
    pre = nrm + be
    T = (x.abs() + m_c.abs()) * r_c * ga + be.abs()
    dpre = dm_c * r_c * (1.0 + dr_c) * ga + dr_c * nrm.abs() + 6.0 * U32 * T
    ref = silu64(pre) if silu else pre
    return ref, _finish(ref, dpre, pre, silu, dtype)


def ln_np(C: int) -> int:
    return (C // 8 + 63) // 64


def gate_layernorm(x, gamma, beta, eps: float, dtype, stats_exact: bool = False):
    """-> (ref, gate) fp64 [rows, C] of layernorm_kernel; stats_exact: the `constant` regime (sum / C is then exactly x)"""
    x = x.double()
    C = x.shape[1]
    E = 8 * ln_np(C) + 5
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    dm = (0.0 if stats_exact else (E + 1) * U32) * x.abs().mean(-1, keepdim=True)
    dv = (E + 3) * U32 * (var + dm * dm) + dm * dm
    dr = _dr(dv / (var + eps), var + eps, eps) + 4.0 * U32
    rstd = 1.0 / torch.sqrt(var + eps)
    ga, be = gamma.double().abs(), beta.double()
    nrm = (x - mean) * rstd * gamma.double()
    ref = nrm + be
    dpre = dm * rstd * (1.0 + dr) * ga + dr * nrm.abs() + 4.0 * U32 * (nrm.abs() + be.abs())
    return ref, _finish(ref, dpre, ref, False, dtype)


def gate_epilogue_acc(t: torch.Tensor, rows_per_batch: int, cg: int, c0: int, groups: int, block_rows: int = 0):
    """t [B, rows_per_batch, N], the stored output -> (S, Q exact, gate on S, gate on Q), fp64 [B, groups] each.
    block_rows: the rows one add covers -- 16 for the split-K combine, 64 for a per-pass fold, BM for a whole tile; 0 where
    the caller cannot know the form the library chose: the most adds (16-row blocks) and the longest column sums (256)."""
    S, Q, S1, cols = group_sums(t, cg, c0, groups)
    adds = ((rows_per_batch + (block_rows or 16) - 1) // (block_rows or 16)) * cols[None, :]
    R = block_rows or min(256, rows_per_batch)
    return S, Q, adds * 0.5 / SUM_SCALE + R * U32 * S1, adds * 0.5 / SQ_SCALE + (R + 1) * U32 * Q


def epilogue_block_rows(rows_per_batch: int, splitk: int) -> int:
    """rows per add of the epilogue accumulators where the form is known whatever tile the library picks: the split-K
    combine folds 16-row blocks; a single pass folds 64-row passes when rows_per_batch = 64 (a 64-row tile is one pass)"""
    return 16 if splitk > 1 else (64 if rows_per_batch == 64 else 0)


def gate_row_stats(t: torch.Tensor):
    """t [M, N] -> (S, Q exact, gate on S, gate on Q) [M, tiles]"""
    S, Q, S1 = row_tile_sums(t)
    return S, Q, 28 * U32 * S1, 29 * U32 * Q


def kernel_moments_eps():
    """(eS, eQ, 0, 0) of row moments formed inside pp_tfront / pp_xattn_block from the stored 16-bit row: a lane folds 20
    quads (three adds and one accumulation each: 80 roundings), two shuffle adds, 1 / C and the product"""
    return 84 * U32, 85 * U32 + 2 * U32, 0.0, 0.0


def folded_pre(x, w16, cs, t, eps: float, terms):
    """-> (ref = LN(x) w16^T + t, dz = its error before any rounding to 16 bits), fp64 [M, N]; t may hold -inf (a masked
    logit: exact)"""
    x, w = x.double(), w16.double()
    K = x.shape[1]
    eS, eQ, _, _ = terms
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    Qn = (x * x).mean(-1, keepdim=True)
    dm = eS * x.abs().mean(-1, keepdim=True)
    dv = eQ * Qn + 2.0 * mean.abs() * dm + dm * dm
    dr = _dr(dv / (var + eps), var + eps, eps) + 4.0 * U32
    rstd = 1.0 / torch.sqrt(var + eps)
    z = ((x - mean) * rstd) @ w.t()
    A = x.abs() @ w.abs().t()
    csd = cs.double().abs()[None, :]
    td = t.double()
    tabs = torch.where(torch.isfinite(td), td.abs(), torch.zeros_like(td))
    dz = rstd * (1.0 + dr) * (K * U32 * A + 3.0 * U32 * csd * mean.abs() + dm * csd) + dr * z.abs() + 3.0 * U32 * (z.abs() + tabs)
    return z + td, dz


def plain_pre(x, w16, t):
    """no LayerNorm folded (ln_stats NULL: mean = 0, rstd = 1): -> (ref = x w16^T + t, dz), as folded_pre: K u32 of the
    absolute products, the (exact) multiplication by rstd = 1 and the addition of t: 3 u32"""
    x, w = x.double(), w16.double()
    td = t.double()
    tabs = torch.where(torch.isfinite(td), td.abs(), torch.zeros_like(td))
    z = x @ w.t()
    return z + td, x.shape[1] * U32 * (x.abs() @ w.abs().t()) + 3.0 * U32 * (z.abs() + tabs)


def gate_folded_ln(x, w16, cs, t, eps: float, tiles: int, dtype, geglu: bool = False, terms=None, fold: bool = True):
    """x [M, K] 16-bit, w16 [N, K] 16-bit (gamma folded in), cs [N] fp32 column sums, t [N] fp32 (bias + W beta) ->
    (ref, gate) fp64 [M, N] (GEGLU: [M, N / 2], value columns first, gate columns second).  terms: the moments' error
    terms, default folded_ln_eps(tiles) (moments given, rounded once to fp32); fold=False: no LayerNorm (plain_pre)"""
    ref, dz = folded_pre(x, w16, cs, t, eps, terms or folded_ln_eps(tiles)) if fold else plain_pre(x, w16, t)
    if geglu:
        h = ref.shape[1] // 2
        a, g, da, dg = ref[:, :h], ref[:, h:], dz[:, :h], dz[:, h:]
        ref = a * gelu64(g)
        dz = da * gelu64(g).abs() + (a.abs() + da) * (1.13 * dg + 2.0 ** -20 * g.abs()) + 2 * U32 * ref.abs()
    return ref, _finish(ref, dz, ref, False, dtype)


def quad_perm(n: int, device="cpu") -> torch.Tensor:
    """rows of a GEGLU weight in interleaved quads (h0, h1, g0, g1) -> [values | gates] order (unit 2q + j = quad q, j)"""
    q = torch.arange(n // 4, device=device)
    return torch.cat([torch.stack([4 * q, 4 * q + 1], 1).reshape(-1), torch.stack([4 * q + 2, 4 * q + 3], 1).reshape(-1)])


def gate_ff_fused(hs, w1, b1, cs1, w2, bias2, eps: float, dtype, tiles: int = 0, fold: bool = True, scale: float = 1.0, res=()):
    """pp_ff_fused: out = round16(GEGLU(LN(hs) w1^T + b1)) w2a^T + hs w2b^T + bias2, w1 [8C, C] in interleaved quads with the
    LayerNorm's gamma folded in, w2 = [w2a | w2b] [C, 4C + C] in natural order.  The GEGLU values carry the folded-LayerNorm
    gate (their 16-bit rounding included); the second GEMM adds K2 u32 of its absolute products (K2 = 5C, any order) and
    propagates the first through |w2a|.  tiles: partial moments per row (default C / 160); fold=False: ln_stats NULL (cs1 is not
    read); the epilogue (acc + bias2) * scale + res[0] + res[1] (full [M, C] tensors, a wrapped one already expanded) adds
    the product and the additions: 4 u32 of the magnitudes.  -> (ref, gate) fp64 [M, C]"""
    C = hs.shape[1]
    perm = quad_perm(w1.shape[0], w1.device)
    act, g_act = gate_folded_ln(hs, w1[perm], cs1[perm] if fold else None, b1[perm], eps, tiles or C // 160, dtype, geglu=True,
                                fold=fold)
    w2a, w2b = w2[:, :4 * C].double(), w2[:, 4 * C:].double()
    hd = hs.double()
    b2 = bias2.double() if bias2 is not None else torch.zeros(C, dtype=torch.float64, device=hs.device)
    ref = act @ w2a.t() + hd @ w2b.t() + b2
    d = g_act @ w2a.abs().t() + 5 * C * U32 * ((act.abs() + g_act) @ w2a.abs().t() + hd.abs() @ w2b.abs().t() + b2.abs())
    if scale != 1.0 or len(res):
        rs = sum((r.double() for r in res), torch.zeros_like(ref))
        ra = sum((r.double().abs() for r in res), torch.zeros_like(ref))
        d = d * abs(scale) + 4 * U32 * (ref.abs() * abs(scale) + ra)
        ref = ref * scale + rs
    return ref, _finish(ref, d, ref, False, dtype)


def gate_tfront_hs(x, gg, gb, w1, b1, dtype, groups: int = 32):
    """pp_tfront, first half: hs = round16(GroupNorm(x)) w1^T + b1, statistics from accumulators (x [B, hw, C], 32 groups,
    eps 1e-6, no SiLU).  The normalised values carry their GroupNorm gate (rounding included) through |w1|; the GEMM adds
    C u32 of its absolute products.  -> (ref, gate) fp64 [B * hw, C]"""
    C = x.shape[2]
    n, gn = gate_groupnorm(x, None, groups, gg, gb, 1e-6, False, dtype, acc_eps())
    n, gn = n.reshape(-1, C), gn.reshape(-1, C)
    wa = w1.double().abs().t()
    ref = n @ w1.double().t() + b1.double()
    d = gn @ wa + C * U32 * ((n.abs() + gn) @ wa + b1.double().abs())
    return ref, _finish(ref, d, ref, False, dtype)


def gate_tfront_qkv(hs_stored, wf, cs, tb, dtype, q_scale: float = 1.0):
    """pp_tfront, second half, from the hs the kernel stored: LayerNorm1 -> QKV with the moments formed in the kernel.
    q_scale: the Q third (the first N / 3 columns) is multiplied by it in fp32 before its one rounding: one more u32"""
    if q_scale == 1.0:
        return gate_folded_ln(hs_stored, wf, cs, tb, 1e-5, 2, dtype, terms=kernel_moments_eps())
    ref, dz = folded_pre(hs_stored, wf, cs, tb, 1e-5, kernel_moments_eps())
    n = ref.shape[1] // 3
    qs = float(np.float32(q_scale))
    ref = torch.cat([ref[:, :n] * qs, ref[:, n:]], 1)
    dz = torch.cat([dz[:, :n] * qs + U32 * ref[:, :n].abs(), dz[:, n:]], 1)
    return ref, _finish(ref, dz, ref, False, dtype)


XA_HEADS, XA_KP = 8, 80


def xattn_kk(device="cpu") -> torch.Tensor:
    """contraction index (head * 80 + key) stored at position kp of H^T (pp_xattn_fold, k-permuted order)"""
    kp = torch.arange(XA_HEADS * XA_KP, device=device)
    s32, kg, j = kp // 32, (kp // 8) % 4, kp % 8
    return 32 * s32 + 16 * (j // 4) + 4 * kg + (j % 4)


def gate_xattn_block(x, st_tiles: int, folded, bo, res, rows_per_batch: int, eps: float, dtype, fold: bool = True, terms=None):
    """pp_xattn_block with the moments given: l = LN(x) gt^T + gbias (exp2 domain), p = softmax2 per head over 80 key slots,
    out = round16(p) ht^T + bo + res.  A logit error <= D (fp32 products included: 2 u32 (|l| + |max|)) moves a probability by
    at most p (2^(2 D) - 1); the sum of 80 exponentials, v_exp, v_rcp and the product add 88 u32 p; p is rounded to 16
    bits (u p); the second GEMM adds 640 u32 of its absolute products, the bias and residual adds 2 u32.
    x [M, K] (K = C: 320, 640 or 1280), bo / res may be None; fold=False: ln_stats NULL (plain_pre; gcs is not used); terms:
    the moments' error terms, default folded_ln_eps(st_tiles) (kernel_moments_eps() where the kernel forms them: pre_w).
    -> (ref, gate) fp64 [M, C]"""
    gt, gcs, gb, ht = folded
    zc = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    bo = zc if bo is None else bo.double()
    res = torch.zeros(x.shape, dtype=torch.float64, device=x.device) if res is None else res.double()
    u = unit_roundoff(dtype)
    M, C = x.shape
    kk = xattn_kk(x.device)
    ref = torch.empty(M, C, dtype=torch.float64, device=x.device)
    d = torch.empty_like(ref)
    for b in range(M // rows_per_batch):
        r = slice(b * rows_per_batch, (b + 1) * rows_per_batch)
        l, dl = folded_pre(x[r], gt[b], gcs[b], gb[b], eps, terms or folded_ln_eps(st_tiles)) if fold else plain_pre(x[r], gt[b], gb[b])
        lh = l.reshape(-1, XA_HEADS, XA_KP)
        live = torch.isfinite(lh)
        mx = torch.where(live, lh, torch.full_like(lh, -1e300)).max(-1, keepdim=True).values
        dl = dl.reshape(-1, XA_HEADS, XA_KP) + 2 * U32 * (torch.where(live, lh.abs(), torch.zeros_like(lh)) + mx.abs())
        D = torch.where(live, dl, torch.zeros_like(dl)).max(-1, keepdim=True).values
        p = torch.softmax(lh * math.log(2.0), -1)
        dp = (p * (torch.exp2(2.0 * D) - 1.0 + 88 * U32 + u)).reshape(-1, XA_HEADS * XA_KP)
        p = p.reshape(-1, XA_HEADS * XA_KP)
        hta = ht[b].double()                                                   # [C, 640], position kp holds key kk[kp]
        o = p[:, kk] @ hta.t()
        A = p[:, kk] @ hta.abs().t()
        ref[r] = o + bo + res[r]
        d[r] = dp[:, kk] @ hta.abs().t() + 640 * U32 * A + 2 * U32 * (o.abs() + bo.abs() + res[r].abs())
    return ref, _finish(ref, d, ref, False, dtype)


def worst_ratio(out: torch.Tensor, expected: torch.Tensor, gate: torch.Tensor) -> float:
    """max |out - expected| / gate; an error where the gate is 0, or a non-finite output, is inf."""
    err = (out.double() - expected).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    r = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ case builders
def affine(C: int, key=0):
    g = _gen(99, C, key)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


def gn_regimes(shape):
    return REGIMES if tuple(shape) == GN_ALL_REGIMES_AT else ("zero", "offset16")


def gn_eps_list(regime: str, silu: bool):
    """eps of a case: SiLU norms of the networks use 1e-5, the plain ones 1e-6; `constant` runs with both"""
    return (1e-5, 1e-6) if regime == "constant" else ((1e-5,) if silu else (1e-6,))


def build_gn_case(shape, regime: str, dtype, path: str):
    """-> dict(x1, x2 [B, hw, c] `dtype` CPU, gamma, beta fp32, terms, exact).  path: "stats" | "acc" """
    c1, c2, groups, hw, B = shape
    C = c1 + c2
    terms = stats_eps(hw, C, groups) if path == "stats" else acc_eps()
    ratio = edge_ratio(terms[0], terms[1], dtype) if regime == "edge" else 0.0
    x = build_x(regime, dtype, B, hw, C, groups, ratio)
    gamma, beta = affine(C)
    x1 = x[:, :, :c1].contiguous()
    x2 = x[:, :, c1:].contiguous() if c2 else None
    return dict(x1=x1, x2=x2, gamma=gamma, beta=beta, terms=terms, exact=regime == "constant", ratio=ratio)


def ln_regimes(C: int):
    return REGIMES if C == LN_ALL_REGIMES_AT else ("zero",)


def build_ln_case(C: int, rows: int, regime: str, dtype):
    ratio = max_ratio_of_format(dtype) if regime == "edge" else 0.0      # (the two-pass form: only the format limits it)
    x = build_x(regime, dtype, rows, 1, C, 1, ratio, key=1).reshape(rows, C)
    gamma, beta = affine(C, key=1)
    return dict(x=x, gamma=gamma, beta=beta, ratio=ratio)


def build_fold_case(kind: str, C: int, regime: str, dtype):
    """A LayerNorm folded into the Linear behind it: x [M, C], w16 = round16(gamma (.) W) [N, C], cs [N], t [N], st [M, C/160, 2]
    fp32 moments rounded once from the exact tile sums (the producer is probed on its own)."""
    M, N, tiles = FOLD_B * FOLD_HW, FOLD_N[kind], C // 160
    terms = folded_ln_eps(tiles)
    ratio = edge_ratio(terms[0], terms[1], dtype) if regime == "edge" else 0.0
    x = build_x(regime, dtype, M, 1, C, 1, ratio, key=2).reshape(M, C)
    g = _gen(7, C, N)
    gamma = torch.randn(C, generator=g) * 0.3 + 1.0
    w = torch.randn(N, C, generator=g) * C ** -0.5
    t = torch.randn(N, generator=g) * 0.2 if kind != "vt" else torch.zeros(N)
    w16 = (w * gamma[None, :]).to(dtype)
    cs = w16.double().sum(1).float()
    S, Q, _ = row_tile_sums(x)
    st = torch.stack([S, Q], -1).float().contiguous()
    return dict(x=x, w16=w16, cs=cs, t=t, st=st, tiles=tiles, ratio=ratio, M=M, N=N)


FF_M, FF_C = 128, 320                    # the smallest shape pp_ff_fused accepts
FUSED_REGIMES = ("offset16", "outlier")


def build_ff_case(regime: str, dtype, M: int = FF_M, tiles: int = 2):
    """hs [M, 320] of the regime and a feed-forward's weights in the layouts of tests/test_ff_fused_gpu.py::_case; the row
    moments st in `tiles` partials per row (column tiles of 320 / tiles)"""
    C = FF_C
    hs = build_x(regime, dtype, M, 1, C, 1, 0.0, key=3).reshape(M, C)
    g = _gen(17, C)
    gam = torch.randn(C, generator=g) * 0.3 + 1.0
    w_ff1 = torch.randn(8 * C, C, generator=g) * C ** -0.5
    b_ff1 = torch.randn(8 * C, generator=g) * 0.1
    w2 = torch.cat([torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5, torch.randn(C, C, generator=g) * C ** -0.5], 1).to(dtype)
    bias2 = torch.randn(C, generator=g) * 0.1
    inv = torch.argsort(quad_perm(8 * C))                      # [values | gates] rows -> interleaved quads
    w1 = (w_ff1 * gam[None, :])[inv].to(dtype).contiguous()
    b1 = b_ff1[inv].contiguous()
    cs1 = w1.double().sum(1).float()
    S, Q, _ = row_tile_sums(hs, C // tiles)
    return dict(hs=hs, w1=w1, b1=b1, cs1=cs1, w2=w2.contiguous(), bias2=bias2, st=torch.stack([S, Q], -1).float().contiguous())


def build_gemm_case(M: int, N: int, K: int, dtype, key=0):
    g = _gen(11, M, N, K, key)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    return x, w, torch.randn(N, generator=g), torch.randn(M, N, generator=g).to(dtype)


# ------------------------------------------------------------------------------------------------ the emulations
F32 = np.float32


def _np(t) -> np.ndarray:
    return t.float().numpy().astype(F32)


def _seq_sum(a: np.ndarray, axis: int) -> np.ndarray:
    """left-to-right fp32 sum along `axis` (np.sum is pairwise)"""
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], F32)
    for i in range(a.shape[0]):
        s = (s + a[i]).astype(F32)
    return s


def _concat_as_read(x1: np.ndarray, x2, defect):
    """[B, hw, C] as the kernels address it; x2_read_with_c1_stride: pixel p of x2 starts at p * c1 of its batch item"""
    if x2 is None:
        return x1
    B, hw, c1 = x1.shape
    c2 = x2.shape[2]
    if defect == "x2_read_with_c1_stride":
        flat = x2.reshape(-1)
        idx = (np.arange(B)[:, None, None] * hw * c2 + np.arange(hw)[None, :, None] * c1 + np.arange(c2)[None, None, :])
        x2 = flat[idx % flat.size]
    return np.concatenate([x1, x2], 2)


def emu_gn_stats(x1, x2, groups: int, defect=None) -> np.ndarray:
    """gn_stats_kernel: fp32 partials [B, nchunk, groups, 2]"""
    x = _concat_as_read(x1, x2, defect)
    B, hw, C = x.shape
    S, P, nchunk, per, _, _ = gn_launch(hw, C)
    if defect == "per_floor":
        per = max(1, hw // nchunk)
    cg = C // groups
    out = np.zeros((B, nchunk, groups, 2), F32)
    for chunk in range(nchunk):
        p0, p1 = chunk * per, min(chunk * per + per, hw)
        if p0 >= p1 or (defect == "last_chunk_dropped" and chunk == nchunk - 1):
            continue
        s, q = np.zeros((B, P, C), F32), np.zeros((B, P, C), F32)
        for i in range((p1 - p0 + P - 1) // P):
            p = p0 + i * P + np.arange(P)
            v = x[:, np.minimum(p, hw - 1), :] * (p < p1)[None, :, None].astype(F32)
            s = (s + v).astype(F32)
            q = (q + (v * v).astype(F32)).astype(F32)
        for k, t in enumerate((s, q)):
            tg = t.reshape(B, P, groups, cg).transpose(0, 2, 1, 3).reshape(B, groups, P * cg)
            out[:, chunk, :, k] = _seq_sum(tg, 2)
    return out


def _round16(r: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(r)).to(dtype)


def emu_gn_apply(x1, x2, groups: int, gamma, beta, eps: float, silu: bool, dtype, partial=None, acc=None, defect=None):
    """gn_fold / gn_fold_acc + gn_apply_kernel -> [B, hw, C] in `dtype`; rows a defect leaves unwritten stay 0"""
    x = _concat_as_read(x1, x2, defect)
    B, hw, C = x.shape
    c1 = x1.shape[2]
    cg = C // groups
    if acc is not None:
        a = acc.astype(np.float64)
        ssc, qsc = (SQ_SCALE, SUM_SCALE) if defect == "acc_scales_swapped" else (SUM_SCALE, SQ_SCALE)
        s, q = a[..., 0] / ssc, a[..., 1] / qsc
    else:
        s, q = partial[..., 0].astype(np.float64).sum(1), partial[..., 1].astype(np.float64).sum(1)
    n = float(hw) * float((c1 if defect == "n_counts_c1_only" else C) // groups)
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0.0)
    mean32, rstd32 = mean.astype(F32), (1.0 / np.sqrt(var + float(F32(eps)))).astype(F32)
    ch = np.arange(C)
    gg = ((ch // 8 * 8) if defect == "slot_group_from_first_channel" else ch) // cg
    sc = (rstd32[:, gg] * gamma[None, :]).astype(F32)                                  # [B, C]
    sh = (beta[None, :] - (mean32[:, gg] * sc).astype(F32)).astype(F32)
    r = ((x * sc[:, None, :]).astype(F32) + sh[:, None, :]).astype(F32)
    if silu:
        with np.errstate(over="ignore"):                   # (exp2 -> inf, rcp -> 0: the kernel's arithmetic for large -x)
            e = np.exp2((r * F32(-1.44269504088896340736)).astype(F32)).astype(F32)
        r = (r * (F32(1.0) / (F32(1.0) + e)).astype(F32)).astype(F32)
    _, _, _, _, R, nb = gn_launch(hw, C)
    if R and defect in ("tail_loop_rows_skipped", "fourth_prefetched_row_dropped"):
        k = np.arange(hw) // (nb * R)
        r[:, (k >= 4) if defect == "tail_loop_rows_skipped" else (k == 3), :] = 0.0
    return _round16(r, dtype)


def emu_epilogue_acc(t: np.ndarray, rows_per_batch: int, subs, block_rows: int, tile_rows: int, defect=None):
    """The epilogue accumulators of a stored output t [M, N] fp32: one add per (row block of `block_rows` rows, column) into
    the group's fixed-point slot; row blocks lie inside tiles of `tile_rows` rows.  -> one int64 [B, groups, 2] per
    subscription (cg, c0, groups)."""
    M, N = t.shape
    B = M // rows_per_batch
    accs = [np.zeros((B, groups, 2), np.int64) for (_, _, groups) in subs]
    ssc, qsc = (SQ_SCALE, SUM_SCALE) if defect == "acc_scales_swapped" else (SUM_SCALE, SQ_SCALE)
    for tile_m0 in range(0, M, tile_rows):
        for m0 in range(tile_m0, min(tile_m0 + tile_rows, M), block_rows):
            rows = t[m0:min(m0 + block_rows, M)]
            b = (tile_m0 if defect == "batch_from_tile_start" else m0) // rows_per_batch
            for n_blk in range(0, N, 160):
                ncols = min(160, N - n_blk)
                if defect == "ragged_column_tile_dropped" and ncols < 160:
                    continue
                blk = rows[:, n_blk:n_blk + ncols]
                sm, sq = _seq_sum(blk, 0), _seq_sum((blk * blk).astype(F32), 0)
                fs = np.rint(sm.astype(np.float64) * ssc).astype(np.int64)
                fq = np.rint(sq.astype(np.float64) * qsc).astype(np.int64)
                for acc, (cg, c0, _) in zip(accs, subs):
                    gi = (c0 + n_blk + np.arange(ncols)) // cg
                    np.add.at(acc[b, :, 0], gi, fs)
                    np.add.at(acc[b, :, 1], gi, fq)
    return accs


def emu_row_stats(t: np.ndarray, defect=None) -> np.ndarray:
    """The row_stats_out producer on a stored output t [M, N] fp32 -> [M, tiles, 2] fp32"""
    M, N = t.shape
    tiles = (N + 159) // 160
    out = np.zeros((M, tiles, 2), F32)
    for ti in range(tiles):
        ncols = min(160, N - ti * 160)
        if defect == "ragged_column_tile_dropped" and ncols < 160:
            continue
        blk = t[:, ti * 160:ti * 160 + ncols].reshape(M, ncols // 8, 4, 2)
        pair = (blk[..., 0] + blk[..., 1]).astype(F32)
        pairq = ((blk[..., 0] * blk[..., 0]).astype(F32) + (blk[..., 1] * blk[..., 1]).astype(F32)).astype(F32)
        out[:, ti, 0] = _seq_sum(_seq_sum(pair, 2), 1)
        out[:, ti, 1] = _seq_sum(_seq_sum(pairq, 2), 1)
    return out


def _butterfly(v: np.ndarray) -> np.ndarray:
    """wave_sum over the last axis (64 lanes)"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(F32)
    return v[..., :1]


def emu_layernorm(x: np.ndarray, gamma, beta, eps: float, dtype, defect=None) -> torch.Tensor:
    """layernorm_kernel on x [rows, C] fp32 -> [rows, C] in `dtype`; what a defect leaves unwritten stays 0"""
    rows, C = x.shape
    S = C // 8
    NP = ln_np(C)
    if defect == "np_one_too_small":
        NP = max(1, NP - 1)
    v = np.zeros((rows, NP * 64 * 8), F32)
    live = min(C, NP * 512)
    v[:, :live] = x[:, :live]
    v = v.reshape(rows, NP, 64, 8).transpose(0, 2, 1, 3).reshape(rows, 64, NP * 8)     # [row][lane][piece i, element j]
    mask = (np.arange(NP)[None, :, None] * 64 + np.arange(64)[:, None, None] < S)       # [lane][i][1]: piece inside the row
    mask = np.broadcast_to(mask, (64, NP, 8)).reshape(64, NP * 8)
    mean = (_butterfly(_seq_sum(v, 2)) / F32(C)).astype(F32)                           # [rows, 1]
    d = ((v - mean[:, :, None]).astype(F32) * mask[None]).astype(F32)
    sq = _butterfly(_seq_sum((d * d).astype(F32), 2))
    rstd = (F32(1.0) / np.sqrt(((sq / F32(C)).astype(F32) + F32(eps)).astype(F32))).astype(F32)
    dn = d.reshape(rows, 64, NP, 8).transpose(0, 2, 1, 3).reshape(rows, NP * 512)[:, :live]
    r = np.zeros((rows, C), F32)
    r[:, :live] = (((dn * rstd).astype(F32) * gamma[None, :live]).astype(F32) + beta[None, :live]).astype(F32)
    if defect == "ln_last_block_skipped" and rows % 4:
        r[rows // 4 * 4:] = 0.0
    return _round16(r, dtype)


def _mm32(x: torch.Tensor, w: torch.Tensor, step: int = 32) -> np.ndarray:
    """x w^T with an fp32 accumulator rounded after every `step` products of the contraction (the MFMA steps in order)"""
    xd, wd = x.double(), w.double()
    acc = np.zeros((x.shape[0], w.shape[0]), F32)
    for k0 in range(0, x.shape[1], step):
        acc = (acc + (xd[:, k0:k0 + step] @ wd[:, k0:k0 + step].t()).numpy().astype(F32)).astype(F32)
    return acc


def emu_folded_ln(x, w16, cs, t, st, eps: float, ln_dim: int, dtype, geglu: bool = False, defect=None, raw: bool = False):
    """pp_gemm_bf16(ln_stats): the fp32 one-pass moments and the corrected epilogue.  x [M, K], w16 [N, K] 16-bit tensors,
    cs / t [N] fp32, st [M, tiles, 2] fp32 -> [M, N] (GEGLU: [M, N / 2]) in `dtype` (raw: the fp32 values, unrounded)"""
    stn = st.numpy()
    s, q = _seq_sum(stn[..., 0], 1), _seq_sum(stn[..., 1], 1)
    inv = F32(1.0) / F32(160 if defect == "folded_ln_dim_is_one_tile" else ln_dim)
    mean = (s * inv).astype(F32)
    var = ((q * inv).astype(F32) - (mean * mean).astype(F32)).astype(F32)
    rstd = (F32(1.0) / np.sqrt((np.maximum(var, F32(0.0)) + F32(eps)).astype(F32))).astype(F32)
    acc = _mm32(x, w16)
    csn, tn = cs.numpy().astype(F32), t.numpy().astype(F32)
    corr = (csn[None, :] * mean[:, None]).astype(F32)
    if defect == "folded_cs_mean_dropped":
        corr = corr * F32(0.0)
    v = (((acc - corr).astype(F32) * rstd[:, None]).astype(F32) + tn[None, :]).astype(F32)
    if geglu:
        h = v.shape[1] // 2
        g = torch.from_numpy(v[:, h:].astype(np.float64))
        v = (v[:, :h] * gelu64(g).numpy().astype(F32)).astype(F32)
    return v if raw else _round16(v, dtype)


def emu_ff_fused(k, eps: float, dtype, defect=None) -> torch.Tensor:
    """pp_ff_fused on a build_ff_case: the folded-LayerNorm GEGLU rounded to 16 bits, then one fp32 GEMM over [act | hs]"""
    C = k["hs"].shape[1]
    perm = quad_perm(k["w1"].shape[0])
    act = emu_folded_ln(k["hs"], k["w1"][perm], k["cs1"][perm], k["b1"][perm], k["st"], eps, C, dtype, geglu=True, defect=defect)
    out = torch.from_numpy(_mm32(torch.cat([act, k["hs"]], 1), k["w2"])) + k["bias2"]
    return out.to(dtype)


# ------------------------------------------------------------------------------------------------ pp_tfront, pp_xattn_block
TF_B, TF_HW, TF_C = 1, 128, 320              # the smallest shape pp_tfront accepts
XA_B, XA_HW, XA_NCTX, XA_C = 2, 128, 7, 320  # ... and pp_xattn_block (one 128-row tile per batch item)


def build_tfront_case(regime: str, dtype, B: int = TF_B, hw: int = TF_HW, groups: int = 32):
    """x [B, hw, 320] of the regime; proj_in chosen so that the rows of hs -- what LayerNorm1 sees -- are in the regime
    too: offset16 adds 16 to its bias (hs has unit spread), outlier multiplies one output channel by 100."""
    C = TF_C
    x = build_x(regime, dtype, B, hw, C, groups, 0.0, key=4)
    g = _gen(19, C)
    gg, gb = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    w1, b1 = torch.randn(C, C, generator=g) * C ** -0.5, torch.randn(C, generator=g) * 0.1
    if regime == "offset16":
        b1 = b1 + 16.0
    if regime == "outlier":
        w1[C // 2 + 3] *= 100.0
        b1[C // 2 + 3] *= 100.0
    g1, be1 = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    wqkv = torch.randn(3 * C, C, generator=g) * C ** -0.5
    wf = (wqkv * g1[None, :]).to(dtype).contiguous()
    return dict(x=x, gg=gg, gb=gb, w1=w1.to(dtype).contiguous(), b1=b1, wf=wf, cs=wf.double().sum(1).float(),
                tb=(wqkv @ be1).contiguous())


def _kernel_moments(h16: torch.Tensor) -> torch.Tensor:
    """[M, 1, 2] fp32 (sum, sum of squares) of stored rows, summed in fp32 in sequence"""
    v = _np(h16)
    return torch.from_numpy(np.stack([_seq_sum(v, 1), _seq_sum((v * v).astype(F32), 1)], -1)[:, None, :])


def emu_tfront(k, dtype, defect=None):
    """-> (hs, qkv [M, 960]) in `dtype`"""
    x = k["x"]
    n16 = emu_gn_apply(_np(x), None, 32, k["gg"].numpy(), k["gb"].numpy(), 1e-6, False, dtype, acc=build_acc(x, None, 32).numpy())
    hs = _round16((_mm32(n16.reshape(-1, TF_C), k["w1"]) + k["b1"].numpy()[None, :]).astype(F32), dtype)
    qkv = emu_folded_ln(hs, k["wf"], k["cs"], k["tb"], _kernel_moments(hs), 1e-5, TF_C, dtype, defect=defect)
    return hs, qkv


def build_xattn_case(regime: str, dtype, B: int = XA_B, hw: int = XA_HW, nctx: int = XA_NCTX, C: int = XA_C, tiles: int = 0):
    """x [B hw, C] of the regime and the folded matrices of a cross-attention over nctx context tokens, folded in fp64 and
    rounded once: gt [B, 640, C] (logit weights, LayerNorm's gamma inside, exp2 domain), gcs = column sums of the stored gt,
    gbias (-inf on the empty key slots), ht [B, C, 640] in the k-permuted order of pp_xattn_fold; st: the row moments in
    `tiles` partials per row (default C / 160)."""
    H = XA_HEADS
    d = C // H
    M = B * hw
    x = build_x(regime, dtype, M, 1, C, 1, 0.0, key=5).reshape(M, C)
    g = _gen(23, C)
    g2, b2 = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    wq = torch.randn(C, C, generator=g, dtype=torch.float64) * C ** -0.5
    wo = (torch.randn(C, C, generator=g) * C ** -0.5).to(dtype).double()
    kc = torch.randn(B, nctx, H, d, generator=g).to(dtype).double()
    vc = torch.randn(B, nctx, H, d, generator=g).to(dtype).double()
    wqf = (wq * g2.double()[None, :]).to(dtype).double().reshape(H, d, C)
    qs = d ** -0.5 * 1.4426950408889634
    gt = torch.zeros(B, H, XA_KP, C, dtype=torch.float64)
    gt[:, :, :nctx] = torch.einsum("bkhd,hdc->bhkc", kc, wqf) * qs
    gt = gt.reshape(B, H * XA_KP, C).to(dtype).contiguous()
    gb = torch.full((B, H, XA_KP), -math.inf)
    gb[:, :, :nctx] = (torch.einsum("bkhd,hd->bhk", kc, (wq @ b2.double()).reshape(H, d)) * qs).float()
    hfull = torch.zeros(B, C, H, XA_KP, dtype=torch.float64)
    hfull[..., :nctx] = torch.einsum("nhd,bkhd->bnhk", wo.reshape(C, H, d), vc)
    ht = hfull.reshape(B, C, H * XA_KP).to(dtype)[:, :, xattn_kk()].contiguous()
    S, Q, _ = row_tile_sums(x, C // tiles if tiles else 160)
    return dict(x=x, gt=gt, gcs=gt.double().sum(-1).float().contiguous(), gb=gb.reshape(B, H * XA_KP).contiguous(), ht=ht,
                bo=torch.randn(C, generator=g) * 0.1, st=torch.stack([S, Q], -1).float().contiguous())


def emu_xattn_block(k, dtype, defect=None) -> torch.Tensor:
    M, C = k["x"].shape
    kk = xattn_kk()
    out = torch.empty(M, C, dtype=dtype)
    for b in range(XA_B):
        r = slice(b * XA_HW, (b + 1) * XA_HW)
        l = emu_folded_ln(k["x"][r], k["gt"][b], k["gcs"][b], k["gb"][b], k["st"][r], 1e-5, C, dtype, defect=defect, raw=True)
        l = l.reshape(XA_HW, XA_HEADS, XA_KP)
        e = np.exp2((l - l.max(-1, keepdims=True)).astype(F32)).astype(F32)
        p = _round16((e * (F32(1.0) / _seq_sum(e, 2))[..., None]).astype(F32).reshape(XA_HW, -1), dtype)
        o = _mm32(p[:, kk], k["ht"][b])
        out[r] = _round16((o + k["bo"].numpy()[None, :] + _np(k["x"][r])).astype(F32), dtype)
    return out
