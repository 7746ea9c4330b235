"""Shared by the probe tests of the fused transformer kernels (not a test file): the case matrix of pp_ff_fused (4-wave and
8-wave form), pp_tfront, pp_xattn_block (plain, pre_w, src_wrap_rows, the wide kernel at C = 640 / 1280) and pp_xattn_fold,
built on the CPU; fp64 references; derived gates (tests/norm_cases.py, extended, not duplicated); a NumPy restatement of each
kernel's index walk with named defects.  Nothing here touches the HIP library.

Probe E -- integers, bit equality.  Every operand is a small integer or a power of two, so every intermediate is exact in fp32
and in the 16-bit format; `build` asserts that on the fp64 reference of every case (`_exact16`).
  pp_ff_fused   ln_stats NULL (mean 0, rstd 1).  The gate rows of W1 are zero and the gate bias is +16 (open unit) or -16:
                exp2f(-16^2 / 2 log2 e) = 2^-184.7 underflows to 0 in fp32, so gelu_fast(16) = 16 and gelu_fast(-16) = 0
                exactly and act = 16 h on open units, +-0 elsewhere.  W2a = +-2^-4 on four output columns per hidden unit
                (the columns identify the unit), W_po two entries per row, every sum below 2^8.  OPEN: which units are open.
  pp_tfront     gn_acc is an input and is trusted: built by hand with sum 0 and q / n + eps within 2^-21 / n of 4^-k, k = 0, 1 per
                (item, group), so that (float)(1 / sqrt(var + eps)) = 2^k (asserted); gamma = +-1, +-2, beta an integer:
                the normalised row and hs are integers, hs is held to bit equality.  Q, K, V carry the in-kernel rstd (not
                exact): integer weights under gate_tfront_qkv from the hs the kernel stored -- a misplaced index moves a
                value by whole units, the gate is a fraction of a 16-bit ulp.
  pp_xattn_block / wide kernel   hand-made gt, gcs, gbias, ht, ln_stats NULL.  A row carries 32 on ONE `signal` channel (and
                small integers on the others, which gt does not see); gt = 32 on the winning keys of (item, head, channel),
                gbias = 0 on the base keys of (item, head), -512 on the other live keys, -inf on the padded ones; key sets
                are aligned dyadic blocks of 1, 2 or 4 keys, so the set of maximal logits has k = 1, 2 or 4 members and
                every other logit is lower by >= 512 (asserted for all (row, head): exp2 underflows to 0 below -149).  The
                probabilities are exactly 1 / k, ht holds multiples of 4: the output is an exact mean of identified H^T
                columns + bias_o + the residual.  Every seventh row is all noise: its winners are the base keys, which a
                padded key with an unmasked bias would join.  With pre_w, x is one-hot and pre_w = 32 P routes it to a signal
                channel; pre_b and res live on the other channels.
  pp_xattn_fold K, V, wq, wo integers.  ht bit-equal in the three layouts; gt / gbias bit-equal to round16(fl32(fl32(sum) qscale))
                evaluated in NumPy float32 (the integer sum is exact in any order); gcs = 0 without q_colsum, else within
                (C / 64 + 6) u32 sum|gt| of the sum of the STORED row (a lane adds C / 128 pair sums, six butterfly adds);
                padded keys: gt = 0, gbias = -inf, ht column 0.

Probe R -- Gaussian data under a derived gate (norm_cases: gate_ff_fused, gate_tfront_hs / _qkv, gate_xattn_block): the folded
LayerNorm with ln_tiles 1, 2, 5, q_scale != 1, real GELU arguments, softmax with close logits.  Assumed (not derived) hardware
bounds, as profiles/small_exact_achieved.txt states its own: v_rcp_f32, v_exp_f32 1 ulp, v_rsq_f32 / rsqrtf 4 u32 (2 ulp + the
operand's rounding), gelu_fast_f within 2^-20 |g| of gelu (norm_cases).  The row moments of pp_xattn_block: a lane folds 10
blocks (three adds and one accumulation each) and two shuffle adds: 42 u32 sum|x|, 43 u32 Q (`gate_row_stats_xattn`).
pre_w: h = round16(x pre_w^T + pre_b + res) is parked in `out` and overwritten, but a second launch with H^T = 0 and no bias
returns exactly it (out = round16(0 + h)): h is held to its own GEMM gate (u |h| + (C + 2) u32 A), and the output to
gate_xattn_block evaluated FROM that h with the in-kernel moments (kernel_moments_eps) -- no rounding has to be carried through
the softmax.  E cases hold h to bit equality the same way.

The walk (`walk`) restates per kernel: the XCD remap, the batch index of a tile, the piece / slab order and the ring stage a
step reads, the pack-time permutations, the peeled tail, the epilogue passes.  DEFECTS names what it can get wrong.  (The batch index taken from a tile's LAST row is no defect: a tile
never straddles two items, rows_per_batch is a multiple of the tile height or the request is refused; `batch_of_tile_end` takes
it from the row behind the tile.)
"""
import math

import numpy as np
import torch

import gemm_cases as GC
import norm_cases as NC

U32, F32 = NC.U32, np.float32
DTYPES = NC.DTYPES
Buf, lay = GC.Buf, GC.lay
GUARD = 2
LOG2E = 1.4426950408889634
LOG2E_F = float(F32(1.44269504088896340736))
PP_OK, PP_ERR_BAD_ARG, PP_ERR_UNSUPPORTED = 0, -1, -2
C320, HID, HEADS, KP, S640 = 320, 1280, 8, 80, 640
SENT16, SENT32, SENT64 = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GRIDS = (1, 2, 3, 7, 8, 9, 17)

DEFECTS = (
    "stale_ring_stage", "drop_t2_chunk37", "dup_t2_chunk38", "drop_t2_chunk39", "drop_tail0", "dup_tail4", "drop_tail5",
    "drop_tail9", "last_geglu_other_parity", "kperm_geglu_identity", "geglu_interleave_identity", "geglu_interleave_inverse",
    "kperm_identity", "kperm_inverse", "quad_h_g_swapped", "wpo_offset_32", "remap_q_off_by_one", "remap_r_off_by_one",
    "batch_of_tile_end", "gn_stats_of_item0", "groups_as_c_over_10", "q_scale_on_k", "vt_at_p0_zero", "res1_wrap_per_tile",
    "scale_after_residuals", "gn_halves_not_split", "ff8_exchange_halves_swapped", "heads47_tables_of_03", "padded_not_masked",
    "wrap_on_parked_h", "row_stats_split_128", "wide_ht_group_offset_dropped", "fold_ht_layout_natural", "fold_padded_not_masked",
)


class Case:
    def __init__(self, kernel, probe, name, **p):
        self.kernel, self.probe, self.p = kernel, probe, p
        self.id = f"{kernel}-{probe}-{name}"

    def __repr__(self):
        return self.id


# ------------------------------------------------------------------------------------------------ the pack-time permutations
def kperm_idx(K: int) -> torch.Tensor:
    """engine._kperm: storage position 8 kg + j of a group of 32 holds index 16 (j >> 2) + 4 kg + (j & 3)"""
    kp = torch.arange(K)
    s32, kg, j = kp // 32, (kp // 8) % 4, kp % 8
    return 32 * s32 + 16 * (j // 4) + 4 * kg + (j % 4)


def kperm_geglu_idx(K: int) -> torch.Tensor:
    """engine._kperm_geglu: storage position 8 kg + 2 q + e holds unit 8 q + 2 kg + e (an involution)"""
    sp = torch.arange(K)
    s32, r = sp // 32, sp % 32
    kg, q, e = r // 8, (r // 2) % 4, r % 2
    return 32 * s32 + 8 * q + 2 * kg + e


def geglu_interleave_idx(F2: int) -> torch.Tensor:
    """engine._geglu_interleave: interleaved row 4 q + i holds row (2 q, 2 q + 1, F + 2 q, F + 2 q + 1)[i] of [h ; g]"""
    F = F2 // 2
    q = torch.arange(F // 2)
    return torch.stack([2 * q, 2 * q + 1, F + 2 * q, F + 2 * q + 1], 1).reshape(-1)


def remap(bid: int, nwg: int, defect=None) -> int:
    """the XCD remap of every kernel here: block bid runs on XCD bid % 8; consecutive tiles share an XCD"""
    q, r = nwg >> 3, nwg & 7
    if defect == "remap_q_off_by_one":
        q += 1
    if defect == "remap_r_off_by_one":
        r += 1
    xcd, idx = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


# ------------------------------------------------------------------------------------------------ memory
def out16(rows, cols, pad, dtype, guard=GUARD) -> Buf:
    return GC.sentinel_out(rows, cols, pad, dtype, guard)


def out_i64(rows, cols, guard=1) -> Buf:
    """zeroed accumulators (the kernels ADD) between sentinel rows"""
    full = torch.full(((rows + 2 * guard) * cols,), SENT64, dtype=torch.int64)
    b = Buf(full, guard * cols, rows, cols, cols)
    b.view.zero_()
    return b


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def outside_clean(b: Buf) -> bool:
    sent = {2: SENT16, 4: SENT32, 8: SENT64}[b.full.element_size()]
    return bool((bits(b.full)[b.outside()] == sent).all())


def emu_like(b: Buf) -> Buf:
    """the emulation's twin of an output window: fp64, NaN = never stored"""
    return Buf(torch.full((b.full.numel(),), math.nan, dtype=torch.float64), b.base, b.rows, b.cols, b.ld)


def _inp(data: torch.Tensor, pad: int, dtype) -> Buf:
    """a strided input: NaN in the pad columns and in the guard rows"""
    return lay(data.to(dtype), pad, GUARD, GUARD, math.nan)


def _gen(*key):
    return NC._gen(*key)


def _sparse(g, shape, p, hi=1):
    m = (torch.rand(*shape, generator=g) < p).double()
    v = torch.randint(1, hi + 1, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    return m * v


def _exact16(v: torch.Tensor, dtype, what, lim=None):
    assert bool((v.to(dtype).double() == v).all()), (what, "must be representable in the format", float(v.abs().max()))
    if lim is not None:
        assert float(v.abs().max()) <= lim, (what, float(v.abs().max()))


def r16(a, dtype) -> np.ndarray:
    """fp32 array -> rounded once to the format (to nearest even) -> fp32"""
    a = np.ascontiguousarray(a, dtype=F32)
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(F32)
    b = a.view(np.uint32)
    r = ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)).view(F32)
    return np.where(np.isfinite(a), r, a)


def _mm(a: np.ndarray, w: np.ndarray) -> np.ndarray:
    """a [M, k] w [N, k]^T: fp64 products and sum, rounded once to fp32 (a piece of the contraction)"""
    if a.dtype != np.float64:
        a = a.astype(np.float64)
    if w.dtype != np.float64:
        w = w.astype(np.float64)
    return (a @ w.T).astype(F32)


def _np(t) -> np.ndarray:
    return t.float().numpy().astype(F32) if t.dtype != torch.float64 else t.numpy().astype(F32)


# ================================================================================================ pp_ff_fused
FF_OPEN = ("single", "chunk", "ends", "all")


def ff_open_units(kind: str) -> torch.Tensor:
    o = torch.zeros(HID, dtype=torch.bool)
    if kind == "single":
        o[[0, 31, 33, 37 * 32 + 5, 38 * 32 + 30, 1279]] = True
    elif kind == "chunk":
        o[17 * 32:18 * 32] = True
    elif kind == "ends":
        o[:32] = True
        o[36 * 32:] = True
    else:
        o[:] = True
    return o


def _ff_cases():
    cs = []

    def add(probe, name, **p):
        d = dict(M=128, rpb=0, open="all", fold=False, tiles=2, bias=True, scale=1.0, res1=False, res2=False, wrap=0, gn=(),
                 pad=(8, 16, 24, 40), regime="zero")
        d.update(p)
        cs.append(Case("ff", probe, name, **d))
    for kind in FF_OPEN:
        add("E", f"open-{kind}", open=kind, res1=True)
    for t in GRIDS[1:]:
        add("E", f"grid{t}", M=128 * t, open="ends", res2=True)
    add("E", "contiguous", M=256, pad=(0, 0, 0, 0), res1=True, res2=True, open="ends")
    add("E", "nobias", bias=False, open="chunk")
    add("E", "scale2-res12", open="ends", scale=2.0, res1=True, res2=True)
    add("E", "scale-half", open="chunk", scale=0.5, res1=True)
    add("E", "wrap64", M=128, open="ends", res1=True, wrap=64)
    add("E", "wrap128", M=256, open="ends", res1=True, res2=True, wrap=128)
    add("E", "wrap-half", M=768, open="ends", res1=True, wrap=384)
    add("E", "wrap-short", M=384, open="ends", res1=True, wrap=256)
    for cg, c0, G in ((8, 0, 40), (10, 0, 32), (16, 0, 20), (20, 0, 16), (40, 0, 8), (10, 320, 64), (20, 310, 32), (8, 4, 41),
                      (40, 20, 9)):
        add("E", f"gn-cg{cg}-c0{c0}", M=256, rpb=128, open="ends", gn=((cg, c0, G),), res1=True)
    add("E", "gn-two", M=384, rpb=128, open="ends", gn=((10, 0, 32), (20, 320, 32)), res2=True)
    add("E", "gn-rpb256", M=768, rpb=256, open="ends", gn=((10, 0, 32), (16, 8, 21)))
    add("E", "gn-rpb384-wrap", M=768, rpb=384, open="ends", gn=((20, 320, 32),), res1=True, wrap=384)
    for tiles in (1, 2, 5):
        add("R", f"ln-tiles{tiles}", fold=True, tiles=tiles, M=256, res1=True)
    add("R", "ln-offset16", fold=True, regime="offset16", res2=True)
    add("R", "ln-outlier", fold=True, regime="outlier")
    add("R", "plain", M=384, scale=0.75, res1=True, res2=True)
    add("R", "plain-gn-wrap", M=512, rpb=256, gn=((10, 0, 32), (20, 320, 32)), res1=True, wrap=256)
    add("R", "ln-contiguous", fold=True, M=1152, pad=(0, 0, 0, 0), res1=True)
    return cs


def build_ff(c: Case, dtype):
    p = c.p
    M, C = p["M"], C320
    wrap = p["wrap"]
    g = _gen(41, M, len(p["gn"]), int(p["scale"] * 4), wrap, FF_OPEN.index(p["open"]))
    il = geglu_interleave_idx(2 * HID)
    t = dict(M=M, probe=c.probe)
    if c.probe == "E":
        hs = GC._ensure_blocks(_sparse(g, (M, C), 0.25))
        w1h = _sparse(g, (HID, C), 0.5)
        opn = ff_open_units(p["open"])
        b1n = torch.cat([torch.randint(-2, 3, (HID,), generator=g).double(), torch.where(opn, 16.0, -16.0).double()])
        w1n = torch.cat([w1h, torch.zeros(HID, C, dtype=torch.float64)])
        w2a = torch.zeros(C, HID, dtype=torch.float64)
        u = torch.arange(HID)
        for j in range(4):
            w2a[(3 * u + 107 * j + 11) % C, u] = (torch.randint(0, 2, (HID,), generator=g).double() * 2 - 1) / 16.0
        w2b = torch.zeros(C, C, dtype=torch.float64)
        n = torch.arange(C)
        w2b[n, (7 * n + 3) % C] = 1.0
        w2b[n, (11 * n + 5) % C] = -1.0
        w2 = torch.cat([w2a, w2b], 1)
        bias2 = torch.randint(-3, 4, (C,), generator=g).double()
        res = [torch.randint(-4, 5, (wrap or M, C), generator=g).double(), torch.randint(-4, 5, (M, C), generator=g).double()]
        cs1 = None
        st = None
    else:
        k = NC.build_ff_case(p["regime"], dtype, M=M, tiles=p["tiles"])
        hs, w2, bias2 = k["hs"].double(), k["w2"].double(), k["bias2"].double()
        w1i, b1i = k["w1"].double(), k["b1"].double()
        inv = torch.argsort(il)
        w1n, b1n = w1i[inv], b1i[inv]                     # (back to [h ; g] order; re-interleaved below)
        cs1, st = (k["cs1"], k["st"]) if p["fold"] else (None, None)
        res = [torch.randn(wrap or M, C, generator=g).to(dtype).double(), torch.randn(M, C, generator=g).to(dtype).double()]
    if not p["bias"]:
        bias2 = None
    res1 = res[0] if p["res1"] else None
    res2 = res[1] if p["res2"] else None
    w1 = w1n[il].to(dtype).contiguous()
    b1 = b1n[il].float().contiguous()
    if cs1 is not None:
        cs1 = w1.double().sum(1).float().contiguous()
    w2_16 = w2.to(dtype).contiguous()
    w2kp = torch.cat([w2_16[:, :HID][:, kperm_geglu_idx(HID)], w2_16[:, HID:]], 1).contiguous()
    px, po, p1, p2 = p["pad"]
    t["inp"] = dict(hs=_inp(hs, px, dtype), res1=_inp(res1, p1, dtype) if res1 is not None else None,
                    res2=_inp(res2, p2, dtype) if res2 is not None else None, w1=w1, b1=b1, cs1=cs1, w2=w2_16, w2kp=w2kp,
                    bias2=bias2.float().contiguous() if bias2 is not None else None, st=st)
    nb = M // p["rpb"] if p["rpb"] else 0
    t["out"] = dict(out=out16(M, C, po, dtype))
    for i, (cg, c0, G) in enumerate(p["gn"]):
        t["out"][f"acc{i}"] = out_i64(nb, G * 2)
    # ---- the reference
    r1w = torch.cat([res1, res1[:M - wrap]]) if (res1 is not None and wrap) else res1
    rs = [r for r in (r1w, res2) if r is not None]
    if c.probe == "E":
        hd = hs
        h = hd @ w1n[:HID].t() + b1n[:HID]
        gl = hd @ w1n[HID:].t() + b1n[HID:]
        assert bool((gl.abs() == 16.0).all()) and bool(((gl > 0) == opn[None, :]).all()), (c.id, "the open-unit pattern")
        act = h * NC.gelu64(gl)
        assert bool((act == torch.where(opn[None, :], 16.0 * h, torch.zeros_like(h))).all()), (c.id, "gelu(+-16) in fp64")
        _exact16(act, dtype, (c.id, "act"))
        acc = act @ w2[:, :HID].t() + hd @ w2[:, HID:].t()
        A = act.abs() @ w2[:, :HID].abs().t() + hd.abs() @ w2[:, HID:].abs().t()
        assert float(A.max()) < 2.0 ** 24 and float((hd.abs() @ w1n[:HID].abs().t()).max()) < 2.0 ** 24
        ref = (acc + (bias2 if bias2 is not None else 0.0)) * p["scale"] + sum(rs, torch.zeros_like(acc))
        _exact16(ref, dtype, (c.id, "out"), 256.0)
        assert GC.gn_partials_exact(ref)
        t["ref"] = dict(out=ref)
        stored = ref
        for i, (cg, c0, G) in enumerate(p["gn"]):
            t["ref"][f"acc{i}"] = GC.gn_expected(stored, p["rpb"], cg, c0, G).reshape(nb, G * 2)
    else:
        ref, gate = NC.gate_ff_fused(hs.to(dtype), w1, b1, cs1, w2_16, bias2, 1e-5, dtype, tiles=p["tiles"], fold=p["fold"],
                                     scale=p["scale"], res=rs)
        t["ref"] = dict(out=(ref, gate))
    return t


FF_PIECES = ([("T1", 0, 0), ("T1", 0, 1)] + [pc for c in range(1, 40) for pc in (("T1", c, 0), ("T1", c, 1), ("T2", c - 1, 0))]
             + [("TAIL", tt, 0) for tt in range(10)] + [("T2", 39, 0)])
assert len(FF_PIECES) == 130
FF_NS = 6


def gelu_fast(v: np.ndarray) -> np.ndarray:
    """gelu_fast_f of the kernels in NumPy float32 (Abramowitz-Stegun 7.1.26, exp2 domain): x Phi(x) = max(x, 0) - |x| p t e"""
    v = v.astype(F32)
    a = np.abs(v)
    tt = (F32(1.0) / (a * F32(0.3275911 * 0.70710678118654752440) + F32(1.0)).astype(F32)).astype(F32)
    pl = (tt * F32(0.5 * 1.061405429) + F32(0.5 * -1.453152027)).astype(F32)
    for k in (0.5 * 1.421413741, 0.5 * -0.284496736, 0.5 * 0.254829592):
        pl = (tt * pl + F32(k)).astype(F32)
    with np.errstate(under="ignore"):
        e = np.exp2(((v * v).astype(F32) * F32(-0.5 * 1.44269504088896340736)).astype(F32)).astype(F32)
    pl = ((pl * tt).astype(F32) * e).astype(F32)
    return (np.maximum(v, F32(0.0)) - (a * pl).astype(F32)).astype(F32)


def _geglu32(S, mean, rstd, b1c, cs1c):
    """64 interleaved columns (h0, h1, g0, g1) of a chunk -> 32 units (2 q + e), fp32"""
    v = ((S - cs1c[None, :] * mean[:, None]).astype(F32) * rstd[:, None]).astype(F32) + b1c[None, :]
    v = v.astype(F32).reshape(S.shape[0], 16, 4)
    return (v[:, :, :2] * gelu_fast(v[:, :, 2:])).astype(F32).reshape(S.shape[0], 32)


def walk_ff(c: Case, t, dtype, w8: bool, defect=None):
    """-> dict of emulated output buffers.  The 4-wave form takes W2' with the hidden index permuted (kperm_geglu) and chains the
    activations in registers; the 8-wave form takes it in natural order: each column half of a chunk (16 units) is written
    by one wave of a pair into the exchange tile and both read all 32."""
    p, i = c.p, t["inp"]
    M, C = p["M"], C320
    x = _np(i["hs"].view)
    w1, b1 = _np(i["w1"]), i["b1"].numpy()
    cs1 = i["cs1"].numpy() if i["cs1"] is not None else np.zeros(2 * HID, F32)
    w2s = _np(i["w2"] if w8 else i["w2kp"])
    if defect == "geglu_interleave_identity":             # W1 / b1 rows left in [h ; g] order
        inv = torch.argsort(geglu_interleave_idx(2 * HID)).numpy()
        w1, b1, cs1 = w1[inv], b1[inv], cs1[inv]
    if defect == "geglu_interleave_inverse":
        il = geglu_interleave_idx(2 * HID).numpy()
        w1, b1, cs1 = w1[il], b1[il], cs1[il]
    if i["st"] is not None:
        st = i["st"].numpy()
        s, q = NC._seq_sum(st[..., 0], 1), NC._seq_sum(st[..., 1], 1)
        mean = (s * F32(1.0 / C)).astype(F32)
        var = ((q * F32(1.0 / C)).astype(F32) - (mean * mean).astype(F32)).astype(F32)
        rstd = (F32(1.0) / np.sqrt((np.maximum(var, F32(0.0)) + F32(1e-5)).astype(F32))).astype(F32)
    else:
        mean, rstd = np.zeros(M, F32), np.ones(M, F32)
    kpg = kperm_geglu_idx(32).numpy()

    def piece_data(pc):
        kind, a, h = pc
        if kind == "T1":
            return w1[64 * a:64 * a + 64, 160 * h:160 * h + 160]
        if kind == "T2":
            return w2s[:, 32 * a:32 * a + 32]
        off = 32 if defect == "wpo_offset_32" else 0
        return w2s[:, HID + 32 * a + off:HID + 32 * a + off + 32] if HID + 32 * a + off + 32 <= HID + C else np.zeros((C, 32), F32)

    seq = list(FF_PIECES)
    for name, key, op in (("drop_t2_chunk37", ("T2", 37, 0), "drop"), ("dup_t2_chunk38", ("T2", 38, 0), "dup"),
                          ("drop_t2_chunk39", ("T2", 39, 0), "drop"), ("drop_tail0", ("TAIL", 0, 0), "drop"),
                          ("dup_tail4", ("TAIL", 4, 0), "dup"), ("drop_tail5", ("TAIL", 5, 0), "drop"),
                          ("drop_tail9", ("TAIL", 9, 0), "drop")):
        if defect == name:
            k = seq.index(key)
            seq = seq[:k] + ([key, key] if op == "dup" else []) + seq[k + 1:]
    ring = [None] * FF_NS
    S = {0: np.zeros((M, 64), F32), 1: np.zeros((M, 64), F32)}
    out = np.zeros((M, C), F32)
    pf = None

    def frag(act, ch):
        """the chunk's 32 activations in the order the second GEMM's B fragment holds them"""
        a16 = r16(act, dtype)
        if defect == "quad_h_g_swapped":                   # the quad read as (g0, g1, h0, h1)
            Sq = S[ch & 1].reshape(M, 16, 4)[:, :, [2, 3, 0, 1]].reshape(M, 64)
            a16 = r16(_geglu32(Sq, mean, rstd, b1[64 * ch:64 * ch + 64], cs1[64 * ch:64 * ch + 64]), dtype)
        if w8:
            return a16[:, np.r_[16:32, 0:16]] if defect == "ff8_exchange_halves_swapped" else a16
        return a16 if defect == "kperm_geglu_identity" else a16[:, kpg]

    for step, pc in enumerate(seq):
        ring[step % FF_NS] = pc if not (defect == "stale_ring_stage" and step == 64) else ring[step % FF_NS]
        kind, a, h = ring[step % FF_NS]
        w = piece_data((kind, a, h))
        kind, a, h = pc                                     # what the code position does with the stage's content
        if kind == "T1":
            if w.shape != (64, 160):
                w = np.resize(w, (64, 160))
            prod = _mm(x[:, 160 * h:160 * h + 160], w)
            S[a & 1] = prod if h == 0 else (S[a & 1] + prod).astype(F32)
            if h == 1 and a >= 1:
                ch = a - 1
                pf = frag(_geglu32(S[ch & 1], mean, rstd, b1[64 * ch:64 * ch + 64], cs1[64 * ch:64 * ch + 64]), ch)
        elif kind == "T2":
            if w.shape != (C, 32):
                w = np.resize(w, (C, 32))
            out = (out + _mm(pf, w)).astype(F32)
        else:
            if w.shape != (C, 32):
                w = np.resize(w, (C, 32))
            out = (out + _mm(x[:, 32 * a:32 * a + 32], w)).astype(F32)
            if a == 1:                                      # the GEGLU of the last chunk rides in tail pieces 0 and 1
                par = 0 if defect == "last_geglu_other_parity" else 1
                pf = frag(_geglu32(S[par], mean, rstd, b1[64 * 39:64 * 40], cs1[64 * 39:64 * 40]), 39)
    # ---- the epilogue: two 64-row passes per tile
    o = {k: emu_like(b) for k, b in t["out"].items() if k == "out"}
    ob = o["out"]
    bias = i["bias2"].numpy() if i["bias2"] is not None else np.zeros(C, F32)
    r1b, r2b = i["res1"], i["res2"]
    r1f = r1b.full.float().numpy() if r1b is not None else None
    r2 = _np(r2b.view) if r2b is not None else np.zeros((M, C), F32)
    accs = [np.zeros((M // p["rpb"], G, 2), np.int64) for (_, _, G) in p["gn"]]
    nwg = M // 128
    scale = F32(p["scale"])
    for bid in range(nwg):
        lid = remap(bid, nwg, defect)
        if lid >= nwg:
            continue
        m_blk = lid * 128
        stored = np.zeros((128, C), F32)
        for ps in range(2):
            m0 = m_blk + 64 * ps
            rows = np.arange(m0, m0 + 64)
            mref = m_blk if defect == "res1_wrap_per_tile" else m0
            shift = p["wrap"] if (p["wrap"] > 0 and mref >= p["wrap"]) else 0
            if r1b is not None:
                addr = r1b.base + (rows - shift)[:, None] * r1b.ld + np.arange(C)[None, :]
                r1 = r1f[np.clip(addr, 0, r1f.size - 1)]
            else:
                r1 = np.zeros((64, C), F32)
            if defect == "scale_after_residuals":
                v = (((out[rows] + bias[None, :]).astype(F32) + (r1 + r2[rows]).astype(F32)).astype(F32) * scale).astype(F32)
            else:
                v = (((out[rows] + bias[None, :]).astype(F32) * scale).astype(F32) + (r1 + r2[rows]).astype(F32)).astype(F32)
            v16 = r16(v, dtype)
            stored[64 * ps:64 * ps + 64] = v16
            addr = ob.base + rows[:, None] * ob.ld + np.arange(C)[None, :]
            ob.full[torch.from_numpy(addr)] = torch.from_numpy(v16.astype(np.float64))
        if p["gn"]:
            b = (m_blk + 128 if defect == "batch_of_tile_end" else m_blk) // p["rpb"]
            sm, sq = NC._seq_sum(stored, 0), NC._seq_sum((stored * stored).astype(F32), 0)
            fs = np.rint(sm.astype(np.float64) * NC.SUM_SCALE).astype(np.int64)
            fq = np.rint(sq.astype(np.float64) * NC.SQ_SCALE).astype(np.int64)
            for acc, (cg, c0, G) in zip(accs, p["gn"]):
                for h0 in (0, 160):                             # one slot set per 160-column half, relative to ITS first group
                    ncols = 160
                    cbase = c0 + (0 if defect == "gn_halves_not_split" else h0)
                    g_first = cbase // cg
                    gl = (cbase + np.arange(ncols)) // cg - g_first
                    gl = np.minimum(gl, NC_GN_SLOTS - 1)      # (a slot set holds 24 groups: what falls behind it is lost)
                    lost = (cbase + np.arange(ncols)) // cg - g_first >= NC_GN_SLOTS
                    gi = g_first + gl
                    ok = (~lost) & (gi < G) & (b < acc.shape[0])
                    np.add.at(acc[min(b, acc.shape[0] - 1), :, 0], gi[ok], fs[h0:h0 + ncols][ok])
                    np.add.at(acc[min(b, acc.shape[0] - 1), :, 1], gi[ok], fq[h0:h0 + ncols][ok])
    for k, acc in enumerate(accs):
        o[f"acc{k}"] = torch.from_numpy(acc.reshape(acc.shape[0], -1))
    return o


NC_GN_SLOTS = 24


# ================================================================================================ pp_tfront
QS_LOG2 = 40 ** -0.5 * LOG2E


def _tfront_cases():
    cs = []

    def add(probe, name, **p):
        d = dict(M=128, rpb=128, groups=32, q_scale=1.0, pad=(8, 16, 24, 8), regime="zero")
        d.update(p)
        cs.append(Case("tfront", probe, name, **d))
    for G in (32, 20, 16, 8, 5, 1):
        add("E", f"groups{G}", M=256, rpb=128, groups=G, q_scale=QS_LOG2 if G in (20, 5) else 1.0)
    for tl in GRIDS:
        add("E", f"grid{tl}", M=128 * tl, rpb=128, groups=(32, 16, 8)[tl % 3])
    add("E", "rpb256-b3", M=768, rpb=256, q_scale=QS_LOG2)
    add("E", "rpb384-b2", M=768, rpb=384, groups=20, pad=(8, 8, 8, 40))
    add("E", "rpb384-b1", M=384, rpb=384, groups=5)
    add("E", "contiguous", M=512, rpb=256, pad=(0, 0, 0, 0))
    for G in (32, 8, 1):
        add("R", f"groups{G}", M=256, rpb=128, groups=G)
    add("R", "qscale", M=256, rpb=256, q_scale=QS_LOG2)
    add("R", "offset16", M=128, rpb=128, regime="offset16", q_scale=QS_LOG2)
    add("R", "outlier-b3", M=384, rpb=128, regime="outlier", groups=16)
    add("R", "contiguous", M=1152, rpb=384, pad=(0, 0, 0, 0))
    return cs


def build_tfront(c: Case, dtype):
    p = c.p
    M, rpb, G, C = p["M"], p["rpb"], p["groups"], C320
    nb, cg = M // rpb, C320 // G
    g = _gen(43, M, rpb, G)
    eps32 = float(F32(1e-6))
    t = dict(M=M, probe=c.probe, eps32=eps32)
    kp = kperm_idx(C)
    if c.probe == "E":
        x = GC._ensure_blocks(_sparse(g, (M, C), 0.25))
        kk = torch.randint(0, 2, (nb, G), generator=g)
        kk[0, 0], kk[-1, -1] = 1, 0
        if nb > 1:
            kk[1] = 1 - kk[0]                              # the items differ in every group
        n_el = float(rpb * cg)
        acc = torch.zeros(nb, G, 2, dtype=torch.int64)
        acc[..., 1] = torch.round((4.0 ** (-kk.double()) - eps32) * n_el * NC.SQ_SCALE).long()
        var = acc[..., 1].double() / NC.SQ_SCALE / n_el
        rstd = (1.0 / torch.sqrt(var + eps32)).float().double()
        assert bool((rstd == 2.0 ** kk.double()).all()), (c.id, "rstd must come out as a power of two")
        gamma = torch.tensor([1.0, 2.0, -1.0, -2.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
        beta = _sparse(g, (C,), 0.25)
        w1 = _sparse(g, (C, C), 0.25)
        b1 = torch.randint(-3, 4, (C,), generator=g).double()
        wf = _sparse(g, (3 * C, C), 0.25)
        tb = torch.randint(-3, 4, (3 * C,), generator=g).double()
        rc = rstd.repeat_interleave(cg, 1).repeat_interleave(rpb, 0)            # [M, C]
        nrm = x * rc * gamma + beta
        _exact16(nrm, dtype, (c.id, "normalised row"))
        hs = nrm @ w1.t() + b1
        assert float((nrm.abs() @ w1.abs().t()).max()) < 2.0 ** 24
        _exact16(hs, dtype, (c.id, "hs"), 256.0)
        t["ref"] = dict(hs=hs)
    else:
        k = NC.build_tfront_case(p["regime"], dtype, B=nb, hw=rpb, groups=G)
        x = k["x"].double().reshape(M, C)
        acc = NC.build_acc(k["x"], None, G)
        gamma, beta, w1, b1, wf, tb = (k[n].double() for n in ("gg", "gb", "w1", "b1", "wf", "tb"))
        ref, gate = NC.gate_tfront_hs(k["x"], k["gg"], k["gb"], k["w1"], k["b1"], dtype, groups=G)
        t["ref"] = dict(hs=(ref, gate))
    wf16 = wf.to(dtype)
    px, ph, pq, pv = p["pad"]
    t["inp"] = dict(x=_inp(x, px, dtype), acc=acc.contiguous(), gamma=gamma.float().contiguous(), beta=beta.float().contiguous(),
                    w1=w1.to(dtype).contiguous(), b1=b1.float().contiguous(), wf=wf16.contiguous(), w2p=wf16[:, kp].contiguous(),
                    cs=wf16.double().sum(1).float().contiguous(), tb=tb.float().contiguous())
    t["out"] = dict(hs=out16(M, C, ph, dtype), qk=out16(M, 2 * C, pq, dtype), vt=out16(nb * C, rpb, pv, dtype))
    return t


def tfront_qkv_windows(c: Case, t, hs_stored: torch.Tensor, dtype, q_scale=None):
    """the (reference, gate) of qk [M, 640] and vt [nb * 320, rpb] from the hs that was stored"""
    i, p = t["inp"], c.p
    ref, gate = NC.gate_tfront_qkv(hs_stored, i["wf"], i["cs"], i["tb"], dtype, q_scale=p["q_scale"] if q_scale is None else q_scale)
    C, nb, rpb = C320, p["M"] // p["rpb"], p["rpb"]

    def vt(a):
        return a[:, 2 * C:].reshape(nb, rpb, C).permute(0, 2, 1).reshape(nb * C, rpb)
    return dict(qk=(ref[:, :2 * C], gate[:, :2 * C]), vt=(vt(ref), vt(gate)))


def walk_tfront(c: Case, t, dtype, defect=None, q_scale=None):
    p, i = c.p, t["inp"]
    M, rpb, G, C = p["M"], p["rpb"], p["groups"], C320
    qs = F32(p["q_scale"] if q_scale is None else q_scale)
    x = _np(i["x"].view)
    acc = i["acc"].numpy()
    gamma, beta = i["gamma"].numpy(), i["beta"].numpy()
    w1, w2p, b1, cs, tb = _np(i["w1"]), _np(i["w2p"]), i["b1"].numpy(), i["cs"].numpy(), i["tb"].numpy()
    kp = kperm_idx(C).numpy()
    o = {k: emu_like(b) for k, b in t["out"].items()}
    nwg = M // 128
    for bid in range(nwg):
        lid = remap(bid, nwg, defect)
        if lid >= nwg:
            continue
        m_blk = lid * 128
        b = (m_blk + 128 if defect == "batch_of_tile_end" else m_blk) // rpb
        bt = 0 if defect == "gn_stats_of_item0" else min(b, acc.shape[0] - 1)
        s = acc[bt, :, 0].astype(np.float64) / NC.SUM_SCALE
        q = acc[bt, :, 1].astype(np.float64) / NC.SQ_SCALE
        n = float(rpb) * float(C // G)
        mean = s / n
        var = np.maximum(q / n - mean * mean, 0.0)
        mean32, rstd32 = mean.astype(F32), (1.0 / np.sqrt(var + t["eps32"])).astype(F32)
        gg = np.arange(C) // (10 if defect == "groups_as_c_over_10" else C // G)
        gg = np.minimum(gg, G - 1) if defect != "groups_as_c_over_10" else gg % max(G, 1)
        sc = (rstd32[gg] * gamma).astype(F32)
        sh = (beta - (mean32[gg] * sc).astype(F32)).astype(F32)
        rows = slice(m_blk, m_blk + 128)
        n16 = r16(((x[rows] * sc[None, :]).astype(F32) + sh[None, :]).astype(F32), dtype)
        # the slabs: t < 5 proj_in (k 64 t ..), then Q, K, V (five each) of the k-permuted weight; ring stage t % 3
        slab = [("w1", 0, tt) for tt in range(5)] + [("w2", ps, kt) for ps in range(3) for kt in range(5)]
        ring = [None] * 3
        a320 = np.zeros((128, C), F32)
        hs16 = None
        qkv = np.zeros((128, 3 * C), F32)
        for tt, sl in enumerate(slab):
            ring[tt % 3] = sl if not (defect == "stale_ring_stage" and tt == 7) else ring[tt % 3]
            kind, ps, kt = ring[tt % 3]
            w = w1[:, 64 * kt:64 * kt + 64] if kind == "w1" else w2p[320 * ps:320 * ps + 320, 64 * kt:64 * kt + 64]
            if tt < 5:
                a320 = (a320 + _mm(n16[:, 64 * tt:64 * tt + 64], w)).astype(F32)
                if tt == 4:
                    hs16 = r16((a320 + b1[None, :]).astype(F32), dtype)
                    sm, sq = NC._seq_sum(hs16, 1), NC._seq_sum((hs16 * hs16).astype(F32), 1)
                    mu = (sm * F32(1.0 / C)).astype(F32)
                    rs = (F32(1.0) / np.sqrt((np.maximum((sq * F32(1.0 / C)).astype(F32) - (mu * mu).astype(F32), F32(0.0))
                                              + F32(1e-5)).astype(F32))).astype(F32)
                    a320 = np.zeros((128, C), F32)
            else:
                kt_ = (tt - 5) % 5
                pos = np.arange(64 * kt_, 64 * kt_ + 64)
                src = pos if defect == "kperm_identity" else (np.argsort(kp)[pos] if defect == "kperm_inverse" else kp[pos])
                a320 = (a320 + _mm(hs16[:, src], w)).astype(F32)
                if kt_ == 4:
                    pz = (tt - 5) // 5
                    v = ((rs[:, None] * (a320 - (mu[:, None] * cs[None, 320 * pz:320 * pz + 320]).astype(F32)).astype(F32)).astype(F32)
                         + tb[None, 320 * pz:320 * pz + 320]).astype(F32)
                    if pz == (1 if defect == "q_scale_on_k" else 0):
                        v = (v * qs).astype(F32)
                    qkv[:, 320 * pz:320 * pz + 320] = r16(v, dtype)
                    a320 = np.zeros((128, C), F32)
        rr = np.arange(m_blk, m_blk + 128)
        for name, val in (("hs", hs16), ("qk", qkv[:, :2 * C])):
            ob = o[name]
            addr = ob.base + rr[:, None] * ob.ld + np.arange(val.shape[1])[None, :]
            ob.full[torch.from_numpy(addr)] = torch.from_numpy(val.astype(np.float64))
        p0 = 0 if defect == "vt_at_p0_zero" else m_blk - b * rpb
        ob = o["vt"]
        addr = ob.base + (b * C + np.arange(C))[:, None] * ob.ld + (p0 + np.arange(128))[None, :]
        okm = (addr >= 0) & (addr < ob.full.numel())
        vals = qkv[:, 2 * C:].T.astype(np.float64)
        ob.full[torch.from_numpy(addr[okm])] = torch.from_numpy(vals[okm])
    return o


# ================================================================================================ pp_xattn_block (+ wide kernel)
NCTX = (1, 7, 77, 79, 80)


def _xattn_cases():
    cs = []

    def add(probe, name, **p):
        d = dict(C=320, M=128, rpb=128, nctx=77, res=True, bias=True, ln=0, stats=True, pre=None, wrap=0, pad=(8, 16, 24),
                 regime="zero")
        d.update(p)
        cs.append(Case("xattn", probe, name, **d))
    for n in NCTX:
        add("E", f"nctx{n}", M=256, rpb=128, nctx=n)
    for tl in GRIDS:
        add("E", f"grid{tl}", M=128 * tl, rpb=128, nctx=(77, 80, 7)[tl % 3])
    add("E", "rpb256-b3", M=768, rpb=256, nctx=80)
    add("E", "rpb384-b2", M=768, rpb=384, nctx=79)
    add("E", "contiguous", M=512, rpb=256, pad=(0, 0, 0))
    add("E", "bare", M=256, res=False, bias=False, stats=False)
    add("E", "res-only", M=128, bias=False)
    add("E", "bias-only", M=128, res=False, stats=False)
    add("E", "pre-w", M=256, pre="w", nctx=80)
    add("E", "pre-wb", M=384, pre="wb", nctx=7)
    add("E", "pre-wb-nores", M=128, pre="wb", res=False)
    add("E", "wrap-2x", M=512, rpb=128, wrap=256)
    add("E", "wrap-3over2", M=384, rpb=128, wrap=256, nctx=80)
    add("E", "wrap-rpb256", M=512, rpb=256, wrap=256, nctx=79)
    add("E", "pre-wrap", M=512, rpb=256, wrap=256, pre="wb")
    add("E", "pre-wrap-3over2", M=384, rpb=128, wrap=256, pre="w", stats=False)
    # the wide kernel: grid = (M / 64) (C / 320) is even (C = 640) or a multiple of four (1280): residues 0, 2, 4, 6 of 8 occur,
    # an odd residue cannot
    for C, tiles in ((640, (1, 2, 3, 4, 9)), (1280, (1, 2, 3, 5))):
        for tl in tiles:
            add("E", f"wide{C}-grid{tl}", C=C, M=64 * tl, rpb=64, nctx=(77, 80, 1)[tl % 3])
    add("E", "wide640-rpb192", C=640, M=384, rpb=192, nctx=79)
    add("E", "wide1280-rpb192", C=1280, M=192, rpb=192, nctx=7, pad=(0, 0, 0))
    add("E", "wide640-bare", C=640, M=128, rpb=64, res=False, bias=False, stats=False)
    for tiles in (1, 2, 5):
        add("R", f"ln-tiles{tiles}", M=256, ln=tiles, nctx=(7, 77, 80)[tiles % 3])
    add("R", "plain", M=256, nctx=77)
    add("R", "ln-offset16", M=128, ln=2, regime="offset16", nctx=79)
    add("R", "ln-outlier-wrap", M=512, rpb=128, wrap=256, ln=2, regime="outlier", nctx=7)
    add("R", "pre-ln", M=256, pre="wb", ln=2, nctx=77)
    add("R", "pre-ln-nob-wrap", M=512, rpb=256, wrap=256, pre="w", ln=2, nctx=80)
    add("R", "pre-plain", M=128, pre="wb", nctx=7, res=False)
    add("R", "wide640-ln", C=640, M=192, rpb=64, ln=4, nctx=77)
    add("R", "wide1280-ln", C=1280, M=128, rpb=64, ln=8, nctx=80)
    add("R", "wide640-plain", C=640, M=192, rpb=192, nctx=7, res=False)
    return cs


def _blocks(nctx: int, k: int, r: int):
    """an aligned dyadic block of min(k, what fits) keys below nctx, chosen by r -> (start, size)"""
    while k > nctx:
        k //= 2
    nblk = nctx // k
    return k * (r % nblk), k


def xattn_signal_channels(C: int) -> torch.Tensor:
    c = torch.arange(C)
    return c[((5 * c + c // 32) % 3) == 0]


def build_xattn(c: Case, dtype):
    p = c.p
    C, M, rpb, nctx, wrap = p["C"], p["M"], p["rpb"], p["nctx"], p["wrap"]
    Ms = wrap or M
    nb = M // rpb
    g = _gen(47, C, M, rpb, nctx, wrap)
    kkp = NC.xattn_kk()
    t = dict(M=M, probe=c.probe)
    pre = p["pre"]
    src = np.arange(M) % Ms
    if c.probe == "E":
        sig = xattn_signal_channels(C)
        nonsig = torch.ones(C, dtype=torch.bool)
        nonsig[sig] = False
        m = torch.arange(Ms)
        sc = sig[(13 * m + 5) % len(sig)]                                     # the row's signal channel
        noise = torch.randint(-2, 3, (Ms, C), generator=g).double() * nonsig[None, :]
        hrow = noise.clone()
        live = (m % 7) != 6                                                     # every seventh row: noise only
        hrow[m[live], sc[live]] = 32.0
        gt = torch.zeros(nb, HEADS, KP, C, dtype=torch.float64)
        gb = torch.full((nb, HEADS, KP), -math.inf, dtype=torch.float64)
        for b in range(nb):
            for h in range(HEADS):
                gb[b, h, :nctx] = -512.0
                s0, k0 = _blocks(nctx, (1, 2, 4)[(h + b) % 3], 5 * h + 3 * b + 1)
                gb[b, h, s0:s0 + k0] = 0.0
                for ch in sig.tolist():
                    s1, k1 = _blocks(nctx, (1, 2, 4)[(ch + h + b) % 3], 7 * ch + 13 * h + 29 * b)
                    gt[b, h, s1:s1 + k1, ch] = 32.0
        key = torch.arange(KP)[None, None, :]
        nn = torch.arange(C)[:, None, None]
        hh = torch.arange(HEADS)[None, :, None]
        ht = torch.stack([4.0 * (((5 * key + 3 * nn + 7 * hh + 11 * b) % 7) - 3) * (key < nctx) for b in range(nb)]).double()
        bo = torch.randint(-3, 4, (C,), generator=g).double()
        res = torch.randint(-3, 4, (Ms, C), generator=g).double()
        gcs = torch.zeros(nb, S640)
        if pre:
            a = (17 * m + 3) % C                                               # x is one-hot at channel a(m); pre_w routes it to sc
            x = torch.zeros(Ms, C, dtype=torch.float64)
            x[m[live], a[live]] = 1.0
            pre_w = torch.zeros(C, C, dtype=torch.float64)
            # a column routes to ONE channel: rows sharing a(m) must share sc(m) -> route by a alone
            route = sig[(13 * torch.arange(C) + 5) % len(sig)]
            pre_w[route, torch.arange(C)] = 32.0
            pre_b = torch.randint(-2, 3, (C,), generator=g).double() * nonsig if pre == "wb" else None
            res = res * nonsig[None, :]
            hrow = x @ pre_w.t() + (pre_b if pre_b is not None else 0.0) + (res if p["res"] else 0.0)
            _exact16(hrow, dtype, (c.id, "h"))
        else:
            x = hrow
            pre_w = pre_b = None
        # ---- reference
        hfull = hrow[src]
        lg = torch.stack([hfull[b * rpb:(b + 1) * rpb] @ gt[b].reshape(S640, C).t() + gb[b].reshape(-1) for b in range(nb)])
        lg = lg.reshape(M, HEADS, KP)
        mx = lg.max(-1, keepdim=True).values
        win = lg == mx
        kwin = win.sum(-1)
        second = torch.where(win, torch.full_like(lg, -math.inf), lg).max(-1).values
        assert bool(((kwin == 1) | (kwin == 2) | (kwin == 4)).all()), (c.id, "1, 2 or 4 maximal logits per (row, head)")
        assert bool((mx[..., 0] - second >= 160.0).all()), (c.id, "every other logit lower by >= 160")
        pr = win.double() / kwin[..., None].double()
        o = torch.stack([pr[b * rpb:(b + 1) * rpb].reshape(rpb, S640) @ ht[b].reshape(C, S640).t() for b in range(nb)]).reshape(M, C)
        resid = hfull if pre else (res[src] if p["res"] else 0.0)
        ref = o + (bo if p["bias"] else 0.0) + resid
        _exact16(ref, dtype, (c.id, "out"), 256.0)
        t["ref"] = dict(out=ref)
        t["winners"] = win
        if p["stats"]:
            S, Q, _ = NC.row_tile_sums(ref)
            t["ref"]["stats"] = torch.stack([S, Q], -1).reshape(M, -1)
        if pre:
            t["ref"]["h"] = hfull
        gt16 = gt.reshape(nb, S640, C).to(dtype)
        ht_nat = ht.reshape(nb, C, S640).to(dtype)
        gbf = gb.reshape(nb, S640).float()
        st = None
    else:
        k = NC.build_xattn_case(p["regime"], dtype, B=nb, hw=rpb, nctx=nctx, C=C, tiles=p["ln"])
        x = k["x"].double()[:Ms]
        gt16, gcs, gbf = k["gt"], k["gcs"], k["gb"]
        ht_nat = None
        bo = k["bo"].double()
        res = torch.randn(Ms, C, generator=g).to(dtype).double()
        st = k["st"][:Ms].contiguous() if (p["ln"] and not pre) else None
        pre_w = pre_b = None
        xs, rsrc = x[src].to(dtype), (res[src].to(dtype) if p["res"] else None)
        if pre:                                            # x is attn1's output, h = x pre_w^T + pre_b + res what the sub-block sees
            pre_w = (torch.randn(C, C, generator=g) * C ** -0.5).to(dtype).double()
            pre_b = (torch.randn(C, generator=g) * 0.1).float().double() if pre == "wb" else None
            hx = xs.double() @ pre_w.t() + (pre_b if pre_b is not None else 0.0) + (rsrc.double() if rsrc is not None else 0.0)
            A1 = xs.double().abs() @ pre_w.abs().t() + (pre_b.abs() if pre_b is not None else 0.0) + \
                (rsrc.double().abs() if rsrc is not None else 0.0)
            t["ref"] = dict(h=(hx, NC._finish(hx, (C + 2) * U32 * A1, hx, False, dtype)))
            t["folded_nat"] = (gt16, gcs, gbf, k["ht"])
        else:
            ref, gate = NC.gate_xattn_block(xs, p["ln"], (gt16, gcs, gbf, k["ht"]), bo if p["bias"] else None, rsrc, rpb, 1e-5, dtype,
                                            fold=bool(p["ln"]))
            t["ref"] = dict(out=(ref, gate))
    px, po, pr_ = p["pad"]
    ht_st = ht_nat[:, :, kkp].contiguous() if ht_nat is not None else k["ht"]
    gt_st = gt16[:, :, kperm_idx(C)].contiguous() if pre else gt16.contiguous()
    t["inp"] = dict(x=_inp(x, px, dtype), res=_inp(res, pr_, dtype) if p["res"] else None, st=st, gt=gt_st, gcs=gcs.contiguous(),
                    gb=gbf.contiguous(), ht=ht_st, bo=bo.float().contiguous() if p["bias"] else None,
                    pre_w=pre_w.to(dtype).contiguous() if pre_w is not None else None,
                    pre_b=pre_b.float().contiguous() if pre_b is not None else None)
    t["out"] = dict(out=out16(M, C, po, dtype))
    if p["stats"]:
        t["out"]["stats"] = GC.sentinel_out(M, (C // 160) * 2, 0, torch.float32, GUARD)
    return t


def gate_row_stats_xattn(stored: torch.Tensor):
    """(S, Q exact, gate S, gate Q) [M, C / 160] of the row moments pp_xattn_block forms from its stored values: per lane 10
    blocks x (three adds + one accumulation) and two shuffle adds = 42 roundings; the squares round once more"""
    S, Q, S1 = NC.row_tile_sums(stored)
    return S, Q, 42 * U32 * S1, 43 * U32 * Q


def walk_xattn(c: Case, t, dtype, defect=None):
    p, i = c.p, t["inp"]
    C, M, rpb, wrap, pre = p["C"], p["M"], p["rpb"], p["wrap"], p["pre"]
    wide = C != 320
    BM = 64 if wide else 128
    NSPLIT = C // 320
    xb, rb = i["x"], i["res"]
    xf = xb.full.float().numpy()
    rf = rb.full.float().numpy() if rb is not None else None
    gt, ht, gcs, gb = _np(i["gt"]), _np(i["ht"]), i["gcs"].numpy(), i["gb"].numpy().copy()
    if defect == "padded_not_masked":
        gb[np.isinf(gb)] = 0.0
    bo = i["bo"].numpy() if i["bo"] is not None else np.zeros(C, F32)
    kk = NC.xattn_kk().numpy()
    kp = kperm_idx(C).numpy()
    o = {k: emu_like(b) for k, b in t["out"].items()}
    ob = o["out"]
    nwg = (M // BM) * NSPLIT
    cols = np.arange(C)
    hall = np.full((M, C), np.nan, F32)

    def rd(buf, full, rows, ncol0=0, ncols=None):
        addr = buf.base + rows[:, None] * buf.ld + (ncol0 + np.arange(ncols or C))[None, :]
        return full[np.clip(addr, 0, full.size - 1)]

    for bid in range(nwg):
        lid = remap(bid, nwg, defect)
        if lid >= nwg:
            continue
        tile, cgp = lid // NSPLIT, lid % NSPLIT             # (the column groups of a row tile are neighbours: they share G)
        m_blk = tile * BM
        b = (m_blk + BM if defect == "batch_of_tile_end" else m_blk) // rpb
        b = min(b, gt.shape[0] - 1)
        rows = np.arange(m_blk, m_blk + BM)
        ms = np.where((wrap > 0) & (rows >= wrap), rows - wrap, rows)
        xr = rd(xb, xf, ms)
        if i["st"] is not None:
            st = i["st"].numpy()[ms]
            s, q = NC._seq_sum(st[..., 0], 1), NC._seq_sum(st[..., 1], 1)
            mean = (s * F32(1.0 / C)).astype(F32)
            var = ((q * F32(1.0 / C)).astype(F32) - (mean * mean).astype(F32)).astype(F32)
            rstd = (F32(1.0) / np.sqrt((np.maximum(var, F32(0.0)) + F32(1e-5)).astype(F32))).astype(F32)
        else:
            mean, rstd = np.zeros(BM, F32), np.ones(BM, F32)
        if pre:
            pw = _np(i["pre_w"])
            pb = i["pre_b"].numpy() if i["pre_b"] is not None else np.zeros(C, F32)
            rr = rd(rb, rf, ms) if rb is not None else np.zeros((BM, C), F32)
            h16 = r16(((_mm(xr, pw) + pb[None, :]).astype(F32) + rr).astype(F32), dtype)
            hall[rows] = h16
            if p["ln"]:                                    # a LayerNorm folded into gt: the moments of the rounded h, in the kernel
                sm, sq = NC._seq_sum(h16, 1), NC._seq_sum((h16 * h16).astype(F32), 1)
                mean = (sm * F32(1.0 / C)).astype(F32)
                rstd = (F32(1.0) / np.sqrt((np.maximum((sq * F32(1.0 / C)).astype(F32) - (mean * mean).astype(F32), F32(0.0))
                                            + F32(1e-5)).astype(F32))).astype(F32)
            addr = ob.base + rows[:, None] * ob.ld + cols[None, :]
            ob.full[torch.from_numpy(addr)] = torch.from_numpy(h16.astype(np.float64))      # parked in the tile's own rows
            src = cols if defect == "kperm_identity" else (np.argsort(kp) if defect == "kperm_inverse" else kp)
            lin = h16[:, src]
        else:
            lin = xr
        # slabs: G^T rows 0..319 (five or C / 64 k slabs), rows 320..639, then ten 64-wide slices of H^T; ring stage t % 3
        ns1 = C // 64
        slabs = [("g", hf, kt) for hf in range(2) for kt in range(ns1)] + [("h", 0, u) for u in range(10)]
        ring = [None] * 3
        acc = np.zeros((BM, 320), F32)
        pfull = np.zeros((BM, S640), F32)
        for tt, sl in enumerate(slabs):
            ring[tt % 3] = sl if not (defect == "stale_ring_stage" and tt == 7) else ring[tt % 3]
            kind, hf, kt = ring[tt % 3]
            if sl[0] == "g":
                w = gt[b, 320 * hf:320 * hf + 320, 64 * kt:64 * kt + 64] if kind == "g" else np.resize(ht[b], (320, 64))
                acc = (acc + _mm(lin[:, 64 * sl[2]:64 * sl[2] + 64], w)).astype(F32)
                if sl[2] == ns1 - 1:                        # softmax of this half's four heads
                    hfc = sl[1]
                    n0 = 0 if (defect == "heads47_tables_of_03") else 320 * hfc
                    lgt = ((rstd[:, None] * (acc - (mean[:, None] * gcs[b, n0:n0 + 320][None, :]).astype(F32)).astype(F32)).astype(F32)
                           + gb[b, n0:n0 + 320][None, :]).astype(F32).reshape(BM, 4, KP)
                    with np.errstate(invalid="ignore", over="ignore"):
                        e = np.exp2((lgt - lgt.max(-1, keepdims=True)).astype(F32)).astype(F32)
                    pfull[:, 320 * hfc:320 * hfc + 320] = r16((e * (F32(1.0) / NC._seq_sum(e, 2))[..., None]).astype(F32).reshape(BM, 320), dtype)
                    acc = np.zeros((BM, 320), F32)
            else:
                u = sl[2]
                hrow0 = 0 if defect == "wide_ht_group_offset_dropped" else cgp * 320
                w = ht[b, hrow0:hrow0 + 320, 64 * kt:64 * kt + 64] if kind == "h" else np.resize(gt[b], (320, 64))
                acc = (acc + _mm(pfull[:, kk[64 * u:64 * u + 64]], w)).astype(F32)
        n_out = cgp * 320
        if pre:
            rsrc = ms if defect == "wrap_on_parked_h" else rows
            addr = ob.base + rsrc[:, None] * ob.ld + cols[None, :]
            resid = ob.full[torch.from_numpy(addr)].numpy().astype(F32)
        elif rb is not None:
            resid = rd(rb, rf, ms, n_out, 320)
        else:
            resid = np.zeros((BM, 320), F32)
        v16 = r16(((acc + bo[None, n_out:n_out + 320]).astype(F32) + resid).astype(F32), dtype)
        addr = ob.base + rows[:, None] * ob.ld + (n_out + np.arange(320))[None, :]
        ob.full[torch.from_numpy(addr)] = torch.from_numpy(v16.astype(np.float64))
        if "stats" in o:
            sb = o["stats"]
            split = 128 if defect == "row_stats_split_128" else 160
            for tl, (c0, c1) in enumerate(((0, split), (split, 320))):
                blk = v16[:, c0:c1]
                sm, sq = NC._seq_sum(blk, 1), NC._seq_sum((blk * blk).astype(F32), 1)
                addr = sb.base + rows * sb.ld + (2 * cgp + tl) * 2
                sb.full[torch.from_numpy(addr)] = torch.from_numpy(sm.astype(np.float64))
                sb.full[torch.from_numpy(addr + 1)] = torch.from_numpy(sq.astype(np.float64))
    if pre:
        o["h"] = torch.from_numpy(hall.astype(np.float64))   # (what the second launch with H^T = 0 returns)
    return o


# ================================================================================================ pp_xattn_fold
def _fold_cases():
    cs = []

    def add(name, **p):
        d = dict(C=320, B=2, nctx=77, kperm=0, ldk_pad=8, ldvt=0, qcs=True, qb=True)
        d.update(p)
        cs.append(Case("fold", "E", name, **d))
    for C in (320, 640, 1280):
        for kperm in ((0, 1, 2) if C == 320 else (0, 2)):
            add(f"c{C}-kperm{kperm}", C=C, kperm=kperm, nctx=(77, 80, 7)[kperm], B=2 if C < 1280 else 1)
    for n in NCTX:
        add(f"nctx{n}", nctx=n, kperm=(0, 1, 2)[n % 3], ldvt=96 if n % 2 else 0)
    add("no-vectors", qcs=False, qb=False, ldk_pad=0)
    add("colsum-only", qb=False, B=3, nctx=79, kperm=1)
    add("bias-only", qcs=False, C=640, B=1, nctx=7, ldvt=96)
    return cs


def build_fold(c: Case, dtype):
    p = c.p
    C, B, nctx, kperm = p["C"], p["B"], p["nctx"], p["kperm"]
    D = C // HEADS
    ldvt = p["ldvt"] or -(-nctx // 8) * 8
    g = _gen(53, C, B, nctx, kperm)
    K = _sparse(g, (B * nctx, C), 0.3)
    V = _sparse(g, (B, C, nctx), 0.3)
    wq = _sparse(g, (C, C), 0.3, hi=2)
    wo = _sparse(g, (C, C), 0.3)
    qcs = torch.randint(-2, 3, (C,), generator=g).float() if p["qcs"] else None
    qb = torch.randint(-2, 3, (C,), generator=g).float() if p["qb"] else None
    scale = D ** -0.5
    qscale = F32(F32(scale) * F32(1.44269504088896340736))
    Kh, Vh = K.reshape(B, nctx, HEADS, D), V.reshape(B, HEADS, D, nctx)
    gsum = torch.zeros(B, HEADS, KP, C, dtype=torch.float64)
    gsum[:, :, :nctx] = torch.einsum("bkhd,hdc->bhkc", Kh, wq.reshape(HEADS, D, C))
    assert float(gsum.abs().max()) < 2.0 ** 24
    gt = torch.from_numpy((gsum.numpy().astype(F32) * qscale).astype(F32)).to(dtype).reshape(B, S640, C)
    if kperm & 1:
        gt = gt[:, :, kperm_idx(C)]
    gbv = torch.full((B, HEADS, KP), -math.inf)
    bsum = torch.einsum("bkhd,hd->bhk", Kh, qb.double().reshape(HEADS, D)) if qb is not None else torch.zeros(B, HEADS, nctx, dtype=torch.float64)
    gbv[:, :, :nctx] = torch.from_numpy((bsum.numpy().astype(F32) * qscale).astype(F32))
    hsum = torch.zeros(B, C, HEADS, KP, dtype=torch.float64)
    hsum[..., :nctx] = torch.einsum("nhd,bhdk->bnhk", wo.reshape(C, HEADS, D), Vh)
    _exact16(hsum, dtype, (c.id, "ht"))
    ht = hsum.reshape(B, C, S640)
    if not (kperm & 2):
        ht = ht[:, :, NC.xattn_kk()]
    t = dict(probe="E", M=B)
    vpad = torch.full((B * C, ldvt), math.nan, dtype=torch.float64)
    vpad[:, :nctx] = V.reshape(B * C, nctx)
    t["inp"] = dict(k=_inp(K, p["ldk_pad"], dtype), vt=lay(vpad.to(dtype), 0, GUARD, GUARD, math.nan), ldvt=ldvt, wq=wq.to(dtype).contiguous(),
                    wo=wo.to(dtype).contiguous(), qcs=qcs, qb=qb, scale=scale)
    t["out"] = dict(gt=out16(B * S640, C, 0, dtype), ht=out16(B * C, S640, 0, dtype),
                    gcs=GC.sentinel_out(B, S640, 0, torch.float32, GUARD), gb=GC.sentinel_out(B, S640, 0, torch.float32, GUARD))
    t["ref"] = dict(gt=gt.reshape(B * S640, C).double(), ht=ht.reshape(B * C, S640), gb=gbv.reshape(B, S640).double())
    gst = gt.double()
    if qcs is None:
        t["ref"]["gcs"] = torch.zeros(B, S640, dtype=torch.float64)
    else:                                                  # (the column sum of the STORED row: any fp32 order)
        t["ref"]["gcs"] = (gst.sum(-1), (C // 64 + 6) * U32 * gst.abs().sum(-1))
    return t


def walk_fold(c: Case, t, dtype, defect=None):
    p, i = c.p, t["inp"]
    C, B, nctx, kperm = p["C"], p["B"], p["nctx"], p["kperm"]
    D = C // HEADS
    o = {k: emu_like(b) for k, b in t["out"].items()}
    K = i["k"].view.double().numpy().reshape(B, nctx, HEADS, D)
    V = i["vt"].view.double().numpy()[:, :nctx].reshape(B, HEADS, D, nctx)
    wq, wo = i["wq"].double().numpy().reshape(HEADS, D, C), i["wo"].double().numpy().reshape(C, HEADS, D)
    qscale = F32(F32(i["scale"]) * F32(1.44269504088896340736))
    gs = np.zeros((B, HEADS, KP, C), F32)
    gs[:, :, :nctx] = np.einsum("bkhd,hdc->bhkc", K, wq).astype(F32)
    g16 = r16((gs * qscale).astype(F32), dtype).reshape(B, S640, C)
    kp = kperm_idx(C).numpy()
    if kperm & 1:
        g16 = g16[:, :, np.arange(C) if defect == "kperm_identity" else (np.argsort(kp) if defect == "kperm_inverse" else kp)]
    hsum = np.zeros((B, C, HEADS, KP), F32)
    hsum[..., :nctx] = np.einsum("nhd,bhdk->bnhk", wo, V).astype(F32)
    h16 = r16(hsum, dtype).reshape(B, C, S640)
    if not (kperm & 2) and defect != "fold_ht_layout_natural":
        h16 = h16[:, :, NC.xattn_kk().numpy()]
    if (kperm & 2) and defect == "fold_ht_layout_natural":
        h16 = h16[:, :, NC.xattn_kk().numpy()]
    gbv = np.full((B, HEADS, KP), 0.0 if defect in ("fold_padded_not_masked", "padded_not_masked") else -np.inf, F32)
    if i["qb"] is not None:
        bs = np.einsum("bkhd,hd->bhk", K, i["qb"].double().numpy().reshape(HEADS, D)).astype(F32)
    else:
        bs = np.zeros((B, HEADS, nctx), F32)
    gbv[:, :, :nctx] = (bs * qscale).astype(F32)
    if i["qcs"] is None:
        gcs = np.zeros((B, S640), F32)
    else:                                                  # one wave per row: lane sums of pair sums, then the butterfly
        pr = (g16.reshape(B, S640, C // 2, 2)[..., 0] + g16.reshape(B, S640, C // 2, 2)[..., 1]).astype(F32)
        lanes = np.zeros((B, S640, 64), F32)
        for j in range(0, C // 2, 64):
            blk = pr[:, :, j:j + 64]
            lanes[:, :, :blk.shape[2]] = (lanes[:, :, :blk.shape[2]] + blk).astype(F32)
        gcs = NC._butterfly(lanes)[..., 0]
    for name, val in (("gt", g16.reshape(B * S640, C)), ("ht", h16.reshape(B * C, S640)), ("gcs", gcs), ("gb", gbv.reshape(B, S640))):
        o[name].view.copy_(torch.from_numpy(np.ascontiguousarray(val, dtype=np.float64)))
    return o


# ================================================================================================ refusals
def _refusals():
    """(kernel, name, the case it is derived from, the overrides of its arguments, the return code)"""
    X = []

    def add(kernel, name, rc, base=None, **over):
        X.append(Case(kernel, "X", name, base=base or {}, over=over, expect=rc))
    B, U = PP_ERR_BAD_ARG, PP_ERR_UNSUPPORTED
    add("ff", "m-not-tile", U, M_arg=64)
    add("ff", "rpb-not-tile", U, rpb=64)
    add("ff", "m-not-rpb", U, base=dict(M=384), rpb=256)
    add("ff", "ldx-odd", B, ldx=324)
    add("ff", "ldx-short", B, ldx=312)
    add("ff", "ldo-odd", B, ldo=324)
    add("ff", "ldo-short", B, ldo=312)
    add("ff", "ldres1-odd", B, base=dict(res1=True), ldres1=324)
    add("ff", "ldres2-odd", B, base=dict(res2=True), ldres2=324)
    add("ff", "ldres1-short", B, base=dict(res1=True), ldres1=312)
    add("ff", "out-misaligned", B, out_off=8)
    add("ff", "res1-misaligned", B, base=dict(res1=True), res1_off=8)
    add("ff", "wrap-not-64", B, base=dict(res1=True, M=256, wrap=128), wrap=96)
    add("ff", "wrap-too-small", B, base=dict(res1=True, M=384, wrap=256), wrap=128)
    add("ff", "wrap-no-res1", B, wrap=64)
    add("ff", "wrap-negative", B, base=dict(res1=True), wrap=-64)
    add("ff", "gn-no-rpb", B, base=dict(gn=((10, 0, 32),), rpb=128), rpb=0)
    add("ff", "gn-cg-small", U, base=dict(gn=((10, 0, 32),), rpb=128), gn_cg=4)
    add("ff", "ln-no-colsum", B, base=dict(fold=True), probe="R", cs1=None)
    for f in ("act", "out_f32", "rowvec", "row_stats_out", "ln_stats", "gn_next_out", "out_dup_rows", "splitk", "out_vt", "gn_in_acc"):
        add("ff", f"g2-{f}", U, g2=f)
    add("ff", "g2-n", U, g2="N")
    add("ff", "g2-k", U, g2="K")
    add("tfront", "m-not-tile", U, M_arg=64)
    add("tfront", "rpb-not-tile", U, rpb=64)
    for G in (0, 64, 3):
        add("tfront", f"groups{G}", U, groups=G)
    add("tfront", "qscale-zero", B, q_scale=0.0)
    add("tfront", "qscale-negative", B, q_scale=-1.0)
    add("tfront", "ldx-odd", B, ldx=324)
    add("tfront", "ldhs-short", B, ldhs=312)
    add("tfront", "ldqk-short", B, ldqk=632)
    add("tfront", "ldqk-odd", B, ldqk=644)
    add("tfront", "ldvt-short", B, ldvt=120)
    add("tfront", "ldvt-odd", B, ldvt=132)
    add("tfront", "hs-misaligned", B, hs_off=8)
    add("tfront", "qk-misaligned", B, qk_off=4)
    add("tfront", "c-640", U, c=640)
    add("xattn", "m-not-tile", U, M_arg=64)
    add("xattn", "rpb-not-tile", U, rpb=64)
    add("xattn", "ldx-odd", B, ldx=324)
    add("xattn", "ldo-short", B, ldo=312)
    add("xattn", "ldres-odd", B, ldres=324)
    add("xattn", "out-misaligned", B, out_off=8)
    add("xattn", "res-misaligned", B, res_off=8)
    add("xattn", "wrap-not-rpb", B, base=dict(M=256, rpb=128, wrap=128), wrap=192)
    add("xattn", "wrap-too-small", B, base=dict(M=384, rpb=128, wrap=256), wrap=128)
    add("xattn", "wrap-negative", B, wrap=-128)
    add("xattn", "preb-no-prew", B, base=dict(pre="wb"), pre_w=None)
    add("xattn", "ln-no-tiles", B, base=dict(ln=2), probe="R", ln_tiles=0)
    add("xattn", "wide-wrap", U, base=dict(C=640, M=128, rpb=64), wrap=64)
    add("xattn", "wide-m-not-tile", U, base=dict(C=640, M=128, rpb=64), M_arg=96)
    add("xattn", "c-960", U, c=960)
    add("fold", "kperm1-c640", U, base=dict(C=640, B=1), kperm=1)
    add("fold", "kperm3", B, kperm=3)
    add("fold", "nctx0", U, nctx=0)
    add("fold", "nctx81", U, nctx=81)
    add("fold", "heads4", U, heads=4)
    add("fold", "ldk-short", B, ldk=312)
    add("fold", "ldvt-short", B, base=dict(nctx=77), ldvt=72)
    add("fold", "batch0", B, batch=0)
    return X


REFUSALS = _refusals()
CASES = _ff_cases() + _tfront_cases() + _xattn_cases() + _fold_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def refusal_base(c: Case) -> Case:
    """the (small) passing case a refusal is derived from"""
    k = c.kernel
    if k == "ff":
        d = dict(_ff_cases()[0].p, open="chunk", res1=False)
    elif k == "tfront":
        d = dict(_tfront_cases()[0].p, M=128)
    elif k == "xattn":
        d = dict(_xattn_cases()[0].p, M=128, nctx=7)
    else:
        d = dict(_fold_cases()[0].p, B=1, nctx=7)
    d.update(c.p["base"])
    if "probe" in c.p["over"]:
        return Case(k, c.p["over"]["probe"], "base-of-" + c.id, **d)
    return Case(k, "E", "base-of-" + c.id, **d)


# ================================================================================================ the common front
BUILD = dict(ff=build_ff, tfront=build_tfront, xattn=build_xattn, fold=build_fold)


def build(c: Case, dtype):
    return BUILD[c.kernel](c, dtype)


def forms(c: Case):
    """the kernel forms a case runs in: both forms of pp_ff_fused, one of everything else"""
    return ("w4", "w8") if c.kernel == "ff" else ("",)


def walk(c: Case, t, dtype, form="", defect=None):
    if c.kernel == "ff":
        return walk_ff(c, t, dtype, form == "w8", defect)
    if c.kernel == "tfront":
        return walk_tfront(c, t, dtype, defect)
    if c.kernel == "xattn":
        return walk_xattn(c, t, dtype, defect)
    return walk_fold(c, t, dtype, defect)


def judge(c: Case, t, dtype, got: dict):
    """What both test files assert of a finished run.  got: name -> tensor of the window's values (the format's values, the
    fp32 / int64 side outputs).  -> (list of failures, worst error / gate of the gated windows or None)"""
    bad, worst = [], None
    ref = dict(t["ref"])
    if c.kernel == "tfront":                               # Q, K, V: under their gate, from the hs that was stored
        hs = got["hs"]
        if bool(torch.isfinite(hs.double()).all()):
            ref.update(tfront_qkv_windows(c, t, hs.to(dtype) if hs.dtype == torch.float64 else hs, dtype))
        else:
            bad.append("hs: not finite")
    if c.kernel == "xattn" and c.probe == "R" and c.p["pre"]:   # the output from the h the kernel formed
        h = got["h"]
        if bool(torch.isfinite(h.double()).all()):
            h16 = h.to(dtype)
            ref["out"] = NC.gate_xattn_block(h16, 2, t["folded_nat"], t["inp"]["bo"], h16, c.p["rpb"], 1e-5, dtype, fold=bool(c.p["ln"]),
                                             terms=NC.kernel_moments_eps())
        else:
            bad.append("h: not finite")
    if c.kernel == "xattn" and c.probe == "R" and "stats" in got and bool(torch.isfinite(got["out"].double()).all()):
        S, Q, gs, gq = gate_row_stats_xattn(got["out"].double())
        ref["stats"] = (torch.stack([S, Q], -1).reshape(S.shape[0], -1), torch.stack([gs, gq], -1).reshape(S.shape[0], -1))
    if c.kernel == "ff" and c.probe == "R" and bool(torch.isfinite(got["out"].double()).all()):
        nb = c.p["M"] // c.p["rpb"] if c.p["rpb"] else 0
        for k, (cg, c0, G) in enumerate(c.p["gn"]):
            S, Q, gs, gq = NC.gate_epilogue_acc(got["out"].double().reshape(nb, c.p["rpb"], C320), c.p["rpb"], cg, c0, G, block_rows=128)
            a = got[f"acc{k}"].double().reshape(nb, G, 2)
            for nm, val, ex, gg in (("sum", a[..., 0] / NC.SUM_SCALE, S, gs), ("sumsq", a[..., 1] / NC.SQ_SCALE, Q, gq)):
                r = NC.worst_ratio(val, ex, gg)
                worst = r if worst is None else max(worst, r)
                if not r <= 1.0:
                    bad.append(f"acc{k} {nm}: error / gate {r:.3f}")
    for name, exp in ref.items():
        if name not in got:
            bad.append(name + ": missing")
            continue
        g = got[name].double()
        if isinstance(exp, tuple):
            r = NC.worst_ratio(g, exp[0], exp[1])
            worst = r if worst is None else max(worst, r)
            if not r <= 1.0:
                e = (g - exp[0]).abs() / exp[1].clamp_min(1e-300)
                e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
                idx = [int(v) for v in np.unravel_index(int(torch.argmax(e)), e.shape)]
                bad.append(f"{name}: error / gate {r:.3f}, worst at {idx}")
        else:
            ne = ~(g == exp.double())                      # (signed zeros compare equal; NaN never does)
            if bool(ne.any()):
                idx = ne.nonzero()[0].tolist()
                bad.append(f"{name}: not bit-equal at {int(ne.sum())} elements, first {idx}: {float(g[tuple(idx)])} "
                           f"expected {float(exp[tuple(idx)])}")
    return bad, worst


def walk_failures(c: Case, t, dtype, form="", defect=None):
    o = walk(c, t, dtype, form, defect)
    got, bad = {}, []
    for name, b in o.items():
        if isinstance(b, Buf):
            got[name] = b.view.clone()
            if not bool(torch.isnan(b.full[b.outside()]).all()):
                bad.append(name + ": stored outside the window")
        else:
            got[name] = b
    jb, worst = judge(c, t, dtype, got)
    return bad + jb, worst
