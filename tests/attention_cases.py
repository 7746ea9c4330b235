"""Shared by the attention probe tests (not a test file): input builders, the fp64 reference, the derived error bounds and
a CPU restatement of the flash algorithm with named defects.  Plain torch; nothing here touches the HIP library.

The op:  O[b,i,h,:] = softmax_j(Q[b,i,h,:] . K[b,j,h,:] * scale) V[b,j,h,:]  (include/pp_hip.h: pp_attention_fwd with V
transposed, pp_attention_small with V in rows and an optional causal mask j <= i).  u is the unit roundoff of the 16-bit
format: 2^-8 for bf16, 2^-11 for fp16.

Memory, as every probe lays it out (`Setup`): q and k are column slices of ONE fused [M, 2C + 8] buffer (C = heads * d), k
has 64 rows behind the last batch item filled with the finite poison 16, vt has ldvt = round8(nk) + 8 with every pad
column [nk, ldvt) filled with the finite poison 1000.  A kernel may read those bytes (a 16-byte load straddles nk) but may
never let them reach the result.

Probe P1, one-hot gather.  Keys are random +-1 vectors, query i of (b, h) is 16 * K[b, pi(i), h] with a stride walk pi that
differs per (b, h): pi(i) = (s i + 3 b + 5 h + nk - 1) mod nk, s the first of 7, 9, 11, 13 coprime to nk (so that nk
consecutive i reach every key; i = 0 of (0, 0) is key nk - 1).  Where nq < nk the walk continues over ceil(nk / nq) launches.
The target's score is 16 d * scale; any other key differs in m >= 1 signs and scores 32 m * scale less, so with
random keys the softmax is one-hot: the builder asserts off-target mass <= 2^-20 per query from the fp64 reference.  The
expected output is V[b, pi(i), h]; the gate is |out - v| <= 2 u |v|: one u for P rounded once to 16 bits (numerator and
denominator see the same rounded P, so it mostly cancels), one u for the output rounding.  V is +-uniform[0.5, 2), so the
off-target contribution (<= 2 * 2^-20 * 2) is below u |v| / 60 and the gate needs no third term.  For the LOG2 form q is
round16(16 * scale * log2 e) * sign pattern: still exactly proportional to the key, products and sums exact in fp32.
A wrong key, tile, ring slot, batch item, head or key order of V against K is an O(1) error here.

Probe P2, uniform count.  q = 0, so every live key weighs 1 / nk whatever K holds; V[t, j] = 1 iff t mod d == j.  The
expected output is count_j / nk (causal: over keys 0..i).  Gate |out - ref| <= u (A + 2 |ref|) with A = P |V| = ref, i.e.
3 u ref: the probabilities are all the same power of two (no rounding at all), u for the denominator, u for the output.
One key too many or too few moves a column by >= 1 / (nk + 1) relative to count / nk with count <= 4: > 10x the gate up to
nk = 129, which is where P2 stops (beyond, the 16-bit output cannot resolve one key).  A pad column that leaks shows up
as 1000 / nk.

Probe P3, random data.  N(0, 1) inputs rounded to the format, fp64 reference.  Gate per element
    u (A + 2 |ref|) + 1e-5 A      [+ 2^-25 sum_j |V_j| for fp16],       A = P |V|:
u A -- every probability is rounded once to 16 bits before the P V MFMA; u |ref| -- the denominator, from rounded or
unrounded probabilities; u |ref| -- the output rounding; 1e-5 A -- fp32 score accumulation and the hardware exp2 at
|score| <= 300 (relative 2^-23 * 300 ~ 4e-5 on the argument only where the score is that large; N(0, 1) scores are < 16).
fp16: probabilities below 2^-14 of the running reference are subnormal (absolute error 2^-25 each); the running reference
lags the true maximum by less than 2^8, so the largest probability, hence the denominator, is >= 1.
pp_attention_small keeps P in fp32 and rounds only the output: u |ref| + 1e-5 A.
These are linear worst-case bounds, not statistics; the faithful emulation below reaches about 0.4 of the P3 gate.

`flash_emulate` restates the algorithm (64-key tiles, running maximum with the rescale deferred while it grows by < 2^8,
P rounded to the format, denominator from the rounded P) and carries the defects of MUTANTS by name;
tests/test_attention_probes.py proves on the CPU that every one of them fails a probe.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

LOG2E = 1.4426950408889634
KB = 64                      # keys per tile
QBLK = 128                   # queries per workgroup of the three-phase kernel
RESCALE_THR = 8.0
K_POISON, VT_POISON, K_EXTRA_ROWS = 16.0, 1000.0, 64
P1_MASS = 2.0 ** -20

MUTANTS = ("drop_last_key", "mask_lets_key_nk_in", "tail_half_skipped_at_33", "v_keys_swapped_in_16_block",
           "k_batch_stride_uses_nq", "b_h_swapped", "no_rescale_on_max_jump", "second_query_block_keeps_state",
           "ring_slot_off_by_one", "causal_lt", "p_rounded_to_bf16_in_fp16_mode")

# ------------------------------------------------------------------------------------------------ the GPU matrix
B_, H_ = 2, 3                # odd head count: b / h asymmetric, C = 3 d keeps ldq % 8 == 0
PHASED_D = (40, 80, 160)
PHASED_NK = (4, 13, 32, 33, 64, 65, 77, 96, 97, 128, 129, 200)
PHASED_NQ = (4, 33, 130)
# K / V-reuse form: launch_attn takes it when ceil(nq / 128) * heads * batch >= 2048, nk <= 128 and d == 40
QR_B, QR_H = 8, 8
QR_CASES = [(nq, nk) for nk in (77, 128) for nq in (4096, 3996, 4224)]
PIPE_CASES = [(200, nk) for nk in (256, 320, 384, 448, 512, 576, 640, 704, 768)] + [(33, 256), (257, 256)]
SMALL_D = 64
SMALL_N = (1, 5, 63, 64, 65, 77, 127, 128)
SMALL_RECT = ((77, 5), (5, 128), (130, 65))


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def round8(n: int) -> int:
    return (n + 7) // 8 * 8


def _gen(*key) -> torch.Generator:
    seed = 0
    for x in key:
        seed = (seed * 1000003 + int(x) + 17) % (2 ** 31 - 1)
    return torch.Generator("cpu").manual_seed(seed)


@dataclass
class Setup:
    """One probe's inputs.  `fused` [M, 2C + 8]: q = fused[:B*nq, :C] (filled per launch from `q`), k = fused[:B*nk+64, C:2C];
    `v` [B*nk, C] the values in rows; expected[l] / gate[l] [B*nq, C] in fp64 per launch l."""
    probe: str
    B: int
    H: int
    nq: int
    nk: int
    d: int
    dtype: torch.dtype
    scale: float
    causal: bool
    log2: bool
    fused: torch.Tensor
    v: torch.Tensor
    q: List[torch.Tensor] = field(default_factory=list)
    expected: List[torch.Tensor] = field(default_factory=list)
    gate: List[torch.Tensor] = field(default_factory=list)

    @property
    def C(self):
        return self.H * self.d

    @property
    def ldvt(self):
        return round8(self.nk) + 8

    def k_view(self):
        return self.fused[:self.B * self.nk + K_EXTRA_ROWS, self.C:2 * self.C]

    def q_view(self, launch: int):
        qv = self.fused[:self.B * self.nq, :self.C]
        qv.copy_(self.q[launch])
        return qv

    def vt_torch(self):
        """vt [B, C, ldvt] with poisoned pads, by plain torch (the GPU tests take ops.transpose_v + poison_vt instead)"""
        vt = self.v.view(self.B, self.nk, self.C).permute(0, 2, 1)
        pad = torch.zeros(self.B, self.C, self.ldvt - self.nk, dtype=self.dtype, device=self.v.device)
        return poison_vt(torch.cat([vt, pad], 2).contiguous(), self.nk)


def poison_vt(vt: torch.Tensor, nk: int) -> torch.Tensor:
    vt[..., nk:] = VT_POISON
    return vt


def _fused(B, H, nq, nk, d, dtype, k_rows: torch.Tensor, device) -> torch.Tensor:
    C = H * d
    M = max(B * nq, B * nk + K_EXTRA_ROWS)
    fused = torch.full((M, 2 * C + 8), K_POISON, dtype=dtype)
    fused[:B * nk, C:2 * C] = k_rows.to(dtype)
    return fused.to(device)


def _heads(t: torch.Tensor, B, n, H, d) -> torch.Tensor:
    return t[:B * n].reshape(B, n, H, d).permute(0, 2, 1, 3)


def reference(q, k, v, B, H, nq, nk, d, scale, causal=False, log2=False, target=None):
    """fp64 attention of the 16-bit operands q [B*nq, C], k [>= B*nk, C], v [B*nk, C], one batch item at a time.
    log2: softmax over exp2(q . k), scale not applied (what PP_ATTN_PIPE_LOG2 computes from a pre-multiplied q).
    -> (ref, A = P |V|, both [B*nq, C] fp64, off-target mass [B*nq, H] where target [B*nq, H] names a key, else None)."""
    C = H * d
    ref = torch.empty(B * nq, C, dtype=torch.float64, device=q.device)
    A = torch.empty_like(ref)
    mass = torch.empty(B * nq, H, dtype=torch.float64, device=q.device) if target is not None else None
    mult = math.log(2.0) if log2 else scale
    for b in range(B):
        qh = q[b * nq:(b + 1) * nq].double().view(nq, H, d).transpose(0, 1)
        kh = k[b * nk:(b + 1) * nk].double().view(nk, H, d).transpose(0, 1)
        vh = v[b * nk:(b + 1) * nk].double().view(nk, H, d).transpose(0, 1)
        s = torch.matmul(qh, kh.transpose(1, 2)) * mult
        if causal:
            i = torch.arange(nq, device=q.device)[:, None]
            j = torch.arange(nk, device=q.device)[None, :]
            s = s.masked_fill(j > i, -math.inf)
        p = torch.softmax(s, -1)
        ref[b * nq:(b + 1) * nq] = torch.matmul(p, vh).transpose(0, 1).reshape(nq, C)
        A[b * nq:(b + 1) * nq] = torch.matmul(p, vh.abs()).transpose(0, 1).reshape(nq, C)
        if target is not None:
            tg = target[b * nq:(b + 1) * nq].transpose(0, 1)[..., None]            # [H, nq, 1]
            mass[b * nq:(b + 1) * nq] = p.scatter(2, tg, 0.0).sum(-1).transpose(0, 1)
    return ref, A, mass


def gate_p3(ref, A, v, B, H, nk, d, dtype, p_fp32=False):
    u = unit_roundoff(dtype)
    if p_fp32:
        return u * ref.abs() + 1e-5 * A
    g = u * (A + 2 * ref.abs()) + 1e-5 * A
    if dtype == torch.float16:
        colsum = v.double().abs().view(B, nk, H * d).sum(1)                        # [B, C]
        nq = ref.shape[0] // B
        g = g + 2.0 ** -25 * colsum.repeat_interleave(nq, 0)
    return g


def worst_ratio(out, expected, gate) -> float:
    """max |out - expected| / gate; an error where the gate is 0, or a non-finite output, is inf."""
    err = (out.double() - expected).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    r = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ builders
def p1_stride(nk: int) -> int:
    return next(s for s in (7, 9, 11, 13) if math.gcd(s, nk) == 1)


def p1_launches(nq: int, nk: int, causal: bool) -> int:
    return 2 if causal else (nk + nq - 1) // nq if nq < nk else 1


def p1_targets(B, H, nq, nk, launch: int, causal: bool) -> torch.Tensor:
    """pi [B*nq, H].  Causal (pi(i) <= i): launch 0 is the diagonal (key i is the last visible one), launch 1 a walk inside
    the visible keys."""
    i = torch.arange(nq)[None, :, None]
    b = torch.arange(B)[:, None, None]
    h = torch.arange(H)[None, None, :]
    s = p1_stride(nk)
    if causal:
        pi = i + 0 * (b + h) if launch == 0 else (s * i + 3 * b + 5 * h) % (i + 1)
    else:
        pi = (s * (i + launch * nq) + 3 * b + 5 * h + nk - 1) % nk
    return pi.reshape(B * nq, H)


def build_p1(B, H, nq, nk, d, dtype, scale=None, causal=False, log2=False, device="cpu") -> Setup:
    scale = d ** -0.5 if scale is None else scale
    g = _gen(1, B, H, nq, nk, d)
    C = H * d
    k = torch.randint(0, 2, (B * nk, C), generator=g).float() * 2 - 1
    sgn = torch.randint(0, 2, (B * nk, C), generator=g).float() * 2 - 1
    v = (sgn * (0.5 + 1.5 * torch.rand(B * nk, C, generator=g))).to(dtype)
    amp = float(torch.tensor(16.0 * scale * LOG2E).to(dtype)) if log2 else 16.0
    s = Setup("P1", B, H, nq, nk, d, dtype, scale, causal, log2, _fused(B, H, nq, nk, d, dtype, k, device), v.to(device))
    kh = k.view(B, nk, H, d)
    vh = v.view(B, nk, H, d)
    u = unit_roundoff(dtype)
    for launch in range(p1_launches(nq, nk, causal)):
        pi = p1_targets(B, H, nq, nk, launch, causal)
        idx = pi.view(B, nq, H, 1).expand(B, nq, H, d)
        s.q.append((amp * torch.gather(kh, 1, idx)).reshape(B * nq, C).to(dtype).to(device))
        want = torch.gather(vh, 1, idx).reshape(B * nq, C).double().to(device)
        _, _, mass = reference(s.q[-1], s.k_view(), s.v, B, H, nq, nk, d, scale, causal, log2, target=pi.to(device))
        assert float(mass.max()) <= P1_MASS, ("P1 precondition: off-target mass", (B, H, nq, nk, d), float(mass.max()))
        s.expected.append(want)
        s.gate.append(2 * u * want.abs())
    return s


def p1_covers_every_key(B, H, nq, nk, causal=False) -> bool:
    hit = torch.zeros(B, H, nk, dtype=torch.bool)
    for launch in range(p1_launches(nq, nk, causal)):
        pi = p1_targets(B, H, nq, nk, launch, causal).view(B, nq, H).permute(0, 2, 1)
        hit.scatter_(2, pi, True)
    return bool(hit.all())


def build_p2(B, H, nq, nk, d, dtype, scale=None, causal=False, log2=False, device="cpu") -> Setup:
    scale = d ** -0.5 if scale is None else scale
    g = _gen(2, B, H, nq, nk, d)
    C = H * d
    k = torch.randn(B * nk, C, generator=g)
    t = torch.arange(nk)
    ind = (t[:, None] % d == torch.arange(d)[None, :]).float()                    # [nk, d]
    v = ind[None, :, None, :].expand(B, nk, H, d).reshape(B * nk, C).to(dtype)
    s = Setup("P2", B, H, nq, nk, d, dtype, scale, causal, log2, _fused(B, H, nq, nk, d, dtype, k, device), v.to(device))
    s.q.append(torch.zeros(B * nq, C, dtype=dtype, device=device))
    if causal:
        ref = ind.double().cumsum(0)[:nq] / (torch.arange(nq).double()[:, None] + 1)     # [nq, d]
    else:
        ref = (ind.double().sum(0) / nk)[None, :].expand(nq, d)
    ref = ref[None, :, None, :].expand(B, nq, H, d).reshape(B * nq, C).contiguous().to(device)
    s.expected.append(ref)
    s.gate.append(3 * unit_roundoff(dtype) * ref)
    return s


def build_p3(B, H, nq, nk, d, dtype, scale=None, causal=False, log2=False, p_fp32=False, device="cpu") -> Setup:
    scale = d ** -0.5 if scale is None else scale
    g = _gen(3, B, H, nq, nk, d)
    C = H * d
    q = torch.randn(B * nq, C, generator=g)
    k = torch.randn(B * nk, C, generator=g)
    v = torch.randn(B * nk, C, generator=g).to(dtype)
    if log2:
        q = q * (scale * LOG2E)
    s = Setup("P3", B, H, nq, nk, d, dtype, scale, causal, log2, _fused(B, H, nq, nk, d, dtype, k, device), v.to(device))
    s.q.append(q.to(dtype).to(device))
    ref, A, _ = reference(s.q[0], s.k_view(), s.v, B, H, nq, nk, d, scale, causal, log2)
    s.expected.append(ref)
    s.gate.append(gate_p3(ref, A, s.v, B, H, nk, d, dtype, p_fp32))
    return s


BUILDERS = {"P1": build_p1, "P2": build_p2, "P3": build_p3}


# ------------------------------------------------------------------------------------------------ the emulation
def _round(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(dtype).float()


def flash_emulate(q, kmem, vt, B, H, nq, nk, d, scale, dtype, mutant: Optional[str] = None, causal=False, log2=False,
                  qrep=1, round_p=True):
    """The algorithm on the memory the kernel is given: q [B*nq, C], kmem [rows >= B*nk, C] (row b*nk + t = key t of item
    b; rows past the buffer read as zeros), vt [B, C, ldvt].  qrep: a workgroup serves qrep blocks of 128 queries in turn
    (the K / V-reuse form); round_p=False keeps P in fp32 (pp_attention_small).  -> o [B*nq, C] in `dtype`."""
    assert mutant is None or mutant in MUTANTS, mutant
    C = H * d
    ntiles = (nk + KB - 1) // KB
    NP = ntiles * KB
    dev = q.device
    # ---- addressing
    kbase = torch.arange(B, device=dev) * (nq if mutant == "k_batch_stride_uses_nq" else nk)
    rows = kbase[:, None] + torch.arange(NP, device=dev)[None, :]                         # [B, NP]
    inside = rows < kmem.shape[0]
    Kg = kmem[rows.clamp_max(kmem.shape[0] - 1)].double() * inside[..., None]            # [B, NP, C]
    Kg = Kg.view(B, NP, H, d).permute(0, 2, 1, 3)                                         # [B, H, NP, d]
    bb, hh = torch.meshgrid(torch.arange(B, device=dev), torch.arange(H, device=dev), indexing="ij")
    lin = hh * B + bb if mutant == "b_h_swapped" else bb * H + hh                         # V^T base of (b, h)
    Vg = vt.reshape(B * H, d, vt.shape[2])[lin].double()                                  # [B, H, d, ldvt]
    if Vg.shape[3] < NP:
        Vg = torch.cat([Vg, torch.zeros(B, H, d, NP - Vg.shape[3], dtype=torch.float64, device=dev)], 3)
    Vg = Vg[..., :NP].transpose(2, 3)                                                     # [B, H, NP, d]
    pos = torch.arange(NP, device=dev)
    if mutant == "v_keys_swapped_in_16_block":
        w = pos % 16
        pos = pos - w + torch.where((w >= 4) & (w < 8), w + 4, torch.where((w >= 8) & (w < 12), w - 4, w))
        Vg = Vg[:, :, pos]
    if mutant == "ring_slot_off_by_one":
        Vg = torch.cat([Vg[:, :, :KB], Vg[:, :, :NP - KB]], 2) if ntiles > 1 else Vg
    # ---- which key positions are live
    limit = nk - 1 if mutant == "drop_last_key" else nk + 1 if mutant == "mask_lets_key_nk_in" else nk
    j = torch.arange(NP, device=dev)
    live = (j < limit)[None, :].expand(nq, NP).clone()
    if mutant == "tail_half_skipped_at_33" and nk - (ntiles - 1) * KB == 33:
        live[:, (ntiles - 1) * KB + 32:] = False
    if causal:
        i = torch.arange(nq, device=dev)[:, None]
        live &= (j[None, :] < i) if mutant == "causal_lt" else (j[None, :] <= i)
    pdt = torch.bfloat16 if mutant == "p_rounded_to_bf16_in_fp16_mode" else dtype
    c = torch.tensor(1.0 if log2 else scale * LOG2E, dtype=torch.float32, device=dev)
    Qh = q.double().view(B, nq, H, d).permute(0, 2, 1, 3)                                 # [B, H, nq, d]

    def run(r0, r1, state):
        R = r1 - r0
        if state is None:
            O = torch.zeros(B, H, R, d, dtype=torch.float32, device=dev)
            m = torch.full((B, H, R), -1.0e30, dtype=torch.float32, device=dev)
            l = torch.zeros(B, H, R, dtype=torch.float32, device=dev)
        else:
            O, m, l = (t[:, :, :R].clone() for t in state)
        for t in range(ntiles):
            sl = slice(t * KB, (t + 1) * KB)
            lv = live[r0:r1, sl][None, None]
            s = torch.matmul(Qh[:, :, r0:r1], Kg[:, :, sl].transpose(2, 3)).float()
            s = torch.where(lv, s, torch.full_like(s, -1.0e30))
            tmax = s.max(-1).values * c
            jump = tmax - m > RESCALE_THR
            m_new = torch.where(jump, torch.maximum(m, tmax), m)
            alpha = torch.where(jump, torch.exp2(m - m_new), torch.ones_like(m))
            if mutant == "no_rescale_on_max_jump":
                alpha = torch.ones_like(m)
            m = m_new
            p = torch.where(lv, torch.exp2(s * c - m[..., None]), torch.zeros_like(s))
            if round_p:
                p = _round(p, pdt)
            O = O * alpha[..., None] + torch.matmul(p.double(), Vg[:, :, sl]).float()
            l = l * alpha + p.sum(-1)
        return O, m, l

    out = torch.empty(B, H, nq, d, dtype=torch.float32, device=dev)
    if qrep == 1:
        O, _, l = run(0, nq, None)
        out[:] = O / l[..., None]
    else:
        for r0 in range(0, nq, QBLK):
            blk = r0 // QBLK
            keep = mutant == "second_query_block_keeps_state" and blk % qrep != 0
            state = run(r0, min(r0 + QBLK, nq), state if keep else None)               # noqa: F821 (set by the block before)
            out[:, :, r0:r0 + QBLK] = state[0] / state[2][..., None]
    return out.permute(0, 2, 1, 3).reshape(B * nq, C).to(dtype)
