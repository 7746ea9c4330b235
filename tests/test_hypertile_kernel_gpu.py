"""-m gpu: the tiled form of attn_pipe_kernel (pp_attention_fwd_tiled) at the smallest shapes at which its address walk can go
wrong (tests/hypertile_cases.py: KERNEL_CASES), batch 2, heads 2, d = 40, bf16 and fp16, every named variant.

Per case, on random N(0, 1) operands in the padded buffers of tests/attention_cases.py (q | k column slices of one fused buffer
with 64 poisoned rows behind it, vt with ldvt = h*w + 8 and finite poison in the pad columns):
  (a) bit equality with the UNTILED kernel of the same variant run on explicitly gathered contiguous copies of the tiles
      (batch' = batch * nh * nw), scattered back: the per-query operation sequence is the same -- a query sits in the same wave
      and lane of the same query block of its tile, sees the same keys in the same 64-key LDS tiles in the same order -- so
      this is an equality, also for the partly filled query blocks of the 320-token tiles;
  (b) the float64 restatement `tiled_attention_f64` within the P3 gate of attention_cases evaluated at the TILE's key count;
  (c) key exactness: K and V^T of every token outside one tile replaced by other finite values -- that tile's output bits do
      not change, every other tile's do;
  (d) no stray writes: o has ldo = C + 8 and 8 extra rows and is pre-filled with a sentinel; nothing outside [batch*h*w, C] is
      touched, and every element inside is written (two runs over different sentinels give the same bits).
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attention_cases as AC  # noqa: E402
import hypertile_cases as HC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
B, H, D = 2, 2, 40
C = H * D
SCALE = D ** -0.5
_INPUTS = {}


def _inputs(h, w, nh, nw, dtype, log2):
    """Operands of one (shape, format, q form), built once and left unchanged: fused q | k buffer, v rows, vt (device), and the
    float64 reference with its gate, computed once from the 16-bit operands."""
    key = (h, w, nh, nw, dtype, log2)
    if key not in _INPUTS:
        n = h * w
        g = AC._gen(41, h, w)
        q = torch.randn(B * n, C, generator=g)
        k = torch.randn(B * n, C, generator=g)
        v = torch.randn(B * n, C, generator=g).to(dtype)
        if log2:
            q = q * (SCALE * AC.LOG2E)
        q = q.to(dtype)
        fused = AC._fused(B, H, n, n, D, dtype, k, DEV)
        fused[:B * n, :C] = q.to(DEV)
        vd = v.to(DEV)
        vt = AC.poison_vt(ops.transpose_v(vd, B, n, ldvt=n + 8), n)
        qc, kc, vc = (t.reshape(B, n, H, D) for t in (q, fused[:B * n, C:2 * C].cpu(), v))
        ref, A = HC.tiled_attention_f64(qc, kc, vc, h, w, nh, nw, math.log(2.0) if log2 else SCALE, with_abs=True)
        _INPUTS[key] = (fused, vd, vt, ref, HC.tile_gate(ref, A, vc, h, w, nh, nw, dtype))
    return _INPUTS[key]


def _guarded(n, dtype, launch_into, sentinel):
    rows = B * n
    full = torch.full((rows + 8, C + 8), sentinel, dtype=torch.int16, device=DEV)
    launch_into(full.view(dtype)[:rows, :C])
    torch.cuda.synchronize()
    out = full.view(dtype)[:rows, :C].clone()
    full[:rows, :C] = sentinel
    assert bool((full == sentinel).all()), "bytes outside the output rows / columns were written"
    assert bool(torch.isfinite(out.float()).all()), "non-finite output"
    return out


@pytest.mark.parametrize("name", ["PIPE_Q32", "PIPE_Q64", "PIPE_LOG2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("h,w,nh,nw", HC.KERNEL_CASES)
def test_tiled_kernel(h, w, nh, nw, dtype, name):
    variant, log2 = getattr(L, "PP_ATTN_" + name), name == "PIPE_LOG2"
    n, T = h * w, nh * nw
    nt = n // T
    assert L.lib().pp_attention_tiled_ok(h, w, nh, nw, D) == 1
    fused, v, vt, ref, gate = _inputs(h, w, nh, nw, dtype, log2)
    q, k = fused[:B * n, :C], fused[:B * n + AC.K_EXTRA_ROWS, C:2 * C]
    i16 = lambda t: t.contiguous().view(torch.int16)      # noqa: E731

    def tiled(k_, vt_):
        return lambda o: ops.attention_tiled(q, k_, vt_, B, H, h, w, nh, nw, D, scale=SCALE, variant=variant, out=o)

    # ---- (d) guarded output, every element written
    out = _guarded(n, dtype, tiled(k, vt), 0x5A5A)
    again = _guarded(n, dtype, tiled(k, vt), 0x2B2B)
    assert torch.equal(i16(out), i16(again)), "an in-range element keeps what the buffer held before the launch"

    # ---- (a) the untiled kernel of the same variant on gathered tiles
    tiles = lambda t: HC.to_tiles(t.reshape(B, n, C), h, w, nh, nw).reshape(B * T * nt, C).contiguous()      # noqa: E731
    qg, kg, vg = tiles(q), tiles(k[:B * n]), tiles(v)
    og = ops.attention(qg, kg, ops.transpose_v(vg, B * T, nt), B * T, H, nt, nt, D, scale=SCALE, variant=variant)
    want = HC.from_tiles(og.reshape(B * T, nt, C), B, h, w, nh, nw).reshape(B * n, C)
    differing = int((i16(out) != i16(want)).sum())
    print(f"[hypertile kernel] {name} {dtype} {(h, w, nh, nw)}: {differing} elements differ from the untiled kernel on gathered tiles")

    # ---- (b) float64 restatement within the gate at the tile's key count
    ratio = AC.worst_ratio(out.cpu().reshape(B, n, H, D), ref, gate)
    print(f"[hypertile kernel] {name} {dtype} {(h, w, nh, nw)}: worst error / gate {ratio:.3f} at {nt} keys per tile")

    # ---- (c) other finite values in K and V^T of every token outside one tile
    keep = T - 1 if T > 2 else 1
    tm = HC.token_map(h, w, nh, nw).to(DEV)
    outside = torch.ones(n, dtype=torch.bool, device=DEV)
    outside[tm[keep]] = False
    g = torch.Generator(device="cpu").manual_seed(7)
    k2 = torch.full_like(fused, AC.K_POISON)[:, C:2 * C]
    k2[:B * n] = torch.where(outside.repeat(B)[:, None], (3.0 * torch.randn(B * n, C, generator=g)).to(dtype).to(DEV), k[:B * n])
    vt2 = vt.clone()
    vt2[:, :, :n] = torch.where(outside[None, None, :], (2.0 * torch.randn(B, C, n, generator=g)).to(dtype).to(DEV), vt[:, :, :n])
    out2 = _guarded(n, dtype, tiled(k2, vt2), 0x5A5A)
    o1, o2 = out.reshape(B, n, C), out2.reshape(B, n, C)
    kept_same = torch.equal(i16(o1[:, tm[keep]]), i16(o2[:, tm[keep]]))
    others_differ = all(not torch.equal(i16(o1[:, tm[t]]), i16(o2[:, tm[t]])) for t in range(T) if t != keep)

    assert differing == 0, f"(a) {differing} elements differ from the untiled kernel on gathered tiles"
    assert ratio <= 1.0, f"(b) error / gate {ratio:.3f}"
    assert kept_same, "(c) keys outside a tile reached its output"
    assert others_differ, "(c) a tile's output ignores its own keys"
