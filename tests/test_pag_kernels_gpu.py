"""-m gpu: the two kernels of perturbed-attention guidance (csrc/pag.hip), bit for bit.

pp_attn_identity_v is a 16-bit bit copy, out[b][p][c] = vt[b][c][p]: compared bitwise with `vt.transpose`, the pad columns of
V^T holding NaN patterns and `out` pre-filled with a sentinel that must survive everywhere outside the addressed rows and
columns.  pp_pag_combine is compared bitwise on operands whose every intermediate is exact in fp32 whatever the contraction
(e's multiples of 1/4 up to 2 in size, g = 7.5, s multiples of 1/4: every product is a multiple of 1/16 below 2^6, every
sum too), and on random operands against the float64 restatement of tests/pag_cases.py under a bound derived below.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import pag_cases as PC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
SENTINEL = 0x5A5A
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}

# (n, C, ldvt, ldo, items, batch0, batch, dtype pattern, element offsets of (vt, out) inside their allocations)
CASES = [
    (1, 8, 8, 8, 1, 0, 1, torch.bfloat16, (0, 0)),
    (4, 1280, 8, 1280, 2, 0, 2, torch.float16, (0, 0)),            # 2x2 latents: ldvt 8
    (15, 40, 16, 40, 3, 0, 3, torch.bfloat16, (0, 0)),
    (60, 320, 64, 320, 3, 2, 1, torch.bfloat16, (0, 0)),           # 6x10; the perturbed third of a CFG batch
    (64, 320, 64, 328, 2, 1, 1, torch.float16, (0, 0)),            # ldo = C + 8
    (72, 40, 96, 40, 2, 0, 2, torch.bfloat16, (0, 0)),             # ldvt = n + 24
    (169, 320, 176, 320, 5, 2, 2, torch.float16, (0, 0)),          # a window inside a larger batch
    (1024, 1280, 1024, 1280, 3, 2, 1, torch.bfloat16, (0, 0)),
    (64, 8, 64, 8, 2, 1, 1, torch.bfloat16, (0, 0)),
    (169, 40, 176, 48, 3, 1, 2, torch.bfloat16, (1, 3)),           # pointers off the 16-byte grid: the narrow-access path
    (130, 72, 136, 72, 2, 0, 2, torch.float16, (8, 8)),            # more than one tile both ways, neither a multiple of 64
]


def _bits(shape, dtype, seed):
    """Random values of the format as int16 bit patterns (normal numbers of both signs, a few zeros)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 3
    x[torch.rand(*shape, generator=g) < 0.01] = 0.0
    return x.to(dtype).view(torch.int16)


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_C{c[1]}_ldvt{c[2]}_ldo{c[3]}_b{c[5]}+{c[6]}of{c[4]}" for c in CASES])
def test_attn_identity_v_is_the_transpose_bit_for_bit(case):
    n, C, ldvt, ldo, items, b0, nb, dtype, (off_v, off_o) = case
    vt = torch.full((items, C, ldvt), NAN16[dtype], dtype=torch.int16)
    vt[:, :, :n] = _bits((items, C, n), dtype, seed=n + C)
    vbuf = torch.full((off_v + vt.numel() + 16,), NAN16[dtype], dtype=torch.int16)
    vbuf[off_v:off_v + vt.numel()] = vt.flatten()
    obuf = torch.full((off_o + items * n * ldo + 16,), SENTINEL, dtype=torch.int16)
    want = obuf.clone()
    w = want[off_o:off_o + items * n * ldo].view(items, n, ldo)
    w[b0:b0 + nb, :, :C] = PC.identity_v_ref(vt[b0:b0 + nb], n)
    vd, od = vbuf.to(DEV), obuf.to(DEV)
    v_view = vd[off_v:off_v + vt.numel()].view(items, C, ldvt).view(dtype)
    o_view = od[off_o:off_o + items * n * ldo].view(items * n, ldo).view(dtype)
    ops.attn_identity_v(v_view, n, o_view, batch0=b0, batch=nb)
    torch.cuda.synchronize()
    got = od.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} 16-bit words differ"
    assert torch.equal(vd.cpu(), vbuf), "V^T was written"


def test_attn_identity_v_inverts_transpose_v():
    B, n, C = 2, 60, 320
    v = _bits((B * n, C), torch.bfloat16, seed=7).view(torch.bfloat16).to(DEV)
    vt = ops.transpose_v(v, B, n)
    assert vt.shape == (B, C, 64)
    out = torch.zeros_like(v)
    ops.attn_identity_v(vt, n, out)
    assert torch.equal(out.view(torch.int16), v.view(torch.int16))


def _exact_operands(segs, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (segs, n), generator=g).float() / 4


@pytest.mark.parametrize("cfg", [1, 0])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 8 * 8 * 2])
def test_pag_combine_exact(n, cfg):
    segs = 3 if cfg else 2
    table = torch.tensor([3.0, 0.25, 1.25, 0.0, 2.5])
    g = 7.5
    for row in (0, 2, 4):
        for off in ((0, 1) if n % 4 == 0 else (0,)):                  # (off 1: n % 4 == 0 but no 16-byte alignment)
            e = _exact_operands(segs, n, seed=n + row)
            buf = torch.full((off + segs * n + 64,), 777.0)
            buf[off:off + segs * n] = e.flatten()
            d = buf.to(DEV)
            step = torch.tensor([row], dtype=torch.int32, device=DEV)
            ops.pag_combine(d[off:off + segs * n].view(segs, n), bool(cfg), g, table.to(DEV), step)
            torch.cuda.synchronize()
            got = d.cpu()
            want = buf.clone()
            want[off:off + n] = torch.from_numpy(PC.combine_f64(e.numpy(), cfg, g, float(table[row]))).float()
            assert torch.equal(got[off:off + n], want[off:off + n]), (row, off)
            assert torch.equal(got, want), "segments 1.., the bytes in front or the guard behind the buffer changed"
            assert int(step.item()) == row, "the step counter moved"


@pytest.mark.parametrize("cfg", [1, 0])
def test_pag_combine_random_against_float64(cfg):
    """Bound.  With u = 2^-24 and d1 = e_c - e_u, d2 = e_c - e_p: each difference, each product and each of the two sums
    rounds once (a contracted multiply-add rounds less).  The products carry (1 + u)^2 - 1 of g|d1| and s|d2|, the sums add
    u of a partial result no larger than M = |e_u| + g|d1| + s|d2|:  |error| <= 2u g|d1| + 2u s|d2| + 2u M <= 4u M, and the
    terms of order u^2 fit in the factor (1 + 2^-20).  g and s are fp32 numbers on both sides."""
    segs, n = (3 if cfg else 2), 4099
    gq = torch.Generator().manual_seed(11 + cfg)
    e = torch.randn(segs, n, generator=gq) * 2
    g32, s32 = np.float32(7.3), np.float32(2.7)
    table = torch.tensor([0.0, float(s32)], dtype=torch.float32)
    d = e.clone().to(DEV)
    ops.pag_combine(d, bool(cfg), float(g32), table.to(DEV), torch.tensor([1], dtype=torch.int32, device=DEV))
    got = d.cpu().numpy().astype(np.float64)
    e64 = e.numpy().astype(np.float64)
    want = PC.combine_f64(e64, cfg, np.float64(g32), np.float64(s32))
    if cfg:
        M = np.abs(e64[0]) + np.float64(g32) * np.abs(e64[1] - e64[0]) + np.float64(s32) * np.abs(e64[1] - e64[2])
    else:
        M = np.abs(e64[0]) + np.float64(s32) * np.abs(e64[0] - e64[1])
    bound = 4 * 2.0 ** -24 * M * (1 + 2.0 ** -20)
    err = np.abs(got[0] - want)
    print(f"[pag combine] cfg={cfg}: worst error / bound {float((err / bound).max()):.3f}, max error {float(err.max()):.3e}")
    assert (err <= bound).all()
    assert np.array_equal(got[1:], e64[1:])
