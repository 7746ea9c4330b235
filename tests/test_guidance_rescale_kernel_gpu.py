"""-m gpu: pp_cfg_rescale (csrc/guidance.hip) -- the guided prediction rescaled per sample, in one launch.

Every launch here runs on a buffer with guard words in front of and behind eps that must survive; segments 1 and up, PAG's
table, the phi cell and the step counter must come back unchanged.

Exact probes (operands multiples of 1/4 up to 2 in size: every combine is exact, whatever the contraction) are compared bit
for bit; so are the batch-of-3 / batch-of-1 runs of the position-independence test.  Random operands are compared with the
float64 restatement of tests/guidance_cases.py under the bound derived in `_bound`.
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
import guidance_cases as GC  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
GUARD, PAD = 777.0, 64
SHAPES = [(1, 2), (1, 3), (3, 140), (2, 1023), (2, 4 * 8 * 8), (5, 4 * 6 * 10), (1, 4 * 64 * 64 + 4), (2, 4 * 128 * 128)]
TABLE = [3.0, 1.25, 0.0]                       # PAG's per-row scales; rows 0 and 2 are used
THREADS, WAVES = 1024, 16                     # the kernel's workgroup: one per sample


def _offsets(per):
    return (0, 1) if per % 4 == 0 else (0,)   # (1: per % 4 == 0 but eps one float off the 16-byte grid: the scalar path)


def _launch(e, g, phi, row=None, off=0):
    """e: float32 [segs][B][per] on the host -> (segment 0 after the launch [B][per], on the host); checks everything the
    launch must not write.  segs = 3 reads TABLE[row]."""
    segs, B, per = e.shape
    n = e.numel()
    buf = torch.full((PAD + off + n + PAD,), GUARD)
    buf[PAD + off:PAD + off + n] = e.flatten()
    d = buf.to(DEV)
    view = d[PAD + off:PAD + off + n].view(segs, B, per)
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    cell = torch.tensor([phi], dtype=torch.float32, device=DEV)
    table = torch.tensor(TABLE, dtype=torch.float32, device=DEV) if segs == 3 else None
    step = torch.tensor([row], dtype=torch.int32, device=DEV) if segs == 3 else None
    ops.cfg_rescale(view, g, cell, pag_table=table, step=step)
    torch.cuda.synchronize()
    got = d.cpu()
    lo, hi = PAD + off, PAD + off + B * per
    assert torch.equal(got[:lo], buf[:lo]), "the words in front of eps changed"
    assert torch.equal(got[hi:], buf[hi:]), "segments 1.. or the guard behind eps changed"
    assert float(cell.item()) == float(np.float32(phi)), "the phi cell was written"
    if segs == 3:
        assert table.cpu().tolist() == TABLE and int(step.item()) == row, "the table or the step counter was written"
    return got[lo:hi].view(B, per).clone()


def _exact(B, per, seed):
    """Multiples of 1/4 up to 2 in size, no sample constant (its first two values differ)."""
    x = torch.randint(-8, 9, (B, per), generator=torch.Generator().manual_seed(seed)).float() / 4
    x[:, 0], x[:, 1] = 0.25, -0.5
    return x


# ------------------------------------------------------------------------------------------------ exact probes
@pytest.mark.parametrize("B,per", SHAPES, ids=[f"b{b}_per{p}" for b, p in SHAPES])
def test_exact_probes_bit_for_bit(B, per):
    """g = 1: the combine IS e_c, the two SSDs are the same numbers, the factor is phi + (1 - phi) = 1: the result is e_c.
    e_u = 0, g = 2: m = 2 e_c exactly, every partial sum of m is twice that of e_c, SSD(m) = 4 SSD(e_c), the ratio is 1/2:
    the result is e_c at phi = 1 and 0.75 m at phi = 0.5.  With a third segment e_p = e_c the PAG term is s * 0 under any s."""
    ec, eu = _exact(B, per, seed=per + B), _exact(B, per, seed=per + B + 1)
    for segs, rows in ((2, (None,)), (3, (0, 2))):
        for row in rows:
            for off in _offsets(per):
                for phi in (0.5, 1.0):
                    e = torch.stack([eu, ec] + ([ec] if segs == 3 else []))
                    got = _launch(e, 1.0, phi, row, off)
                    assert torch.equal(got, ec), ("g = 1", segs, row, off, phi)
                for phi, want in ((1.0, ec), (0.5, 0.75 * (2.0 * ec))):
                    e = torch.stack([torch.zeros_like(ec), ec] + ([ec] if segs == 3 else []))
                    got = _launch(e, 2.0, phi, row, off)
                    assert torch.equal(got, want), ("e_u = 0, g = 2", segs, row, off, phi)


# ------------------------------------------------------------------------------------------------ position independence
@pytest.mark.parametrize("segs", [2, 3])
@pytest.mark.parametrize("per", [140, 1023, 4 * 8 * 8, 4 * 6 * 10])
def test_a_sample_does_not_see_its_batch(per, segs):
    """One base sample scaled by 1, 2^10 and 2^-10 (exact in fp32: every intermediate scales with it, the ratio does not
    move).  A deviation taken over the whole batch would be dominated by the 2^10 sample."""
    gq = torch.Generator().manual_seed(per + segs)
    base = torch.randn(segs, 1, per, generator=gq) + 0.5
    e = torch.cat([base, base * 2.0 ** 10, base * 2.0 ** -10], dim=1)
    row = 0 if segs == 3 else None
    for off in _offsets(per):
        got = _launch(e, 7.5, 0.7, row, off)
        assert torch.equal(_launch(e, 7.5, 0.7, row, off), got), "two runs differ"
        for b in range(3):
            assert torch.equal(_launch(e[:, b:b + 1].contiguous(), 7.5, 0.7, row, off)[0], got[b]), f"sample {b} alone differs"
        assert torch.equal(got[0] * 2.0 ** 10, got[1]) and torch.equal(got[0] * 2.0 ** -10, got[2])
        # and as the last of five, behind other samples
        five = torch.cat([torch.randn(segs, 4, per, generator=gq) * 3, base], dim=1)
        assert torch.equal(_launch(five, 7.5, 0.7, row, off)[4], got[0])


# ------------------------------------------------------------------------------------------------ random input
def _depth(per, vec):
    """The longest chain of additions one term of a sum passes through in the kernel: thread t adds its elements in sequence
    (on the 16-byte path four at a time, as (x0 + x1) + (x2 + x3): 2 levels in front of the chain), 6 __shfl_xor levels,
    16 wave totals in sequence."""
    chain = -(-(per // 4 if vec else per) // THREADS)
    return chain + (2 if vec else 0) + 6 + WAVES


def _bound(e64, segs, g, s, phi, vec):
    """Per-element bound on |kernel - rescale_f64|, first order in u = 2^-24 with 1 % for the higher orders (asserted small).

    Combine.  m^ = m + eps, |eps| <= 4 u M with M = |e_u| + g |e_c - e_u| + s |e_c - e_p| (test_pag_kernels_gpu.py; the
    two-segment combine rounds less).
    Mean.  A sum of n terms in which every term passes through at most D additions carries at most D u sum|x|; the division
    by n rounds once more: |mean^ - mean| <= (D + 1) u mean|x| =: dmu (for m the data are m^: mean|m^| <= mean M, and the
    mean of eps adds 4 u mean M).
    SSD.  d^_i = fl(x^_i - mean^) = a_i + p_i with a_i the true deviation and |p_i| <= |eps_i| + dmu + u |a_i|; by the
    triangle inequality | ||d^|| - ||a|| | <= ||eps|| + sqrt(n) dmu + u ||a||.  Squares round once (u), the sum of the
    non-negative squares carries D u relatively; the square root halves both.  Relative error of sqrt(SSD):
        rho(x) = (||eps|| + sqrt(n) dmu) / ||a|| + u + (D + 1) u / 2
    Factor.  r^ = sqrt(SSD_c^ / SSD_m^): the division and the root round once each (the root halves the division's):
    |r^ - r| <= r (rho(c) + rho(m) + 2 u).  f^ = phi r^ + fl(1 - phi): at most three roundings of non-negative terms:
    |f^ - f| <= phi |r^ - r| + 3 u f.
    Output.  out = fl(m^ f^):  |out - m f| <= |eps| f + |m| |f^ - f| + u |m| f."""
    n = e64.shape[2]
    D = _depth(n, vec)
    eu, ec = e64[0], e64[1]
    M = np.abs(eu) + g * np.abs(ec - eu) + (s * np.abs(ec - e64[2]) if segs == 3 else 0.0)
    m = GC.combine_f64(e64, segs, g, s)
    eps = 4 * U * M
    norm = lambda x: np.sqrt((x * x).sum(axis=1, keepdims=True))      # noqa: E731
    dev = lambda x: x - x.mean(axis=1, keepdims=True)                # noqa: E731
    dmu_c = (D + 1) * U * np.abs(ec).mean(axis=1, keepdims=True)
    dmu_m = (D + 1 + 4) * U * M.mean(axis=1, keepdims=True)
    rho_c = np.sqrt(n) * dmu_c / norm(dev(ec)) + U + (D + 1) * U / 2
    rho_m = (norm(eps) + np.sqrt(n) * dmu_m) / norm(dev(m)) + U + (D + 1) * U / 2
    assert float(max(rho_c.max(), rho_m.max())) < 2.0 ** -10, "the first-order bound needs small relative errors"
    r = GC.ratio_f64(e64, segs, g, s)
    f = phi * r + (1.0 - phi)
    df = phi * r * (rho_c + rho_m + 2 * U) + 3 * U * f
    return 1.01 * (eps * f + np.abs(m) * df + U * np.abs(m) * f)


@pytest.mark.parametrize("B,per", SHAPES, ids=[f"b{b}_per{p}" for b, p in SHAPES])
def test_random_against_float64(B, per):
    """Per element under `_bound`; g, s and phi are fp32 numbers on both sides."""
    g32, phi32 = np.float32(7.3), np.float32(0.7)
    for segs, rows in ((2, (None,)), (3, (0, 2))):
        for row in rows:
            for off in _offsets(per):
                e = torch.randn(segs, B, per, generator=torch.Generator().manual_seed(per + 7 * segs + B)) * 2
                if per < 4:
                    e[1, :, 0] += 1.0                       # (two or three values: keep e_c's deviation away from 0)
                got = _launch(e, float(g32), float(phi32), row, off).numpy().astype(np.float64)
                e64 = e.numpy().astype(np.float64)
                s = TABLE[row] if segs == 3 else 0.0
                want = GC.rescale_f64(e64, segs, np.float64(g32), s, np.float64(phi32))
                bound = _bound(e64, segs, np.float64(g32), s, np.float64(phi32), vec=(per % 4 == 0 and off == 0))
                err = np.abs(got - want)
                print(f"[cfg_rescale] b={B} per={per} segs={segs} row={row} off={off}: worst error / bound "
                      f"{float((err / bound).max()):.3f}, max error {float(err.max()):.3e}")
                assert (err <= bound).all()


@pytest.mark.parametrize("per", [140, 16384])
def test_the_factor_where_the_mean_is_large_against_the_spread(per):
    """Values 8 + randn / 16, g = 7.5: the mean is 128 standard deviations from 0.  Per sample the ratio r_b must be within
    64 u of the float64 one (tests/test_guidance_rescale.py: fp32 two-pass arithmetic alone stays inside this, a one-pass sum
    of squares does not).  The ratio is read off exactly: phi = 1, and one planted element per sample with e_u = e_c = 8, whose
    combine is 8 whatever the rounding, so its output is 8 r_b^ to the bit."""
    B = 3
    e = 8.0 + torch.randn(2, B, per, generator=torch.Generator().manual_seed(per)) / 16
    e[:, :, 5] = 8.0
    for segs, row in ((2, None), (3, 2), (3, 0)):
        full = e if segs == 2 else torch.cat([e, e[1:2]])                # (e_p = e_c: the PAG term is s * 0)
        got = _launch(full, 7.5, 1.0, row).numpy().astype(np.float64)
        r_hat = got[:, 5] / 8.0
        r64 = GC.ratio_f64(full.numpy().astype(np.float64), segs, 7.5, TABLE[row] if segs == 3 else 0.0)[:, 0]
        err = np.abs(r_hat - r64) / r64 / U
        print(f"[cfg_rescale] per={per} segs={segs}: ratio error per sample, in u: {[round(float(v), 2) for v in err]} (gate 64)")
        assert (err <= 64.0).all()


# ------------------------------------------------------------------------------------------------ the live cell
def test_phi_is_read_from_the_cell_at_launch():
    B, per = 2, 4 * 8 * 8
    e = (torch.randn(2, B, per, generator=torch.Generator().manual_seed(1)) * 2).to(DEV)
    cell = torch.zeros(1, dtype=torch.float32, device=DEV)
    outs = []
    for phi in (0.3, 0.9):
        d = e.clone()
        cell.fill_(phi)
        ops.cfg_rescale(d, 7.5, cell)
        torch.cuda.synchronize()
        got = d[0].cpu().numpy().astype(np.float64)
        e64 = e.cpu().numpy().astype(np.float64)
        phi32 = np.float64(np.float32(phi))
        want = GC.rescale_f64(e64, 2, 7.5, 0.0, phi32)
        assert (np.abs(got - want) <= _bound(e64, 2, 7.5, 0.0, phi32, vec=True)).all(), phi
        assert torch.equal(d[1], e[1])
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1])
