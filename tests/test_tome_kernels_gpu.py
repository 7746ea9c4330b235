"""-m gpu: the four token-merging kernels (csrc/tome.hip) against the float64 restatement of tests/tome_cases.py.

Exact probes.  Rows are one-hot or four-hot (four equal entries) times a power of two, so every norm is a power of two and every
cosine is one of 0, 1/4, 1/2, 1 -- exact in fp32 and in float64 (two-hot rows would give 1 / sqrt 2, which is not; the point of
the probe is exact representability).  Only a few channels are used, so most maxima and most scores are exact ties: the best
destination, the selected set, pos and the lists must equal the reference's, which pins both lower-index rules.

Random inputs.  DELTA bounds |kernel score - exact cosine| * 2 for rows of C entries (u = 2^-24, first order in u):
  * the MFMA dot product is an fp32 fma chain over C terms, one rounding each: |err| <= C u sum|a_i b_i| <= C u |a| |b|;
  * a sum of squares carries <= (C/8 + 10) u relative error (8-term fma chains, 8 chains joined by 3 additions, C/64 chunks --
    bounded here by C u), the square root halves it and adds u, the reciprocal adds u: an inverse norm is off by <= (C/2 + 2) u;
  * two multiplications by the inverse norms add 2 u.
  On normalised rows (|a| |b| dinv sinv = 1, |cos| <= 1) a score is therefore off by <= (C + 2 (C/2 + 2) + 2) u = (2 C + 6) u, and
  the difference of two scores by twice that:  DELTA(C) = 2 (2 C + 6) 2^-24  (7.7e-5 at C = 320).
A kernel decision that differs from the reference's is accepted only if the reference's cosine of the kernel's choice is within
DELTA of the reference maximum (selection: only if the r-th and (r+1)-th reference scores are within DELTA).  The inputs are
chosen (tome_cases.twin_tokens, the first seed that qualifies) so that the REFERENCE has no decision within DELTA, and the test
asserts that before it looks at the GPU -- so in effect the decisions must be equal.

Every output lives in a sentinel-filled buffer with padding rows / columns that must come back untouched.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tome_cases as TC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
RATIOS = (0.25, 0.5, 0.75, 0.9)
S32, S16 = 0x5A5A5A5A, 0x5A5A


def DELTA(C):
    return 2 * (2 * C + 6) * 2.0 ** -24


def _guard(shape, dtype):
    """A sentinel-filled buffer with 8 extra rows and 8 extra columns; -> (full int view, the [shape] window in `dtype`)."""
    rows, cols = shape
    if dtype in (torch.int32, torch.float32):
        full = torch.full((rows + 8, cols + 8), S32, dtype=torch.int32, device=DEV)
    else:
        full = torch.full((rows + 8, cols + 8), S16, dtype=torch.int16, device=DEV)
    return full, full.view(dtype)[:rows, :cols]


def _guard_flat(shape, dtype):
    """A dense [shape] array of 4-byte elements with 8 sentinel words in front and 8 behind; -> (full, the window)."""
    n = shape[0] * shape[1]
    full = torch.full((n + 16,), S32, dtype=torch.int32, device=DEV)
    return full, full[8:8 + n].view(dtype).view(shape)


def _intact(full, shape, what):
    rows, cols = shape
    s = S32 if full.dtype == torch.int32 else S16
    chk = full.clone()
    chk[:rows, :cols] = s
    assert bool((chk == s).all()), f"{what}: bytes outside the output were written"


def _windows(h, w, seed, sx=2, sy=2):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(sx * sy, ((h // sy) * (w // sx),), generator=g).to(torch.uint8)


def _run_match_select(x16, B, h, w, win, r, ld_pad=0):
    """x16 [B, N, C] 16-bit on the CPU -> the kernels' (best, score, pos, rowtok, seg, lst) on the CPU; sentinels checked."""
    N, C = h * w, x16.shape[-1]
    nd = TC.window_count(h, w, 2, 2)
    xd = torch.zeros(B * N, C + ld_pad, dtype=x16.dtype, device=DEV)
    if ld_pad:
        xd[:, C:] = float("nan")                  # the gap of a padded leading dimension is never read
    xd[:, :C] = x16.reshape(B * N, C).to(DEV)
    # row 1 of a three-row table, selected through the device word; rows 0 and 2 hold another pattern
    table = torch.stack([(win + 1) % 4, win, (win + 2) % 4]).to(DEV)
    row = torch.tensor([1], dtype=torch.int32, device=DEV)
    (fb, best), (fs, score) = _guard_flat((B, N), torch.int32), _guard_flat((B, N), torch.float32)
    ops.tome_match(xd[:, :C], B, h, w, table, row_idx=row, best=best, score=score)
    guards = [_guard_flat((B, m), torch.int32) for m in (N, N - r, nd + 1, max(r, 1))]
    outs = [g_[1] for g_ in guards]
    ops.tome_select(best, score, nd, r, out=tuple(outs))
    torch.cuda.synchronize()
    for (full, win_), what in zip([(fb, best), (fs, score)] + guards, ("best_dst", "score", "pos", "rowtok", "seg", "lst")):
        assert bool((full[:8] == S32).all()) and bool((full[8 + win_.numel():] == S32).all()), f"{what}: written out of bounds"
    return [t.cpu() for t in (best, score, outs[0], outs[1], outs[2], outs[3])]


def _check_against(dec, got, r, what):
    best, score, pos, rowtok, seg, lst = got
    assert torch.equal(best.to(torch.int64), dec["best"]), (what, "best destination")
    assert torch.equal(pos.to(torch.int64), dec["pos"]), (what, "pos")
    assert torch.equal(rowtok.to(torch.int64), dec["rowtok"]), (what, "rowtok")
    flat = [t for l_ in dec["lists"] for t in l_]
    assert lst[:r].tolist() == flat, (what, "lists")
    bounds = [0]
    for l_ in dec["lists"]:
        bounds.append(bounds[-1] + len(l_))
    assert seg.tolist() == bounds, (what, "list bounds")


def _probe_rows(B, h, w, C, seed):
    """One-hot and four-hot rows times powers of two on a handful of channels: cosines in {0, 1/4, 1/2, 1}, mostly tied."""
    g = torch.Generator().manual_seed(seed)
    N = h * w
    x = torch.zeros(B, N, C, dtype=torch.float64)
    base = [0, 3, C - 4, C // 2]                                    # four-hot blocks start here (one reaches the last column)
    for b in range(B):
        for t in range(N):
            kind, where, k = torch.randint(0, 2, (1,), generator=g).item(), torch.randint(0, 4, (1,), generator=g).item(), \
                torch.randint(-2, 3, (1,), generator=g).item()
            if kind == 0:
                x[b, t, base[where] + torch.randint(0, 4, (1,), generator=g).item()] = 2.0 ** k
            else:
                x[b, t, base[where]:base[where] + 4] = 2.0 ** k
    return x


@pytest.mark.parametrize("dtype,fmt", DTYPES)
@pytest.mark.parametrize("h,w", [(8, 8), (5, 7), (32, 32)])
def test_exact_probes_pin_the_decisions_and_both_tie_rules(h, w, dtype, fmt):
    B, C = 2, 320
    x = _probe_rows(B, h, w, C, seed=h * 100 + w)
    x16 = x.to(dtype)
    assert torch.equal(x16.to(torch.float64), x)
    win = _windows(h, w, 7)
    nd = TC.window_count(h, w, 2, 2)
    ties = 0
    for ratio in (0.5, 0.9):
        r = TC.merged_count(h * w, ratio, nd)
        got = _run_match_select(x16, B, h, w, win, r)
        for b in range(B):
            dec = TC.decide(x[b], h, w, 2, 2, win, r)
            ties += int((dec["best_margin"][dec["src"]] == 0).sum()) + int(dec["sel_margin"] == 0)
            _check_against(dec, [t[b] for t in got], r, (fmt, h, w, ratio, b))
            assert torch.equal(got[1][b].to(torch.float64), dec["score"]), "the cosines of the probe are exact in fp32"
    assert ties > 0, "the probe holds no exact tie"


_REF = {}


def _random_case(h, w, C, dtype):
    """(x16, win, {ratio: [decisions per item]}) of the first seed whose reference has no decision within DELTA; cached."""
    key = (h, w, C, dtype)
    if key not in _REF:
        nd, B = TC.window_count(h, w, 2, 2), 2
        for seed in range(16):
            win = _windows(h, w, seed)
            x16 = TC.twin_tokens(B, h, w, C, win, seed).to(dtype)
            decs = {ratio: [TC.decide(x16[b], h, w, 2, 2, win, TC.merged_count(h * w, ratio, nd)) for b in range(B)]
                    for ratio in RATIOS}
            worst = min(min(float(d["best_margin"][d["src"]].min()), d["sel_margin"]) for v in decs.values() for d in v)
            if worst >= DELTA(C):
                _REF[key] = (x16, win, decs, worst)
                break
    # the precondition: the reference itself is unambiguous at DELTA
    assert key in _REF, "no seed in range(16) gives a reference without a decision inside DELTA"
    return _REF[key]


def _accept(dec, got, r, C, what):
    """The decision rule of the module docstring (with the precondition it reduces to equality; kept as stated)."""
    best = got[0].to(torch.int64)
    diff = (best != dec["best"]).nonzero().flatten().tolist()
    if diff:
        alt = TC.decide(dec["x"], *dec["geom"], dec["win"], r, best_override=best)
        for t in diff:
            assert float(dec["score"][t] - alt["score"][t]) <= DELTA(C), (what, "best destination of token", t)
    merged_gpu = torch.zeros_like(dec["merged"])
    merged_gpu[got[5][:r].to(torch.int64)] = True
    if not torch.equal(merged_gpu, dec["merged"]):
        assert dec["sel_margin"] <= DELTA(C), (what, "selected set")
    if not diff and torch.equal(merged_gpu, dec["merged"]):
        _check_against(dec, got, r, what)
        err = float((got[1].to(torch.float64) - dec["score"]).abs().max())
        print(f"[tome match] {what}: max |score - cosine| = {err:.3e}  (DELTA / 2 = {DELTA(C) / 2:.3e})")
        assert err <= DELTA(C) / 2, (what, "score")


@pytest.mark.parametrize("dtype,fmt", DTYPES)
@pytest.mark.parametrize("h,w,C,ld_pad", [(8, 8, 320, 0), (6, 10, 320, 8), (5, 7, 320, 0), (32, 32, 320, 0), (4, 4, 640, 0)])
def test_random_inputs_decide_as_float64(h, w, C, ld_pad, dtype, fmt):
    """C = 640 at 4 x 4: the second level of a 8 x 8 latent (max_downsample = 2).  32 x 32: four destination tiles, eight token
    tiles."""
    x16, win, decs, worst = _random_case(h, w, C, dtype)
    assert worst >= DELTA(C)
    B, nd = 2, TC.window_count(h, w, 2, 2)
    for ratio in RATIOS:
        r = TC.merged_count(h * w, ratio, nd)
        if ratio == 0.75:
            assert r == h * w - nd or (h * w) % 4, "ratio 0.75 merges every source of an even grid"
        if ratio == 0.9:
            assert r == h * w - nd, "ratio 0.9 is capped at the number of sources"
        got = _run_match_select(x16, B, h, w, win, r, ld_pad=ld_pad)
        for b in range(B):
            dec = dict(decs[ratio][b], x=x16[b], geom=(h, w, 2, 2), win=win)
            _accept(dec, [t[b] for t in got], r, C, (fmt, h, w, C, ratio, b))


@pytest.mark.parametrize("dtype,fmt", DTYPES)
@pytest.mark.parametrize("h,w,ratio", [(8, 8, 0.5), (5, 7, 0.25), (6, 10, 0.9), (32, 32, 0.5)])
def test_merge_and_unmerge_from_reference_decisions(h, w, ratio, dtype, fmt):
    """Merged rows within one rounding of the float64 mean (|err| <= ulp of the result in the output format), copies exact,
    V^T padding columns zero, unmerge exact, guards intact, two runs bitwise equal.  32 x 32 at 0.5: 512 merged rows."""
    B, C = 2, 320
    N, nd = h * w, TC.window_count(h, w, 2, 2)
    r = TC.merged_count(N, ratio, nd)
    nm, ldvt_in, ldvt_out = N - r, (N + 7) // 8 * 8 + 8, (N - r + 7) // 8 * 8
    x16, win, decs, _ = _random_case(h, w, C, dtype)
    g = torch.Generator().manual_seed(5)
    qk = torch.randn(B, N, 2 * C, generator=g).to(dtype)
    v = torch.randn(B, N, C, generator=g).to(dtype)
    qk_d = torch.full((B * N, 2 * C + 8), float("nan"), dtype=dtype, device=DEV)       # ld = 2C + 8: the gap is never read
    qk_d[:, :2 * C] = qk.reshape(B * N, 2 * C).to(DEV)
    vt_d = torch.full((B, C, ldvt_in), float("nan"), dtype=dtype, device=DEV)          # columns behind n are never read
    vt_d[:, :, :N] = v.transpose(1, 2).to(DEV)
    dec = [TC.decide(x16[b], h, w, 2, 2, win, r) for b in range(B)]
    rowtok = torch.stack([d["rowtok"] for d in dec]).to(torch.int32).to(DEV)
    pos = torch.stack([d["pos"] for d in dec]).to(torch.int32).to(DEV)
    seg = torch.zeros(B, nd + 1, dtype=torch.int32)
    lst = torch.zeros(B, max(r, 1), dtype=torch.int32)
    for b, d in enumerate(dec):
        flat = [t for l_ in d["lists"] for t in l_]
        lst[b, :r] = torch.tensor(flat, dtype=torch.int32)
        seg[b, 1:] = torch.tensor([len(l_) for l_ in d["lists"]]).cumsum(0).to(torch.int32)
    seg, lst = seg.to(DEV), lst.to(DEV)

    def run():
        fq, qo = _guard((B * nm, 2 * C), dtype)
        fv, vo = _guard((B * C, ldvt_out), dtype)
        ops.tome_merge(qk_d[:, :2 * C], vt_d, B, N, nd, r, rowtok, seg, lst, qk_out=qo,
                       vt_out=vo.unflatten(0, (B, C)))
        fu, uo = _guard((B * N, C), dtype)
        ops.tome_unmerge(qo[:, :C], pos, out=uo)
        torch.cuda.synchronize()
        _intact(fq, (B * nm, 2 * C), "merged Q|K")
        _intact(fv, (B * C, ldvt_out), "merged V^T")
        _intact(fu, (B * N, C), "unmerged rows")
        return qo.clone(), vo.clone().unflatten(0, (B, C)), uo.clone()

    qo, vo, uo = run()
    qo2, vo2, uo2 = run()
    assert torch.equal(qo.view(torch.int16), qo2.view(torch.int16)) and torch.equal(vo.view(torch.int16), vo2.view(torch.int16))
    assert torch.equal(uo.view(torch.int16), uo2.view(torch.int16))
    eps = torch.finfo(dtype).eps
    worst = 0.0
    for b, d in enumerate(dec):
        for name, got, rows in (("Q|K", qo[b * nm:(b + 1) * nm].cpu(), qk[b]), ("V^T", vo[b, :, :nm].T.cpu(), v[b])):
            ref = TC.merge_rows(rows, d)
            copied = torch.tensor([m < d["nkept"] or not d["lists"][m - d["nkept"]] for m in range(nm)])
            assert torch.equal(got[copied].to(torch.float64), ref[copied]), (name, "a copied row changed")
            err = (got.to(torch.float64) - ref).abs()
            ulp = torch.maximum(ref.abs(), torch.tensor(float(torch.finfo(dtype).tiny), dtype=torch.float64)) * eps
            worst = max(worst, float((err / ulp).max()))
            assert bool((err <= ulp).all()), (name, "merged row off by more than one rounding", float((err / ulp).max()))
        assert bool((vo[b, :, nm:] == 0).all()), "V^T padding columns must hold zeros"
        want = qo[b * nm:(b + 1) * nm, :C].cpu()[d["pos"]]
        assert torch.equal(uo[b * N:(b + 1) * N].cpu().view(torch.int16), want.view(torch.int16)), "unmerge is a row gather"
    print(f"[tome merge] {fmt} {h}x{w} ratio {ratio}: worst error {worst:.3f} ulp of the output format")


def test_refusals_by_return_code():
    lib = L.lib()
    assert lib.pp_tome_supported(64, 64, 320, 2, 2) == 1 and lib.pp_tome_supported(128, 128, 320, 2, 2) == 1
    assert lib.pp_tome_supported(1, 8, 320, 2, 2) == 0 and lib.pp_tome_supported(8, 8, 324, 2, 2) == 0
    assert lib.pp_tome_supported(256, 128, 320, 2, 2) == 0 and lib.pp_tome_supported(8, 8, 320, 32, 32) == 0
    x = torch.zeros(64, 320, dtype=torch.bfloat16, device=DEV)
    tb = torch.zeros(1, 16, dtype=torch.uint8, device=DEV)
    bo = torch.full((64,), S32, dtype=torch.int32, device=DEV)
    so = torch.full((64,), S32, dtype=torch.int32, device=DEV)
    f = lib.pp_tome_match
    args = lambda **k: [k.get("x", x.data_ptr()), k.get("ld", 320), 1, k.get("h", 8), 8, k.get("C", 320), 2, 2, tb.data_ptr(),  # noqa: E731
                        k.get("stride", 16), 1, None, bo.data_ptr(), so.data_ptr(), k.get("dt", L.PP_DT_BF16), None]
    assert f(*args(x=None)) == -1 and f(*args(ld=316)) == -1 and f(*args(stride=8)) == -1 and f(*args(dt=0)) == -1
    assert f(*args(h=1)) == -2 and f(*args(C=324, ld=328)) == -2
    assert lib.pp_tome_select(bo.data_ptr(), so.data_ptr(), 1, 64, 16, 49, bo.data_ptr(), bo.data_ptr(), bo.data_ptr(),
                              bo.data_ptr(), None) == -1                       # r above the number of sources
    torch.cuda.synchronize()
    assert bool((bo == S32).all()) and bool((so == S32).all()), "a refused call wrote"
