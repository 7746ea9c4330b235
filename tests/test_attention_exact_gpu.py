"""-m gpu: every shipping attention kernel under the three probes of tests/attention_cases.py (derivations of the gates: that
module's docstring; proof that the probes notice a wrong kernel: tests/test_attention_probes.py), at the smallest shapes at
which each of its paths exists.

The only gates:  P1 |out - v| <= 2 u |v|;  P2 |out - ref| <= 3 u ref;  P3 |out - ref| <= u (A + 2 |ref|) + 1e-5 A
(+ 2^-25 sum_j |V_j| in fp16), for pp_attention_small u |ref| + 1e-5 A.

Buffers are never tight: q and k are column slices of one fused [M, 2C + 8] buffer, k has 64 poisoned rows behind the last
batch item, vt has ldvt = round8(nk) + 8 with poisoned pad columns, o has ldo = C + 8 and 8 extra rows and is pre-filled with
a sentinel bit pattern: after every launch every element outside [batch*nq, C] is bit-for-bit unchanged and the output
is finite.  Where the dispatch rule of pp_attention_fwd names the kernel under test, PP_ATTN_AUTO gives the same bits.

The worst error / gate per (kernel, format, probe) is printed, and appended to profiles/attention_exact_achieved.txt when
the module ends (one line per key; every case has entered its figure before it asserts).
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attention_cases as AC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
SENTINEL = 0x5A5A
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    yield
    try:
        with open(os.path.join(ROOT, "profiles", "attention_exact_achieved.txt"), "a") as f:
            for (kernel, fmt, probe), (r, where) in sorted(WORST.items()):
                f.write(f"[attention exact] {kernel} {fmt} {probe}: worst error / gate {r:.3f} at {where}\n")
    except OSError:
        pass


def _note(kernel, fmt, probe, ratio, where):
    print(f"[attention exact] {kernel} {fmt} {probe} {where}: error / gate {ratio:.3f}")
    if ratio >= WORST.get((kernel, fmt, probe), (-1.0, None))[0]:
        WORST[(kernel, fmt, probe)] = (ratio, where)


def _guarded(s: AC.Setup, launch_into):
    """Run one launch into a sentinel-filled, padded output; -> the [B*nq, C] result (a copy)."""
    rows, C = s.B * s.nq, s.C
    full = torch.full((rows + 8, C + 8), SENTINEL, dtype=torch.int16, device=DEV)
    launch_into(full.view(s.dtype)[:rows, :C])
    torch.cuda.synchronize()
    out = full.view(s.dtype)[:rows, :C].clone()
    full[:rows, :C] = SENTINEL
    assert bool((full == SENTINEL).all()), ("bytes outside the output rows / columns were written", s.probe, s.nq, s.nk, s.d)
    assert bool(torch.isfinite(out.float()).all()), ("non-finite output", s.probe, s.nq, s.nk, s.d)
    return out


def _vt(s: AC.Setup):
    return AC.poison_vt(ops.transpose_v(s.v, s.B, s.nk, ldvt=s.ldvt), s.nk)


def _run_attention(kernel, variant, B, H, nq, nk, d, probes, log2=False, auto_is=None):
    """All probes x both formats on pp_attention_fwd_variant(variant).  auto_is: the variant the dispatch rule names for this
    shape -- PP_ATTN_AUTO must then give the bits of that kernel."""
    failures = []
    for dtype, fmt in DTYPES:
        for probe in probes:
            s = AC.BUILDERS[probe](B, H, nq, nk, d, dtype, log2=log2, device=DEV)
            vt, k = _vt(s), s.k_view()
            worst = 0.0
            for launch in range(len(s.q)):
                q = s.q_view(launch)

                def go(o, v_=variant):
                    ops.attention(q, k, vt, B, H, nq, nk, d, scale=s.scale, variant=v_, out=o)

                out = _guarded(s, go)
                worst = max(worst, AC.worst_ratio(out, s.expected[launch], s.gate[launch]))
                if auto_is is not None:
                    named = out if auto_is == variant else _guarded(s, lambda o: go(o, auto_is))
                    auto = _guarded(s, lambda o: go(o, L.PP_ATTN_AUTO))
                    assert torch.equal(auto.view(torch.int16), named.view(torch.int16)), \
                        ("PP_ATTN_AUTO differs from the kernel the dispatch rule names", auto_is, probe, fmt, nq, nk, d)
            _note(kernel, fmt, probe, worst, f"d={d} nq={nq} nk={nk}")
            if not worst <= 1.0:
                failures.append((kernel, fmt, probe, worst))
    assert not failures, failures


def _probes(nk):
    return ("P1", "P2", "P3") if nk <= 129 else ("P1", "P3")


# ------------------------------------------------------------------------------------------------ attn_fwd_kernel
@pytest.mark.parametrize("nq", AC.PHASED_NQ)
@pytest.mark.parametrize("nk", AC.PHASED_NK)
@pytest.mark.parametrize("d", AC.PHASED_D)
def test_phased_kernel(d, nk, nq):
    """PP_ATTN_PHASED.  nk: below one 16-key block (4, 13), the <= 32-live-keys tail at both edges (32 | 33, 96 | 97), the
    masked full tail (33, 65, 77 is the 13-key tail, 97, 129), exactly one, two and three tiles with and without a tail.
    nq: below one wave's 32 rows, one row into the second wave, two rows into the second 128-row workgroup.
    AUTO takes this kernel for all of them (nk < 256 or nk % 64 != 0, or d != 40)."""
    _run_attention(f"phased_d{d}", L.PP_ATTN_PHASED, AC.B_, AC.H_, nq, nk, d, _probes(nk), auto_is=L.PP_ATTN_PHASED)


@pytest.mark.parametrize("nq,nk", AC.QR_CASES)
def test_phased_kernel_kv_reuse_form(nq, nk):
    """attn_fwd_kernel<40, EDT, QR = true>: launch_attn takes it when `D == 40 && nk <= 2 * KB && wgs >= 2048` with
    wgs = ceil(nq / 128) * heads * batch.  batch = heads = 8: nq = 4096 -> 32 * 64 = 2048 workgroups' worth, every second
    block whole; 3996 -> 32 blocks, the last second block ragged (28 rows); 4224 -> 33 blocks = 2112, an odd count: the last
    workgroup's second block lies wholly past nq."""
    assert (nq + 127) // 128 * AC.QR_H * AC.QR_B >= 2048 and nk <= 128
    _run_attention("phased_d40_kv_reuse", L.PP_ATTN_PHASED, AC.QR_B, AC.QR_H, nq, nk, 40, ("P1", "P3"),
                   auto_is=L.PP_ATTN_PHASED)


# ------------------------------------------------------------------------------------------------ attn_pipe_kernel
@pytest.mark.parametrize("nq,nk", AC.PIPE_CASES)
@pytest.mark.parametrize("name", ["PIPE_Q32", "PIPE_Q64", "PIPE_LOG2"])
def test_pipelined_kernels(name, nq, nk):
    """Tile counts 4 .. 12 at nq = 200: every residue of the ring depths 3, 4 and 5 in prologue and drain; at nk = 256 also
    nq = 33 and 257 (one row into the second wave and into the second workgroup of both forms).  AUTO is PIPE_Q32 here:
    batch * heads * ceil(nq / 256) = 6 or 12 < 512.  LOG2 (the 32-queries form at these shapes) gets q' = Q * scale * log2 e
    rounded once and the reference softmax over exp2(q' . k)."""
    B, H = AC.B_, AC.H_
    assert nk % 64 == 0 and nk >= 256 and B * H * ((nq + 255) // 256) < 512
    log2 = name == "PIPE_LOG2"
    if log2:
        assert L.lib().pp_attention_log2_ok(nq, nk, 40) == 1
    _run_attention(name.lower(), getattr(L, "PP_ATTN_" + name), B, H, nq, nk, 40, _probes(nk), log2=log2,
                   auto_is=None if log2 else L.PP_ATTN_PIPE_Q32)


# ------------------------------------------------------------------------------------------------ attn_small_kernel
def _run_small(nq, nk, causal):
    B, H, d = AC.B_, AC.H_, AC.SMALL_D
    C = H * d
    kernel = "small_causal" if causal else "small"
    failures = []
    for dtype, fmt in DTYPES:
        for probe in _probes(nk):
            kw = dict(p_fp32=True) if probe == "P3" else {}
            s = AC.BUILDERS[probe](B, H, nq, nk, d, dtype, causal=causal, device=DEV, **kw)
            M = s.fused.shape[0]
            worst = 0.0
            for launch in range(len(s.q)):
                s.q_view(launch)
                qkv = torch.full((M, 3 * C + 8), AC.K_POISON, dtype=dtype, device=DEV)     # one fused q | k | v buffer
                qkv[:, :2 * C] = s.fused[:, :2 * C]
                qkv[:B * nk, 2 * C:3 * C] = s.v
                q, k, v = qkv[:B * nq, :C], qkv[:B * nk, C:2 * C], qkv[:B * nk, 2 * C:3 * C]
                out = _guarded(s, lambda o: ops.attention_small(q, k, v, B, H, nq, nk, causal=causal, scale=s.scale, out=o))
                worst = max(worst, AC.worst_ratio(out, s.expected[launch], s.gate[launch]))
            _note(kernel, fmt, probe, worst, f"nq={nq} nk={nk}")
            if not worst <= 1.0:
                failures.append((kernel, fmt, probe, worst))
    assert not failures, failures


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("n", AC.SMALL_N)
def test_small_kernel(n, causal):
    """pp_attention_small, d = 64: one key, a few, around the 64-key lane block (63 | 64 | 65), CLIP's 77, around its limit
    of 128.  Causal P1 targets pi(i) <= i (the diagonal: the last visible key; then a walk inside the visible ones)."""
    _run_small(n, n, causal)


@pytest.mark.parametrize("nq,nk", AC.SMALL_RECT)
def test_small_kernel_nq_differs_from_nk(nq, nk):
    _run_small(nq, nk, False)
