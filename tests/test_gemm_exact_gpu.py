"""-m gpu: the GEMM / implicit-GEMM conv kernels (csrc/gemm.hip, the halo-tile loop of csrc/conv_gn.hip, the split-K combines)
through the C ABI on the matrix of tests/gemm_cases.py, in bf16 and fp16.  Derivations: that module's docstring; proof that
every probe can fail: tests/test_gemm_probes.py.

  E / T cases   the output -- and the fp32 output, the V^T store, out_dup_rows, res1_wrap_rows, the row moments and the int64
                GroupNorm accumulators where the case has them -- EQUALS the fp64 reference cast once, bit for bit;
  R cases       |out - ref| <= u |ref| + n_r 2^-24 A (the derived gate, nothing fitted);
  every case    outputs are windows of sentinel-filled buffers (64 rows in front and behind, 8 pad columns, a sentinel tail
                behind the split-K workspace): every byte outside a window is unchanged after the launch; operands carry
                poisoned pads, rows and tails; a split-K or in-kernel-combine case is launched twice and must repeat itself
                bit for bit, with its tile counters re-armed and no combine fault;
  refusals      a combination the library refuses is refused before any launch, with the error code the case states.

References are computed in fp64 on the device.  A failure names the case, the first bad index and the tile / slice / image
borders it lies on.  The worst achieved / gate per (kernel family, format, regime) is printed and, after a whole run of the
file, written to profiles/gemm_exact_achieved.txt with the case count and the file's wall time; no threshold is pinned on it.
"""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gemm_cases as GC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
GN_SIDES = ("gn", "gnnext")
WS_TAIL = 4096               # fp32 sentinel words behind the split-K workspace
WORST, COUNT, T0 = {}, {}, [None]
ACHIEVED_HEADER = ("# tests/test_gemm_exact_gpu.py on one MI355X: per (kernel family, format, regime) the largest achieved error / gate\n"
                   "# of the R cases (gate: u |ref| + (K + splits + 5) 2^-24 A, tests/gemm_cases.py; worst case, not fitted: the ratio\n"
                   "# shows the slack, no threshold is pinned on it; folded-LayerNorm and softmax cases: the terms of tests/norm_cases.py)\n"
                   "# and the number of E / T cases that held bit equality.  A family is named after the tile id the case REQUESTS (the\n"
                   "# library has no query for the form it ran; the split count is checked against its workspace size).  The wall time\n"
                   "# is rounded to 5 s, at least 5 s, so that this tracked file is the same after every run.\n")


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    """After a WHOLE run of the file profiles/gemm_exact_achieved.txt is rewritten (the figures are deterministic; the wall
    time is rounded to 5 s)."""
    T0[0] = time.time()
    yield
    if sum(COUNT.values()) != sum(len(GC.case_dtypes(c)) for c in GC.CASES if not c.expect):
        return
    try:
        with open(os.path.join(ROOT, "profiles", "gemm_exact_achieved.txt"), "w") as f:
            f.write(ACHIEVED_HEADER)
            for key in sorted(COUNT):
                fam, fmt, regime = key
                line = f"[gemm exact] {fam} {fmt} {regime}: {COUNT[key]} cases"
                if key in WORST:
                    line += f", worst error / gate {WORST[key][0]:.3f} at {WORST[key][1]}"
                else:
                    line += ", bit-equal"
                f.write(line + "\n")
            wall = max(5, 5 * round((time.time() - T0[0]) / 5))          # (to 5 s: the tracked file stays as committed)
            f.write(f"# {len(GC.CASES)} cases of the matrix, {sum(COUNT.values())} (case, format) runs checked; wall time of the "
                    f"file about {wall} s\n")
    except OSError:
        pass


def _family(c):
    fam, bm, sk, pp = GC.launch_form(c)
    if fam == "halo":
        return "halo-subpix" if c.kind == "subpix" else "halo"
    name = {"v1": "v1", "v2": "v2-pingpong" if pp else "v2-lockstep"}[fam] if c.tile else "auto"
    return ("conv-" if c.kind == "conv" else "") + name + ("-splitk" if sk > 1 else "")


def _nhwc(b, B, H, W):
    return b.full.as_strided((B, H, W, b.cols), (H * W * b.ld, W * b.ld, b.ld, 1), b.base)


def _where(c, idx):
    """the borders a failing element (row, column) lies on"""
    m, n = int(idx[0]), int(idx[1])
    fam, bm, sk, _ = GC.launch_form(c)
    tags = [f"tile ({m // bm}, {n // 160})"]
    if m % bm in (0, bm - 1) or n % 160 in (0, 159):
        tags.append("on a tile border")
    if m % 64 in (0, 63):
        tags.append("on a 64-row pass border")
    if c.kind != "plain":
        ho, wo = c.hw_out
        rem = m % (ho * wo)
        if rem // wo in (0, ho - 1) or rem % wo in (0, wo - 1):
            tags.append("on an image border")
    if sk > 1:
        tags.append(f"{sk} K slices starting {GC.slice_start_kinds(c) or 'at K tiles of x'}")
    return ", ".join(tags)


def _launch(c, t, o, dtype, ctr=None):
    """one call of the library for case `c` on the operands `t` into the windows `o`"""
    view = lambda k: t[k].view if t.get(k) is not None else None      # noqa: E731
    act = (L.PP_ACT_SILU if "silu" in c.epi else L.PP_ACT_GEGLU if "geglu" in c.epi else
           L.PP_ACT_SOFTMAX80 if "softmax" in c.epi else L.PP_ACT_NONE)
    ln = dict(ln_stats=t["ln_stats"], ln_colsum=t["ln_colsum"][:c.N], ln_dim=c.K, ln_eps=GC.LN_EPS) if "ln" in c.epi else {}
    fuse = (ctr if ctr is not None else "force") if c.side == "fuse" else False
    gn = [(a, cg, c0, g) for a, (cg, c0, g) in zip(o["gn"], GC.gn_subs(c))] if c.side in GN_SIDES else None
    kw = dict(scale=c.scale, tile=c.tile, splitk=c.splitk, gn=gn, fuse_combine=fuse, workspace=o["ws"])
    N = c.N
    if c.kind == "plain":
        ops.gemm(view("x1"), t["w"][:N], t["bias"][:N] if t["bias"] is not None else None, x2=view("x2"), res1=view("res1"),
                 res2=view("res2"), act=act, rowvec=t["rowvec"], rows_per_batch=c.rows_per_batch, out_f32=c.side == "f32",
                 vt_col0=160 if c.side == "vt" else 0, row_stats=c.side == "stats", res1_wrap=t["wrap"], out=o["out"].view,
                 vt=o["vt"].view.view(t["nb"], N - 160, -1) if c.side == "vt" else None,
                 stats=o["stats"].view.view(c.rows, -1, 2) if c.side == "stats" else None, **ln, **kw)
        return
    B, H, W = c.B, c.H, c.W
    ho, wo = c.hw_out
    k = 2 if c.kind == "subpix" else 1
    nh = lambda name, h, w_: _nhwc(t[name], B, h, w_) if t.get(name) is not None else None     # noqa: E731
    common = dict(bias=t["bias"][:N] if t["bias"] is not None else None, rowvec=t["rowvec"], res1=nh("res1", k * ho, k * wo),
                  res2=nh("res2", k * ho, k * wo), out=_nhwc(o["out"], B * (2 if c.side == "dup" else 1), k * ho, k * wo))
    if c.kind == "subpix":
        kw.pop("fuse_combine")
        ops.conv3x3_up_subpix(nh("x1", H, W), t["w"][:4 * N].view(4, N, -1), **common, **kw)
    else:
        ops.conv3x3(nh("x1", H, W), t["w"][:N], stride=c.stride, up=c.up, x2=nh("x2", H, W), x3=nh("x3", ho, wo),
                    x4=nh("x4", ho, wo), res1_wrap=t["wrap"], dup=c.side == "dup", **common, **kw,
                    **(dict(gn_next=(t["gamma"], t["beta"], 1e-5, True, 0), ynext=o["ynext"].view.view(B, ho, wo, N))
                       if c.side == "gnnext" else {}))


def _windows(c, t, dtype):
    M, N = c.rows, c.N
    n_out = N // 2 if "geglu" in c.epi else (160 if c.side == "vt" else N)
    orows = M * (4 if c.kind == "subpix" else 1) * (2 if c.side == "dup" else 1)
    pad = 4 if c.side == "ld4" else 0 if c.side == "gnnext" else GC.PAD_COLS     # (gn_next_* needs ldo == N)
    o = {"out": GC.sentinel_out(orows, n_out, pad, torch.float32 if c.side == "f32" else dtype).to(DEV)}
    if c.side == "vt":
        o["vt"] = GC.sentinel_out(t["nb"] * (N - 160), c.rows_per_batch, GC.PAD_COLS, dtype).to(DEV)
    if c.side == "stats":
        o["stats"] = GC.sentinel_out(M, (N + 159) // 160 * 2, 0, torch.float32).to(DEV)
    if c.side == "gnnext":                             # dense by the ABI: guard rows only, as for the row moments
        o["ynext"] = GC.sentinel_out(orows, N, 0, dtype).to(DEV)
        g = GC._gen(5, N)
        t["gamma"], t["beta"] = (torch.randn(N, generator=g) * 0.3 + 1.0).to(DEV), (torch.randn(N, generator=g) * 0.2).to(DEV)
    if c.side in GN_SIDES:
        o["gn"] = [torch.zeros(t["nb"], g, 2, dtype=torch.int64, device=DEV) for _, _, g in GC.gn_subs(c)]
    # the workspace: 8 slabs + the in-kernel combine's scratch always suffice; everything behind what the library asks for
    # is sentinel and must stay so
    words = 8 * M * N + ((M + 63) // 64) * ((N + 159) // 160) * 6144 // 4 + WS_TAIL
    o["ws"] = torch.full((words,), GC.SENTINEL32, dtype=torch.int32, device=DEV).view(torch.float32)
    return o


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _check_outside(c, o, what):
    for name in ("out", "vt", "stats", "ynext"):
        if name in o:
            b = o[name]
            s = GC.SENTINEL32 if b.full.dtype == torch.float32 else GC.SENTINEL16
            assert bool((_bits(b.full)[b.outside()] == s).all()), (what, name, "bytes outside the window were written")
    used = (ops.last_workspace["bytes"] + 3) // 4
    assert bool((o["ws"].view(torch.int32)[used:] == GC.SENTINEL32).all()), (what, "the workspace's sentinel tail was written")


def _run(c, dtype, fmt, tamper=None, after=None, record=True):
    """tamper(t) / after(o): hooks of the negative controls below (a reference or a buffer made wrong on purpose)"""
    what = f"{c.id} {fmt}"
    t = GC.build(c, dtype, DEV)
    if tamper:
        tamper(t)
    o = _windows(c, t, dtype)
    if c.expect:
        with pytest.raises(L.PPError, match=L.PP_ERR[c.expect]):
            _launch(c, t, o, dtype)
        torch.cuda.synchronize()
        _check_outside(c, o, what)                     # refused before any launch: nothing was written at all
        assert bool((_bits(o["out"].view) == GC.SENTINEL16).all()), (what, "a refused request wrote to `out`")
        return
    if c.kind != "plain":                              # the case reaches the form it means to reach
        ho, wo = c.hw_out
        nh = lambda n_, h, w_: _nhwc(t[n_], c.B, h, w_) if n_ in t else None      # noqa: E731
        routed = ops.conv_halo_routed(nh("x1", c.H, c.W), c.N, x2=nh("x2", c.H, c.W), x3=nh("x3", ho, wo), x4=nh("x4", ho, wo),
                                      stride=c.stride, up=c.up, tile=c.tile) if c.kind == "conv" else \
            ops.upconv_subpix_supported(_nhwc(t["x1"], c.B, c.H, c.W), c.N) >= 1
        assert bool(routed) == c.halo, (what, "routing changed: halo-tile loop", routed)
    if c.kind == "subpix":                             # pp_upconv_fold itself: bit-exact on integer weights
        wf = ops.upconv_fold(t["w9"].contiguous())
        assert bool((wf.view(4 * c.N, -1) == t["w"][:4 * c.N]).all()), (what, "pp_upconv_fold")
    _launch(c, t, o, dtype)
    torch.cuda.synchronize()
    if after:
        after(o)
    fam, bm, sk, _ = GC.launch_form(c)
    if c.side == "fuse":
        assert ops.last_combine["fused"], (what, "the launch did not combine in-kernel")
    # the split the case means to reach, from what the library itself sized (slabs of M x N floats + < one slab of scratch);
    # the rows of a tile have no query: a change of BM shows only in the bit equality of the probes
    if c.splitk > 0 or fam == "halo":
        sk_lib = max(1, ops.last_workspace["bytes"] // (c.rows * c.N * 4))
        assert sk_lib == sk, (what, "routing changed: the library runs", sk_lib, "K splits, the case means", sk)
    got = {k: o[k].view.clone() for k in ("out", "vt", "stats", "ynext") if k in o}
    gn_got = [a.clone() for a in o["gn"]] if c.side in GN_SIDES else None
    _check_outside(c, o, what)
    if sk > 1:                                         # a second, identical launch repeats the first bit for bit
        ctr = ops.last_combine["ctr"] if c.side == "fuse" else None
        for a in o.get("gn", []):
            a.zero_()
        _launch(c, t, o, dtype, ctr=ctr)
        torch.cuda.synchronize()
        for k in got:
            assert bool((_bits(o[k].view) == _bits(got[k])).all()), (what, k, "the second launch differs")
        if gn_got:
            assert all(bool((a == b).all()) for a, b in zip(o["gn"], gn_got)), (what, "gn_acc: the second launch differs")
        if c.side == "fuse":
            assert ops.last_combine["fused"] and int((ctr & ((1 << 40) - 1)).abs().sum()) == 0, (what, "tile counters not re-armed")
            assert ops.combine_faults(DEV) == 0, what
        _check_outside(c, o, what)
    # ---- values
    key = (_family(c), fmt, c.probe)
    if record:
        COUNT[key] = COUNT.get(key, 0) + 1
    if c.probe.startswith("R"):
        for name, (ref, g) in GC.gated_windows(c, t, dtype).items():
            assert bool(torch.isfinite(got[name].float()).all()), (what, name, "non-finite output")
            r = GC.worst_ratio(got[name], ref, g)
            print(f"[gemm exact] {key[0]} {fmt} {c.probe} {c.id} {name}: error / gate {r:.3f}")
            if record and r > WORST.get(key, (-1.0, None))[0]:
                WORST[key] = (r, c.id)
            if not r <= 1.0:
                bad = ((got[name].double() - ref).abs() > g).nonzero()
                raise AssertionError((what, name, "error / gate", r, "first bad index", bad[0].tolist(),
                                      _where(c, bad[0]) if name == "out" else ""))
        return
    if c.side == "gnnext":                             # bit for bit the apply launch on the raw output and its accumulators
        ho, wo = c.hw_out
        y = ops.groupnorm_apply_acc(got["out"].reshape(c.B, ho, wo, c.N).contiguous(), gn_got[0], t["gamma"], t["beta"], 1e-5, True)
        assert bool((_bits(y.reshape(-1, c.N)) == _bits(got["ynext"])).all()), (what, "gn_next output differs from the apply launch")
        assert bool(torch.isfinite(got["ynext"].float()).all()), (what, "gn_next output")
    for name, e in GC.expected_windows(c, t, dtype).items():
        ne = got[name].double() != e
        if bool(ne.any()):
            i = ne.nonzero()[0]
            where = _where(c, i) if name == "out" else ""
            raise AssertionError((what, name, "not bit-equal", int(ne.sum()), "elements; first bad index", i.tolist(),
                                  "got", float(got[name][tuple(i)]), "expected", float(e[tuple(i)]), where))
    sides = GC.expected_sides(c, t, dtype)
    if "stats" in sides:
        ne = got["stats"].view(c.rows, -1, 2) != sides["stats"].to(DEV)
        assert not bool(ne.any()), (what, "row_stats", ne.nonzero()[0].tolist())
    if "gn" in sides:
        for k, (a, b) in enumerate(zip(gn_got, sides["gn"])):
            ne = a != b.to(DEV)
            assert not bool(ne.any()), (what, f"gn_acc[{k}]", ne.nonzero()[0].tolist(), int(a[ne][0]), int(b.to(DEV)[ne][0]))


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_case(c):
    failures = []
    for dtype, fmt in GC.case_dtypes(c):
        try:
            _run(c, dtype, fmt)
        except (AssertionError, L.PPError) as e:       # both formats are run and reported; an unexpected refusal fails
            failures.append(e.args[0] if e.args else repr(e))
    assert not failures, failures


def test_the_checks_notice_what_they_are_for():
    """negative controls on the device: one expected value off by half a unit, one sentinel overwritten behind the last row,
    one in a pad column, one behind the workspace -- each must fail the case that passes untouched"""
    c = next(k for k in GC.CASES if k.id == "plain-E-M264-N160-K704-t54-sk3")
    dtype, fmt = GC.DTYPES[0]
    _run(c, dtype, fmt, record=False)

    def off_by_half(t):
        t["ref"][c.rows - 1, c.N - 1] += 0.5

    def behind(o):
        b = o["out"]
        b.full[b.base + b.rows * b.ld] = 1.0

    def pad(o):
        b = o["out"]
        b.full[b.base + b.cols] = 1.0

    def ws_tail(o):
        o["ws"][-1] = 1.0
    for kw, msg in ((dict(tamper=off_by_half), "not bit-equal"), (dict(after=behind), "outside the window"),
                    (dict(after=pad), "outside the window"), (dict(after=ws_tail), "sentinel tail")):
        with pytest.raises(AssertionError, match=msg):
            _run(c, dtype, fmt, record=False, **kw)
    r = next(k for k in GC.CASES if k.kind == "plain" and k.probe == "R+" and k.tile == 54 and not k.expect)

    def two_u(t):                                      # a 2 u error must fail the R+ gate
        t["ref"] *= 1 + 2 * GC.unit_roundoff(dtype)
    with pytest.raises(AssertionError, match="error / gate"):
        _run(r, dtype, fmt, tamper=two_u, record=False)


def test_the_wrappers_refuse_buffers_that_do_not_fit():
    """ops.gemm / conv3x3 / conv3x3_up_subpix: a caller's out / vt / stats / workspace of the wrong shape, format, stride or
    device raises PPError before anything is launched; a fitting strided window is taken with its row stride as ldo"""
    M, N, K = 128, 160, 64
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    buf = torch.zeros(M, N + 8, dtype=torch.bfloat16, device=DEV)
    assert ops.gemm(x, w, out=buf[:, :N]).data_ptr() == buf.data_ptr()
    for bad in (buf[:, :N - 8], buf[:M - 1, :N], buf[:, :N].float(), buf.t()[:N, :M].t()[:, ::1].cpu(), buf[:, :2 * N:2][:, :N // 2]):
        with pytest.raises(L.PPError, match="`out`"):
            ops.gemm(x, w, out=bad)
    with pytest.raises(L.PPError, match="`vt`"):
        ops.gemm(x, w, vt_col0=0, vt=torch.zeros(1, N, M, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(L.PPError, match="`vt`"):
        ops.gemm(x, torch.zeros(320, K, dtype=torch.bfloat16, device=DEV), vt_col0=160, rows_per_batch=64,
                 vt=torch.zeros(2, 160, 64, dtype=torch.float16, device=DEV))
    with pytest.raises(L.PPError, match="`stats`"):
        ops.gemm(x, w, row_stats=True, stats=torch.zeros(M, 2, 2, dtype=torch.float32, device=DEV))
    with pytest.raises(L.PPError, match="`workspace`"):
        ops.gemm(x, w, tile=32, splitk=1, workspace=torch.zeros(16, dtype=torch.float16, device=DEV))
    xk = torch.zeros(M, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.PPError, match="`workspace`"):                # two slabs of M x N floats do not fit into 16 words
        ops.gemm(xk, torch.zeros(N, 128, dtype=torch.bfloat16, device=DEV), tile=32, splitk=2,
                 workspace=torch.zeros(16, dtype=torch.float32, device=DEV))
    xc = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=DEV)
    wc = torch.zeros(N, 9 * 64, dtype=torch.bfloat16, device=DEV)
    cb = torch.zeros(1, 8, 8, N + 8, dtype=torch.bfloat16, device=DEV)
    assert ops.conv3x3(xc, wc, None, tile=32, splitk=1, out=cb[..., :N]).data_ptr() == cb.data_ptr()
    for bad in (cb[..., :N - 8], cb[:, :, ::2, :N], cb[..., :N].to(torch.float16), cb[..., :N].permute(0, 2, 1, 3)):
        with pytest.raises(L.PPError, match="`out`"):
            ops.conv3x3(xc, wc, None, tile=32, splitk=1, out=bad)
    for bad in (cb[..., :N - 8], cb[:, :, ::2, :N], cb[..., :N].to(torch.float16), cb[..., :N].cpu()):   # residuals: as `out`
        with pytest.raises(L.PPError, match="`res1`"):
            ops.conv3x3(xc, wc, None, tile=32, splitk=1, res1=bad)
        with pytest.raises(L.PPError, match="`res2`"):
            ops.conv3x3(xc, wc, None, tile=32, splitk=1, res2=bad)
    assert ops.conv3x3(xc, wc, None, tile=32, splitk=1, res1=cb[..., :N], res2=cb[..., 8:]).shape == (1, 8, 8, N)
    with pytest.raises(L.PPError, match="`ynext`"):
        ops.conv3x3(xc, wc, None, tile=32, splitk=1, ynext=torch.zeros(1, 8, 8, N, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(L.PPError, match="`out`"):
        ops.conv3x3_up_subpix(xc, torch.zeros(4, N, 4 * 64, dtype=torch.bfloat16, device=DEV), out=cb[..., :N])


def test_matrix_size():
    print(f"[gemm exact] {len(GC.CASES)} cases, {sum(len(GC.case_dtypes(c)) for c in GC.CASES)} (case, format) runs")
    assert len(GC.CASES) >= 250
