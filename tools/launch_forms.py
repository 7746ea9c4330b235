"""The pinned decision table of the GEMM / conv launch-form queries: tests/golden/launch_forms.json.

    python -m tools.launch_forms            # rewrite the fixture from the library that is loaded (powerpaint_amd/_lib.py)
    python -m tools.launch_forms --check    # compare the loaded library with the fixture instead

The six host queries around pp_gemm_bf16 (include/pp_hip.h) are pure host logic, so a fixed grid of synthetic requests with
dummy non-null pointers pins what the launch-plan compiler is told, request by request, without a GPU.  The fixture carries
pp_build_id() of the library that answered: a table meant to pin a refactor is written from the PARENT commit's build, and
tests/test_abi.py shows how to recompute that id from a checkout.  pp_gemm_combine_ctr_bytes consults the placement probe
(pp_xcd_placement_ok), which needs a device: that column is null when the generator runs without one.

COLUMNS of a row, in order:
    ws           pp_gemm_workspace_bytes
    gn_stats     pp_gemm_gn_stats_ok
    halo         pp_conv_gn_supported (0 / 1 / 2)
    preferred    pp_conv_gn_preferred where gn_in_* is set, else null (0 in every shipping build: no class is fused any more)
    fused        pp_gemm_combine_fused with a dummy tile_ctr, nothing else set
    fused_gn     ... with one gn_acc subscription
    fused_next   ... with gn_next_* as well
    gn_next      pp_gemm_gn_next_ok(., 0) with that subscription
    ctr          pp_gemm_combine_ctr_bytes (null without a device)
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from powerpaint_amd import _lib as L  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_forms.json")
COLUMNS = ["ws", "gn_stats", "halo", "preferred", "fused", "fused_gn", "fused_next", "gn_next", "ctr"]
V2_TILES = [21, 31, 22, 32, 42, 62, 23, 33, 24, 53, 44, 54]          # the internal ids pp_gemm_bf16 accepts in PPGemmArgs.tile
PTR = {"x1": 0x1000, "x2": 0x2000, "x3": 0x3000, "x4": 0x4000, "w": 0x5000, "out": 0x6000, "gn_in_acc": 0x7000,
       "gn_in_gb": 0x8000, "workspace": 0x9000, "gn_acc": 0xa000, "gn_next_out": 0xb000, "gn_next_gamma": 0xc000,
       "gn_next_beta": 0xd000, "tile_ctr": 0xe000, "res1": 0xf000, "rowvec": 0x10000, "out_vt": 0x11000,
       "row_stats_out": 0x12000, "ln_stats": 0x13000, "ln_colsum": 0x14000}
BATCHES, WIDTHS = (1, 2, 4, 8), (8, 16, 32, 64, 128)


def _conv(B, W, c1, c2, cout, kind, tile, splitk, gn_in):
    """kind: plain / stride2 / up / tail (the merged 1x1 shortcut over c3 + c4 channels at the output pixel)"""
    stride, up = (2 if kind == "stride2" else 1), int(kind == "up")
    c3, c4 = ((2 * cout, cout) if c2 else (cout, 0)) if kind == "tail" else (0, 0)
    wo = (2 * W if up else W) // stride
    r = dict(x_mode=L.PP_X_CONV3X3, M=B * wo * wo, N=cout, K=9 * (c1 + c2) + c3 + c4, c1=c1, c2=c2, c3=c3, c4=c4, batch=B,
             hin=W, win=W, hout=wo, wout=wo, stride=stride, up=up, rows_per_batch=wo * wo, ldo=cout, ldres1=cout, ldres2=cout,
             tile=tile, splitk=splitk)
    for i, c in enumerate((c1, c2, c3, c4)):
        if c:
            r["x%d" % (i + 1)] = PTR["x%d" % (i + 1)]
    if gn_in:
        r.update(gn_in_acc=PTR["gn_in_acc"], gn_in_gb=PTR["gn_in_gb"], gn_in_groups=32, gn_in_silu=1, gn_in_eps=1e-5)
    return r


def _gemm(M, hw, K1, K2, N, act, tile, splitk, flag):
    """flag: one of the request features that steer choose(), v2_ok() and the combine predicates"""
    r = dict(x_mode=L.PP_X_PLAIN, M=M, N=N, K=K1 + K2, c1=K1, c2=K2, ldx1=K1, ldx2=K2, x1=PTR["x1"], act=act,
             ldo=N // 2 if act == L.PP_ACT_GEGLU else N, ldres1=N, ldres2=N, tile=tile, splitk=splitk, _hw=hw)
    if K2:
        r["x2"] = PTR["x2"]
    if flag == "out_f32":
        r["out_f32"] = 1
    elif flag in ("out_vt", "out_vt_off160"):
        r["vt_col0"] = max(160, N // 320 * 160) + (8 if flag == "out_vt_off160" else 0)
        r.update(out_vt=PTR["out_vt"], vt_ld=hw, rows_per_batch=hw, ldo=r["vt_col0"])
    elif flag == "row_stats":
        r["row_stats_out"] = PTR["row_stats_out"]
    elif flag == "ln_stats":
        r.update(ln_stats=PTR["ln_stats"], ln_colsum=PTR["ln_colsum"], ln_tiles=(K1 + 159) // 160, ln_dim=K1, ln_eps=1e-5)
    elif flag == "rowvec":
        r.update(rowvec=PTR["rowvec"], ld_rowvec=N, rows_per_batch=hw)
    elif flag == "dup":
        r["out_dup_rows"] = M
    elif flag == "res1_odd_ld":
        r.update(res1=PTR["res1"], ldres1=N + 4)
    elif flag in ("n4", "n12", "n324"):
        r["N"] = r["ldo"] = r["ldres1"] = r["ldres2"] = int(flag[1:])
        r["act"] = L.PP_ACT_NONE
    elif flag == "softmax80":
        r.update(act=L.PP_ACT_SOFTMAX80, ldo=N, w_batch_stride=N * (K1 + K2), rows_per_batch=hw)
    return r


def requests():
    """The fixed grid, thinned by fixed strides (every shape appears; the tile / split / feature axes rotate over the shapes)."""
    out = []
    cins = [(c, 0) for c in (320, 640, 960, 1280, 1920, 2560)] + [(640, 320), (1280, 640), (1280, 1280), (320, 320), (640, 640)]
    axes = [(kind, tile, sk, gn_in) for kind in ("plain", "stride2", "up", "tail") for tile in (0, 1, 2, 3, 54)
            for sk in (0, 1, 2, 4, 8) for gn_in in (0, 1)]
    i = 0
    for B in BATCHES:
        for W in WIDTHS:
            for c1, c2 in cins:
                for cout in (320, 640, 1280):
                    for j in range(5):                        # 5 of the 200 (kind, tile, splitk, gn_in) combinations per shape
                        out.append(_conv(B, W, c1, c2, cout, *axes[(i * 5 + j) * 37 % len(axes)]))
                    i += 1
    flags = ["", "out_f32", "out_vt", "out_vt_off160", "row_stats", "ln_stats", "rowvec", "dup", "res1_odd_ld", "n4", "n12", "n324",
             "softmax80"]
    tiles = [0, 1, 2, 3] + V2_TILES
    i = 0
    for B in BATCHES:
        for W in WIDTHS:
            for Cc in (320, 640, 1280):
                for K1, K2, N, act in ((Cc, 0, Cc, 0), (Cc, 0, 3 * Cc, 0), (Cc, 0, 8 * Cc, L.PP_ACT_GEGLU), (4 * Cc, 0, Cc, 0),
                                       (4 * Cc, Cc, Cc, 0), (Cc, 0, 2 * Cc, 0)):
                    for j in range(7):
                        h = (i * 7 + j) * 2654435761 >> 8            # (a fixed scramble: the axes must not rotate in step)
                        flag = flags[(h >> 7) % len(flags)] if (h >> 11) % 3 else ""
                        out.append(_gemm(B * W * W, W * W, K1, K2, N, act, tiles[h % len(tiles)], (0, 0, 1, 2, 4, 8)[(h >> 4) % 6], flag))
                    i += 1
    return out


def describe(r) -> str:
    return " ".join("%s=%s" % (k, hex(v) if k in PTR else v) for k, v in sorted(r.items()) if not k.startswith("_"))


def grid_digest(reqs) -> str:
    return hashlib.sha256("\n".join(describe(r) for r in reqs).encode()).hexdigest()[:12]


def _args(r):
    a = L.PPGemmArgs()
    a.dtype, a.scale = L.PP_DT_BF16, 1.0
    a.w, a.out, a.workspace = PTR["w"], PTR["out"], PTR["workspace"]
    for k, v in r.items():
        if not k.startswith("_"):
            setattr(a, k, v)
    return a


def answers(lib, r):
    q = lambda fn, a, *more: int(fn(C.byref(a), *more))      # noqa: E731
    a = _args(r)
    row = [q(lib.pp_gemm_workspace_bytes, a), q(lib.pp_gemm_gn_stats_ok, a), q(lib.pp_conv_gn_supported, a),
           q(lib.pp_conv_gn_preferred, a) if "gn_in_acc" in r else None]
    ctr = q(lib.pp_gemm_combine_ctr_bytes, a)
    a.tile_ctr = PTR["tile_ctr"]
    row.append(q(lib.pp_gemm_combine_fused, a))
    if not a.rows_per_batch:
        a.rows_per_batch = r["_hw"]
    a.gn_acc[0], a.gn_cg[0], a.gn_c0[0], a.gn_groups[0] = PTR["gn_acc"], a.N // 32, 0, 32
    row.append(q(lib.pp_gemm_combine_fused, a))
    gn_next = q(lib.pp_gemm_gn_next_ok, a, 0)
    a.gn_next_out, a.gn_next_gamma, a.gn_next_beta = PTR["gn_next_out"], PTR["gn_next_gamma"], PTR["gn_next_beta"]
    a.gn_next_eps, a.gn_next_silu, a.gn_next_sub = 1e-5, 1, 0
    row += [q(lib.pp_gemm_combine_fused, a), gn_next, ctr]
    return row


def table(lib, reqs, with_ctr: bool):
    rows = [answers(lib, r) for r in reqs]
    if not with_ctr:
        for row in rows:
            row[-1] = None
    return rows


def check_discriminates(reqs, rows):
    """A table every column of which is constant, or that never sees a split or a fused launch, pins nothing."""
    for k, name in enumerate(COLUMNS):
        vals = {row[k] for row in rows}
        assert len(vals) >= 2 or (name == "ctr" and vals == {None}), "column %s is constant: %s" % (name, vals)
    splits = {row[0] // (4 * r["M"] * r["N"]) if row[0] else 1 for r, row in zip(reqs, rows)}      # (the scratch behind the slabs
    assert {1, 2, 4, 8} <= splits, splits                                                          #  is far below one slab)
    assert {row[2] for row in rows} == {0, 1, 2}
    for k in (4, 5, 6):
        ones = sum(row[k] for row in rows)
        assert ones >= 50 and len(rows) - ones >= 50, "%s: %d of %d" % (COLUMNS[k], ones, len(rows))


def device_present(lib) -> bool:
    return lib.pp_xcd_placement_ok() == 1


def main(argv):
    lib = L.lib()
    reqs = requests()
    assert len(reqs) <= 6000, len(reqs)
    with_ctr = device_present(lib)
    rows = table(lib, reqs, with_ctr)
    check_discriminates(reqs, rows)
    if "--check" in argv:
        fx = json.load(open(FIXTURE))
        assert fx["grid"] == grid_digest(reqs), "the request grid is not the fixture's"
        bad = [(r, want, got) for r, want, got in zip(reqs, fx["rows"], rows)
               if want[:-1] != got[:-1] or (with_ctr and want[-1] is not None and want[-1] != got[-1])]
        for r, want, got in bad[:20]:
            print("MISMATCH %s\n  fixture %s\n  library %s" % (describe(r), want, got))
        print("%d requests, %d mismatches (library %s, fixture %s)" % (len(reqs), len(bad), L.build_id(), fx["build_id"]))
        return 1 if bad else 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else FIXTURE
    with open(out, "w") as f:
        f.write('{"build_id": "%s", "grid": "%s", "columns": %s, "rows": [\n' % (L.build_id(), grid_digest(reqs), json.dumps(COLUMNS)))
        f.write(",\n".join(json.dumps(row, separators=(",", ":")) for row in rows))
        f.write("\n]}\n")
    print("%s: %d requests, %d distinct answer rows, build %s, ctr column %s" %
          (out, len(reqs), len({tuple(row) for row in rows}), L.build_id(), "recorded" if with_ctr else "null (no device)"))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
