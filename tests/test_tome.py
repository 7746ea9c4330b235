"""CPU: token merging -- the invariants of the float64 restatement (tests/tome_cases.py), the public surface
(powerpaint_amd/tome.py) and the launch plans with and without it (dry builds: no launch runs in this file)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tome_cases as TC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import tome  # noqa: E402
from test_ip_adapter import TINY, _describe, _hip_unet, _net, _pipe  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ restatement
def _case(h=6, w=10, c=24, seed=0, ratio=0.5, win=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(h * w, c, generator=g, dtype=torch.float64)
    win = torch.randint(4, ((h // 2) * (w // 2),), generator=g).to(torch.uint8) if win is None else win
    nd = TC.window_count(h, w, 2, 2)
    return x, win, TC.merged_count(h * w, ratio, nd), nd


def test_r_zero_is_the_identity():
    x, win, _, _ = _case()
    d = TC.decide(x, 6, 10, 2, 2, win, 0)
    m = TC.merge_rows(x, d)
    assert m.shape == x.shape and torch.equal(TC.unmerge_rows(m, d), x)
    assert sorted(d["rowtok"].tolist()) == list(range(60)) and not d["merged"].any()


@pytest.mark.parametrize("h,w,ratio", [(6, 10, 0.5), (5, 7, 0.25), (8, 8, 0.75), (5, 7, 0.9)])
def test_unmerge_after_merge_keeps_every_kept_token(h, w, ratio):
    x, win, r, nd = _case(h, w, ratio=ratio)
    d = TC.decide(x, h, w, 2, 2, win, r)
    assert int(d["merged"].sum()) == r and d["rowtok"].numel() == h * w - r
    back = TC.unmerge_rows(TC.merge_rows(x, d), d)
    kept = d["src"][~d["merged"][d["src"]]]
    assert torch.equal(back[kept], x[kept])
    lone = [int(d["rowtok"][d["nkept"] + k]) for k, l_ in enumerate(d["lists"]) if not l_]
    assert torch.equal(back[lone], x[lone])
    # a merged source receives its destination's row: the mean of the destination and everything merged into it
    for k, l_ in enumerate(d["lists"]):
        if l_:
            t = int(d["rowtok"][d["nkept"] + k])
            want = x[[t] + l_].mean(dim=0)
            assert torch.allclose(back[l_], want.expand(len(l_), -1), rtol=0, atol=1e-14)
            assert torch.allclose(back[t], want, rtol=0, atol=1e-14)
    # the order of the merged sequence: kept sources ascending, then destinations ascending
    assert d["rowtok"][:d["nkept"]].tolist() == sorted(kept.tolist())
    assert d["rowtok"][d["nkept"]:].tolist() == sorted(d["dst"].tolist())


def test_merging_projected_rows_is_projecting_merged_rows():
    """The identity the engine rests on: merge is a mean, the Q / K / V projections are affine."""
    x, win, r, _ = _case(8, 8, c=32, ratio=0.5)
    g = torch.Generator().manual_seed(9)
    Wm, b = torch.randn(32, 48, generator=g, dtype=torch.float64), torch.randn(48, generator=g, dtype=torch.float64)
    d = TC.decide(x, 8, 8, 2, 2, win, r)
    a, c = TC.merge_rows(x @ Wm + b, d), TC.merge_rows(x, d) @ Wm + b
    assert float((a - c).abs().max()) <= 1e-12
    # ... and unmerging in front of an affine map equals unmerging behind it
    assert float((TC.unmerge_rows(c, d) @ Wm.T[:, :32] - TC.unmerge_rows(c @ Wm.T[:, :32], d)).abs().max()) <= 1e-12


def test_draw_order_and_count_per_evaluation():
    """One draw per eligible block per evaluation, in execution order, of shape (hsy, wsx, 1); none when use_rand is off or the
    logical batch is odd (the generator is then not advanced)."""
    blocks = [(8, 8), (8, 8), (4, 4)]
    g, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    dr = TC.Draws(g)
    got = [[dr.draw(h, w, 2, 2, 2) for h, w in blocks] for _ in range(2)]
    want = [[torch.randint(4, (h // 2, w // 2, 1), generator=g2).reshape(-1).to(torch.uint8) for h, w in blocks] for _ in range(2)]
    assert dr.count == 6 and all(torch.equal(a, b) for ra, rb in zip(got, want) for a, b in zip(ra, rb))
    assert not torch.equal(got[0][0], got[1][0])
    for kw, batch in ((dict(use_rand=False), 2), (dict(use_rand=True), 3)):
        g3 = torch.Generator().manual_seed(3)
        state = g3.get_state()
        dr = TC.Draws(g3, **kw)
        assert all(not dr.draw(h, w, 2, 2, batch).any() for h, w in blocks) and dr.count == 0
        assert torch.equal(g3.get_state(), state)


def test_leftover_rows_and_columns_are_sources():
    h, w = 5, 7
    win = torch.tensor([3, 0, 1, 2, 2, 3], dtype=torch.uint8)          # 2 x 3 windows
    src, dst = TC.partition(h, w, 2, 2, win)
    assert dst.tolist() == sorted([1 * 7 + 1, 0 * 7 + 2, 0 * 7 + 5, 3 * 7 + 0, 3 * 7 + 2, 3 * 7 + 5])
    assert all(t in src.tolist() for t in list(range(28, 35)) + [6, 13, 20, 27])     # row 4 and column 6
    assert src.numel() + dst.numel() == 35 and TC.merged_count(35, 0.9, 6) == 29 and TC.merged_count(35, 0.25, 6) == 8
    assert TC.downsample_of(64 * 64, 32 * 32) == 2 and TC.downsample_of(63 * 63, 32 * 32) == 2
    assert TC.eligible(4096, 4096, 1) and not TC.eligible(4096, 1024, 1) and TC.eligible(4096, 1024, 2)


def test_ties_go_to_the_lower_index():
    x = torch.zeros(16, 4, dtype=torch.float64)
    x[:, 0] = 1.0                                                      # every cosine is exactly 1
    win = torch.zeros(4, dtype=torch.uint8)
    d = TC.decide(x, 4, 4, 2, 2, win, 5)
    assert d["dst"].tolist() == [0, 2, 8, 10] and bool((d["best"][d["src"]] == 0).all())
    assert d["merged"].nonzero().flatten().tolist() == [1, 3, 4, 5, 6] and d["lists"][0] == [1, 3, 4, 5, 6]
    assert d["sel_margin"] == 0


# ------------------------------------------------------------------------------------------------------------ public surface
def test_apply_patch_validates_and_refuses_by_name():
    u = _hip_unet(**TINY)
    with pytest.raises(NotImplementedError, match="merge_crossattn"):
        tome.apply_patch(u, merge_crossattn=True)
    with pytest.raises(NotImplementedError, match="merge_mlp"):
        tome.apply_patch(u, merge_mlp=True)
    for bad in (dict(ratio=-0.1), dict(max_downsample=3), dict(sx=0), dict(sy=1.5), dict(generator=3)):
        with pytest.raises(ValueError):
            tome.apply_patch(u, **bad)
    assert u.net.tome is None
    with pytest.raises(TypeError):
        tome.apply_patch(object())
    assert tome.apply_patch(u) is u and tuple(u.net.tome) == (0.5, 1, 2, 2, True)
    p = _pipe(u)
    tome.apply_patch(p, ratio=0.25, use_rand=False)                    # a pipeline patches its UNet
    assert tuple(u.net.tome) == (0.25, 1, 2, 2, False)
    assert tome.remove_patch(p) is p and u.net.tome is None
    tome.apply_patch(u, merge_attn=False)
    assert u.net.tome is None


# ------------------------------------------------------------------------------------------------------------ plans
def _names(plan):
    return [c[2] for c in plan.calls]


NEW = ["tome_match", "tome_select", "tome_merge", "attention", "tome_unmerge"]


@pytest.mark.parametrize("twin", [False, True])
def test_plans_patched_and_unpatched(twin):
    from powerpaint_amd.engine import ToMe
    from powerpaint_amd.runtime import NetRuntime
    lib = L.lib()
    B, H, W = 2, 16, 16                                                # TINY: levels 16x16 (C = 320) and 8x8 (C = 640)
    never, net = _net(**TINY), _net(**TINY)
    rt0, rt = NetRuntime(never, "cpu"), NetRuntime(net, "cpu")
    rt0.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    want = (_describe(rt0.step_plan), _describe(rt0.setup_plan), rt0.arena.size, rt0.key)
    assert (_describe(rt.step_plan), _describe(rt.setup_plan), rt.arena.size, rt.key) == want
    assert not any(n.startswith("tome") for n in _names(rt.step_plan)) and rt.tome_blocks() == {}

    # the defaults: exactly the top-level transformers gain the four launches, their attention runs on n - r rows
    net.tome = ToMe(0.5, 1, 2, 2, True)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    assert rt.key != rt0.key
    top = ["down_blocks.0.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1"]
    assert list(rt.tome_blocks()) == top
    assert all((b.h, b.w, b.nd, b.r) == (16, 16, 64, 128) for b in rt.tome_blocks().values())
    assert [b.offset for b in rt.tome_blocks().values()] == [0, 64, 128] and rt.lay["tome"]["stride"] == 192
    names = _names(rt.step_plan)
    assert names.count("tome_match") == names.count("tome_select") == names.count("tome_merge") == \
        names.count("tome_unmerge") == 3
    for i, n in enumerate(names):
        if n == "tome_match":
            assert names[i:i + 5] == NEW
    stripped = [n for n in names if not n.startswith("tome")]
    assert stripped == _names(rt0.step_plan)
    att, att0 = [c for c in rt.step_plan.calls if c[2] == "attention"], [c for c in rt0.step_plan.calls if c[2] == "attention"]
    merged = [c for c in att if (c[1][10], c[1][11]) == (128, 128)]                 # nq, nk
    assert len(merged) == 3 and len(att) == len(att0)
    assert sum(1 for c in att0 if (c[1][10], c[1][11]) == (256, 256)) == 3
    assert not any((c[1][10], c[1][11]) == (256, 256) for c in att)
    for c in [c for c in rt.step_plan.calls if c[2] == "tome_match"]:
        assert c[0] is lib.pp_tome_match and c[1][11] is rt._tome_row and c[1][9] == 192      # the row cell, the row stride
    # every other launch is the unpatched plan's
    assert rt.step_plan.flops < rt0.step_plan.flops + 3 * 2.0 * 2 * 256 * 64 * 320

    # max_downsample = 2 adds the second level (8 x 8 tokens of 640 channels, mid block included)
    net.tome = ToMe(0.5, 2, 2, 2, True)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    assert list(rt.tome_blocks()) == top[:1] + ["mid_block.attentions.0"] + top[1:]
    assert (rt.tome_blocks()["mid_block.attentions.0"].nd, rt.tome_blocks()["mid_block.attentions.0"].r) == (16, 32)
    assert _names(rt.step_plan).count("tome_match") == 4

    # ratio 0: nothing merges, the plan is the unpatched one launch for launch (only the key knows)
    net.tome = ToMe(0.0, 1, 2, 2, True)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    assert _describe(rt.step_plan) == want[0] and rt.arena.size == want[2] and rt.tome_blocks() == {}

    # removed: the plan, the arena and the key of a network that never had it
    net.tome = None
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    assert (_describe(rt.step_plan), _describe(rt.setup_plan), rt.arena.size, rt.key) == want


def test_remove_patch_restores_the_models_plan():
    u = _hip_unet(**TINY)
    u.rt.ensure(2, 16, 16, 77, 4, ("plain",))
    want = (_describe(u.rt.step_plan), u.rt.key)
    tome.apply_patch(u, ratio=0.5)
    u.rt.ensure(2, 16, 16, 77, 4, ("plain",))
    assert "tome_match" in _names(u.rt.step_plan)
    tome.remove_patch(u)
    u.rt.ensure(2, 16, 16, 77, 4, ("plain",))
    assert (_describe(u.rt.step_plan), u.rt.key) == want


def test_window_table_rows_follow_the_generator():
    """NetRuntime.tome_fill: evaluations x blocks draws in evaluation-major, execution order; none for use_rand = False or an
    odd batch."""
    from powerpaint_amd.runtime import NetRuntime
    net = _net(**TINY)
    tome.apply_patch(type("M", (), {"net": net})(), generator=torch.Generator().manual_seed(11))
    rt = NetRuntime(net, "cpu")
    rt.ensure(2, 16, 16, 77, 4, ("plain",))
    assert rt.tome_fill(3, net.tome_state) == 9
    tb = rt.tome_table()
    ref = TC.Draws(torch.Generator().manual_seed(11))
    want = torch.stack([torch.cat([ref.draw(16, 16, 2, 2, 2) for _ in range(3)]) for _ in range(3)])
    assert tb.shape == (3, 192) and torch.equal(tb, want) and not torch.equal(tb[0], tb[1])
    rt.ensure(3, 16, 16, 77, 4, ("plain",))                            # an odd batch: index 0 everywhere, no draw
    assert rt.tome_fill(2, net.tome_state) == 0 and not rt.tome_table().any()
    with pytest.raises(L.PPError, match="window table"):
        rt.tome_fill(100000, net.tome_state)
