"""CPU: HyperTile -- the tiling rule and the float64 restatement (tests/hypertile_cases.py), the public surface
(powerpaint_amd/hypertile.py), the host-side predicate and argument checks of the two C entries, and the launch plans with and
without the patch (dry builds: no launch runs in this file)."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hypertile_cases as HC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import hypertile, tome  # noqa: E402
from test_ip_adapter import TINY, _describe, _hip_unet, _net, _pipe  # noqa: E402

TOP = ["down_blocks.0.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1"]


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("v,tile_size", sorted(HC.RULE_SIDES))
def test_rule_on_a_table_of_sides(v, tile_size):
    want = HC.RULE_SIDES[(v, tile_size)]
    assert HC.split(v, tile_size) == want                                  # the restatement against the hand-made table
    assert hypertile.layout(v, v, tile_size) == (want, want)               # the product against both
    s = v // want
    T = max(32, tile_size) // 8
    assert v % s == 0 and s >= min(T, v) and not any(v % c == 0 for c in range(min(T, v), s))


def test_rule_on_the_layouts_the_issue_names():
    for (H, W), want in HC.RULE_LAYOUTS.items():
        assert hypertile.layout(H, W) == want == HC.layout(H, W), (H, W)
    assert hypertile.layout(96, 64, tile_size=256) == (3, 2) and hypertile.layout(64, 96, tile_size=256) == (2, 3)
    assert hypertile.layout(128, 128, tile_size=512) == (2, 2)
    for bad in (0, -8, 12, 100, 8.5):
        with pytest.raises(ValueError, match="tile_size"):
            hypertile.layout(64, 64, tile_size=bad)


@pytest.mark.parametrize("h,w,nh,nw", [(4, 6, 2, 3), (6, 4, 1, 2), (5, 8, 5, 1), (3, 3, 1, 1)])
def test_token_map_and_rearrange_agree(h, w, nh, nw):
    tm = HC.token_map(h, w, nh, nw)
    assert sorted(tm.flatten().tolist()) == list(range(h * w))             # a permutation of the grid
    x = torch.arange(2 * h * w * 3, dtype=torch.float64).reshape(2, h * w, 3)
    t = HC.to_tiles(x, h, w, nh, nw)
    assert torch.equal(t, x[:, tm].reshape(2 * nh * nw, -1, 3))            # rearrange == gather through token(r)
    assert torch.equal(HC.from_tiles(t, 2, h, w, nh, nw), x)
    th, tw = h // nh, w // nw
    for tile in range(nh * nw):                                            # every token of a tile lies inside the tile's box
        ys, xs = tm[tile] // w, tm[tile] % w
        assert int(ys.min()) == (tile // nw) * th and int(ys.max()) == (tile // nw) * th + th - 1
        assert int(xs.min()) == (tile % nw) * tw and int(xs.max()) == (tile % nw) * tw + tw - 1


def test_tiled_attention_restatement():
    g = torch.Generator().manual_seed(0)
    B, h, w, H, d = 2, 4, 6, 2, 5
    q, k, v = (torch.randn(B, h * w, H, d, generator=g, dtype=torch.float64) for _ in range(3))
    full = HC.tiled_attention_f64(q, k, v, h, w, 1, 1, 0.3)
    p = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * 0.3, -1)
    assert torch.allclose(full, torch.einsum("bhij,bjhd->bihd", p, v), rtol=0, atol=1e-13)      # one tile: plain attention
    out, A = HC.tiled_attention_f64(q, k, v, h, w, 2, 3, 0.3, with_abs=True)
    tm = HC.token_map(h, w, 2, 3)
    for tile in range(6):                                                  # a tile's output depends on the tile alone
        idx = tm[tile]
        alone = HC.tiled_attention_f64(q[:, idx], k[:, idx], v[:, idx], 2, 2, 1, 1, 0.3)
        assert torch.allclose(out[:, idx], alone, rtol=0, atol=1e-13)
    assert bool((A >= out.abs() - 1e-13).all()) and not torch.allclose(out, full)
    k2, v2 = k.clone(), v.clone()
    k2[:, tm[1:].flatten()] += 7.0                                        # keys outside tile 0 do not reach tile 0
    v2[:, tm[1:].flatten()] -= 3.0
    out2 = HC.tiled_attention_f64(q, k2, v2, h, w, 2, 3, 0.3)
    assert torch.equal(out2[:, tm[0]], out[:, tm[0]]) and not torch.equal(out2[:, tm[1]], out[:, tm[1]])


# ------------------------------------------------------------------------------------------------------------ public surface
def test_apply_patch_validates_and_refuses_by_name():
    u = _hip_unet(**TINY)
    with pytest.raises(NotImplementedError, match="swap_size"):
        hypertile.apply_patch(u, swap_size=2)
    with pytest.raises(NotImplementedError, match="max_depth"):
        hypertile.apply_patch(u, max_depth=1)
    for bad in (0, -256, 100, 12, 255.5):
        with pytest.raises(ValueError, match="tile_size"):
            hypertile.apply_patch(u, tile_size=bad)
    assert u.net.hypertile is None
    with pytest.raises(TypeError):
        hypertile.apply_patch(object())
    assert hypertile.apply_patch(u) is u and tuple(u.net.hypertile) == (256,)
    p = _pipe(u)
    hypertile.apply_patch(p, tile_size=128)                                # a pipeline patches the networks it holds
    assert tuple(u.net.hypertile) == (128,)
    assert hypertile.remove_patch(p) is p and u.net.hypertile is None


def test_hypertile_with_token_merging_is_refused_naming_both():
    u = _hip_unet(**TINY)
    tome.apply_patch(u)
    with pytest.raises(L.PPError, match=r"HyperTile.*token merging \(ToMe\)"):
        hypertile.apply_patch(u)
    assert u.net.hypertile is None
    tome.remove_patch(u)
    hypertile.apply_patch(u)
    tome.apply_patch(u)                                                    # the other order: refused when the plan is built
    with pytest.raises(L.PPError, match=r"HyperTile.*token merging \(ToMe\)"):
        u.rt.ensure(2, 16, 64, 77, 4, ("plain",))


# ------------------------------------------------------------------------------------------------------------ C entries
TILED_OK = [
    # h, w, nh, nw, d -> ok
    ((64, 64, 2, 2, 40), 1), ((128, 128, 4, 4, 40), 1), ((96, 64, 3, 2, 40), 1), ((16, 64, 1, 2, 40), 1),
    ((8, 128, 1, 2, 40), 1), ((4, 256, 1, 2, 40), 1), ((32, 32, 2, 1, 40), 1), ((20, 32, 2, 1, 40), 1),
    ((10, 64, 1, 2, 40), 1), ((32, 40, 2, 1, 40), 1),                     # bands of any width: 16 x 40 = 640 keys
    ((64, 192, 1, 2, 40), 1),                                              # tw = 96: a multiple of 32, not of 64
    ((64, 64, 1, 1, 40), 0),                                               # one tile: not the tiled kernel's business
    ((64, 64, 3, 2, 40), 0), ((64, 64, 2, 3, 40), 0),                      # h % nh, w % nw
    ((64, 64, 2, 2, 80), 0), ((64, 64, 2, 2, 160), 0), ((64, 64, 2, 2, 64), 0),        # head dims of the deeper levels
    ((16, 16, 2, 2, 40), 0),                                               # 64-token tiles: fewer than four LDS tiles
    ((8, 64, 2, 2, 40), 0),                                                # 4 x 32 = 128 keys
    ((32, 80, 2, 2, 40), 0),                                               # tw = 40 with nw > 1: a half would straddle a run
    ((30, 48, 2, 2, 40), 0),                                               # 15 x 24 = 360 keys: no multiple of 64
    ((0, 64, 1, 2, 40), 0), ((64, 64, 0, 2, 40), 0), ((64, 64, -2, -2, 40), 0),
]


@pytest.mark.parametrize("args,want", TILED_OK)
def test_tiled_ok_on_a_table(args, want):
    lib = L.lib()
    assert lib.pp_attention_tiled_ok(*args) == want
    h, w, nh, nw, d = args
    if want:                                                               # ... and it restates nothing: the pieces it is made of
        nt = (h // nh) * (w // nw)
        assert lib.pp_attention_log2_ok(nt, nt, d) == 1 and (nw == 1 or (w // nw) % 32 == 0)


def test_entry_rejects_bad_arguments_without_a_gpu():
    lib = L.lib()
    BAD, UNSUP = -1, -2
    P = 0x10000                                                            # never dereferenced: every call returns before a launch

    def call(q=P, ldq=648, k=P, ldk=648, vt=P, ldvt=1024, o=P, ldo=320, batch=1, heads=8, h=16, w=64, nh=1, nw=2, d=40,
             variant=L.PP_ATTN_AUTO, dtype=L.PP_DT_BF16):
        return lib.pp_attention_fwd_tiled(q, ldq, k, ldk, vt, ldvt, o, ldo, batch, heads, h, w, nh, nw, d, 0.158, variant, dtype,
                                          None)

    for kw in (dict(q=None), dict(k=None), dict(vt=None), dict(o=None)):                      # null
        assert call(**kw) == BAD, kw
    for kw in (dict(ldq=644), dict(ldk=650), dict(ldvt=1028), dict(ldo=322), dict(ldvt=1016)):      # misaligned, ldvt < h*w
        assert call(**kw) == BAD, kw
    for kw in (dict(nh=3), dict(nw=5), dict(nh=0), dict(h=0), dict(batch=0), dict(heads=0), dict(dtype=0), dict(dtype=7),
               dict(variant=9), dict(variant=-1)):
        assert call(**kw) == BAD, kw
    assert call(variant=L.PP_ATTN_PHASED) == UNSUP
    assert call(d=80) == UNSUP and call(nh=1, nw=1) == UNSUP and call(h=4) == UNSUP          # outside pp_attention_tiled_ok
    assert L.ABI_VERSION == 29 and lib.pp_abi_version() == 29


# ------------------------------------------------------------------------------------------------------------ plans
def _attn(plan):
    return [c for c in plan.calls if c[2] == "attention"]


def _launches(rt, plan):
    """Every launch of a plan with every argument: (name, entry, args), arena pointers as offsets from the arena's base (an
    arena is allocated anew by every re-plan), PPGemmArgs field by field, ctypes cells by value."""
    lo, hi = rt.arena.base, rt.arena.base + max(rt.arena.size, 1)

    def norm(v):
        obj = getattr(v, "_obj", None)
        if isinstance(obj, ctypes.Structure):
            return tuple((f[0], norm(getattr(obj, f[0]))) for f in obj._fields_)
        if isinstance(v, ctypes.Array):
            return tuple(norm(x) for x in v)
        if isinstance(v, ctypes._SimpleCData):
            v = v.value
        if isinstance(v, int) and not isinstance(v, bool) and lo <= v < hi:
            return ("arena", v - lo)
        return v

    return [(c[2], c[0].__name__, tuple(norm(a) for a in c[1])) for c in plan.calls]


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("H,W", [(64, 64), (16, 64), (13, 24)])
def test_unpatched_plans_are_the_parents(H, W, twin):
    """A network that had the patch and lost it, and one whose patch leaves the latent in one tile, compile the plans of a
    network that never saw it: launch for launch, argument for argument, the same arena and (removed) the same key."""
    from powerpaint_amd.engine import HyperTile
    from powerpaint_amd.runtime import NetRuntime
    never, net = _net(**TINY), _net(**TINY)
    rt0, rt = NetRuntime(never, "cpu"), NetRuntime(net, "cpu")
    rt0.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    want = (_describe(rt0.step_plan), _describe(rt0.setup_plan), rt0.arena.size, rt0.step_plan.flops, rt0.key)
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    before = (_launches(rt, rt.step_plan), _launches(rt, rt.setup_plan))
    net.hypertile = HyperTile(256)
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    net.hypertile = None
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    assert (_describe(rt.step_plan), _describe(rt.setup_plan), rt.arena.size, rt.step_plan.flops, rt.key) == want
    assert (_launches(rt, rt.step_plan), _launches(rt, rt.setup_plan)) == before          # argument for argument
    assert not any(c[0] is L.lib().pp_attention_fwd_tiled for c in rt.step_plan.calls)
    net.hypertile = HyperTile(2048)                                        # T = 256 latent pixels: every side stays whole
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    assert (_describe(rt.step_plan), _describe(rt.setup_plan), rt.arena.size, rt.step_plan.flops) == want[:4]
    assert rt.key != rt0.key and all(not v[2] for v in net.hypertile_layout(H, W).values())


def test_remove_patch_restores_the_models_plan_key():
    u = _hip_unet(**TINY)
    u.rt.ensure(2, 64, 64, 77, 4, ("plain",))
    want = (_describe(u.rt.step_plan), u.rt.key)
    hypertile.apply_patch(u)
    u.rt.ensure(2, 64, 64, 77, 4, ("plain",))
    assert u.rt.key != want[1] and ("hypertile", (256,)) in u.rt.key
    assert any(c[0] is L.lib().pp_attention_fwd_tiled for c in u.rt.step_plan.calls)
    hypertile.remove_patch(u)
    u.rt.ensure(2, 64, 64, 77, 4, ("plain",))
    assert (_describe(u.rt.step_plan), u.rt.key) == want


@pytest.mark.parametrize("twin", [False, True])
def test_patched_plan_of_a_64x64_unet(twin):
    """The same launch count; only the attn1 launches of the C = 320 blocks differ: the tiled entry on the same operands with
    the grid geometry in place of (nq, nk), and a quarter of their FLOPs in the plan's count."""
    from powerpaint_amd.runtime import NetRuntime
    lib = L.lib()
    B, H, W = 2, 64, 64
    never, net = _net(**TINY), _net(**TINY)
    rt0, rt = NetRuntime(never, "cpu"), NetRuntime(net, "cpu")
    rt0.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    hypertile.apply_patch(type("M", (), {"net": net})())
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    lay = net.hypertile_layout(H, W)
    assert [p for p, v in lay.items() if v[2]] == TOP and all(lay[p] == (2, 2, True, "tiled") for p in TOP)
    assert lay["mid_block.attentions.0"][:3] == (1, 1, False) and "depth" in lay["mid_block.attentions.0"][3]
    assert len(rt.step_plan.calls) == len(rt0.step_plan.calls) and rt.arena.size == rt0.arena.size
    assert _describe(rt.setup_plan) == _describe(rt0.setup_plan)
    assert _describe(rt0.step_plan) == _describe(rt.step_plan)
    # argument for argument on ONE network (parameter pointers are the network's): unpatch the same runtime
    d1 = _launches(rt, rt.step_plan)
    hypertile.remove_patch(type("M", (), {"net": net})())
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    d0 = _launches(rt, rt.step_plan)
    diff = [i for i, (a, b) in enumerate(zip(d0, d1)) if a != b]
    assert len(diff) == 3 and len(d0) == len(d1)
    saved, flops0 = 0.0, rt.step_plan.flops
    assert flops0 == rt0.step_plan.flops
    hypertile.apply_patch(type("M", (), {"net": net})())
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    for i in diff:
        c0, c1 = d0[i], d1[i]
        assert c0[0] == c1[0] == "attention" and c1[1] == "pp_attention_fwd_tiled"
        assert c0[1] in ("pp_attention_fwd", "pp_attention_fwd_variant")
        a0, a1 = list(c0[2]), list(c1[2])
        assert a1[:10] == a0[:10]                                          # q, ldq, k, ldk, vt, ldvt, o, ldo, batch, heads
        assert a0[10:13] == [H * W, H * W, 40] and a1[10:15] == [H, W, 2, 2, 40] and a1[15] == a0[13]
        log2 = c0[1] == "pp_attention_fwd_variant"
        assert a1[16] == (L.PP_ATTN_PIPE_LOG2 if log2 else L.PP_ATTN_AUTO) and a1[17] == a0[14]
        saved += 4.0 * a0[8] * a0[9] * (H * W) ** 2 * 40 * 0.75
    assert rt0.step_plan.flops - rt.step_plan.flops == pytest.approx(saved, rel=1e-12)


def test_a_tiled_and_an_untiled_block_in_one_plan():
    """hypertile_layout names every transformer and says why it is or is not tiled."""
    from powerpaint_amd.runtime import NetRuntime
    net = _net(**TINY)
    hypertile.apply_patch(type("M", (), {"net": net})())
    lay = net.hypertile_layout(16, 64)
    assert list(lay) == [p for p, _ in net._attn_specs()]
    assert all(lay[p] == (1, 2, True, "tiled") for p in TOP) and not lay["mid_block.attentions.0"][2]
    lay = net.hypertile_layout(16, 40)                                     # side(40) = 40, side(16) = 16: one tile
    assert all(v[:3] == (1, 1, False) for v in lay.values()) and "one tile" in lay[TOP[0]][3]
    lay = net.hypertile_layout(4, 64)                                      # 1 x 2 tiles of 4 x 32 = 128 keys: the predicate says no
    assert all(lay[p][:3] == (1, 2, False) and "pp_attention_tiled_ok" in lay[p][3] for p in TOP)
    rt = NetRuntime(net, "cpu")
    rt.ensure(2, 4, 64, 77, 4, ("plain",))
    assert not any(c[0] is L.lib().pp_attention_fwd_tiled for c in rt.step_plan.calls)
    rt.ensure(2, 16, 64, 77, 4, ("plain",))
    att = _attn(rt.step_plan)
    tiled = [c for c in att if c[0] is L.lib().pp_attention_fwd_tiled]
    assert len(tiled) == 3 and len(att) > 3                                # the mid block's attention stays as it is
    assert hypertile.remove_patch(type("M", (), {"net": net})()) and net.hypertile_layout(16, 64) == {}


def test_pag_layer_keeps_the_tiled_launch_on_the_leading_items():
    from powerpaint_amd.engine import PAG
    from powerpaint_amd.runtime import NetRuntime
    lib = L.lib()
    net = _net(**TINY)
    hypertile.apply_patch(type("M", (), {"net": net})())
    rt = NetRuntime(net, "cpu")
    rt.ensure(3, 16, 64, 77, 4, ("plain",), pag=PAG((TOP[0], "mid_block.attentions.0"), 1))
    calls = rt.step_plan.calls
    ids = [i for i, c in enumerate(calls) if c[2] == "attn_identity_v"]
    assert len(ids) == 2
    first = calls[ids[0] - 1]
    assert first[0] is lib.pp_attention_fwd_tiled and list(first[1])[8] == 2 and list(first[1])[10:14] == [16, 64, 1, 2]
    assert list(calls[ids[0]][1])[2:4] == [2, 1]                           # identity for the last item, unchanged
    assert calls[ids[1] - 1][0] is not lib.pp_attention_fwd_tiled          # the mid block: the untiled launch
