"""CPU: latent sizes that are no multiple of 2^(levels - 1) -- the size chain, the launch plans of the three networks and of
the VAE on a CPU arena, the widened `up` contract of PP_X_CONV3X3 (ABI v29) as far as the host decides it, and the fixture
tests/golden/ref_any_size.pt against its generator.  The arithmetic is checked on the GPU (tests/test_any_size_gpu.py)."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd.engine import Act, Arena, Builder, SDNet, level_sizes  # noqa: E402
from powerpaint_amd.runtime import NetRuntime  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "ref_any_size.pt"), weights_only=False)
SIZES = [(13, 10), (9, 11), (10, 12)]
FIX = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1)      # the fixture's architecture


def test_level_sizes_is_the_ceil_halving_chain():
    """Downsample2D = conv3x3, stride 2, padding 1: h -> (h - 1) // 2 + 1.  The chains of the fixture's sizes, and the sizes accepted before
    (multiples of 8), where the chain is h >> level."""
    assert level_sizes(13, 10, 4) == [(13, 10), (7, 5), (4, 3), (2, 2)]
    assert level_sizes(9, 11, 4) == [(9, 11), (5, 6), (3, 3), (2, 2)]
    assert level_sizes(10, 12, 4) == [(10, 12), (5, 6), (3, 3), (2, 2)]
    assert level_sizes(106, 80, 4) == [(106, 80), (53, 40), (27, 20), (14, 10)]
    for h, w in ((64, 64), (16, 16), (72, 40), (8, 24)):
        assert level_sizes(h, w, 4) == [(h >> i, w >> i) for i in range(4)]
    assert level_sizes(5, 7, 1) == [(5, 7)]


def _runtime(kind, cin, H, W, B=2, twin=False, **kw):
    cfg = dict(brushnet=dict(conditioning_channels=5), controlnet=dict(conditioning_channels=3)).get(kind, {})
    net = SDNet(kind, cin, **cfg, **kw)
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    rt = NetRuntime(net, "cpu")
    wiring = ("plain",)
    if kind == "unet" and cin == 4:         # the UNet behind a BrushNet: 8 + 1 + 11 residual slots
        shapes = rt._residual_shapes(B, H, W, with_up=True)
        wiring = ("brushnet", {k: [0] * len(v) for k, v in shapes.items()})
    rt.ensure(B, H, W, 77, net.cin0, wiring, cond_hw=(8 * H, 8 * W) if kind == "controlnet" else None, twin=twin)
    return rt


def _shape(a):
    return (a.B, a.C, a.H, a.W)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plans_build_at_sizes_off_the_grid(hw):
    """SDNet.build_setup + build_step for the UNet (alone and behind a BrushNet), the BrushNet and the ControlNet: the skip and
    hidden sizes agree in every up block (the assert inside build_step), the residual tensors have the reference's shapes,
    every upsampler is the nine-tap `up` request with the next skip tensor's size as its target."""
    H, W = hw
    gold = GOLD["nets"][f"{H}x{W}"]
    chain = level_sizes(H, W, 4)
    for twin in (False, True):
        rt = _runtime("brushnet", 4, H, W, twin=twin, **FIX)
        outs = rt.outputs
        got = [_shape(a) for a in outs["down"] + [outs["mid"]] + outs["up"]]
        assert got == [tuple(s) for s in gold["res_shapes"]]
        assert (len(outs["down"]), len(outs["up"])) == (gold["n_down"], gold["n_up"])
        assert not rt.net.upfold and not rt.net.xa          # no sub-pixel fold, no folded cross-attention at these sizes
        rt = _runtime("controlnet", 4, H, W, twin=twin, **FIX)
        got = [_shape(a) for a in rt.outputs["down"] + [rt.outputs["mid"]]]
        assert got == [tuple(s) for s in gold["ctrl_shapes"]]
        for cin in (9, 4):
            rt = _runtime("unet", cin, H, W, twin=twin, **FIX)
            assert "eps" in rt.outputs and not rt.net.xa
            if cin == 4:                                    # the slots the foreign residuals are copied into
                sh = rt._residual_shapes(2, H, W, with_up=True)
                assert [(b, c, h, w) for k in ("down", "mid", "up") for (b, c, h, w) in sh[k]] == [tuple(s) for s in gold["res_shapes"]]
            ups = [c[1][0]._obj for c in rt.step_plan.calls if c[1] and isinstance(getattr(c[1][0], "_obj", None), L.PPGemmArgs)
                   and c[1][0]._obj.up]
            assert [(a.hin, a.win, a.hout, a.wout) for a in ups] == [chain[i] + chain[i - 1] for i in (3, 2, 1)]
            assert all(a.stride == 1 and not a.subpix and a.M == 2 * a.hout * a.wout for a in ups)


def test_folded_cross_attention_operands_follow_the_step_geometry():
    """29x32 latents on the SD-1.5 architecture: 29 -> 15 -> 8 -> 4, so level 2 is 8x8 = 64 rows per item and its C = 1280
    transformers take the two-GEMM form (whole 64-row tiles) -- by `H >> level` it would be 7x8 = 56 and build_setup would fold
    nothing for a geometry build_step then meets.  Level 0 (928 rows, no multiple of 128) and level 1 (240) keep the chain,
    the mid block (4x4) as well: operands exist exactly where the step takes them, and the step plan builds."""
    rt = _runtime("unet", 9, 29, 32)
    assert level_sizes(29, 32, 4)[2] == (8, 8)
    assert sorted(rt.net.xa) == ["down_blocks.2.attentions.0", "down_blocks.2.attentions.1", "up_blocks.1.attentions.0",
                                 "up_blocks.1.attentions.1", "up_blocks.1.attentions.2"]
    assert all(v[4] == 2 for v in rt.net.xa.values())
    names = [c[2] for c in rt.step_plan.calls]
    assert names.count("xattn_block") == 0
    # a size accepted before: 32x32 folds the same five at level 2 (8x8) and the fused block elsewhere
    rt32 = _runtime("unet", 9, 32, 32)
    assert {k for k, v in rt32.net.xa.items() if v[4] == 2} == set(rt.net.xa)


def test_sub_pixel_upsamplers_only_for_exact_targets():
    """36x40 latents (36 -> 18 -> 9 -> 5, 40 -> 20 -> 10 -> 5): the upsampler 18x20 -> 36x40 is exact and wide enough for the
    sub-pixel form; 9x10 -> 18x20 is exact but below the routed width; 5x5 -> 9x10 is cropped."""
    lib = L.lib()
    rt = _runtime("unet", 9, 36, 40, B=8)
    assert level_sizes(36, 40, 4) == [(36, 40), (18, 20), (9, 10), (5, 5)]
    want = ["up_blocks.2.upsamplers.0.conv"] if lib.pp_upconv_subpix_supported(8, 18, 20, 640, 640, L.PP_DT_BF16) == 2 else []
    assert sorted(rt.net.upfold) == want
    gemms = [c[1][0]._obj for c in rt.step_plan.calls if c[1] and isinstance(getattr(c[1][0], "_obj", None), L.PPGemmArgs)]
    assert [(a.hin, a.win, a.hout, a.wout) for a in gemms if a.up] == [(5, 5, 9, 10), (9, 10, 18, 20)] + \
        ([] if want else [(18, 20, 36, 40)])
    assert len([a for a in gemms if a.subpix]) == len(want)


def _up_args(hin, win, hout, wout, c=64, B=2):
    a = L.conv3x3_args(L.PP_DT_BF16, B, hin, win, c, c, 0x1000, up=True, w=0x5000, out=0x6000)
    a.hout, a.wout, a.M, a.rows_per_batch = hout, wout, B * hout * wout, hout * wout
    return a


def test_up_target_contract_without_a_gpu():
    """PP_X_CONV3X3 with up = 1 (ABI v29): hout in {2 hin - 1, 2 hin}, wout likewise, the axes independent; anything else is
    PP_ERR_BAD_ARG before a launch is attempted (the pattern of test_bad_args_are_rejected_without_a_gpu).  A request that
    validates is not launched here: a forced split shows it through pp_gemm_workspace_bytes, which answers 0 for a request
    pp_gemm_bf16 would refuse."""
    lib = L.lib()
    assert lib.pp_abi_version() == 29
    for hout, wout in ((2 * 4 - 2, 6), (2 * 4 + 1, 6), (8, 2 * 3 - 2), (8, 2 * 3 + 1), (0, 6)):
        a = _up_args(4, 3, hout, wout)
        assert lib.pp_gemm_bf16(C.byref(a), None) == -1, (hout, wout)
        a.splitk = 2
        assert lib.pp_gemm_workspace_bytes(C.byref(a)) == 0
    for hout, wout in ((7, 5), (8, 5), (7, 6), (8, 6)):
        a = _up_args(4, 3, hout, wout)
        a.splitk = 2
        assert lib.pp_gemm_workspace_bytes(C.byref(a)) >= 2 * a.M * a.N * 4, (hout, wout)
    # without `up` the output size is the input's: the widened rule does not leak
    a = _up_args(4, 3, 7, 5)
    a.up = 0
    assert lib.pp_gemm_bf16(C.byref(a), None) == -1
    # the binding builds the cropped geometry and refuses targets that are no nearest-resize size
    a = L.conv3x3_args(L.PP_DT_BF16, 2, 7, 5, 64, 64, 0x1000, up=True, up_size=(13, 10), w=0x5000, out=0x6000)
    assert (a.hout, a.wout, a.M, a.rows_per_batch) == (13, 10, 260, 130)
    for bad in ((12, 10), (15, 10), (13, 8)):
        with pytest.raises(ValueError):
            L.conv3x3_args(L.PP_DT_BF16, 2, 7, 5, 64, 64, 0x1000, up=True, up_size=bad)
    with pytest.raises(ValueError):
        L.conv3x3_args(L.PP_DT_BF16, 2, 7, 5, 64, 64, 0x1000, up=False, up_size=(13, 10))


def test_halo_tile_loop_and_sub_pixel_form_decline_a_cropped_target():
    """Which kernel runs an `up` request is the library's answer: the halo-tile loop (pp_conv_gn_supported == 2) and the
    sub-pixel form take the exact 2x target only; a cropped one stays on the tap-major kernels."""
    lib = L.lib()
    exact = _up_args(16, 16, 32, 32, c=320, B=8)
    assert lib.pp_conv_gn_supported(C.byref(exact)) == 2
    for hout, wout in ((31, 32), (32, 31), (31, 31)):
        assert lib.pp_conv_gn_supported(C.byref(_up_args(16, 16, hout, wout, c=320, B=8))) == 0
    sup, to = lib.pp_upconv_subpix_supported, lib.pp_upconv_subpix_supported_to
    for (B, h, w, c) in ((8, 32, 32, 320), (8, 16, 16, 640), (8, 8, 8, 1280), (2, 7, 5, 320), (2, 18, 20, 640)):
        assert to(B, h, w, 2 * h, 2 * w, c, c, L.PP_DT_BF16) == sup(B, h, w, c, c, L.PP_DT_BF16)
        for hout, wout in ((2 * h - 1, 2 * w), (2 * h, 2 * w - 1), (2 * h - 1, 2 * w - 1)):
            assert to(B, h, w, hout, wout, c, c, L.PP_DT_BF16) == 0
    assert sup(8, 32, 32, 320, 320, L.PP_DT_BF16) == 2


def test_vae_plans_build_for_a_104x80_image():
    """13x10 = 130 tokens in the mid-block attention: the keys are padded to 192, P's row stride and V^T's as well."""
    from powerpaint_amd.vae import VAENet
    net = VAENet(block_out_channels=(64, 128, 256, 256), layers_per_block=1)
    net.load_state_dict(net.synthetic_state_dict(seed=1), "cpu")
    for direction in ("decode", "encode"):
        dry = Arena()
        pb = Builder(dry)
        if direction == "decode":
            shape = net.build_decode(pb, Act(dry.alloc(2 * 13 * 10 * 16), 2, 13, 10, 8), dry.alloc(2 * 4 * 104 * 80 * 4))
            assert shape == (2, 4, 104, 80)
        else:
            m = net.build_encode(pb, Act(dry.alloc(2 * 104 * 80 * 16), 2, 104, 80, 8))
            assert (m.B, m.H, m.W, m.C) == (2, 13, 10, 8)
        calls = pb.plan.calls
        sm = [c[1] for c in calls if c[2] == "softmax_rows"]
        assert len(sm) == 2 and all((a[1], a[2], a[3], a[6]) == (192, 130, 130, 192) for a in sm)
        tv = [c[1] for c in calls if c[2] == "transpose_v"]
        assert len(tv) == 1 and (tv[0][3], tv[0][6]) == (130, 192)
        qk = [c[1][0]._obj for c in calls if c[2] == "attn_qk"]
        pv = [c[1][0]._obj for c in calls if c[2] == "attn_pv"]
        assert all((a.M, a.N, a.K, a.ldo) == (130, 192, 256, 192) for a in qk)
        assert all((a.M, a.N, a.K, a.ldx1) == (130, 256, 192, 192) for a in pv)
    # a token count on the grid: the plan that always was (no padding)
    dry = Arena()
    pb = Builder(dry)
    net.build_decode(pb, Act(dry.alloc(16 * 16 * 16), 1, 16, 16, 8), dry.alloc(4 * 128 * 128 * 4))
    sm = [c[1] for c in pb.plan.calls if c[2] == "softmax_rows"]
    assert [(a[1], a[2], a[3], a[6]) for a in sm] == [(256, 256, 256, 256)]


def test_controller_sizes_that_used_to_be_refused():
    """What the demo path produces: fit_short_side to 640 then snap_to_eight -- a 4:3 photo is 848x640 (106x80 latents), a
    16:9 one 1136x640 (142x80).  The UNet plans build at both."""
    for H, W in ((106, 80), (142, 80)):
        rt = _runtime("unet", 9, H, W)
        assert rt.step_plan.calls and (rt.H, rt.W) == (H, W)


def _reference_tree():
    from oracle import ref_shim
    return os.path.isdir(ref_shim.REF_ROOT)


@pytest.mark.skipif(not _reference_tree(), reason="the reference sources are not here (the fixture travels without them)")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    """The generator runs in a process of its own: oracle/ref_shim.py installs a `diffusers` stand-in for the reference's model
    files, which must not reach the other tests' imports."""
    import subprocess
    out = str(tmp_path / "ref_any_size.pt")
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_ref_any_size.py"), out], check=True,
                   capture_output=True, timeout=600)
    new = torch.load(out, weights_only=False)
    assert sorted(new["nets"]) == sorted(GOLD["nets"]) and sorted(new["calls"]) == sorted(GOLD["calls"])
    for k, g in GOLD["nets"].items():
        for name, v in g.items():
            if torch.is_tensor(v):
                assert torch.allclose(new["nets"][k][name], v, atol=2e-4, rtol=1e-4), (k, name)
            else:
                assert new["nets"][k][name] == v, (k, name)
    for k, v in GOLD["calls"].items():        # (four CFG-7.5 steps on latents of magnitude ~17)
        assert torch.allclose(new["calls"][k], v, atol=2e-3, rtol=1e-4), k
