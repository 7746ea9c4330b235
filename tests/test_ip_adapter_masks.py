"""CPU: IP-Adapter masks -- IPAdapterMaskProcessor against the restated rule, the argument checks of the UNet and of the three
pipelines, the launch plans with and without masks, the ABI of pp_ip_attn_add_masked, and the oracle loop against the fixture."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ip_adapter_cases as IC  # noqa: E402
import ip_mask_cases as MC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ip_adapter as IPA  # noqa: E402
from powerpaint_amd.pipelines.image_processor import IPAdapterMaskProcessor, VaeImageProcessor  # noqa: E402
from test_ip_adapter import TINY, _adapter, _describe, _hip_unet, _net, _pipe  # noqa: E402

GOLD_PATH = os.path.join(HERE, "golden", "ref_ip_adapter_masks.pt")


def _rect(h, w):
    return MC.rect_mask(h, w, h // 8, w // 4, 5 * h // 8, 7 * w // 8)


# ------------------------------------------------------------------------------------------------------------ processor
@pytest.mark.parametrize("hw,queries", [((128, 128), (256, 64)), ((144, 96), (216, 54)), ((136, 104), (221, 63)),
                                        ((128, 64), (256, 64))])
def test_downsample_is_the_restated_rule(hw, queries):
    m = _rect(*hw)
    for nq in queries:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = IPAdapterMaskProcessor.downsample(m, 2, nq, 3)
            want = MC.downsample(m, 2, nq, 3)
        assert got.shape == (2, nq, 3) and got.dtype == torch.float32
        assert torch.equal(got, want)
        assert torch.equal(got[0], got[1]) and torch.equal(got[..., 0], got[..., 2])        # shared by batch and channels
        # the rows away from the rectangle's edges are EXACT zeros
        assert float((got[0, :, 0] == 0).float().mean()) > 0.3
    if hw == (128, 128):
        # bicubic is not clamped: edges that fall between the taps of a sample ring below 0 and above 1 (taps -0.09375)
        w = IPAdapterMaskProcessor.downsample(MC.rect_mask(128, 128, 21, 21, 85, 85), 1, 256, 1)
        assert -0.12 < float(w.min()) < -0.09 and 1.09 < float(w.max()) < 1.2
    if hw == (128, 64):
        # the off-aspect mask: a (23, 11) grid for 256 queries, 253 values and 3 pad zeros at the end
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            w = IPAdapterMaskProcessor.downsample(torch.ones(1, 128, 64), 1, 256, 1).reshape(-1)
        assert bool((w[:253] != 0).all()) and bool((w[253:] == 0).all())


def test_downsample_pads_with_a_warning_and_never_cuts():
    """The warning is asserted on the padding case.  The rule's cutting branch (area > num_queries) cannot be reached through
    the rule itself: mask_w = num_queries // mask_h, so area = mask_h * (num_queries // mask_h) <= num_queries for every mask
    and query count -- there is no truncating case to add to the table; a sweep asserts exactly that."""
    m = torch.ones(1, 128, 64)
    with pytest.warns(UserWarning, match="aspect ratio"):
        got = IPAdapterMaskProcessor.downsample(m, 1, 256, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert torch.equal(got, MC.downsample(m, 1, 256, 1))
        for hw in ((8, 24), (24, 8), (16, 16), (10, 14)):
            for nq in range(4, 80):
                w = IPAdapterMaskProcessor.downsample(torch.ones(1, *hw), 1, nq, 1).reshape(-1)
                assert w.shape == (nq,) and torch.equal(w, MC.downsample(torch.ones(1, *hw), 1, nq, 1).reshape(-1))
                live = int((w != 0).sum())
                assert live <= nq and bool((w[live:] == 0).all())                      # values, then pad zeros; nothing cut
    m2 = _rect(64, 96)
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # an exact grid warns about nothing
        a = IPAdapterMaskProcessor.downsample(m2, 1, 96, 2)
    assert a.shape == (1, 96, 2) and torch.equal(a, MC.downsample(m2, 1, 96, 2))
    with pytest.raises(ValueError, match="grid"):
        IPAdapterMaskProcessor.downsample(torch.ones(1, 8, 64), 1, 1, 1)


def test_preprocess_binarises_converts_to_grey_and_resizes():
    import PIL.Image
    p = IPAdapterMaskProcessor()
    assert isinstance(p, VaeImageProcessor)
    assert (p.config.do_normalize, p.config.do_binarize, p.config.do_convert_grayscale, p.config.resample) == \
        (False, True, True, "lanczos")
    rgb = np.zeros((40, 48, 3), dtype=np.uint8)
    rgb[8:30, 10:40] = (250, 240, 255)
    rgb[0:4, 0:4] = (90, 90, 90)                 # grey below one half: binarised away
    imgs = [PIL.Image.fromarray(rgb), PIL.Image.fromarray(255 - rgb)]
    out = p.preprocess(imgs, height=32, width=24)
    assert out.shape == (2, 1, 32, 24) and out.dtype == torch.float32
    assert set(out.unique().tolist()) == {0.0, 1.0}
    assert out[0, 0, 16, 12] == 1.0 and out[0, 0, 1, 1] == 0.0 and out[1, 0, 16, 12] == 0.0 and out[1, 0, 1, 1] == 1.0
    soft = torch.tensor([0.2, 0.7, 0.5, 0.49]).repeat(16).reshape(1, 8, 8)                 # [n, H, W] tensor masks
    t = p.preprocess(soft)
    assert t.shape == (1, 1, 8, 8) and t.flatten().tolist() == [0.0, 1.0, 1.0, 0.0] * 16
    assert p.preprocess(imgs[0]).shape == (1, 1, 40, 48)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_unet_mask_checks_in_order():
    u = _hip_unet(**TINY)
    good = torch.ones(1, 1, 64, 64)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        u._check_ip_masks(good)
    assert u._check_ip_masks(None) is None
    u._load_ip_adapter_weights([_adapter(u.net, seed=1), _adapter(u.net, seed=2)])
    for bad in (torch.ones(2, 64, 64), [torch.ones(1, 64, 64)] * 2, torch.ones(2, 1, 64, 64, dtype=torch.int64),
                torch.ones(3, 64, 64) * float("nan")):                                     # (rank before anything else)
        with pytest.raises(ValueError, match="IPAdapterMaskProcessor"):
            u._check_ip_masks(bad)
    with pytest.raises(ValueError, match="one mask per adapter"):
        u._check_ip_masks(torch.ones(3, 2, 64, 64))                                        # (second dimension before the count)
    with pytest.raises(ValueError, match=r"Number of ip_adapter_masks \(1\).*\(2\)"):
        u._check_ip_masks(torch.full((1, 1, 64, 64), float("inf")))                        # (count before finiteness)
    with pytest.raises(ValueError, match="non-finite"):
        u._check_ip_masks(torch.full((2, 1, 64, 64), float("nan")))
    two = torch.ones(2, 1, 64, 48)
    assert u._check_ip_masks(two) is two
    # forward / prepare read cross_attention_kwargs["ip_adapter_masks"]: a bad one is refused before any plan is built
    x, ehs = torch.zeros(2, 4, 8, 8), torch.zeros(2, 77, 768)
    with pytest.raises(ValueError, match="Number of ip_adapter_masks"):
        u(x, 1, ehs, cross_attention_kwargs={"ip_adapter_masks": good},
          added_cond_kwargs={"image_embeds": [torch.zeros(2, 1, 32)] * 2})
    with pytest.raises(ValueError, match="Number of ip_adapter_masks"):
        u.prepare((2, 4, 8, 8), ehs, ip_adapter_masks=good)
    u._unload_ip_adapter()
    with pytest.raises(ValueError, match="load_ip_adapter"):
        u(x, 1, ehs, cross_attention_kwargs={"ip_adapter_masks": good})


def test_pipelines_refuse_or_take_the_key():
    from powerpaint_amd import pipelines as PP
    m = torch.ones(1, 1, 64, 64)
    for cls in (PP.StableDiffusionInpaintPipeline, PP.StableDiffusionControlNetInpaintPipeline):
        with pytest.raises(ValueError, match="ip_adapter_masks.*never applies"):
            cls()(promptA="a", cross_attention_kwargs={"ip_adapter_masks": m})
    u = _hip_unet(**TINY)
    p = _pipe(u)
    e = [torch.zeros(2, 1, 32)]
    with pytest.raises(ValueError, match="load_ip_adapter"):                   # no adapter: refused, never dropped
        p(promptA="a", ip_adapter_image_embeds=e, cross_attention_kwargs={"ip_adapter_masks": m})
    p.load_ip_adapter(_adapter(u.net))
    with pytest.raises(ValueError, match="IPAdapterMaskProcessor"):
        p(promptA="a", ip_adapter_image_embeds=e, cross_attention_kwargs={"ip_adapter_masks": m[0]})
    with pytest.raises(ValueError, match="Number of ip_adapter_masks"):
        p(promptA="a", ip_adapter_image_embeds=e, cross_attention_kwargs={"ip_adapter_masks": torch.cat([m, m])})
    with pytest.raises(ValueError, match="ip_adapter_image"):
        p(promptA="a", cross_attention_kwargs={"ip_adapter_masks": m})
    # load_ip_adapter never took masks: its refusal points at the call
    with pytest.raises(L.PPError, match="ip_adapter_masks.*cross_attention_kwargs"):
        p.load_ip_adapter(_adapter(u.net), ip_adapter_masks=[m])


# ------------------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("n_adapters,images", [(1, [1]), (2, [1, 2])])
def test_plan_with_masks(n_adapters, images):
    from powerpaint_amd.runtime import NetRuntime
    lib = L.lib()
    net, never = _net(**TINY), _net(**TINY)
    ads = [IPA.check_ip_adapter(net, _adapter(net, seed=i)) for i in range(n_adapters)]
    net.set_ip_adapters(ads)
    never.set_ip_adapters([IPA.check_ip_adapter(never, _adapter(never, seed=i)) for i in range(n_adapters)])
    rt, rt0 = NetRuntime(net, "cpu"), NetRuntime(never, "cpu")
    B, H, W = 2, 18, 12                                      # levels 18x12 and 9x6
    rt0.ensure(B, H, W, 77, 4, ("plain",), ip_n=images)
    rt.ensure(B, H, W, 77, 4, ("plain",), ip_n=images, ip_masked=True)
    assert rt.key != rt0.key
    calls = [c for c in rt.step_plan.calls if c[2] == "ip_attn_add"]
    plain = [c for c in rt0.step_plan.calls if c[2] == "ip_attn_add"]
    assert len(calls) == len(plain) == 4 * n_adapters
    # every record is the masked entry, with the weight buffer of (its level's query count, its adapter); the transformers
    # of a level share the buffer; the rest of the record is the unmasked record's
    bufs = rt.lay["ip_row_w"]
    assert sorted(bufs) == [54, 216] and all(len(v) == n_adapters for v in bufs.values())
    assert len({p for v in bufs.values() for p in v}) == 2 * n_adapters
    for k, (c, c0) in enumerate(zip(calls, plain)):
        assert c[0] is lib.pp_ip_attn_add_masked and c0[0] is lib.pp_ip_attn_add
        nq = c[1][8]
        assert c[1][13] == bufs[nq][k % n_adapters] and c[1][13] % 4 == 0
        assert c[1][12] is rt._ip_scale_cells[k % n_adapters]
        assert c[1][5:12] == c0[1][5:12] and c[1][14] == c0[1][13] and len(c[1]) == len(c0[1]) + 1
    assert [c[2] for c in rt.step_plan.calls] == [c[2] for c in rt0.step_plan.calls]
    assert rt.step_plan.flops == rt0.step_plan.flops
    assert rt.arena.size >= rt0.arena.size
    # without masks: the plan of a net that never saw one; given and then dropped: that plan again
    want = (_describe(rt0.step_plan), _describe(rt0.setup_plan), rt0.arena.size, rt0.key)
    rt.ensure(B, H, W, 77, 4, ("plain",), ip_n=images)
    assert "ip_row_w" not in rt.lay and not net.ip_row_w
    assert (_describe(rt.step_plan), _describe(rt.setup_plan), rt.arena.size, rt.key) == want
    assert all(c[0] is lib.pp_ip_attn_add for c in rt.step_plan.calls if c[2] == "ip_attn_add")
    assert [c[1][5:12] + c[1][13:] for c in rt.step_plan.calls if c[2] == "ip_attn_add"] == [c[1][5:12] + c[1][13:] for c in plain]
    # masks need an adapter
    net.set_ip_adapters([])
    with pytest.raises(L.PPError, match="IP-Adapter"):
        NetRuntime(net, "cpu").ensure(B, H, W, 77, 4, ("plain",), ip_masked=True)


def test_set_ip_masks_fills_the_buffers_with_the_processors_rule():
    """The runtime's weights ARE IPAdapterMaskProcessor.downsample(mask_i, 1, nq, 1), per adapter and level; new masks of the
    same count rewrite them in place (same plan, same arena)."""
    from powerpaint_amd.runtime import NetRuntime
    net = _net(**TINY)
    net.set_ip_adapters([IPA.check_ip_adapter(net, _adapter(net, seed=i)) for i in range(2)])
    rt = NetRuntime(net, "cpu")
    rt.ensure(2, 16, 16, 77, 4, ("plain",), ip_n=[1, 1], ip_masked=True)
    plan, arena = rt.step_plan, rt.arena
    for masks in (MC.case_masks("two"), torch.stack([_rect(128, 64), 1.0 - _rect(128, 64)])):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rt.set_ip_masks(masks)
            for nq, ptrs in rt.lay["ip_row_w"].items():
                for i, ptr in enumerate(ptrs):
                    got = rt.arena.view(ptr, (nq,), torch.float32)
                    assert torch.equal(got, MC.downsample(masks[i], 1, nq, 1).reshape(nq))
        rt.ensure(2, 16, 16, 77, 4, ("plain",), ip_n=[1, 1], ip_masked=True)
        assert rt.step_plan is plan and rt.arena is arena
    with pytest.raises(ValueError, match="Number of ip_adapter_masks"):
        rt.set_ip_masks(MC.case_masks("one"))


# ------------------------------------------------------------------------------------------------------------ ABI
def test_abi_of_pp_ip_attn_add_masked():
    import ctypes
    lib = L.lib()
    assert lib.pp_abi_version() == 29 and L.ABI_VERSION == 29
    assert "pp_ip_attn_add_masked" in L.SIGNATURES and hasattr(ctypes.CDLL(L.LIB_PATH), "pp_ip_attn_add_masked")
    q, k, v, o, w = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000           # (never dereferenced: every call is refused)

    def call(q_=q, ldq=320, k_=k, v_=v, o_=o, ldo=320, batch=2, heads=8, nq=64, nk=4, d=40, scale=1.0, w_=w, dtype=L.PP_DT_BF16):
        return lib.pp_ip_attn_add_masked(q_, ldq, k_, v_, o_, ldo, batch, heads, nq, nk, d, d ** -0.5, scale, w_, dtype, None)

    bad, unsup = -1, -2
    assert call(w_=None) == bad and call(w_=w + 2) == bad and call(w_=w + 1) == bad
    assert call(scale=float("nan")) == bad
    # the limits of the unmasked entry
    assert call(q_=None) == bad and call(k_=None) == bad and call(v_=None) == bad and call(o_=None) == bad
    assert call(d=24) == unsup and call(d=44) == bad
    assert call(nk=0) == bad and call(nk=L.PP_IP_MAX_TOKENS + 1) == unsup
    assert call(heads=128, ldq=128 * 40, ldo=128 * 40) == unsup and call(batch=65536) == unsup
    assert call(ldq=319) == bad and call(ldo=312) == bad and call(ldo=324) == bad
    assert call(q_=q + 2) == bad and call(o_=o + 8) == bad and call(o_=q) == bad
    assert call(dtype=L.PP_DT_F32) == bad and call(batch=0) == bad and call(nq=0) == bad
    # ip_scale == 0 launches nothing: PP_OK with pointers no kernel could follow, and no GPU
    assert call(scale=0.0) == 0
    # a NULL weight pointer is refused even then (the argument check comes first)
    assert call(scale=0.0, w_=None) == bad


# ------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_discriminates_and_is_small():
    G = torch.load(GOLD_PATH, weights_only=False)
    assert os.path.getsize(GOLD_PATH) < 110 * 1024
    assert set(G) == {"one", "two", "one_b"}
    for name, e in G.items():
        assert set(e) == {"latents", "unmasked", "next_draw"}
        assert e["latents"].shape == (2, 4, 16, 16) and e["latents"].dtype == torch.float32
        cos, err, ok = IC.loop_gate(e["unmasked"], e["latents"])
        assert not ok, (name, cos, err)                     # dropped masks cannot pass
    assert not IC.loop_gate(G["one_b"]["latents"], G["one"]["latents"])[2]
    # the unmasked latents are those of the same call in ref_ip_adapter.pt (same adapters, embeds, seed)
    P = torch.load(os.path.join(HERE, "golden", "ref_ip_adapter.pt"), weights_only=False)
    for name in ("one", "two"):
        assert torch.allclose(G[name]["unmasked"], P[name]["latents"], atol=IC.ATOL, rtol=IC.RTOL)


@pytest.mark.parametrize("name", ["one", "two", "one_b"])
def test_oracle_loop_with_masked_ip_attention_reproduces_the_fixture(name):
    import make_ref_ip_adapter_masks as MM
    G = torch.load(GOLD_PATH, weights_only=False)[name]
    out, nxt = MM.oracle_run(name)
    err = (out - G["latents"]).abs()
    assert bool((err <= IC.ATOL + IC.RTOL * G["latents"].abs()).all()), float(err.max())
    assert torch.equal(nxt, G["next_draw"])


def test_masked_attention_with_all_ones_weights_is_the_unmasked_module():
    """The restated module: a mask of ones at the latents' aspect gives weights of exactly 1 and IC.IPAttention's output."""
    from oracle import sd_modules as OM
    torch.manual_seed(3)
    o = OM.UNet2DConditionModel(in_channels=4, **TINY).eval()
    sds = [IC.adapter_state_dict(o, 50)]
    ipu = MC.MaskedIPUNet(o, sds, [0.8]).eval()
    g = torch.Generator().manual_seed(0)
    x, ehs, t = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 77, 768, generator=g), torch.tensor(500)
    e = {"image_embeds": [torch.randn(2, 1, IC.EMBED_DIM, generator=g)]}
    with torch.no_grad():
        plain = ipu(x, t, ehs, added_cond_kwargs=e)[0]
        ones = ipu(x, t, ehs, added_cond_kwargs=e, cross_attention_kwargs={"ip_adapter_masks": torch.ones(1, 1, 64, 64)})[0]
        half = ipu(x, t, ehs, added_cond_kwargs=e, cross_attention_kwargs={"ip_adapter_masks": MC.case_masks("one")})[0]
    assert torch.allclose(ones, plain, atol=1e-5, rtol=1e-5) and not torch.allclose(half, plain, atol=1e-2)
    with pytest.raises(ValueError, match="Number of ip_adapter_masks"):
        ipu(x, t, ehs, added_cond_kwargs=e, cross_attention_kwargs={"ip_adapter_masks": torch.ones(2, 1, 64, 64)})
    with pytest.raises(ValueError, match="IPAdapterMaskProcessor"):
        ipu(x, t, ehs, added_cond_kwargs=e, cross_attention_kwargs={"ip_adapter_masks": torch.ones(1, 64, 64)})
