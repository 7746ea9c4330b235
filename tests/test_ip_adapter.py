"""CPU: IP-Adapter -- the loader (file forms, index order, refusals), the model / pipeline state, the launch plans with and
without adapters, the pipeline's argument checks, the oracle loop against the fixture, and the ABI of pp_ip_attn_add."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ip_adapter_cases as IC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ip_adapter as IPA  # noqa: E402

GOLD_PATH = os.path.join(HERE, "golden", "ref_ip_adapter.pt")
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))


def _net(**kw):
    from powerpaint_amd.engine import SDNet
    net = SDNet("unet", 4, **kw)
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    return net


def _adapter(net, T=4, D=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    width = dict(net._attn_specs())
    ad = {}
    for k, pre in enumerate(net.ip_attn_order()):
        for n in ("to_k_ip", "to_v_ip"):
            ad[f"{2 * k + 1}.{n}.weight"] = torch.randn(width[pre], 768, generator=g)
    ip = {"proj.weight": torch.randn(T * 768, D, generator=g), "proj.bias": torch.randn(T * 768, generator=g),
          "norm.weight": torch.randn(768, generator=g), "norm.bias": torch.randn(768, generator=g)}
    return {"image_proj": ip, "ip_adapter": ad}


def _hip_unet(**cfg):
    """A HIP UNet whose packed buffer lives on the CPU (no launch ever runs in this file)."""
    from powerpaint_amd.models import UNet2DConditionModel as U
    u = U(in_channels=4, device="cpu", **cfg)
    return u.load_state_dict(u.net.synthetic_state_dict(meta=True), materialize=False)


# ------------------------------------------------------------------------------------------------------------ loader
def test_index_order_is_down_up_mid():
    net = _net()
    order = net.ip_attn_order()
    assert len(order) == 16 and order[:6] == [f"down_blocks.{i}.attentions.{j}" for i in range(3) for j in range(2)]
    assert order[6:15] == [f"up_blocks.{i}.attentions.{j}" for i in (1, 2, 3) for j in range(3)]
    assert order[15] == "mid_block.attentions.0"
    assert sorted(order) == sorted(p for p, _ in net._attn_specs()) and order != [p for p, _ in net._attn_specs()]
    sd = _adapter(net)
    ad = IPA.check_ip_adapter(net, sd)
    # index 2 k + 1 lands on the k-th transformer of that order: 13 is the FIRST up-block attention, 31 the mid block
    assert torch.equal(ad["kv"]["up_blocks.1.attentions.0"][0], sd["ip_adapter"]["13.to_k_ip.weight"])
    assert torch.equal(ad["kv"]["mid_block.attentions.0"][1], sd["ip_adapter"]["31.to_v_ip.weight"])
    assert (ad["T"], ad["D"]) == (4, 32)
    assert IPA.check_ip_adapter(net, _adapter(net, T=8, D=64))["T"] == 8          # T from the shapes


def test_file_forms_round_trip(tmp_path):
    net = _net(**{k: v for k, v in TINY.items()})
    sd = _adapter(net)
    torch.save(sd, tmp_path / "ip.bin")
    flat = {f"{a}.{k}": v for a in sd for k, v in sd[a].items()}
    from safetensors.torch import save_file
    save_file(flat, str(tmp_path / "ip.safetensors"))
    forms = [sd, str(tmp_path / "ip.bin"), str(tmp_path / "ip.safetensors"), flat]
    for f in forms:
        got = IPA.read_ip_adapter(f)
        assert set(got) == {"image_proj", "ip_adapter"}
        for a in sd:
            assert set(got[a]) == set(sd[a]) and all(torch.equal(got[a][k], sd[a][k]) for k in sd[a])
    got = IPA.read_ip_adapter(str(tmp_path), subfolder="", weight_name="ip.safetensors")
    assert torch.equal(got["image_proj"]["proj.bias"], sd["image_proj"]["proj.bias"])
    with pytest.raises(L.PPError, match="does not exist"):
        IPA.read_ip_adapter(str(tmp_path / "missing.bin"))
    with pytest.raises(L.PPError, match="weight_name"):
        IPA.read_ip_adapter(str(tmp_path))
    with pytest.raises(L.PPError, match="other.key"):
        IPA.read_ip_adapter(dict(flat, **{"other.key": torch.zeros(1)}))


@pytest.mark.parametrize("where,key,value,match", [
    ("image_proj", "latents", torch.zeros(1, 16, 768), "latents.*Plus"),
    ("image_proj", "proj_in.weight", torch.zeros(768, 1280), "proj_in.weight.*Plus"),
    ("image_proj", "layers.0.0.to_q.weight", torch.zeros(8, 8), "layers.0.0.to_q.weight.*Plus"),
    ("image_proj", "proj.0.weight", torch.zeros(8, 8), "proj.0.weight.*FaceID"),
    ("ip_adapter", "1.to_k_lora.down.weight", torch.zeros(8, 8), "1.to_k_lora.down.weight.*FaceID"),
    ("image_proj", "extra.weight", torch.zeros(8), "extra.weight"),
    ("ip_adapter", "33.to_k_ip.weight", torch.zeros(320, 768), "33.to_k_ip.weight"),
    ("ip_adapter", "2.to_k_ip.weight", torch.zeros(320, 768), "2.to_k_ip.weight"),
])
def test_refused_families_are_named(where, key, value, match):
    net = _net()
    sd = _adapter(net)
    sd[where][key] = value
    with pytest.raises(L.PPError, match=match):
        IPA.check_ip_adapter(net, sd)


def test_wrong_shapes_and_missing_indices_are_named():
    net = _net()
    sd = _adapter(net)
    del sd["ip_adapter"]["13.to_v_ip.weight"]
    with pytest.raises(L.PPError, match="13.to_v_ip.weight"):
        IPA.check_ip_adapter(net, sd)
    sd = _adapter(net)
    sd["ip_adapter"]["1.to_k_ip.weight"] = torch.zeros(640, 768)
    with pytest.raises(L.PPError, match=r"1.to_k_ip.weight.*\(320, 768\)"):
        IPA.check_ip_adapter(net, sd)
    sd = _adapter(net)
    sd["image_proj"]["proj.weight"] = torch.zeros(4 * 768 + 1, 32)
    with pytest.raises(L.PPError, match="proj.weight"):
        IPA.check_ip_adapter(net, sd)
    sd = _adapter(net)
    sd["image_proj"]["norm.bias"] = torch.zeros(767)
    with pytest.raises(L.PPError, match="norm.bias"):
        IPA.check_ip_adapter(net, sd)
    sd = _adapter(net)
    del sd["image_proj"]["proj.bias"]
    with pytest.raises(L.PPError, match="proj.bias"):
        IPA.check_ip_adapter(net, sd)
    sd = _adapter(net, T=L.PP_IP_MAX_TOKENS + 1, D=8)
    with pytest.raises(L.PPError, match="tokens"):
        IPA.check_ip_adapter(net, sd)


# ------------------------------------------------------------------------------------------------------------ state
def test_model_state_after_load_and_unload_and_failed_load():
    u = _hip_unet(**TINY)
    before = (u.config.encoder_hid_dim_type, u.encoder_hid_proj, u.net.params.total, sorted(u.net.P))
    assert before[:2] == (None, None)
    sds = [_adapter(u.net, seed=1), _adapter(u.net, T=8, D=64, seed=2)]
    u._load_ip_adapter_weights(sds)
    assert u.config.encoder_hid_dim_type == "ip_image_proj"
    layers = u.encoder_hid_proj.image_projection_layers
    assert len(layers) == 2 and all(isinstance(m, IPA.ImageProjection) for m in layers)
    for m, sd in zip(layers, sds):
        ip = sd["image_proj"]
        assert torch.equal(m.image_embeds.weight, ip["proj.weight"]) and torch.equal(m.image_embeds.bias, ip["proj.bias"])
        assert torch.equal(m.norm.weight, ip["norm.weight"]) and torch.equal(m.norm.bias, ip["norm.bias"])
        assert m.num_image_text_embeds == ip["proj.weight"].shape[0] // 768
    assert u.net.ip == [(4, 32), (8, 64)]
    # packed: [to_k_ip; to_v_ip] per transformer, the projection zero-padded to 64 columns; in the ONE parameter buffer
    P = u.net.params
    kv = P.tensor("ip_adapter.1.mid_block.attentions.0.kv.weight")
    assert kv.shape == (1280, 768) and kv.dtype == torch.bfloat16
    assert torch.equal(kv[:640].float(), sds[1]["ip_adapter"]["7.to_k_ip.weight"].to(torch.bfloat16).float())
    assert torch.equal(kv[640:].float(), sds[1]["ip_adapter"]["7.to_v_ip.weight"].to(torch.bfloat16).float())
    pw = P.tensor("ip_adapter.0.proj.weight")
    assert pw.shape == (4 * 768, 64) and bool((pw[:, 32:] == 0).all())
    lo, hi = u.param_buffer().data_ptr(), u.param_buffer().data_ptr() + u.param_buffer().numel()
    assert all(lo <= p < hi for p in u.net.P.values())
    # not LoRA targets; a refused dtype still refuses
    from powerpaint_amd.lora import unet_targets
    assert not any("ip" in m.split(".")[0] or "_ip" in m for m in unet_targets(u.net))
    assert not any(r.name.startswith("ip_adapter") for r in u.net.pack_table() if hasattr(r, "rows"))
    with pytest.raises(L.PPError):
        u.to(torch.float16)
    # a failed load (second adapter is a Plus file) leaves the loaded state exactly as it was
    ver, ptrs = P.version, dict(u.net.P)
    bad = _adapter(u.net, seed=3)
    bad["image_proj"]["latents"] = torch.zeros(1, 16, 768)
    with pytest.raises(L.PPError, match="latents"):
        u._load_ip_adapter_weights([_adapter(u.net, seed=4), bad])
    assert (P.version, dict(u.net.P), u.net.ip) == (ver, ptrs, [(4, 32), (8, 64)]) and u.encoder_hid_proj.image_projection_layers is layers
    u._unload_ip_adapter()
    assert (u.config.encoder_hid_dim_type, u.encoder_hid_proj, u.net.params.total, sorted(u.net.P)) == before
    assert u.net.ip == []
    with pytest.raises(L.PPError, match="no IP-Adapter"):
        u.set_ip_adapter_scale(0.5)
    # a failed FIRST load leaves nothing behind either
    with pytest.raises(L.PPError):
        u._load_ip_adapter_weights(bad)
    assert (u.config.encoder_hid_dim_type, u.encoder_hid_proj, u.net.params.total, sorted(u.net.P)) == before


def test_projection_module_is_the_multi_adapter_projection():
    u = _hip_unet(**TINY)
    sds = [_adapter(u.net, seed=1), _adapter(u.net, T=8, D=64, seed=2)]
    u._load_ip_adapter_weights(sds)
    proj, _ = IC.load_into_oracle(__import__("oracle.sd_modules", fromlist=["x"]).UNet2DConditionModel(in_channels=4, **TINY), sds, [1, 1])
    g = torch.Generator().manual_seed(0)
    embeds = [torch.randn(2, 1, 32, generator=g), torch.randn(2, 2, 64, generator=g)]
    with torch.no_grad():
        a, b = u.encoder_hid_proj(embeds), proj(embeds)
    assert [tuple(t.shape) for t in a] == [(2, 4, 768), (2, 16, 768)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="same length"):
        u.encoder_hid_proj(embeds[:1])


def test_any_size_forward_restatement_is_the_oracle_forward_at_even_sizes():
    from oracle import sd_modules as OM
    torch.manual_seed(3)
    o = OM.UNet2DConditionModel(in_channels=4, **TINY).eval()
    g = torch.Generator().manual_seed(0)
    x, ehs, t = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 77, 768, generator=g), torch.tensor(500)
    with torch.no_grad():
        assert torch.equal(IC.forward_any_size(o, x, t, ehs)[0], o(x, t, ehs)[0])
        assert IC.forward_any_size(o, torch.randn(1, 4, 5, 6, generator=g), t, ehs)[0].shape == (1, 4, 5, 6)


# ------------------------------------------------------------------------------------------------------------ plans
def _describe(plan):
    return [plan.describe(i) for i in range(len(plan.calls))]


def test_plans_without_an_adapter_are_the_parents():
    """A net that loaded and unloaded an adapter compiles the plans of a net that never saw one, launch for launch (and so
    does the benchmark's program, which never loads one)."""
    from powerpaint_amd.runtime import NetRuntime
    never, was = _net(), _net()
    was.set_ip_adapters([IPA.check_ip_adapter(was, _adapter(was))])
    rt_w = NetRuntime(was, "cpu")
    rt_w.ensure(2, 64, 64, 77, 4, ("plain",), twin=True, ip_n=[1])
    assert "ip_attn_add" in [c[2] for c in rt_w.step_plan.calls]
    was.set_ip_adapters([])
    rt_n, rt_w = NetRuntime(never, "cpu"), NetRuntime(was, "cpu")
    for rt in (rt_n, rt_w):
        rt.ensure(2, 64, 64, 77, 4, ("plain",), twin=True)
    assert rt_n.key == rt_w.key
    assert _describe(rt_n.step_plan) == _describe(rt_w.step_plan) and _describe(rt_n.setup_plan) == _describe(rt_w.setup_plan)
    assert rt_n.step_plan.flops == rt_w.step_plan.flops and rt_n.arena.size == rt_w.arena.size
    names = [c[2] for c in rt_w.step_plan.calls]
    assert "ip_attn_add" not in names and "xattn_block" in names
    assert was.params.total == never.params.total and sorted(was.P) == sorted(never.P)


@pytest.mark.parametrize("n_adapters,images", [(1, [1]), (2, [1, 2])])
def test_plan_with_adapters(n_adapters, images):
    from powerpaint_amd.runtime import NetRuntime
    net, plain = _net(), _net()
    net.set_ip_adapters([IPA.check_ip_adapter(net, _adapter(net, seed=i)) for i in range(n_adapters)])
    rt, rt0 = NetRuntime(net, "cpu"), NetRuntime(plain, "cpu")
    B, hw = 2, 64
    rt.ensure(B, hw, hw, 77, 4, ("plain",), twin=True, ip_n=images)
    rt0.ensure(B, hw, hw, 77, 4, ("plain",), twin=True)
    calls = rt.step_plan.calls
    names = [c[2] for c in calls]
    assert names.count("ip_attn_add") == 16 * n_adapters
    assert "xattn_block" not in names and "xattn_fold" not in [c[2] for c in rt.setup_plan.calls]
    assert not rt.net.twin_prefix_ok(rt.lib, B, hw, hw, 77)                  # (the twin prefix is refused, as pad_uncond does)
    assert names.count("attention") == 32                                    # every attn2 on the generic chain
    # every launch sits between its attention and to_out, on the attention's output, with the adapter's token count
    ip_calls = [c for c in calls if c[2] == "ip_attn_add"]
    for k, c in enumerate(ip_calls):
        i = calls.index(c)
        prev = calls[i - 1 - k % n_adapters]
        assert prev[2] == "attention" and prev[1][6] == c[1][4]              # (attention's `out` is the launch's `o`)
        assert c[1][9] == 4 * images[k % n_adapters] and c[1][12] is rt._ip_scale_cells[k % n_adapters]
    # FLOPs: 4 * rows * T * C per launch
    want = 0.0
    sizes = {"down_blocks.0": 64, "down_blocks.1": 32, "down_blocks.2": 16, "mid_block": 8, "up_blocks.1": 16, "up_blocks.2": 32,
             "up_blocks.3": 64}
    for pre, c in net._attn_specs():
        s = sizes[pre.split(".attentions")[0]]
        want += sum(4.0 * B * s * s * 4 * n * c for n in images)
    assert rt.step_plan.flops_by_kind["ip_attn_add"] == want
    # scales: by-value cells shared by the adapter's launches; changing one drops the runtime's graph
    rt.graph = "captured"
    rt.set_ip_scales([0.25] * n_adapters)
    assert rt.graph is None and rt.ip_scales() == (0.25,) * n_adapters and ip_calls[0][1][12].value == 0.25
    rt.graph = "captured"
    rt.set_ip_scales([0.25] * n_adapters)
    assert rt.graph == "captured"
    # setup plan: projection + LayerNorm per adapter, K_i and V_i per transformer
    sn, sn0 = [c[2] for c in rt.setup_plan.calls], [c[2] for c in rt0.setup_plan.calls]
    assert sn.count("layernorm") == n_adapters and sn.count("linear") == 16 + n_adapters * (1 + 32)
    assert sn0.count("xattn_fold") > 0
    # too many images for the kernel's token limit
    with pytest.raises(L.PPError, match="tokens"):
        rt.ensure(B, hw, hw, 77, 4, ("plain",), ip_n=[17] * n_adapters)


# ------------------------------------------------------------------------------------------------------------ pipeline
def _pipe(unet=None):
    from powerpaint_amd import pipelines as PP
    return PP.StableDiffusionPowerPaintBrushNetPipeline(unet=unet)


def test_check_inputs_messages():
    p = _pipe()
    e = [torch.zeros(2, 1, 32)]
    with pytest.raises(ValueError, match="Provide either `ip_adapter_image` or `ip_adapter_image_embeds`. Cannot leave both "
                                         "`ip_adapter_image` and `ip_adapter_image_embeds` defined."):
        p(promptA="a", ip_adapter_image=torch.zeros(1, 3, 8, 8), ip_adapter_image_embeds=e)
    with pytest.raises(ValueError, match="`ip_adapter_image_embeds` has to be of type `list` but is <class 'torch.Tensor'>"):
        p(promptA="a", ip_adapter_image_embeds=e[0])
    with pytest.raises(ValueError, match="`ip_adapter_image_embeds` has to be a list of 3D or 4D tensors but is 2D"):
        p(promptA="a", ip_adapter_image_embeds=[torch.zeros(2, 32)])


def test_image_prompt_without_adapter_or_encoder_is_an_error():
    u = _hip_unet(**TINY)
    p = _pipe(u)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        p.prepare_ip_adapter_image_embeds(None, [torch.zeros(2, 1, 32)], "cpu", 1, True)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        p.prepare_ip_adapter_image_embeds(torch.zeros(1, 3, 8, 8), None, "cpu", 1, True)
    p.load_ip_adapter(_adapter(u.net))
    assert u.config.encoder_hid_dim_type == "ip_image_proj"
    with pytest.raises(ValueError, match="image_encoder"):
        p.prepare_ip_adapter_image_embeds(torch.zeros(1, 3, 8, 8), None, "cpu", 1, True)
    with pytest.raises(ValueError, match="must have same length as the number of IP Adapters. Got 2 images and 1 IP Adapters"):
        p.prepare_ip_adapter_image_embeds([torch.zeros(1, 3, 8, 8)] * 2, None, "cpu", 1, True)
    with pytest.raises(L.PPError, match="image_encoder_folder"):
        p.load_ip_adapter(_adapter(u.net), image_encoder_folder="image_encoder")
    with pytest.raises(L.PPError, match="ip_adapter_masks"):
        p.load_ip_adapter(_adapter(u.net), ip_adapter_masks=[torch.zeros(1, 8, 8)])
    with pytest.raises(ValueError, match="same length"):
        p.set_ip_adapter_scale([1.0, 2.0])
    p.unload_ip_adapter()
    assert u.config.encoder_hid_dim_type is None and u.encoder_hid_proj is None


def test_prepare_image_embeds_follows_the_reference():
    """Precomputed embeds: chunk(2) under CFG, each half repeated num_images_per_prompt times, negative half first; images:
    through the registered encoder with zeros as the negative embeds (pipeline_PowerPaint_Brushnet_CA.py:657-706)."""
    import make_ref_ip_adapter as M
    u = _hip_unet(**TINY)
    p = _pipe(u)
    p.load_ip_adapter([_adapter(u.net, seed=1), _adapter(u.net, seed=2)])
    prompt = IC.case_prompt("two")
    got = p.prepare_ip_adapter_image_embeds(None, prompt["ip_adapter_image_embeds"], "cpu", M.NB, True)
    want = M.prepared_embeds("two")
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want)) and got[1].shape == (4, 2, 32)
    got = p.prepare_ip_adapter_image_embeds(None, prompt["ip_adapter_image_embeds"], "cpu", 3, False)
    assert got[0].shape == (6, 1, 32) and torch.equal(got[0][::2], prompt["ip_adapter_image_embeds"][0][:1].expand(3, 1, 32))
    p.load_ip_adapter(_adapter(u.net, seed=1))
    p.image_encoder = IC.TinyImageEncoder().eval()
    img = IC.case_prompt("image")["ip_adapter_image"]
    got = p.prepare_ip_adapter_image_embeds(img, None, "cpu", M.NB, True)
    want = M.prepared_embeds("image")
    assert len(got) == 1 and torch.equal(got[0], want[0]) and bool((got[0][:M.NB] == 0).all())


# ------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_discriminates_and_is_small():
    G = torch.load(GOLD_PATH, weights_only=False)
    assert os.path.getsize(GOLD_PATH) < 110 * 1024
    assert set(G) == {"one", "two", "image", "one_b"}
    for name, e in G.items():
        assert e["latents"].shape == (2, 4, 16, 16) and e["latents"].dtype == torch.float32
        cos, err, ok = IC.loop_gate(e["plain"], e["latents"])
        assert not ok and abs(cos - e["cos_plain"]) < 1e-6, (name, cos, err)
    assert not IC.loop_gate(G["one_b"]["latents"], G["one"]["latents"])[2]


@pytest.mark.parametrize("name", ["one", "two", "image"])
def test_oracle_loop_with_ip_attention_reproduces_the_fixture(name):
    import make_ref_ip_adapter as M
    G = torch.load(GOLD_PATH, weights_only=False)[name]
    out, nxt = M.oracle_run(name)
    err = (out - G["latents"]).abs()
    assert bool((err <= IC.ATOL + IC.RTOL * G["latents"].abs()).all()), float(err.max())
    assert torch.equal(nxt, G["next_draw"])


# ------------------------------------------------------------------------------------------------------------ ABI
def test_abi_of_pp_ip_attn_add():
    import ctypes
    lib = L.lib()
    assert lib.pp_abi_version() == 29 and L.ABI_VERSION == 29
    assert "pp_ip_attn_add" in L.SIGNATURES and hasattr(ctypes.CDLL(L.LIB_PATH), "pp_ip_attn_add")
    q, k, v, o = 0x10000, 0x20000, 0x30000, 0x40000           # (never dereferenced: every call is refused)

    def call(q_=q, ldq=320, k_=k, v_=v, o_=o, ldo=320, batch=2, heads=8, nq=64, nk=4, d=40, dtype=L.PP_DT_BF16):
        return lib.pp_ip_attn_add(q_, ldq, k_, v_, o_, ldo, batch, heads, nq, nk, d, d ** -0.5, 1.0, dtype, None)

    bad, unsup = -1, -2
    assert call(q_=None) == bad and call(k_=None) == bad and call(v_=None) == bad and call(o_=None) == bad
    assert call(d=24) in (bad, unsup) and call(d=24) == unsup and call(d=44) == bad
    assert call(nk=0) == bad and call(nk=L.PP_IP_MAX_TOKENS + 1) == unsup
    assert call(ldq=319) == bad and call(ldo=312) == bad and call(ldo=324) == bad
    assert call(q_=q + 2) == bad and call(o_=o + 8) == bad and call(o_=q) == bad
    assert call(dtype=L.PP_DT_F32) == bad and call(batch=0) == bad and call(nq=0) == bad
    assert L.PP_IP_MAX_TOKENS == 64
