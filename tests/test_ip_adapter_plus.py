"""IP-Adapter Plus without a GPU: reading and refusing Plus files, the host-side IPAdapterPlusImageProjection against the
Resampler restated from the file format (tests/ip_plus_cases.py), the 4-D embeds plumbing of the UNet and the pipeline, the
shape of the setup plan, pp_perceiver_attn's argument checks, and the fixture tests/golden/ref_ip_adapter_plus.pt against the
oracle loop."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ip_adapter_cases as IC  # noqa: E402
import ip_plus_cases as PC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ip_adapter as IPA  # noqa: E402

GOLD_PATH = os.path.join(HERE, "golden", "ref_ip_adapter_plus.pt")
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
SMALL = dict(Q=16, dim=128, E=64, depth=2, heads=2, ff=256)
PP_ERR_BAD_ARG, PP_ERR_UNSUPPORTED = -1, -2       # include/pp_hip.h
SD15_PLUS = dict(Q=16, dim=768, E=1280, depth=4, heads=12, ff=3072)


def _net(**kw):
    from powerpaint_amd.engine import SDNet
    net = SDNet("unet", 4, **kw)
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    return net


def _hip_unet(**cfg):
    """A HIP UNet whose packed buffer lives on the CPU (no launch ever runs in this file)."""
    from powerpaint_amd.models import UNet2DConditionModel as U
    u = U(in_channels=4, device="cpu", **cfg)
    return u.load_state_dict(u.net.synthetic_state_dict(meta=True), materialize=False)


def _kv(net, g, zeros=False):
    width = dict(net._attn_specs())
    return {f"{2 * k + 1}.{n}.weight": (torch.zeros(width[pre], 768) if zeros else
                                        IC.bf16_round(torch.randn(width[pre], 768, generator=g) / 768 ** 0.5))
            for k, pre in enumerate(net.ip_attn_order()) for n in ("to_k_ip", "to_v_ip")}


def _plus(net, seed=0, **sizes):
    g = torch.Generator().manual_seed(seed)
    return {"image_proj": PC.plus_image_proj(g, **dict(SMALL, **sizes)), "ip_adapter": _kv(net, g)}


def _base(net, T=4, D=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    ip = {"proj.weight": torch.randn(T * 768, D, generator=g), "proj.bias": torch.randn(T * 768, generator=g),
          "norm.weight": torch.randn(768, generator=g), "norm.bias": torch.randn(768, generator=g)}
    return {"image_proj": ip, "ip_adapter": _kv(net, g)}


# ------------------------------------------------------------------------------------------------------------ loader
def test_plus_file_forms_load_and_the_module_is_the_resampler(tmp_path):
    u = _hip_unet(**TINY)
    sd = _plus(u.net, seed=1)
    torch.save(sd, tmp_path / "plus.bin")
    from safetensors.torch import save_file
    save_file({f"{a}.{k}": v.contiguous() for a in sd for k, v in sd[a].items()}, str(tmp_path / "plus.safetensors"))
    want = PC.Resampler.from_file(sd["image_proj"])
    x = torch.randn(3, 10, SMALL["E"], generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref = want(x)
    for form in (sd, str(tmp_path / "plus.bin"), str(tmp_path / "plus.safetensors")):
        u._load_ip_adapter_weights(IPA.read_ip_adapter(form))
        (m,) = u.encoder_hid_proj.image_projection_layers
        assert isinstance(m, IPA.IPAdapterPlusImageProjection) and not isinstance(m, IPA.ImageProjection)
        assert all(p.dtype == torch.float32 and p.device.type == "cpu" for p in m.parameters())
        with torch.no_grad():
            got = m(x)
        assert got.shape == (3, 16, 768)
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        sp = u.net.ip[0]
        assert isinstance(sp, IPA.IPPlus) and tuple(sp) == (16, 64, 128, 768, 2, 2, 256)
        u._unload_ip_adapter()
    # the packed entries: matrices and latents 16-bit, LayerNorm parameters and biases fp32, to_kv as filed
    u._load_ip_adapter_weights(sd)
    P, ip = u.net.params, sd["image_proj"]
    for name, key, dt in (("latents", "latents", torch.bfloat16), ("proj_in.weight", "proj_in.weight", torch.bfloat16),
                          ("proj_in.bias", "proj_in.bias", torch.float32), ("norm_out.weight", "norm_out.weight", torch.float32),
                          ("layers.1.to_kv.weight", "layers.1.0.to_kv.weight", torch.bfloat16),
                          ("layers.0.ff2.weight", "layers.0.1.3.weight", torch.bfloat16),
                          ("layers.1.norm2.bias", "layers.1.0.norm2.bias", torch.float32),
                          ("layers.0.ff_norm.weight", "layers.0.1.0.weight", torch.float32)):
        t = P.tensor(f"ip_adapter.0.resampler.{name}")
        assert t.dtype == dt and torch.equal(t.float().reshape(-1), ip[key].to(dt).float().reshape(-1)), name
    assert P.tensor("ip_adapter.0.mid_block.attentions.0.kv.weight").shape == (1280, 768)
    assert not any(r.name.startswith("ip_adapter") for r in u.net.pack_table() if hasattr(r, "rows"))


def test_module_state_dict_has_the_diffusers_names():
    m = IPA.plus_projection_module(IPA.check_ip_adapter(_net(**TINY), _plus(_net(**TINY))))
    want = {"latents", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias", "norm_out.weight", "norm_out.bias"}
    for i in range(SMALL["depth"]):
        want |= {f"layers.{i}.{n}.{wb}" for n in ("0", "1", "3.0") for wb in ("weight", "bias")}
        want |= {f"layers.{i}.2.{n}.weight" for n in ("to_q", "to_k", "to_v", "to_out.0")}
        want |= {f"layers.{i}.3.1.net.0.proj.weight", f"layers.{i}.3.1.net.2.weight"}
    assert set(m.state_dict()) == want
    # to_kv split in halves: first half of the rows K
    sd = _plus(_net(**TINY))
    m = IPA.plus_projection_module(IPA.check_ip_adapter(_net(**TINY), sd))
    kv = sd["image_proj"]["layers.1.0.to_kv.weight"]
    assert torch.equal(m.layers[1][2].to_k.weight, kv[:128]) and torch.equal(m.layers[1][2].to_v.weight, kv[128:])
    assert set(IPA.plus_key_conversion(2)) == set(sd["image_proj"])


def _edit(fn):
    def make(net):
        sd = _plus(net)
        fn(sd)
        return sd
    return make


def _resize(**sizes):
    def make(net):
        return _plus(net, **sizes)
    return make


REFUSALS = [
    ("out != ctx", _edit(lambda sd: sd["image_proj"].update({"proj_out.weight": torch.zeros(1024, 128),
                                                             "proj_out.bias": torch.zeros(1024),
                                                             "norm_out.weight": torch.zeros(1024),
                                                             "norm_out.bias": torch.zeros(1024)})), "Plus.*out = 1024"),
    ("dim % 64", _resize(dim=96), "Plus.*dim = 96"),
    ("ff % 64", _resize(ff=200), "Plus.*ff = 200"),
    ("inner % 64", _edit(lambda sd: [sd["image_proj"].update({f"layers.{i}.0.to_q.weight": torch.zeros(96, 128),
                                                              f"layers.{i}.0.to_kv.weight": torch.zeros(192, 128),
                                                              f"layers.{i}.0.to_out.weight": torch.zeros(128, 96)})
                                     for i in range(2)]), "Plus.*inner = 96"),
    ("Q > 64", _resize(Q=65), "Plus.*Q = 65"),
    ("missing key", _edit(lambda sd: sd["image_proj"].pop("layers.1.0.norm2.bias")), "Plus.*layers.1.0.norm2.bias"),
    ("missing proj_in", _edit(lambda sd: sd["image_proj"].pop("proj_in.weight")), "Plus.*proj_in.weight"),
    ("surplus key", _edit(lambda sd: sd["image_proj"].update({"extra.weight": torch.zeros(4)})), "Plus.*extra.weight"),
    ("wrong shape", _edit(lambda sd: sd["image_proj"].update({"layers.0.1.3.weight": torch.zeros(128, 300)})),
     "Plus.*layers.0.1.3.weight"),
    ("FaceID lora", _edit(lambda sd: sd["ip_adapter"].update({"1.to_k_lora.down.weight": torch.zeros(8, 8)})),
     "1.to_k_lora.down.weight.*FaceID"),
    ("FaceID Plus", _edit(lambda sd: sd["image_proj"].update({"perceiver_resampler.proj_in.weight": torch.zeros(8, 8)})),
     "perceiver_resampler.proj_in.weight.*FaceID"),
    ("full face", _edit(lambda sd: sd["image_proj"].update({"proj.0.weight": torch.zeros(8, 8)})), "proj.0.weight.*full-face"),
    ("ip_adapter half", _edit(lambda sd: sd["ip_adapter"].pop("3.to_v_ip.weight")), "3.to_v_ip.weight"),
]


@pytest.mark.parametrize("what,make,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_family_or_the_key_and_leave_the_model_as_it_was(what, make, match):
    u = _hip_unet(**TINY)
    u._load_ip_adapter_weights(_base(u.net, seed=7))
    before = (u.net.params.version, dict(u.net.P), list(u.net.ip), u.net.params.total, u.encoder_hid_proj)
    buf = u.net.params.buf
    with pytest.raises(L.PPError, match=match):
        u._load_ip_adapter_weights([_base(u.net, seed=8), make(u.net)])
    assert (u.net.params.version, dict(u.net.P), list(u.net.ip), u.net.params.total, u.encoder_hid_proj) == before
    assert u.net.params.buf is buf


def test_mixed_list_and_the_embeds_of_each_kind():
    u = _hip_unet(**TINY)
    sds = [_base(u.net, seed=1), _plus(u.net, seed=2)]
    u._load_ip_adapter_weights(sds)
    assert u.net.ip[0] == (4, 32) and isinstance(u.net.ip[1], IPA.IPPlus) and not isinstance(u.net.ip[0], IPA.IPPlus)
    g = torch.Generator().manual_seed(0)
    B, S, E = 2, 10, SMALL["E"]
    embeds = [torch.randn(B, 2, 32, generator=g), torch.randn(B, 2, S, E, generator=g)]
    with torch.no_grad():
        a, b = u.encoder_hid_proj(embeds)
        want = PC.Resampler.from_file(sds[1]["image_proj"])(embeds[1].reshape(B * 2, S, E)).reshape(B, 32, 768)
    assert a.shape == (B, 8, 768) and b.shape == (B, 32, 768)
    assert float((b - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert [tuple(e.shape) for e in u._ip_image_embeds({"image_embeds": embeds}, B)] == [(B, 2, 32), (B, 2, S, E)]
    # each kind refuses the other's rank by name; five images of 16 tokens pass the kernel's 64
    with pytest.raises(ValueError, match=r"image_embeds\[1\].*Plus.*4-D"):
        u._ip_image_embeds({"image_embeds": [embeds[0], torch.zeros(B, 2, E)]}, B)
    with pytest.raises(ValueError, match=r"image_embeds\[0\].*base.*3-D"):
        u._ip_image_embeds({"image_embeds": [torch.zeros(B, 1, S, 32), embeds[1]]}, B)
    with pytest.raises(ValueError, match=r"image_embeds\[1\]"):
        u._ip_image_embeds({"image_embeds": [embeds[0], torch.zeros(B, 2, S, E + 64)]}, B)
    assert u._ip_image_embeds({"image_embeds": [embeds[0], torch.zeros(B, 4, S, E)]}, B)[1].shape[1] == 4
    with pytest.raises(L.PPError, match="5 images of 16 tokens.*64"):
        u._ip_image_embeds({"image_embeds": [embeds[0], torch.zeros(B, 5, S, E)]}, B)
    from powerpaint_amd.runtime import NetRuntime
    with pytest.raises(L.PPError, match="tokens"):
        NetRuntime(u.net, "cpu").ensure(B, 8, 8, 77, 4, ("plain",), ip_n=[1, (5, S)])


# ------------------------------------------------------------------------------------------------------------ pipeline
def test_prepare_image_embeds_takes_the_hidden_states_branch():
    """pipeline_PowerPaint_Brushnet_CA.py:639-648, 657-706 with a Plus layer: hidden_states[-2] of the image, and of the ZERO
    image for the negative half, stacked num_images_per_prompt times."""
    from powerpaint_amd import pipelines as PP
    u = _hip_unet(**TINY)
    p = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=u)
    p.load_ip_adapter(_plus(u.net, E=PC.FIX["E"]))
    enc = PC.HiddenStateEncoder().eval()
    p.image_encoder = enc
    img = PC.case_prompt("plus_image")["ip_adapter_image"]
    with torch.no_grad():
        pos = enc(img, output_hidden_states=True).hidden_states[-2]
        neg = enc(torch.zeros_like(img), output_hidden_states=True).hidden_states[-2]
        (got,) = p.prepare_ip_adapter_image_embeds(img, None, "cpu", 3, True)
        (single,) = p.prepare_ip_adapter_image_embeds(img, None, "cpu", 2, False)
    S, E = PC.FIX_S, PC.FIX["E"]
    assert got.shape == (6, 1, S, E) and single.shape == (2, 1, S, E)
    assert all(torch.equal(got[i], neg) for i in range(3)) and all(torch.equal(got[3 + i], pos) for i in range(3))
    assert float(neg.abs().max()) > 0.1 and not torch.equal(pos, enc(img, output_hidden_states=True).hidden_states[-1])
    assert all(torch.equal(single[i], pos) for i in range(2))
    # precomputed 4-D embeds: chunk(2), each half repeated
    e = PC.case_prompt("plus")["ip_adapter_image_embeds"]
    (got,) = p.prepare_ip_adapter_image_embeds(None, e, "cpu", 2, True)
    assert got.shape == (4, 1, S, E) and torch.equal(got[1], e[0][0]) and torch.equal(got[2], e[0][1])
    # a mixed list takes each adapter's own branch
    p.load_ip_adapter([_base(u.net, D=IC.EMBED_DIM), _plus(u.net, E=PC.FIX["E"])])

    class Both(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = IC.TinyImageEncoder().eval(), enc

        def forward(self, image, output_hidden_states=False):
            return self.b(image, output_hidden_states=True) if output_hidden_states else self.a(image)

    p.image_encoder = Both()
    with torch.no_grad():
        got = p.prepare_ip_adapter_image_embeds([img, img], None, "cpu", 1, True)
    assert got[0].shape == (2, 1, IC.EMBED_DIM) and got[1].shape == (2, 1, S, E) and bool((got[0][0] == 0).all())
    assert torch.equal(got[1][0], neg)
    # hidden states serve a Plus adapter: with base adapters only, or none, the request is refused by name
    p.load_ip_adapter(_base(u.net, D=IC.EMBED_DIM))
    with pytest.raises(L.PPError, match="no Plus adapter is loaded"):
        p.encode_image(img, "cpu", 1, output_hidden_states=True)
    assert p.encode_image(img, "cpu", 1)[0].shape == (1, IC.EMBED_DIM)
    p.unload_ip_adapter()
    with pytest.raises(L.PPError, match="no Plus adapter is loaded"):
        p.encode_image(img, "cpu", 1, output_hidden_states=True)


# ------------------------------------------------------------------------------------------------------------ plans
def _describe(plan):
    return [plan.describe(i) for i in range(len(plan.calls))]


PER_LAYER = ["layernorm", "layernorm", "linear", "linear", "linear", "perceiver_attn", "linear", "layernorm", "linear", "linear"]


def test_setup_plan_of_the_sd15_plus_resampler():
    from powerpaint_amd.runtime import NetRuntime
    net = _net()
    z = SD15_PLUS
    g = torch.Generator().manual_seed(0)
    shapes = IPA.plus_image_proj_shapes(z["Q"], z["dim"], z["E"], 768, z["depth"], z["heads"] * 64, z["ff"])
    sd = {"image_proj": {k: torch.zeros(s) for k, s in shapes.items()}, "ip_adapter": _kv(net, g, zeros=True)}
    net.set_ip_adapters([IPA.check_ip_adapter(net, sd)])
    assert tuple(net.ip[0]) == (16, 1280, 768, 768, 4, 12, 3072)
    rt = NetRuntime(net, "cpu")
    B, S = 2, 257
    rt.ensure(B, 64, 64, 77, 4, ("plain",), ip_n=[(1, S)])
    calls = rt.setup_plan.calls
    names = [c[2] for c in calls]
    n_res = 10 * z["depth"] + 3
    assert names[:n_res] == ["linear"] + PER_LAYER * z["depth"] + ["linear", "layernorm"]
    assert names.count("perceiver_attn") == z["depth"] and "perceiver_attn" not in names[n_res:]
    assert names[n_res:].count("linear") == 16 * 3 and "xattn_fold" not in names      # text K / V^T, K_i, V_i per transformer
    gm = [c[1][0]._obj for c in calls[:n_res] if c[2] == "linear"]
    proj_in, (to_q, kvx, kvl, to_out, ff1, ff2), proj_out = gm[0], gm[1:7], gm[-1]
    assert (proj_in.M, proj_in.N, proj_in.K) == (B * S, 768, 1280) and proj_in.bias
    assert (to_q.M, to_q.N, to_q.K) == (B * 16, 768, 768) and not to_q.bias
    assert (kvx.M, kvx.N, kvx.K) == (B * S, 1536, 768) and (kvl.M, kvl.N, kvl.K) == (B * 16, 1536, 768) and kvx.w == kvl.w
    assert (to_out.M, to_out.N, to_out.K) == (B * 16, 768, 768) and to_out.res1
    assert (ff1.M, ff1.N, ff1.K, ff1.act) == (B * 16, 3072, 768, L.PP_ACT_GELU)
    assert (ff2.M, ff2.N, ff2.K, ff2.act) == (B * 16, 768, 3072, L.PP_ACT_NONE) and ff2.res1 == to_out.out
    assert (proj_out.M, proj_out.N, proj_out.K) == (B * 16, 768, 768) and proj_out.bias
    att = [c[1] for c in calls if c[2] == "perceiver_attn"][0]
    # (q, ldq, kv_x, ldkx, nx, kv_l, ldkl, nl, o, ldo, batch, heads, nq, d, scale, dtype)
    assert att[0] == to_q.out and att[2] == kvx.out and att[5] == kvl.out and att[8] == to_out.x1
    assert (att[1], att[3], att[4], att[6], att[7], att[9]) == (768, 1536, S, 1536, 16, 768)
    assert att[10:14] == (B, 12, 16, 64) and att[14] == 0.125
    # the first layer reads the latents the runtime repeats over the images; the tokens feed the K_i / V_i GEMMs
    lat0 = rt.lay["ip_in"][0][3]
    ln2 = [c[1] for c in calls[:n_res] if c[2] == "layernorm"][1]
    assert ln2[0] == lat0 and to_out.res1 == lat0
    tokens = calls[n_res - 1][1][6]
    k_i = [c[1][0]._obj for c in calls[n_res:] if c[2] == "linear" and c[1][0]._obj.x1 == tokens]
    assert len(k_i) == 32 and all(a.M == B * 16 and a.K == 768 for a in k_i)
    # the step plan is the base adapter's, with 16 keys per launch
    ip_calls = [c for c in rt.step_plan.calls if c[2] == "ip_attn_add"]
    assert len(ip_calls) == 16 and all(c[1][9] == 16 for c in ip_calls)
    # four images: 64 keys; the plan is keyed by (n, S)
    key = rt.key
    rt.ensure(B, 64, 64, 77, 4, ("plain",), ip_n=[(4, S)])
    assert rt.key != key and all(c[1][9] == 64 for c in rt.step_plan.calls if c[2] == "ip_attn_add")
    assert rt.setup_plan.flops_by_kind["perceiver_attn"] == 4 * 4.0 * (B * 4) * 12 * 16 * (S + 16) * 64


def test_plans_after_unload_are_those_of_a_net_that_never_saw_an_adapter():
    from powerpaint_amd.runtime import NetRuntime
    never, was = _net(**TINY), _net(**TINY)
    was.set_ip_adapters([IPA.check_ip_adapter(was, _plus(was)), IPA.check_ip_adapter(was, _base(was))])
    rt_w = NetRuntime(was, "cpu")
    rt_w.ensure(2, 16, 16, 77, 4, ("plain",), twin=True, ip_n=[(1, 10), 1])
    assert "perceiver_attn" in [c[2] for c in rt_w.setup_plan.calls]
    was.set_ip_adapters([])
    rt_n, rt_w = NetRuntime(never, "cpu"), NetRuntime(was, "cpu")
    for rt in (rt_n, rt_w):
        rt.ensure(2, 16, 16, 77, 4, ("plain",), twin=True)
    assert rt_n.key == rt_w.key
    assert _describe(rt_n.step_plan) == _describe(rt_w.step_plan) and _describe(rt_n.setup_plan) == _describe(rt_w.setup_plan)
    assert rt_n.step_plan.flops == rt_w.step_plan.flops and rt_n.arena.size == rt_w.arena.size
    assert "perceiver_attn" not in [c[2] for c in rt_w.setup_plan.calls]
    assert was.params.total == never.params.total and sorted(was.P) == sorted(never.P) and was.ip == []


def test_base_only_plans_do_not_change_with_the_plus_code():
    """A base adapter's setup plan holds no Resampler launch and its image-embed inputs stay (pointer, n) pairs."""
    from powerpaint_amd.runtime import NetRuntime
    net = _net(**TINY)
    net.set_ip_adapters([IPA.check_ip_adapter(net, _base(net))])
    rt = NetRuntime(net, "cpu")
    rt.ensure(2, 16, 16, 77, 4, ("plain",), ip_n=[2])
    names = [c[2] for c in rt.setup_plan.calls]
    assert names[:2] == ["linear", "layernorm"] and "perceiver_attn" not in names and len(rt.lay["ip_in"][0]) == 2


# ------------------------------------------------------------------------------------------------------------ kernel
def test_pp_perceiver_attn_argument_checks():
    f = L.lib().pp_perceiver_attn
    p = 1 << 20                                                   # (never dereferenced: every call below is refused first)

    def call(q=p, ldq=128, kvx=p, ldkx=256, nx=10, kvl=p, ldkl=256, nl=16, o=2 * p, ldo=128, batch=2, heads=2, nq=16, d=64,
             dt=L.PP_DT_BF16):
        return f(q, ldq, kvx, ldkx, nx, kvl, ldkl, nl, o, ldo, batch, heads, nq, d, 0.125, dt, None)

    assert call(d=40) == PP_ERR_UNSUPPORTED and call(d=128) == PP_ERR_UNSUPPORTED
    for kw in (dict(ldq=132), dict(ldkx=260), dict(ldkl=260), dict(ldo=132), dict(ldq=64), dict(ldkx=128), dict(ldo=120),
               dict(q=p + 8), dict(kvx=p + 2), dict(kvl=p + 4), dict(o=2 * p + 8), dict(nq=0), dict(nx=0), dict(nl=-1),
               dict(kvl=None), dict(kvl=p, nl=0), dict(q=None), dict(o=p), dict(dt=0), dict(d=0), dict(batch=0)):
        assert call(**kw) == PP_ERR_BAD_ARG, kw
    assert L.lib().pp_abi_version() == 29


# ------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_is_small_and_the_adapter_free_latents_fail_the_gate():
    G = torch.load(GOLD_PATH, weights_only=False)
    assert os.path.getsize(GOLD_PATH) < 110 * 1024
    assert set(G) == {"plus", "plus_image", "mixed", "plus_b"}
    for name, e in G.items():
        assert e["latents"].shape == (2, 4, 16, 16) and e["latents"].dtype == torch.float32
        cos, err, ok = PC.loop_gate(e["plain"], e["latents"])
        assert not ok and abs(cos - e["cos_plain"]) < 1e-6, (name, cos, err)
    assert not PC.loop_gate(G["plus_b"]["latents"], G["plus"]["latents"])[2]
    # zeros in place of the zero image's hidden states are a different (and wrong) call
    z = G["plus_image"]
    err = float((z["latents_zero_negative"] - z["latents"]).abs().max())
    assert abs(err - z["err_zero_negative"]) < 1e-6 and err > 10 * (IC.ATOL + IC.RTOL * float(z["latents"].abs().max()))


@pytest.mark.parametrize("name", ["plus", "plus_image", "mixed"])
def test_oracle_loop_reproduces_the_fixture(name):
    import make_ref_ip_adapter_plus as M
    G = torch.load(GOLD_PATH, weights_only=False)[name]
    out, nxt = M.oracle_run(name)
    err = (out - G["latents"]).abs()
    assert bool((err <= IC.ATOL + IC.RTOL * G["latents"].abs()).all()), float(err.max())
    assert torch.equal(nxt, G["next_draw"])
