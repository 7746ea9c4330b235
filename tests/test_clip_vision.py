"""The CLIP vision tower (`image_encoder` of an IP-Adapter pipeline) on the HIP path.

The pin is `transformers.CLIPVisionModelWithProjection` itself (tests/vit_cases.py::hf_vision: same weights, matrices rounded
to bf16).  CPU: checkpoint key compatibility and `from_pretrained` from a folder, refusals by name, the plan's shape for
ViT-H/14 at 224 x 224, `CLIPImageProcessor` against transformers' PIL processor, `load_ip_adapter(image_encoder_folder=...)`,
the ABI.  GPU: the tower against transformers at the text tower's gate (tests/test_clip.py: cosine >= 0.9995, max error <=
0.03 max(1, max|want|)) on every hidden state, and an image prompt through the BrushNet pipeline end to end.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vit_cases as VC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd.engine import Arena, Builder  # noqa: E402
from powerpaint_amd.models import CLIPVisionModelWithProjection  # noqa: E402
from powerpaint_amd.pipelines.image_processor import CLIPImageProcessor  # noqa: E402

transformers = pytest.importorskip("transformers")


# ------------------------------------------------------------------------------------------------ CPU: checkpoints
def test_checkpoint_key_compatibility_and_from_pretrained(tmp_path):
    hf = VC.hf_vision(**VC.TINY)
    m = CLIPVisionModelWithProjection(device="cpu", **VC.TINY)
    want = {k for k in hf.state_dict() if not k.endswith("position_ids")}
    want = {k if k.startswith(("vision_model.", "visual_projection.")) else "vision_model." + k for k in want}
    assert set(m.state_dict()) == want                                      # transformers' names, `pre_layrnorm` included
    assert "vision_model.pre_layrnorm.weight" in want and "visual_projection.weight" in want
    assert all(p.dtype == torch.float32 for p in m.parameters())            # fp32 masters
    r = m.load_state_dict(hf.state_dict())                                  # as this transformers names them
    assert not r.missing_keys and not r.unexpected_keys
    assert torch.equal(m.vision_model.embeddings.patch_embedding.weight, hf.state_dict()[
        [k for k in hf.state_dict() if k.endswith("patch_embedding.weight")][0]])
    # the other form: the tower's keys without / with the `vision_model.` prefix
    strip = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): torch.randn_like(v)
             for k, v in hf.state_dict().items()}
    r = m.load_state_dict(strip)
    assert not r.missing_keys and not r.unexpected_keys
    assert torch.equal(m.vision_model.post_layernorm.bias, strip["post_layernorm.bias"])
    pre = {("vision_model." + k if not k.startswith("visual_projection.") else k): v for k, v in strip.items()}
    pre["vision_model.embeddings.position_ids"] = torch.arange(10)[None]    # (a 4.x buffer some checkpoints carry)
    r = m.load_state_dict(pre)
    assert not r.missing_keys and not r.unexpected_keys
    # from_pretrained(local_dir): config.json + model.safetensors
    VC.save_tiny_checkpoint(str(tmp_path / "image_encoder"), hf)
    m2 = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="image_encoder", device="cpu")
    assert m2.config.hidden_size == 320 and m2.config.projection_dim == 64 and m2.config.image_size == 42
    assert all(torch.equal(v, hf.state_dict()[k]) for k, v in m2.state_dict().items())
    with pytest.raises(L.PPError, match="GPU"):                              # loud without a GPU, like the text model
        m2(torch.zeros(1, 3, 42, 42))


def test_unrunnable_configs_are_refused_by_name():
    with pytest.raises(L.PPError, match="head_dim.*ViT-L/14"):
        CLIPVisionModelWithProjection(device="cpu", hidden_size=1024, num_attention_heads=16, intermediate_size=4096)   # d = 64
    with pytest.raises(L.PPError, match="head_dim"):
        CLIPVisionModelWithProjection(device="cpu", hidden_size=1664, num_attention_heads=16, intermediate_size=8192)   # d = 104
    with pytest.raises(L.PPError, match="hidden_act='quick_gelu'"):
        CLIPVisionModelWithProjection(device="cpu", hidden_act="quick_gelu", **VC.TINY)
    with pytest.raises(L.PPError, match="num_channels=4"):
        CLIPVisionModelWithProjection(device="cpu", num_channels=4, **VC.TINY)
    with pytest.raises(L.PPError, match="multiples of 64"):
        CLIPVisionModelWithProjection(device="cpu", hidden_size=160, num_attention_heads=2, intermediate_size=640)
    with pytest.raises(L.PPError, match="multiples of 64"):
        CLIPVisionModelWithProjection(device="cpu", **dict(VC.TINY, intermediate_size=600))


# ------------------------------------------------------------------------------------------------ CPU: the plan
def test_plan_shape_of_vit_h_at_224():
    from powerpaint_amd.clip_vision import CLIPVisionNet
    layers, B = 3, 2
    net = CLIPVisionNet(num_hidden_layers=layers)                            # ViT-H/14 otherwise
    sd = {}
    for k, shape in [("embeddings.class_embedding", (1280,)), ("embeddings.patch_embedding.weight", (1280, 3, 14, 14)),
                     ("embeddings.position_embedding.weight", (257, 1280)), ("visual_projection.weight", (1024, 1280))]:
        sd[k] = torch.zeros(shape)
    for n in ("pre_layrnorm", "post_layernorm"):
        sd[f"{n}.weight"], sd[f"{n}.bias"] = torch.ones(1280), torch.zeros(1280)
    for i in range(layers):
        p = f"encoder.layers.{i}"
        for n in ("layer_norm1", "layer_norm2"):
            sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"] = torch.ones(1280), torch.zeros(1280)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[f"{p}.self_attn.{n}.weight"], sd[f"{p}.self_attn.{n}.bias"] = torch.zeros(1280, 1280), torch.zeros(1280)
        sd[f"{p}.mlp.fc1.weight"], sd[f"{p}.mlp.fc1.bias"] = torch.zeros(5120, 1280), torch.zeros(5120)
        sd[f"{p}.mlp.fc2.weight"], sd[f"{p}.mlp.fc2.bias"] = torch.zeros(1280, 5120), torch.zeros(1280)
    net.pack(sd, "cpu")
    dry = Arena()
    pb = Builder(dry)
    net.build(pb, dry.alloc(B * 3 * 224 * 224 * 4), B, 224, 224)
    calls = pb.plan.calls
    names = [c[2] for c in calls]
    # front: patchify, patch GEMM, embed + pre_layrnorm; per layer: LN, QKV, V^T, attention, out-proj, LN, fc1, fc2; back: one
    # post_layernorm per image on its class-token row, visual_projection
    per_layer = ["layernorm", "linear", "transpose_v", "attention", "linear", "layernorm", "linear", "linear"]
    assert names == ["vit_patchify", "linear", "vit_embed_ln"] + per_layer * layers + ["layernorm"] * B + ["linear"]
    assert len(names) == 3 + 8 * layers + B + 1
    gemms = [c[1][0]._obj for c in calls if c[2] == "linear"]
    patch, fc1, fc2, proj = gemms[0], gemms[3], gemms[4], gemms[-1]
    assert (patch.M, patch.N, patch.K) == (B * 256, 1280, 640) and not patch.bias and patch.act == L.PP_ACT_NONE
    assert (fc1.M, fc1.N, fc1.K, fc1.act) == (B * 257, 5120, 1280, L.PP_ACT_GELU)
    assert (fc2.M, fc2.N, fc2.K, fc2.act) == (B * 257, 1280, 5120, L.PP_ACT_NONE) and fc2.res1
    assert [g.act for g in gemms].count(L.PP_ACT_GELU) == layers
    assert (gemms[1].N, gemms[1].K) == (3840, 1280) and not gemms[1].out_vt          # fused q|k|v; V^T by pp_transpose_v
    assert (proj.M, proj.N, proj.K) == (B, 1024, 1280) and not proj.bias
    att = [c[1] for c in calls if c[2] == "attention"][0]
    # (q, ldq, k, ldk, vt, ldvt, o, ldo, batch, heads, nq, nk, d, scale, dtype)
    assert att[1] == att[3] == 3840 and att[5] == 264 and att[8:13] == (B, 16, 257, 257, 80)
    tv = [c[1] for c in calls if c[2] == "transpose_v"][0]
    assert tv[1:5] == (3840, B, 257, 1280) and tv[6] == 264
    pat = calls[0][1]
    assert pat[1:6] == (L.PP_DT_F32, B, 224, 224, 14) and pat[7:9] == (640, 640)
    post = [c[1] for c in calls if c[2] == "layernorm"][-B:]
    assert all(p[1] == 1 and p[2] == 1280 for p in post) and post[1][0] - post[0][0] == 257 * 1280 * 2
    assert len(net.hidden) == layers + 1
    with pytest.raises(L.PPError, match="tokens"):
        net.tokens(224, 210)


# ------------------------------------------------------------------------------------------------ CPU: preprocessing
@pytest.mark.parametrize("hw", [(260, 300), (300, 260), (150, 100), (224, 224)], ids=["260x300", "300x260", "150x100", "224x224"])
def test_clip_image_processor_matches_transformers(hw):
    import PIL.Image
    g = np.random.default_rng(hw[0] * 1000 + hw[1])
    arr = g.integers(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8)
    img = PIL.Image.fromarray(arr)
    ref = transformers.CLIPImageProcessor()(img, return_tensors="pt").pixel_values
    ours = CLIPImageProcessor()
    got = ours(img, return_tensors="pt").pixel_values
    assert got.shape == ref.shape == (1, 3, 224, 224) and got.dtype == torch.float32
    assert float((got - ref).abs().max()) <= 1e-6                             # both run the same PIL bicubic
    got_np = ours(arr, return_tensors="pt").pixel_values                      # HWC uint8 arrays, lists of either
    assert torch.equal(got_np, got)
    two = ours([img, arr]).pixel_values
    assert two.shape == (2, 3, 224, 224) and torch.equal(two[0], got[0]) and torch.equal(two[1], got[0])


def test_clip_image_processor_from_config(tmp_path):
    import json
    import PIL.Image
    ref = transformers.CLIPImageProcessor(size={"shortest_edge": 42}, crop_size={"height": 42, "width": 42})
    with open(tmp_path / "preprocessor_config.json", "w") as f:
        json.dump({k: v for k, v in ref.to_dict().items() if k != "resample"} | {"resample": 3}, f)
    ours = CLIPImageProcessor.from_pretrained(str(tmp_path))
    assert ours.size == 42 and ours.crop_size == (42, 42)
    img = PIL.Image.fromarray(np.random.default_rng(3).integers(0, 256, size=(90, 61, 3), dtype=np.uint8))
    got, want = ours(img).pixel_values, ref(img, return_tensors="pt").pixel_values
    assert got.shape == (1, 3, 42, 42) and float((got - want).abs().max()) <= 1e-6
    with pytest.raises(ValueError, match="bicubic"):
        CLIPImageProcessor(resample=2)


# ------------------------------------------------------------------------------------------------ CPU: the pipeline
def _ip_folder(tmp_path, unet, hf):
    from test_ip_adapter import _adapter
    root = tmp_path / "ip"
    os.makedirs(root / "models")
    torch.save(_adapter(unet.net), str(root / "models" / "ip.bin"))
    VC.save_tiny_checkpoint(str(root / "models" / "image_encoder"), hf)
    return str(root)


def test_load_ip_adapter_loads_the_image_encoder_from_its_folder(tmp_path):
    from powerpaint_amd import pipelines as PP
    from test_ip_adapter import TINY, _adapter, _hip_unet
    hf = VC.hf_vision(**dict(VC.TINY, projection_dim=32))
    u = _hip_unet(**TINY)
    p = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=u)
    root = _ip_folder(tmp_path, u, hf)
    p.load_ip_adapter(root, subfolder="models", weight_name="ip.bin")         # the default: no encoder is loaded
    assert p.image_encoder is None and p.feature_extractor is None
    p.load_ip_adapter(root, subfolder="models", weight_name="ip.bin", image_encoder_folder="image_encoder")
    enc, fe = p.image_encoder, p.feature_extractor
    assert isinstance(enc, CLIPVisionModelWithProjection) and isinstance(fe, CLIPImageProcessor)
    assert enc.config.projection_dim == 32 and p._modules["image_encoder"] is enc
    assert torch.equal(enc.visual_projection.weight, hf.state_dict()["visual_projection.weight"])
    assert next(enc.parameters()).dtype == torch.float32                     # what encode_image reads
    p.load_ip_adapter(root, subfolder="models", weight_name="ip.bin", image_encoder_folder="image_encoder")
    assert p.image_encoder is enc and p.feature_extractor is fe               # a second call keeps the same objects
    p.unload_ip_adapter()
    assert p.image_encoder is enc                                            # (stays registered)
    # a path with "/" is relative to the model folder, as diffusers resolves it
    p2 = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=_hip_unet(**TINY))
    p2.load_ip_adapter(root, subfolder="models", weight_name="ip.bin", image_encoder_folder="models/image_encoder")
    assert isinstance(p2.image_encoder, CLIPVisionModelWithProjection)
    with pytest.raises(L.PPError, match="does not exist"):
        p2.load_ip_adapter(root, subfolder="models", weight_name="ip.bin", image_encoder_folder="nowhere")
    # a state-dict source has no folder to resolve the argument against
    with pytest.raises(L.PPError, match="image_encoder_folder"):
        p2.load_ip_adapter(_adapter(u.net), image_encoder_folder="image_encoder")
    # Plus stays refused
    with pytest.raises(L.PPError, match="Plus"):
        p.encode_image(torch.zeros(1, 3, 42, 42), "cpu", 1, output_hidden_states=True)


def test_pipeline_folder_loader_picks_up_an_image_encoder(tmp_path):
    import json
    from powerpaint_amd import pipelines as PP
    hf = VC.hf_vision(**VC.TINY)
    VC.save_tiny_checkpoint(str(tmp_path / "image_encoder"), hf)
    with open(tmp_path / "model_index.json", "w") as f:
        json.dump({"_class_name": "StableDiffusionPowerPaintBrushNetPipeline",
                   "image_encoder": ["transformers", "CLIPVisionModelWithProjection"], "feature_extractor": [None, None]}, f)
    p = PP.StableDiffusionPowerPaintBrushNetPipeline.from_pretrained(str(tmp_path), device="cpu")
    assert isinstance(p.image_encoder, CLIPVisionModelWithProjection) and p.feature_extractor is None
    assert torch.equal(p.image_encoder.visual_projection.weight, hf.state_dict()["visual_projection.weight"])
    p = PP.StableDiffusionPowerPaintBrushNetPipeline.from_pretrained(str(tmp_path), device="cpu", image_encoder=None)
    assert p.image_encoder is None                                           # an override leaves it out


# ------------------------------------------------------------------------------------------------ CPU: ABI
def test_abi_of_the_vit_kernels_and_the_gelu_code():
    lib = L.lib()
    assert lib.pp_abi_version() == 29 and L.ABI_VERSION == 29 and L.PP_ACT_GELU == 4
    so = ctypes.CDLL(L.LIB_PATH)
    for s in ("pp_vit_patchify", "pp_vit_embed_ln"):
        assert s in L.SIGNATURES and hasattr(so, s)
    src, dst = 0x10000, 0x20000                               # (never dereferenced: every call is refused)

    def patchify(src_=src, sdt=0, batch=1, h=28, w=28, p=14, dst_=dst, cols=640, ldo=640, dt=L.PP_DT_BF16):
        return lib.pp_vit_patchify(src_, sdt, batch, h, w, p, dst_, cols, ldo, dt, None)

    bad = -1
    assert patchify(src_=None) == bad and patchify(dst_=None) == bad and patchify(batch=0) == bad and patchify(batch=-1) == bad
    assert patchify(h=13) == bad and patchify(w=-28) == bad and patchify(p=0) == bad and patchify(sdt=3) == bad
    assert patchify(cols=584) == bad and patchify(cols=644, ldo=648) == bad and patchify(ldo=632) == bad
    assert patchify(dt=L.PP_DT_F32) == bad and patchify(dst_=dst + 2) == bad

    def embed(p_=src, ldp=320, cls=0x30000, pos=0x40000, batch=1, np_=4, C=320, g=0x50000, b=0x60000, y=dst, dt=L.PP_DT_BF16):
        return lib.pp_vit_embed_ln(p_, ldp, cls, pos, batch, np_, C, g, b, 1e-5, y, dt, None)

    assert embed(p_=None) == bad and embed(cls=None) == bad and embed(pos=None) == bad and embed(g=None) == bad
    assert embed(b=None) == bad and embed(y=None) == bad and embed(batch=0) == bad and embed(np_=0) == bad and embed(np_=-3) == bad
    assert embed(C=324) == bad and embed(C=-8) == bad and embed(ldp=312) == bad and embed(ldp=324) == bad
    assert embed(dt=0) == bad and embed(y=dst + 8) == bad
    assert embed(C=2056, ldp=2056) == -2                      # PP_ERR_UNSUPPORTED: wider than pp_layernorm's rows
    # the GEMM's activation code: 4 is defined now, anything outside 0 .. 4 is a bad argument (it used to run as PP_ACT_NONE)
    a = L.gemm_args(L.PP_DT_BF16, 64, 64, 64, 0x1000, 0x2000, 0x3000)
    for act, want in ((5, -1), (-1, -1), (17, -1)):
        a.act = act
        assert lib.pp_gemm_bf16(ctypes.byref(a), None) == want, act
    a.act = L.PP_ACT_GELU
    a.row_stats_out = 0x4000                                   # (no GELU beside the folded LayerNorm's row moments)
    assert lib.pp_gemm_bf16(ctypes.byref(a), None) == -2
    c = L.conv3x3_args(L.PP_DT_BF16, 1, 8, 8, 64, 64, 0x1000, w=0x2000, out=0x3000)
    c.act = L.PP_ACT_GELU
    assert lib.pp_gemm_bf16(ctypes.byref(c), None) == -2      # (nor on a conv)


# ------------------------------------------------------------------------------------------------ GPU
def _gate(got, want):
    got, want = got.float().cpu(), want.float()
    cos = F.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    err = (got - want).abs().max().item()
    return cos, err, cos >= 0.9995 and err <= 0.03 * max(1.0, want.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(VC.TOWER_CASES))
def test_tower_matches_transformers_gpu(case):
    """(a) 10 tokens, batch 2; (b) 257 tokens; (c) ViT-H/14's widths at 257 tokens, batch 3 -- two layers each (depth adds no
    kernel shape).  Every hidden state, last_hidden_state and image_embeds; then other pixels at the same shape (stale
    arena / plan state would show)."""
    cfg, B = VC.tower_cfg(case), VC.TOWER_CASES[case][6]
    hf = VC.hf_vision(seed=len(case) + ord(case), **cfg)
    m = CLIPVisionModelWithProjection(device="cuda", **cfg)
    m.load_state_dict(hf.state_dict())
    g = torch.Generator().manual_seed(7)
    S = cfg["image_size"]
    runs = []
    for k in range(2):
        px = torch.randn(B, 3, S, S, generator=g) * (1.0 + 0.5 * k)
        with torch.no_grad():
            ref = hf(pixel_values=px, output_hidden_states=True)
        out = m(px.cuda(), output_hidden_states=True)
        n = (S // 14) ** 2 + 1
        assert len(out.hidden_states) == len(ref.hidden_states) == cfg["num_hidden_layers"] + 1
        assert out.image_embeds.shape == (B, cfg["projection_dim"]) and out.image_embeds.dtype == torch.float32
        assert out.last_hidden_state.shape == (B, n, cfg["hidden_size"])
        fails = []
        for name, a, b in [(f"hidden_states[{i}]", x, y) for i, (x, y) in enumerate(zip(out.hidden_states, ref.hidden_states))] + \
                [("last_hidden_state", out.last_hidden_state, ref.last_hidden_state), ("image_embeds", out.image_embeds, ref.image_embeds)]:
            cos, err, ok = _gate(a, b)
            print(f"[clip_vision] case {case} run {k} {name}: cosine {cos:.6f} max-abs {err:.4g} of max|want| {float(b.abs().max()):.4g}")
            if not ok:
                fails.append((name, cos, err))
        assert not fails, fails
        assert torch.equal(out.last_hidden_state, out.hidden_states[-1])
        plain = m(px.cuda())                                                    # without hidden states: the same embeds
        assert plain.hidden_states is None and torch.equal(plain.image_embeds, out.image_embeds)
        runs.append(out.image_embeds.clone())
    assert not torch.equal(runs[0], runs[1])
    names = [c[2] for c in m._rt.plan.calls]
    assert names.count("vit_patchify") == 1 and names.count("vit_embed_ln") == 1
    if case == "a":
        # a parameter change is picked up (repack on version change)
        with torch.no_grad():
            m.visual_projection.weight.mul_(2.0)
        again = m(px.cuda()).image_embeds
        assert torch.allclose(again, 2.0 * runs[1], rtol=2e-2, atol=1e-3) and not torch.equal(again, runs[1])


class _Keep:
    """An image prompt that survives the `.to(device)` the shared pipeline caller applies to every prompt value."""

    def __init__(self, v):
        self.v = v

    def to(self, *a, **k):
        return self.v


@pytest.mark.gpu
def test_image_prompt_end_to_end_gpu():
    """`ip_adapter_image=<PIL image>` through the registered HIP tower and processor gives the latents of
    `ip_adapter_image_embeds=` built from that tower's own output, bit for bit, and not those of the run without an image."""
    import PIL.Image
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ip_adapter_cases as IC
    import make_ref_ip_adapter as M
    from test_ip_adapter_gpu import _pipeline
    pipe, call = _pipeline(torch.bfloat16, "one")
    cfg = dict(VC.TINY, projection_dim=IC.EMBED_DIM)
    hf = VC.hf_vision(seed=11, **cfg)
    enc = CLIPVisionModelWithProjection(device="cuda", **cfg)
    enc.load_state_dict(hf.state_dict())
    pipe.image_encoder = enc
    pipe.feature_extractor = CLIPImageProcessor(size=42, crop_size=42)
    img = PIL.Image.fromarray(np.random.default_rng(5).integers(0, 256, size=(70, 55, 3), dtype=np.uint8))
    out_img, _ = call(dict(ip_adapter_image=_Keep(img)))
    assert "vit_embed_ln" in [c[2] for c in enc._rt.plan.calls]
    embeds = pipe.prepare_ip_adapter_image_embeds(img, None, torch.device("cuda"), 1, True)
    assert len(embeds) == 1 and embeds[0].shape == (2, 1, IC.EMBED_DIM) and bool((embeds[0][0] == 0).all())
    px = pipe.feature_extractor(img).pixel_values
    with torch.no_grad():
        want = hf(pixel_values=px).image_embeds
    cos, err, ok = _gate(embeds[0][1], want)
    assert ok, (cos, err)
    out_emb, _ = call(dict(ip_adapter_image_embeds=embeds))
    assert torch.equal(out_img, out_emb)
    pipe.unload_ip_adapter()
    out_plain, _ = call()
    assert bool(torch.isfinite(out_img).all()) and not torch.equal(out_img, out_plain)
    assert M.NB == 2 and out_img.shape[0] == 2
