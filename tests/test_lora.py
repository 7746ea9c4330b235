"""CPU: LoRA adapter files (both key conventions, what is refused), the packing table behind SDNet.load_state_dict /
SDNet.repack, the pp_lora_merge argument checks and the text tower's merge.

The key conventions are restated from the published form of diffusers / PEFT (`unet.<module>.lora_A.weight`, the older
`.lora.down.weight`) and kohya-ss (`lora_unet_<module with underscores>.lora_down.weight`, `.alpha`) files.  diffusers
and peft are not importable where this suite runs, so the conventions are NOT pinned against the libraries (the same
standing as the other unpinned parts, tests/golden/README.md): the adapters are generated from seeds, written to
`.safetensors` files in tmp_path and read back.  Float64 torch is the reference of the merge.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lora_cases import diffusers_keys, kohya_keys, make_factors, merged_weights_f64  # noqa: E402

from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import engine as E  # noqa: E402
from powerpaint_amd import lora  # noqa: E402
from powerpaint_amd.engine import PackRecipe, PackVec, SDNet  # noqa: E402
from powerpaint_amd.lora import LoraAdapter, read_lora  # noqa: E402

TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))


def _save(tmp_path, name, sd):
    from safetensors.torch import save_file
    f = os.path.join(str(tmp_path), name)
    save_file({k: v.contiguous() for k, v in sd.items()}, f)
    return f


@pytest.fixture(scope="module")
def full_adapter():
    """Rank-3 factors over EVERY target of the full SD-1.5 UNet and of the SD-1.5 text tower."""
    ut, tt = lora._default_unet_targets(), lora._default_text_targets()
    return ut, tt, LoraAdapter(unet=make_factors(ut, None, 3, seed=1), text_encoder=make_factors(tt, None, 2, seed=2))


def test_targets_are_every_matrix_of_the_unet_and_the_six_projections_of_the_tower(full_adapter):
    ut, tt, _ = full_adapter
    spec = SDNet("unet", 4).state_dict_spec()
    assert set(ut) == {k[:-7] for k, s in spec.items() if k.endswith(".weight") and len(s) in (2, 4)}
    kinds = {m.rsplit(".", 1)[-1] if not m.endswith("to_out.0") else "to_out.0" for m in ut}
    for want in ("to_q", "to_k", "to_v", "to_out.0", "proj", "2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut",
                 "time_emb_proj", "conv", "conv_in", "conv_out", "linear_1", "linear_2"):
        assert want in kinds, want
    assert not any(".norm" in m for m in ut)
    assert len(tt) == 12 * 6 and all(m.startswith("text_model.encoder.layers.") for m in tt)


@pytest.mark.parametrize("style", ["peft", "old", "kohya"])
def test_both_conventions_parse_to_the_adapter_they_were_written_from(full_adapter, style, tmp_path):
    ut, tt, ad = full_adapter
    sd = kohya_keys(ad) if style == "kohya" else diffusers_keys(ad, style)
    if style == "kohya":
        assert "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_out_0.lora_down.weight" in sd
        assert "lora_unet_mid_block_attentions_0_transformer_blocks_0_ff_net_0_proj.alpha" in sd
        assert "lora_te_text_model_encoder_layers_11_self_attn_q_proj.lora_up.weight" in sd
        assert len([k for k in sd if k.endswith(".alpha")]) == len(ut) + len(tt)       # every target resolved, none skipped
    else:
        assert ("unet.mid_block.attentions.0.proj_in" + (".lora_A.weight" if style == "peft" else ".lora.down.weight")) in sd
    back = read_lora(_save(tmp_path, "a.safetensors", sd))
    assert sorted(back.unet) == sorted(ut) and sorted(back.text_encoder) == sorted(tt)
    assert back.equal(ad)
    assert read_lora(sd).equal(ad)                                                     # a state dict instead of a path
    # a directory + weight_name, and the .bin form
    torch.save(sd, os.path.join(str(tmp_path), "pytorch_lora_weights.bin"))
    assert read_lora(str(tmp_path), weight_name="pytorch_lora_weights.bin").equal(ad)


def test_kohya_alpha_is_kept_and_defaults_to_the_rank(tmp_path):
    ut = lora._default_unet_targets()
    m = "up_blocks.1.attentions.2.transformer_blocks.0.attn2.to_k"
    ad = LoraAdapter(unet=make_factors(ut, None, 8, seed=3, alpha=2.0, modules=[m]))
    sd = kohya_keys(ad)
    assert read_lora(sd, text_modules={}).unet[m][2] == 2.0
    del sd["lora_unet_" + m.replace(".", "_") + ".alpha"]
    assert read_lora(sd, text_modules={}).unet[m][2] == 8.0
    f64 = merged_weights_f64({m + ".weight": torch.zeros(ut[m])}, [(ad.unet, 0.5)], scale=0.6)[m + ".weight"]
    down, up, alpha = ad.unet[m]
    assert torch.allclose(f64, 0.5 * 0.6 * (2.0 / 8) * (up.double() @ down.double()))


def _one(module="mid_block.attentions.0.transformer_blocks.0.attn1.to_q", rank=4):
    ut = lora._default_unet_targets()
    return ut, LoraAdapter(unet=make_factors(ut, None, rank, seed=4, modules=[module]))


@pytest.mark.parametrize("case", ["no_module", "no_module_kohya", "shape", "dora", "hada", "lokr", "mid", "bias", "bias_kohya",
                                  "rank", "half", "unknown"])
def test_refused_by_name(case):
    ut, ad = _one()
    m = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    sd, ksd = diffusers_keys(ad), kohya_keys(ad)
    kn = "lora_unet_" + m.replace(".", "_")
    if case == "no_module":
        bad = "unet.mid_block.attentions.0.transformer_blocks.0.attn3.to_q.lora_A.weight"
        sd[bad] = sd.pop(f"unet.{m}.lora_A.weight")
    elif case == "no_module_kohya":
        sd, bad = ksd, "lora_unet_mid_block_attentions_0_transformer_blocks_0_attn1_to_qq.lora_down.weight"
        sd[bad] = sd.pop(kn + ".lora_down.weight")
    elif case == "shape":
        bad = f"unet.{m}.lora_A.weight"
        sd[bad] = torch.zeros(4, 640)
    elif case == "dora":
        sd, bad = ksd, kn + ".dora_scale"
        sd[bad] = torch.ones(1280)
    elif case == "hada":
        sd, bad = ksd, kn + ".hada_w1_a"
        sd[bad] = torch.ones(4, 4)
    elif case == "lokr":
        sd, bad = ksd, kn + ".lokr_w1"
        sd[bad] = torch.ones(4, 4)
    elif case == "mid":
        sd, bad = ksd, kn + ".lora_mid.weight"
        sd[bad] = torch.ones(4, 4, 3, 3)
    elif case == "bias":
        bad = f"unet.{m}.lora_B.bias"
        sd[bad] = torch.zeros(1280)
    elif case == "bias_kohya":
        sd, bad = ksd, kn + ".diff_b"
        sd[bad] = torch.zeros(1280)
    elif case == "rank":
        _, big = _one(rank=L.PP_LORA_MAX_RANK + 1)
        sd, bad = diffusers_keys(big), f"unet.{m}.lora_"
    elif case == "half":
        bad = f"unet.{m}.lora_A.weight"
        del sd[f"unet.{m}.lora_B.weight"]
    else:
        bad = "some_other.tensor"
        sd[bad] = torch.zeros(1)
    with pytest.raises(L.PPError) as ei:
        read_lora(sd, text_modules={})
    assert bad in str(ei.value), str(ei.value)


def test_adapter_set_bookkeeping():
    s = lora.AdapterSet()
    s.add("a", {})
    s.add("b", {})
    assert list(s.active) == ["a", "b"] and s.state(0.5) == ((("a", 1, 1.0), ("b", 2, 1.0)), 0.5)
    s.set(["b"], [0.25])
    assert s.state(1.0) == ((("b", 2, 0.25),), 1.0)
    with pytest.raises(ValueError):
        s.add("a", {})
    with pytest.raises(ValueError):
        s.set(["c"])
    s.delete("b")
    assert s.state(1.0) is None and list(s.loaded) == ["a"]
    s.add("b", {})                                    # the name comes back: another load, another state
    s.set(["b"], [0.25])
    assert s.state(1.0) == ((("b", 3, 0.25),), 1.0)
    s.delete("b")
    for i in range(L.PP_LORA_MAX_ADAPTERS):
        s.add(f"x{i}", {})
    with pytest.raises(L.PPError, match="at most 8"):
        s.set(["a"] + [f"x{i}" for i in range(L.PP_LORA_MAX_ADAPTERS)])


# ------------------------------------------------------------------------------------------------ the packing table
@pytest.mark.parametrize("kind,kw", [("unet", dict(in_channels=9)), ("unet", dict(in_channels=4)),
                                     ("brushnet", dict(in_channels=4, conditioning_channels=5)),
                                     ("controlnet", dict(in_channels=4, conditioning_channels=3))])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_packing_table_is_complete_and_is_what_load_state_dict_packs(kind, kw, dt):
    tiny = {k: v for k, v in TINY.items() if not (kind == "controlnet" and k == "up_block_types")}
    net = SDNet(kind, dtype=dt, **kw, **tiny)
    sd = net.synthetic_state_dict(seed=0)
    for k in sd:                                       # (norm affine away from (1, 0): the folds must show)
        if sd[k].dim() == 1:
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(len(k)))
    net.load_state_dict(sd, "cpu")
    pk = net.params
    table = net.pack_table()
    assert all(isinstance(it, (PackRecipe, PackVec)) for it in table)
    W = lambda k: sd[k].float()                        # noqa: E731
    made = []
    for it in table:
        for name, t, d in net.pack_host(it, W):
            made.append(name)
            assert pk.shapes[name][1] == d
            assert torch.equal(pk.tensor(name), t.to(d)), name          # bitwise what the buffer holds
    assert made == list(pk.offsets)                                     # every packed entry, in buffer order, once
    used = set()
    for it in table:
        if isinstance(it, PackRecipe):
            used |= {m + ".weight" for m in it.sources()}
    want = {k for k, s in net.state_dict_spec().items() if k.endswith(".weight") and len(s) in (2, 4)}
    assert used == want                                                 # every non-norm source weight is in a recipe
    # and the recipes say what the buffer holds, restated by hand (the loop above goes through pack_host on both sides; the
    # sha256 of the whole buffer against the parent commit is recorded in profiles/lora_merge.txt)
    bf = dt
    tbm = "mid_block.attentions.0.transformer_blocks.0"
    assert torch.equal(pk.tensor(f"{tbm}.attn2.kv.weight"),
                       torch.cat([sd[f"{tbm}.attn2.to_k.weight"], sd[f"{tbm}.attn2.to_v.weight"]], 0).to(bf))
    assert torch.equal(pk.tensor(f"{tbm}.attn2.to_q.weight"), (sd[f"{tbm}.attn2.to_q.weight"] * sd[f"{tbm}.norm2.weight"][None, :]).to(bf))
    assert torch.equal(pk.tensor(f"{tbm}.attn2.to_q.bias"), sd[f"{tbm}.attn2.to_q.weight"] @ sd[f"{tbm}.norm2.bias"])
    tws = [p for p, _, _ in net._resnet_specs()]
    assert torch.equal(pk.tensor("temb_all.weight"), torch.cat([sd[f"{p}.time_emb_proj.weight"] for p in tws], 0).to(bf))
    assert torch.equal(pk.tensor("temb_all.bias"), torch.cat([sd[f"{p}.time_emb_proj.bias"] for p in tws], 0))
    r0 = "down_blocks.0.resnets.0"
    assert torch.equal(pk.tensor(f"{r0}.conv1.weight"), E._conv_igemm(sd[f"{r0}.conv1.weight"]).to(bf))
    assert torch.equal(pk.tensor(f"{r0}.norm1.gb"), torch.stack([sd[f"{r0}.norm1.weight"], sd[f"{r0}.norm1.bias"]], 1))
    assert torch.equal(pk.tensor("down_blocks.0.downsamplers.0.conv.weight"),
                       E._conv_igemm(sd["down_blocks.0.downsamplers.0.conv.weight"]).to(bf))
    if kind == "brushnet":
        assert torch.equal(pk.tensor("conv_in.weight"), E._conv_igemm_cpad(sd["conv_in_condition.weight"], 64).to(bf))
        assert torch.equal(pk.tensor("conv_in.bias"), sd["conv_in_condition.bias"])
        for z in ("brushnet_down_blocks.0", "brushnet_mid_block", "brushnet_up_blocks.0"):
            assert torch.equal(pk.tensor(z + ".weight"), sd[z + ".weight"].reshape(sd[z + ".weight"].shape[0], -1).to(bf)), z
        r = "up_blocks.0.resnets.0"                 # 1280 -> 640 channels: conv_shortcut rides as conv2's K tail
        co, ci = sd[f"{r}.conv_shortcut.weight"].shape[:2]
        assert torch.equal(pk.tensor(f"{r}.conv2.weight"),
                           torch.cat([E._conv_igemm(sd[f"{r}.conv2.weight"]), sd[f"{r}.conv_shortcut.weight"].reshape(co, ci)], 1).to(bf))
        assert torch.equal(pk.tensor(f"{r}.conv2.bias"), sd[f"{r}.conv2.bias"] + sd[f"{r}.conv_shortcut.bias"])
    if kind == "controlnet":
        assert torch.equal(pk.tensor("conv_in.weight"), E._conv_igemm_cpad(sd["conv_in.weight"], 64).to(bf))
        for z in ("controlnet_down_blocks.0", "controlnet_mid_block"):
            assert torch.equal(pk.tensor(z + ".weight"), sd[z + ".weight"].reshape(sd[z + ".weight"].shape[0], -1).to(bf)), z
        for n in ("conv_in", "blocks.0", "blocks.5", "conv_out"):
            k = f"controlnet_cond_embedding.{n}"
            assert torch.equal(pk.tensor(k + ".weight"), E._conv_direct(sd[k + ".weight"]).to(bf)), k
            assert torch.equal(pk.tensor(k + ".bias"), sd[k + ".bias"])
        assert not any(n.startswith("up_blocks.") for n in pk.offsets)
    if kind == "unet":
        tb = "down_blocks.0.attentions.0.transformer_blocks.0"
        qkv = torch.cat([sd[f"{tb}.attn1.to_{x}.weight"] for x in "qkv"], 0) * sd[f"{tb}.norm1.weight"][None, :]
        assert torch.equal(pk.tensor(f"{tb}.attn1.qkv.weight"), qkv.to(bf))
        assert torch.equal(pk.tensor(f"{tb}.attn1.qkv.weight_kp"), E._kperm(qkv).to(bf))
        assert torch.equal(pk.tensor(f"{tb}.attn1.qkv.colsum"), qkv.to(bf).float().sum(1))
        ff1 = sd[f"{tb}.ff.net.0.proj.weight"]
        assert torch.equal(pk.tensor(f"{tb}.ff1.weight"), E._geglu_interleave(ff1 * sd[f"{tb}.norm3.weight"][None, :]).to(bf))
        assert torch.equal(pk.tensor(f"{tb}.ff1.bias"),
                           E._geglu_interleave(ff1 @ sd[f"{tb}.norm3.bias"] + sd[f"{tb}.ff.net.0.proj.bias"]))
        pre = "down_blocks.0.attentions.0"
        po = sd[f"{pre}.proj_out.weight"].reshape(320, 320)
        assert torch.equal(pk.tensor(f"{pre}.ff2_proj_out.weight"), torch.cat([po @ sd[f"{tb}.ff.net.2.weight"], po], 1).to(bf))
        r = "down_blocks.1.resnets.0"
        assert torch.equal(pk.tensor(f"{r}.conv2.weight"),
                           torch.cat([E._conv_igemm(sd[f"{r}.conv2.weight"]), sd[f"{r}.conv_shortcut.weight"].reshape(640, 320)], 1).to(bf))
        assert torch.equal(pk.tensor("conv_in.weight"), E._conv_igemm_cpad(sd["conv_in.weight"], 64).to(bf))
        assert net.temb_off["down_blocks.1.resnets.0"] == 320 and net.temb_total == pk.shapes["temb_all.weight"][0][0]


def test_recipes_of_names_what_depends_on_a_module():
    net = SDNet("unet", 4, **TINY)
    tb = "down_blocks.0.attentions.0.transformer_blocks.0"
    names = lambda mods: [r.name for r in net.recipes_of(mods)]      # noqa: E731
    assert names([f"{tb}.attn1.to_k"]) == [f"{tb}.attn1.qkv.weight", f"{tb}.attn1.qkv.weight_kp"]
    assert names([f"{tb}.ff.net.2"]) == ["down_blocks.0.attentions.0.ff2_proj_out.weight"]
    assert names(["down_blocks.0.attentions.0.proj_out"]) == ["down_blocks.0.attentions.0.ff2_proj_out.weight"]
    assert names(["down_blocks.1.resnets.0.conv_shortcut"]) == ["down_blocks.1.resnets.0.conv2.weight"]
    assert names(["mid_block.resnets.1.time_emb_proj"]) == ["temb_all.weight"]
    assert names([f"{tb}.norm1"]) == []


# ------------------------------------------------------------------------------------------------ ABI
def test_lora_merge_bad_args_are_rejected_without_a_gpu():
    lib = L.lib()
    BAD = -1                                                            # PP_ERR_BAD_ARG
    assert lib.pp_lora_merge(None, None) == BAD
    a = L.PPLoraMergeArgs()
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # null pointers

    def ok_args():
        a = L.PPLoraMergeArgs()
        a.N, a.K, a.w, a.ldw, a.out, a.ldo, a.out_rows, a.out_cols, a.out_dtype = 64, 64, 0x1000, 64, 0x2000, 64, 64, 64, L.PP_DT_BF16
        return a

    a = ok_args()
    a.n_adapters = L.PP_LORA_MAX_ADAPTERS + 1
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # more than 8 adapters
    a = ok_args()
    a.n_adapters, a.rank[0], a.up[0], a.down[0] = 1, L.PP_LORA_MAX_RANK + 1, 0x3000, 0x4000
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # rank above 128
    a.rank[0] = 0
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD
    a.rank[0], a.up[0] = 8, None
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # a factor missing
    a = ok_args()
    a.row_off = 1
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # the block leaves the destination
    a = ok_args()
    a.col_mode, a.taps, a.cin_pad = L.PP_LORA_COLS_IGEMM, 9, 8
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # 64 is no multiple of 9 taps
    a = ok_args()
    a.col_mode, a.K, a.ldw = L.PP_LORA_COLS_KPERM, 48, 48
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD              # permutation groups of 32
    a = ok_args()
    a.out_dtype = 7
    assert lib.pp_lora_merge(ctypes.byref(a), None) == BAD
    assert ctypes.sizeof(L.PPLoraMergeArgs) == _c_sizeof()


def _c_sizeof():
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write('#include <stdio.h>\n#include "pp_hip.h"\nint main(){printf("%zu", sizeof(PPLoraMergeArgs));}')
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe])
        return int(subprocess.check_output([exe]))


# ------------------------------------------------------------------------------------------------ the text tower
def _rounded_once(p, w64):
    """p is the float64 value rounded once to fp32 (half an ulp; the float64 sum itself may associate differently)."""
    return bool(((p.double() - w64).abs() <= 2.0 ** -24 * w64.abs() + 1e-30).all())


def test_text_tower_merge_is_the_float64_merge_and_restores():
    from powerpaint_amd.models import CLIPTextModel
    torch.manual_seed(0)
    enc = CLIPTextModel(device="cpu", vocab_size=64, num_hidden_layers=2)
    tt = lora.text_targets(enc)
    assert len(tt) == 12
    w0 = {m + ".weight": dict(enc.named_modules())[m].weight.detach().clone() for m in tt}
    f1, f2 = make_factors(tt, w0, 4, seed=5, rel=0.2), make_factors(tt, w0, 2, seed=6, rel=0.2, alpha=1.0, modules=list(tt)[:5])
    stamp0 = enc._params_stamp()
    assert enc.merge_adapters(0.5) is False                            # no adapter: a scale is a no-op
    enc.load_lora_adapter(LoraAdapter(text_encoder=f1), "a")
    enc.load_lora_adapter(f2, "b")
    enc.set_adapters(["a", "b"], [1.0, -0.5])
    assert enc.merge_adapters(0.7) is True and enc.merge_adapters(0.7) is False
    assert enc._params_stamp() != stamp0                               # the tower repacks on its next forward
    want = merged_weights_f64(w0, [(f1, 1.0), (f2, -0.5)], 0.7)
    mods = dict(enc.named_modules())
    for k, w in want.items():
        assert _rounded_once(mods[k[:-7]].weight.detach(), w), k
    enc.set_adapters(["b"])
    enc.merge_adapters(1.0)
    want = merged_weights_f64(w0, [(f2, 1.0)], 1.0)
    for k in w0:
        assert _rounded_once(mods[k[:-7]].weight.detach(), want[k]) if k in want else torch.equal(mods[k[:-7]].weight.detach(), w0[k]), k
    # an adapter swapped under a kept name while another stays active: the new contents reach the parameters
    f3 = make_factors(tt, w0, 4, seed=7, rel=0.2)
    enc.set_adapters(["a", "b"])
    enc.merge_adapters(1.0)
    enc.delete_adapters("a")
    enc.load_lora_adapter(f3, "a")
    assert enc.active_adapters() == ["b", "a"]
    assert enc.merge_adapters(1.0) is True
    want = merged_weights_f64(w0, [(f2, 1.0), (f3, 1.0)], 1.0)
    for k in w0:
        assert _rounded_once(mods[k[:-7]].weight.detach(), want[k]), k
    enc.__dict__["lora_scale_fixed"] = 0.5            # what pipeline.fuse_lora(lora_scale=0.5) sets: later scales have no effect
    assert enc.merge_adapters(1.0) is True and enc.merge_adapters(0.3) is False
    want = merged_weights_f64(w0, [(f2, 1.0), (f3, 1.0)], 0.5)
    for k in w0:
        assert _rounded_once(mods[k[:-7]].weight.detach(), want[k]), k
    del enc.__dict__["lora_scale_fixed"]
    enc.delete_adapters(["a", "b"])
    for k in w0:
        assert torch.equal(mods[k[:-7]].weight.detach(), w0[k]), k
    with pytest.raises(L.PPError, match="matches no target"):
        enc.load_lora_adapter({"text_model.encoder.layers.9.mlp.fc1": f1["text_model.encoder.layers.0.mlp.fc1"]}, "c")
