"""Parity pin: the restated IP-Adapter pieces of tests/ip_adapter_cases.py against diffusers itself (0.27.0 is the version the
reference pins).  Skipped where diffusers is not installed -- tests/golden/README_ip_adapter.md says "parity unpinned until this
runs".  Three questions: is `IPAttention` the arithmetic of `IPAdapterAttnProcessor2_0`, is `MultiProjection` over
`ImageProjection` that of `MultiIPAdapterImageProjection`, and does `unet._load_ip_adapter_weights` number the cross-attentions
the way `SDNet.ip_attn_order` says (down blocks, up blocks, mid block; index 2 k + 1)."""
import os
import sys

import pytest
import torch

diffusers = pytest.importorskip("diffusers")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ip_adapter_cases as IC  # noqa: E402

TINY = dict(block_out_channels=(320, 640), layers_per_block=1, cross_attention_dim=768, attention_head_dim=8,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))


def test_ip_attention_is_the_diffusers_processor():
    from diffusers.models.attention_processor import Attention, IPAdapterAttnProcessor2_0
    from oracle import sd_modules as OM
    torch.manual_seed(0)
    o = OM.Attention(320, 768, 8, 40)
    m = IC.IPAttention(o, 2).eval()
    m.scale = [0.7, 0.4]
    a = Attention(query_dim=320, cross_attention_dim=768, heads=8, dim_head=40, bias=False)
    proc = IPAdapterAttnProcessor2_0(hidden_size=320, cross_attention_dim=768, num_tokens=(4, 8), scale=[0.7, 0.4])
    a.set_processor(proc)
    a.load_state_dict({k: v for k, v in o.state_dict().items()}, strict=False)
    with torch.no_grad():
        for i in range(2):
            proc.to_k_ip[i].weight.copy_(m.to_k_ip[i].weight)
            proc.to_v_ip[i].weight.copy_(m.to_v_ip[i].weight)
    g = torch.Generator().manual_seed(1)
    x, text = torch.randn(2, 64, 320, generator=g), torch.randn(2, 77, 768, generator=g)
    ips = [torch.randn(2, 4, 768, generator=g), torch.randn(2, 8, 768, generator=g)]
    with torch.no_grad():
        want = a(x, encoder_hidden_states=(text, ips))
        got = m(x, (text, ips))
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), float((got - want).abs().max())


def test_multi_projection_is_the_diffusers_module():
    from diffusers.models.embeddings import ImageProjection, MultiIPAdapterImageProjection
    torch.manual_seed(2)
    mine = [IC.ImageProjection(32, 768, 4), IC.ImageProjection(64, 768, 8)]
    theirs = [ImageProjection(image_embed_dim=32, cross_attention_dim=768, num_image_text_embeds=4),
              ImageProjection(image_embed_dim=64, cross_attention_dim=768, num_image_text_embeds=8)]
    for a, b in zip(mine, theirs):
        b.load_state_dict(a.state_dict())
    g = torch.Generator().manual_seed(3)
    embeds = [torch.randn(2, 1, 32, generator=g), torch.randn(2, 2, 64, generator=g)]
    with torch.no_grad():
        want = MultiIPAdapterImageProjection(theirs)(embeds)
        got = IC.MultiProjection(mine)(embeds)
    assert all(torch.allclose(x, y, atol=1e-6) for x, y in zip(got, want))


def test_key_order_is_the_one_load_ip_adapter_weights_uses():
    from oracle import sd_modules as OM
    from powerpaint_amd.engine import SDNet
    u = diffusers.UNet2DConditionModel(in_channels=4, out_channels=4, **TINY)
    o = OM.UNet2DConditionModel(in_channels=4, **{k: v for k, v in TINY.items()})
    sd = IC.adapter_state_dict(o, 5)
    u._load_ip_adapter_weights([sd])
    net = SDNet("unet", 4, block_out_channels=TINY["block_out_channels"], layers_per_block=1,
                down_block_types=TINY["down_block_types"], up_block_types=TINY["up_block_types"])
    procs = [(n, p) for n, p in u.attn_processors.items()]
    cross = [(i, n) for i, (n, p) in enumerate(procs) if "attn2" in n]
    assert [n.split(".transformer_blocks")[0] for _, n in cross] == net.ip_attn_order()
    for k, (i, n) in enumerate(cross):
        assert i == 2 * k + 1
        assert torch.equal(procs[i][1].to_k_ip[0].weight, sd["ip_adapter"][f"{i}.to_k_ip.weight"])
