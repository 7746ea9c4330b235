"""CPU: AsymmetricAutoencoderKL -- the published structure (state-dict shapes of both checkpoints' configs), what the
constructor refuses, the weight layout of the 4x4 stride-2 convolution, the loader's dispatch on `_class_name`, the launch
plans on a dry arena, and properties of the restatement (tests/asym_vae_cases.py) the GPU tests rely on."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import asym_vae_cases as AC
from powerpaint_amd import _lib as L
from powerpaint_amd.engine import Act, Arena, Builder
from powerpaint_amd.vae_asym import AsymVAENet, condition_channels, conv4x4_igemm

DOWN, UP = "DownEncoderBlock2D", "UpDecoderBlock2D"


def net_of(cfg, **kw):
    return AsymVAENet(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], cfg["down"], cfg["layers_down"],
                      cfg["up"], cfg["layers_up"], cfg["groups"], **kw)


def model_kwargs(cfg, **over):
    kw = dict(down_block_types=(DOWN,) * len(cfg["down"]), down_block_out_channels=cfg["down"],
              layers_per_down_block=cfg["layers_down"], up_block_types=(UP,) * len(cfg["up"]),
              up_block_out_channels=cfg["up"], layers_per_up_block=cfg["layers_up"], device="cpu")
    kw.update(over)
    return kw


def test_state_dict_spec_has_the_published_shapes():
    for cfg, want in ((AC.X15, AC.X15_CONDITION_WEIGHTS),
                      (AC.X2, [(256, 3, 3, 3), (512, 256, 3, 3), (1024, 512, 4, 4), (1024, 1024, 4, 4), (1024, 1024, 4, 4)])):
        sp = net_of(cfg).state_dict_spec()
        got = [sp[f"decoder.condition_encoder.layers.{l}.weight"] for l in range(5)]
        assert got == want == AC.condition_encoder_weight_shapes(cfg)              # published = the library's loop = the product
        assert [sp[f"decoder.condition_encoder.layers.{l}.bias"] for l in range(5)] == [(s[0],) for s in want]
        assert "decoder.condition_encoder.layers.5.weight" not in sp
        assert condition_channels(cfg["up"]) == AC.condition_encoder_channels(cfg["up"][0], cfg["up"][-1])
        up, lu = cfg["up"], cfg["layers_up"]
        assert sp["decoder.conv_in.weight"] == (up[-1], 4, 3, 3) and sp["decoder.conv_out.weight"] == (3, up[0], 3, 3)
        assert sp["decoder.mid_block.attentions.0.to_q.weight"] == (up[-1], up[-1])
        assert sp["encoder.mid_block.attentions.0.to_q.weight"] == (512, 512) and sp["encoder.conv_out.weight"] == (8, 512, 3, 3)
        for i in range(4):
            assert f"decoder.up_blocks.{i}.resnets.{lu}.conv2.weight" in sp
            assert f"decoder.up_blocks.{i}.resnets.{lu + 1}.conv2.weight" not in sp
            assert (f"decoder.up_blocks.{i}.upsamplers.0.conv.weight" in sp) == (i != 3)
            assert f"encoder.down_blocks.{i}.resnets.1.conv1.weight" in sp and f"encoder.down_blocks.{i}.resnets.2.conv1.weight" not in sp
        assert sp["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (up[1], up[2], 1, 1)
        assert sp["decoder.up_blocks.3.resnets.0.conv1.weight"] == (up[0], up[1], 3, 3)
        assert sp["quant_conv.weight"] == (8, 8, 1, 1) and sp["post_quant_conv.weight"] == (4, 4, 1, 1)
    # x-1-5: the SD-1.5 encoder (34.16 M) + the 1.5x decoder; the condition encoder alone is 21.0 M
    sp = net_of(AC.X15).state_dict_spec()
    n = lambda pre: sum(torch.Size(s).numel() for k, s in sp.items() if k.startswith(pre))      # noqa: E731
    assert n("decoder.condition_encoder.") == sum(torch.Size(s).numel() + s[0] for s in AC.X15_CONDITION_WEIGHTS)
    assert n("encoder.") + n("quant_conv.") == 34_163_592 + 72                   # the stock AutoencoderKL's encoder side


def test_constructor_refuses_by_name():
    from powerpaint_amd.models import AsymmetricAutoencoderKL, AutoencoderKL  # noqa: F401
    ok = AsymmetricAutoencoderKL(**model_kwargs(AC.TINY))
    assert ok.config.block_out_channels == AC.TINY["up"] and ok.config.force_upcast is False
    assert ok.config.down_block_out_channels == AC.TINY["down"] and ok.config.scaling_factor == 0.18215
    AsymmetricAutoencoderKL(**model_kwargs(AC.X15))
    AsymmetricAutoencoderKL(**model_kwargs(AC.X2))
    for over, word in ((dict(down_block_types=("AttnDownEncoderBlock2D", DOWN)), "AttnDownEncoderBlock2D"),
                       (dict(up_block_types=(UP, UP, UP, "AttnUpDecoderBlock2D")), "AttnUpDecoderBlock2D"),
                       (dict(act_fn="relu"), "act_fn"),
                       (dict(up_block_out_channels=(96, 192, 384, 384)), "multiples of 64"),
                       (dict(down_block_out_channels=(64, 100)), "multiples of 64"),
                       (dict(norm_num_groups=48), "norm_num_groups"),
                       (dict(up_block_out_channels=(64, 128, 256), up_block_types=(UP,) * 3), "four up blocks"),
                       (dict(up_block_out_channels=(64, 128, 128, 256)), "condition"),      # up[2] != min(4 up[0], up[3])
                       (dict(up_block_out_channels=(64, 192, 256, 256)), "condition"),      # up[1] != 2 up[0]
                       (dict(dtype=torch.float32), "bf16 or fp16")):
        with pytest.raises(L.PPError, match=word):
            AsymmetricAutoencoderKL(**model_kwargs(AC.TINY, **over))
    # the library's own defaults describe a one-block decoder, which cannot take a condition either
    with pytest.raises(L.PPError, match="four up blocks"):
        AsymmetricAutoencoderKL(device="cpu")
    with pytest.raises(L.PPError, match="load_state_dict"):
        ok.decode(torch.zeros(1, 4, 4, 4))
    ok.load_state_dict(ok.net.synthetic_state_dict(seed=1))
    with pytest.raises(ValueError, match="divisible by 8"):                      # image size the latents do not decode to
        ok.decode(torch.zeros(1, 4, 4, 4), image=torch.zeros(1, 3, 36, 32), mask=torch.zeros(1, 1, 36, 32))
    with pytest.raises(ValueError):
        ok.encode(torch.zeros(1, 3, 31, 32))
    bad = ok.net.synthetic_state_dict(seed=1)
    bad.pop("decoder.condition_encoder.layers.4.bias")
    with pytest.raises(L.PPError, match="condition_encoder.layers.4.bias"):
        ok.load_state_dict(bad)


def test_conv4x4_weight_layout_is_the_stride_2_convolution():
    """The [Cout][16 Cin] matrix pp_conv4x4s2 contracts, applied to the 16-tap im2col of the zero-padded input (column
    (4 ky + kx) Cin + c = pixel (2 oy - 1 + ky, 2 ox - 1 + kx), channel c), is F.conv2d(stride=2, padding=1): float64, 8 x 8."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 8, 8, generator=g, dtype=torch.float64)
    w = torch.randn(7, 5, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(7, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, b, stride=2, padding=1)
    xp = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1)                               # NHWC, padded
    rows = []
    for n in range(2):
        for oy in range(4):
            for ox in range(4):
                rows.append(torch.cat([xp[n, 2 * oy + ky, 2 * ox + kx] for ky in range(4) for kx in range(4)]))
    got = (torch.stack(rows) @ conv4x4_igemm(w).t() + b).reshape(2, 4, 4, 7).permute(0, 3, 1, 2)
    assert conv4x4_igemm(w).shape == (7, 80)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)


def test_plans_on_a_dry_arena():
    net = net_of(AC.X15)
    net.load_state_dict(net.synthetic_state_dict(seed=1), "cpu")
    B, h = 1, 64

    def build(cond):
        dry = Arena()
        pb = Builder(dry)
        z = Act(dry.alloc(B * h * h * 16), B, h, h, 8)
        out = dry.alloc(B * 4 * 512 * 512 * 4)
        kw = {}
        if cond:
            kw = dict(img8=Act(dry.alloc(B * 512 * 512 * 16), B, 512, 512, 8), mask=dry.alloc(B * 512 * 512 * 4), mask_hw=(512, 512))
        assert net.build_decode(pb, z, out, **kw) == (B, 4, 512, 512)
        return pb.plan

    pu, pc = build(False), build(True)
    nu, nc = [c[2] for c in pu.calls], [c[2] for c in pc.calls]
    # the conditioned plan = the unconditioned one + the condition encoder (direct conv, ReLU, GEMM conv, three 4x4 convs)
    assert nc[:1] == nu[:1] == ["zero_u64"]
    assert nc[1:7] == ["conv3x3_direct", "relu", "conv3x3", "conv4x4s2", "conv4x4s2", "conv4x4s2"] and nc[7:] == nu[1:]
    assert nu.count("mask_blend") == nc.count("mask_blend") == 5 and "conv4x4s2" not in nu and "relu" not in nu
    assert nu.count("conv3x3") == 2 * 18 + 3 and nu.count("softmax_rows") == 1
    # five norms read the blends' sums: 2 * 18 + 1 norms + the attention's, 5 of them without a statistics launch
    assert nu.count("groupnorm_apply") == 38 and nu.count("groupnorm_stats") == 33
    # what the 4x4 convs execute: all sixteen taps, 16 Cin Cout MACs per output pixel -- and no more
    want = 2.0 * 16 * (256 * 256 * 384 * 768 + 128 * 128 * 768 * 768 + 64 * 64 * 768 * 768)
    assert pc.flops_by_kind["conv4x4s2"] == want and pc.flops_skipped == 0
    layer1 = 2.0 * 9 * 512 * 512 * 192 * 384
    assert abs((pc.flops - pu.flops) - (want + layer1)) < 1e-6 * want
    assert 1.3e12 < want + layer1 < 1.45e12                                       # "about 1.4 TFLOP per image"
    # a decoder that cannot take a condition builds its unconditioned plan and refuses the other
    odd = AsymVAENet(down_block_out_channels=(64, 128), layers_per_down_block=1, up_block_out_channels=(64, 64), layers_per_up_block=1)
    assert "four up blocks" in odd.condition_mismatch()


def test_taps_name_every_block_and_keep_their_bytes():
    """`lay["taps"]` of the three plans, default (x-1-5) and TINY configuration: the names are the structure lists' in plan
    order (condition encoder first, a blend in front of every up block and behind the last), no tap's bytes are handed out
    again behind it, and a blend's tap is the tensor in front of it with its accumulator slot, one slot per blend."""
    from collections import defaultdict

    import vae_cases as VC
    from powerpaint_amd.vae_asym import AsymVAERuntime
    for cfg in (AC.X15, AC.TINY):
        net = net_of(cfg)
        net.P = defaultdict(lambda: 1 << 30)                                # pointers only: nothing runs on a dry arena
        s = 2 ** (len(cfg["down"]) - 1)
        for direction, (B, H, W) in (("decode", (2, 4, 6)), ("decode_cond", (2, 4, 6)), ("encode", (2, 4 * s, 6 * s))):
            lay, plan, log = VC.dry_build(AsymVAERuntime(net, "cpu", direction), B, H, W)
            taps = lay["taps"]
            assert [t[0] for t in taps] == VC.expected_tap_names(net, direction.split("_")[0], direction == "decode_cond")
            assert VC.tap_layout_violations(taps, log) == []
            accs = [t[2] for t in taps if len(t) == 3]
            assert len(accs) == (0 if direction == "encode" else 5) and len(set(accs)) == len(accs)
            assert [c[2] for c in plan.calls].count("mask_blend") == len(accs)


def test_loader_dispatches_on_class_name(tmp_path):
    from powerpaint_amd import loaders, models as PM
    c = AC.TINY
    net = net_of(c)
    cfg = dict(_class_name="AsymmetricAutoencoderKL", _diffusers_version="0.27.0", act_fn="silu", in_channels=3, out_channels=3,
               latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215,
               down_block_types=[DOWN] * 2, down_block_out_channels=list(c["down"]), layers_per_down_block=1,
               up_block_types=[UP] * 4, up_block_out_channels=list(c["up"]), layers_per_up_block=1)
    d = tmp_path / "pipe" / "vae"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(cfg))
    torch.save(net.synthetic_state_dict(seed=2), str(d / "diffusion_pytorch_model.bin"))
    vae = loaders.load_vae(str(tmp_path / "pipe"), device="cpu", torch_dtype=torch.float16)
    assert type(vae) is PM.AsymmetricAutoencoderKL and vae.net.dtype == torch.float16 and vae.net.params is not None
    assert vae.config.up_block_out_channels == c["up"] and vae.config.layers_per_up_block == 1
    assert type(PM.AsymmetricAutoencoderKL.from_pretrained(str(d), device="cpu")) is PM.AsymmetricAutoencoderKL
    # every other class name: the stock VAE, as before
    d2 = tmp_path / "pipe2" / "vae"
    d2.mkdir(parents=True)
    from powerpaint_amd.vae import VAENet
    small = dict(block_out_channels=[64, 128, 256, 256], layers_per_block=1)
    (d2 / "config.json").write_text(json.dumps(dict(_class_name="AutoencoderKL", **small)))
    torch.save(VAENet(**small).synthetic_state_dict(seed=2), str(d2 / "diffusion_pytorch_model.bin"))
    assert type(loaders.load_vae(str(tmp_path / "pipe2"), device="cpu")) is PM.AutoencoderKL
    assert loaders.config_class_name(str(d2)) == "AutoencoderKL"


def test_restatement_properties():
    """What the GPU structure tests assume of the published form, in float64: the nearest rule is F.interpolate's; a mask of ones
    is the unconditioned decode; a mask of zeros forgets the latents; the blend is linear in the mask."""
    m = torch.rand(2, 1, 24, 40)
    for h, w in ((24, 40), (12, 20), (6, 10), (3, 5)):
        assert torch.equal(AC.nearest_mask(m, h, w), F.interpolate(m, size=(h, w), mode="nearest"))
    cfg = AC.TINY
    sd = {k: v.double() for k, v in net_of(cfg).synthetic_state_dict(seed=4).items()}
    g = torch.Generator().manual_seed(1)
    z, z2 = torch.randn(2, 4, 3, 5, generator=g, dtype=torch.float64), torch.randn(2, 4, 3, 5, generator=g, dtype=torch.float64)
    img = torch.rand(2, 3, 24, 40, generator=g, dtype=torch.float64) * 2 - 1
    ones, zeros = torch.ones(2, 1, 24, 40, dtype=torch.float64), torch.zeros(2, 1, 24, 40, dtype=torch.float64)
    with torch.no_grad():
        u = AC.decode(sd, cfg, z)
        assert u.shape == (2, 3, 24, 40)
        assert torch.equal(AC.decode(sd, cfg, z, img, ones), u)
        assert torch.equal(AC.decode(sd, cfg, z, img, zeros), AC.decode(sd, cfg, z2, img, zeros))
        mk = AC.two_masks(2, 24, 40).double()
        c = AC.decode(sd, cfg, z, img, mk)
        cos = F.cosine_similarity(c.flatten(), u.flatten(), dim=0).item()
        assert cos < 0.99, cos                                 # the condition matters: a product that ignored it would fail the gate
        assert AC.encode_moments(sd, cfg, img).shape == (2, 8, 12, 20)
