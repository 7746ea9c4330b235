"""CPU: AutoencoderTiny (TAESD) -- the published key and shape list, the config defaults, what the constructor refuses, the
loader's dispatch on `_class_name`, the pack-time fold of `2 y - 1`, the latent scaling and forward()'s quantisation against
the restatement (tests/taesd_cases.py), `_vae_encode` on a VAE without a posterior, and the launch plans on a dry arena."""
import json

import pytest
import torch
import torch.nn.functional as F

import taesd_cases as TC
from powerpaint_amd import _lib as L
from powerpaint_amd.engine import Arena
from powerpaint_amd.vae_tiny import TinyVAENet, TinyVAERuntime

C = (64, 64, 3, 3)


def test_state_dict_spec_is_the_published_list():
    want = {"encoder.layers.0.weight": (64, 3, 3, 3), "encoder.layers.0.bias": (64,),
            "encoder.layers.14.weight": (4, 64, 3, 3), "encoder.layers.14.bias": (4,),
            "decoder.layers.0.weight": (64, 4, 3, 3), "decoder.layers.0.bias": (64,),
            "decoder.layers.18.weight": (3, 64, 3, 3), "decoder.layers.18.bias": (3,)}
    for i in (2, 6, 10):                                       # stride-2 convs: no bias
        want[f"encoder.layers.{i}.weight"] = C
    for i in (6, 11, 16):                                      # the convs behind the Upsamples (5, 10, 15): no bias
        want[f"decoder.layers.{i}.weight"] = C
    for side, blocks in (("encoder", (1, 3, 4, 5, 7, 8, 9, 11, 12, 13)), ("decoder", (2, 3, 4, 7, 8, 9, 12, 13, 14, 17))):
        for i in blocks:
            for c in (0, 2, 4):
                want[f"{side}.layers.{i}.conv.{c}.weight"] = C
                want[f"{side}.layers.{i}.conv.{c}.bias"] = (64,)
    got = TinyVAENet().state_dict_spec()
    assert got == want == TC.spec(TC.DEFAULT)
    assert len(want) == 8 + 6 + 2 * 10 * 6
    # the parameterless layers have no keys: the decoder's ReLU (1) and the Upsamples
    assert not any(k.startswith(f"decoder.layers.{i}.") for k in got for i in (1, 5, 10, 15))
    # other block counts: any tuple of positive ints
    small = TinyVAENet(num_encoder_blocks=TC.SMALL["enc_blocks"], num_decoder_blocks=TC.SMALL["dec_blocks"])
    assert small.state_dict_spec() == TC.spec(TC.SMALL)
    assert "encoder.layers.2.weight" in TC.spec(TC.SMALL) and "encoder.layers.5.bias" in TC.spec(TC.SMALL)
    sd = TinyVAENet().synthetic_state_dict(seed=0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_config_defaults():
    from powerpaint_amd.models import AutoencoderTiny
    c = AutoencoderTiny(device="cpu").config
    assert (c.in_channels, c.out_channels, c.latent_channels, c.upsampling_scaling_factor) == (3, 3, 4, 2)
    assert c.encoder_block_out_channels == c.decoder_block_out_channels == c.block_out_channels == (64,) * 4
    assert (c.act_fn, c.upsample_fn) == ("relu", "nearest")
    assert c.num_encoder_blocks == (1, 3, 3, 3) and c.num_decoder_blocks == (3, 3, 3, 1)
    assert (c.latent_magnitude, c.latent_shift, c.force_upcast, c.scaling_factor) == (3, 0.5, False, 1.0)
    assert 2 ** (len(c.block_out_channels) - 1) == 8              # what the pipelines compute vae_scale_factor from


def test_constructor_refuses_by_name():
    from powerpaint_amd.models import AutoencoderTiny
    AutoencoderTiny(device="cpu", num_encoder_blocks=(1, 2), num_decoder_blocks=(2, 1), encoder_block_out_channels=(64, 64),
                    decoder_block_out_channels=(64, 64))
    for over, word in ((dict(encoder_block_out_channels=(64, 128, 64, 64)), r"encoder_block_out_channels=\(64, 128, 64, 64\)"),
                       (dict(decoder_block_out_channels=(32,) * 4), r"decoder_block_out_channels=\(32, 32, 32, 32\)"),
                       (dict(act_fn="swish"), "act_fn='swish'"),
                       (dict(upsample_fn="bilinear"), "upsample_fn='bilinear'"),
                       (dict(upsampling_scaling_factor=4), "upsampling_scaling_factor=4"),
                       (dict(latent_channels=16), "latent_channels=16"),
                       (dict(num_encoder_blocks=(1, 0, 3, 3)), r"num_encoder_blocks=\(1, 0, 3, 3\)"),
                       (dict(num_decoder_blocks=(3, 3, 1)), r"num_decoder_blocks=\(3, 3, 1\)"),
                       (dict(dtype=torch.float32), "bf16 or fp16")):
        with pytest.raises(L.PPError, match=word):
            AutoencoderTiny(device="cpu", **over)
    vae = AutoencoderTiny(device="cpu")
    with pytest.raises(L.PPError, match="enable_tiling"):
        vae.enable_tiling()
    with pytest.raises(L.PPError, match="enable_slicing"):
        vae.enable_slicing()
    with pytest.raises(L.PPError, match="load_state_dict first"):
        vae.decode(torch.zeros(1, 4, 2, 2))
    sd = vae.net.synthetic_state_dict(seed=1)
    sd.pop("decoder.layers.6.weight")
    with pytest.raises(L.PPError, match="decoder.layers.6.weight"):
        vae.load_state_dict(sd)


def test_loader_dispatches_on_class_name(tmp_path):
    from powerpaint_amd import loaders, models as PM
    cfg = dict(_class_name="AutoencoderTiny", _diffusers_version="0.27.0", act_fn="relu", in_channels=3, out_channels=3,
               latent_channels=4, encoder_block_out_channels=[64] * 4, decoder_block_out_channels=[64] * 4,
               num_encoder_blocks=[1, 3, 3, 3], num_decoder_blocks=[3, 3, 3, 1], upsampling_scaling_factor=2,
               latent_magnitude=3, latent_shift=0.5, force_upcast=False, scaling_factor=1.0)
    d = tmp_path / "pipe" / "vae"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(cfg))
    torch.save(TinyVAENet().synthetic_state_dict(seed=2), str(d / "diffusion_pytorch_model.bin"))
    vae = loaders.load_vae(str(tmp_path / "pipe"), device="cpu", torch_dtype=torch.float16)
    assert type(vae) is PM.AutoencoderTiny and vae.net.dtype == torch.float16 and vae.net.params is not None
    assert vae.config.num_decoder_blocks == (3, 3, 3, 1) and vae.config.scaling_factor == 1.0
    assert loaders.load_vae(str(tmp_path / "pipe"), device="cpu").net.dtype == torch.bfloat16
    assert type(PM.AutoencoderTiny.from_pretrained(str(d), device="cpu")) is PM.AutoencoderTiny


def test_fold_of_the_output_map_is_exact():
    """decode's 2 y - 1 as (2 w, 2 b - 1) of the last conv: the same float64 value, and 2 w is exact in either 16-bit format."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(3, 64, 3, 3, generator=g, dtype=torch.float64) / 24
    b = torch.randn(3, generator=g, dtype=torch.float64)
    a, f = 2 * F.conv2d(x, w, b, padding=1) - 1, F.conv2d(x, 2 * w, 2 * b - 1, padding=1)
    assert (a - f).abs().max() <= 1e-13 * a.abs().max()
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal((2 * w.float()).to(dt), 2 * w.float().to(dt))
    # ... and it is what load_state_dict packs: [4][9 * 64] rows of 2 w (row 3 zero), bias 2 b - 1 (entry 3 zero)
    net = TinyVAENet(dtype=torch.float16)
    sd = net.synthetic_state_dict(seed=4)
    net.load_state_dict(sd, "cpu")
    wp, bp = net.params.tensor("decoder.layers.18.weight"), net.params.tensor("decoder.layers.18.bias")
    want = (2 * sd["decoder.layers.18.weight"]).permute(0, 2, 3, 1).reshape(3, -1).to(torch.float16)
    assert torch.equal(wp[:3], want) and bool((wp[3] == 0).all())
    assert torch.equal(bp[:3], 2 * sd["decoder.layers.18.bias"] - 1) and bp[3] == 0
    # the encoder's last conv is packed as it is
    assert torch.equal(net.params.tensor("encoder.layers.14.bias"), sd["encoder.layers.14.bias"])


def test_latent_scaling_and_quantisation_follow_the_restatement():
    from powerpaint_amd.models import AutoencoderTiny
    vae = AutoencoderTiny(device="cpu")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 6, 5, generator=g) * 3
    x[0, 0, 0, :4] = torch.tensor([-3.0, 3.0, -40.0, 40.0])
    assert torch.equal(vae.scale_latents(x), TC.scale_latents(x)) and torch.equal(vae.unscale_latents(x), TC.unscale_latents(x))
    s = vae.scale_latents(x)
    assert s.min() == 0 and s.max() == 1 and s[0, 0, 0, 0] == 0 and s[0, 0, 0, 1] == 1
    assert torch.allclose(vae.unscale_latents(vae.scale_latents(x.clamp(-3, 3))), x.clamp(-3, 3), atol=1e-6)
    # forward(): what decode receives is the restatement's quantisation of what encode returned
    seen = {}
    vae.encode = lambda im: type("O", (), {"latents": x})()
    vae.decode = lambda z, return_dict=True: seen.setdefault("z", z)
    vae.forward(torch.zeros(2, 3, 48, 40))
    assert torch.equal(seen["z"], TC.quantise(x))
    q = TC.scale_latents(TC.quantise(x)) * 255
    assert (q - q.round()).abs().max() < 1e-4 and len(torch.unique(q.round())) > 50          # 256 levels, many of them hit


def test_vae_encode_takes_latents_and_leaves_the_generator():
    from powerpaint_amd import pipelines as PP
    from powerpaint_amd.models._base import Output
    from powerpaint_amd.models.autoencoder_kl import DiagonalGaussianDistribution
    from types import SimpleNamespace
    lat = torch.arange(2 * 4 * 3 * 3, dtype=torch.float32).view(2, 4, 3, 3)

    class Tiny:
        config = SimpleNamespace(scaling_factor=0.5)

        def encode(self, x):
            return Output(latents=lat[:x.shape[0]])

    class KL:
        config = SimpleNamespace(scaling_factor=0.5)

        def encode(self, x):
            return Output(latent_dist=DiagonalGaussianDistribution(torch.zeros(x.shape[0], 8, 3, 3)))

    img = torch.zeros(2, 3, 24, 24)
    pipe = PP.StableDiffusionInpaintPipeline(vae=None)
    pipe.vae = Tiny()
    g = torch.Generator().manual_seed(7)
    before = g.get_state().clone()
    assert torch.equal(pipe._vae_encode(img, g), 0.5 * lat)
    assert torch.equal(g.get_state(), before)                                       # byte-identical: nothing was drawn
    gl = [torch.Generator().manual_seed(8), torch.Generator().manual_seed(9)]
    states = [x.get_state().clone() for x in gl]
    assert torch.equal(pipe._vae_encode(img, gl), 0.5 * torch.cat([lat[:1], lat[:1]]))
    assert all(torch.equal(x.get_state(), s) for x, s in zip(gl, states))
    # with a posterior it draws as before: mean 0, std 1 -> the generator's own normal draw, scaled
    pipe.vae = KL()
    g, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    assert torch.equal(pipe._vae_encode(img, g), 0.5 * torch.randn(2, 4, 3, 3, generator=g2))
    assert torch.equal(g.get_state(), g2.get_state()) and not torch.equal(g.get_state(), before)
    with pytest.raises(AttributeError, match="latent_dist"):
        PP._base.retrieve_latents(Output(sample=lat))


DECODE_ORDER = (["taesd_pack", "conv3x3_direct", "relu"] + ["conv3x3_c64"] * 9 + ["conv3x3_c64"] + ["conv3x3_c64"] * 9 +
                ["conv3x3_c64"] + ["conv3x3_c64"] * 9 + ["conv3x3_c64"] + ["conv3x3_c64"] * 3 + ["conv_out"])
ENCODE_ORDER = ["taesd_pack", "conv3x3_direct"] + ["conv3x3_c64"] * 33 + ["conv_out"]


def _modes(plan):
    """(mode, relu, has bias, has residual) of every pp_conv3x3_c64 launch."""
    return [(a[7], a[8], a[5] is not None, a[6] is not None) for _, a, n in plan.calls if n == "conv3x3_c64"]


def test_plans_on_a_dry_arena():
    net = TinyVAENet()
    net.load_state_dict(net.synthetic_state_dict(seed=1), "cpu")
    blk = [(0, 1, True, False), (0, 1, True, False), (0, 1, True, True)]
    for direction, (B, H, W), order, shape in (("decode", (2, 8, 12), DECODE_ORDER, (2, 4, 64, 96)),
                                               ("encode", (2, 64, 96), ENCODE_ORDER, (2, 4, 8, 12))):
        rt = TinyVAERuntime(net, "cpu", direction)
        dry = Arena()
        lay, plan = rt._build(dry, B, H, W)
        names = [c[2] for c in plan.calls]
        assert names == order and len(names) == (37 if direction == "decode" else 36)
        assert lay["shape"] == shape
        taps = lay["taps"]
        assert len(taps) == len(names) and len({t[0] for t in taps}) == len(taps)        # one tap per launch
        up, down = (2, 0, False, False), (1, 0, False, False)
        if direction == "decode":
            assert _modes(plan) == blk * 3 + [up] + blk * 3 + [up] + blk * 3 + [up] + blk
            assert [t[0] for t in taps][:6] == ["pack", "decoder.layers.0", "decoder.layers.1", "decoder.layers.2.conv.0",
                                                "decoder.layers.2.conv.2", "decoder.layers.2.conv.4"]
            assert [t[0] for t in taps][-2:] == ["decoder.layers.17.conv.4", "decoder.layers.18"]
            assert (taps[12][0], taps[12][1].H, taps[12][1].W) == ("decoder.layers.6", 16, 24)
            assert plan.calls[0][1][6] == 1                                               # latents: 3 tanh(z / 3)
        else:
            assert _modes(plan) == blk + [down] + blk * 3 + [down] + blk * 3 + [down] + blk * 3
            assert (taps[5][0], taps[5][1].H, taps[5][1].W) == ("encoder.layers.2", 32, 48)
            assert plan.calls[0][1][6] == 0                                               # image: (x + 1) / 2
        # the taps keep their bytes: no two of them overlap, none overlaps the input staging or the output
        spans = sorted([(lay["src"], lay["src"] + 4 * B * (4 if direction == "decode" else 3) * H * W)] +
                       [(t[1].ptr, t[1].ptr + t[1].nbytes) for t in taps])
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        # what the 64 -> 64 convs execute: 2 * 576 * 64 FLOP per output pixel (73.7 kFLOP), nothing else is counted
        assert plan.flops == 2.0 * 9 * 64 * 64 * sum(t[1].rows for t, n in zip(taps, names) if n == "conv3x3_c64")
    # odd image sides: the stride-2 convs take the ceil half, as the published convs do
    rt = TinyVAERuntime(net, "cpu", "encode")
    assert rt._build(Arena(), 1, 21, 35)[0]["shape"] == (1, 4, 3, 5)
    # other block counts
    small = TinyVAENet(num_encoder_blocks=(1, 2), num_decoder_blocks=(2, 1))
    small.load_state_dict(small.synthetic_state_dict(seed=1), "cpu")
    lay, plan = TinyVAERuntime(small, "cpu", "decode")._build(Arena(), 1, 4, 4)
    assert lay["shape"] == (1, 4, 8, 8) and len(plan.calls) == 3 + 6 + 1 + 3 + 1


def test_restatement_properties():
    """The restatement itself: shapes, the rounded variant differs from the pure one but stays close, forward = decode of the
    quantised encode, decode is bounded by the tanh clamp (3 tanh(z / 3) saturates)."""
    cfg = TC.SMALL
    net = TinyVAENet(num_encoder_blocks=cfg["enc_blocks"], num_decoder_blocks=cfg["dec_blocks"])
    sd = TC.as_double(net.synthetic_state_dict(seed=4))
    g = torch.Generator().manual_seed(1)
    img = torch.rand(2, 3, 10, 14, generator=g, dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        lat = TC.encode(sd, cfg, img)
        assert lat.shape == (2, 4, 5, 7)
        out = TC.forward(sd, cfg, img)
        assert out.shape == (2, 3, 10, 14) and torch.equal(out, TC.decode(sd, cfg, TC.quantise(lat)))
        r = TC.rounder(torch.bfloat16)
        lr = TC.encode(TC.rounded_weights(sd, torch.bfloat16), cfg, img, r)
        assert not torch.equal(lr, lat) and F.cosine_similarity(lr.flatten(), lat.flatten(), dim=0) > 0.999
        big = torch.full((1, 4, 2, 2), 1e6, dtype=torch.float64)
        assert torch.equal(TC.decode(sd, cfg, big), TC.decode(sd, cfg, big * 10))
