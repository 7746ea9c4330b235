"""Shared by the IP-Adapter mask tests and the fixture generator (not a test file; nothing here is imported by the product).

`ip_adapter_masks` as diffusers 0.27 runs them: `cross_attention_kwargs={"ip_adapter_masks": m}` with m ONE tensor
[num_adapters, 1, H, W] reaches every attn2's IPAdapterAttnProcessor2_0, which multiplies adapter i's attention output
a_i [B, nq, C] by `IPAdapterMaskProcessor.downsample(m[i], B, nq, C)` in front of `hidden += scale_i * (a_i * w_i)`.
diffusers is not a dependency of this repository and the reference tree does not carry the processor, so the rule is RESTATED
here from its contract -- parity with the library is unpinned until tests/test_diffusers_pin_ip_adapter_masks.py runs
somewhere diffusers imports.

  * `downsample`: the restated rule (bicubic, unclamped, the mask's own aspect ratio, zero pad / cut to nq).
  * `MaskedIPAttention(IC.IPAttention)`: each adapter's term times its weights.
  * `MaskedIPUNet(IC.IPUNet)`: takes the masks out of `cross_attention_kwargs`, checks them as the processor does, hands the
    rest to the oracle UNet.
  * `kernel_weights` / `kernel_ref` / `kernel_gate`: pp_ip_attn_add_masked against float64.

The kernel's gate.  The masked entry computes, per element, fl16(o + ((s w_r) / l) acc) where the unmasked one computes
fl16(o + (s / l) acc): ONE more fp32 operation, the product s w_r, relative error at most u = 2^-24 on the term
|s w_r| sum_j |p_j v_j|.  With the magnitude taken at the row's effective scale, mag_r = |o| + |s w_r| sum_j |p_j v_j| (that
is IC.kernel_ref's `mag` with ip_scale -> s w_r), the bound of tests/test_ip_adapter_gpu.py's docstring holds term for term --
r16 |ref| for the one rounding at the store and u (2 (d + 2) S + nk + 40) mag_r for the fp32 evaluation, neither of which
sees the weight except as a factor of the term -- plus u mag_r for the extra product:

    |out - ref| <= IC.kernel_gate(ref, mag_r, S, d, nk, dtype) + u mag_r

A row with w_r = 0 is not part of this: its bits must be o's (asserted separately).  Nothing in the gate comes from the
kernel's output.
"""
import math
import warnings

import torch

import ip_adapter_cases as IC

MASK_HW = (128, 128)          # the fixture's image size (16x16 latents)


def downsample(mask, batch_size, num_queries, value_embed_dim):
    """mask [1, H, W] -> [batch_size, num_queries, value_embed_dim] (the issue's restatement of diffusers 0.27)."""
    o_h, o_w = mask.shape[1], mask.shape[2]
    ratio = o_w / o_h
    mask_h = int(math.sqrt(num_queries / ratio))
    mask_h = int(mask_h) + int((num_queries % int(mask_h)) != 0)
    mask_w = num_queries // mask_h
    m = torch.nn.functional.interpolate(mask.unsqueeze(0), size=(mask_h, mask_w), mode="bicubic").squeeze(0)
    if batch_size < m.shape[0]:
        m = m[:batch_size]
    elif batch_size > m.shape[0]:
        m = m.repeat(batch_size, 1, 1)
    m = m.view(m.shape[0], -1)
    area = mask_h * mask_w
    if area < num_queries:
        warnings.warn("The aspect ratio of the mask does not match the aspect ratio of the output image. "
                      "Please update your masks or adjust the output size for optimal performance.", UserWarning)
        m = torch.nn.functional.pad(m, (0, num_queries - m.shape[1]), value=0.0)
    if area > num_queries:
        warnings.warn("The aspect ratio of the mask does not match the aspect ratio of the output image. "
                      "Please update your masks or adjust the output size for optimal performance.", UserWarning)
        m = m[:, :num_queries]
    return m.reshape(m.shape[0], m.shape[1], 1).repeat(1, 1, value_embed_dim)


def check_masks(masks, n_adapters):
    """The two refusals of the processor (texts from memory: the pin test compares them)."""
    if not isinstance(masks, torch.Tensor) or masks.ndim != 4:
        raise ValueError(" ip_adapter_mask should be a tensor with shape [num_ip_adapter, 1, height, width]."
                         " Please use `IPAdapterMaskProcessor` to preprocess your mask")
    if len(masks) != n_adapters:
        raise ValueError(f"Number of ip_adapter_masks ({len(masks)}) must match number of IP-Adapters ({n_adapters})")


class MaskedIPAttention(IC.IPAttention):
    """IC.IPAttention with `self.ip_masks` ([n, 1, H, W] or None): a_i * downsample(mask_i, B, nq, C) per adapter."""
    ip_masks = None

    def forward(self, x, ctx=None):
        if self.ip_masks is None:
            return super().forward(x, ctx)
        text, ips = ctx
        check_masks(self.ip_masks, len(self.scale))
        q = self._heads(self.to_q(x))
        a = self._sdpa(q, self._heads(self.to_k(text)), self._heads(self.to_v(text)))
        for e, wk, wv, s, m in zip(ips, self.to_k_ip, self.to_v_ip, self.scale, self.ip_masks):
            ai = self._sdpa(q, self._heads(wk(e)), self._heads(wv(e)))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                w = downsample(m, ai.shape[0], ai.shape[1], ai.shape[2])
            a = a + s * (ai * w.to(dtype=ai.dtype, device=ai.device))
        return self.to_out[0](a)


class MaskedIPUNet(IC.IPUNet):
    """IC.IPUNet whose attn2s are MaskedIPAttentions; `cross_attention_kwargs["ip_adapter_masks"]` is taken out of the call and
    bound to them, the rest goes to the oracle UNet as it came."""

    def __init__(self, unet, state_dicts, scales):
        super().__init__(unet, state_dicts, scales)
        as_masked(self)

    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, cross_attention_kwargs=None, **kw):
        rest = dict(cross_attention_kwargs or {})
        masks = rest.pop("ip_adapter_masks", None)
        if masks is not None:
            check_masks(masks, len(self.ip_modules[0].scale))
        for m in self.ip_modules:
            m.ip_masks = masks
        try:
            if cross_attention_kwargs is not None and (rest or kw):
                kw["cross_attention_kwargs"] = rest or None
            return super().forward(sample, timestep, encoder_hidden_states, added_cond_kwargs=added_cond_kwargs, **kw)
        finally:
            for m in self.ip_modules:
                m.ip_masks = None


def as_masked(ipu):
    """Any IC.IPUNet (ip_plus_cases.PlusIPUNet included: it differs in its constructor only) -> the same object as a
    MaskedIPUNet over MaskedIPAttentions."""
    for m in ipu.ip_modules:
        m.__class__ = MaskedIPAttention
    ipu.__class__ = MaskedIPUNet
    return ipu


# ---------------------------------------------------------------------------------------------------------------- fixture
# name -> (ip_adapter_cases case: adapters / scales / embeds, mask variant)
CASES = dict(one=("one", 0), two=("two", 0), one_b=("one", 1))


def rect_mask(h, w, top, left, bottom, right):
    m = torch.zeros(1, h, w)
    m[:, top:bottom, left:right] = 1.0
    return m


def case_masks(name, hw=MASK_HW):
    """[n, 1, H, W] binary masks of a fixture case: `one` a rectangle in the upper left, `one_b` another in the lower right,
    `two` the left and the right half (complementary)."""
    H, W = hw
    if name == "one":
        return rect_mask(H, W, H // 8, W // 8, H // 2, 5 * W // 8).unsqueeze(0)
    if name == "one_b":
        return rect_mask(H, W, H // 2, 3 * W // 8, 15 * H // 16, W).unsqueeze(0)
    left = rect_mask(H, W, 0, 0, H, W // 2)
    return torch.stack([left, 1.0 - left])


# ---------------------------------------------------------------------------------------------------------------- kernel
W_PATTERN = [0.5, 1.0, -0.09375, 1.09375, 0.25, 1.0, 0.75]
W_ZERO_RUNS = [(3, 10), (17, 47), (53, 58), (70, 83)]       # lengths 7, 30, 5, 13: no multiple of the 12-row group of one
#                                                             40-channel head; [24, 48) are two whole groups of it, skipped


def kernel_weights(nq):
    """fp32 [nq]: 1.0, fractions, the bicubic overshoots -0.09375 / 1.09375, and runs of exact zeros."""
    w = torch.tensor([W_PATTERN[r % len(W_PATTERN)] for r in range(nq)], dtype=torch.float32)
    for a, b in W_ZERO_RUNS:
        w[a:b] = 0.0
    return w


def kernel_ref(q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale, w):
    """IC.kernel_ref with ip_scale * w_r per row, float64 -> (ref, mag, smax); w: fp32 [nq], shared by the batch items."""
    one, mag1, smax = IC.kernel_ref(q, k, v, o, batch, heads, d, nq, nk, qk_scale, 1.0)
    od = o[:, :heads * d].double()
    a, absa = one - od, mag1 - od.abs()              # sum_j p_j v_j and sum_j |p_j v_j| (float64: exact to 2^-53)
    s = (float(torch.tensor(ip_scale, dtype=torch.float32)) * w.double()).repeat(batch).unsqueeze(1)
    return od + s * a, od.abs() + s.abs() * absa, smax


def kernel_gate(ref, mag, smax, d, nk, dtype):
    """Per-element bound on |kernel - ref| (derived in the module docstring)."""
    return IC.kernel_gate(ref, mag, smax, d, nk, dtype) + IC.U32 * mag
