// The kernels AsymmetricAutoencoderKL (diffusers-0.27 autoencoder_asym_kl.py; vae.py: MaskConditionEncoder /
// MaskConditionDecoder -- the asymmetric VQGAN of Zhu et al., arXiv:2306.04632) adds to the VAE path:
//   pp_conv4x4s2         the 4x4 stride-2 pad-1 convolution of the condition encoder's layers 2..4, an implicit GEMM on the
//                        matrix cores over all 16 taps (K = 16 Cin); optional ReLU on the operand as it is loaded, so the
//                        pre-ReLU tensor the decoder's blends read is the only copy
//   pp_relu              the one ReLU that has no loader to live in (layer 0 -> layer 1, a conv of the stock GEMM)
//   pp_masked_image_pack (1 - mask) * image, fp32 NCHW -> the 8-channel NHWC image pp_conv3x3_direct reads
//   pp_mask_blend        sample * m + cond * (1 - m) at the nearest-resampled mask pixel, + the (sum, sum of squares) of what
//                        it stored for the GroupNorm behind it, in the fixed point of PPGemmArgs.gn_acc
#include "pp_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// conv 4x4, stride 2, pad 1:  out[b][oy][ox][n] = bias[n] + sum_{ky,kx,c} act(x[b][2 oy - 1 + ky][2 ox - 1 + kx][c]) w[n][(4 ky + kx) Cin + c]
// 128 (pixels) x 128 (out channels) tile per 256-thread workgroup, 64-deep K steps (one tap x 64 channels: Cin % 64 == 0),
// operands through registers into two LDS buffers (the loader zero-fills the padding and applies the ReLU, which an
// LDS-DMA cannot), one barrier per step.  The weights are the MFMA's A operand, the pixels its B operand: the accumulator
// then holds four consecutive out channels of one pixel per register quad -> 8-byte stores.
// ------------------------------------------------------------------------------------------------------------------
constexpr int C4_T = 256;
constexpr int C4_BM = 128;   // output pixels per tile
constexpr int C4_BN = 128;   // out channels per tile
constexpr int C4_BK = 64;
constexpr int C4_TILE_CHUNKS = 128 * (C4_BK / 8);   // 16-byte chunks of one operand tile
constexpr int C4_GROUP_M = 8;                       // pixel panels per group of the tile order (tile_order.h)

struct Conv4Args {
  const uint16_t* x;
  const uint16_t* w;
  const float* bias;
  uint16_t* out;
  int H, W, Cin, Cout, Ho, Wo, M, K, relu_in, tiles_m, tiles_n;
};

PP_DEVINL u32x4_t relu16x8(u32x4_t v) {
  // both 16-bit formats: a set sign bit clears the value (-0 -> +0; a NaN with the sign bit set -> +0 as well)
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] &= ~(((v[i] >> 15) & 0x00010001u) * 0xffffu);
  return v;
}

template <int EDT>
__global__ void __launch_bounds__(C4_T) conv4x4s2_kernel(const Conv4Args a) {
  typedef E16<EDT> E;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u32x4_t* lds = reinterpret_cast<u32x4_t*>(smem);   // [2][pixels 128x8 chunks | weights 128x8 chunks], chunk ^ (row & 7)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // every XCD walks a contiguous range of tile ids, in groups of C4_GROUP_M pixel panels
  int tm, tn;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid % PP_XCDS, idx = bid / PP_XCDS, q = nwg / PP_XCDS, r = nwg % PP_XCDS;
    const int first = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    pp_tile_decode(first + idx, a.tiles_m, a.tiles_n, C4_GROUP_M, &tm, &tn);
  }
  const int m0 = tm * C4_BM, n0 = tn * C4_BN;
  const int ck = tid & 7, r0 = tid >> 3;             // this thread stages chunk ck of rows r0 + 32 i

  int iy0[4], ix0[4];
  size_t xb[4];
  bool mv[4], wv[4];
  const uint16_t* wrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + r0 + 32 * i;
    mv[i] = m < a.M;
    const int mm = mv[i] ? m : 0;
    const int b = mm / (a.Ho * a.Wo), rem = mm - b * (a.Ho * a.Wo);
    const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
    iy0[i] = 2 * oy - 1;
    ix0[i] = 2 * ox - 1;
    xb[i] = (size_t)b * a.H * a.W * a.Cin + ck * 8;
    const int n = n0 + r0 + 32 * i;
    wv[i] = n < a.Cout;
    wrow[i] = a.w + (size_t)(wv[i] ? n : 0) * a.K + ck * 8;
  }

  u32x4_t xr[4], wr[4];
  auto load = [&](int kt) {
    const int k0 = kt * C4_BK;
    const int tap = k0 / a.Cin, c0 = k0 - tap * a.Cin;
    const int ky = tap >> 2, kx = tap & 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int iy = iy0[i] + ky, ix = ix0[i] + kx;
      const bool ok = mv[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (ok) v = *reinterpret_cast<const u32x4_t*>(a.x + xb[i] + ((size_t)iy * a.W + ix) * a.Cin + c0);
      xr[i] = a.relu_in ? relu16x8(v) : v;
      u32x4_t u = {0u, 0u, 0u, 0u};
      if (wv[i]) u = *reinterpret_cast<const u32x4_t*>(wrow[i] + k0);
      wr[i] = u;
    }
  };
  auto stage = [&](int buf) {
    u32x4_t* base = lds + buf * 2 * C4_TILE_CHUNKS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = r0 + 32 * i;
      base[row * 8 + (ck ^ (row & 7))] = xr[i];
      base[C4_TILE_CHUNKS + row * 8 + (ck ^ (row & 7))] = wr[i];
    }
  };

  f32x16_t acc[2][2];      // [out-channel block j][pixel block i]
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;

  const int wn = wave & 1, wm = wave >> 1;           // the wave's 64 (channels) x 64 (pixels) quarter of the tile
  const int l31 = lane & 31, lh = lane >> 5;
  const int nk = a.K / C4_BK;
  load(0);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
    const u32x4_t* base = lds + buf * 2 * C4_TILE_CHUNKS;
#pragma unroll
    for (int kk = 0; kk < C4_BK / 16; ++kk) {
      const int chunk = kk * 2 + lh;
      typename E::v8 wf[2], xf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int rn = wn * 64 + j * 32 + l31;
        wf[j] = __builtin_bit_cast(typename E::v8, base[C4_TILE_CHUNKS + rn * 8 + (chunk ^ (rn & 7))]);
        const int rm = wm * 64 + j * 32 + l31;
        xf[j] = __builtin_bit_cast(typename E::v8, base[rm * 8 + (chunk ^ (rm & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = E::mfma32(wf[j], xf[i], acc[j][i]);
    }
    // (buffer buf ^ 1 was last read in step kt - 1, which every wave left at the barrier below)
    if (kt + 1 < nk) stage(buf ^ 1);
    __syncthreads();
  }

  // accumulator of block (j, i): column = lane & 31 = the pixel, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) = the out channel
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 64 + i * 32 + l31;
    if (m >= a.M) continue;
    uint16_t* orow = a.out + (size_t)m * a.Cout;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + j * 32 + 8 * g + 4 * lh;
        if (n >= a.Cout) continue;                   // (Cout % 4 == 0: a quad is whole or absent)
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
        if (a.bias) { b0 = a.bias[n]; b1 = a.bias[n + 1]; b2 = a.bias[n + 2]; b3 = a.bias[n + 3]; }
        u32x2_t o;
        o[0] = E::pack2(acc[j][i][4 * g] + b0, acc[j][i][4 * g + 1] + b1);
        o[1] = E::pack2(acc[j][i][4 * g + 2] + b2, acc[j][i][4 * g + 3] + b3);
        *reinterpret_cast<u32x2_t*>(orow + n) = o;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) relu16_kernel(const u32x4_t* __restrict__ x, u32x4_t* __restrict__ y, long long n8) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) y[i] = relu16x8(x[i]);
}

// (1 - mask) * image: one thread per pixel, fp32 planes in (coalesced along pixels), one 16-byte pixel out
template <int EDT>
__global__ void __launch_bounds__(256) masked_image_pack_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                                int c, long long hw, u32x4_t* __restrict__ out) {
  typedef E16<EDT> E;
  const int b = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const float om = 1.0f - mask[(size_t)b * hw + p];
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = k < c ? om * img[((size_t)b * c + k) * hw + p] : 0.f;
  u32x4_t o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = E::pack2(v[2 * k], v[2 * k + 1]);
  out[(size_t)b * hw + p] = o;
}

// ------------------------------------------------------------------------------------------------------------------
// mask blend.  A workgroup owns one batch item x 256 pixels x a slab of 64 channels; a thread 8 channels (16 bytes) of 8
// pixels.  The statistics sum the values AS STORED: per thread in fp32 (8 values per channel, fixed order), then in fixed
// point with 64-bit integer atomics (LDS, then one global add per group and workgroup) => the sums do not depend on the
// order the workgroups run in; no floating-point atomics.
// ------------------------------------------------------------------------------------------------------------------
constexpr int MB_T = 256;
constexpr int MB_SLAB = 64;
constexpr int MB_PIX = 256;

struct BlendArgs {
  const uint16_t* s;
  const uint16_t* c;       // null: nothing is blended or stored, the launch only sums s
  const float* mask;
  uint16_t* out;
  unsigned long long* acc;
  int h, w, C, Hm, Wm, groups;
};

template <int EDT>
__global__ void __launch_bounds__(MB_T) mask_blend_kernel(const BlendArgs a) {
  typedef E16<EDT> E;
  __shared__ unsigned long long slots[MB_SLAB * 2];
  const int tid = threadIdx.x, l8 = tid & 7, pl = tid >> 3;
  const int b = blockIdx.z, c0 = blockIdx.y * MB_SLAB + l8 * 8;
  const int hw = a.h * a.w;
  const size_t img = (size_t)b * hw;
  if (a.acc && tid < MB_SLAB * 2) slots[tid] = 0ull;
  float sm[8], sq[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) sm[k] = sq[k] = 0.f;
#pragma unroll
  for (int it = 0; it < MB_PIX / 32; ++it) {
    const int p = blockIdx.x * MB_PIX + it * 32 + pl;
    if (p >= hw) break;
    const size_t off = (img + p) * a.C + c0;
    u32x4_t sv = *reinterpret_cast<const u32x4_t*>(a.s + off);
    if (a.c) {
      const int y = p / a.w, x = p - y * a.w;
      // F.interpolate(mode="nearest"): source index floor(i * H / h) (the host admits whole ratios only)
      const float m = a.mask[(size_t)b * a.Hm * a.Wm + (size_t)((y * a.Hm) / a.h) * a.Wm + (x * a.Wm) / a.w];
      const float om = 1.0f - m;
      const u32x4_t cv = *reinterpret_cast<const u32x4_t*>(a.c + off);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float lo = __builtin_fmaf(E::lo(sv[k]), m, E::lo(cv[k]) * om);
        const float hi = __builtin_fmaf(E::hi(sv[k]), m, E::hi(cv[k]) * om);
        sv[k] = E::pack2(lo, hi);
      }
      *reinterpret_cast<u32x4_t*>(a.out + off) = sv;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v0 = E::lo(sv[k]), v1 = E::hi(sv[k]);
      sm[2 * k] += v0; sq[2 * k] += v0 * v0;
      sm[2 * k + 1] += v1; sq[2 * k + 1] += v1 * v1;
    }
  }
  if (!a.acc) return;
  __syncthreads();                                   // (slots are zero)
  const int cg = a.C / a.groups;
  const int g_first = (blockIdx.y * MB_SLAB) / cg;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int gl = (c0 + k) / cg - g_first;
    const unsigned long long fs = (unsigned long long)(long long)__float2ll_rn(sm[k] * PP_GN_SUM_SCALE);
    const unsigned long long fq = (unsigned long long)(long long)__float2ll_rn(sq[k] * PP_GN_SQ_SCALE);
    __hip_atomic_fetch_add(slots + gl * 2, fs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(slots + gl * 2 + 1, fq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  const int g_last = (blockIdx.y * MB_SLAB + MB_SLAB - 1) / cg;
  if (tid <= g_last - g_first) {
    unsigned long long* dst = a.acc + ((size_t)b * a.groups + g_first + tid) * 2;
    __hip_atomic_fetch_add(dst, slots[tid * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(dst + 1, slots[tid * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

extern "C" int pp_conv4x4s2(const void* x, int batch, int hin, int win, int cin, const void* w, const float* bias, int cout,
                            int relu_in, void* out, int dtype, void* stream) {
  if (!x || !w || !out || !pp_dt_ok(dtype) || batch <= 0 || hin < 2 || win < 2 || cin <= 0 || cout <= 0) return PP_ERR_BAD_ARG;
  if (cin % C4_BK || cout % 4) return PP_ERR_BAD_ARG;
  if (((uintptr_t)x | (uintptr_t)w) & 15 || ((uintptr_t)out & 7) || ((uintptr_t)bias & 3)) return PP_ERR_BAD_ARG;
  const int ho = (hin - 2) / 2 + 1, wo = (win - 2) / 2 + 1;
  const long long M = (long long)batch * ho * wo;
  if (M > 0x7fffffffLL - C4_BM || (long long)hin * win > 0x7fffffffLL) return PP_ERR_UNSUPPORTED;
  Conv4Args a;
  a.x = (const uint16_t*)x;
  a.w = (const uint16_t*)w;
  a.bias = bias;
  a.out = (uint16_t*)out;
  a.H = hin; a.W = win; a.Cin = cin; a.Cout = cout; a.Ho = ho; a.Wo = wo; a.M = (int)M; a.K = 16 * cin;
  a.relu_in = relu_in ? 1 : 0;
  a.tiles_m = (int)((M + C4_BM - 1) / C4_BM);
  a.tiles_n = (cout + C4_BN - 1) / C4_BN;
  const long long grid = (long long)a.tiles_m * a.tiles_n;
  if (grid > 0x7fffffffLL) return PP_ERR_UNSUPPORTED;
  const int lds = 2 * 2 * C4_TILE_CHUNKS * 16;
  if (dtype == PP_DT_F16) {
    if (pp_func_lds((const void*)conv4x4s2_kernel<PP_DT_F16>, lds, "conv4x4s2_kernel") != PP_OK) return PP_ERR_LAUNCH;
  } else {
    if (pp_func_lds((const void*)conv4x4s2_kernel<PP_DT_BF16>, lds, "conv4x4s2_kernel") != PP_OK) return PP_ERR_LAUNCH;
  }
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL(conv4x4s2_kernel<EDT>, dim3((unsigned)grid), dim3(C4_T), lds, (hipStream_t)stream, a));
  PP_CHECK_LAUNCH("conv4x4s2_kernel");
  return PP_OK;
}

extern "C" int pp_relu(const void* x, void* out, long long n, int dtype, void* stream) {
  if (!x || !out || !pp_dt_ok(dtype) || n <= 0 || n % 8 || (((uintptr_t)x | (uintptr_t)out) & 15)) return PP_ERR_BAD_ARG;
  const long long n8 = n / 8;
  long long nb = (n8 + 255) / 256;
  const long long cap = (long long)pp_cu_count() * 16;
  if (nb > cap) nb = cap;
  hipLaunchKernelGGL(relu16_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)x, (u32x4_t*)out, n8);
  PP_CHECK_LAUNCH("relu16_kernel");
  return PP_OK;
}

extern "C" int pp_masked_image_pack(const float* image, const float* mask, int batch, int c, int h, int w, void* out, int dtype,
                                    void* stream) {
  if (!image || !mask || !out || !pp_dt_ok(dtype) || batch <= 0 || batch > 65535 || c <= 0 || c > 8 || h <= 0 || w <= 0)
    return PP_ERR_BAD_ARG;
  if ((((uintptr_t)image | (uintptr_t)mask) & 3) || ((uintptr_t)out & 15)) return PP_ERR_BAD_ARG;
  const long long hw = (long long)h * w;
  const long long nb = (hw + 255) / 256;
  if (nb > 0x7fffffffLL) return PP_ERR_UNSUPPORTED;
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL(masked_image_pack_kernel<EDT>, dim3((unsigned)nb, batch), dim3(256), 0,
                                         (hipStream_t)stream, image, mask, c, hw, (u32x4_t*)out));
  PP_CHECK_LAUNCH("masked_image_pack_kernel");
  return PP_OK;
}

extern "C" int pp_mask_blend(const void* sample, const void* cond, const float* mask, void* out, int batch, int h, int w, int c,
                             int mask_h, int mask_w, int64_t* acc, int groups, int dtype, void* stream) {
  if (!sample || !pp_dt_ok(dtype) || batch <= 0 || batch > 65535 || h <= 0 || w <= 0 || c <= 0 || c % MB_SLAB)
    return PP_ERR_BAD_ARG;
  if (((uintptr_t)sample | (uintptr_t)cond | (uintptr_t)out) & 15) return PP_ERR_BAD_ARG;
  if (cond) {
    if (!mask || !out || ((uintptr_t)mask & 3) || mask_h <= 0 || mask_w <= 0 || mask_h % h || mask_w % w) return PP_ERR_BAD_ARG;
    if ((long long)mask_h * mask_w > 0x7fffffffLL) return PP_ERR_UNSUPPORTED;
  } else if (!acc) {
    return PP_ERR_BAD_ARG;                             // nothing to do
  }
  if (acc && (((uintptr_t)acc & 7) || groups <= 0 || c % groups)) return PP_ERR_BAD_ARG;
  if ((long long)h * w > 0x7fffffffLL - MB_PIX || c / MB_SLAB > 65535) return PP_ERR_UNSUPPORTED;
  BlendArgs a;
  a.s = (const uint16_t*)sample;
  a.c = (const uint16_t*)cond;
  a.mask = mask;
  a.out = (uint16_t*)out;
  a.acc = (unsigned long long*)acc;
  a.h = h; a.w = w; a.C = c; a.Hm = mask_h; a.Wm = mask_w; a.groups = acc ? groups : 1;
  const int nb = (h * w + MB_PIX - 1) / MB_PIX;
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL(mask_blend_kernel<EDT>, dim3(nb, c / MB_SLAB, batch), dim3(MB_T), 0, (hipStream_t)stream, a));
  PP_CHECK_LAUNCH("mask_blend_kernel");
  return PP_OK;
}
