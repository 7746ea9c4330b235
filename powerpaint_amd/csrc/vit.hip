// CLIP vision tower (transformers.CLIPVisionModelWithProjection, the `image_encoder` of the IP-Adapter pipelines): the two
// kernels in front of the encoder layers.  Everything behind them is pp_layernorm / pp_gemm_bf16 / pp_attention_fwd.
//   vit_patchify_kernel : NCHW pixels -> im2col rows of the stride-P patch convolution (a copy with one rounding), so the
//                         patch embedding is a plain GEMM against the flattened conv weight
//   vit_embed_ln_kernel : [class | patches] + position embedding, then pre_layrnorm, one wave per token row
#include "pp_common.h"

namespace {

PP_DEVINL float vit_load_f32(const void* p, int dtype, size_t i) {
  if (dtype == PP_DT_F32) return ((const float*)p)[i];
  if (dtype == PP_DT_BF16) return bf2f(((const uint16_t*)p)[i]);
  return (float)(((const _Float16*)p)[i]);
}

// thread = 8 consecutive columns of one output row (one 16-byte store); columns [3 P P, cols) are zeros, [cols, ldo) untouched
template <int EDT>
__global__ void __launch_bounds__(256) vit_patchify_kernel(const void* __restrict__ src, int dtype, int H, int W, int P, int gh,
                                                          int gw, long long rows, uint16_t* __restrict__ dst, int cols,
                                                          int ldo) {
  const int S = cols >> 3, PP2 = P * P, K = 3 * PP2;
  const long long total = rows * S;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / S;
    const int k0 = (int)(i - r * S) * 8;
    const int gx = (int)(r % gw), gy = (int)((r / gw) % gh);
    const long long b = r / ((long long)gw * gh);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      v[j] = 0.f;
      if (k < K) {
        const int c = k / PP2, t = k - c * PP2, ky = t / P, kx = t - ky * P;
        v[j] = vit_load_f32(src, dtype, (((size_t)b * 3 + c) * H + (size_t)gy * P + ky) * W + (size_t)gx * P + kx);
      }
    }
    u32x4_t o;
    o[0] = E16<EDT>::pack2(v[0], v[1]); o[1] = E16<EDT>::pack2(v[2], v[3]); o[2] = E16<EDT>::pack2(v[4], v[5]); o[3] = E16<EDT>::pack2(v[6], v[7]);
    *reinterpret_cast<u32x4_t*>(dst + (size_t)r * ldo + k0) = o;
  }
}

// One wave per token row, <= 4 16-B pieces per lane (C <= 2048): the fp32 sum of the two stored 16-bit operands stays in
// registers, then the two-pass statistics and the apply of layernorm_kernel (norm.hip), term for term.
template <int NP, int EDT>
__global__ void __launch_bounds__(256) vit_embed_ln_kernel(const uint16_t* __restrict__ patches, int ldp,
                                                          const uint16_t* __restrict__ cls, const uint16_t* __restrict__ pos,
                                                          int rows, int np, int C, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, uint16_t* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = row / (np + 1), t = row - b * (np + 1);
  const uint16_t* xa = t == 0 ? cls : patches + ((size_t)b * np + (t - 1)) * ldp;
  const uint16_t* xb = pos + (size_t)t * C;
  const int S = C >> 3;
  float v[NP][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int pc = lane + i * 64;
    if (pc < S) {
      const u32x4_t u = *reinterpret_cast<const u32x4_t*>(xa + pc * 8);
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(xb + pc * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[i][2 * j] = E16<EDT>::lo(u[j]) + E16<EDT>::lo(w[j]);
        v[i][2 * j + 1] = E16<EDT>::hi(u[j]) + E16<EDT>::hi(w[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += v[i][j];
  }
  const float mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int pc = lane + i * 64;
    if (pc < S) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; sq += d * d; }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int pc = lane + i * 64;
    if (pc < S) {
      const int c = pc * 8;
      const f32x4_t g0 = *reinterpret_cast<const f32x4_t*>(gamma + c), g1 = *reinterpret_cast<const f32x4_t*>(gamma + c + 4);
      const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(beta + c), b1 = *reinterpret_cast<const f32x4_t*>(beta + c + 4);
      float r[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = (v[i][j] - mean) * rstd * g0[j] + b0[j];
        r[4 + j] = (v[i][4 + j] - mean) * rstd * g1[j] + b1[j];
      }
      u32x4_t o;
      o[0] = E16<EDT>::pack2(r[0], r[1]); o[1] = E16<EDT>::pack2(r[2], r[3]); o[2] = E16<EDT>::pack2(r[4], r[5]); o[3] = E16<EDT>::pack2(r[6], r[7]);
      *reinterpret_cast<u32x4_t*>(y + (size_t)row * C + c) = o;
    }
  }
}

int vit_grid(long long total) {
  const long long nb = (total + 255) / 256;
  return (int)(nb < 1 ? 1 : nb > 65536 ? 65536 : nb);
}

}  // namespace

extern "C" int pp_vit_patchify(const void* src, int src_dtype, int batch, int h, int w, int patch, void* dst, int cols,
                               int ldo, int dtype, void* stream) {
  if (!src || !dst || batch <= 0 || patch <= 0 || h < patch || w < patch || src_dtype < 0 || src_dtype > 2 || !pp_dt_ok(dtype))
    return PP_ERR_BAD_ARG;
  if (patch > 64 || cols % 8 != 0 || cols < 3 * patch * patch || ldo % 8 != 0 || ldo < cols || ((uintptr_t)dst & 15)) return PP_ERR_BAD_ARG;
  const int gh = h / patch, gw = w / patch;
  const long long rows = (long long)batch * gh * gw;
  if (rows * ldo >= 0x40000000ll || (long long)batch * 3 * h * w >= 0x40000000ll) return PP_ERR_UNSUPPORTED;
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL(vit_patchify_kernel<EDT>, dim3(vit_grid(rows * (cols / 8))), dim3(256), 0,
                                         (hipStream_t)stream, src, src_dtype, h, w, patch, gh, gw, rows, (uint16_t*)dst, cols,
                                         ldo));
  PP_CHECK_LAUNCH("vit_patchify_kernel");
  return PP_OK;
}

extern "C" int pp_vit_embed_ln(const void* patches, int ldp, const void* class_embedding, const void* pos, int batch, int np,
                               int C, const float* gamma, const float* beta, float eps, void* y, int dtype, void* stream) {
  if (!patches || !class_embedding || !pos || !gamma || !beta || !y || batch <= 0 || np <= 0 || C <= 0 || C % 8 || ldp < C ||
      ldp % 8 || !pp_dt_ok(dtype))
    return PP_ERR_BAD_ARG;
  if ((((uintptr_t)patches | (uintptr_t)class_embedding | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15))
    return PP_ERR_BAD_ARG;   // (16-byte loads and stores)
  const long long rows_ll = (long long)batch * (np + 1);
  if (rows_ll * (ldp > C ? ldp : C) >= 0x40000000ll) return PP_ERR_UNSUPPORTED;
  const int rows = (int)rows_ll, S = C / 8;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((rows + 3) / 4), block(256);
#define PP_VIT_LN(NP_)                                                                                                      \
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL((vit_embed_ln_kernel<NP_, EDT>), grid, block, 0, st, (const uint16_t*)patches, ldp, \
                                         (const uint16_t*)class_embedding, (const uint16_t*)pos, rows, np, C, gamma, beta,  \
                                         eps, (uint16_t*)y))
  if (S <= 64) PP_VIT_LN(1);
  else if (S <= 128) PP_VIT_LN(2);
  else if (S <= 192) PP_VIT_LN(3);
  else if (S <= 256) PP_VIT_LN(4);
  else return PP_ERR_UNSUPPORTED;
#undef PP_VIT_LN
  PP_CHECK_LAUNCH("vit_embed_ln_kernel");
  return PP_OK;
}
