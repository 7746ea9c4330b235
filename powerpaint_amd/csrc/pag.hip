// Perturbed-attention guidance (PAG, diffusers' PAGMixin): the two launches the feature adds to a step.
//   pp_attn_identity_v  the "attention" of the perturbed batch items of a selected attn1: its output is V itself, copied out
//                       of the V^T layout every self-attention producer leaves (the inverse of pp_transpose_v)
//   pp_pag_combine      e = e_u + g (e_c - e_u) + s (e_c - e_p)  (or e_c + s (e_c - e_p)) into segment 0 of the fp32 eps
//                       buffer, s read from a per-row device table, in front of the scheduler's step launch run with cfg = 0
#include "pp_common.h"

namespace {

// One 64 (c) x 64 (p) tile of 16-bit values through LDS.  In: vt[b][c][p], 8 lanes x 16 B per row c.  Out: out[b][p][c], 8 lanes
// x 16 B per row p.  LDS image: row c holds its eight 16-byte chunks (8 positions each) at chunk index q ^ (c >> 3):
//   * the ds_write_b128 of 8 consecutive lanes (one lane group) covers one whole 128-byte row = all 32 banks once, whatever
//     the permutation;
//   * the 16-bit reads of a 32-lane group go to rows 8 cg + j (cg = lane & 7) at positions p = 8 q + (lane >> 3): dword
//     4 (q ^ cg) + (p & 7) / 2 of a row (rows are 32 dwords, so the row does not move the bank): 8 x 2 distinct banks, the
//     two lanes of a bank reading the same dword.  Without the XOR all eight cg would meet in one bank.
__global__ void __launch_bounds__(256) attn_identity_v_kernel(const uint16_t* __restrict__ vt, int ldvt, int batch0, int n, int C,
                                                             uint16_t* __restrict__ out, int ldo, int vec) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[64 * 64];
  const int b = batch0 + blockIdx.z;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const uint16_t* src = vt + (size_t)b * C * ldvt;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = threadIdx.x + 256 * k;
    const int c = i >> 3, q = i & 7;
    u32x4_t v = {0u, 0u, 0u, 0u};
    // (a chunk that starts below n ends at round8(n) <= ldvt at the latest: inside the row, pad columns are read, never copied out)
    if (c0 + c < C && p0 + 8 * q < n) {
      const uint16_t* s = src + (size_t)(c0 + c) * ldvt + p0 + 8 * q;
      if (vec) {
        v = *reinterpret_cast<const u32x4_t*>(s);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (uint32_t)s[2 * j] | ((uint32_t)s[2 * j + 1] << 16);
      }
    }
    *reinterpret_cast<u32x4_t*>(&tile[c * 64 + 8 * (q ^ (c >> 3))]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = threadIdx.x + 256 * k;
    const int cg = i & 7, pl = i >> 3;
    const uint16_t* t = &tile[8 * cg * 64 + 8 * ((pl >> 3) ^ cg) + (pl & 7)];
    u32x4_t v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (uint32_t)t[(2 * j) * 64] | ((uint32_t)t[(2 * j + 1) * 64] << 16);
    if (p0 + pl < n && c0 + 8 * cg < C) {      // (C % 8 == 0: a chunk of 8 channels is inside the row or outside it)
      uint16_t* d = out + ((size_t)b * n + p0 + pl) * ldo + c0 + 8 * cg;
      if (vec) {
        *reinterpret_cast<u32x4_t*>(d) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          d[2 * j] = (uint16_t)(v[j] & 0xffffu);
          d[2 * j + 1] = (uint16_t)(v[j] >> 16);
        }
      }
    }
  }
}

PP_DEVINL float pag_one(float a, float c, float p, int cfg, float g, float s) {
  // cfg: a = e_u, c = e_c, p = e_p.  else: a = e_c, p = e_p (c unused)
  return cfg ? a + g * (c - a) + s * (c - p) : a + s * (a - p);
}

__global__ void __launch_bounds__(256) pag_combine_kernel(float* __restrict__ eps, int cfg, float g,
                                                         const float* __restrict__ table, const int32_t* __restrict__ step_dev,
                                                         int n, int vec) {
  const float s = table[step_dev[0]];
  const long long stride = (long long)gridDim.x * 256;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (vec) {                                   // n % 4 == 0 and eps 16-byte aligned: every segment starts on a 16-byte boundary
    const int n4 = n >> 2;
    f32x4_t* e0 = reinterpret_cast<f32x4_t*>(eps);
    const f32x4_t* e1 = reinterpret_cast<const f32x4_t*>(eps + n);
    const f32x4_t* e2 = reinterpret_cast<const f32x4_t*>(eps + 2 * (size_t)n);
    for (long long i = i0; i < n4; i += stride) {
      const f32x4_t a = e0[i], c = e1[i];
      const f32x4_t p = cfg ? e2[i] : c;
      f32x4_t r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = pag_one(a[j], c[j], p[j], cfg, g, s);
      e0[i] = r;
    }
    return;
  }
  for (long long i = i0; i < n; i += stride) {
    const float a = eps[i], c = eps[(size_t)n + i];
    const float p = cfg ? eps[2 * (size_t)n + i] : c;
    eps[i] = pag_one(a, c, p, cfg, g, s);
  }
}

}  // namespace

extern "C" int pp_attn_identity_v(const void* vt, int ldvt, int batch0, int batch, int n, int C, void* out, int ldo,
                                  void* stream) {
  if (!vt || !out || batch0 < 0 || batch <= 0 || batch > 65535 || n <= 0 || C <= 0) return PP_ERR_BAD_ARG;
  if (C % 8 || ldvt < n || ldvt % 8 || ldo < C || ldo % 8) return PP_ERR_BAD_ARG;
  if ((((uintptr_t)vt) | ((uintptr_t)out)) & 1) return PP_ERR_BAD_ARG;
  const int vec = ((((uintptr_t)vt) | ((uintptr_t)out)) & 15) == 0;
  const long long gx = ((long long)n + 63) / 64, gy = (C + 63) / 64;
  if (gy > 65535) return PP_ERR_BAD_ARG;
  hipLaunchKernelGGL(attn_identity_v_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)vt, ldvt, batch0, n, C, (uint16_t*)out, ldo, vec);
  PP_CHECK_LAUNCH("attn_identity_v_kernel");
  return PP_OK;
}

extern "C" int pp_pag_combine(float* eps, int cfg, float guidance, const float* pag_table, const int32_t* step_dev, int n,
                              void* stream) {
  if (!eps || !pag_table || !step_dev || n <= 0 || (cfg != 0 && cfg != 1)) return PP_ERR_BAD_ARG;
  if (((uintptr_t)eps) & 3) return PP_ERR_BAD_ARG;
  const int vec = (n % 4 == 0) && ((((uintptr_t)eps) & 15) == 0);
  long long nb = ((vec ? n / 4 : n) + 255LL) / 256;
  nb = nb > 4096 ? 4096 : nb;
  hipLaunchKernelGGL(pag_combine_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, eps, cfg, guidance, pag_table,
                     step_dev, n, vec);
  PP_CHECK_LAUNCH("pag_combine_kernel");
  return PP_OK;
}
