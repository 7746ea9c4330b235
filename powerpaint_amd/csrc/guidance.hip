// guidance_rescale (diffusers' rescale_noise_cfg; Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed",
// section 3.4): the one guidance step of the loop that is not elementwise.
//   pp_cfg_rescale   m = e_u + g (e_c - e_u) [+ s (e_c - e_p)] pulled back, per sample, to the spread of e_c:
//                    segment 0 <- m (phi r_b + 1 - phi),  r_b = sqrt(SSD(e_c[b]) / SSD(m[b])),  SSD = the sum of squared
//                    deviations from the sample's own mean.  In front of the scheduler's step launch run with cfg = 0, in the
//                    place of pp_pag_combine.
#include "pp_common.h"

namespace {

constexpr int RS_THREADS = 1024;                  // one workgroup per sample
constexpr int RS_WAVES = RS_THREADS / 64;

// The combine, as the step kernels (small.hip: eu + g * (ec - eu)) and pag_one (pag.hip) spell it.  Every pass below calls this
// one function on the same operands: its result feeds a subtraction, a product or a sum of its own, never a place a
// multiply-add contraction could reach into, so the three passes see the same bits.
template <int PAG>
PP_DEVINL float guided_one(float a, float c, float p, float g, float s) {
  return PAG ? a + g * (c - a) + s * (c - p) : a + g * (c - a);
}

// Two sums over the workgroup, the same value in every thread: lanes by __shfl_xor (a butterfly: every lane ends with the
// same bits), the wave totals through LDS, added in wave order.  No atomics: the order is a function of the thread index.
PP_DEVINL void block_sum2(float& x, float& y, float (*red)[RS_WAVES]) {
  x = wave_sum(x);
  y = wave_sum(y);
  __syncthreads();                                // (the previous reduction's readers are done with `red`)
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = x;
    red[1][threadIdx.x >> 6] = y;
  }
  __syncthreads();
  x = 0.f;
  y = 0.f;
#pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) {
    x += red[0][w];
    y += red[1][w];
  }
}

// Three passes over the sample's segments, re-read from global memory / L2 (one segment of one sample at 1024^2 is 256 KB):
//   1  sum(e_c), sum(m)  -> the two means          2  sum((e_c - mean_c)^2), sum((m - mean_m)^2)  -> the factor      3  write
// Thread t takes elements (16-byte groups where vec) t, t + 1024, ...: a sample's summation order depends on `per` and `vec`
// alone, not on the batch or on the sample's place in it.  PAG (the third segment) is a template argument: a branch on it
// inside the loops would stand between the loads of one iteration and those of the next, and one CU walking 256 KB segments
// lives on the loads it has in flight.
template <int PAG>
__global__ void __launch_bounds__(RS_THREADS) cfg_rescale_kernel(float* __restrict__ eps, float g,
                                                                const float* __restrict__ table,
                                                                const int32_t* __restrict__ step_dev,
                                                                const float* __restrict__ phi_dev, int batch, int per, int vec) {
  __shared__ float red[2][RS_WAVES];
  const float s = PAG ? table[step_dev[0]] : 0.f;
  const float phi = phi_dev[0];
  const size_t seg = (size_t)batch * per;
  float* e0 = eps + (size_t)blockIdx.x * per;
  const float* e1 = e0 + seg;
  const float* e2 = PAG ? e1 + seg : e1;
  const int t = threadIdx.x;
  float sc = 0.f, sm = 0.f;
  if (vec) {                                     // per % 4 == 0 and eps 16-byte aligned: so is every sample of every segment
    const int n4 = per >> 2;
    f32x4_t* v0 = reinterpret_cast<f32x4_t*>(e0);
    const f32x4_t* v1 = reinterpret_cast<const f32x4_t*>(e1);
    const f32x4_t* v2 = reinterpret_cast<const f32x4_t*>(e2);
#pragma unroll 4
    for (int i = t; i < n4; i += RS_THREADS) {
      const f32x4_t a = v0[i], c = v1[i];
      const f32x4_t p = PAG ? v2[i] : c;
      float m[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = guided_one<PAG>(a[j], c[j], p[j], g, s);
      sc += (c[0] + c[1]) + (c[2] + c[3]);
      sm += (m[0] + m[1]) + (m[2] + m[3]);
    }
    block_sum2(sc, sm, red);
    const float mean_c = sc / (float)per, mean_m = sm / (float)per;
    float qc = 0.f, qm = 0.f;
#pragma unroll 4
    for (int i = t; i < n4; i += RS_THREADS) {
      const f32x4_t a = v0[i], c = v1[i];
      const f32x4_t p = PAG ? v2[i] : c;
      float dc[4], dm[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dc[j] = c[j] - mean_c;
        dm[j] = guided_one<PAG>(a[j], c[j], p[j], g, s) - mean_m;
      }
      qc += (dc[0] * dc[0] + dc[1] * dc[1]) + (dc[2] * dc[2] + dc[3] * dc[3]);
      qm += (dm[0] * dm[0] + dm[1] * dm[1]) + (dm[2] * dm[2] + dm[3] * dm[3]);
    }
    block_sum2(qc, qm, red);
    const float f = phi * sqrtf(qc / qm) + (1.0f - phi);
#pragma unroll 4
    for (int i = t; i < n4; i += RS_THREADS) {
      const f32x4_t a = v0[i], c = v1[i];
      const f32x4_t p = PAG ? v2[i] : c;
      f32x4_t r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = guided_one<PAG>(a[j], c[j], p[j], g, s) * f;
      v0[i] = r;
    }
    return;
  }
#pragma unroll 4
  for (int i = t; i < per; i += RS_THREADS) {
    const float c = e1[i];
    sc += c;
    sm += guided_one<PAG>(e0[i], c, PAG ? e2[i] : c, g, s);
  }
  block_sum2(sc, sm, red);
  const float mean_c = sc / (float)per, mean_m = sm / (float)per;
  float qc = 0.f, qm = 0.f;
#pragma unroll 4
  for (int i = t; i < per; i += RS_THREADS) {
    const float c = e1[i];
    const float dc = c - mean_c;
    const float dm = guided_one<PAG>(e0[i], c, PAG ? e2[i] : c, g, s) - mean_m;
    qc += dc * dc;
    qm += dm * dm;
  }
  block_sum2(qc, qm, red);
  const float f = phi * sqrtf(qc / qm) + (1.0f - phi);
#pragma unroll 4
  for (int i = t; i < per; i += RS_THREADS) e0[i] = guided_one<PAG>(e0[i], e1[i], PAG ? e2[i] : e1[i], g, s) * f;
}

}  // namespace

extern "C" int pp_cfg_rescale(float* eps, int segs, float guidance, const float* pag_table, const float* phi_dev,
                              const int32_t* step_dev, int batch, int per, void* stream) {
  if (!eps || !phi_dev || (segs != 2 && segs != 3) || batch <= 0 || per < 2) return PP_ERR_BAD_ARG;
  if ((segs == 3) != (pag_table != nullptr)) return PP_ERR_BAD_ARG;
  if (pag_table && !step_dev) return PP_ERR_BAD_ARG;
  if (((uintptr_t)eps) & 3) return PP_ERR_BAD_ARG;
  const int vec = (per % 4 == 0) && ((((uintptr_t)eps) & 15) == 0);
  if (segs == 3)
    hipLaunchKernelGGL(cfg_rescale_kernel<1>, dim3((unsigned)batch), dim3(RS_THREADS), 0, (hipStream_t)stream, eps, guidance,
                       pag_table, step_dev, phi_dev, batch, per, vec);
  else
    hipLaunchKernelGGL(cfg_rescale_kernel<0>, dim3((unsigned)batch), dim3(RS_THREADS), 0, (hipStream_t)stream, eps, guidance,
                       pag_table, step_dev, phi_dev, batch, per, vec);
  PP_CHECK_LAUNCH("cfg_rescale_kernel");
  return PP_OK;
}
