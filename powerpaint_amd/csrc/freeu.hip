// FreeU (diffusers-0.27 `apply_freeu` / `fourier_filter`, called per resnet by the first two up blocks:
// powerpaint/models/unet_2d_blocks.py:2563-2587, 2706-2730 of the reference) in front of an up-block resnet, ONE launch:
//   hidden[:, :Ch/2] *= b            (the backbone half)
//   skip = fourier_filter(skip, threshold = 1, scale = s)
// and, optionally, the GroupNorm statistics of concat(hidden', skip') for the resnet's norm1 (the producers' epilogues summed
// the tensors as they were BEFORE FreeU; this launch replaces their subscription).
//
// With threshold = 1 the mask scales exactly the four frequency bins (u, v) in {-1, 0}^2, so per channel plane
//   y[h,w] = x[h,w] + (s - 1) / (H W) * Re sum_{(u,v)} X(u,v) e^{+2 pi i (u h / H + v w / W)}
// is seven real sums (S, and the cos / sin moments along h, along w and along h + w) and one multiply-add pass: no FFT.  The
// bin set is not Hermitian-symmetric; taking the real part is part of the definition.
//
// Layout: NHWC 16-bit.  A workgroup owns one batch item x a slab of 64 channels of ONE of the two tensors; lanes run along
// channels (a lane = a channel pair, 32 lanes = one 128-byte line of a pixel), the 8 half-waves along pixels.  Pass 1 sums, an
// LDS tree folds the 8 pixel lanes, pass 2 applies -- from an LDS copy of the slab where it fits (<= 320 pixels), from L2
// otherwise (a slab is at most 128 KiB at the 32x32 level).  Arithmetic fp32, one rounding to the storage format; the
// statistics sum the ROUNDED values (the convention of the GEMM epilogues, gemm_gn.h) in fixed point with 64-bit integer
// atomics => order-independent, bit-reproducible.
#include "pp_common.h"

namespace {

constexpr int FU_T = 256;          // threads
constexpr int FU_SLAB = 64;        // channels per workgroup
constexpr int FU_PL = FU_T / 32;   // pixel lanes
constexpr int FU_NS = 7;           // sums per plane
constexpr int FU_CACHE_PIX = 320;  // slab kept in LDS up to this many pixels (40 KiB)
constexpr int FU_MAX_HW_SUM = 512; // H + W the twiddle table holds

struct FreeuArgs {
  const uint16_t* hid_in;
  uint16_t* hid_out;
  const uint16_t* skip_in;
  uint16_t* skip_out;
  const float* bs;                 // device: (b, s)
  unsigned long long* acc;         // [B][groups][2] or null
  int ch, cs, H, W, groups, nslab_h, nslab_s, cache;
};

PP_DEVINL void fu_stats(unsigned long long* slots, int gl, float sm, float sq) {
  const unsigned long long fs = (unsigned long long)(long long)__float2ll_rn(sm * PP_GN_SUM_SCALE);
  const unsigned long long fq = (unsigned long long)(long long)__float2ll_rn(sq * PP_GN_SQ_SCALE);
  __hip_atomic_fetch_add(slots + gl * 2, fs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(slots + gl * 2 + 1, fq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int EDT>
__global__ void __launch_bounds__(FU_T) freeu_kernel(const FreeuArgs a) {
  typedef E16<EDT> E;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS: slots [64][2] u64 | red [FU_PL][FU_NS][64] f32 | fin [FU_NS][64] f32 | twiddles [2 (H + W)] f32 | slab copy
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(smem);
  float* red = reinterpret_cast<float*>(smem + FU_SLAB * 2 * 8);
  float* fin = red + FU_PL * FU_NS * FU_SLAB;
  float* tw = fin + FU_NS * FU_SLAB;                  // cosH[H] sinH[H] cosW[W] sinW[W]
  uint32_t* cache = reinterpret_cast<uint32_t*>(tw + 2 * FU_MAX_HW_SUM);

  const int tid = threadIdx.x;
  const int nslab = a.nslab_h + a.nslab_s;
  const int b = blockIdx.x / nslab;
  const int sl = blockIdx.x - b * nslab;
  const bool is_skip = sl >= a.nslab_h;
  const int C = is_skip ? a.cs : a.ch;
  const int c0 = (is_skip ? sl - a.nslab_h : sl) * FU_SLAB;      // first channel of the slab inside its tensor
  const int nch = min(FU_SLAB, C - c0);
  const int HW = a.H * a.W;
  const int cp = tid & 31, pl = tid >> 5;
  const bool live = 2 * cp < nch;                               // (C is even: a pair is whole or absent)
  const uint16_t* xin = (is_skip ? a.skip_in : a.hid_in) + (size_t)b * HW * C + c0 + 2 * cp;
  uint16_t* xout = (is_skip ? a.skip_out : a.hid_out) + (size_t)b * HW * C + c0 + 2 * cp;
  // statistics: position of the slab in concat(hidden, skip), channels per group
  const int cg = a.acc ? (a.ch + a.cs) / a.groups : 1;
  const int cbase = (is_skip ? a.ch : 0) + c0;
  const int g_first = cbase / cg;
  const int gl0 = (cbase + 2 * cp) / cg - g_first, gl1 = (cbase + 2 * cp + 1) / cg - g_first;

  if (a.acc && tid < FU_SLAB * 2) slots[tid] = 0ull;
  float sm0 = 0.f, sq0 = 0.f, sm1 = 0.f, sq1 = 0.f;             // (sum, sum of squares) of the stored values, per channel

  if (!is_skip) {
    // backbone: channels below Ch / 2 times b; the rest is copied (out of place) or only summed (in place)
    const float bsc = a.bs[0];
    const bool scaled = c0 + 2 * cp < a.ch / 2;                  // (Ch / 2 is even: a pair lies on one side)
    const bool store = scaled || xout != xin;
    if (live && (store || a.acc)) {
      for (int p = pl; p < HW; p += FU_PL) {
        uint32_t u = *reinterpret_cast<const uint32_t*>(xin + (size_t)p * C);
        if (scaled) u = E::pack2(E::lo(u) * bsc, E::hi(u) * bsc);
        if (store) *reinterpret_cast<uint32_t*>(xout + (size_t)p * C) = u;
        const float v0 = E::lo(u), v1 = E::hi(u);
        sm0 += v0; sq0 += v0 * v0;
        sm1 += v1; sq1 += v1 * v1;
      }
    }
  } else {
    // twiddles: cos / sin (2 pi h / H), (2 pi w / W)
    for (int i = tid; i < a.H + a.W; i += FU_T) {
      const bool along_h = i < a.H;
      const int k = along_h ? i : i - a.H, n = along_h ? a.H : a.W;
      float sn, cs;
      sincospif(2.0f * (float)k / (float)n, &sn, &cs);
      float* t = along_h ? tw : tw + 2 * a.H;
      t[k] = cs;
      t[n + k] = sn;
    }
    __syncthreads();
    const float* cH = tw, *sH = tw + a.H, *cW = tw + 2 * a.H, *sW = tw + 2 * a.H + a.W;
    float acc0[FU_NS], acc1[FU_NS];
#pragma unroll
    for (int k = 0; k < FU_NS; ++k) acc0[k] = acc1[k] = 0.f;
    if (live) {
      for (int p = pl; p < HW; p += FU_PL) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(xin + (size_t)p * C);
        if (a.cache) cache[p * 32 + cp] = u;
        const int h = p / a.W, w = p - h * a.W;
        const float ch = cH[h], sh = sH[h], cw = cW[w], sw = sW[w];
        const float cd = ch * cw - sh * sw, sd = sh * cw + ch * sw;      // cos / sin of the diagonal phase
        const float f[FU_NS] = {1.f, ch, sh, cw, sw, cd, sd};
        const float v0 = E::lo(u), v1 = E::hi(u);
#pragma unroll
        for (int k = 0; k < FU_NS; ++k) {
          acc0[k] = __builtin_fmaf(v0, f[k], acc0[k]);
          acc1[k] = __builtin_fmaf(v1, f[k], acc1[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < FU_NS; ++k) {
      red[(pl * FU_NS + k) * FU_SLAB + 2 * cp] = acc0[k];
      red[(pl * FU_NS + k) * FU_SLAB + 2 * cp + 1] = acc1[k];
    }
    __syncthreads();
    const float kf = (a.bs[1] - 1.0f) / (float)HW;
    for (int i = tid; i < FU_NS * FU_SLAB; i += FU_T) {          // i = k * 64 + channel
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < FU_PL; ++q) t += red[q * FU_NS * FU_SLAB + i];
      fin[i] = t * kf;
    }
    __syncthreads();
    if (live) {
      float m0[FU_NS], m1[FU_NS];
#pragma unroll
      for (int k = 0; k < FU_NS; ++k) {
        m0[k] = fin[k * FU_SLAB + 2 * cp];
        m1[k] = fin[k * FU_SLAB + 2 * cp + 1];
      }
      for (int p = pl; p < HW; p += FU_PL) {
        const uint32_t u = a.cache ? cache[p * 32 + cp] : *reinterpret_cast<const uint32_t*>(xin + (size_t)p * C);
        const int h = p / a.W, w = p - h * a.W;
        const float ch = cH[h], sh = sH[h], cw = cW[w], sw = sW[w];
        const float cd = ch * cw - sh * sw, sd = sh * cw + ch * sw;
        const float f[FU_NS] = {1.f, ch, sh, cw, sw, cd, sd};
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int k = 0; k < FU_NS; ++k) {
          d0 = __builtin_fmaf(m0[k], f[k], d0);
          d1 = __builtin_fmaf(m1[k], f[k], d1);
        }
        const uint32_t o = E::pack2(E::lo(u) + d0, E::hi(u) + d1);
        *reinterpret_cast<uint32_t*>(xout + (size_t)p * C) = o;
        const float v0 = E::lo(o), v1 = E::hi(o);
        sm0 += v0; sq0 += v0 * v0;
        sm1 += v1; sq1 += v1 * v1;
      }
    }
  }
  if (!a.acc) return;
  __syncthreads();                                              // (slots are zero)
  if (live) {
    fu_stats(slots, gl0, sm0, sq0);
    fu_stats(slots, gl1, sm1, sq1);
  }
  __syncthreads();
  const int g_last = (cbase + nch - 1) / cg;
  if (tid <= g_last - g_first) {
    unsigned long long* dst = a.acc + ((size_t)b * a.groups + g_first + tid) * 2;
    __hip_atomic_fetch_add(dst, slots[tid * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(dst + 1, slots[tid * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

extern "C" int pp_freeu(const void* hidden, void* hidden_out, int ch, const void* skip, void* skip_out, int cs, int batch,
                        int h, int w, const float* bs, int64_t* acc, int groups, int dtype, void* stream) {
  if (!hidden || !hidden_out || !skip || !skip_out || !bs || !pp_dt_ok(dtype)) return PP_ERR_BAD_ARG;
  if (((uintptr_t)hidden | (uintptr_t)hidden_out | (uintptr_t)skip | (uintptr_t)skip_out | (uintptr_t)bs) & 3)
    return PP_ERR_BAD_ARG;
  if (batch <= 0 || h < 2 || w < 2 || ch <= 0 || cs <= 0 || ch % 4 || cs % 2) return PP_ERR_BAD_ARG;   // (Ch / 2 must be even)
  if (skip_out == hidden || skip_out == hidden_out || hidden_out == skip) return PP_ERR_BAD_ARG;
  if (acc && (((uintptr_t)acc & 7) || groups <= 0 || groups > FU_SLAB || (ch + cs) % groups)) return PP_ERR_BAD_ARG;
  if (h + w > FU_MAX_HW_SUM) return PP_ERR_UNSUPPORTED;
  FreeuArgs a;
  a.hid_in = (const uint16_t*)hidden;
  a.hid_out = (uint16_t*)hidden_out;
  a.skip_in = (const uint16_t*)skip;
  a.skip_out = (uint16_t*)skip_out;
  a.bs = bs;
  a.acc = (unsigned long long*)acc;
  a.ch = ch; a.cs = cs; a.H = h; a.W = w; a.groups = groups;
  a.nslab_h = (ch + FU_SLAB - 1) / FU_SLAB;
  a.nslab_s = (cs + FU_SLAB - 1) / FU_SLAB;
  a.cache = h * w <= FU_CACHE_PIX ? 1 : 0;
  const long long grid = (long long)batch * (a.nslab_h + a.nslab_s);
  if (grid > 0x7fffffffLL) return PP_ERR_UNSUPPORTED;
  const size_t lds = FU_SLAB * 2 * 8 + (size_t)(FU_PL * FU_NS * FU_SLAB + FU_NS * FU_SLAB + 2 * FU_MAX_HW_SUM) * sizeof(float) +
                     (a.cache ? (size_t)h * w * 32 * 4 : 0);
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL(freeu_kernel<EDT>, dim3((unsigned)grid), dim3(FU_T), lds, (hipStream_t)stream, a));
  PP_CHECK_LAUNCH("freeu_kernel");
  return PP_OK;
}
