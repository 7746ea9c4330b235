// pp_ip_attn_add: the image-prompt term of IP-Adapter's decoupled cross-attention, added IN PLACE to the output of the text
// cross-attention (include/pp_hip.h, "IP-Adapter"):
//     o[b,r,h*d:(h+1)*d] += ip_scale * sum_j softmax_j(qk_scale * q[b,r,h] . k_ip[b,j,h]) * v_ip[b,j,h]
// A bandwidth kernel: it reads q, reads o and writes o (3 * M * C * 2 bytes); the nk <= 64 image tokens of a batch item are a
// few KB that every row of the item reuses.
//
// Work layout.  A lane owns 8 consecutive channels (one 16-byte load of q, one of o, one 16-byte store of o) of one row, so a
// head of d = 40 / 80 / 160 channels spans L = 5 / 10 / 20 lanes.  A wave takes a SLAB of G heads (the largest divisor of
// `heads` with G * L <= 64: 40 lanes at 8 heads) of R = 64 / (G * L) rows at a time and walks down the rows of ONE batch item
// with that slab, IP_ROWS row groups per pass with all their loads issued up front (a wave that waited for memory once per
// row group took 11 us whatever the size).  The channels a lane owns never change, so for nk <= 4 (one image per adapter,
// the common case) its slices of K and V sit in registers for the whole launch (IP_NKR); above that they are streamed per
// row through the vector cache (all rows of the workgroup read the same few KB).  The L partial dot products of a head are summed inside the wave by
// window sums over lane shifts (1, 2, 4, ... then the remainder: L = 4 + 1, 8 + 2, 16 + 4) and handed back from the head's
// first lane: 4 to 6 lane exchanges per score, a fixed fp32 summation order.
// Scores, softmax (maximum subtracted), the weighted sum and the add are fp32; ONE rounding to the 16-bit format at the store.
// Every element of o is read once and written once by the same lane; lanes outside [rows) x [columns) neither load nor store.
//
// pp_ip_attn_add_masked (diffusers' ip_adapter_masks) is the same body with MASK = true: the term of row r is multiplied by
// row_w[r], one fp32 weight per query row shared by the batch items, READ from device memory (a captured graph follows new
// values).  The weights of a pass are fetched ahead of its q / o loads -- one dependent load per pass, IP_ROWS values in
// flight together -- because a row whose weight is exactly 0 keeps its bits: its lanes load neither q nor o and do not
// store.  A row group without a live lane is skipped by a wave-uniform branch; in a group that runs, every lane executes
// every lane exchange of head_sum (a dead lane computes on zeros and stores nothing).  The weight multiplies ip_scale in
// fp32 in front of the division by the softmax denominator: with a weight of 1.0 that product is ip_scale itself and the
// result is pp_ip_attn_add's bit for bit.  The MASK = false instantiations are the code they were.
#include "pp_common.h"

namespace {

constexpr int IP_T = 256;      // threads per workgroup (4 waves)
constexpr int IP_NKR = 4;      // up to this many image tokens: K / V slices in registers
constexpr int IP_ROWS = 4;     // row groups per wave pass, their loads in flight together (amortises the K / V register fill)

struct IpArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* o;
  long long ldq, ldo;
  int nq, nk, C, L, span, R;     // span = G * L lanes per row of the slab; R rows per wave pass
  float qk_scale, ip_scale;
  const float* row_w;            // MASK only: fp32 [nq], one weight per query row (behind the unmasked form's fields)
};

template <int DT>
PP_DEVINL void unpack8(const u32x4_t u, float* f) {
  typedef E16<DT> E;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = E::lo(u[i]);
    f[2 * i + 1] = E::hi(u[i]);
  }
}

template <int DT>
PP_DEVINL float dot8(const float* qf, const u32x4_t ku) {
  float kf[8];
  unpack8<DT>(ku, kf);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s = __builtin_fmaf(qf[i], kf[i], s);
  return s;
}

// sum over the L lanes [lane, lane + L) -- exact for the first lane of a head (its window stays inside the head) -- then
// every lane takes the value of its head's first lane.  All 64 lanes execute every exchange.
PP_DEVINL float head_sum(float x, int L, int leader) {
  const float w2 = x + __shfl_down(x, 1, 64);
  const float w4 = w2 + __shfl_down(w2, 2, 64);
  float t;
  if (L == 5) {
    t = w4 + __shfl_down(x, 4, 64);
  } else {
    const float w8 = w4 + __shfl_down(w4, 4, 64);
    if (L == 10) {
      t = w8 + __shfl_down(w2, 8, 64);
    } else {      // L == 20
      const float w16 = w8 + __shfl_down(w8, 8, 64);
      t = w16 + __shfl_down(w4, 16, 64);
    }
  }
  return __shfl(t, leader, 64);
}

template <int DT, bool REG, bool MASK>
__global__ __launch_bounds__(IP_T) void ip_attn_add_kernel(const IpArgs a) {
  typedef E16<DT> E;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rsub = lane / a.span, within = lane - rsub * a.span;
  const bool lane_on = rsub < a.R;
  const int leader = lane - within % a.L;
  const int b = blockIdx.z;
  const size_t col = (size_t)blockIdx.y * a.span * 8 + (size_t)within * 8;       // first of the lane's 8 channels
  const uint16_t* kb = a.k + (size_t)b * a.nk * a.C + col;
  const uint16_t* vb = a.v + (size_t)b * a.nk * a.C + col;
  const int nk = a.nk, L = a.L;
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  u32x4_t kr[IP_NKR], vr[IP_NKR];
  if (REG) {
#pragma unroll
    for (int j = 0; j < IP_NKR; ++j) {
      const bool on = lane_on && j < nk;
      kr[j] = on ? *reinterpret_cast<const u32x4_t*>(kb + (size_t)j * a.C) : zero4;
      vr[j] = on ? *reinterpret_cast<const u32x4_t*>(vb + (size_t)j * a.C) : zero4;
    }
  }

  // A wave pass covers IP_ROWS row groups: all their loads of q and o are issued before the first score is formed, so a wave
  // waits for memory once per pass, not once per row group (the launch is sized for ONE pass per wave).
  const int wg = blockIdx.x * (IP_T / 64) + wave, nwaves = gridDim.x * (IP_T / 64);
  for (int r0 = wg * a.R * IP_ROWS; r0 < a.nq; r0 += nwaves * a.R * IP_ROWS) {        // (wave-uniform trip count)
    u32x4_t qu[IP_ROWS], ou[IP_ROWS];
    float rw[IP_ROWS];
    if (MASK) {
#pragma unroll
      for (int t = 0; t < IP_ROWS; ++t) {
        const int r = r0 + t * a.R + rsub;
        rw[t] = (lane_on && r < a.nq) ? a.row_w[r] : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < IP_ROWS; ++t) {
      const int r = r0 + t * a.R + rsub;
      const bool ok = lane_on && r < a.nq && (!MASK || rw[t] != 0.f);
      const size_t row = (size_t)b * a.nq + (size_t)(ok ? r : 0);
      qu[t] = ok ? *reinterpret_cast<const u32x4_t*>(a.q + row * a.ldq + col) : zero4;
      ou[t] = ok ? *reinterpret_cast<const u32x4_t*>(a.o + row * a.ldo + col) : zero4;
    }
#pragma unroll
    for (int t = 0; t < IP_ROWS; ++t) {
      if (r0 + t * a.R >= a.nq) break;                               // (wave-uniform: no row of this group exists)
      const int r = r0 + t * a.R + rsub;
      const bool ok = lane_on && r < a.nq && (!MASK || rw[t] != 0.f);
      if (MASK && !__any(ok)) continue;                              // (wave-uniform: every row of this group has weight 0)
      float qf[8], acc[8];
      unpack8<DT>(qu[t], qf);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.f;
      float l = 0.f;
      if (REG) {
        float s[IP_NKR], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < IP_NKR; ++j) {
          const float sc = head_sum(dot8<DT>(qf, kr[j]), L, leader) * a.qk_scale;
          s[j] = j < nk ? sc : -INFINITY;
          m = fmaxf(m, s[j]);
        }
#pragma unroll
        for (int j = 0; j < IP_NKR; ++j) {
          const float p = __expf(s[j] - m);                          // (a token past nk: exp(-inf) = 0)
          float vf[8];
          unpack8<DT>(vr[j], vf);
          l += p;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(p, vf[i], acc[i]);
        }
      } else {
        float m = -INFINITY;
        for (int j = 0; j < nk; ++j) {                               // online softmax over the streamed tokens
          const u32x4_t ku = lane_on ? *reinterpret_cast<const u32x4_t*>(kb + (size_t)j * a.C) : zero4;
          const u32x4_t vu = lane_on ? *reinterpret_cast<const u32x4_t*>(vb + (size_t)j * a.C) : zero4;
          const float sc = head_sum(dot8<DT>(qf, ku), L, leader) * a.qk_scale;
          const float mn = fmaxf(m, sc);
          const float corr = __expf(m - mn), p = __expf(sc - mn);    // (first token: exp(-inf) = 0)
          float vf[8];
          unpack8<DT>(vu, vf);
          l = __builtin_fmaf(l, corr, p);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(p, vf[i], acc[i] * corr);
          m = mn;
        }
      }
      if (ok) {
        const float w = (MASK ? a.ip_scale * rw[t] : a.ip_scale) / l;   // (l >= 1: the maximum's own term)
        float of[8];
        unpack8<DT>(ou[t], of);
        u32x4_t out;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          out[i] = E::pack2(__builtin_fmaf(w, acc[2 * i], of[2 * i]), __builtin_fmaf(w, acc[2 * i + 1], of[2 * i + 1]));
        *reinterpret_cast<u32x4_t*>(a.o + ((size_t)b * a.nq + r) * a.ldo + col) = out;
      }
    }
  }
}

}  // namespace

namespace {

template <bool MASK>
int ip_attn_add_launch(const void* q, int ldq, const void* k_ip, const void* v_ip, void* o, int ldo, int batch, int heads, int nq,
                       int nk, int d, float qk_scale, float ip_scale, const float* row_w, int dtype, void* stream) {
  if (MASK && (!row_w || ((uintptr_t)row_w & 3))) return PP_ERR_BAD_ARG;
  if (!q || !k_ip || !v_ip || !o || !pp_dt_ok(dtype)) return PP_ERR_BAD_ARG;
  if (batch <= 0 || heads <= 0 || nq <= 0 || nk <= 0 || d <= 0 || d % 8) return PP_ERR_BAD_ARG;
  if (d != 40 && d != 80 && d != 160) return PP_ERR_UNSUPPORTED;
  if (nk > PP_IP_MAX_TOKENS || heads > 64 || batch > 65535) return PP_ERR_UNSUPPORTED;
  const int C = heads * d;
  if (ldq < C || ldo < C || ldq % 8 || ldo % 8) return PP_ERR_BAD_ARG;
  if (((uintptr_t)q | (uintptr_t)k_ip | (uintptr_t)v_ip | (uintptr_t)o) & 15) return PP_ERR_BAD_ARG;
  if (q == o) return PP_ERR_BAD_ARG;
  if (!(qk_scale == qk_scale) || !(ip_scale == ip_scale)) return PP_ERR_BAD_ARG;
  if (ip_scale == 0.f) return PP_OK;          // the term is exactly zero: o stays as it is, bit for bit (no launch)
  IpArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k_ip;
  a.v = (const uint16_t*)v_ip;
  a.o = (uint16_t*)o;
  a.ldq = ldq; a.ldo = ldo; a.nq = nq; a.nk = nk; a.C = C;
  a.L = d / 8;
  int G = 1;
  for (int g = 1; g <= heads; ++g)
    if (heads % g == 0 && g * a.L <= 64) G = g;
  a.span = G * a.L;
  a.R = 64 / a.span;
  a.qk_scale = qk_scale; a.ip_scale = ip_scale;
  a.row_w = row_w;
  const int rows_per_wg = (IP_T / 64) * a.R * IP_ROWS;
  const dim3 grid((unsigned)((nq + rows_per_wg - 1) / rows_per_wg), (unsigned)(heads / G), (unsigned)batch);
  if (nk <= IP_NKR) {
    PP_DT_SWITCH(dtype, hipLaunchKernelGGL((ip_attn_add_kernel<EDT, true, MASK>), grid, dim3(IP_T), 0, (hipStream_t)stream, a));
  } else {
    PP_DT_SWITCH(dtype, hipLaunchKernelGGL((ip_attn_add_kernel<EDT, false, MASK>), grid, dim3(IP_T), 0, (hipStream_t)stream, a));
  }
  PP_CHECK_LAUNCH("ip_attn_add_kernel");
  return PP_OK;
}

}  // namespace

extern "C" int pp_ip_attn_add(const void* q, int ldq, const void* k_ip, const void* v_ip, void* o, int ldo, int batch, int heads,
                              int nq, int nk, int d, float qk_scale, float ip_scale, int dtype, void* stream) {
  return ip_attn_add_launch<false>(q, ldq, k_ip, v_ip, o, ldo, batch, heads, nq, nk, d, qk_scale, ip_scale, nullptr, dtype, stream);
}

extern "C" int pp_ip_attn_add_masked(const void* q, int ldq, const void* k_ip, const void* v_ip, void* o, int ldo, int batch,
                                     int heads, int nq, int nk, int d, float qk_scale, float ip_scale, const float* row_w,
                                     int dtype, void* stream) {
  return ip_attn_add_launch<true>(q, ldq, k_ip, v_ip, o, ldo, batch, heads, nq, nk, d, qk_scale, ip_scale, row_w, dtype, stream);
}
