// pp_perceiver_attn: the attention of IP-Adapter Plus's Resampler (include/pp_hip.h, "IP-Adapter Plus") -- a handful of
// latent queries over the keys of TWO row-major [K | V] segments (the image rows, then the latent rows: the two outputs of
// the to_kv GEMMs), never concatenated:
//     o[b,i,h] = softmax_t(scale * q[b,i,h] . K[b,t,h]) V[b,t,h],   t over nx + nl keys,   d = 64.
//
// Work layout.  One wave per (16-query tile, head, batch item); it walks the keys 32 at a time with a running maximum and
// sum, so there is no cap on nx + nl.  Both products run on v_mfma_f32_16x16x32 in their TRANSPOSED form, which needs no
// lane movement between them:
//   S^T = K Q^T : A = K (row = key: one 16-byte global load per lane and k-step, straight from the segment's row), B = Q^T
//                 (column = query, loaded once).  Lane (c = lane & 15, g = lane >> 4) then holds, for query c, the scores
//                 of keys 16 j + 4 g + r (j = 0, 1: the two 16-key halves of the tile; r = 0..3).
//   O^T = V^T P^T : those 8 probabilities, rounded once to the 16-bit format, ARE the lane's B fragment (column = query c)
//                 under the contraction order  slot e -> key 16 (e >> 2) + 4 g + (e & 3);  the A operand (row = channel)
//                 reads V in the same order from the tile's LDS image -- V goes global -> LDS as 16-byte row chunks and
//                 comes back as 16-bit column reads (row stride 72 elements: the four lane groups land 16 banks apart).
//                 Lane holds O^T rows 16 dt + 4 g + r of column c: four consecutive channels of its query, 8-byte stores.
// Scores, the softmax (maximum subtracted; the sum is taken over the UNROUNDED probabilities) and the accumulation are fp32;
// the probabilities are rounded to the 16-bit format for the second MFMA; one rounding of the result at the store.
// Keys past nx + nl score -inf and their V rows enter LDS as zeros; queries past nq load zeros and store nothing; a tile
// always holds at least one real key, so the running maximum is finite from the first tile on.
#include "pp_common.h"

namespace {

constexpr int PA_D = 64;       // head dimension (the Resampler's format fixes it)
constexpr int PA_QT = 16;      // queries per workgroup: one MFMA N tile
constexpr int PA_KT = 32;      // keys per step: one MFMA k-step of the second product
constexpr int PA_VLD = 72;     // LDS row stride of the V tile, elements (144 bytes: 16-byte aligned rows, 36 banks)

struct PaArgs {
  const uint16_t* q;
  const uint16_t* kx;
  const uint16_t* kl;
  uint16_t* o;
  long long ldq, ldkx, ldkl, ldo;
  int nq, nx, nl, heads;
  float scale;
};

template <int DT>
__global__ __launch_bounds__(64) void perceiver_attn_kernel(const PaArgs a) {
  typedef E16<DT> E;
  typedef typename E::v8 v8;
  __shared__ __attribute__((aligned(16))) uint16_t vs[PA_KT * PA_VLD];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * PA_QT, h = blockIdx.y, b = blockIdx.z;
  const int nk = a.nx + a.nl;
  const size_t vcol = (size_t)a.heads * PA_D + (size_t)h * PA_D;      // first V column of this head in a [K | V] row
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  // first element of key kk's row (kk < nk) of this batch item
  auto key_row = [&](int kk) -> const uint16_t* {
    return kk < a.nx ? a.kx + ((size_t)b * a.nx + kk) * a.ldkx : a.kl + ((size_t)b * a.nl + (kk - a.nx)) * a.ldkl;
  };

  const int qi = q0 + c;
  const bool q_on = qi < a.nq;
  u32x4_t qf[2];
  {
    const uint16_t* qp = a.q + ((size_t)b * a.nq + (q_on ? qi : 0)) * a.ldq + (size_t)h * PA_D + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = q_on ? *reinterpret_cast<const u32x4_t*>(qp + 32 * ks) : zero4;
  }

  f32x4_t acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;      // lsum: this lane's share (its 8 keys per tile) of the query's denominator

  for (int k0 = 0; k0 < nk; k0 += PA_KT) {
    u32x4_t kf[2][2], vf[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k0 + 16 * j + c;
      const bool on = kk < nk;
      const uint16_t* kp = key_row(on ? kk : 0) + (size_t)h * PA_D + 8 * g;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[j][ks] = on ? *reinterpret_cast<const u32x4_t*>(kp + 32 * ks) : zero4;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int id = lane + 64 * t, kk = k0 + (id >> 3);
      const bool on = kk < nk;
      vf[t] = on ? *reinterpret_cast<const u32x4_t*>(key_row(on ? kk : 0) + vcol + 8 * (id & 7)) : zero4;
    }
    __syncthreads();                      // the previous tile's column reads are done
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int id = lane + 64 * t;
      *reinterpret_cast<u32x4_t*>(&vs[(id >> 3) * PA_VLD + 8 * (id & 7)]) = vf[t];
    }
    __syncthreads();

    f32x4_t s[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      s[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        s[j] = E::mfma16(__builtin_bit_cast(v8, kf[j][ks]), __builtin_bit_cast(v8, qf[ks]), s[j]);
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = (k0 + 16 * j + 4 * g + r < nk) ? s[j][r] * a.scale : -INFINITY;
        tmax = fmaxf(tmax, s[j][r]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));      // (the tile's first key is real: finite in every lane)
    const float mn = fmaxf(m, tmax);
    const float corr = __expf(m - mn);                 // (first tile: exp(-inf) = 0)
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = __expf(s[j][r] - mn);                // (a key past nk: exp(-inf) = 0)
        psum += s[j][r];
      }
    lsum = __builtin_fmaf(lsum, corr, psum);
    m = mn;
    u32x4_t pu;
    pu[0] = E::pack2(s[0][0], s[0][1]);
    pu[1] = E::pack2(s[0][2], s[0][3]);
    pu[2] = E::pack2(s[1][0], s[1][1]);
    pu[3] = E::pack2(s[1][2], s[1][3]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      u32x4_t vu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {                    // slots 2 i, 2 i + 1 -> keys 16 (i >> 1) + 4 g + 2 (i & 1) + {0, 1}
        const int key = 16 * (i >> 1) + 4 * g + 2 * (i & 1);
        const uint32_t lo = vs[key * PA_VLD + 16 * dt + c], hi = vs[(key + 1) * PA_VLD + 16 * dt + c];
        vu[i] = lo | (hi << 16);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[dt][r] *= corr;
      acc[dt] = E::mfma16(__builtin_bit_cast(v8, vu), __builtin_bit_cast(v8, pu), acc[dt]);
    }
  }

  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (q_on) {
    const float inv = 1.0f / lsum;                     // (lsum >= 1: the maximum's own term)
    uint16_t* op = a.o + ((size_t)b * a.nq + qi) * a.ldo + (size_t)h * PA_D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      u32x2_t out;
      out[0] = E::pack2(acc[dt][0] * inv, acc[dt][1] * inv);
      out[1] = E::pack2(acc[dt][2] * inv, acc[dt][3] * inv);
      *reinterpret_cast<u32x2_t*>(op + 16 * dt) = out;
    }
  }
}

}  // namespace

extern "C" int pp_perceiver_attn(const void* q, int ldq, const void* kv_x, int ldkx, int nx, const void* kv_l, int ldkl, int nl,
                                 void* o, int ldo, int batch, int heads, int nq, int d, float scale, int dtype, void* stream) {
  if (!q || !kv_x || !o || !pp_dt_ok(dtype)) return PP_ERR_BAD_ARG;
  if (batch <= 0 || heads <= 0 || nq <= 0 || nx <= 0 || nl < 0 || d <= 0) return PP_ERR_BAD_ARG;
  if ((nl > 0) != (kv_l != nullptr)) return PP_ERR_BAD_ARG;
  if (d != PA_D) return PP_ERR_UNSUPPORTED;
  if (batch > 65535 || heads > 65535 || (long long)nx + nl > (1 << 30)) return PP_ERR_UNSUPPORTED;
  const int C = heads * PA_D;
  if (ldq < C || ldo < C || ldkx < 2 * C || ldq % 8 || ldo % 8 || ldkx % 8) return PP_ERR_BAD_ARG;
  if (nl > 0 && (ldkl < 2 * C || ldkl % 8)) return PP_ERR_BAD_ARG;
  if (((uintptr_t)q | (uintptr_t)kv_x | (uintptr_t)kv_l | (uintptr_t)o) & 15) return PP_ERR_BAD_ARG;
  if (q == o || !(scale == scale)) return PP_ERR_BAD_ARG;
  PaArgs a;
  a.q = (const uint16_t*)q;
  a.kx = (const uint16_t*)kv_x;
  a.kl = (const uint16_t*)kv_l;
  a.o = (uint16_t*)o;
  a.ldq = ldq; a.ldkx = ldkx; a.ldkl = nl > 0 ? ldkl : 0; a.ldo = ldo;
  a.nq = nq; a.nx = nx; a.nl = nl; a.heads = heads;
  a.scale = scale;
  const dim3 grid((unsigned)((nq + PA_QT - 1) / PA_QT), (unsigned)heads, (unsigned)batch);
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL((perceiver_attn_kernel<EDT>), grid, dim3(64), 0, (hipStream_t)stream, a));
  PP_CHECK_LAUNCH("perceiver_attn_kernel");
  return PP_OK;
}
