// The kernels AutoencoderTiny (diffusers' `autoencoder_tiny.py` / `vae.py`: EncoderTiny, DecoderTiny, AutoencoderTinyBlock --
// TAESD, the 64-channel norm-free conv net on the SD latent space) adds to the VAE path:
//   pp_conv3x3_c64   the 3x3 pad-1 convolution for exactly 64 -> 64 channels, stride 1, stride 2, or behind a nearest 2x
//                    upsample; bias, residual and ReLU in its epilogue.  The whole weight matrix lives in LDS for the life of
//                    a persistent workgroup, the input tile with its halo is staged in LDS once per tile.
//   pp_taesd_pack    the two boundary maps, NCHW fp32 | 16-bit -> the 8-channel NHWC tensor pp_conv3x3_direct reads:
//                    (x + 1) / 2 of the image, 3 tanh(x / 3) of the latents; the pad channels are written as zeros.
#include "pp_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// conv 3x3, 64 -> 64:  out[b][oy][ox][n] = [relu](bias[n] + res[b][oy][ox][n] + sum_{ky,kx,c} v(oy, ox, ky, kx)[c] w[n][(3 ky + kx) 64 + c])
//   mode 0: v = x[oy - 1 + ky][ox - 1 + kx]          mode 1: v = x[2 oy - 1 + ky][2 ox - 1 + kx]
//   mode 2: v = x[(oy - 1 + ky) >> 1][(ox - 1 + kx) >> 1]  (the padding at the OUTPUT resolution: up-pixels -1 and 2 hin map to
//           source pixels -1 and hin, and to nothing else, so "a source pixel outside the image is zero" is the same rule)
// A 256-thread workgroup owns output tiles of TH rows x 32 columns (TH = 8; 4 at stride 2, whose source tile is four times
// the size) and walks tile ids blockIdx.x, + gridDim.x, ...  LDS: the weights [64][576] (72 KiB, loaded once) and ONE source
// tile; the next tile's source is fetched into registers while the matrix cores work on this one.  Both images are rows of
// 16-byte chunks XOR-swizzled so that the 16 lanes of a ds_read_b128 group fall on 16 different slots of a bank row.
// The weights are the MFMA's A operand, the pixels its B operand (32x32x16): a lane's accumulator registers are four
// consecutive out channels of ONE pixel per quad -> 8-byte residual loads and stores.  Wave w computes all 64 channels of
// rows [w TH/4, (w+1) TH/4) of the tile.  Every output value is one fixed-order sum: it does not depend on the batch size,
// on the item's place in the batch or on which workgroup computes it.  No atomics, no workspace.
// ------------------------------------------------------------------------------------------------------------------
constexpr int C64_T = 256;
constexpr int C64_TW = 32;                          // output columns per tile
constexpr int C64_K = 576;                          // 9 taps x 64 channels
constexpr int C64_WCHUNKS = 64 * (C64_K / 8);       // 16-byte chunks of the weight image

template <int MODE>
struct C64Geo {
  static constexpr int TH = MODE == 1 ? 4 : 8;                                  // output rows per tile
  static constexpr int PB = TH / 4;                                             // output rows (32-pixel blocks) per wave
  static constexpr int SH = MODE == 0 ? TH + 2 : MODE == 1 ? 2 * TH + 1 : TH / 2 + 2;              // source tile rows
  static constexpr int SW = MODE == 0 ? C64_TW + 2 : MODE == 1 ? 2 * C64_TW + 1 : C64_TW / 2 + 2;  // source tile columns
  static constexpr int CHUNKS = SH * SW * 8;
  static constexpr int PER_THREAD = (CHUNKS + C64_T - 1) / C64_T;
  static constexpr int LDS_BYTES = (C64_WCHUNKS + CHUNKS) * 16;
};

struct C64Args {
  const uint16_t* x;
  const uint16_t* w;
  const float* bias;
  const uint16_t* res;
  uint16_t* out;
  int hin, win, hout, wout, tiles_x, tiles_y, tiles, relu;
};

template <int EDT, int MODE>
__global__ void __launch_bounds__(C64_T) conv3x3_c64_kernel(const C64Args a) {
  typedef E16<EDT> E;
  typedef C64Geo<MODE> G;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u32x4_t* wl = reinterpret_cast<u32x4_t*>(smem);    // [64 rows][72 chunks], chunk ^ ((row >> 1) & 7) in its group of 8
  u32x4_t* xl = wl + C64_WCHUNKS;                    // [SH * SW pixels][8 chunks], chunk ^ ((pixel >> 1) & 7)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;

  for (int q = tid; q < C64_WCHUNKS; q += C64_T) {
    const int n = q / 72, c = q - n * 72;
    wl[n * 72 + (c ^ ((n >> 1) & 7))] = *reinterpret_cast<const u32x4_t*>(a.w + (size_t)q * 8);
  }

  u32x4_t pre[G::PER_THREAD];
  // fetch the source tile of tile id t: a pixel outside the image is zero
  auto fetch = [&](int t) {
    const int b = t / (a.tiles_y * a.tiles_x), r = t - b * (a.tiles_y * a.tiles_x);
    const int ty = r / a.tiles_x, tx = r - ty * a.tiles_x;
    const int oy0 = ty * G::TH, ox0 = tx * C64_TW;
    const int sy0 = MODE == 0 ? oy0 - 1 : MODE == 1 ? 2 * oy0 - 1 : oy0 / 2 - 1;
    const int sx0 = MODE == 0 ? ox0 - 1 : MODE == 1 ? 2 * ox0 - 1 : ox0 / 2 - 1;
    const uint16_t* xb = a.x + (size_t)b * a.hin * a.win * 64;
#pragma unroll
    for (int i = 0; i < G::PER_THREAD; ++i) {
      const int q = tid + i * C64_T;
      const int p = q >> 3, c = q & 7;
      const int py = p / G::SW, px = p - py * G::SW;
      const int sy = sy0 + py, sx = sx0 + px;
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (q < G::CHUNKS && sy >= 0 && sy < a.hin && sx >= 0 && sx < a.win)
        v = *reinterpret_cast<const u32x4_t*>(xb + ((size_t)sy * a.win + sx) * 64 + c * 8);
      pre[i] = v;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < G::PER_THREAD; ++i) {
      const int q = tid + i * C64_T;
      const int p = q >> 3, c = q & 7;
      if (q < G::CHUNKS) xl[p * 8 + (c ^ ((p >> 1) & 7))] = pre[i];
    }
  };

  int t = blockIdx.x;
  if (t < a.tiles) fetch(t);
  for (; t < a.tiles; t += gridDim.x) {
    __syncthreads();                                 // every wave has left the previous tile's source (and, first, the weights are stored)
    stage();
    __syncthreads();
    if (t + (int)gridDim.x < a.tiles) fetch(t + gridDim.x);

    f32x16_t acc[2][G::PB];                          // [out-channel block j][row i of the wave]
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < G::PB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      int p[G::PB];
#pragma unroll
      for (int i = 0; i < G::PB; ++i) {
        const int ry = wave * G::PB + i;
        if (MODE == 0) p[i] = (ry + ky) * G::SW + l31 + kx;
        if (MODE == 1) p[i] = (2 * ry + ky) * G::SW + 2 * l31 + kx;
        if (MODE == 2) p[i] = ((ry + ky + 1) >> 1) * G::SW + ((l31 + kx + 1) >> 1);
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int c = 2 * kk + lh;
        typename E::v8 wf[2], xf[G::PB];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = j * 32 + l31;
          wf[j] = __builtin_bit_cast(typename E::v8, wl[n * 72 + tap * 8 + (c ^ ((n >> 1) & 7))]);
        }
#pragma unroll
        for (int i = 0; i < G::PB; ++i) xf[i] = __builtin_bit_cast(typename E::v8, xl[p[i] * 8 + (c ^ ((p[i] >> 1) & 7))]);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < G::PB; ++i) acc[j][i] = E::mfma32(wf[j], xf[i], acc[j][i]);
      }
    }

    // accumulator of block (j, i): column = lane & 31 = the pixel, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) = the out channel
    const int b = t / (a.tiles_y * a.tiles_x), r = t - b * (a.tiles_y * a.tiles_x);
    const int ty = r / a.tiles_x, tx = r - ty * a.tiles_x;
    const int ox = tx * C64_TW + l31;
#pragma unroll
    for (int i = 0; i < G::PB; ++i) {
      const int oy = ty * G::TH + wave * G::PB + i;
      if (oy >= a.hout || ox >= a.wout) continue;
      const size_t off = (((size_t)b * a.hout + oy) * a.wout + ox) * 64;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = j * 32 + 8 * g + 4 * lh;
          float v0 = acc[j][i][4 * g], v1 = acc[j][i][4 * g + 1], v2 = acc[j][i][4 * g + 2], v3 = acc[j][i][4 * g + 3];
          if (a.bias) {
            const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(a.bias + n);
            v0 += bv[0]; v1 += bv[1]; v2 += bv[2]; v3 += bv[3];
          }
          if (a.res) {
            const u32x2_t rv = *reinterpret_cast<const u32x2_t*>(a.res + off + n);
            v0 += E::lo(rv[0]); v1 += E::hi(rv[0]); v2 += E::lo(rv[1]); v3 += E::hi(rv[1]);
          }
          if (a.relu) {
            v0 = __builtin_fmaxf(v0, 0.f); v1 = __builtin_fmaxf(v1, 0.f);
            v2 = __builtin_fmaxf(v2, 0.f); v3 = __builtin_fmaxf(v3, 0.f);
          }
          u32x2_t o;
          o[0] = E::pack2(v0, v1);
          o[1] = E::pack2(v2, v3);
          *reinterpret_cast<u32x2_t*>(a.out + off + n) = o;
        }
      }
    }
  }
}

template <int EDT, int MODE>
int c64_launch(const C64Args& a, int grid, hipStream_t st) {
  const int lds = C64Geo<MODE>::LDS_BYTES;
  if (pp_func_lds((const void*)conv3x3_c64_kernel<EDT, MODE>, lds, "conv3x3_c64_kernel") != PP_OK) return PP_ERR_LAUNCH;
  hipLaunchKernelGGL((conv3x3_c64_kernel<EDT, MODE>), dim3((unsigned)grid), dim3(C64_T), lds, st, a);
  PP_CHECK_LAUNCH("conv3x3_c64_kernel");
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// boundary maps: one thread per pixel, planes in (coalesced along pixels), one 16-byte pixel out
// ------------------------------------------------------------------------------------------------------------------
template <int SDT>
PP_DEVINL float pack_src(const void* src, size_t i) {
  if (SDT == PP_DT_F32) return reinterpret_cast<const float*>(src)[i];
  return E16<SDT == PP_DT_F32 ? PP_DT_BF16 : SDT>::to_f(reinterpret_cast<const uint16_t*>(src)[i]);
}

template <int EDT, int SDT>
__global__ void __launch_bounds__(256) taesd_pack_kernel(const void* __restrict__ src, int c, long long hw, int mode,
                                                         u32x4_t* __restrict__ out) {
  typedef E16<EDT> E;
  const int b = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float f = 0.f;
    if (k < c) {
      const float s = pack_src<SDT>(src, ((size_t)b * c + k) * hw + p);
      f = mode == 0 ? (s + 1.0f) * 0.5f : 3.0f * tanhf(s / 3.0f);
    }
    v[k] = f;
  }
  u32x4_t o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = E::pack2(v[2 * k], v[2 * k + 1]);
  out[(size_t)b * hw + p] = o;
}

}  // namespace

extern "C" int pp_conv3x3_c64(const void* x, int batch, int hin, int win, const void* w, const float* bias, const void* res,
                              int mode, int relu, void* out, int dtype, void* stream) {
  if (!x || !w || !out || !pp_dt_ok(dtype) || mode < 0 || mode > 2 || batch <= 0 || hin <= 0 || win <= 0) return PP_ERR_BAD_ARG;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias) & 15) || (((uintptr_t)out | (uintptr_t)res) & 7)) return PP_ERR_BAD_ARG;
  if (hin > (1 << 28) || win > (1 << 28)) return PP_ERR_UNSUPPORTED;
  C64Args a;
  a.x = (const uint16_t*)x;
  a.w = (const uint16_t*)w;
  a.bias = bias;
  a.res = (const uint16_t*)res;
  a.out = (uint16_t*)out;
  a.hin = hin; a.win = win;
  a.hout = mode == 0 ? hin : mode == 1 ? (hin - 1) / 2 + 1 : 2 * hin;
  a.wout = mode == 0 ? win : mode == 1 ? (win - 1) / 2 + 1 : 2 * win;
  a.relu = relu ? 1 : 0;
  const int th = mode == 1 ? C64Geo<1>::TH : C64Geo<0>::TH;
  a.tiles_x = (a.wout + C64_TW - 1) / C64_TW;
  a.tiles_y = (a.hout + th - 1) / th;
  const long long tiles = (long long)batch * a.tiles_y * a.tiles_x;
  if (tiles > 0x7fffffffLL / 2) return PP_ERR_UNSUPPORTED;
  a.tiles = (int)tiles;
  const int grid = (int)(tiles < pp_cu_count() ? tiles : pp_cu_count());
  const hipStream_t st = (hipStream_t)stream;
  if (mode == 0) PP_DT_SWITCH(dtype, return (c64_launch<EDT, 0>(a, grid, st)));
  if (mode == 1) PP_DT_SWITCH(dtype, return (c64_launch<EDT, 1>(a, grid, st)));
  PP_DT_SWITCH(dtype, return (c64_launch<EDT, 2>(a, grid, st)));
  return PP_OK;
}

extern "C" int pp_taesd_pack(const void* src, int src_dtype, int batch, int c, int h, int w, int mode, void* out, int dtype,
                             void* stream) {
  if (!src || !out || !pp_dt_ok(dtype) || src_dtype < PP_DT_F32 || src_dtype > PP_DT_F16 || mode < 0 || mode > 1) return PP_ERR_BAD_ARG;
  if (batch <= 0 || batch > 65535 || c <= 0 || c > 8 || h <= 0 || w <= 0) return PP_ERR_BAD_ARG;
  if (((uintptr_t)src & (src_dtype == PP_DT_F32 ? 3 : 1)) || ((uintptr_t)out & 15)) return PP_ERR_BAD_ARG;
  const long long hw = (long long)h * w;
  const long long nb = (hw + 255) / 256;
  if (nb > 0x7fffffffLL) return PP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)nb, batch);
  const hipStream_t st = (hipStream_t)stream;
  u32x4_t* o = (u32x4_t*)out;
  if (src_dtype == PP_DT_F32)
    PP_DT_SWITCH(dtype, hipLaunchKernelGGL((taesd_pack_kernel<EDT, PP_DT_F32>), grid, dim3(256), 0, st, src, c, hw, mode, o));
  else if (src_dtype == PP_DT_BF16)
    PP_DT_SWITCH(dtype, hipLaunchKernelGGL((taesd_pack_kernel<EDT, PP_DT_BF16>), grid, dim3(256), 0, st, src, c, hw, mode, o));
  else
    PP_DT_SWITCH(dtype, hipLaunchKernelGGL((taesd_pack_kernel<EDT, PP_DT_F16>), grid, dim3(256), 0, st, src, c, hw, mode, o));
  PP_CHECK_LAUNCH("taesd_pack_kernel");
  return PP_OK;
}
