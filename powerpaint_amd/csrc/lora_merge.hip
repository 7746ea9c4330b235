// pp_lora_merge (ABI v23): one packed destination block of a network rebuilt ON THE DEVICE from its fp32 source weight
// plus low-rank adapters,
//     W_eff = W + sum_a c_a U_a D_a          (fp32: an fmaf chain over the rank per adapter, one fmaf per adapter on top of W)
//     out[row_map(n)][col_map(k)] = round16(W_eff[n][k] * gamma[k])
// with the row / column orders of the pack-time layouts of engine.py (_geglu_interleave, _conv_igemm(_cpad), _kperm,
// _kperm_geglu, row and column blocks of concatenated entries) and the fp32 side vectors of a LayerNorm-folded entry
// (colsum of the ROUNDED values, bias = W_eff beta + b) in the same pass.
//
// Tiling: 64 source rows x 64 DESTINATION columns per workgroup step, 256 threads, a 4 x 4 register tile per thread whose
// four columns are consecutive in the destination (16-byte stores in fp32, 8-byte in the 16-bit formats).  The column maps
// permute inside groups of 32 (or gather one tap of a conv), so the source columns of a thread's quad are consecutive for
// plain / _kperm (16-byte loads of W) and gathered otherwise.  U (transposed) and the D panel of the tile sit in LDS in
// chunks of 32 ranks; any rank 1..128 runs (the tail chunk is short, nothing is padded in memory).
// A launch that asks for side vectors walks all column tiles of its 64 rows in one workgroup (fixed summation order: the
// result is reproducible bit for bit, which the adapter round trip relies on); otherwise column tiles spread over grid.y.
#include "pp_common.h"

namespace {
constexpr int LM_ROWS = 64, LM_COLS = 64, LM_RC = 32, LM_ULD = 68;

PP_DEVINL int lm_src_col(const PPLoraMergeArgs& a, int kd) {
  switch (a.col_mode) {
    case PP_LORA_COLS_IGEMM: {
      const int t = kd / a.cin_pad, c = kd - t * a.cin_pad, cin = a.K / a.taps;
      return c < cin ? c * a.taps + t : -1;                      // zero-padded input channel
    }
    case PP_LORA_COLS_KPERM: {
      const int j = kd & 7, kg = (kd >> 3) & 3;
      return (kd & ~31) + 16 * (j >> 2) + 4 * kg + (j & 3);
    }
    case PP_LORA_COLS_KPERM_GEGLU: {
      const int r = kd & 31, kg = r >> 3, q = (r >> 1) & 3, e = r & 1;
      return (kd & ~31) + 8 * q + 2 * kg + e;
    }
    default:
      return kd;
  }
}

PP_DEVINL int lm_dst_row(const PPLoraMergeArgs& a, int n) {
  if (a.row_mode == PP_LORA_ROWS_GEGLU) {
    const int F = a.N >> 1, m = n < F ? n : n - F;
    n = 4 * (m >> 1) + (m & 1) + (n < F ? 0 : 2);
  }
  return a.row_off + n;
}

template <int ODT>
PP_DEVINL float lm_round(float v, uint16_t& h) {
  if constexpr (ODT == PP_DT_F32) {
    h = 0;
    return v;
  } else {
    h = E16<ODT>::from_f(v);
    return E16<ODT>::to_f(h);
  }
}

template <int ODT>
__global__ __launch_bounds__(256) void lora_merge_kernel(const PPLoraMergeArgs a, int Kd, int walk_cols, int vec_load,
                                                         int vec_store) {
  __shared__ __attribute__((aligned(16))) float Dl[LM_RC][LM_COLS];
  __shared__ __attribute__((aligned(16))) float Ul[LM_RC][LM_ULD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.x * LM_ROWS;
  const int ntiles = (Kd + LM_COLS - 1) / LM_COLS;
  const int ct0 = walk_cols ? 0 : (int)blockIdx.y, ct1 = walk_cols ? ntiles : ct0 + 1;
  float cs[4] = {0.f, 0.f, 0.f, 0.f}, bs[4] = {0.f, 0.f, 0.f, 0.f};

  for (int ct = ct0; ct < ct1; ++ct) {
    const int kd0 = ct * LM_COLS;
    const int jl = tid & 63;                                   // the D-panel column this thread gathers
    const int ksl = kd0 + jl < Kd ? lm_src_col(a, kd0 + jl) : -1;
    int ks[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ks[j] = kd0 + tx * 4 + j < Kd ? lm_src_col(a, kd0 + tx * 4 + j) : -1;
    const bool quad = vec_load && ks[0] >= 0 && !(ks[0] & 3) && ks[1] == ks[0] + 1 && ks[2] == ks[0] + 2 && ks[3] == ks[0] + 3;

    float tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + ty * 4 + i;
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[i][j] = 0.f;
      if (n < a.N) {
        const float* wr = a.w + (size_t)n * (size_t)a.ldw;
        if (quad) {
          const f32x4_t v = *reinterpret_cast<const f32x4_t*>(wr + ks[0]);
          tot[i][0] = v[0]; tot[i][1] = v[1]; tot[i][2] = v[2]; tot[i][3] = v[3];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (ks[j] >= 0) tot[i][j] = wr[ks[j]];
        }
      }
    }

    for (int ad = 0; ad < a.n_adapters; ++ad) {
      const int r = a.rank[ad];
      const float* __restrict__ U = a.up[ad];
      const float* __restrict__ D = a.down[ad];
      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
      for (int r0 = 0; r0 < r; r0 += LM_RC) {
        const int rc = r - r0 < LM_RC ? r - r0 : LM_RC;
        __syncthreads();
        for (int rr = tid >> 6; rr < LM_RC; rr += 4)
          Dl[rr][jl] = (rr < rc && ksl >= 0) ? D[(size_t)(r0 + rr) * (size_t)a.K + ksl] : 0.f;
#pragma unroll
        for (int i = 0; i < (LM_ROWS * LM_RC) / 256; ++i) {
          const int e = tid + 256 * i, rr = e & (LM_RC - 1), row = e >> 5;
          Ul[rr][row] = (rr < rc && n0 + row < a.N) ? U[(size_t)(n0 + row) * (size_t)r + r0 + rr] : 0.f;
        }
        __syncthreads();
        for (int rr = 0; rr < rc; ++rr) {
          const f32x4_t u = *reinterpret_cast<const f32x4_t*>(&Ul[rr][ty * 4]);
          const f32x4_t d = *reinterpret_cast<const f32x4_t*>(&Dl[rr][tx * 4]);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(u[i], d[j], acc[i][j]);
        }
      }
      const float c = a.coef[ad];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[i][j] = __builtin_fmaf(c, acc[i][j], tot[i][j]);
    }

    float g[4] = {1.f, 1.f, 1.f, 1.f}, be[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ks[j] >= 0) {
        if (a.gamma) g[j] = a.gamma[ks[j]];
        if (a.beta) be[j] = a.beta[ks[j]];
      }
    const int kdq = kd0 + tx * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + ty * 4 + i;
      if (n >= a.N) continue;
      float v[4];
      uint16_t h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bs[i] = __builtin_fmaf(tot[i][j], be[j], bs[i]);
        v[j] = lm_round<ODT>(a.gamma ? tot[i][j] * g[j] : tot[i][j], h[j]);
        if (kdq + j < Kd) cs[i] += v[j];
      }
      const size_t o = (size_t)lm_dst_row(a, n) * (size_t)a.ldo + (size_t)a.col_off + (size_t)kdq;
      if constexpr (ODT == PP_DT_F32) {
        float* op = reinterpret_cast<float*>(a.out) + o;
        if (vec_store && kdq + 3 < Kd) {
          const f32x4_t q = {v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4_t*>(op) = q;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (kdq + j < Kd) op[j] = v[j];
        }
      } else {
        uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + o;
        if (vec_store && kdq + 3 < Kd) {
          const u32x2_t q = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
          *reinterpret_cast<u32x2_t*>(op) = q;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (kdq + j < Kd) op[j] = h[j];
        }
      }
    }
  }

  if (a.colsum || a.bias) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {                        // the 16 threads of a row quad are consecutive lanes
        cs[i] += __shfl_xor(cs[i], o, 64);
        bs[i] += __shfl_xor(bs[i], o, 64);
      }
      const int n = n0 + ty * 4 + i;
      if (tx == 0 && n < a.N) {
        const int dr = lm_dst_row(a, n);
        if (a.colsum) a.colsum[dr] = cs[i];
        if (a.bias) a.bias[dr] = bs[i] + (a.badd ? a.badd[n] : 0.f);
      }
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int pp_lora_merge(const PPLoraMergeArgs* a, void* stream) {
  if (!a || !a->w || !a->out || a->N <= 0 || a->K <= 0 || a->ldw < a->K || a->ldo <= 0) return PP_ERR_BAD_ARG;
  if (a->n_adapters < 0 || a->n_adapters > PP_LORA_MAX_ADAPTERS) return PP_ERR_BAD_ARG;
  for (int i = 0; i < a->n_adapters; ++i)
    if (!a->up[i] || !a->down[i] || a->rank[i] < 1 || a->rank[i] > PP_LORA_MAX_RANK) return PP_ERR_BAD_ARG;
  if (a->out_dtype != PP_DT_F32 && !pp_dt_ok(a->out_dtype)) return PP_ERR_BAD_ARG;
  if (a->row_mode != PP_LORA_ROWS_PLAIN && a->row_mode != PP_LORA_ROWS_GEGLU) return PP_ERR_BAD_ARG;
  if (a->row_mode == PP_LORA_ROWS_GEGLU && (a->N & 3)) return PP_ERR_BAD_ARG;
  int Kd = a->K;
  switch (a->col_mode) {
    case PP_LORA_COLS_PLAIN:
      break;
    case PP_LORA_COLS_IGEMM:
      if (a->taps < 1 || a->K % a->taps || a->cin_pad < a->K / a->taps) return PP_ERR_BAD_ARG;
      Kd = a->taps * a->cin_pad;
      break;
    case PP_LORA_COLS_KPERM:
    case PP_LORA_COLS_KPERM_GEGLU:
      if (a->K % 32) return PP_ERR_BAD_ARG;
      break;
    default:
      return PP_ERR_BAD_ARG;
  }
  // the block must lie inside the destination matrix the caller describes (nothing is written outside it)
  if (a->row_off < 0 || a->col_off < 0 || (long long)a->row_off + a->N > a->out_rows ||
      (long long)a->col_off + Kd > a->out_cols || a->out_cols > a->ldo)
    return PP_ERR_BAD_ARG;
  if (a->bias && !a->beta && !a->badd) return PP_ERR_BAD_ARG;
  const int esz = a->out_dtype == PP_DT_F32 ? 4 : 2;
  const int vec_load = al16(a->w) && a->ldw % 4 == 0;
  const int vec_store = ((uintptr_t)a->out % (4 * esz)) == 0 && a->ldo % 4 == 0 && a->col_off % 4 == 0;
  const int walk = (a->colsum || a->bias) ? 1 : 0;
  const dim3 grid((a->N + LM_ROWS - 1) / LM_ROWS, walk ? 1 : (Kd + LM_COLS - 1) / LM_COLS);
  if (a->out_dtype == PP_DT_F32)
    hipLaunchKernelGGL(lora_merge_kernel<PP_DT_F32>, grid, dim3(256), 0, (hipStream_t)stream, *a, Kd, walk, vec_load, vec_store);
  else
    PP_DT_SWITCH(a->out_dtype, hipLaunchKernelGGL(lora_merge_kernel<EDT>, grid, dim3(256), 0, (hipStream_t)stream, *a, Kd,
                                                  walk, vec_load, vec_store));
  PP_CHECK_LAUNCH("lora_merge_kernel");
  return PP_OK;
}
