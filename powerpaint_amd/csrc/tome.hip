// Token merging (ToMe for Stable Diffusion, Bolya & Hoffman 2023) in front of a self-attention (include/pp_hip.h, "Token
// merging").  Four launches between "Q | K and V^T written" and "attention output read":
//
//   pp_tome_match    per source token: argmax over the destination tokens of the cosine of the two hidden-state rows.  A GEMM
//                    with an arg-max epilogue: S^T = D X^T on v_mfma_f32_32x32x16 (A operand = 32 destination rows, B operand =
//                    32 token rows), so a lane owns ONE token column and 16 of the 32 destinations of a block -- the running
//                    (maximum, destination) is a per-lane scalar pair, joined across the two lane halves once at the end.  A
//                    workgroup owns 128 tokens (4 waves x 32) and walks every 64-destination tile; both operands are staged
//                    through LDS in 64-deep chunks of the contraction (any C that is a multiple of 8), the next chunk in flight
//                    in registers behind the MFMAs of the current one.  The sums of squares of the rows are taken from the same
//                    staged 16-bit values (fixed order: 8 partial sums per row, joined by lane exchanges), the inverse norms
//                    multiply the fp32 dot product.  ALL tokens are walked as columns, the destinations among them too (their
//                    result is discarded): 1 / (sx sy) of the MFMAs buys a token tile that needs no index list.
//   pp_tome_select   one workgroup per batch item: the r sources with the highest score (radix select on the order-preserving
//                    integer image of the score, four 8-bit passes; equal scores in ascending token order), the merged-sequence
//                    row of every token by two prefix sums, and the per-destination lists of merged sources by a bitonic sort
//                    of (destination rank, token) keys in LDS -- ascending token order inside a list, whatever the input.
//   pp_tome_merge    merged Q | K rows and merged V^T columns: fp32 sums in list order, one division, one rounding.
//   pp_tome_unmerge  row gather of the attention output through pos.
// Integer LDS atomics build the select's histograms (their result does not depend on the order); no floating-point atomic
// anywhere: the same inputs give the same bits.
#include "pp_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- match
constexpr int M_T = 256;            // threads (4 waves)
constexpr int M_SRC = 128;          // token columns per workgroup
constexpr int M_DST = 64;           // destinations per tile
constexpr int M_KC = 64;            // contraction chunk
constexpr int M_RS = M_KC * 2 + 16; // LDS row stride in bytes: an odd number of 16-byte slots
constexpr int M_BUF = (M_SRC + M_DST) * M_RS;

struct MatchArgs {
  const uint16_t* x;
  long long ldx;
  int N, w, C, sx, sy, wsx, nd;
  const uint8_t* table;
  int row_stride, rows;
  const int* row_idx;
  int* best;
  float* score;
};

// token of destination window `win` under the table row `tb` (in-window index k -> row k / sx, column k % sx)
PP_DEVINL int win_token(const MatchArgs& a, const uint8_t* tb, int win) {
  const int k = min((int)tb[win], a.sx * a.sy - 1);
  const int wy = win / a.wsx, wx = win - wy * a.wsx;
  return (wy * a.sy + k / a.sx) * a.w + wx * a.sx + k % a.sx;
}

PP_DEVINL bool token_is_dst(const MatchArgs& a, const uint8_t* tb, int t) {
  const int y = t / a.w, x = t - y * a.w;
  const int wy = y / a.sy, wx = x / a.sx;
  if (wx >= a.wsx || wy * a.wsx + wx >= a.nd) return false;      // leftover rows and columns are sources
  return win_token(a, tb, wy * a.wsx + wx) == t;
}

template <int DT>
PP_DEVINL float sumsq8(const u32x4_t u, float s) {
  typedef E16<DT> E;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = E::lo(u[i]), hi = E::hi(u[i]);
    s = __builtin_fmaf(lo, lo, s);
    s = __builtin_fmaf(hi, hi, s);
  }
  return s;
}

PP_DEVINL float group8_sum(float v) {      // the 8 lanes that staged the pieces of one row
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

template <int DT>
__global__ void __launch_bounds__(M_T, 2) tome_match_kernel(const MatchArgs a) {
  typedef E16<DT> E;
  typedef typename E::v8 v8_t;
  __shared__ __attribute__((aligned(16))) char smem[2 * M_BUF];
  __shared__ float dinv_s[M_DST];
  __shared__ float sinv_s[M_SRC];
  __shared__ int dtok_s[2][M_DST];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = lane & 31, half = lane >> 5;
  const int b = blockIdx.y, s0 = blockIdx.x * M_SRC;
  int ri = a.row_idx ? *a.row_idx : 0;
  ri = ri < 0 ? 0 : (ri >= a.rows ? a.rows - 1 : ri);
  const uint8_t* tb = a.table + (size_t)ri * a.row_stride;
  const uint16_t* xb = a.x + (size_t)b * a.N * a.ldx;
  const int nkc = (a.C + M_KC - 1) / M_KC, ndt = (a.nd + M_DST - 1) / M_DST;
  const int total = nkc * ndt;
  const int prow = tid >> 3, sl = tid & 7;      // piece i of a thread: row prow + 32 i, 16-byte slot sl of the chunk

  const uint16_t* sp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = s0 + prow + 32 * i;
    sp[i] = xb + (size_t)(t < a.N ? t : 0) * a.ldx;
  }
  const uint16_t* dp[2];
  u32x4_t sreg[4], dreg[2];
  float ss_s[4] = {0.f, 0.f, 0.f, 0.f}, ss_d[2] = {0.f, 0.f};

  auto load_chunk = [&](int it) {
    const int dt = it / nkc, kc = it - dt * nkc;
    if (kc == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int win = dt * M_DST + prow + 32 * i;
        const int tok = win < a.nd ? win_token(a, tb, win) : -1;
        dp[i] = xb + (size_t)(tok < 0 ? 0 : tok) * a.ldx;
        if (sl == 0) dtok_s[dt & 1][prow + 32 * i] = tok;
      }
    }
    const int k0 = kc * M_KC + sl * 8;
    const u32x4_t zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) sreg[i] = k0 < a.C ? *reinterpret_cast<const u32x4_t*>(sp[i] + k0) : zero4;
#pragma unroll
    for (int i = 0; i < 2; ++i) dreg[i] = k0 < a.C ? *reinterpret_cast<const u32x4_t*>(dp[i] + k0) : zero4;
  };
  auto store_chunk = [&](int it) {
    char* sb = smem + (it & 1) * M_BUF;
    char* db = sb + M_SRC * M_RS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4_t*>(sb + (prow + 32 * i) * M_RS + sl * 16) = sreg[i];
      if (it < nkc) ss_s[i] = sumsq8<DT>(sreg[i], ss_s[i]);      // (the token rows are the same for every destination tile)
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4_t*>(db + (prow + 32 * i) * M_RS + sl * 16) = dreg[i];
      ss_d[i] = sumsq8<DT>(dreg[i], ss_d[i]);
    }
  };

  f32x16_t sacc[2];
  float bv = -INFINITY;
  int bt = 0x7fffffff;

  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int dt = it / nkc, kc = it - dt * nkc;
    const bool more = it + 1 < total;
    if (more) load_chunk(it + 1);
    if (kc == 0) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[j][r] = 0.f;
    }
    const char* sb = smem + (it & 1) * M_BUF;
    const char* db = sb + M_SRC * M_RS;
#pragma unroll
    for (int s = 0; s < M_KC / 16; ++s) {
      const v8_t xf = *reinterpret_cast<const v8_t*>(sb + (wave * 32 + qi) * M_RS + (16 * s + 8 * half) * 2);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const v8_t df = *reinterpret_cast<const v8_t*>(db + (32 * j + qi) * M_RS + (16 * s + 8 * half) * 2);
        sacc[j] = E::mfma32(df, xf, sacc[j]);
      }
    }
    if (kc == nkc - 1) {
      // every chunk of this destination tile has been staged (and none of the next): its sums of squares are complete
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float ss = group8_sum(ss_d[i]);
        if (sl == 0) dinv_s[prow + 32 * i] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
        ss_d[i] = 0.f;
      }
      if (dt == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float ss = group8_sum(ss_s[i]);
          if (sl == 0) sinv_s[prow + 32 * i] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
        }
      }
      __syncthreads();
      // C/D layout: column = lane & 31 (the token), row = (r & 3) + 8 (r >> 2) + 4 half (the destination of the block)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dl = 32 * j + (r & 3) + 8 * (r >> 2) + 4 * half;
          const int tok = dtok_s[dt & 1][dl];
          const float s = sacc[j][r] * dinv_s[dl];
          if (tok >= 0 && (s > bv || (s == bv && tok < bt))) {
            bv = s;
            bt = tok;
          }
        }
    }
    if (more) store_chunk(it + 1);
    __syncthreads();
  }
  {   // the other 16 destinations of every block live in the other lane half
    const float ov = __shfl_xor(bv, 32, 64);
    const int ot = __shfl_xor(bt, 32, 64);
    if (ov > bv || (ov == bv && ot < bt)) {
      bv = ov;
      bt = ot;
    }
  }
  const int row = wave * 32 + qi, t = s0 + row;
  if (half == 0 && t < a.N) {
    const bool isd = token_is_dst(a, tb, t);
    a.best[(size_t)b * a.N + t] = isd ? -1 : bt;
    a.score[(size_t)b * a.N + t] = isd ? -2.0f : bv * sinv_s[row];
  }
}

// --------------------------------------------------------------------------------------------------------------- select
constexpr int S_T = 1024;
static_assert(PP_TOME_MAX_TOKENS / S_T <= 32, "a thread's tokens are one bit each of a 32-bit mask");
static_assert(PP_TOME_MAX_TOKENS <= (1 << 14), "(destination rank, token) sort keys pack two 14-bit fields");

PP_DEVINL uint32_t score_key(float f) {                   // order-preserving image of a float in the unsigned integers
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total; wsum: S_T / 64 words of LDS
PP_DEVINL uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();                      // (wsum is free of its previous use)
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int i = 0; i < S_T / 64; ++i) {
    const uint32_t s = wsum[i];
    if (i < wave) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

__global__ void __launch_bounds__(S_T) tome_select_kernel(const int* __restrict__ best, const float* __restrict__ score, int N,
                                                          int nd, int r, int P, int* __restrict__ pos, int* __restrict__ rowtok,
                                                          int* __restrict__ seg, int* __restrict__ lst) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  uint32_t* keys = reinterpret_cast<uint32_t*>(sm);           // [P]: the sort's keys
  uint16_t* posl = reinterpret_cast<uint16_t*>(keys + P);     // [N]: merged-sequence row of the kept and destination tokens
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[S_T / 64];
  __shared__ uint32_t bc[2];
  const int tid = threadIdx.x, b = blockIdx.x;
  best += (size_t)b * N;
  score += (size_t)b * N;
  pos += (size_t)b * N;
  rowtok += (size_t)b * (N - r);
  seg += (size_t)b * (nd + 1);
  lst += (size_t)b * r;
  const int nkept = N - nd - r;
  const int per = (N + S_T - 1) / S_T;
  const int t0 = min(tid * per, N), t1 = min(t0 + per, N);

  // the key of the r-th highest score among the sources, and how many tokens of exactly that key are still to take
  uint32_t thr = 0, remaining = (uint32_t)r;
  if (r > 0) {
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int i = tid; i < 256; i += S_T) hist[i] = 0;
      __syncthreads();
      for (int t = t0; t < t1; ++t)
        if (best[t] >= 0) {
          const uint32_t k = score_key(score[t]);
          if (pass == 0 || (k >> (shift + 8)) == thr) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
      __syncthreads();
      if (tid == 0) {
        uint32_t cum = 0;
        int bin = 255;
        for (; bin > 0; --bin) {
          if (cum + hist[bin] >= remaining) break;
          cum += hist[bin];
        }
        bc[0] = (uint32_t)bin;
        bc[1] = remaining - cum;
      }
      __syncthreads();
      thr = (thr << 8) | bc[0];
      remaining = bc[1];
    }
  }
  // merged = key above the threshold, or equal to it and among the first `remaining` such tokens
  uint32_t eq = 0;
  if (r > 0)
    for (int t = t0; t < t1; ++t) eq += (best[t] >= 0 && score_key(score[t]) == thr) ? 1u : 0u;
  uint32_t tot;
  uint32_t eqrank = block_excl_scan(eq, wsum, &tot);
  uint32_t mmask = 0, cnt = 0;          // bit i: token t0 + i is merged; cnt: kept sources | destinations << 16
  for (int t = t0; t < t1; ++t) {
    const int bd = best[t];
    bool merged = false;
    if (bd >= 0 && r > 0) {
      const uint32_t k = score_key(score[t]);
      merged = k > thr || (k == thr && eqrank++ < remaining);
    }
    if (merged) mmask |= 1u << (t - t0);
    else cnt += bd >= 0 ? 1u : 0x10000u;
  }
  const uint32_t base = block_excl_scan(cnt, wsum, &tot);
  uint32_t kb = base & 0xffffu, db = base >> 16;
  for (int t = t0; t < t1; ++t) {
    if (mmask & (1u << (t - t0))) continue;
    const int p = best[t] >= 0 ? (int)kb++ : nkept + (int)db++;
    posl[t] = (uint16_t)p;
    rowtok[p] = t;
    pos[t] = p;
  }
  for (int i = N + tid; i < P; i += S_T) keys[i] = 0xffffffffu;
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    uint32_t k = 0xffffffffu;
    if (mmask & (1u << (t - t0))) {
      const int p = posl[best[t]];
      pos[t] = p;
      k = ((uint32_t)(p - nkept) << 14) | (uint32_t)t;       // (destination rank, token): PP_TOME_MAX_TOKENS = 2^14
    }
    keys[t] = k;
  }
  __syncthreads();
  if (r > 0) {
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P / 2; i += S_T) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
          const bool up = (lo & k) == 0;
          const uint32_t x = keys[lo], y = keys[hi];
          if ((x > y) == up) {
            keys[lo] = y;
            keys[hi] = x;
          }
        }
        __syncthreads();
      }
  }
  for (int i = tid; i < r; i += S_T) lst[i] = (int)(keys[i] & 0x3fffu);
  for (int d = tid; d <= nd; d += S_T) {          // seg[d]: first list entry of destination rank d (lower bound of d << 14)
    const uint32_t want = (uint32_t)d << 14;
    int lo = 0, hi = r;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    seg[d] = lo;
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
struct MergeArgs {
  const uint16_t* qk;
  const uint16_t* vt;
  uint16_t* qk_out;
  uint16_t* vt_out;
  long long ldqk, ldvt, ldqk_out, ldvt_out;
  int N, C, nd, r, nm, nkept;
  int qk_blocks, vt_mtiles, vcols;
  const int* rowtok;
  const int* seg;
  const int* lst;
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

// blockIdx.x < qk_blocks: four merged Q | K rows (one per wave); behind them: a 64-column x 64-channel tile of merged V^T
template <int DT>
__global__ void __launch_bounds__(256) tome_merge_kernel(const MergeArgs a) {
  typedef E16<DT> E;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int* rowtok = a.rowtok + (size_t)b * a.nm;
  const int* seg = a.seg + (size_t)b * (a.nd + 1);
  const int* lst = a.lst + (size_t)b * a.r;
  if ((int)blockIdx.x < a.qk_blocks) {
    const int m = blockIdx.x * 4 + wave;
    if (m >= a.nm) return;
    const int tok = rowtok[m];
    int l0 = 0, l1 = 0;
    if (m >= a.nkept) {
      l0 = seg[m - a.nkept];
      l1 = seg[m - a.nkept + 1];
    }
    const uint16_t* in = a.qk + (size_t)b * a.N * a.ldqk;
    uint16_t* out = a.qk_out + ((size_t)b * a.nm + m) * a.ldqk_out;
    for (int pc = lane; pc < a.C / 4; pc += 64) {            // 2 C columns in pieces of 8
      u32x4_t v = *reinterpret_cast<const u32x4_t*>(in + (size_t)tok * a.ldqk + pc * 8);
      if (l1 > l0) {
        float acc[8];
        unpack8<DT>(v, acc);
        for (int i = l0; i < l1; ++i) {
          float f[8];
          unpack8<DT>(*reinterpret_cast<const u32x4_t*>(in + (size_t)lst[i] * a.ldqk + pc * 8), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += f[e];
        }
        const float n = (float)(l1 - l0 + 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = E::pack2(acc[2 * e] / n, acc[2 * e + 1] / n);
      }
      *reinterpret_cast<u32x4_t*>(out + pc * 8) = v;
    }
    return;
  }
  const int vb = blockIdx.x - a.qk_blocks;
  const int mt = vb % a.vt_mtiles, ct = vb / a.vt_mtiles;
  const int m = mt * 64 + lane;
  if (m >= a.vcols) return;
  int tok = 0, l0 = 0, l1 = 0;
  if (m < a.nm) {
    tok = rowtok[m];
    if (m >= a.nkept) {
      l0 = seg[m - a.nkept];
      l1 = seg[m - a.nkept + 1];
    }
  }
  const float n = (float)(l1 - l0 + 1);
  const int cend = min(ct * 64 + 64, a.C);
  for (int c = ct * 64 + wave; c < cend; c += 4) {
    const uint16_t* in = a.vt + ((size_t)b * a.C + c) * a.ldvt;
    uint16_t o = 0;                                          // (the padding columns [nm, round8(nm)) hold zeros)
    if (m < a.nm) {
      o = in[tok];
      if (l1 > l0) {
        float acc = E::to_f(o);
        for (int i = l0; i < l1; ++i) acc += E::to_f(in[lst[i]]);
        o = E::from_f(acc / n);
      }
    }
    a.vt_out[((size_t)b * a.C + c) * a.ldvt_out + m] = o;
  }
}

// -------------------------------------------------------------------------------------------------------------- unmerge
__global__ void __launch_bounds__(256) tome_unmerge_kernel(const uint16_t* __restrict__ in, long long ldi,
                                                           const int* __restrict__ pos, int N, int nm, int C,
                                                           uint16_t* __restrict__ out, long long ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y, t = blockIdx.x * 4 + wave;
  if (t >= N) return;
  int p = pos[(size_t)b * N + t];
  p = p < 0 ? 0 : (p >= nm ? nm - 1 : p);
  const uint16_t* src = in + ((size_t)b * nm + p) * ldi;
  uint16_t* dst = out + ((size_t)b * N + t) * ldo;
  for (int pc = lane; pc < C / 8; pc += 64)
    *reinterpret_cast<u32x4_t*>(dst + pc * 8) = *reinterpret_cast<const u32x4_t*>(src + pc * 8);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int geometry_ok(int h, int w, int sx, int sy) {
  if (h < 2 || w < 2 || sx < 1 || sy < 1 || sx * sy > 256) return 0;
  if (h / sy < 1 || w / sx < 1) return 0;
  return (long long)h * w <= PP_TOME_MAX_TOKENS;
}

}  // namespace

extern "C" int pp_tome_supported(int h, int w, int C, int sx, int sy) {
  return (geometry_ok(h, w, sx, sy) && C >= 8 && C % 8 == 0) ? 1 : 0;
}

extern "C" int pp_tome_match(const void* x, int ldx, int batch, int h, int w, int C, int sx, int sy, const void* table,
                             int table_row_stride, int table_rows, const void* row_idx, void* best_dst, void* score, int dtype,
                             void* stream) {
  if (!x || !table || !best_dst || !score || batch <= 0 || batch > 65535 || !pp_dt_ok(dtype)) return PP_ERR_BAD_ARG;
  if (h < 1 || w < 1 || C < 1 || sx < 1 || sy < 1 || table_rows < 1) return PP_ERR_BAD_ARG;
  if (!pp_tome_supported(h, w, C, sx, sy)) return PP_ERR_UNSUPPORTED;
  const int nd = (h / sy) * (w / sx);
  if (ldx < C || ldx % 8 || !aligned16(x) || table_row_stride < nd) return PP_ERR_BAD_ARG;
  if (((uintptr_t)best_dst | (uintptr_t)score | (uintptr_t)row_idx) & 3) return PP_ERR_BAD_ARG;
  MatchArgs a;
  a.x = (const uint16_t*)x;
  a.ldx = ldx;
  a.N = h * w; a.w = w; a.C = C; a.sx = sx; a.sy = sy; a.wsx = w / sx; a.nd = nd;
  a.table = (const uint8_t*)table;
  a.row_stride = table_row_stride; a.rows = table_rows;
  a.row_idx = (const int*)row_idx;
  a.best = (int*)best_dst;
  a.score = (float*)score;
  const dim3 grid((a.N + M_SRC - 1) / M_SRC, batch);
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL((tome_match_kernel<EDT>), grid, dim3(M_T), 0, (hipStream_t)stream, a));
  PP_CHECK_LAUNCH("tome_match_kernel");
  return PP_OK;
}

extern "C" int pp_tome_select(const void* best_dst, const void* score, int batch, int n, int nd, int r, void* pos, void* rowtok,
                              void* seg, void* lst, void* stream) {
  if (!best_dst || !score || !pos || !rowtok || !seg || !lst || batch <= 0 || batch > 65535) return PP_ERR_BAD_ARG;
  if (n < 2 || nd < 1 || nd >= n || r < 0 || r > n - nd) return PP_ERR_BAD_ARG;
  if (n > PP_TOME_MAX_TOKENS) return PP_ERR_UNSUPPORTED;
  if (((uintptr_t)best_dst | (uintptr_t)score | (uintptr_t)pos | (uintptr_t)rowtok | (uintptr_t)seg | (uintptr_t)lst) & 3)
    return PP_ERR_BAD_ARG;
  int P = 2;
  while (P < n) P <<= 1;
  const int lds = P * 4 + ((n + 7) / 8 * 8) * 2;
  if (lds > 60 * 1024 && pp_func_lds(reinterpret_cast<const void*>(tome_select_kernel), lds, "hipFuncSetAttribute(tome_select)") != PP_OK)
    return PP_ERR_LAUNCH;
  hipLaunchKernelGGL(tome_select_kernel, dim3(batch), dim3(S_T), lds, (hipStream_t)stream, (const int*)best_dst,
                     (const float*)score, n, nd, r, P, (int*)pos, (int*)rowtok, (int*)seg, (int*)lst);
  PP_CHECK_LAUNCH("tome_select_kernel");
  return PP_OK;
}

extern "C" int pp_tome_merge(const void* qk, int ldqk, const void* vt, int ldvt, int batch, int n, int C, int nd, int r,
                             const void* rowtok, const void* seg, const void* lst, void* qk_out, int ldqk_out, void* vt_out,
                             int ldvt_out, int dtype, void* stream) {
  if (!qk || !vt || !rowtok || !seg || !lst || !qk_out || !vt_out || batch <= 0 || batch > 65535 || !pp_dt_ok(dtype))
    return PP_ERR_BAD_ARG;
  if (n < 2 || nd < 1 || nd >= n || r < 0 || r > n - nd || C < 8 || C % 8) return PP_ERR_BAD_ARG;
  if (n > PP_TOME_MAX_TOKENS) return PP_ERR_UNSUPPORTED;
  const int nm = n - r;
  if (ldqk < 2 * C || ldqk % 8 || ldqk_out < 2 * C || ldqk_out % 8 || ldvt < n || ldvt_out < (nm + 7) / 8 * 8 || ldvt_out % 8)
    return PP_ERR_BAD_ARG;
  if (!aligned16(qk) || !aligned16(qk_out) || ((uintptr_t)vt & 1) || ((uintptr_t)vt_out & 1)) return PP_ERR_BAD_ARG;
  if (((uintptr_t)rowtok | (uintptr_t)seg | (uintptr_t)lst) & 3) return PP_ERR_BAD_ARG;
  if (qk == qk_out || vt == vt_out) return PP_ERR_BAD_ARG;
  MergeArgs a;
  a.qk = (const uint16_t*)qk; a.vt = (const uint16_t*)vt;
  a.qk_out = (uint16_t*)qk_out; a.vt_out = (uint16_t*)vt_out;
  a.ldqk = ldqk; a.ldvt = ldvt; a.ldqk_out = ldqk_out; a.ldvt_out = ldvt_out;
  a.N = n; a.C = C; a.nd = nd; a.r = r; a.nm = nm; a.nkept = n - nd - r;
  a.qk_blocks = (nm + 3) / 4;
  a.vcols = (nm + 7) / 8 * 8;
  a.vt_mtiles = (a.vcols + 63) / 64;
  a.rowtok = (const int*)rowtok; a.seg = (const int*)seg; a.lst = (const int*)lst;
  const dim3 grid(a.qk_blocks + a.vt_mtiles * ((C + 63) / 64), batch);
  PP_DT_SWITCH(dtype, hipLaunchKernelGGL((tome_merge_kernel<EDT>), grid, dim3(256), 0, (hipStream_t)stream, a));
  PP_CHECK_LAUNCH("tome_merge_kernel");
  return PP_OK;
}

extern "C" int pp_tome_unmerge(const void* a, int lda, const void* pos, int batch, int n, int nm, int C, void* out, int ldo,
                               void* stream) {
  if (!a || !pos || !out || batch <= 0 || batch > 65535 || n < 1 || nm < 1 || nm > n || C < 8 || C % 8) return PP_ERR_BAD_ARG;
  if (lda < C || lda % 8 || ldo < C || ldo % 8 || !aligned16(a) || !aligned16(out) || ((uintptr_t)pos & 3) || a == out)
    return PP_ERR_BAD_ARG;
  const dim3 grid((n + 3) / 4, batch);
  hipLaunchKernelGGL(tome_unmerge_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)a, (long long)lda,
                     (const int*)pos, n, nm, C, (uint16_t*)out, (long long)ldo);
  PP_CHECK_LAUNCH("tome_unmerge_kernel");
  return PP_OK;
}
