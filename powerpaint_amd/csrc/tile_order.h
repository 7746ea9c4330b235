// Tile order of the GEMM-class kernels (pp_gemm_kernel, pp_gemm_kernel_v2, pp_conv_gn_kernel): the decode of a linear tile
// id, the fabric-read model of an order and the host-side chooser.  Plain C++: no HIP header, no device query -- a host-only
// program compiles this file as it stands (tests/test_tile_order.py does), and the kernels include it for the decode.
//
// The kernels remap blockIdx.x so that each of the 8 XCDs (private 4 MiB L2 each) owns a contiguous range of tile ids, and
// the workgroups resident on an XCD at one time hold consecutive ids of that range.  What those ids share decides what the
// XCD's L2 serves twice: tiles of one M panel share the activation rows, tiles of one N strip share the weight rows.
//
// GROUPED ORDER: ids walk groups of `group_m` M panels; inside a group tile_m runs fastest, then tile_n; the last group
// may be shorter.  group_m = 1 is the M-major order (ids walk the N tiles of one panel), group_m = tiles_m the N-major order
// (ids walk the M tiles of one strip); between them a window of R resident workgroups holds group_m panels and about
// R / group_m strips.
#pragma once

#if defined(__HIPCC__)
#define PP_TO_FN __host__ __device__ __forceinline__
#else
#define PP_TO_FN inline
#endif

constexpr int PP_XCDS = 8;   // the XCD remap of the kernels is written for eight

// tile id -> (tile_m, tile_n): a bijection of [0, tiles_m * tiles_n) onto the grid for every 1 <= group_m <= tiles_m
PP_TO_FN void pp_tile_decode(int id, int tiles_m, int tiles_n, int group_m, int* tile_m, int* tile_n) {
  const int per_group = group_m * tiles_n;
  const int g = id / per_group;
  const int first = g * group_m;
  int h = tiles_m - first;                    // height of this group: the last one may be ragged
  if (h > group_m) h = group_m;
  const int r = id - g * per_group;
  const int tn = r / h;
  *tile_m = first + (r - tn * h);
  *tile_n = tn;
}

// first tile id and id count of XCD `xcd` under the kernels' remap of blockIdx.x (nwg = tiles of the launch)
inline void pp_xcd_range(int nwg, int xcd, int* first, int* count) {
  const int q = nwg / PP_XCDS, r = nwg % PP_XCDS;
  *first = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  *count = q + (xcd < r ? 1 : 0);
}

struct PPTileOrderIn {
  int tiles_m, tiles_n;
  int splits;              // K splits (blockIdx.y): every split walks the same tile order over its own K share
  long long panel_bytes;   // one activation panel over the whole K: the halo rows of a halo tile included; source rows,
                           // not the im2col expansion, for the tap-major conv
  long long strip_bytes;   // one weight strip over the whole K
  long long row_bytes;     // one operand row over the whole K (2 K bytes): panel_bytes / row_bytes = rows of a panel
  int resident_per_xcd;    // workgroups of this tile form resident on one XCD at a time
  long long l2_bytes;      // one XCD's L2
};

// MODELLED bytes the XCDs read through the fabric for one launch in the order `group_m`: every XCD walks its id range in
// windows of the workgroups resident at one time and reads each DISTINCT panel and strip of a window once; nothing is
// retained from one window to the next.  The splits of a launch are dispatched split after split (blockIdx.x runs fastest),
// each reads 1 / splits of every operand, so the sum over the splits is the one-split walk over whole operands -- except
// that a window never holds more tiles than the XCD owns.  Sharing inside a window is credited only while the slices the
// window streams together (four 64-deep K steps of every distinct operand row, the depth of the pipelines, in every
// split) fit the L2; beyond that every workgroup is charged its own operands.
inline double pp_tile_order_bytes(const PPTileOrderIn& in, int group_m) {
  const int tiles = in.tiles_m * in.tiles_n;
  if (tiles <= 0 || group_m < 1) return 0.0;
  if (group_m > in.tiles_m) group_m = in.tiles_m;
  constexpr int MAXT = 64;                    // distinct-operand marks of one window: two workgroups on each of 32 CUs
  const int window = in.resident_per_xcd < 1 ? 1 : in.resident_per_xcd > MAXT ? MAXT : in.resident_per_xcd;
  double total = 0.0;
  for (int x = 0; x < PP_XCDS; ++x) {
    int first, count;
    pp_xcd_range(tiles, x, &first, &count);
    for (int w0 = 0; w0 < count; w0 += window) {
      const int w1 = w0 + window < count ? w0 + window : count;
      int pm[MAXT], pn[MAXT], npm = 0, npn = 0;
      for (int i = w0; i < w1; ++i) {
        int tm, tn;
        pp_tile_decode(first + i, in.tiles_m, in.tiles_n, group_m, &tm, &tn);
        bool seen = false;
        for (int k = 0; k < npm; ++k) seen |= pm[k] == tm;
        if (!seen && npm < MAXT) pm[npm++] = tm;
        seen = false;
        for (int k = 0; k < npn; ++k) seen |= pn[k] == tn;
        if (!seen && npn < MAXT) pn[npn++] = tn;
      }
      const double shared = (double)npm * (double)in.panel_bytes + (double)npn * (double)in.strip_bytes;
      // the slices in flight together: 4 K steps of 128 bytes per distinct operand row, in every split
      const double rows = shared / (double)(in.row_bytes > 0 ? in.row_bytes : 1);
      const double together = rows * 512.0 * (double)(in.splits > 0 ? in.splits : 1);
      const bool unshared = together > (double)in.l2_bytes;
      total += unshared ? (double)(w1 - w0) * (double)(in.panel_bytes + in.strip_bytes) : shared;
    }
  }
  return total;
}

// A launch whose modelled saving is below this fraction of the legacy order's bytes keeps that order.  Source: the halo-tile
// convs of the headline step, the class the library asks the chooser for (gemm.hip: form_group_m).  The smallest modelled
// saving among them is 18 % (32x32 level, K = 5760) and none of the re-ordered launches is slower beyond the +-2 % spread of
// the unchanged ones of their size in the per-launch listing (profiles/tile_order_launches.txt); with the bar at 30 % instead, the 32x32
// level back on the legacy order, the step gains 0.12 % against 0.20 % on the same box (profiles/tile_order_step_ab.txt).
// Below 10 % the model's own simplifications (no retention between windows, whole operands) are larger than the saving.
constexpr double PP_TILE_ORDER_MIN_SAVING = 0.10;

// today's orders, before the grouped one: N-major for the short grids whose weights are the big operand, else M-major
inline int pp_tile_order_legacy(int tiles_m, int tiles_n) { return (tiles_m < tiles_n && tiles_m <= 8) ? tiles_m : 1; }

// The order of a launch: the group height with the fewest modelled bytes among {1, 2, 4, ..., tiles_m}; the legacy order on a
// tie or where the saving against it is below PP_TILE_ORDER_MIN_SAVING.  Pure: touches nothing but its argument.
inline int pp_tile_order_choose(const PPTileOrderIn& in, double min_saving = PP_TILE_ORDER_MIN_SAVING) {
  const int legacy = pp_tile_order_legacy(in.tiles_m, in.tiles_n);
  if (in.tiles_m <= 1 || in.tiles_n <= 1) return legacy;
  const double base = pp_tile_order_bytes(in, legacy);
  int best = legacy;
  double best_bytes = base;
  for (int g = 1;; g *= 2) {
    if (g > in.tiles_m) g = in.tiles_m;
    const double b = pp_tile_order_bytes(in, g);
    if (b < best_bytes) {
      best_bytes = b;
      best = g;
    }
    if (g == in.tiles_m) break;
  }
  if (best_bytes > base * (1.0 - min_saving)) return legacy;
  return best;
}
