"""CPU: the tile order of the GEMM-class kernels (powerpaint_amd/csrc/tile_order.h) -- the decode of a tile id, the fabric-read
model and the chooser -- in a stand-alone host program compiled from that header alone (it includes no HIP header and asks no
device), and the orders the loaded library resolves for the SD-1.5 launches (pp_gemm_tile_group_m: pure host logic).

The shape classes are the launches of the headline step at batch 8: operand bytes as the library
computes them -- a halo tile's panel is (rows + 2 W) pixels x input channels, a strip is 160 rows x K -- 32 CUs per XCD, a
4 MiB L2, one workgroup per CU for the 160 KiB tiles and two for the 64- and 128-row GEMM tiles.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "powerpaint_amd", "csrc")

#          name           tiles_m tiles_n splits panel_bytes            strip_bytes        row_bytes resident
CLASSES = [("conv16_k11520", 8, 8, 4, (256 + 32) * 1280 * 2, 160 * 11520 * 2, 2 * 11520, 32),
           ("conv16_k23040", 8, 8, 4, (256 + 32) * 2560 * 2, 160 * 23040 * 2, 2 * 23040, 32),
           ("conv32_k11520", 32, 4, 2, (256 + 64) * 1280 * 2, 160 * 11520 * 2, 2 * 11520, 32),
           ("conv32_k5760", 64, 4, 1, (128 + 64) * 640 * 2, 160 * 5760 * 2, 2 * 5760, 32),
           ("conv64_k2880", 128, 2, 1, (256 + 128) * 320 * 2, 160 * 2880 * 2, 2 * 2880, 32),
           ("conv64_k8640", 128, 2, 1, (256 + 128) * 960 * 2, 160 * 8640 * 2, 2 * 8640, 32),
           ("geglu32", 64, 32, 1, 128 * 640 * 2, 160 * 640 * 2, 2 * 640, 64),
           ("qkv16", 32, 24, 1, 64 * 1280 * 2, 160 * 1280 * 2, 2 * 1280, 64),
           ("ff2_16", 16, 8, 2, 128 * 6400 * 2, 160 * 6400 * 2, 2 * 6400, 32)]

MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "tile_order.h"
int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "decode")) {
    long checked = 0;
    for (int tm = 1; tm <= 24; ++tm)
      for (int tn = 1; tn <= 24; ++tn)
        for (int g = 1; g <= tm; ++g) {
          std::vector<int> hit(tm * tn, 0);
          for (int id = 0; id < tm * tn; ++id) {
            int m = -1, n = -1;
            pp_tile_decode(id, tm, tn, g, &m, &n);
            if (m < 0 || m >= tm || n < 0 || n >= tn) { printf("BAD range %d %d %d id %d -> %d %d\n", tm, tn, g, id, m, n); return 1; }
            if (hit[m * tn + n]++) { printf("BAD twice %d %d %d id %d -> %d %d\n", tm, tn, g, id, m, n); return 1; }
            // the order itself: groups of g panels, tile_m fastest inside a group, then tile_n
            const int grp = m / g, h = (tm - grp * g < g) ? tm - grp * g : g;
            if (id != grp * g * tn + n * h + (m - grp * g)) { printf("BAD order %d %d %d id %d -> %d %d\n", tm, tn, g, id, m, n); return 1; }
            ++checked;
          }
          // the two orders the kernels had are special cases
          for (int id = 0; id < tm * tn; ++id) {
            int m, n;
            pp_tile_decode(id, tm, tn, 1, &m, &n);
            if (m != id / tn || n != id % tn) { printf("BAD m-major %d %d\n", tm, tn); return 1; }
            pp_tile_decode(id, tm, tn, tm, &m, &n);
            if (n != id / tm || m != id % tm) { printf("BAD n-major %d %d\n", tm, tn); return 1; }
          }
        }
    // the XCD ranges partition the ids, for grids that are no multiple of 8 as well
    for (int nwg = 1; nwg <= 600; ++nwg) {
      int next = 0;
      for (int x = 0; x < PP_XCDS; ++x) {
        int f, c;
        pp_xcd_range(nwg, x, &f, &c);
        if (f != next || c < 0) { printf("BAD xcd range %d %d\n", nwg, x); return 1; }
        next = f + c;
      }
      if (next != nwg) { printf("BAD xcd cover %d\n", nwg); return 1; }
    }
    printf("OK %ld\n", checked);
    return 0;
  }
  PPTileOrderIn in;
  long long pb, sb, rb;
  if (argc != 9 || sscanf(argv[2], "%d", &in.tiles_m) != 1 || sscanf(argv[3], "%d", &in.tiles_n) != 1 ||
      sscanf(argv[4], "%d", &in.splits) != 1 || sscanf(argv[5], "%lld", &pb) != 1 || sscanf(argv[6], "%lld", &sb) != 1 ||
      sscanf(argv[7], "%lld", &rb) != 1 || sscanf(argv[8], "%d", &in.resident_per_xcd) != 1) return 2;
  in.panel_bytes = pb; in.strip_bytes = sb; in.row_bytes = rb; in.l2_bytes = 4ll << 20;
  const int legacy = pp_tile_order_legacy(in.tiles_m, in.tiles_n), chosen = pp_tile_order_choose(in);
  printf("%d %d %.0f %.0f %.0f %.3f\n", legacy, chosen, pp_tile_order_bytes(in, legacy), pp_tile_order_bytes(in, chosen),
         pp_tile_order_bytes(in, in.tiles_m), PP_TILE_ORDER_MIN_SAVING);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the chooser's source must compile without HIP")
    d = tmp_path_factory.mktemp("tile_order")
    src, exe = str(d / "main.cpp"), str(d / "tile_order")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


def test_the_decode_is_a_bijection_in_the_stated_order(host_program):
    """tiles_m, tiles_n in 1..24, every group height 1..tiles_m (heights that do not divide tiles_m and grids that are no
    multiple of 8 included): every tile exactly once, in the grouped order; group_m = 1 / tiles_m are the M- / N-major orders"""
    out = subprocess.check_output([host_program, "decode"]).decode()
    assert out.startswith("OK "), out
    assert int(out.split()[1]) == sum(tm * tn * tm for tm in range(1, 25) for tn in range(1, 25))


def _model(host_program, cls):
    name, *nums = cls
    legacy, chosen, b_legacy, b_chosen, b_nmajor, thr = subprocess.check_output([host_program, "choose"] + [str(n) for n in nums]).split()
    return int(legacy), int(chosen), float(b_legacy), float(b_chosen), float(b_nmajor), float(thr)


@pytest.mark.parametrize("cls", CLASSES, ids=[c[0] for c in CLASSES])
def test_the_chooser_never_models_more_bytes_than_the_legacy_order(host_program, cls):
    legacy, chosen, b_legacy, b_chosen, _, thr = _model(host_program, cls)
    print(f"[tile order] {cls[0]}: legacy group_m {legacy} {b_legacy / 1e6:.1f} MB -> group_m {chosen} {b_chosen / 1e6:.1f} MB (modelled)")
    assert 1 <= chosen <= cls[1]
    assert b_chosen <= b_legacy
    if chosen != legacy:                               # a changed order clears the threshold recorded next to the chooser
        assert b_chosen <= b_legacy * (1.0 - thr)


def test_the_16x16_convs_share_weights_and_the_64x64_convs_keep_their_order(host_program):
    for cls in CLASSES[:2]:                            # 8 x 8 tiles, 4 splits: every XCD ran one image against all eight strips
        legacy, chosen, b_legacy, b_chosen, _, _ = _model(host_program, cls)
        assert legacy == 1 and chosen > 1, cls[0]      # several panels of a window share each weight strip
        assert b_chosen < 0.5 * b_legacy, cls[0]
    for cls in CLASSES[4:6]:
        legacy, chosen, _, _, _, _ = _model(host_program, cls)
        assert legacy == 1 and chosen == 1, cls[0]


def _conv(B, H, cin, cout, c2=0):
    from powerpaint_amd import _lib as L
    return L.conv3x3_args(L.PP_DT_BF16, B, H, H, cin, cout, 0x1000, 0x2000 if c2 else None, c2, w=0x5000, out=0x6000)


def test_the_library_resolves_those_orders_for_the_step_launches():
    """pp_gemm_tile_group_m on the requests of the headline step (batch 8): what Plan.describe() prints"""
    from powerpaint_amd import _lib as L
    lib = L.lib()
    q = lambda a: lib.pp_gemm_tile_group_m(C.byref(a))      # noqa: E731
    assert q(_conv(8, 16, 1280, 1280)) > 1 and q(_conv(8, 16, 1280, 1280, c2=1280)) > 1       # 16x16, K = 11520 / 23040
    assert q(_conv(8, 64, 320, 320)) == 1 and q(_conv(8, 64, 640, 320, c2=320)) == 1          # 64x64: the order they had
    a = _conv(8, 8, 1280, 1280)                                                                # 8x8: N-major as before
    assert q(a) == 4
    # plain GEMMs keep the order they had (slower or no gain on the grouped order: profiles/tile_order_step_ab.txt)
    for M, N, K, want in ((8192, 5120, 640, 1), (2048, 3840, 1280, 1), (512, 3840, 1280, 8)):      # (the last: 8 x 24 tiles of 64 rows, N-major as before)
        assert q(L.gemm_args(L.PP_DT_BF16, M, N, K, 0x1000, 0x2000, 0x3000)) == want, (M, N, K)
    # forced heights: clamped to the M tiles of the form; 0 = automatic; negative = refused (the request does not run)
    a = _conv(8, 16, 1280, 1280)
    for want, got in ((1, 1), (2, 2), (3, 3), (8, 8), (1000, 8)):
        a.tile_group_m = want
        assert q(a) == got
    a.tile_group_m = -1
    assert q(a) == 0 and lib.pp_gemm_bf16(C.byref(a), None) == -1
    assert q(L.PPGemmArgs()) == 0
