"""Case tables of test_tile_walk_cpu.py (which proves from the library's geometry queries that every
case walks) and test_tile_walk_gpu.py (which runs them): small shapes on which, with the CU count
overridden through yms_cu_count_set, a block of a persistent kernel owns several tiles.

"Walks" = tiles >= 2 * grid + 1: some block owns at least three tiles (the first, one in the middle of
the prefetch ring / double buffer, and the last).  Where the library reports the grid (statistics rows,
BN-reduce rows, weight-gradient workspace bytes) the CPU file asserts it; where it does not, the
geometry is derived here in a comment from the host selector, for the override values used.

Not covered, on purpose: the implicit-GEMM input gradient (stride 1 and the stride-2 parity classes)
launches one block per tile (NT_DGRAD_MULT in conv_igemm.hip), so the CU count does not reach it."""
import ctypes

import pytest

from hiputil import DT, shape
from yms import _lib as L

OVERRIDES = (1, 3)              # conv forward / direct kernels
DW_OVERRIDES = (1, 2, 3)        # depthwise (2: the multi-strip derivations below)
WG_OVERRIDES = (1, 2048)        # split-K weight gradients: one split / as many as the work allows
LOWP = ("bf16", "f16")


@pytest.fixture
def cu_count():
    """yms_cu_count_set(n) for the test, the process' setting restored after it."""
    prev = L.lib().yms_cu_count_set(-1)
    yield lambda n: L.lib().yms_cu_count_set(int(n))
    L.lib().yms_cu_count_set(prev)


def cdiv(a, b):
    return -(-a // b)


def case_id(c):
    return "x".join(str(v) for v in c)


# ---- persistent implicit-GEMM forward (conv_ntp_kernel) ----------------------------------------------
# (n, cin, h, w, cout, k, stride, BM, BN, OCC): the tile config is choose_tile(cout) / ntp_geo of
# conv_igemm.hip -- cout <= 32: 256 x 32 at 2 blocks per CU; <= 64: 128 x 64 at 3; <= 128: 128 x 128 at 2;
# 130: 128 x 64 (three column tiles: 128-column tiles would pad by more than 25 %).
# grid = min(tiles, mult * OCC * CUs), mult = 1 with statistics (rounded down to a multiple of the column
# tiles), 4 in eval.  Statistics grids under overrides 1 / 3: 2 / 6, 3 / 9, 2 / 6 blocks; eval grids under
# override 1: 8 / 12 / 8 blocks, so an eval case walks with >= 17 / 25 / 17 tiles (under override 3 the eval
# grids are 24 / 36 / 24: these shapes then own one or two tiles per block, the default regime again).
# None of them takes the direct 3x3 route (that needs 32 / 64 reduction channels and a width % 16 == 0).
#   M = n * ho * wo rows; tiles = ceil(M / BM) * ceil(cout / BN)
NTP = [
    (2, 64, 33, 37, 80, 1, 1, 128, 128, 2),    # 1x1, one k-tile deep; M 2442: 20 tiles, last one 10 rows
    (2, 128, 33, 35, 128, 3, 1, 128, 128, 2),  # 3x3 stride 1, 128 reduction channels; M 2310: 19 tiles
    (1, 40, 47, 49, 80, 3, 1, 128, 128, 2),    # 3x3, cin 40 (non-uniform taps); M 2303: 18 tiles
    (2, 64, 81, 79, 128, 3, 2, 128, 128, 2),   # 3x3 stride 2; M 2 * 41 * 40 = 3280: 26 tiles
    (2, 32, 41, 43, 64, 1, 1, 128, 64, 3),     # 1x1, cin 32 (half a k-tile); M 3526: 28 tiles
    (1, 128, 33, 35, 130, 3, 1, 128, 64, 3),   # cout 130: 3 column tiles (the last 2 wide) x 10 row tiles
    (2, 40, 85, 83, 64, 3, 2, 128, 64, 3),     # 3x3 stride 2, cin 40; M 2 * 43 * 42 = 3612: 29 tiles
    (2, 16, 47, 45, 24, 1, 1, 256, 32, 2),     # cout 24, 1x1 cin 16; M 4230: 17 tiles of 256 rows
    (1, 128, 65, 67, 32, 3, 1, 256, 32, 2),    # cout 32, 3x3; M 4355: 18 tiles
]


def ntp_shape(case, dt):
    n, cin, h, w, cout, k, s = case[:7]
    return shape(n, h, w, cin, cout, k, s, DT[dt])


def ntp_tiles(case, dt="bf16"):
    """-> (tiles, column tiles) of the case"""
    sh = ntp_shape(case, dt)
    bm, bn = case[7], case[8]
    tn = cdiv(sh.cout, bn)
    return cdiv(sh.n * sh.ho * sh.wo, bm) * tn, tn


def ntp_stats_grid(case, dt):
    """the statistics launch's grid from yms_conv_stats_rows (= grid / column tiles * BM / 128)"""
    sh = ntp_shape(case, dt)
    rows = L.lib().yms_conv_stats_rows(ctypes.pointer(sh))
    return rows // (case[7] // 128) * ntp_tiles(case, dt)[1]


def ntp_eval_grid(case, cus):
    """no query: min(tiles, 4 * OCC * CUs) (nt_fwd_mult(false) = 4, launch_ntp)"""
    return min(ntp_tiles(case)[0], 4 * case[9] * cus)


# grouped forward (yms_conv_fwd_group): B = 3 members of one kernel variant on maps of 40 / 24 / 8 ->
# M = 4800 / 1728 / 192 rows = 38 / 14 / 2 tiles of 128 rows; with statistics under override 1 the members'
# sub-grids are 2 (cout 80) or 3 (cout 64) blocks, so the first two members walk and the third does not
GROUP_MAPS = (40, 24, 8)
GROUP_CONVS = [(128, 80, 3), (64, 64, 1)]        # (cin, cout, k): the 128 x 128 and the 128 x 64 variant


# ---- direct 3x3 (conv_direct.hip) ----------------------------------------------------------------------
# (n, cin, h, w, cout) of the forward; the stride-1 input gradient reads the same tuple as
# (n, reduction = conv cout, h, w, outputs = conv cin), as test_conv_direct_gpu.py does.
# Tiles: TW = 32 for w % 32 == 0 else 16, TH = 256 / TW rows; tiles = n * (w / TW) * ceil(h / TH).
# grid = min(tiles, OCC * CUs) with OCC <= 2 (DirGeo::OCC), so <= 6 blocks under override 3: 13 tiles walk.
DIRECT = [
    (3, 32, 37, 32, 32),     # TW 32, 32 reduction channels, one fragment; 3 * 5 = 15 tiles, last row tile 5 rows
    (2, 64, 53, 32, 64),     # TW 32, 64 channels, two fragments; 2 * 7 = 14 tiles
    (5, 64, 40, 16, 64),     # TW 16, 64 channels, two fragments; 5 * 3 = 15 tiles, last row tile 8 rows
    (2, 30, 27, 64, 40),     # cin padded to 32, cout 40 (second fragment partly valid); 2 * 2 * 4 = 16 tiles
    (1, 64, 100, 48, 8),     # TW 16, 8 output channels; 3 * 7 = 21 tiles
    (5, 32, 37, 16, 24),     # TW 16, 32 channels, 24 outputs; 5 * 3 = 15 tiles
]


def direct_tiles(n, h, w):
    tw = 32 if w % 32 == 0 else 16
    assert w % tw == 0
    return n * (w // tw) * cdiv(h, 256 // tw)


def direct_fwd_grid(n, cin, h, w, cout, dt):
    """the direct forward's grid = its statistics rows (one per block)"""
    return L.lib().yms_conv_stats_rows(ctypes.pointer(shape(n, h, w, cin, cout, 3, 1, DT[dt])))


def direct_dgrad_grid(case, dt):
    """stride-1 input gradient of the conv (cin = case[4]) -> (cout = case[1]): conv_direct_geometry sizes
    it as the forward of the channel-swapped conv (same TW, reduction width, fragments, DirGeo::OCC), so the
    forward query of the swapped shape is its grid"""
    n, cred, h, w, cout_dx = case
    return direct_fwd_grid(n, cred, h, w, cout_dx, dt)


# stride-2 input gradient by parity class: (n, cin = dx channels, h, w, cout = reduction); the tile grid is
# over the class positions, ho x wo = ceil(h / 2) x ceil(w / 2), TW from wo; the direct kernel does not
# take 32 reduction channels with 33..64 outputs.  No query for the plain launch: grid = min(tiles,
# DirGeo2::OCC * CUs), OCC <= 2, so <= 2 / 6 blocks under overrides 1 / 3 (the BN-reduce launch: OCC 1).
DIRECT_S2 = [
    (2, 32, 100, 64, 64),    # wo 32: TW 32; 2 * ceil(50 / 8) = 14 tiles
    (5, 16, 75, 31, 32),     # odd map, wo 16: TW 16; 5 * ceil(38 / 16) = 15 tiles; 32 reduction channels
    (2, 64, 105, 64, 64),    # two fragments; 2 * ceil(53 / 8) = 14 tiles
    (2, 24, 109, 63, 64),    # odd map, 24 dx channels; 2 * ceil(55 / 8) = 14 tiles
]


def direct_s2_tiles(n, h, w):
    return direct_tiles(n, (h + 1) // 2, (w + 1) // 2)


# yms_conv_dgrad_bnred, in the tuple of test_dgrad_bnred_gpu.py: (n, cin = dx channels, h, w, cout =
# reduction, stride, accumulate).  One fragment only (dx channels <= 32), one block per CU.
BNRED = [
    (2, 32, 53, 32, 32, 1, 0),     # 2 * 7 = 14 tiles: 5 5 4 under override 3
    (1, 8, 100, 48, 64, 1, 1),
    (5, 24, 37, 16, 32, 1, 1),
    (2, 32, 100, 64, 64, 2, 0),
    (5, 16, 75, 31, 32, 2, 1),
    (2, 24, 109, 63, 64, 2, 1),
]


def bnred_tiles(case):
    n, cin, h, w, cout, s, acc = case
    return direct_s2_tiles(n, h, w) if s == 2 else direct_tiles(n, h, w)


def bnred_grid(case, dt):
    n, cin, h, w, cout, s, acc = case
    return L.lib().yms_conv_dgrad_bnred_rows(ctypes.pointer(shape(n, h, w, cin, cout, 3, s, DT[dt])))


# ---- depthwise (dwconv.hip), (n, h, w, c, k), through run_all_passes of test_dwconv_edges_gpu.py -----------
# Derived from the host selectors for 1 / 2 / 3 CUs.
# Strip walker (dw_strip_grid; forward and dgrad): w 41 -> TX 32 / TY 8: 2 column tiles (the last 9 wide) x 7 row
#   tiles per image, base = n * 2 * channel groups blocks per strip row, slots = occupancy * CUs, cost(tps) =
#   rounds * (8 tps + k - 1), the longest strip among equal costs.  tps (strips of a tile column):
#     (1, 53, 41, 24, 3) 16-bit (occ 4)  4 (4 + 3) | 2 (2 2 2 1) | 2          fp32 (occ 2)  7 | 4 (4 + 3) | 3 (3 3 1)
#     (1, 53, 41, 24, 5) 16-bit (occ 3)  3 (3 3 1) | 3           | 2 (2 2 2 1) fp32 (occ 1)  7 | 7         | 3 (3 3 1)
#     (1, 53, 41, 24, 9) 16-bit (occ 2)  7         | 4 (4 + 3)   | 3 (3 3 1)   fp32 (occ 1)  7 | 7         | 7
#     (1, 53, 41, 24, 7) fp32   (occ 1)  7         | 7           | 3 (3 3 1)   (16-bit: the MFMA kernel, below)
#     (1, 53, 64, 64, 3) 16-bit, 64-channel blocks (2 slots per CU): 7 | 4 (4 + 3) | 3 (3 3 1)
#     (1, 45, 40, 56, 3) 16-bit, 56-channel blocks, TX 40 / TY 6: 1 x 8 tiles: 4 (4 4) | 2 | 2
#   so every one of them walks >= 2 tiles per strip under every override, and override 2 (16-bit k 3: 2 2 2 1,
#   k 9 and fp32 k 3: 4 + 3) is the multi-strip case with a shorter last strip that needs no 256-CU device.
# k = 3 strip weight gradient (dw_wg3_grid: 32-channel blocks, 2 slots per CU, cost rounds * (8 tps + 2 + 24)):
#     (1, 53, 41, 24, 3): tps 7 | 4 (4 + 3) | 3 (3 3 1) -> 2 | 4 | 6 workspace rows (n * 2 column tiles * strips)
#     (1, 45, 40, 56, 3): tps 8 | 4 | 3 (3 3 2)         -> 1 | 2 | 3 rows (one column tile; two 32-channel groups share them)
#     (1, 53, 64, 64, 3): tps 7 under each              -> 2 rows
# k = 7 MFMA forward / dgrad (dw_fm_grid: units = n * ceil(h / 16), upb = ceil(units * (c / 8) / (4 CUs))):
#     (3, 40, 24, 16, 7): 9 units, 2 channel groups: upb 5 (5 + 4) | 3 | 2 (2 2 2 2 1)
#     (1, 53, 41, 24, 7): 4 units, 3 channel groups: upb 3 (3 + 1) | 2 | 1
# MFMA weight gradient (dw_wgm_cfg: 16 channels per block, one slot per CU; upb = the fewest units per block
#   that keep the grid within one round): workspace rows = unit groups
#     (3, 40, 24, 16, 7) one column chunk, 9 units:  upb 9 | 5 (5 + 4) | 3 -> 1 | 2 | 3 rows
#     (3, 40, 41, 16, 9) two column chunks, 9 units: upb 9 | 5 (5 + 4) | 3 -> 1 | 2 | 3 rows
#     (3, 24, 24, 16, 5) both 16-row blocks per unit (NB 2), 3 units: upb 3 | 2 (2 + 1) | 1 -> 1 | 2 | 3 rows
#     (1, 53, 41, 24, 5 / 9) two chunks, 4 units, two channel groups: one group of 4 under each -> 1 row
# dwconv_wgrad2_kernel (dw_wg2_blocks = min(tiles, 2 CUs / channel groups); TX 32, TY 9 / 7 / 12 for k 7 / 9 / 5):
#     (1, 40, 65, 24, 7): 3 x 5 = 15 tiles; (1, 40, 65, 24, 9): 3 x 6 = 18; (1, 40, 97, 24, 5): 4 x 4 = 16;
#     2 | 4 | 6 blocks = workspace rows, so 7.5 / 9 / 8 tiles per block under override 1 and >= 2.5 under 3
# fp32 weight gradients run the tile kernel, whose grid does not depend on the CU count.
DW_ALL_DT = [(1, 53, 41, 24, 3), (1, 53, 41, 24, 5), (1, 53, 41, 24, 9), (1, 53, 41, 24, 7)]
DW_LOWP = [(1, 53, 64, 64, 3), (1, 45, 40, 56, 3), (3, 40, 24, 16, 7), (3, 40, 41, 16, 9), (3, 24, 24, 16, 5),
           (1, 40, 65, 24, 7), (1, 40, 65, 24, 9), (1, 40, 97, 24, 5)]
DW_CASES = [(dt, s) for s in DW_ALL_DT for dt in ("f32",) + LOWP] + [(dt, s) for s in DW_LOWP for dt in LOWP]
# 16-bit weight-gradient workspace rows (yms_dwconv_wgrad_ws_bytes / (k * k * c * 4)) under 1 | 2 | 3 CUs, from the
# derivations above; units = what the rows split: strips' tiles, MFMA units, wgrad2 tiles
DW_WS_ROWS = {
    (1, 53, 41, 24, 3): (2, 4, 6), (1, 45, 40, 56, 3): (1, 2, 3), (1, 53, 64, 64, 3): (2, 2, 2),
    (3, 40, 24, 16, 7): (1, 2, 3), (3, 40, 41, 16, 9): (1, 2, 3), (3, 24, 24, 16, 5): (1, 2, 3),
    (1, 53, 41, 24, 5): (1, 1, 1), (1, 53, 41, 24, 9): (1, 1, 1), (1, 53, 41, 24, 7): (1, 1, 1),
    (1, 40, 65, 24, 7): (2, 4, 6), (1, 40, 65, 24, 9): (2, 4, 6), (1, 40, 97, 24, 5): (2, 4, 6),
}
DW_WS_UNITS = {
    (1, 53, 41, 24, 3): 14, (1, 45, 40, 56, 3): 8, (1, 53, 64, 64, 3): 14,
    (3, 40, 24, 16, 7): 9, (3, 40, 41, 16, 9): 9, (3, 24, 24, 16, 5): 3,
    (1, 53, 41, 24, 5): 4, (1, 53, 41, 24, 9): 4, (1, 53, 41, 24, 7): 4,
    (1, 40, 65, 24, 7): 15, (1, 40, 65, 24, 9): 18, (1, 40, 97, 24, 5): 16,
}


def dw_ws_rows(shp, dt):
    n, h, w, c, k = shp
    sp = ctypes.pointer(L.DwShape(n, h, w, c, k, L.dtype_code(DT[dt])))
    wsb = L.lib().yms_dwconv_wgrad_ws_bytes(sp)
    assert wsb % (k * k * c * 4) == 0
    return wsb // (k * k * c * 4)


# ---- split-K weight gradients (route and TT kernel in wgrad.hip, wgrad_ring.hip, wgrad_halo.hip) ---------
# (n, cin, h, w, cout, k, stride); the route is forced with YMS_WG_RING / YMS_WG_HALO as test_conv_gpu.py does.
# wgrad_splits = min(work / minimum per split, ceil(4 CUs / tiles) (halo: ceil(2 CUs / tiles)), slab cap).  Every
# case has >= 4 (halo: >= 2) tiles of its weight-gradient GEMM, so override 1 gives one split: one block per tile
# walks every pixel.  Under 2048 the work bound decides: ceil(M / 32 / 16) (TT), ceil(M / 64 / 8) (ring), the
# patches (halo), or the slab cap where that is lower.  The workspace is splits slabs (wg_slab_bytes).
WG_ENV = {"tt": {"YMS_WG_RING": "0", "YMS_WG_HALO": "0"}, "ring": {"YMS_WG_RING": "2", "YMS_WG_HALO": "0"},
          "halo": {"YMS_WG_HALO": "2"}}
WG_GEMM = [(2, 64, 40, 40, 128, 3, 1), (2, 200, 37, 39, 130, 1, 1), (2, 64, 40, 40, 64, 3, 1),
           (2, 72, 81, 83, 96, 3, 2), (3, 40, 29, 27, 130, 3, 1)]
WG_HALO = [(2, 64, 40, 40, 128, 3, 1), (3, 40, 13, 27, 48, 3, 1), (2, 40, 33, 41, 64, 3, 2),
           (3, 64, 21, 32, 128, 3, 1), (2, 64, 40, 40, 32, 3, 1)]
WG_CASES = [(r, s) for r in ("tt", "ring") for s in WG_GEMM] + [("halo", s) for s in WG_HALO]


def wg_ws_bytes(shp, dt):
    n, cin, h, w, cout, k, s = shp
    return L.lib().yms_conv_wgrad_ws_bytes(ctypes.pointer(shape(n, h, w, cin, cout, k, s, DT[dt])))


def wg_slab_bytes(route, shp):
    """one split's fp32 slab(s), WgradRoute's slabs_per_split x slab_rows x slab_ld of wgrad.hip: the weight
    gradient rounded up to the route's tiles (wgrad_plan there, wgrad_ring_plan, wgrad_halo_plan: 32- or
    64-output-channel blocks, the 32-channel one with a slab per k-half)"""
    n, cin, h, w, cout, k, s = shp
    cin8 = cdiv(cin, 8) * 8
    kf = k * k * cin8
    if route == "halo":
        mb = 1 if cout <= 32 else 2
        return (2 if mb == 1 else 1) * cdiv(cout, 32 * mb) * 32 * mb * kf * 4
    if route == "ring":
        bm = 64 if cout <= 64 else 128
    else:
        bm = 32 if cout <= 32 else 64 if cout <= 64 else 96 if cout <= 96 else 128
    bn = 64 if kf <= 64 else 128
    return cdiv(cout, bm) * bm * cdiv(kf, bn) * bn * 4


# ---- through the plans -------------------------------------------------------------------------------------
# Eval forward + decode of YOLOv8-n and YOLO-MS-xs at 2 x 3 x 64 x 64, override 1: the eval grids are 8 / 12 / 8
# blocks; the 32^2 and 16^2 maps hold M = 2048 / 512 rows = 16 / 4 tiles of 128, 8 / 2 of 256: two tiles per block
# on the stem-side layers, one below.  The C2f block of test_c2f_lowp_train_grads (4 x 64 x 20 x 20, M = 1600):
# statistics grids 3 (64 outputs: 13 tiles) and 2 (32 outputs, w = 20 is off the direct kernel's tile grid: 7 tiles
# of 256 rows), weight gradients in one split.
PLAN_MODELS = ("n", "ms-xs")
