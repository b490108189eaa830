"""The CU-count seam (yms_cu_count_set) and, from the library's geometry queries alone, the proof that
every queried case of test_tile_walk_gpu.py walks under its overrides: tiles >= 2 * grid + 1, so some
block owns at least three tiles, and for each kernel at least one case where tiles % grid != 0, so the
blocks own unequal counts.  A case that does not walk is a broken case: nothing here skips.

Runs without a GPU: the queries are host arithmetic, and with no device the library's own CU count falls
back to 256.  The geometry that has no query (the eval forward's grid, the depthwise strip length and units
per block, the stride-2 direct input gradient) is derived in tile_walk_cases.py."""
import pytest

import tile_walk_cases as T
from tile_walk_cases import cu_count  # noqa: F401  (fixture)
from yms import _lib as L


def walks(tiles, grid):
    return grid >= 1 and tiles >= 2 * grid + 1


# ---- the seam ------------------------------------------------------------------------------------------
def test_seam_set_query_restore(cu_count):
    lib = L.lib()
    assert lib.yms_cu_count_set(-1) == 0                 # the default: the device's own count
    case = T.DIRECT[0]
    dev_rows = T.direct_fwd_grid(*case, "bf16")
    assert cu_count(1) == 0                              # returns the previous setting
    assert lib.yms_cu_count_set(-1) == 1                 # a negative argument only queries
    assert lib.yms_cu_count_set(-7) == 1 and lib.yms_cu_count_set(-1) == 1
    rows1 = T.direct_fwd_grid(*case, "bf16")
    assert cu_count(3) == 1
    rows3 = T.direct_fwd_grid(*case, "bf16")
    assert 1 <= rows1 < rows3 <= 6                       # at most two blocks per CU
    assert rows3 % 3 == 0 and rows1 * 3 == rows3
    assert cu_count(0) == 3                              # 0: back to the device's count
    assert lib.yms_cu_count_set(-1) == 0
    assert T.direct_fwd_grid(*case, "bf16") == dev_rows


def test_seam_reaches_every_sizing_query(cu_count):
    """statistics rows of both forward kernels, the BN-reduce rows and both workspace queries follow it"""
    def all_queries():
        return (T.ntp_stats_grid(T.NTP[0], "bf16"), T.direct_fwd_grid(*T.DIRECT[0], "bf16"),
                T.bnred_grid(T.BNRED[0], "bf16"), T.wg_ws_bytes(T.WG_GEMM[0], "bf16"),
                T.dw_ws_rows((1, 40, 65, 24, 7), "bf16"))
    cu_count(1)
    one = all_queries()
    cu_count(2048)
    many = all_queries()
    assert all(a < b for a, b in zip(one, many)), (one, many)


# ---- every queried case walks -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", T.LOWP)
def test_ntp_stats_cases_walk(dt, cu_count):
    uneven = 0
    for case in T.NTP:
        tiles, tn = T.ntp_tiles(case, dt)
        for ov in T.OVERRIDES:
            cu_count(ov)
            grid = T.ntp_stats_grid(case, dt)
            occ = case[9]
            assert grid == max(tn, occ * ov - occ * ov % tn), (case, ov, grid)      # ntp_grid's rule
            assert walks(tiles, grid), (case, ov, tiles, grid)
            # blocks walk tiles of one column tile: unequal counts = the row tiles do not divide
            uneven += (tiles // tn) % (grid // tn) != 0
        # eval under override 1 (derived, no query): 4 x the blocks per CU
        assert walks(tiles, T.ntp_eval_grid(case, 1)), case
    assert uneven >= 3
    # the ragged last row tile belongs to a block that owns earlier tiles too: true of every walking case, as
    # block b owns tiles b, b + G, ... and every block owns >= 2
    cu_count(0)
    assert all(T.ntp_shape(c, dt).n * T.ntp_shape(c, dt).ho * T.ntp_shape(c, dt).wo % c[7] != 0 for c in T.NTP)


def test_ntp_cases_cover_the_tile_configs():
    assert {c[7:10] for c in T.NTP} == {(128, 128, 2), (128, 64, 3), (256, 32, 2)}
    assert any(c[5] == 1 and c[1] <= 64 for c in T.NTP)                 # shallow 1x1 GEMMs
    assert any(c[5] == 3 and c[6] == 1 for c in T.NTP) and any(c[5] == 3 and c[6] == 2 for c in T.NTP)
    assert any(c[4] % 8 for c in T.NTP) and any(c[4] % 64 for c in T.NTP) and any(c[4] % 128 for c in T.NTP)


def test_group_members_differ_in_tiles(cu_count):
    cu_count(1)
    for cin, cout, k in T.GROUP_CONVS:
        bm, bn, occ = (128, 128, 2) if cout > 64 else (128, 64, 3)
        tiles, grids = [], []
        for hw in T.GROUP_MAPS:
            case = (3, cin, hw, hw, cout, k, 1, bm, bn, occ)
            tiles.append(T.ntp_tiles(case)[0])
            grids.append(T.ntp_stats_grid(case, "bf16"))
        assert len(set(tiles)) == 3
        assert walks(tiles[0], grids[0]) and walks(tiles[1], grids[1]) and not walks(tiles[2], grids[2])


@pytest.mark.parametrize("dt", T.LOWP)
def test_direct_cases_walk(dt, cu_count):
    uneven_f = uneven_d = 0
    for case in T.DIRECT:
        n, cin, h, w, cout = case
        tiles = T.direct_tiles(n, h, w)
        for ov in T.OVERRIDES:
            cu_count(ov)
            gf, gd = T.direct_fwd_grid(*case, dt), T.direct_dgrad_grid(case, dt)
            assert gf in (ov, 2 * ov) and gd in (ov, 2 * ov)                 # the direct route, OCC 1 or 2
            assert walks(tiles, gf) and walks(tiles, gd), (case, ov, tiles, gf, gd)
            uneven_f += tiles % gf != 0
            uneven_d += tiles % gd != 0
    assert uneven_f >= 1 and uneven_d >= 1
    # TW 32 and 16, 32 and 64 reduction channels, one and two fragments, ragged heights
    assert {c[3] % 32 == 0 for c in T.DIRECT} == {True, False}
    assert {(c[1] + 7) // 8 * 8 for c in T.DIRECT} == {32, 64} and {c[4] <= 32 for c in T.DIRECT} == {True, False}
    assert any(c[2] % (256 // (32 if c[3] % 32 == 0 else 16)) for c in T.DIRECT)


def test_direct_stride2_cases_walk():
    """no query for the plain launch: at most two blocks per CU (DirGeo2::OCC)"""
    for n, cin, h, w, cout in T.DIRECT_S2:
        tiles = T.direct_s2_tiles(n, h, w)
        assert all(walks(tiles, 2 * ov) for ov in T.OVERRIDES), (n, cin, h, w, cout, tiles)
        assert tiles % 6 != 0 or tiles % 3 != 0


@pytest.mark.parametrize("dt", T.LOWP)
def test_bnred_cases_walk(dt, cu_count):
    uneven = {1: 0, 2: 0}
    for case in T.BNRED:
        tiles = T.bnred_tiles(case)
        for ov in T.OVERRIDES:
            cu_count(ov)
            grid = T.bnred_grid(case, dt)
            assert grid == ov, (case, ov, grid)                                # one block per CU
            assert walks(tiles, grid)
            uneven[case[5]] += tiles % grid != 0
    assert uneven[1] >= 1 and uneven[2] >= 1
    assert {c[6] for c in T.BNRED if c[5] == 1} == {0, 1} == {c[6] for c in T.BNRED if c[5] == 2}


@pytest.mark.parametrize("dt", T.LOWP)
def test_dw_wgrad_rows_as_derived(dt, cu_count):
    """the 16-bit depthwise weight gradients: workspace rows = strips / unit groups / blocks as
    tile_walk_cases.py derives them, each kernel with a setting under which a row covers >= 3 tiles or
    units, and one where the rows cover unequal counts"""
    for shp, rows in T.DW_WS_ROWS.items():
        got = []
        for ov in T.DW_OVERRIDES:
            cu_count(ov)
            got.append(T.dw_ws_rows(shp, dt))
        assert tuple(got) == rows, (shp, got)
    # strip kernel (k 3), MFMA (one chunk, two chunks, NB 2), wgrad2: rows = n * column tiles * strips for the
    # first, so its tiles-per-row bound is per tile column
    for shp in ((3, 40, 24, 16, 7), (3, 40, 41, 16, 9), (1, 40, 65, 24, 7), (1, 40, 65, 24, 9), (1, 40, 97, 24, 5),
                (1, 53, 41, 24, 3), (1, 45, 40, 56, 3)):
        units, rows = T.DW_WS_UNITS[shp], T.DW_WS_ROWS[shp]
        assert any(walks(units, r) for r in rows), shp
        assert any(units % r for r in rows), shp
    assert T.DW_WS_UNITS[(3, 24, 24, 16, 5)] % 2 == 1 and T.DW_WS_ROWS[(3, 24, 24, 16, 5)][1] == 2   # NB 2: 2 + 1 units
    assert set(T.DW_WS_ROWS) == {s for _, s in T.DW_CASES}


def test_dw_fp32_wgrad_ignores_the_cu_count(cu_count):
    for shp in T.DW_ALL_DT:
        rows = set()
        for ov in T.DW_OVERRIDES:
            cu_count(ov)
            rows.add(T.dw_ws_rows(shp, "f32"))
        assert len(rows) == 1


@pytest.mark.parametrize("route,shp", T.WG_CASES, ids=lambda v: v if isinstance(v, str) else T.case_id(v))
@pytest.mark.parametrize("dt", T.LOWP)
def test_wgrad_split_counts(route, shp, dt, cu_count, monkeypatch):
    """override 1: one split, so the workspace is one slab (the halo kernel's 32-output-channel blocks keep
    one per k-half); override 2048: a whole number of those, at least three"""
    for k, v in T.WG_ENV[route].items():
        monkeypatch.setenv(k, v)
    cu_count(1)
    one = T.wg_ws_bytes(shp, dt)
    cu_count(2048)
    many = T.wg_ws_bytes(shp, dt)
    assert one == T.wg_slab_bytes(route, shp), (one, T.wg_slab_bytes(route, shp))
    assert many % one == 0 and many // one >= 3, (one, many)
