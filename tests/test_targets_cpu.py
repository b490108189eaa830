"""The float64 restatement of yms_box_targets (tests/targets_ref.py) against the host path it replaces
(yms.data.transform_boxes / mosaic_targets), without a GPU: identical kept sets and coordinates within
2^-23 over a committed list of seeds with the full augmentation config, and every filter's edge."""
import numpy as np
import pytest
import torch

import targets_cases as TC
import targets_ref as R
from yms import cache as C
from yms import data as D

H, W = TC.H, TC.W
# both sides are float32 roundings of doubles that differ by BLAS-level rounding, and the values lie
# in [0, 1], where one float32 spacing is at most 2^-23
TOL = 2.0 ** -23


def _ref(case):
    return R.box_targets(case["tiles"], case["layers"], case["m_cap"], case["boxes"], case["labels"])


@pytest.mark.parametrize("seed", TC.SEEDS)
def test_restatement_matches_the_host_path(seed):
    case = TC.make_batch(seed, 150, eight=(seed == TC.SEEDS[0]))
    ref = _ref(case)
    got, host = R.compact(ref), case["host"]
    kinds = {a for _, p in case["samples"] for a in p.applied}
    assert {"mosaic", "mixup", "affine", "perspective", "resize"} <= kinds, kinds
    assert ref.shape == (150, 6) and 0 < got.shape[0] < 150          # some kept, some filtered
    assert np.array_equal(got[:, :2], host[:, :2]), "kept sets differ"   # (image, class = annotation row)
    diff = np.abs(got[:, 2:] - host[:, 2:]).max()
    print(f"seed {seed}: kept {got.shape[0]} of 150, max |diff| = {diff * 2 ** 23:.3g} x 2^-23")
    assert diff <= TOL
    dropped = ref[ref[:, 0] < 0]
    assert np.array_equal(dropped, np.tile(np.float32(R.IGNORED), (dropped.shape[0], 1)))


def test_row_order_is_the_hosts():
    """Samples in batch order, a MixUp sample's layer 0 before its layer 1: the class column of the
    kept rows (= annotation rows) is the host's."""
    case = TC.make_batch(3, 257)
    mix = case["samples"][2][1]
    first = {case["samples"][2][0][t.src] for t in mix.layers[0].tiles}
    assert first <= set(range(5, 9))
    t = case["tiles"]
    assert np.all(np.diff(t["out0"]) > 0) and int(t["out0"][-1] + t["count"][-1]) == 257
    assert np.array_equal(t["image"], np.sort(t["image"])) and set(t["image"]) == {0, 1, 2}
    assert np.array_equal(R.compact(_ref(case))[:, 1], case["host"][:, 1])


# ------------------------------------------------------------------------------------------
# edges: one hand-built Mosaic layer whose TL tile is cropped by the canvas, identity canvas stage
# ------------------------------------------------------------------------------------------
def _layer():
    """Sources 32 x 48 -> tiles 64 x 96 (gain 2) about the centre (40, 30): TL sits at (-56, -34) and is
    visible in the rect (0, 0, 40, 30); the stage is the identity, so output = canvas coordinates."""
    ly = D.MosaicLayer(2 * H, 2 * W)
    ly.center = (40, 30)
    ly.tiles = D.mosaic_tiles([(32, 48)] * 4, 40, 30, H, W)
    ly.add(np.eye(3), W, H, D.AUG_CONSTANT, "affine")
    t = ly.tiles[0]
    assert (t.ox, t.oy, t.nw, t.nh, t.rect) == (-56, -34, 96, 64, (0, 0, 40, 30))
    return ly


def _mosaic_rows(anns):
    """(restatement's padded rows, host rows) of the edge layer over per-source annotations."""
    ly = _layer()
    offsets = np.zeros(5, np.int64)
    np.cumsum([len(lab) for _, lab in anns], out=offsets[1:])
    boxes = np.array([b for bx, _ in anns for b in bx], np.float64).reshape(-1, 4)
    labels = np.array([c for _, lab in anns for c in lab], np.int32)
    tiles, layers, m = C.target_tables([([0, 1, 2, 3], D.MosaicPlan([ly]))], offsets)
    return R.box_targets(tiles, layers, m, boxes, labels), D.mosaic_boxes(ly, anns).numpy(), tiles


def _areas(box):
    """(unclipped area, clipped area) of a TL-tile source box in the edge layer, restatement arithmetic."""
    x, y, w, h = box
    u = (-56 + x * 2.0, -34 + y * 2.0, -56 + (x + w) * 2.0, -34 + (y + h) * 2.0)
    k = (max(u[0], 0.0), max(u[1], 0.0), min(u[2], 40.0), min(u[3], 30.0))
    return (u[2] - u[0]) * (u[3] - u[1]), max(k[2] - k[0], 0.0) * max(k[3] - k[1], 0.0)


NONE = ([], [])


def test_box_outside_its_tile_rect_is_ignored():
    box = [2.0, 2.0, 10.0, 8.0]                   # canvas x in [-52, -32]: left of the rect
    assert -56 + (box[0] + box[2]) * 2.0 <= 0.0
    ref, host, _ = _mosaic_rows([([box], [1]), NONE, NONE, NONE])
    assert ref.tolist() == [list(R.IGNORED)] and host.shape[0] == 0


def test_box_straddling_the_rect_is_clipped_to_it():
    box = [20.0, 18.0, 20.0, 10.0]                # canvas [-16, 24] x [2, 22] -> [0, 24] x [2, 22]
    ref, host, _ = _mosaic_rows([([box], [2]), NONE, NONE, NONE])
    want = [0.0, 2.0, 12.0 / 96, 12.0 / 64, 24.0 / 96, 20.0 / 64]    # exact in float32
    assert ref.tolist() == [want] and host.tolist() == [want[1:]]


def test_clipped_area_below_one_pixel_is_ignored():
    box = [27.75, 19.5, 0.6, 0.5]                 # canvas [-0.5, 0.7] x [5, 6] -> 0.7 x 1
    area, carea = _areas(box)
    assert carea < 1.0 and carea / area >= 0.1 and area > 1.0        # min_area alone drops it
    ref, host, _ = _mosaic_rows([([box], [3]), NONE, NONE, NONE])
    assert ref.tolist() == [list(R.IGNORED)] and host.shape[0] == 0


def test_visibility_below_a_tenth_is_ignored():
    box = [13.0, 18.0, 16.0, 10.0]                # canvas [-30, 2] x [2, 22] -> 2 x 20 of 32 x 20
    area, carea = _areas(box)
    assert carea >= 1.0 and carea / area < 0.1                       # min_visibility alone drops it
    ref, host, _ = _mosaic_rows([([box], [4]), NONE, NONE, NONE])
    assert ref.tolist() == [list(R.IGNORED)] and host.shape[0] == 0
    box2 = [13.0, 18.0, 16.5, 10.0]               # one more canvas pixel inside: 3 / 33 -> still below
    box3 = [13.0, 18.0, 18.0, 10.0]               # 6 / 36 = 1 / 6: kept
    ref, host, _ = _mosaic_rows([([box2, box3], [5, 6]), NONE, NONE, NONE])
    assert ref[0].tolist() == list(R.IGNORED) and ref[1, :2].tolist() == [0.0, 6.0] and host[:, 0].tolist() == [6.0]


def test_normalised_width_at_or_below_a_thousandth_is_ignored():
    """A plain plan whose only stage is the identity Resize of a 50 x 1000 frame: a box 1 px wide has
    w = 1 / 1000, which is not > 1e-3; its area (20 px) and visibility pass."""
    plan = D.sample_augmentation(np.random.default_rng(0), {}, 50, 1000, 50, 1000, is_train=False)
    assert len(plan.stages) == 1 and np.array_equal(plan.stages[0][0], np.eye(3))
    boxes = [[10.0, 5.0, 1.0, 20.0], [10.0, 5.0, 0.5, 20.0], [10.0, 5.0, 1.5, 20.0]]
    assert (11.0 - 10.0) / 1000.0 == 1e-3
    tiles, layers, m = C.target_tables([([0], plan)], np.array([0, 3]))
    assert int(tiles["clip"][0]) == 0
    ref = R.box_targets(tiles, layers, m, np.array(boxes), np.array([7, 8, 9], np.int32))
    host = D.transform_boxes(boxes, [7, 8, 9], plan).numpy()
    assert ref[0].tolist() == list(R.IGNORED) and ref[1].tolist() == list(R.IGNORED)
    assert np.array_equal(ref[2, 1:], host[0]) and host.shape[0] == 1
    assert ref[2].tolist() == [0.0, 9.0, np.float32(10.75 / 1000), np.float32(15.0 / 50), np.float32(1.5 / 1000),
                               np.float32(20.0 / 50)]


def test_source_without_annotations_gets_no_tile():
    box = [20.0, 18.0, 20.0, 10.0]
    ref, host, tiles = _mosaic_rows([([box], [2]), NONE, ([[1.0, 1.0, 30.0, 20.0]], [1]), NONE])
    assert len(tiles) == 2 and tiles["count"].tolist() == [1, 1] and tiles["out0"].tolist() == [0, 1]
    assert ref.shape[0] == 2 and np.array_equal(R.compact(ref)[:, 1:], host)
    # a batch without any annotation: no tile, no row
    tiles, layers, m = C.target_tables([([0, 1, 2, 3], D.MosaicPlan([_layer()]))], np.zeros(5, np.int64))
    assert len(tiles) == 0 and len(layers) == 1 and m == 0
    assert R.box_targets(tiles, layers, m, np.zeros((0, 4)), np.zeros(0, np.int32)).shape == (0, 6)


def test_table_layouts_match_the_library():
    from yms import _lib as L
    assert L.lib().yms_tgt_tile_bytes() == C.TILE_DT.itemsize == 88
    assert L.lib().yms_tgt_layer_bytes() == C.LAYER_DT.itemsize == 16 + 72 * D.AUG_MAX_STAGES


def test_box_targets_argument_validation():
    """yms_box_targets returns before any launch: M_cap == 0 is YMS_OK, a broken argument is
    YMS_ERR_INVALID (host dummies, never dereferenced)."""
    import ctypes
    from yms import _lib as L
    buf = (ctypes.c_double * 16)()
    P = ctypes.addressof(buf)
    fn = L.lib().yms_box_targets
    assert fn(0, None, 0, None, None, None, 0, 0, None, None) == 0
    assert fn(3, P, 1, P, P, P, 5, 0, P, None) == 0
    good = dict(ntiles=1, tiles=P, nlayers=1, layers=P, boxes=P, labels=P, nann=4, m_cap=4, out=P, stream=None)
    for change in (dict(m_cap=-1), dict(ntiles=0), dict(nlayers=0), dict(nann=0), dict(tiles=None), dict(layers=None),
                   dict(boxes=None), dict(labels=None), dict(out=None), dict(out=P + 4), dict(ntiles=-1)):
        assert fn(*[change.get(k, v) for k, v in good.items()]) == 1, change


def test_compact_targets_drops_the_padding():
    t = torch.tensor([[-1.0, 0, 0, 0, 0, 0], [0, 3, .5, .5, .1, .1], [-1, 0, 0, 0, 0, 0], [2, 1, .2, .2, .1, .1]])
    assert torch.equal(C.compact_targets(t), t[[1, 3]])
    assert C.compact_targets(t[:1]).shape == (0, 6)
