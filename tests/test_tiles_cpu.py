"""CPU tier of tiled inference (yms.tiles): the window grid on cases worked out by hand, the frames and
suppression bounds of the slots, the argument checks that come before any GPU work, and the merge's
restatement (tests/tiles_ref.py) on a six-row case with one row on each side of each strict comparison."""
import types

import numpy as np
import pytest
import torch

import tiles_ref as TR
from yms import data as D
from yms import tiles

F32 = np.float32
INF = float("inf")


# ------------------------------------------------------------------------------------------
# slice_grid
# ------------------------------------------------------------------------------------------
def test_grid_size_equals_span():
    assert tiles.slice_grid(64, 64, 64) == [(0, 0, 64, 64)]
    assert tiles.slice_grid(64, 64, 64, overlap=0.5) == [(0, 0, 64, 64)]


def test_grid_size_below_span():
    """An axis shorter than the span: the single window [0, size)."""
    assert tiles.slice_grid(40, 64, 64) == [(0, 0, 64, 40)]
    assert tiles.slice_grid(40, 30, 64) == [(0, 0, 30, 40)]


def test_grid_size_span_plus_one():
    """span 64, overlap 0.2: step 64 - int(12.8) = 52; the second window would cross the end and is
    shifted back to size - span = 1."""
    assert tiles.slice_grid(64, 65, 64) == [(0, 0, 64, 64), (1, 0, 65, 64)]
    assert tiles.slice_grid(65, 64, 64) == [(0, 0, 64, 64), (0, 1, 64, 65)]


def test_grid_overlap_zero_and_half():
    # overlap 0: step 64; 128 is covered exactly, 130 needs a shifted third window
    assert [w[0] for w in tiles.slice_grid(64, 128, 64, overlap=0)] == [0, 64]
    assert [w[0] for w in tiles.slice_grid(64, 130, 64, overlap=0)] == [0, 64, 66]
    # overlap 0.5: step 32; 128 = 32 * 3 + 64 ends exactly on the border with the fourth window
    assert [w[0] for w in tiles.slice_grid(64, 128, 64, overlap=0.5)] == [0, 32, 64]
    assert [w[0] for w in tiles.slice_grid(64, 129, 64, overlap=0.5)] == [0, 32, 64, 65]


def test_grid_shifted_last_window_not_repeated():
    """size 100, span 64, step 32: starts 0, 32 (ends at 96 < 100), then 64 would cross the end and is
    shifted to 36, which reaches the end: the walk stops.  A walk that went on to start 96 would shift
    it to 36 again; that repeat is dropped.  No grid holds the same window twice, and the last window
    of each axis ends on the border."""
    assert [w[0] for w in tiles.slice_grid(64, 100, 64, overlap=0.5)] == [0, 32, 36]
    assert tiles._axis(100, 64, 32) == [(0, 64), (32, 96), (36, 100)]
    for size in range(1, 300, 7):
        for span, ov in ((64, 0.0), (64, 0.2), (64, 0.5), (32, 0.9), (96, 0.99)):
            step = span - int(span * ov)
            ax = tiles._axis(size, span, step)
            assert ax == TR.axis_windows(size, span, step)
            assert len(set(ax)) == len(ax) and ax[0][0] == 0 and ax[-1][1] == size
            assert all(b[0] > a[0] and b[0] <= a[1] for a, b in zip(ax, ax[1:]))       # ascending, no gap
            assert all(e - s == span for s, e in ax) or ax == [(0, size)]


def test_grid_non_square_and_zoom():
    """h0 = 70, w0 = 150, span 64, step 52: rows 0 and 6; columns 0, 52, then 104 would cross -> 86."""
    want = [(x, y, x + 64, y + 64) for y in (0, 6) for x in (0, 52, 86)]
    assert tiles.slice_grid(70, 150, 64) == want == TR.slice_grid(70, 150, 64)
    # zoom 2: a 64-pixel tile shows span 32 source pixels; step 32 - int(6.4) = 26
    assert tiles.slice_grid(32, 70, 64, zoom=2.0) == [(0, 0, 32, 32), (26, 0, 58, 32), (38, 0, 70, 32)]
    assert tiles.slice_grid(200, 333, 96, 0.3) == TR.slice_grid(200, 333, 96, 0.3)


# ------------------------------------------------------------------------------------------
# tile_plans: frames, bounds, drawing records
# ------------------------------------------------------------------------------------------
def test_plans_frames_and_bounds():
    """160 x 160 at tile 64, overlap 0.25: step 48, starts 0, 48, 96 per axis -> 9 windows."""
    (slots,) = tiles.tile_plans([(160, 160)], 64, overlap=0.25, full_view=True, edge=3)
    assert len(slots) == 10
    full, corner, interior, last = slots[0], slots[1], slots[5], slots[9]
    lb = D.Letterbox(160, 160, 64, 64)
    assert full.window is None and full.frame == lb.frame[:4] == (0.4, 0.4, 0.0, 0.0)
    assert full.bounds == (-INF, -INF, INF, INF)
    assert corner.window == (0, 0, 64, 64) and corner.frame == (1.0, 1.0, 0.0, 0.0)
    assert corner.bounds == (-INF, -INF, 61.0, 61.0)             # only the cut sides
    assert interior.window == (48, 48, 112, 112) and interior.frame == (1.0, 1.0, -48.0, -48.0)
    assert interior.bounds == (3.0, 3.0, 61.0, 61.0)
    assert last.window == (96, 96, 160, 160) and last.bounds == (3.0, 3.0, INF, INF)
    # the drawing record: a 1:1 tile whose taps land on integer source pixels
    t = interior.plan.layers[0].tiles[0]
    assert (t.nw, t.nh, t.ox, t.oy, t.rect) == (160, 160, -48.0, -48.0, (0, 0, 64, 64))
    assert t.map == (1.0, 1.0, 48.0, 48.0) and interior.plan.frame == (64, 64)
    assert interior.plan.layers[0].fill == D.MOSAIC_FILL and not interior.plan.layers[0].stages
    # against the restatement, every slot
    (want,) = TR.slots([(160, 160)], 64, 0.25, 1.0, True, 3)
    assert [(s.frame, s.bounds, s.window) for s in slots] == [(tuple(f), b, w) for f, b, w in want]


def test_plans_edge_none_against_zero():
    """edge=None: no bound at all; edge=0: bounds on the cut itself (a box sticking out is cut)."""
    (none,) = tiles.tile_plans([(64, 128)], 64, overlap=0, full_view=False)
    (zero,) = tiles.tile_plans([(64, 128)], 64, overlap=0, full_view=False, edge=0)
    assert [s.bounds for s in none] == [(-INF, -INF, INF, INF)] * 2
    assert [s.bounds for s in zero] == [(-INF, -INF, 64.0, INF), (0, -INF, INF, INF)]
    assert [s.frame for s in zero] == [(1.0, 1.0, 0.0, 0.0), (1.0, 1.0, -64.0, 0.0)]


def test_plans_short_image_and_zoom():
    (slots,) = tiles.tile_plans([(40, 100)], 64, overlap=0.5, full_view=False, edge=2)
    assert [s.window for s in slots] == [(0, 0, 64, 40), (32, 0, 96, 40), (36, 0, 100, 40)]
    assert [s.plan.layers[0].tiles[0].rect for s in slots] == [(0, 0, 64, 40)] * 3
    assert slots[1].bounds == (2.0, -INF, 62.0, INF)             # y: the image's own borders
    (z,) = tiles.tile_plans([(32, 70)], 64, zoom=2.0, full_view=False, edge=4)
    assert z[1].window == (26, 0, 58, 32) and z[1].frame == (2.0, 2.0, -52.0, 0.0)
    assert z[1].bounds == (4.0, -INF, 60.0, INF)
    t = z[1].plan.layers[0].tiles[0]
    assert (t.nw, t.nh, t.rect) == (140, 64, (0, 0, 64, 64)) and t.map[:2] == (0.5, 0.5)


def test_table_ragged():
    plans = tiles.tile_plans([(64, 128), (64, 64)], 64, overlap=0, full_view=True, edge=1)
    tab = tiles.slot_table(plans)
    assert tab.shape == (2, 3) and tab.dtype.itemsize == 48
    assert tab["tile"].tolist() == [[0, 1, 2], [3, 4, -1]]
    want = TR.table(TR.slots([(64, 128), (64, 64)], 64, 0, 1.0, True, 1))
    names = ("tile", "gain_x", "gain_y", "pad_x", "pad_y", "lo_x", "lo_y", "hi_x", "hi_y")
    got = np.stack([tab[k].astype(np.float64) for k in names], -1)
    assert np.array_equal(got, want.astype(F32).astype(np.float64))
    assert tab[1, 2]["lo_x"] == -INF and tab[1, 2]["hi_y"] == INF and tab[1, 2]["gain_x"] == 1


def test_locate():
    t = tiles.Tiles(torch.zeros(5, 21, 7), None, None, [[(0, 0, 64, 64), (64, 0, 128, 64)], [(0, 0, 64, 64)]],
                    [(64, 128), (64, 64)], 3, True, 64)
    assert t.locate(0, 0) == (0, None, 0) and t.locate(0, 20) == (0, None, 20)
    assert t.locate(0, 21) == (1, (0, 0, 64, 64), 0) and t.locate(0, 62) == (2, (64, 0, 128, 64), 20)
    assert t.locate(1, 41) == (1, (0, 0, 64, 64), 20)
    for image, row in ((1, 42), (0, 63), (0, -1)):
        with pytest.raises(IndexError):
            t.locate(image, row)


# ------------------------------------------------------------------------------------------
# argument checks, before anything touches a GPU
# ------------------------------------------------------------------------------------------
def fake_model(training=False, strides=(8.0, 16.0, 32.0)):
    """What predict_tiles reads of a model before it runs it (it is not callable: it must not run)."""
    return types.SimpleNamespace(training=training, head=types.SimpleNamespace(
        yms_decode_info=lambda: {"nc": 3, "strides": list(strides)}))


def test_argument_errors():
    im = [torch.zeros(64, 128, 3, dtype=torch.uint8)]
    for bad in (dict(overlap=1.0), dict(overlap=-0.1), dict(zoom=0.0), dict(zoom=3.0), dict(tile=0)):
        with pytest.raises(ValueError):
            tiles.slice_grid(**{**dict(h0=64, w0=128, tile=64), **bad})
    with pytest.raises(ValueError):
        tiles.slice_grid(0, 64, 64)
    with pytest.raises(ValueError):
        tiles.tile_plans([(64, 64)], 64, edge=-1)
    with pytest.raises(RuntimeError):                             # eval mode first
        tiles.predict_tiles(fake_model(training=True), im, tile=64)
    for bad in (dict(tile=48), dict(tile=0), dict(tile=64, overlap=1.0), dict(tile=64, zoom=3.0),
                dict(tile=64, tile_batch=0), dict(tile=64, edge=-2.0)):
        with pytest.raises(ValueError):
            tiles.predict_tiles(fake_model(), im, **bad)
    with pytest.raises(ValueError):
        tiles.predict_tiles(fake_model(strides=(8.0, 16.0, 32.0, 64.0)), im, tile=96)
    with pytest.raises(ValueError):
        tiles.predict_tiles(fake_model(), [], tile=64)
    with pytest.raises(ValueError):
        tiles.detect_tiles(fake_model(), im, tile=64, frames=None)
    with pytest.raises(RuntimeError):                             # host tensors: no CPU fallback
        tiles.predict_tiles(fake_model(), im, tile=64)
    with pytest.raises(RuntimeError):
        tiles.merge_slots(torch.zeros(1, 2, 7), torch.zeros(48, dtype=torch.uint8), 1, 1)


# ------------------------------------------------------------------------------------------
# the reference merge by hand
# ------------------------------------------------------------------------------------------
def test_reference_merge_hand_case():
    """One slot with frame (2, 2, -10, -20) and bounds lo (4, 6), hi (60, 58); boxes (cx, cy, w, h):
      r0  (14, 16, 20, 20)  left side 4 == lo_x, top 6 == lo_y          kept (strict)
      r1  (13.5, 16, 20, 20)  left side 3.5 < 4                          cut
      r2  (50, 48, 20, 20)  right side 60 == hi_x, bottom 58 == hi_y    kept
      r3  (50, 48.5, 20, 20)  bottom 58.5 > 58                           cut
      r4  (30, 15.5, 8, 20)  top 5.5 < 6                                 cut
      r5  (50.5, 30, 20, 8)  right side 60.5 > 60                        cut
    Un-map: cx0 = (cx + 10) / 2, cy0 = (cy + 20) / 2, w0 = w / 2, h0 = h / 2, cut or not."""
    boxes = [(14, 16, 20, 20), (13.5, 16, 20, 20), (50, 48, 20, 20), (50, 48.5, 20, 20), (30, 15.5, 8, 20),
             (50.5, 30, 20, 8)]
    pred = np.zeros((1, 6, 6), F32)
    pred[0, :, :4] = boxes
    pred[0, :, 4] = np.arange(6) / 8 + 0.125
    pred[0, :, 5] = 0.5
    tab = np.array([[[0, 2, 2, -10, -20, 4, 6, 60, 58], [-1, 1, 1, 0, 0, -INF, -INF, INF, INF],
                     [1, 1, 1, 0, 0, -INF, -INF, INF, INF]]], np.float64)
    out = TR.merge(pred, tab)
    assert out.shape == (1, 18, 6)
    want_boxes = [((cx + 10) / 2, (cy + 20) / 2, w / 2, h / 2) for cx, cy, w, h in boxes]
    assert np.array_equal(out[0, :6, :4], F32(want_boxes))
    kept = [True, False, True, False, False, False]
    for a, k in enumerate(kept):
        assert np.array_equal(out[0, a, 4:], pred[0, a, 4:] if k else F32([-1, -1])), a
    # the empty slot and the slot whose tile index is outside pred
    assert np.array_equal(out[0, 6:], np.tile(F32([0, 0, 0, 0, -1, -1]), (12, 1)))
    # no bounds: nothing is cut; a NaN coordinate cuts nothing either and is copied
    tab[0, 0, 5:] = (-INF, -INF, INF, INF)
    assert np.array_equal(TR.merge(pred, tab)[0, :6, 4:], pred[0, :, 4:])
    tab[0, 0, 5:] = (4, 6, 60, 58)
    p2 = pred.copy()
    p2[0, 1, 0] = np.nan
    o2 = TR.merge(p2, tab)
    assert np.isnan(o2[0, 1, 0]) and np.array_equal(o2[0, 1, 4:], pred[0, 1, 4:])
