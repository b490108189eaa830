"""CPU tier of test-time augmentation (yms.tta): the view-size and row-trim rules, the geometry of
the view merge as a round trip that does not depend on the restatement being right, the argument
checks that come before any GPU work, and box voting's restatement on a case worked out by hand."""
import ctypes

import numpy as np
import pytest

import tta_ref as T
from yms import _lib as L
from yms import data as D
from yms import tta

F32 = np.float32
ORIGINALS = [(120, 200), (200, 120), (97, 131)]                # (h0, w0)
VIEWS = [(128, 128), (96, 96), (64, 64)]


def forward_boxes(boxes0, frame, size, flip):
    """Boxes (cx, cy, w, h) in original pixels -> view pixels, in float64: v = x0 * gain + pad through
    the letterbox's frame, then the flip W - v."""
    gx, gy, px, py = frame[:4]
    H, W = size
    b = np.asarray(boxes0, np.float64)
    cx, cy = b[:, 0] * gx + px, b[:, 1] * gy + py
    if flip & 1:
        cx = W - cx
    if flip & 2:
        cy = H - cy
    return np.stack([cx, cy, b[:, 2] * gx, b[:, 3] * gy], 1)


def round_trip_case(h0, w0, size, flip, nc=2, seed=0):
    """-> (boxes in original pixels [m, 4] float64, pred [1, m, 4+nc] fp32 in view pixels, frame)."""
    rng = np.random.default_rng(seed + 1000 * flip + h0)
    m = 16
    boxes0 = np.stack([rng.uniform(0, w0, m), rng.uniform(0, h0, m), rng.uniform(1, w0, m), rng.uniform(1, h0, m)], 1)
    frame = D.Letterbox(h0, w0, *size).frame
    pred = np.zeros((1, m, 4 + nc), F32)
    pred[0, :, :4] = forward_boxes(boxes0, frame, size, flip)
    pred[0, :, 4:] = rng.uniform(0, 1, (m, nc))
    return boxes0, pred, frame


@pytest.mark.parametrize("flip", [0, 1, 2, 3])
@pytest.mark.parametrize("size", VIEWS)
@pytest.mark.parametrize("orig", ORIGINALS)
def test_geometry_round_trip(orig, size, flip):
    """Four fp32 roundings on coordinates below 2048 give at most ~5e-4 px."""
    boxes0, pred, frame = round_trip_case(*orig, size, flip)
    out = T.merge([pred], [F32([frame])], [size], [flip])
    assert out.shape == pred.shape and out.dtype == F32
    err = np.abs(out[0, :, :4].astype(np.float64) - boxes0).max()
    print(orig, size, flip, "max error", err)
    assert err <= 1e-3
    assert np.array_equal(out[0, :, 4:], pred[0, :, 4:])


def test_view_sizes():
    assert tta.view_sizes((640, 640), (1, .83, .67)) == [(640, 640), (544, 544), (448, 448)]
    assert tta.view_sizes(640, (1, .83, .67)) == [(640, 640), (544, 544), (448, 448)]
    assert tta.view_sizes((128, 128), (1, .75, .5)) == [(128, 128), (96, 96), (64, 64)]
    assert tta.view_sizes((480, 640), (0.5,), stride=64) == [(256, 320)]
    assert T.view_sizes((640, 640), (1, .83, .67)) == tta.view_sizes((640, 640), (1, .83, .67))


def test_trim_rows():
    want = [(0, 320), (0, 189), (64, 84)]
    assert tta.trim_rows((128, 96, 64), (8, 16, 32)) == want
    assert tta.trim_rows(VIEWS, (8, 16, 32)) == want
    assert T.trim_rows(VIEWS, (8, 16, 32)) == want
    assert tta.trim_rows([(128, 128)], (8, 16, 32)) == [(0, 336)]              # one view keeps everything
    assert tta.trim_rows([(64, 128), (64, 64)], (8, 16, 32)) == [(0, 160), (64, 84)]
    v = tta.Views([np.zeros((1, 336, 5)), np.zeros((1, 189, 5)), np.zeros((1, 84, 5))], [None] * 3, VIEWS, (0, 1, 0))
    assert v.rows() == [(0, 336), (0, 189), (0, 84)] and v.rows(True) == want
    assert v.locate(0) == (0, 0) and v.locate(336) == (1, 0) and v.locate(336 + 189 + 83) == (2, 83)
    assert v.locate(319, True) == (0, 319) and v.locate(320, True) == (1, 0) and v.locate(509, True) == (2, 64)
    with pytest.raises(IndexError):
        v.locate(609)


class _Untouched:
    """A model that fails the test if predict_views gets as far as looking at it."""

    @property
    def training(self):
        raise AssertionError("the argument checks come first")


def test_predict_views_argument_errors():
    for kw in (dict(scales=(1.0, 0.5), flips=(0,)), dict(scales=(1.0,) * 9, flips=(0,) * 9),
               dict(scales=(1.0,), flips=(4,)), dict(scales=(1.0,), flips=(-1,)), dict(scales=(), flips=())):
        with pytest.raises(ValueError):
            tta.predict_views(_Untouched(), [object()], size=64, **kw)


def test_view_plans_flip_stages():
    """The letterbox tile plus one stage per flip bit, with sample_mosaic's matrices."""
    for flip, names in ((0, []), (1, ["fliplr"]), (2, ["flipud"]), (3, ["fliplr", "flipud"])):
        (lb, plan), = tta.view_plans([(97, 131)], (64, 96), flip)
        ly = plan.layers[0]
        assert plan.applied == ["mosaic", "letterbox"] + names and plan.frame == (96, 64)
        assert lb.frame == D.Letterbox(97, 131, 64, 96).frame
        for (F, in_w, in_h, out_w, out_h, border), name in zip(ly.stages, names):
            assert (in_w, in_h, out_w, out_h, border) == (96, 64, 96, 64, D.AUG_CLAMP)
            want = [[-1, 0, 95], [0, 1, 0], [0, 0, 1]] if name == "fliplr" else [[1, 0, 0], [0, -1, 63], [0, 0, 1]]
            assert np.array_equal(F, np.float64(want))


def test_merge_argument_errors_without_gpu():
    """yms_tta_merge's checks return YMS_ERR_INVALID before any launch (host dummies, never read)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    P, I = ctypes.c_void_p, ctypes.c_int

    def call(n=2, nc=3, nv=2, A=(8, 8), a0=(0, 2), a1=(8, 6), H=(64, 32), W=(64, 32), flips=(1, 2),
             preds=None, frames=None, out=p):
        m = len(A)
        preds = [p] * m if preds is None else preds
        frames = [p] * m if frames is None else frames
        return L.lib().yms_tta_merge(n, nc, nv, (P * m)(*preds), (I * m)(*A), (I * m)(*a0), (I * m)(*a1), (I * m)(*H),
                                     (I * m)(*W), (I * m)(*flips), (P * m)(*frames), out, None)
    big = [1 << 20] * 9
    bad = (dict(nv=0), dict(nv=9, A=big, a0=[0] * 9, a1=big, H=[64] * 9, W=[64] * 9, flips=[0] * 9),
           dict(a0=(0, 6)), dict(a0=(0, 7)), dict(a1=(9, 6)), dict(a0=(-1, 2)), dict(flips=(1, 4)), dict(flips=(-1, 0)),
           dict(H=(64, 0)), dict(W=(0, 32)), dict(n=0), dict(nc=0), dict(out=None), dict(preds=[p, None]),
           dict(frames=[None, p]),
           # sum of rows * nc reaches 2^31: 2 views x 2^20 rows x 1024 classes
           dict(nc=1024, A=big[:2], a0=(0, 0), a1=big[:2]))
    for kw in bad:
        assert call(**kw) == 1, kw


def test_vote_argument_errors_without_gpu():
    """yms_det_finalize_vote: a valid argument list with ONE argument broken (never launched)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) & ~15
    ok = [1, 8, 4, p, p, p, p, p, p, None, p, p, ctypes.c_double(0.5), p, p, p, None]
    for i, v in ((0, 0), (1, 0), (1, 65537), (2, 0), (2, 1025), (3, None), (10, None), (11, None), (13, None),
                 (12, ctypes.c_double(float("nan"))), (3, p + 4)):
        a = list(ok)
        a[i] = v
        assert L.lib().yms_det_finalize_vote(*a) == 1, i


def test_vote_by_hand():
    """Two identical boxes with scores 0.75 and 0.25 and one disjoint box: NMS keeps the 0.75 box and
    the disjoint one; the voted box of the first is (0.75 b + 0.25 b) / 1 = b, the disjoint box has
    itself as its only member and does not move.  With the second score a different box: the mean."""
    pred = np.zeros((4, 5), F32)
    pred[0] = (20, 20, 10, 10, 0.75)
    pred[1] = (20, 20, 10, 10, 0.25)
    pred[2] = (60, 60, 8, 8, 0.5)
    pred[3] = (90, 90, 8, 8, 0.01)                           # below conf: not live, never a member
    cand = T.R.candidates(pred, 0.1, True, None, 8)
    kept = T.R.nms_rows(cand, 0.5, False)
    assert cand["count"] == 3 and list(kept) == [0, 2]
    det, anchor, m, rows = T.finalize_vote(cand, kept, 4, 0.5, False)
    assert m == 2 and list(rows) == [0, 2] and list(anchor[:2]) == [0, 2]
    assert list(T.members(cand, 0, 0.5, False)) == [0, 1] and list(T.members(cand, 2, 0.5, False)) == [2]
    assert np.array_equal(det[0, :4], F32([15, 15, 25, 25])) and np.array_equal(det[1, :4], F32([56, 56, 64, 64]))
    assert np.array_equal(det[:2, 4], F32([0.75, 0.5]))
    # a shifted partner: IoU((15,15,25,25), (16,15,26,25)) = 90 / 110 > 0.5; mean x = 15 + 0.25 = 15.25
    pred[1, 0] = 21
    cand = T.R.candidates(pred, 0.1, True, None, 8)
    det, _, m, _ = T.finalize_vote(cand, T.R.nms_rows(cand, 0.5, False), 4, 0.5, False)
    assert m == 2 and np.array_equal(det[0, :4], F32([15.25, 15, 25.25, 25]))
    # a frame applies after the vote
    det, _, _, _ = T.finalize_vote(cand, T.R.nms_rows(cand, 0.5, False), 4, 0.5, False, (0.5, 0.5, 1, 2, 40, 40))
    assert np.array_equal(det[0, :4], F32([28.5, 26, 40, 40]))
    # zero-area kept box and an infinite score keep their own boxes
    pred[2, 2] = 0
    pred[0, 4] = np.inf
    cand = T.R.candidates(pred, 0.1, True, None, 8)
    kept = T.R.nms_rows(cand, 0.5, False)
    det, _, m, rows = T.finalize_vote(cand, kept, 4, 0.5, False)
    assert list(rows) == [0, 2] and len(T.members(cand, 2, 0.5, False)) == 0
    assert np.array_equal(det[0, :4], F32([15, 15, 25, 25])) and np.array_equal(det[1, :4], F32([60, 56, 60, 64]))
