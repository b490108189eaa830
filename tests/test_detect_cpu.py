"""CPU tier of the COCO-protocol detect: the numpy restatement (tests/detect_ref.py) against answers
worked out by hand, the LetterBox geometry, and the argument checks of the new C entry points.

The hand case: 6 anchors, 3 classes, conf 0.25, IoU 0.5, a 32 x 32 input that letterboxes a
40 x 64 (h0 x w0) original: r = min(32/40, 32/64) = 0.5, the image is 32 x 20 at left 0, top
round(6 - 0.1) = 6, frame (0.5, 0.5, 0, 6, 64, 40) -- divisions by 0.5 are exact.

  anchor  box xyxy (input px)   scores c0 / c1 / c2     unmapped ((x - 0) / .5, (y - 6) / .5, clipped)
  a0      (-2,  8, 10, 18)      .9   .5   .1            (0, 4, 20, 24)    x1 clipped low
  a1      (-1,  9, 11, 19)      .3   .8   .2            (0, 6, 22, 26)    IoU(a0, a1) = 99 / 141 = .70
  a2      (20,  2, 34, 12)      .5   .1   .5            (40, 0, 64, 12)   y1 clipped low, x2 clipped high
  a3      (12, 20, 22, 30)      .1   .5   .25           (24, 28, 44, 40)  y2 clipped high; .25 is not > conf
  a4      ( 4,  0, 12,  5)      .0   .6   .0            (8, 0, 24, 0)     wholly in the top padding
  a5      (24, 14, 30, 20)      .5   .2   .7            (48, 16, 60, 28)
No other pair of boxes overlaps.

Multi-label candidates, p = 3 a + c: p0 .9, p1 .5, p3 .3, p4 .8, p6 .5, p8 .5, p10 .5, p13 .6, p15 .5,
p17 .7: ten.  Best-class: a0 c0 .9, a1 c1 .8, a2 c0 .5 (tie c0 / c2 to the lower), a3 c1 .5, a4 c1 .6,
a5 c2 .7: six.  classes = [1, 2]: multi keeps p1, p4, p8, p10, p13, p17; best-class keeps a1, a3,
a4, a5 only -- a2's arg-max is c0, so its c2 = .5 is not a candidate.

Cap K = 6 (multi): by score .9 p0, .8 p4, .7 p17, .6 p13, then two of the five at .5, the lowest
p: p1, p6.  Rows in p order: (a0 c0), (a0 c1), (a1 c1), (a2 c0), (a4 c1), (a5 c2).
  class-wise NMS: c1 = rows 2 (.8, a1), 4 (.6, a4), 1 (.5, a0): row 1 overlaps row 2 -> kept 0, 2, 3, 4, 5.
  agnostic: by score rows 0, 2, 5, 4, 1, 3: row 2 (a1) falls to row 0 (a0) ACROSS classes, row 1 is
  a0's own box -> kept 0, 3, 4, 5.

No cap (K = 10), rows r0..r9 = p0, p1, p3, p4, p6, p8, p10, p13, p15, p17.  Class-wise: c0 = r0, r4,
r8, r2 with r2 (a1) suppressed by r0; c1 = r3, r7, r1, r6 with r1 (a0) suppressed by r3 (a1); c2 = r9,
r5.  Kept: r0 r3 r4 r5 r6 r7 r8 r9.  By (score, row): r0 .9, r3 .8, r9 .7, r7 .6, then .5: r4, r5, r6,
r8.  max_det = 7 cuts the tie: r4, r5, r6 stay, r8 goes."""
import ctypes

import numpy as np
import pytest

import detect_ref as R
from yms import _lib as L
from yms import data as D

F32 = np.float32
XYXY = np.array([[-2, 8, 10, 18], [-1, 9, 11, 19], [20, 2, 34, 12], [12, 20, 22, 30], [4, 0, 12, 5],
                 [24, 14, 30, 20]], F32)
SCORES = np.array([[.9, .5, .1], [.3, .8, .2], [.5, .1, .5], [.1, .5, .25], [.0, .6, .0], [.5, .2, .7]], F32)
FRAME = (0.5, 0.5, 0.0, 6.0, 64.0, 40.0)
UNMAPPED = np.array([[0, 4, 20, 24], [0, 6, 22, 26], [40, 0, 64, 12], [24, 28, 44, 40], [8, 0, 24, 0],
                     [48, 16, 60, 28]], F32)


def pred():
    p = np.zeros((1, 6, 7), F32)
    p[0, :, 0] = (XYXY[:, 0] + XYXY[:, 2]) / 2
    p[0, :, 1] = (XYXY[:, 1] + XYXY[:, 3]) / 2
    p[0, :, 2] = XYXY[:, 2] - XYXY[:, 0]
    p[0, :, 3] = XYXY[:, 3] - XYXY[:, 1]
    p[0, :, 4:] = SCORES
    return p


def pairs(c):
    return list(zip(c["anchor"][:c["count"]].tolist(), c["label"][:c["count"]].tolist()))


def test_candidates_multi_best_and_class_filter():
    p = pred()[0]
    m = R.candidates(p, 0.25, True, None, 16)
    assert (m["count"], m["total"]) == (10, 10)
    assert pairs(m) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 2), (3, 1), (4, 1), (5, 0), (5, 2)]
    assert np.array_equal(m["boxes"][:10], XYXY[[0, 0, 1, 1, 2, 2, 3, 4, 5, 5]])
    assert np.array_equal(m["score"][:10], F32([.9, .5, .3, .8, .5, .5, .5, .6, .5, .7]))
    assert (m["label"][10:] == -1).all() and (m["anchor"][10:] == -1).all() and not m["boxes"][10:].any()
    b = R.candidates(p, 0.25, False, None, 16)
    assert pairs(b) == [(0, 0), (1, 1), (2, 0), (3, 1), (4, 1), (5, 2)]
    assert np.array_equal(b["score"][:6], F32([.9, .8, .5, .5, .6, .7]))
    assert pairs(R.candidates(p, 0.25, True, [1, 2], 16)) == [(0, 1), (1, 1), (2, 2), (3, 1), (4, 1), (5, 2)]
    assert pairs(R.candidates(p, 0.25, False, [1, 2], 16)) == [(1, 1), (3, 1), (4, 1), (5, 2)]


def test_cap_cuts_through_a_score_tie():
    c = R.candidates(pred()[0], 0.25, True, None, 6)
    assert (c["count"], c["total"]) == (6, 10)
    assert pairs(c) == [(0, 0), (0, 1), (1, 1), (2, 0), (4, 1), (5, 2)]
    assert np.array_equal(c["score"], F32([.9, .5, .8, .5, .6, .7]))
    one = R.candidates(pred()[0], 0.25, True, None, 1)
    assert pairs(one) == [(0, 0)] and one["total"] == 10


def test_classwise_and_agnostic_nms():
    c = R.candidates(pred()[0], 0.25, True, None, 6)
    assert R.nms_rows(c, 0.5, False).tolist() == [0, 2, 3, 4, 5]
    assert R.nms_rows(c, 0.5, True).tolist() == [0, 3, 4, 5]
    full = R.candidates(pred()[0], 0.25, True, None, 10)
    assert R.nms_rows(full, 0.5, False).tolist() == [0, 3, 4, 5, 6, 7, 8, 9]


def test_max_det_tie_and_letterbox_frame():
    out = R.detect(pred(), 0.25, 0.5, multi_label=True, max_det=7, max_nms=10, frames=[FRAME])
    assert out["count"].tolist() == [7] and out["candidates"].tolist() == [10] and out["kept"].tolist() == [8]
    anchors = [0, 1, 5, 4, 2, 2, 3]                   # r0 r3 r9 r7 r4 r5 r6
    assert out["anchor"][0].tolist() == anchors
    assert out["det"][0, :, 5].tolist() == [0, 1, 2, 1, 0, 2, 1]
    assert np.array_equal(out["det"][0, :, 4], F32([.9, .8, .7, .6, .5, .5, .5]))
    assert np.array_equal(out["det"][0, :, :4], UNMAPPED[anchors])
    b = out["det"][0, :, :4]
    assert (b[3, 3] - b[3, 1]) == 0 and (b[3, 2] - b[3, 0]) == 16        # a4: in the padding, zero area, kept
    # without a frame the boxes pass through; a smaller max_det pads nothing, a larger one pads with -1
    raw = R.detect(pred(), 0.25, 0.5, multi_label=True, max_det=9, max_nms=10)
    assert raw["count"].tolist() == [8] and np.array_equal(raw["det"][0, :8, :4], XYXY[anchors + [5]])
    assert raw["anchor"][0, 8] == -1 and raw["det"][0, 8].tolist() == [0, 0, 0, 0, 0, -1]
    # agnostic end to end on the capped rows: rows 0, 5, 4, 3 by score
    ag = R.detect(pred(), 0.25, 0.5, multi_label=True, agnostic=True, max_det=3, max_nms=6)
    assert ag["kept"].tolist() == [4] and ag["anchor"][0].tolist() == [0, 5, 4]
    assert ag["det"][0, :, 5].tolist() == [0, 2, 1]


def test_pick16_is_the_prep_rule():
    """Max score, ties to the lower class; with more than 16 classes across the lanes' strides."""
    rng = np.random.default_rng(0)
    s = (rng.integers(0, 8, (50, 37)) / 8).astype(F32)
    best, bl = R.pick16(s)
    assert np.array_equal(best, s.max(1)) and np.array_equal(bl, s.argmax(1))
    best, bl = R.pick16(s[:, :1])
    assert np.array_equal(best, s[:, 0]) and (bl == 0).all()


@pytest.mark.parametrize("h0,w0,H,W,r,nw,nh,left,top", [
    (120, 200, 320, 320, 1.6, 320, 192, 0, 64),
    (200, 120, 320, 320, 1.6, 192, 320, 64, 0),
    (1, 1, 320, 320, 320.0, 320, 320, 0, 0),
    (641, 3, 320, 320, 320 / 641, 1, 320, 159, 0),        # 3 r = 1.4977 -> 1; (320 - 1) / 2 - .1 = 159.4
    (120, 200, 96, 128, 0.64, 128, 77, 0, 9),             # 76.8 -> 77; (96 - 77) / 2 - .1 = 9.4
    (200, 120, 96, 128, 0.48, 58, 96, 35, 0),             # 57.6 -> 58; (128 - 58) / 2 - .1 = 34.9
    (1, 1, 96, 128, 96.0, 96, 96, 16, 0),                 # (128 - 96) / 2 - .1 = 15.9
    (641, 3, 96, 128, 96 / 641, 1, 96, 63, 0),            # 3 r = .449 -> 0, at least 1; 63.5 - .1 = 63.4
])
def test_letterbox_geometry(h0, w0, H, W, r, nw, nh, left, top):
    g = D.Letterbox(h0, w0, H, W)
    assert (g.nw, g.nh, g.left, g.top) == (nw, nh, left, top)
    assert g.r == pytest.approx(r, rel=1e-15)
    assert g.frame == (g.r, g.r, float(left), float(top), float(w0), float(h0))
    (ly,) = g.plan().layers
    (t,) = ly.tiles
    assert ly.fill == 114.0 and not ly.stages and ly.frame == (W, H)
    assert t.rect == (left, top, left + nw, top + nh) and (t.ox, t.oy, t.nw, t.nh) == (left, top, nw, nh)


def test_frames_stretch_rows():
    f = D.frames_stretch([(120, 200), (1, 1)], (96, 128), device=None)
    assert f.tensor is None
    assert np.array_equal(f.host, F32([[0.64, 0.8, 0, 0, 200, 120], [128, 96, 0, 0, 1, 1]]))


def test_dataset_letterbox_sample(tmp_path):
    """COCODataset(is_train=False, letterbox=True): decoded image, targets in ORIGINAL pixels as
    (class, x1, y1, x2, y2), the image's Letterbox; the default keeps the Resize plan and targets."""
    from test_data_cpu import _coco
    ann = _coco(tmp_path, [(32, 48), (40, 40)])
    ds = D.COCODataset(str(tmp_path), str(ann), is_train=False, img_size=(64, 64), num_classes=3, letterbox=True)
    img, t, g = ds[1]                                   # image id 10: 32 x 48, one valid box [2, 4, 10, 6] of cat 3
    assert img.shape == (32, 48, 3) and isinstance(g, D.Letterbox)
    assert t.tolist() == [[1.0, 2.0, 4.0, 12.0, 10.0]]
    assert (g.h0, g.w0, g.nw, g.nh, g.left, g.top) == (32, 48, 64, 43, 0, 10)     # r = 4/3; 42.67 -> 43; 10.5 - .1
    _, targets = D.collate_targets([ds[1], ds[0]])[1:]
    assert targets.tolist() == [[0.0, 1.0, 2.0, 4.0, 12.0, 10.0], [1.0, 0.0, 1.0, 2.0, 21.0, 12.0]]
    plain = D.COCODataset(str(tmp_path), str(ann), is_train=False, img_size=(64, 64), num_classes=3)
    _, t0, plan = plain[1]
    assert isinstance(plan, D.AugPlan) and t0.shape == (1, 5) and float(t0[0, 1:].max()) <= 1.0
    train = D.COCODataset(str(tmp_path), str(ann), is_train=True, img_size=(64, 64), num_classes=3, letterbox=True)
    assert isinstance(train[1][2], D.AugPlan)           # evaluation only


def test_new_entry_points_reject_bad_arguments():
    """Each row is a valid call with ONE argument broken and returns YMS_ERR_INVALID before any
    launch (the pointers are 16-byte aligned host dummies, never dereferenced)."""
    raw = (ctypes.c_char * 64)()
    P = (ctypes.addressof(raw) + 15) & ~15
    lib = L.lib()

    def rows(name, good, **broken):
        fn = getattr(lib, name)
        for label, change in broken.items():
            assert set(change) <= set(good), (name, label)
            assert fn(*[change.get(k, v) for k, v in good.items()]) == 1, (name, label)

    need = lib.yms_det_ws_bytes(2, 100, 80, 64)
    assert need > 0 and lib.yms_det_ws_bytes(256, 33600, 1024, 65536) < 64 << 20
    cf = ctypes.c_float
    rows("yms_det_candidates",
         dict(n=2, A=100, nc=80, pred=P, conf=cf(0.25), multi=1, mask=None, K=64, boxes=P, score=P, label=P, anchor=P,
              count=P, total=P, ws=P, ws_bytes=need, stream=None),
         n=dict(n=0), A=dict(A=0), nc=dict(nc=0), nc_big=dict(nc=1025), pred_null=dict(pred=None),
         conf_neg=dict(conf=cf(-0.001)), conf_nan=dict(conf=cf(float("nan"))), K0=dict(K=0), K_big=dict(K=65537),
         boxes_null=dict(boxes=None), score_null=dict(score=None), label_null=dict(label=None),
         anchor_null=dict(anchor=None), count_null=dict(count=None), total_null=dict(total=None),
         ws_null=dict(ws=None), ws_short=dict(ws_bytes=need - 1), boxes_unaligned=dict(boxes=P + 4))
    rows("yms_det_finalize",
         dict(n=2, K=64, max_det=300, boxes=P, score=P, label=P, anchor=P, keep=P, counts=P, frames=None, det=P,
              det_anchor=P, det_count=P, stream=None),
         n=dict(n=0), K0=dict(K=0), K_big=dict(K=65537), max_det0=dict(max_det=0), max_det_big=dict(max_det=1025),
         boxes_null=dict(boxes=None), score_null=dict(score=None), label_null=dict(label=None),
         anchor_null=dict(anchor=None), keep_null=dict(keep=None), counts_null=dict(counts=None),
         det_null=dict(det=None), det_anchor_null=dict(det_anchor=None), det_count_null=dict(det_count=None))


def test_detect_rejects_cpu_tensors_and_bad_ranges():
    import torch
    from yms import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect(torch.zeros(1, 6, 7))
