"""COCO AP (mAP@[.5:.95], AP by size, AR@1/10/100), CPU tier: hand-computed answers of the COCOeval
restatement (tests/cocoeval_ref.py), its agreement with the mAP@0.5 oracle (oracle/map_ref.py) at
thresholds [0.5] / area all / maxDets 100, the native host accumulation (yms_map_accumulate_coco)
cell for cell against the restatement's, and the metric's constructor."""
import ctypes

import numpy as np
import pytest

import cocoeval_ref as C
from oracle import map_ref as R
from yms import _lib as L
from yms.metrics import MeanAveragePrecision


def _d(boxes, scores, labels):
    return {"boxes": np.array(boxes, np.float32).reshape(-1, 4), "scores": np.array(scores, np.float32),
            "labels": np.array(labels, np.int64)}


def _t(boxes, labels):
    return {"boxes": np.array(boxes, np.float32).reshape(-1, 4), "labels": np.array(labels, np.int64)}


def test_known_answer_one_box_iou_077():
    # IoU 0.77: matched at 0.50 .. 0.75 (six thresholds), area 10000 is 'large'
    s = C.coco_eval([_d([[0, 0, 100, 77]], [0.9], [0])], [_t([[0, 0, 100, 100]], [0])])["summary"]
    ap = lambda v: pytest.approx(v, abs=1e-12)
    assert s["map"] == ap(0.6) and s["map_50"] == ap(1.0) and s["map_75"] == ap(1.0)
    assert s["map_large"] == ap(0.6)
    assert s["map_small"] == -1 and s["map_medium"] == -1
    assert s["mar_1"] == ap(0.6) and s["mar_10"] == ap(0.6) and s["mar_100"] == ap(0.6) and s["mar_large"] == ap(0.6)
    assert s["mar_small"] == -1 and s["mar_medium"] == -1


def test_known_answer_small_and_medium():
    # areas 900 (small) and 1600 (medium); each detection is its ground truth.  In the 'small' range the
    # 40x40 pair is ignored (ground truth out of range -> its match is ignored), in 'medium' the 30x30
    g = [[0, 0, 30, 30], [0, 0, 40, 40]]
    s = C.coco_eval([_d(g, [0.9, 0.8], [2, 2])], [_t(g, [2, 2])])["summary"]
    ap = lambda v: pytest.approx(v, abs=1e-12)
    assert s["map"] == ap(1.0) and s["map_small"] == ap(1.0) and s["map_medium"] == ap(1.0)
    assert s["map_large"] == -1
    assert s["mar_1"] == ap(0.5) and s["mar_10"] == ap(1.0)
    assert set(s["map_per_class"]) == {2} and s["mar_100_per_class"][2] == ap(1.0)


def test_restatement_equals_map50_oracle_at_one_threshold():
    preds, targets = C.clustered(np.random.default_rng(11), 24)
    out = C.coco_eval(preds, targets, [0.5])
    m_ref, ap_ref = R.map50(preds, targets)
    assert len(ap_ref) == 6
    for c, v in ap_ref.items():
        assert float(np.mean(out["precision"][0, :, c, 0, 2])) == v, c        # bit for bit
    assert out["summary"]["map_per_class"] == ap_ref
    for (p, t), (rank, matched, ignored, _) in zip(zip(preds, targets), out["per_image"]):
        tp, kept = R.match_image(p["boxes"], p["scores"], p["labels"], t["boxes"], t["labels"])
        assert np.array_equal(matched[0, 0], tp.astype(bool))
        assert np.array_equal(rank < 100, kept.astype(bool))
        assert not ignored[0].any()
    assert m_ref == pytest.approx(out["summary"]["map_50"], abs=1e-12)


def test_host_accumulate_matches_restatement():
    rng = np.random.default_rng(0)
    T, K = 10, 8
    per_image, npig = [], np.zeros((K, 4), np.int32)
    scores, labels, image, rank, mt, ig = [], [], [], [], [], []
    for i in range(25):
        n = int(rng.integers(0, 60))
        sc = rng.choice(np.linspace(0, 1, 17).astype(np.float32), n)     # many exact ties
        lb = rng.integers(0, 6, n)
        rk = np.zeros(n, np.int32)
        for c in range(6):
            idx = np.nonzero(lb == c)[0]
            rk[idx[np.argsort(-sc[idx], kind="mergesort")]] = np.arange(len(idx))
        if i == 3 and n:
            rk[lb == lb[0]] += 98                                          # some ranks beyond the 100 kept
        m = rng.random((4, T, n)) < 0.4
        g = rng.random((4, T, n)) < 0.2
        per_image.append((sc, lb, rk, m, g))
        bits = (1 << np.arange(T)).reshape(1, T, 1)
        scores.append(sc); labels.append(lb); image.append(np.full(n, i)); rank.append(rk)
        mt.append((m * bits).sum(1)); ig.append((g * bits).sum(1))
        for c in rng.integers(0, 7, int(rng.integers(0, 5))):
            npig[c] += rng.integers(0, 2, 4)
    npig[7] = 0
    p_ref, r_ref = C.accumulate_flags(per_image, npig, K, T)
    cat = lambda xs, dt, ax=0: np.ascontiguousarray(np.concatenate(xs, axis=ax).astype(dt))
    sc, lb, im, rk = cat(scores, np.float32), cat(labels, np.int32), cat(image, np.int32), cat(rank, np.int32)
    m16, g16 = cat(mt, np.uint16, 1), cat(ig, np.uint16, 1)
    prec = np.zeros((T, 101, K, 4, 3))
    rec = np.zeros((T, K, 4, 3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.lib().yms_map_accumulate_coco(sc.size, p(sc), p(lb), p(im), p(rk), p(m16), p(g16), T, K, p(npig),
                                           p(prec), p(rec)) == 0
    assert np.array_equal(prec, p_ref)                                   # every cell identical
    assert np.array_equal(rec, r_ref)
    assert (p_ref[:, :, 7] == -1).all() and (p_ref > -1).any() and (r_ref > 0).any()
    # argument checks
    assert L.lib().yms_map_accumulate_coco(sc.size, p(sc), p(lb), p(im), p(rk), p(m16), p(g16), 17, K, p(npig),
                                           p(prec), p(rec)) == 1
    assert L.lib().yms_map_match_coco(1, 0, None, None, None, None, None, None, None, 17, p(np.full(17, 0.5)), None,
                                      None, None, None, 0, None) == 1


def test_constructor():
    assert np.array_equal(MeanAveragePrecision().iou_thresholds, C.IOU_THRS)
    assert list(MeanAveragePrecision(iou_thresholds=[0.3, 0.6]).iou_thresholds) == [0.3, 0.6]
    MeanAveragePrecision(box_format="xyxy", iou_type="bbox", iou_thresholds=[0.5])
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_thresholds=list(np.linspace(0.1, 0.9, 17)))
    with pytest.raises(ValueError):
        MeanAveragePrecision(box_format="xywh")
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_type="segm")
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_thresholds=[])
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_thresholds=[0.6, 0.5])
