"""CPU tier of COCO AP with iscrowd and annotation area: pins the restatement tests/cocoeval_crowd_ref.py
(against cocoeval_ref without the two fields, and on hand-worked single-image cases whose expected flags
are written out here), checks that the generator the GPU tier uses exercises what it is meant to, and
covers the host-side pieces: coco_results, COCODetection.eval_annotations, pad_targets(flags=True)."""
import json

import numpy as np
import pytest
import torch

import cocoeval_crowd_ref as R
import cocoeval_ref as C

GPU_SEEDS = (21, 22, 23)          # tests/test_map_crowd_gpu.py: clustered_crowd(default_rng(seed), 8)
T = len(C.IOU_THRS)


def _one(dets, gts, crowd=None, area=None, dscores=None, label=0):
    """one image, one class -> the restatement's result dict"""
    dets, gts = np.asarray(dets, np.float32).reshape(-1, 4), np.asarray(gts, np.float32).reshape(-1, 4)
    sc = np.linspace(0.9, 0.5, len(dets)).astype(np.float32) if dscores is None else np.asarray(dscores, np.float32)
    t = {"boxes": gts, "labels": np.full(len(gts), label, np.int64)}
    if crowd is not None:
        t["iscrowd"] = np.asarray(crowd, np.uint8)
    if area is not None:
        t["area"] = np.asarray(area, np.float32)
    return R.coco_eval([{"boxes": dets, "scores": sc, "labels": np.full(len(dets), label, np.int64)}], [t])


# ------------------------------------------------------------------------------------------
# the restatement without the two fields is cocoeval_ref
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 11])
def test_no_crowd_no_area_equals_cocoeval_ref(seed):
    preds, targets = C.clustered(np.random.default_rng(seed), 12)
    want, got = C.coco_eval(preds, targets), R.coco_eval(preds, targets)
    for w, g in zip(want["per_image"], got["per_image"]):
        for x, y in zip(w, g):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    for k in ("precision", "recall", "npig"):
        assert want[k].tobytes() == got[k].tobytes(), k
    assert want["summary"] == got["summary"]
    # ... also with the fields spelled out as their defaults
    spelled = [dict(t, iscrowd=np.zeros(len(t["labels"]), np.uint8)) for t in targets]
    again = R.coco_eval(preds, spelled)
    assert again["precision"].tobytes() == want["precision"].tobytes() and again["summary"] == want["summary"]


# ------------------------------------------------------------------------------------------
# hand-worked cases
# ------------------------------------------------------------------------------------------
def test_a_detection_inside_a_crowd_is_matched_and_ignored():
    r = _one([[10, 10, 30, 30]], [[0, 0, 100, 100]], crowd=[1])
    rank, matched, ignored, gt_ignore = r["per_image"][0]
    assert matched.shape == (4, T, 1) and matched.all() and ignored.all()
    assert gt_ignore.all() and not r["npig"].any()
    # no other ground truth of the class: the cell is empty (-1), not an AP of 0
    assert (r["precision"] == -1).all() and (r["recall"] == -1).all()
    assert r["summary"]["map"] == -1.0 and r["summary"]["map_per_class"] == {}
    # the same box as an ordinary ground truth: IoU 400 / 10000, a plain false positive and an AP of 0
    o = _one([[10, 10, 30, 30]], [[0, 0, 100, 100]])
    assert not o["per_image"][0][1].any() and o["summary"]["map"] == 0.0


def test_b_three_detections_match_the_same_crowd():
    r = _one([[10, 10, 30, 30], [40, 40, 70, 70], [5, 50, 25, 90]], [[0, 0, 100, 100]], crowd=[1])
    _, matched, ignored, _ = r["per_image"][0]
    assert matched.all() and ignored.all()                    # [4, T, 3]: every one of them, everywhere
    # an ordinary ground truth is used up by the first (here a 100 x 100 one and exact copies of it)
    o = _one([[0, 0, 100, 100]] * 3, [[0, 0, 100, 100]])
    assert o["per_image"][0][1][0].sum(1).tolist() == [1] * T


def test_c_crowd_iou_is_intersection_over_detection_area():
    det, crowd = [[50, 50, 60, 60]], [[0, 0, 200, 200]]
    assert R.crowd_iou(det, crowd, [True])[0, 0] == 1.0
    assert R.crowd_iou(det, crowd, [False])[0, 0] == 100.0 / 40000.0 == 0.0025
    r = _one(det, crowd, crowd=[1])
    assert r["per_image"][0][1][:, T - 1, 0].all()            # matched at 0.95
    assert not _one(det, crowd)["per_image"][0][1].any()      # 0.0025 matches nowhere
    # half inside: 50 of its 100 px^2 -> 0.5 exactly, matched at the first threshold only
    h = _one([[195, 50, 205, 60]], crowd, crowd=[1])
    assert R.crowd_iou([[195, 50, 205, 60]], crowd, [True])[0, 0] == 0.5
    assert h["per_image"][0][1][0, :, 0].tolist() == [True] + [False] * (T - 1)


def test_d_a_regular_match_wins_over_a_better_crowd():
    # crowd first in the input: COCOeval's sort still visits the regular one first
    r = _one([[0, 0, 100, 100]], [[0, 0, 200, 200], [0, 0, 100, 60]], crowd=[1, 0])
    reg = 6000.0 / 10000.0                                    # IoU with the regular one; 1.0 with the crowd
    takes_regular = [bool(reg >= t) for t in C.IOU_THRS]
    assert takes_regular[:2] == [True, True] and takes_regular[3:] == [False] * (T - 3)
    _, matched, ignored, gt_ignore = r["per_image"][0]
    assert matched.all()                                      # above 0.6 the crowd takes it
    # the regular ground truth is 6000 px^2: medium.  all / medium: a TP while it qualifies, else crowd-ignored
    assert ignored[0, :, 0].tolist() == [not x for x in takes_regular]
    assert ignored[2, :, 0].tolist() == [not x for x in takes_regular]
    assert ignored[1, :, 0].all() and ignored[3, :, 0].all()  # small / large: both ground truths are ignore
    assert gt_ignore.T.tolist() == [[True] * 4, [False, True, False, True]]
    assert r["npig"].tolist() == [[1, 0, 1, 0]]
    assert r["recall"][:2, 0, 0, 2].tolist() == [1.0, 1.0] and r["recall"][3:, 0, 0, 2].tolist() == [0.0] * (T - 3)


def test_e_annotation_area_decides_the_size_class():
    box = [[100, 100, 140, 140]]                              # 1600 px^2: medium by w*h
    r = _one(box, box, area=[900.0])                          # the mask's 900 px^2: small
    _, matched, ignored, gt_ignore = r["per_image"][0]
    assert r["npig"].tolist() == [[1, 1, 0, 0]]
    assert gt_ignore[:, 0].tolist() == [False, False, True, True]
    assert matched.all()
    assert not ignored[0].any() and not ignored[1].any()      # a TP in 'all' and in 'small'
    assert ignored[2].all() and ignored[3].all()              # matched-ignored in 'medium' (its own class) and 'large'
    assert (r["precision"][:, :, 0, 1, 2] == 1.0 / (1.0 + C.EPS)).all() and (r["precision"][:, :, 0, 2, 2] == -1).all()
    o = _one(box, box)                                        # without the area: medium
    assert o["npig"].tolist() == [[1, 0, 1, 0]]
    # both ends of a range are inclusive; a negative area is in no range, a NaN in every one
    edges = _one(box * 4, box * 4, area=[1024.0, 9216.0, -1.0, np.nan])
    assert edges["per_image"][0][3].T.tolist() == [[False, False, False, True], [False, True, False, False],
                                                   [True] * 4, [False] * 4]


def test_f_crowd_ground_truths_never_count():
    gts = [[0, 0, 20, 20], [0, 0, 50, 50], [0, 0, 200, 200], [300, 300, 320, 320]]
    r = _one(np.zeros((0, 4)), gts, crowd=[1, 0, 1, 0])
    assert r["npig"].tolist() == [[2, 1, 1, 0]]               # the 50 x 50 and the second 20 x 20
    r = _one(np.zeros((0, 4)), gts, crowd=[1, 1, 1, 1], area=[10, 2000, 20000, 10])
    assert not r["npig"].any() and r["per_image"][0][3].all()


# ------------------------------------------------------------------------------------------
# the generator exercises what the GPU tier needs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_generator_sanity(seed):
    preds, targets = R.clustered_crowd(np.random.default_rng(seed), 8)
    ref = R.coco_eval(preds, targets)
    shared = resized = 0
    for p, t, (rank, matched, ignored, gt_ignore) in zip(preds, targets, ref["per_image"]):
        assert len(p["scores"]) <= 300 and len(t["labels"]) <= 70
        assert t["iscrowd"].dtype == np.uint8 and t["area"].dtype == np.float32
        by_box = C.evaluate_image(p["boxes"], p["scores"], p["labels"], t["boxes"], t["labels"])[3]
        resized += int((by_box[:, t["iscrowd"] == 0] != gt_ignore[:, t["iscrowd"] == 0]).any(0).sum())
        for j in np.nonzero(t["iscrowd"])[0]:                 # detections inside crowd j that nothing else explains
            others = [g for g in range(len(t["labels"])) if g != j and t["labels"][g] == t["labels"][j]]
            if others:
                continue
            inside = (p["labels"] == t["labels"][j]) & matched[0, 0] & (rank < 100)
            shared += int(inside.sum() >= 2)
    assert shared >= 1, "no crowd is matched by two or more detections"
    assert resized >= 1, "no ground truth changes its size class through area"
    assert (ref["npig"].max(0) > 0).all(), "an area column without any counted ground truth"
    assert sum(int(t["iscrowd"].sum()) for t in targets) >= 2
    assert any(m.any() and i.any() and (m & ~i).any() for _, m, i, _ in ref["per_image"])


# ------------------------------------------------------------------------------------------
# host-side pieces of the library
# ------------------------------------------------------------------------------------------
def test_coco_results_round_trip():
    from yms.metrics import coco_results
    boxes = torch.zeros(2, 3, 4)
    boxes[0, 0], boxes[0, 1], boxes[1, 0] = (torch.tensor([10.5, 20.0, 40.0, 60.25]), torch.tensor([0.0, 0.0, 5.0, 5.0]),
                                             torch.tensor([1.0, 2.0, 3.0, 4.0]))
    boxes[1, 1] = torch.tensor([9.0, 9.0, 99.0, 99.0])        # beyond the count: never reported
    scores = torch.tensor([[0.9, 0.5, 0.0], [0.25, 0.7, 0.0]])
    labels = torch.tensor([[2, 0, -1], [1, 1, -1]], dtype=torch.int32)
    counts = torch.tensor([2, 1], dtype=torch.int32)
    out = coco_results((boxes, scores, labels, counts), [397133, 37777], {0: 1, 1: 2, 2: 18})
    assert out == [{"image_id": 397133, "category_id": 18, "bbox": [10.5, 20.0, 29.5, 40.25], "score": float(np.float32(0.9))},
                   {"image_id": 397133, "category_id": 1, "bbox": [0.0, 0.0, 5.0, 5.0], "score": 0.5},
                   {"image_id": 37777, "category_id": 2, "bbox": [1.0, 2.0, 2.0, 2.0], "score": 0.25}]
    assert all(type(v) is float for r in out for v in r["bbox"] + [r["score"]])
    json.dumps(out)                                           # what a results file needs
    assert [r["category_id"] for r in coco_results((boxes, scores, labels, counts), ["a", "b"])] == [2, 0, 1]
    assert coco_results((boxes[:0], scores[:0], labels[:0], counts[:0]), []) == []
    with pytest.raises(ValueError):
        coco_results((boxes, scores, labels, counts), [1])

    class Det:                                                # a Detections-shaped object
        pass
    d = Det()
    d.boxes, d.scores, d.labels, d.counts = boxes, scores, labels, counts
    assert coco_results(d, [397133, 37777], [1, 2, 18]) == out


def _tiny_coco(tmp_path):
    (tmp_path / "img").mkdir()
    for name in ("a.jpg", "b.jpg"):
        (tmp_path / "img" / name).write_bytes(b"")
    ann = {"images": [{"id": 7, "file_name": "a.jpg", "height": 100, "width": 200},
                      {"id": 9, "file_name": "b.jpg", "height": 50, "width": 50}],
           "categories": [{"id": 1, "name": "person"}, {"id": 18, "name": "dog"}],
           "annotations": [
               {"id": 1, "image_id": 7, "category_id": 18, "bbox": [10, 20, 40, 40], "area": 900.5, "iscrowd": 0},
               {"id": 2, "image_id": 7, "category_id": 1, "bbox": [0, 0, 150.5, 80], "area": 7000, "iscrowd": 1},
               {"id": 3, "image_id": 7, "category_id": 99, "bbox": [1, 1, 5, 5], "area": 25, "iscrowd": 0},
               {"id": 4, "image_id": 7, "category_id": 1, "bbox": [5, 5, 10, 10], "area": 0, "iscrowd": 0},
               {"id": 5, "image_id": 7, "category_id": 1, "bbox": [60, 60, 4, 8], "iscrowd": 0}]}
    (tmp_path / "ann.json").write_text(json.dumps(ann))
    return str(tmp_path / "img"), str(tmp_path / "ann.json")


def test_eval_annotations_keeps_what_annotations_drops(tmp_path):
    from yms.data import COCODetection
    ds = COCODetection(*_tiny_coco(tmp_path))
    assert ds.image_ids == [7, 9]
    boxes, labels = ds.annotations(0)                         # training: no crowd, no zero area
    assert boxes == [[10, 20, 40, 40]] and labels == [1]
    t = ds.eval_annotations(0)
    assert t["boxes"].dtype == np.float32 and t["labels"].dtype == np.int64
    assert t["iscrowd"].dtype == np.uint8 and t["area"].dtype == np.float32
    assert t["boxes"].tolist() == [[10, 20, 50, 60], [0, 0, 150.5, 80], [5, 5, 15, 15], [60, 60, 64, 68]]     # xyxy pixels
    assert t["labels"].tolist() == [1, 0, 0, 0]               # the unknown category 99 is gone, as in pycocotools' catIds
    assert t["iscrowd"].tolist() == [0, 1, 0, 0]
    assert t["area"].tolist() == [900.5, 7000.0, 0.0, 32.0]   # the annotation's own; w*h only where it has none
    e = ds.eval_annotations(1)
    assert e["boxes"].shape == (0, 4) and all(len(e[k]) == 0 for k in ("labels", "iscrowd", "area"))


def test_pad_targets_flags():
    from yms.metrics import CocoEvaluator
    two = np.float32(2.0)
    edge = [0, 0, np.float32(32) + two ** -18, np.float32(32) - two ** -19]      # w*h = 1024 + 2^-14 - 2^-37 in double
    targets = [{"boxes": np.array([[1, 2, 3, 4], [5, 6, 7, 8], [0, 0, 10, 10]], np.float64), "labels": np.array([4, 0, 2]),
                "iscrowd": np.array([0, 1, 0]), "area": torch.tensor([1.5, 2.5, 77.0])},
               {"boxes": np.zeros((0, 4), np.float32), "labels": np.zeros(0, np.int64)},
               {"boxes": np.array([[0, 0, 10, 20], edge], np.float32), "labels": torch.tensor([7, 7])},
               {"boxes": torch.tensor([[0.5, 1.5, 2.5, 3.5]]), "labels": torch.tensor([1]), "iscrowd": torch.tensor([True])}]
    plain = CocoEvaluator.pad_targets(targets, "cpu")
    assert len(plain) == 3                                    # the default return is unchanged
    out = CocoEvaluator.pad_targets(targets, "cpu", flags=True)
    assert len(out) == 5
    gb, gl, gc, crowd, area = out
    for x, y in zip(out[:3], plain):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert crowd.shape == (4, 3) and crowd.dtype == torch.uint8 and area.shape == (4, 3) and area.dtype == torch.float32
    assert crowd.tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]]       # 0 for targets without the key and for padding
    assert area[0].tolist() == [1.5, 2.5, 77.0] and area[1].tolist() == [0, 0, 0] and area[2, 2] == 0
    assert area[2, 0] == 200.0 and area[3].tolist() == [4.0, 0, 0]                # the default: w*h
    # a product just above 32^2 that fp32 rounds onto it stays above: medium only, as without any area
    assert float(edge[2]) * float(edge[3]) > 1024.0 and np.float32(float(edge[2]) * float(edge[3])) == 1024.0
    assert area[2, 1].item() > 1024.0
    assert crowd.is_contiguous() and area.is_contiguous()     # update() hands them to the kernel as they are
    base = gb.untyped_storage().data_ptr()                    # still one upload
    assert all(t.untyped_storage().data_ptr() == base for t in (gl, gc, crowd, area))
    # no target has either key: all defaults
    gb2, gl2, gc2, crowd2, area2 = CocoEvaluator.pad_targets(targets[1:3], "cpu", flags=True)
    assert crowd2.shape == (2, 2) and not crowd2.any() and area2[1, 0] == 200.0
    e = CocoEvaluator.pad_targets([], "cpu", flags=True)
    assert e[3].shape == (0, 0) and e[4].shape == (0, 0)
    e = CocoEvaluator.pad_targets([targets[1]] * 2, "cpu", flags=True)
    assert e[3].shape == (2, 0) and e[4].shape == (2, 0)
    with pytest.raises(ValueError, match="iscrowd"):
        CocoEvaluator.pad_targets([{"boxes": np.zeros((2, 4)), "labels": np.zeros(2), "iscrowd": np.zeros(1)}], "cpu", flags=True)
    with pytest.raises(ValueError, match="area"):
        CocoEvaluator.pad_targets([{"boxes": np.zeros((2, 4)), "labels": np.zeros(2), "area": np.zeros(3)}], "cpu", flags=True)
