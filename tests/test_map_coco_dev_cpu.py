"""CPU tier of the device-resident COCO evaluator: the argument checks of yms_map_match_coco_fixed and
yms_map_accumulate_coco_dev (each row is a valid call with ONE argument broken and must return before
any launch: the pointers are host dummies that are never dereferenced), the workspace size, and
CocoEvaluator's host-side pieces (constructor, pad_targets)."""
import ctypes

import numpy as np
import pytest
import torch

from yms import _lib as L
from yms.metrics import CocoEvaluator

INVALID, UNSUPPORTED = 1, 2


def _rows(name, good, status=INVALID, **broken):
    fn = getattr(L.lib(), name)
    for label, change in broken.items():
        assert set(change) <= set(good), (name, label)
        assert fn(*[change.get(k, v) for k, v in good.items()]) == status, (name, label)


def test_match_fixed_argument_validation():
    buf = (ctypes.c_double * 16)(*np.linspace(0.5, 0.95, 10), *([0.0] * 6))
    P = ctypes.addressof(buf)
    keep = [(ctypes.c_double * 17)(*np.linspace(0.1, 0.9, 17)), (ctypes.c_double * 2)(0.6, 0.5),
            (ctypes.c_double * 2)(0.5, 0.5), (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(1.5)]
    A = [ctypes.addressof(k) for k in keep]
    good = dict(n_images=2, max_det=8, det_boxes=P, det_scores=P, det_labels=P, det_count=P, max_gt=4, gt_boxes=P,
                gt_labels=P, gt_count=P, n_thr=10, iou_thrs=P, n_classes=6, cap=64, row0=16, score=P, label=P, rank=P,
                matched=P, ignored=P, npig=P, order_ws=P, stream=None)
    nulls = {k + "_null": {k: None} for k in ("det_boxes", "det_scores", "det_labels", "det_count", "gt_boxes",
                                               "gt_labels", "gt_count", "iou_thrs", "score", "label", "rank", "matched",
                                               "ignored", "npig", "order_ws")}
    _rows("yms_map_match_coco_fixed", good, **nulls,
          n_thr0=dict(n_thr=0), n_thr17=dict(n_thr=17, iou_thrs=A[0]), decreasing=dict(n_thr=2, iou_thrs=A[1]),
          repeated=dict(n_thr=2, iou_thrs=A[2]), thr_zero=dict(n_thr=1, iou_thrs=A[3]), thr_above_one=dict(n_thr=1, iou_thrs=A[4]),
          max_det0=dict(max_det=0), max_det1025=dict(max_det=1025), n_classes0=dict(n_classes=0),
          n_classes4097=dict(n_classes=4097), max_gt_negative=dict(max_gt=-1), row0_negative=dict(row0=-8),
          block_past_cap=dict(row0=49))
    _rows("yms_map_match_coco_fixed", good, status=UNSUPPORTED, max_gt2049=dict(max_gt=2049))
    # an empty batch is legal, but only with valid settings
    assert L.lib().yms_map_match_coco_fixed(*[dict(good, n_images=0)[k] for k in good]) == 0
    assert L.lib().yms_map_match_coco_fixed(*[dict(good, n_images=0, max_det=0)[k] for k in good]) == INVALID


def test_accumulate_dev_argument_validation():
    buf = (ctypes.c_double * 16)()
    P = ctypes.addressof(buf)
    ws = L.lib().yms_map_accumulate_coco_dev_ws_bytes(100, 10, 6)
    good = dict(n_rows=100, cap=128, score=P, label=P, rank=P, matched=P, ignored=P, n_thr=10, n_classes=6, npig=P,
                precision=P, recall=P, ws=P, ws_bytes=ws, stream=None)
    nulls = {k + "_null": {k: None} for k in ("score", "label", "rank", "matched", "ignored", "npig", "precision",
                                               "recall", "ws")}
    _rows("yms_map_accumulate_coco_dev", good, **nulls, n_thr0=dict(n_thr=0), n_thr17=dict(n_thr=17),
          n_classes0=dict(n_classes=0), n_classes4097=dict(n_classes=4097), rows_negative=dict(n_rows=-1),
          rows_past_cap=dict(cap=99), rows_past_int=dict(n_rows=2 ** 31, cap=2 ** 31), ws_small=dict(ws_bytes=ws - 1))


def test_workspace_size():
    ws = L.lib().yms_map_accumulate_coco_dev_ws_bytes
    assert ws(0, 10, 80) > 0 and ws(0, 1, 1) > 0                       # never 0: the caller always has a buffer
    rows = [0, 1, 63, 64, 2047, 2048, 2049, 10 ** 4, 10 ** 5, 1500000, 2 ** 31 - 1]
    sizes = [ws(n, 10, 80) for n in rows]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(s >= 24 * n for s, n in zip(sizes, rows))               # two (key, row) ping-pong buffers
    assert ws(1500000, 10, 80) < 26 * 1500000 + (1 << 20)              # and little else: per-tile digit counts
    for n in (0, 5000, 1500000):                                       # non-decreasing in n_thr and n_classes
        by_t = [ws(n, t, 80) for t in (1, 2, 10, 16)]
        by_k = [ws(n, 10, k) for k in (1, 2, 80, 255, 256, 4096)]
        assert all(b >= a for a, b in zip(by_t, by_t[1:])) and all(b >= a for a, b in zip(by_k, by_k[1:]))


def test_pad_targets():
    targets = [{"boxes": np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.float64), "labels": np.array([4, 0, 2])},
               {"boxes": np.zeros((0, 4), np.float32), "labels": np.zeros(0, np.int64)},
               {"boxes": torch.tensor([[0.5, 1.5, 2.5, 3.5]]), "labels": torch.tensor([7])}]
    gb, gl, gc = CocoEvaluator.pad_targets(targets, "cpu")
    assert gb.shape == (3, 3, 4) and gb.dtype == torch.float32
    assert gl.shape == (3, 3) and gl.dtype == torch.int32 and gc.shape == (3,) and gc.dtype == torch.int32
    assert gc.tolist() == [3, 0, 1]
    assert gl.tolist() == [[4, 0, 2], [-1, -1, -1], [7, -1, -1]]       # -1 beyond each image's count
    assert gb[0].tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]] and gb[2, 0].tolist() == [0.5, 1.5, 2.5, 3.5]
    assert not gb[1].any() and not gb[2, 1:].any()
    # one upload: the three results are views of one buffer
    assert gb.untyped_storage().data_ptr() == gl.untyped_storage().data_ptr() == gc.untyped_storage().data_ptr()
    e = CocoEvaluator.pad_targets([{"boxes": np.zeros((0, 4)), "labels": np.zeros(0)}] * 2, "cpu")
    assert e[0].shape == (2, 0, 4) and e[1].shape == (2, 0) and e[2].tolist() == [0, 0]
    e = CocoEvaluator.pad_targets([], "cpu")
    assert e[0].shape == (0, 0, 4) and e[1].shape == (0, 0) and e[2].shape == (0,)
    with pytest.raises(ValueError):
        CocoEvaluator.pad_targets([{"boxes": np.zeros((2, 4)), "labels": np.zeros(1)}], "cpu")


def test_constructor_and_cpu_input():
    ev = CocoEvaluator(80)
    assert len(ev.iou_thresholds) == 10 and ev.iou_thresholds[0] == 0.5 and ev.num_classes == 80
    assert list(CocoEvaluator(3, [0.3, 0.6], capacity_images=1).iou_thresholds) == [0.3, 0.6]
    for bad in (dict(num_classes=0), dict(num_classes=4097), dict(num_classes=2, iou_thresholds=[]),
                dict(num_classes=2, iou_thresholds=[0.6, 0.5]), dict(num_classes=2, iou_thresholds=list(np.linspace(0.1, 0.9, 17))),
                dict(num_classes=2, capacity_images=0)):
        with pytest.raises(ValueError):
            CocoEvaluator(**bad)
    gts = CocoEvaluator.pad_targets([{"boxes": np.zeros((1, 4)), "labels": np.zeros(1)}], "cpu")
    dets = (torch.zeros(1, 8, 4), torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(dets, *gts)
