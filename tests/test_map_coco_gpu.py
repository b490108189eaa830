"""GPU tier of COCO AP: the multi-threshold, multi-area matching kernel (yms_map_match_coco) and the
full metric (yms.metrics, default construction) against the COCOeval restatement
(tests/cocoeval_ref.py): identical matched / ignored masks and ranks for every (area range,
detection), and the twelve summary values and per-class dicts within 1e-10.

Where the 1e-10 comes from: a summary value is a float64 mean of at most 16 * 101 * 80 numbers in
[0, 1] (the table cells themselves are identical: the host accumulation is pinned cell for cell in
test_map_coco_cpu.py); whatever the summation order, two such means differ by less than
n * 2^-53 ~ 1.4e-11.  1e-10 is that bound with headroom."""
import numpy as np
import pytest
import torch

import cocoeval_ref as C
from yms.metrics import MeanAveragePrecision

pytestmark = pytest.mark.gpu

TOL = 1e-10
KEYS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large",
        "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")


def _torch(ds, dev="cuda"):
    return [{k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in d.items()} for d in ds]


def _bits(mask, T):
    """[4, n] uint16 masks -> [4, T, n] booleans"""
    return ((mask[:, None, :] >> np.arange(T).reshape(1, T, 1)) & 1).astype(bool)


def _check(preds, targets, thresholds=None, batch=None, torch_preds=None):
    """Run the metric (in update() batches of ``batch`` images) and compare everything with the restatement."""
    metric = MeanAveragePrecision() if thresholds is None else MeanAveragePrecision(iou_thresholds=thresholds)
    n = len(preds)
    step = batch or max(n, 1)
    tp = torch_preds if torch_preds is not None else _torch(preds)
    for i in range(0, n, step):
        metric.update(tp[i:i + step], _torch(targets[i:i + step]))
    out = metric.compute()
    ref = C.coco_eval(preds, targets, thresholds)
    T = len(metric.iou_thresholds)
    # per-detection state of the kernel, every (area, threshold, detection)
    cat = lambda xs, ax: np.concatenate(xs, axis=ax)
    ref_rank = cat([f[0] for f in ref["per_image"]], 0)
    ref_m = cat([f[1] for f in ref["per_image"]], 2)
    ref_i = cat([f[2] for f in ref["per_image"]], 2)
    ref_g = cat([f[3] for f in ref["per_image"]], 1)
    rank = cat(metric._rank, 0)
    kept = rank < 100
    assert np.array_equal(rank, ref_rank)
    assert np.array_equal(kept, ref_rank < 100)
    got_m, got_i = _bits(cat(metric._matched, 1), T), _bits(cat(metric._ignored, 1), T)
    assert got_m.shape == ref_m.shape
    assert np.array_equal(got_m[:, :, kept], ref_m[:, :, kept])
    assert np.array_equal(got_i[:, :, kept], ref_i[:, :, kept])
    assert not got_m[:, :, ~kept].any()                      # beyond the 100 kept: never matched
    # no bit above the T thresholds is ever set
    assert not (cat(metric._matched, 1) >> T).any() and not (cat(metric._ignored, 1) >> T).any()
    got_g = cat(metric._gignore, 0)
    assert np.array_equal(((got_g[None, :] >> np.arange(4).reshape(4, 1)) & 1).astype(bool), ref_g)
    # tables: every cell
    precision, recall, npig = metric.tables()
    assert np.array_equal(npig, ref["npig"])
    assert np.array_equal(precision, ref["precision"])
    assert np.array_equal(recall, ref["recall"])
    # summary
    s = ref["summary"]
    for k in KEYS:
        assert out[k].dtype == torch.float64 and out[k].ndim == 0
        assert abs(out[k].item() - s[k]) <= TOL, (k, out[k].item(), s[k])
    for k in ("map_per_class", "mar_100_per_class"):
        assert set(out[k]) == set(s[k]), k
        for c, v in s[k].items():
            assert abs(out[k][c] - v) <= TOL, (k, c, out[k][c], v)
    return out, ref, metric


def test_clustered_default_thresholds():
    preds, targets = C.clustered(np.random.default_rng(11), 24)
    out, ref, metric = _check(preds, targets, batch=7)         # 7 + 7 + 7 + 3 images
    # the input exercises what it is meant to: all sizes populated, > 100 detections of one class in
    # an image, ignored detections, exact score ties
    for k in KEYS:
        assert 0.10 <= out[k].item() <= 0.85, k
    assert max(np.bincount(p["labels"]).max() for p in preds if len(p["labels"])) > 100
    assert np.concatenate(metric._ignored, 1).any()
    sc = np.concatenate([p["scores"] for p in preds])
    assert len(np.unique(sc)) < len(sc)
    assert out["classes"].tolist() == list(range(6))


def test_150_ground_truths_300_detections_one_class():
    """Ground-truth and detection loops stride past 64 (and past 128) lanes; 300 > 100 detections."""
    rng = np.random.default_rng(5)
    side = np.exp(rng.uniform(np.log(10), np.log(150), (150, 2)))
    ctr = rng.uniform(100, 500, (150, 2))
    gb = np.concatenate([ctr - side / 2, ctr + side / 2], 1).astype(np.float32)
    src = rng.integers(0, 150, 300)
    db = (gb[src] + rng.normal(0, 0.06, (300, 4)) * np.tile(side[src], 2)).astype(np.float32)
    db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
    preds = [{"boxes": db, "scores": (np.round(rng.random(300) * 64) / 64).astype(np.float32),
              "labels": np.zeros(300, np.int64)}]
    targets = [{"boxes": gb, "labels": np.zeros(150, np.int64)}]
    out, ref, _ = _check(preds, targets)
    assert ref["per_image"][0][1].any() and out["map"].item() > 0


def test_ground_truths_span_70_classes():
    """More classes in one image than the workgroup has waves, or a wave has lanes."""
    rng = np.random.default_rng(6)
    n = 90
    gl = np.concatenate([np.arange(70), rng.integers(0, 70, n - 70)])
    rng.shuffle(gl)
    side = np.exp(rng.uniform(np.log(10), np.log(200), (n, 2)))
    ctr = rng.uniform(100, 500, (n, 2))
    gb = np.concatenate([ctr - side / 2, ctr + side / 2], 1).astype(np.float32)
    src = rng.integers(0, n, 200)
    db = (gb[src] + rng.normal(0, 0.06, (200, 4)) * np.tile(side[src], 2)).astype(np.float32)
    db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
    dl = np.where(rng.random(200) < 0.9, gl[src], rng.integers(0, 75, 200))     # some classes without ground truth
    preds = [{"boxes": db, "scores": (np.round(rng.random(200) * 32) / 32).astype(np.float32),
              "labels": dl.astype(np.int64)}]
    targets = [{"boxes": gb, "labels": gl.astype(np.int64)}]
    out, _, _ = _check(preds, targets)
    assert len(out["map_per_class"]) == 70


@pytest.mark.parametrize("thresholds", [list(np.linspace(0.2, 0.95, 16)), [0.3]], ids=["T16", "T1"])
def test_threshold_counts(thresholds):
    """T = 16: all 64 (threshold, area) lanes live; T = 1: one lane per area range.  0.2, 0.25, .., 0.95
    holds 0.5 and 0.75 only up to rounding and [0.3] holds neither: the np.isclose look-up decides
    map_50 / map_75."""
    preds, targets = C.clustered(np.random.default_rng(11), 24)
    out, _, _ = _check(preds[:10], targets[:10], thresholds, batch=4)
    if len(thresholds) == 1:
        assert out["map_50"].item() == -1 and out["map_75"].item() == -1
    else:
        assert out["map_50"].item() > 0 and out["map_75"].item() > 0


def test_iou_equal_to_threshold_matches():
    preds = [{"boxes": np.array([[0, 0, 10, 5]], np.float32), "scores": np.array([1.0], np.float32),
              "labels": np.array([0])}]
    targets = [{"boxes": np.array([[0, 0, 10, 10]], np.float32), "labels": np.array([0])}]
    out, _, metric = _check(preds, targets)
    assert metric._matched[0][0, 0] == 1                       # matched at 0.5 exactly, at nothing above
    assert out["map_50"].item() == pytest.approx(1.0, abs=1e-12)
    assert out["map"].item() == pytest.approx(0.1, abs=1e-12)


def test_empty_images_and_empty_batch():
    preds, targets = C.clustered(np.random.default_rng(11), 24)
    e4, e1 = np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
    el = np.zeros(0, np.int64)
    preds = [preds[1], {"boxes": e4, "scores": e1, "labels": el}, preds[2],
             {"boxes": e4, "scores": e1, "labels": el}]
    targets = [targets[1], targets[2], {"boxes": e4, "labels": el}, {"boxes": e4, "labels": el}]
    _check(preds, targets, batch=2)             # second batch: only-detections image + fully empty image
    _check(preds[3:], targets[3:])              # a batch of one empty image
    metric = MeanAveragePrecision()
    metric.update([], [])                       # an entirely empty batch is legal
    out = metric.compute()
    assert all(out[k].item() == -1 for k in KEYS)
    assert out["map_per_class"] == {} and out["mar_100_per_class"] == {}


def test_more_than_2048_ground_truths_is_unsupported():
    n = 2049
    gb = np.tile(np.array([[0, 0, 10, 10]], np.float32), (n, 1))
    metric = MeanAveragePrecision()
    with pytest.raises(RuntimeError, match=r"yms_map_match_coco failed.*status 2"):
        metric.update(_torch([{"boxes": gb[:1], "scores": np.ones(1, np.float32), "labels": np.zeros(1, np.int64)}]),
                      _torch([{"boxes": gb, "labels": np.zeros(n, np.int64)}]))


def test_default_metric_on_model_postprocess_output():
    """The validation flow (eval forward -> class-wise NMS post-process -> metric) with the default
    construction, on the random-init model with ground truth jittered from its own detections."""
    from yms import ops
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    m = YOLOv8("n", 80).cuda().eval()
    m.head.stride = torch.tensor([8.0, 16.0, 32.0])
    x = torch.randn(4, 3, 256, 256, generator=torch.Generator().manual_seed(3)).cuda()
    dets = ops.postprocess(m(x), 0.25, 0.45)
    rng = np.random.default_rng(1)
    targets = []
    for d in dets:
        k = min(6, d["boxes"].shape[0])
        b = d["boxes"][:k].cpu().numpy() + rng.normal(0, 2, (k, 4)).astype(np.float32)
        targets.append({"boxes": b, "labels": d["labels"][:k].cpu().numpy()})
    preds = [{k: v.cpu().numpy() for k, v in d.items()} for d in dets]
    out, _, _ = _check(preds, targets, torch_preds=dets)
    assert -1.0 <= out["map"].item() <= 1.0
