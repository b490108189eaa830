"""GPU tier of COCO AP with iscrowd and annotation area: the matching entry points
yms_map_match_coco_gt (ragged layout) and yms_map_match_coco_fixed_gt (padded layout) driven directly,
and MeanAveragePrecision / CocoEvaluator on top of them, against the plain restatement
tests/cocoeval_crowd_ref.py (pinned on the CPU by tests/test_map_crowd_cpu.py).  Flags, counts and
tables are compared for equality: they are integers and single float64 divisions of integers.

The padded layout runs at max_det = 300 with G = the batch's largest ground-truth count; rows beyond an
image's counts hold poison (huge boxes, score 2, label 0; crowd 1, area -1) that a kernel reading them
would turn into wrong results, and every output buffer starts as 0xFF bytes.

Written against the kernel's sizes at this commit: a class' ground truths are scored 64 at a time (one per
lane), at most 100 detections per class and image take part."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cocoeval_crowd_ref as R
import cocoeval_ref as C
from yms import _lib as L
from yms.metrics import CocoEvaluator, MeanAveragePrecision

pytestmark = pytest.mark.gpu

KEYS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large",
        "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")
MAX_DET = 300
T16 = tuple(np.linspace(0.2, 0.95, 16))
T1 = (0.3,)


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _torch(ds):
    return [{k: _cuda(np.asarray(v)) for k, v in d.items()} for d in ds]


def _thr(thresholds):
    return C.IOU_THRS.copy() if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)


def _strip(targets, *keys):
    return [{k: v for k, v in t.items() if k not in keys} for t in targets]


def _cat(xs, dt, shape=(0,)):
    return np.ascontiguousarray(np.concatenate([np.zeros(shape, dt)] + [np.asarray(x).astype(dt) for x in xs]))


def _bits(mask, T):
    """[4, n] uint16 masks -> [4, T, n] booleans"""
    return ((mask[:, None, :] >> np.arange(T).reshape(1, T, 1)) & 1).astype(bool)


def _stream():
    return L.stream_ptr(torch.device("cuda"))


def _ragged(preds, targets, thresholds=None, crowd=True, area=True, entry="yms_map_match_coco_gt"):
    """The ragged entry point on the whole batch -> rank [n], matched / ignored [4, n] uint16, gt_ignore [g]"""
    thr = _thr(thresholds)
    nd, ng = [len(p["scores"]) for p in preds], [len(t["labels"]) for t in targets]
    n, g = sum(nd), sum(ng)
    db = _cuda(_cat([p["boxes"] for p in preds], np.float32, (0, 4)))
    ds, dl = _cuda(_cat([p["scores"] for p in preds], np.float32)), _cuda(_cat([p["labels"] for p in preds], np.int32))
    gb = _cuda(_cat([t["boxes"] for t in targets], np.float32, (0, 4)))
    gl = _cuda(_cat([t["labels"] for t in targets], np.int32))
    gcr = _cuda(_cat([t["iscrowd"] for t in targets], np.uint8)) if crowd else None
    gar = _cuda(_cat([t["area"] for t in targets], np.float32)) if area else None
    doff = _cuda(np.concatenate([[0], np.cumsum(nd)]).astype(np.int32))
    goff = _cuda(np.concatenate([[0], np.cumsum(ng)]).astype(np.int32))
    D, G = max(n, 1), max(g, 1)
    matched = torch.full((4, D), -1, dtype=torch.int16, device="cuda")
    ignored = torch.full((4, D), -1, dtype=torch.int16, device="cuda")
    gign = torch.full((G,), 0xFF, dtype=torch.uint8, device="cuda")
    rank = torch.full((2 * D,), -1, dtype=torch.int32, device="cuda")
    p = lambda t, k: t.data_ptr() if t is not None and k else None
    args = [len(preds), n, p(db, n), p(ds, n), p(dl, n), doff.data_ptr(), p(gb, g), p(gl, g), goff.data_ptr(),
            int(thr.size), thr.ctypes.data_as(ctypes.c_void_p), matched.data_ptr(), ignored.data_ptr(), gign.data_ptr(),
            rank.data_ptr(), max(ng + [0])]
    if entry.endswith("_gt"):
        args += [p(gcr, g), p(gar, g)]
    L.call(entry, *args, _stream())
    return (rank[:n].cpu().numpy(), matched[:, :n].cpu().numpy().view(np.uint16),
            ignored[:, :n].cpu().numpy().view(np.uint16), gign[:g].cpu().numpy())


def _pad_dets(preds, M=MAX_DET):
    """(boxes, scores, labels, counts) device tensors; rows beyond the count are poison"""
    B = len(preds)
    boxes = np.tile(np.array([-1e6, -1e6, 1e6, 1e6], np.float32), (B, M, 1))
    scores, labels, counts = np.full((B, M), 2.0, np.float32), np.zeros((B, M), np.int32), np.zeros(B, np.int32)
    for i, p in enumerate(preds):
        k = len(p["scores"])
        boxes[i, :k], scores[i, :k], labels[i, :k], counts[i] = p["boxes"], p["scores"], p["labels"], k
    return _cuda(boxes), _cuda(scores), _cuda(labels), _cuda(counts)


def _pad_gts(targets, crowd=True, area=True):
    """padded device ground truths; slots beyond the count are poison (a crowd of area -1 around everything)"""
    B = len(targets)
    G = max([len(t["labels"]) for t in targets] + [0])
    boxes = np.tile(np.array([-1e6, -1e6, 1e6, 1e6], np.float32), (B, G, 1))
    labels, counts = np.zeros((B, G), np.int32), np.zeros(B, np.int32)
    cr, ar = np.ones((B, G), np.uint8), np.full((B, G), -1.0, np.float32)
    for i, t in enumerate(targets):
        k = len(t["labels"])
        boxes[i, :k], labels[i, :k], counts[i] = t["boxes"], t["labels"], k
        if crowd:
            cr[i, :k] = t["iscrowd"]
        if area:
            ar[i, :k] = t["area"]
    return _cuda(boxes), _cuda(labels), _cuda(counts), (_cuda(cr) if crowd else None), (_cuda(ar) if area else None)


def _fixed(preds, targets, K, thresholds=None, crowd=True, area=True, entry="yms_map_match_coco_fixed_gt"):
    """The padded entry point -> the call's own rows of score, label, rank, matched / ignored [4, B * M], npig
    [K, 4], and the bytes of everything it was given to write into."""
    thr = _thr(thresholds)
    B, M = len(preds), MAX_DET
    db, ds, dl, dc = _pad_dets(preds)
    gb, gl, gc, gcr, gar = _pad_gts(targets, crowd, area)
    G = int(gl.shape[1])
    row0, cap = 8, B * M + 24
    ff = lambda *shape: torch.full(shape, 0xFF, dtype=torch.uint8, device="cuda")
    score, label, rank, matched, ignored = ff(cap * 4), ff(cap * 4), ff(cap * 4), ff(4, cap * 2), ff(4, cap * 2)
    npig = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
    order = torch.empty(max(B * M, 1), dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr() if t is not None and G else None
    args = [B, M, db.data_ptr(), ds.data_ptr(), dl.data_ptr(), dc.data_ptr(), G, p(gb), p(gl), gc.data_ptr(),
            int(thr.size), thr.ctypes.data_as(ctypes.c_void_p), K, cap, row0, score.data_ptr(), label.data_ptr(),
            rank.data_ptr(), matched.data_ptr(), ignored.data_ptr(), npig.data_ptr(), order.data_ptr()]
    if entry.endswith("_gt"):
        args += [p(gcr), p(gar)]
    L.call(entry, *args, _stream())
    raw = [t.cpu().numpy() for t in (score, label, rank, matched, ignored, npig)]
    own = slice(row0, row0 + B * M)
    sc, lb, rk = raw[0].view(np.float32), raw[1].view(np.int32), raw[2].view(np.int32)
    mt, ig = raw[3].view(np.uint16), raw[4].view(np.uint16)
    outside = np.ones(cap, bool)
    outside[own] = False
    assert (lb[outside] == -1).all() and (rk[outside] == -1).all() and (mt[:, outside] == 0xFFFF).all() \
        and (ig[:, outside] == 0xFFFF).all() and (raw[0].reshape(cap, 4)[outside] == 0xFF).all()      # as found
    return (sc[own], lb[own], rk[own], mt[:, own], ig[:, own], raw[5]), raw


def _ref_cat(ref):
    cat = lambda k, ax, z: np.concatenate([z] + [f[k] for f in ref["per_image"]], axis=ax)
    T = ref["precision"].shape[0]
    return (cat(0, 0, np.zeros(0, np.int64)), cat(1, 2, np.zeros((4, T, 0), bool)), cat(2, 2, np.zeros((4, T, 0), bool)),
            cat(3, 1, np.zeros((4, 0), bool)))


def _check_flags(rank, mt, ig, ref, T):
    """kernel rank / masks of the live detections == the restatement's, every (area, threshold, detection)"""
    ref_rank, ref_m, ref_i, _ = _ref_cat(ref)
    kept = ref_rank < 100
    assert np.array_equal(rank, ref_rank)
    gm, gi = _bits(mt, T), _bits(ig, T)
    assert gm.shape == ref_m.shape
    assert np.array_equal(gm[:, :, kept], ref_m[:, :, kept])
    assert np.array_equal(gi[:, :, kept], ref_i[:, :, kept])
    assert not gm[:, :, ~kept].any()                            # beyond the 100 kept: never matched
    assert not (mt >> T).any() and not (ig >> T).any()          # no bit above the T thresholds


def _both(preds, targets, thresholds=None, crowd=True, area=True, ref=None):
    """Both layouts on one batch against the restatement (which sees exactly the fields the kernel is given)."""
    seen = _strip(targets, *([] if crowd else ["iscrowd"]), *([] if area else ["area"]))
    ref = ref or R.coco_eval(preds, seen, None if thresholds is None else list(thresholds))
    T = len(_thr(thresholds))
    # ragged
    rank, mt, ig, gign = _ragged(preds, targets, thresholds, crowd, area)
    _check_flags(rank, mt, ig, ref, T)
    ref_g = _ref_cat(ref)[3]
    assert np.array_equal(((gign[None, :] >> np.arange(4).reshape(4, 1)) & 1).astype(bool), ref_g)
    assert not (gign >> 4).any()                                # a crowd is reported as the four range bits only
    # padded
    K = ref["npig"].shape[0]
    (sc, lb, rk, fmt, fig, npig), _ = _fixed(preds, targets, K, thresholds, crowd, area)
    live = np.concatenate([np.zeros(0, np.int64)] + [i * MAX_DET + np.arange(len(p["scores"])) for i, p in enumerate(preds)])
    _check_flags(rk[live], fmt[:, live], fig[:, live], ref, T)
    assert np.array_equal(sc[live], _cat([p["scores"] for p in preds], np.float32))
    assert np.array_equal(lb[live], _cat([p["labels"] for p in preds], np.int32))
    dead = np.ones(sc.size, bool)
    dead[live] = False
    assert not sc[dead].any() and (lb[dead] == -1).all() and (rk[dead] == -1).all()
    assert not fmt[:, dead].any() and not fig[:, dead].any()
    assert np.array_equal(npig, ref["npig"])
    # the two layouts agree with each other on every live row
    assert np.array_equal(fmt[:, live][:, rank < 100], mt[:, rank < 100])
    return ref


@functools.lru_cache(maxsize=None)
def _case(seed, thresholds=None):
    """clustered_crowd at 8 images and its restatement, computed once and never written to"""
    preds, targets = R.clustered_crowd(np.random.default_rng(seed), 8)
    return preds, targets, R.coco_eval(preds, targets, None if thresholds is None else list(thresholds))


def _gts(rng, n, lo=10, hi=150):
    side = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    ctr = rng.uniform(100, 500, (n, 2))
    return np.concatenate([ctr - side / 2, ctr + side / 2], 1).astype(np.float32), side


def _boxes_around(rng, gb, side, n, sigma=0.06):
    src = rng.integers(0, len(gb), n)
    db = (gb[src] + rng.normal(0, sigma, (n, 4)) * np.tile(side[src], 2)).astype(np.float32)
    db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
    return db


def _wh_area(gb, u=1.0):
    return ((gb[:, 2] - gb[:, 0]).astype(np.float64) * (gb[:, 3] - gb[:, 1]).astype(np.float64) * u).astype(np.float32)


def _target(gb, labels, crowd, area):
    return {"boxes": np.asarray(gb, np.float32).reshape(-1, 4), "labels": np.asarray(labels, np.int64),
            "iscrowd": np.asarray(crowd, np.uint8), "area": np.asarray(area, np.float32)}


def _pred(db, scores, labels):
    return {"boxes": np.asarray(db, np.float32).reshape(-1, 4), "scores": np.asarray(scores, np.float32),
            "labels": np.asarray(labels, np.int64)}


def _check_summary(out, want):
    """the twelve numbers and map_per_class, for equality; every figure is printed before anything is asserted"""
    assert set(out["map_per_class"]) == set(want["map_per_class"])
    rows = [(k, out[k].item(), float(want[k])) for k in KEYS]
    rows += [(f"map_per_class[{c}]", out["map_per_class"][c], float(v)) for c, v in want["map_per_class"].items()]
    for k, got, ref in rows:
        print(f"{k:20s} {got!r:24} {ref!r:24} diff {got - ref:.3g}")
    for k in KEYS:
        assert out[k].dtype == torch.float64 and out[k].ndim == 0
    assert [r for r in rows if r[1] != r[2]] == []


# ------------------------------------------------------------------------------------------
# 1. both layouts on the clustered input, T = 10 / 1 / 16
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,thresholds", [(21, None), (21, T1), (21, T16), (22, T1), (23, T16)],
                         ids=["T10", "T1", "T16", "seed22-T1", "seed23-T16"])
def test_flags_both_layouts(seed, thresholds):
    preds, targets, ref = _case(seed, thresholds)
    _both(preds, targets, thresholds, ref=ref)
    _, ref_m, ref_i, ref_g = _ref_cat(ref)
    crowd = np.concatenate([t["iscrowd"] for t in targets]).astype(bool)
    assert crowd.any() and ref_g[:, crowd].all() and (ref_m & ref_i).any() and (ref_m & ~ref_i).any()


# ------------------------------------------------------------------------------------------
# 2. tables and summary through the two metric classes
# ------------------------------------------------------------------------------------------
def _run_metric(preds, targets, thresholds=None, batch=3):
    metric = MeanAveragePrecision() if thresholds is None else MeanAveragePrecision(iou_thresholds=list(thresholds))
    for i in range(0, len(preds), batch):
        metric.update(_torch(preds[i:i + batch]), _torch(targets[i:i + batch]))
    return metric


def _run_evaluator(preds, targets, K, thresholds=None, batch=3, crowd=True, area=True):
    ev = CocoEvaluator(K, None if thresholds is None else list(thresholds), capacity_images=4)
    for i in range(0, len(preds), batch):
        gb, gl, gc, cr, ar = CocoEvaluator.pad_targets(targets[i:i + batch], "cuda", flags=True)
        ev.update(_pad_dets(preds[i:i + batch]), gb, gl, gc, gt_crowd=cr if crowd else None, gt_area=ar if area else None)
    return ev


@functools.lru_cache(maxsize=None)
def _both_metrics():
    preds, targets, ref = _case(21)
    return _run_metric(preds, targets), _run_evaluator(preds, targets, ref["npig"].shape[0])


def test_tables_and_list_summary():
    preds, targets, ref = _case(21)
    metric, ev = _both_metrics()
    for tables in (metric.tables(), ev.tables()):
        precision, recall, npig = tables
        assert np.array_equal(npig, ref["npig"])
        assert np.array_equal(precision, ref["precision"]) and np.array_equal(recall, ref["recall"])
    assert (ref["precision"] > 0).any() and (ref["npig"].max(0) > 0).all()
    out_m, out_e = metric.compute(), ev.compute()
    _check_summary(out_m, ref["summary"])
    # crowd ground truths count as present: torchmetrics lists their classes too
    seen = set(np.concatenate([t["labels"] for t in targets]).tolist())
    assert seen <= set(out_m["classes"].tolist()) and out_e["classes"].tolist() == out_m["classes"].tolist()
    assert set(out_e["map_per_class"]) == set(out_m["map_per_class"])


def test_device_summary_is_identical():
    """CocoEvaluator.compute()'s twelve numbers and map_per_class == the restatement's == MeanAveragePrecision's,
    for equality as the tables above are: an epoch that was given gt_crowd / gt_area averages the tables on the
    host in numpy's order of summation (one without them keeps the device reduction it always had)."""
    _, _, ref = _case(21)
    metric, ev = _both_metrics()
    out_m, out_e = metric.compute(), ev.compute()
    _check_summary(out_e, ref["summary"])
    _check_summary(out_e, {k: (v.item() if k in KEYS else v) for k, v in out_m.items()})


def test_mixed_targets_get_the_defaults():
    """only some targets of a batch carry the keys: the others are not crowd and w*h"""
    preds, targets, _ = _case(21)
    preds = preds[:4]
    targets = [targets[0], _strip(targets[1:2], "iscrowd", "area")[0], _strip(targets[2:3], "area")[0],
               _strip(targets[3:4], "iscrowd")[0]]
    ref = R.coco_eval(preds, targets)
    K = ref["npig"].shape[0]
    metric, ev = _run_metric(preds, targets, batch=4), _run_evaluator(preds, targets, K, batch=4)
    for precision, recall, npig in (metric.tables(), ev.tables()):
        assert np.array_equal(npig, ref["npig"])
        assert np.array_equal(precision, ref["precision"]) and np.array_equal(recall, ref["recall"])


def test_default_area_of_a_box_on_a_range_border():
    """A target without 'area' beside one with it: its default must fall where the double w*h falls.  The box's
    w*h is 1024 + 2^-14 - 2^-37 in double (medium only) and rounds to 1024.0 in fp32 (small and medium)."""
    two = np.float32(2.0)
    edge = np.array([[0, 0, np.float32(32) + two ** -18, np.float32(32) - two ** -19]], np.float32)
    assert float(edge[0, 2]) * float(edge[0, 3]) > 1024.0 and np.float32(float(edge[0, 2]) * float(edge[0, 3])) == 1024.0
    preds = [_pred([[100, 100, 140, 140]], [0.9], [0]), _pred(edge, [0.8], [0])]
    targets = [_target([[100, 100, 140, 140]], [0], [0], [900.0]), {"boxes": edge, "labels": np.zeros(1, np.int64)}]
    ref = R.coco_eval(preds, targets)
    assert ref["npig"].tolist() == [[2, 1, 1, 0]]             # the 900 px^2 one is the only small one
    metric, ev = _run_metric(preds, targets), _run_evaluator(preds, targets, 1)
    for precision, recall, npig in (metric.tables(), ev.tables()):
        assert np.array_equal(npig, ref["npig"])
        assert np.array_equal(precision, ref["precision"]) and np.array_equal(recall, ref["recall"])


# ------------------------------------------------------------------------------------------
# 3. edges
# ------------------------------------------------------------------------------------------
def test_70_ground_truths_of_one_class_crowds_at_the_chunk_border():
    """One class spans two 64-lane chunks; crowds at indices 0, 63, 64 and 69."""
    rng = np.random.default_rng(31)
    gb, side = _gts(rng, 70)
    crowd = np.zeros(70, np.uint8)
    crowd[[0, 63, 64, 69]] = 1
    db = np.concatenate([_boxes_around(rng, gb, side, 170), _boxes_around(rng, gb[[0, 63, 64, 69]], side[[0, 63, 64, 69]], 60)])
    preds = [_pred(db, np.round(rng.random(230) * 32) / 32, np.zeros(230))]
    targets = [_target(gb, np.zeros(70), crowd, _wh_area(gb, rng.uniform(0.3, 1.0, 70)))]
    ref = _both(preds, targets)
    rank, m, i, _ = ref["per_image"][0]
    assert (m[0, 0] & i[0, 0]).sum() >= 4 and (m[0, 0] & ~i[0, 0]).any() and (rank >= 100).any()


def test_all_ground_truths_crowd():
    rng = np.random.default_rng(32)
    gb, side = _gts(rng, 5, 60, 200)
    preds = [_pred(_boxes_around(rng, gb, side, 40, 0.15), rng.random(40), rng.integers(0, 2, 40))]
    targets = [_target(gb, [0, 1, 0, 1, 1], np.ones(5), _wh_area(gb))]
    ref = _both(preds, targets)
    assert not ref["npig"].any() and (ref["precision"] == -1).all()
    _, m, i, _ = ref["per_image"][0]
    assert m.any() and not (m & ~i).any() and (~m[0, 0]).any()   # matched ones are all ignored; some match nothing


def test_no_detections_and_no_ground_truths():
    preds, targets, _ = _case(21)
    full = max(range(8), key=lambda k: len(targets[k]["labels"]) * bool(targets[k]["iscrowd"].any()))
    assert targets[full]["iscrowd"].any()
    e4, e1 = np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
    none_d, none_t = _pred(e4, e1, e1), _target(e4, e1, e1, e1)
    _both([none_d, preds[full], none_d], [targets[full], none_t, none_t])
    _both([none_d], [targets[full]])                          # no detection in the whole batch
    _both([preds[full]], [none_t])                            # no ground-truth column at all: G = 0


def test_130_detections_over_one_crowd():
    """The 100 cap meets repeated matching: 100 detections match the one crowd, 30 are not evaluated."""
    rng = np.random.default_rng(33)
    xy = rng.uniform(0, 360, (130, 2))
    wh = rng.uniform(5, 40, (130, 2))
    db = np.concatenate([xy, xy + wh], 1)
    preds = [_pred(db, np.round(rng.random(130) * 16) / 16, np.zeros(130))]              # exact score ties
    targets = [_target([[0, 0, 400, 400]], [0], [1], [160000])]
    ref = _both(preds, targets)
    rank, m, i, _ = ref["per_image"][0]
    assert m[:, :, rank < 100].all() and i[:, :, rank < 100].all() and not m[:, :, rank >= 100].any()
    assert not ref["npig"].any()


@pytest.mark.parametrize("crowd,area", [(False, True), (True, False)], ids=["area_only", "crowd_only"])
def test_one_field_without_the_other(crowd, area):
    preds, targets, full = _case(21)
    ref = _both(preds[:5], targets[:5], crowd=crowd, area=area)
    both = R.coco_eval(preds[:5], targets[:5])
    assert not np.array_equal(ref["npig"], both["npig"])       # the missing field does matter on this input


def test_areas_on_the_range_borders():
    """1024.0 and 9216.0 belong to both ranges they bound; one fp32 step off they do not."""
    f = np.float32
    area = np.array([1024, np.nextafter(f(1024), f(0)), np.nextafter(f(1024), f(1e9)), 9216,
                     np.nextafter(f(9216), f(0)), np.nextafter(f(9216), f(1e9)), 0, -1, 1e10, 2e10, np.nan], np.float32)
    n = len(area)
    gb = np.array([[50 * k, 10, 50 * k + 40, 50] for k in range(n)], np.float32)         # 40 x 40 boxes side by side
    preds = [_pred(gb + 1, np.linspace(0.9, 0.1, n), np.zeros(n))]
    targets = [_target(gb, np.zeros(n), np.zeros(n), area)]
    ref = _both(preds, targets)
    g = ref["per_image"][0][3].T.tolist()
    assert g[0] == [False, False, False, True] and g[1] == [False, False, True, True] and g[2] == [False, True, False, True]
    assert g[3] == [False, True, False, False] and g[4] == [False, True, False, True] and g[5] == [False, True, True, False]
    assert g[6] == [False, False, True, True] and g[7] == [True] * 4 and g[8] == [False, True, True, False]
    assert g[9] == [True, True, True, True] and g[10] == [False] * 4
    assert ref["npig"].tolist() == [[9, 4, 5, 4]]


@pytest.mark.parametrize("crowd_first", [False, True])
def test_iou_tie_between_crowd_and_area_ignored_takes_the_later(crowd_first):
    """Detections 1 and 2 (equal scores) have IoU 0.8 exactly with an area-ignored ground truth R (1600 / 2000)
    and with a crowd C (1280 / 1600).  In the 'medium' range both are ignore, so the later index wins.
    R first: both take C and R stays free for detection 3, which reaches only R above 0.55.
    C first: detection 1 uses R up, detection 2 falls back to C, detection 3 finds nothing: a false positive."""
    R_box, C_box = [100, 100, 140, 150], [100, 100, 140, 132]
    d12, d3 = [100, 100, 140, 140], [100, 110, 140, 150]
    assert 1280.0 / 1600.0 == 1600.0 / 2000.0
    gts, crowd, area = ([C_box, R_box], [1, 0], [1280, 900]) if crowd_first else ([R_box, C_box], [0, 1], [900, 1280])
    preds = [_pred([d12, d12, d3], [0.9, 0.9, 0.5], [0, 0, 0])]
    targets = [_target(gts, [0, 0], crowd, area)]
    ref = _both(preds, targets)
    _, m, i, _ = ref["per_image"][0]
    at = [k for k, t in enumerate(C.IOU_THRS) if 0.58 < t < 0.78]                         # 0.6, 0.65, 0.7, 0.75
    assert len(at) == 4
    assert m[2][at][:, :2].all() and i[2][at][:, :2].all()                                # 1 and 2: matched, ignored
    assert m[2][at][:, 2].tolist() == [not crowd_first] * 4
    assert i[2][at][:, 2].tolist() == [not crowd_first] * 4                               # unmatched and medium itself: an FP


# ------------------------------------------------------------------------------------------
# 4. unchanged behaviour
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain():
    preds, targets = C.clustered(np.random.default_rng(11), 8)
    preds = [{k: v[:MAX_DET] for k, v in p.items()} for p in preds]
    return preds, targets, C.coco_eval(preds, targets)


def test_null_pointers_are_the_old_entry_points_byte_for_byte():
    preds, targets, ref = _plain()
    for thresholds in (None, T16):
        old = _ragged(preds, targets, thresholds, False, False, entry="yms_map_match_coco")
        new = _ragged(preds, targets, thresholds, False, False)
        for x, y in zip(old, new):
            assert x.tobytes() == y.tobytes()
        _, raw_old = _fixed(preds, targets, 6, thresholds, False, False, entry="yms_map_match_coco_fixed")
        _, raw_new = _fixed(preds, targets, 6, thresholds, False, False)
        for x, y in zip(raw_old, raw_new):
            assert x.tobytes() == y.tobytes()
    _check_flags(*_ragged(preds, targets, None, False, False)[:3], ref, 10)


def test_targets_without_the_keys_match_cocoeval_ref():
    preds, targets, ref = _plain()
    metric = _run_metric(preds, targets)
    ev = CocoEvaluator(6)
    for i in range(0, 8, 3):
        ev.update(_pad_dets(preds[i:i + 3]), *CocoEvaluator.pad_targets(targets[i:i + 3], "cuda"))
    for precision, recall, npig in (metric.tables(), ev.tables()):
        assert np.array_equal(npig, ref["npig"])
        assert np.array_equal(precision, ref["precision"]) and np.array_equal(recall, ref["recall"])
    _check_summary(metric.compute(), ref["summary"])


# ------------------------------------------------------------------------------------------
# 5. API contract
# ------------------------------------------------------------------------------------------
def test_reference_mode_refuses_crowd_and_ignores_area():
    preds, targets, _ = _case(21)
    preds, targets = preds[:3], targets[:3]
    assert any(t["iscrowd"].any() for t in targets)
    with pytest.raises(ValueError, match="COCO mode"):
        MeanAveragePrecision(iou_thresholds=[0.5]).update(_torch(preds), _torch(targets))
    no_crowd = [dict(t, iscrowd=np.zeros_like(t["iscrowd"])) for t in targets]           # zeros are accepted
    with_area, without = MeanAveragePrecision(iou_thresholds=[0.5]), MeanAveragePrecision(iou_thresholds=[0.5])
    with_area.update(_torch(preds), _torch(no_crowd))
    without.update(_torch(preds), _torch(_strip(targets, "iscrowd", "area")))
    a, b = with_area.compute(), without.compute()
    assert a["map_50"].item() == b["map_50"].item() and a["map_per_class"] == b["map_per_class"] and b["map_50"].item() > 0
    with pytest.raises(ValueError, match="gt_crowd"):
        gb, gl, gc, cr, ar = CocoEvaluator.pad_targets(targets, "cuda", flags=True)
        CocoEvaluator(6).update(_pad_dets(preds), gb, gl, gc, gt_crowd=cr[:, :1])
    with pytest.raises(ValueError, match="iscrowd"):
        MeanAveragePrecision().update(_torch(preds), _torch([dict(t, iscrowd=np.zeros(1, np.uint8)) for t in targets]))


# ------------------------------------------------------------------------------------------
# 6. end to end from detect()
# ------------------------------------------------------------------------------------------
def test_end_to_end_from_detect_with_crowd_flags():
    from yms import ops
    from yms.metrics import coco_results
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    nc = 3
    model = YOLOv8("n", nc).cuda().eval()
    model.head.stride = torch.tensor([8.0, 16.0, 32.0])
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        pred = model(x)
    det = ops.detect(pred, 0.0, 0.7, multi_label=True, max_det=300)
    lists = det.to_list()                                     # detect's own output read back
    preds = [{k: v.cpu().numpy() for k, v in d.items()} for d in lists]
    assert min(len(p["scores"]) for p in preds) >= 6
    rng = np.random.default_rng(7)
    targets = []
    for b, p in enumerate(preds):
        pick = rng.choice(len(p["scores"]), 6, replace=False)
        gb = p["boxes"][pick] + rng.normal(0, 0.5, (6, 4)).astype(np.float32)
        gl = p["labels"][pick].copy()
        gl[1] = 2                                             # the top class has ground truth: K = 3
        gl[0] = np.bincount(p["labels"]).argmax()             # a crowd around every detection of the commonest class
        of = p["boxes"][p["labels"] == gl[0]]
        gb[0] = [of[:, 0].min(), of[:, 1].min(), of[:, 2].max(), of[:, 3].max()]
        targets.append(_target(gb, gl, [1, 0, 0, 0, 0, 0], _wh_area(gb, rng.uniform(0.3, 1.0, 6))))
    ev = CocoEvaluator(nc)
    gb, gl, gc, cr, ar = CocoEvaluator.pad_targets(targets, "cuda", flags=True)
    ev.update(det, gb, gl, gc, gt_crowd=cr, gt_area=ar)       # Detections straight in
    ref = R.coco_eval(preds, targets)
    precision, recall, npig = ev.tables()
    assert np.array_equal(npig, ref["npig"])
    assert np.array_equal(precision, ref["precision"]) and np.array_equal(recall, ref["recall"])
    assert any((m & i)[0].any() for _, m, i, _ in ref["per_image"])                       # something did land in the crowd
    res = coco_results(det, [11, 12], {0: 1, 1: 2, 2: 3})     # and the same detections as COCO result dicts
    assert len(res) == sum(len(p["scores"]) for p in preds)
    assert [r["score"] for r in res] == [float(s) for p in preds for s in p["scores"]]
    assert {r["image_id"] for r in res} == {11, 12} and {r["category_id"] for r in res} <= {1, 2, 3}
