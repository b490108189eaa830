"""GPU tier of the device-resident COCO evaluator (yms.metrics.CocoEvaluator): the padded-layout
matcher yms_map_match_coco_fixed against yms_map_match_coco and the COCOeval restatement
(tests/cocoeval_ref.py), and the device accumulation yms_map_accumulate_coco_dev cell for cell
(np.array_equal, nothing to tolerate: integer counts and single fp64 divisions) against the host
yms_map_accumulate_coco on the downloaded epoch buffers and against the restatement on the ragged
originals.

Ragged inputs are padded to max_det = the largest count rounded up to a multiple of 8; the padding
rows hold poison (huge boxes, score 2, label 0), which a kernel that read them would turn into wrong
ranks.  The summary tolerance 1e-10 is tests/test_map_coco_gpu.py's (a float64 mean of at most
16 * 101 * 80 cells in [0, 1]).

Written against the kernels' sizes at this commit: the accumulate walks a class' sorted segment in
chunks of 64 rows (ACC_CHUNK), the sort gives each wave a tile of 2048 rows (SORT_TILE), four waves a
workgroup."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cocoeval_ref as C
from yms import _lib as L
from yms.metrics import CocoEvaluator, MeanAveragePrecision

pytestmark = pytest.mark.gpu

TOL = 1e-10
KEYS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large",
        "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")
ACC_CHUNK, SORT_TILE = 64, 2048


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _torch(ds):
    return [{k: _cuda(np.asarray(v)) for k, v in d.items()} for d in ds]


def _max_det(preds):
    return max(8, -(-max([len(p["scores"]) for p in preds] + [1]) // 8) * 8)


def _pad_dets(preds, M):
    """(boxes, scores, labels, counts) device tensors; rows beyond the count are poison"""
    B = len(preds)
    boxes = np.tile(np.array([-1e6, -1e6, 1e6, 1e6], np.float32), (B, M, 1))
    scores = np.full((B, M), 2.0, np.float32)
    labels = np.zeros((B, M), np.int32)
    counts = np.zeros(B, np.int32)
    for i, p in enumerate(preds):
        k = len(p["scores"])
        boxes[i, :k], scores[i, :k], labels[i, :k], counts[i] = p["boxes"], p["scores"], p["labels"], k
    return _cuda(boxes), _cuda(scores), _cuda(labels), _cuda(counts)


def _top(preds, targets):
    return max([int(np.max(l)) + 1 for d in list(preds) + list(targets) for l in [d["labels"]] if len(l)] + [1])


def _run(preds, targets, thresholds=None, batch=None, K=None, **kw):
    """An evaluator fed the ragged data in update() batches of `batch` images."""
    K = K or _top(preds, targets)
    ev = CocoEvaluator(K, thresholds, **kw)
    M = _max_det(preds)
    n = len(preds)
    step = batch or max(n, 1)
    for i in range(0, n, step):
        ev.update(_pad_dets(preds[i:i + step], M), *CocoEvaluator.pad_targets(targets[i:i + step], "cuda"))
    return ev


def _download(ev):
    """The epoch buffers' first n_rows rows as numpy: score, label, rank, matched [4, n], ignored [4, n]"""
    n = ev._n_images * (ev._max_det or 0)
    if not n:
        z = np.zeros(0, np.int32)
        return z.astype(np.float32), z, z, np.zeros((4, 0), np.uint16), np.zeros((4, 0), np.uint16)
    s, l, r, m, g = ev._buf
    c = lambda t: np.ascontiguousarray(t[..., :n].cpu().numpy())
    return c(s), c(l), c(r), c(m).view(np.uint16), c(g).view(np.uint16)


def _bits(mask, T):
    """[4, n] uint16 masks -> [4, T, n] booleans"""
    return ((mask[:, None, :] >> np.arange(T).reshape(1, T, 1)) & 1).astype(bool)


def _live(ev, preds):
    """row index of every live detection, images in order"""
    M = ev._max_det
    return np.concatenate([np.zeros(0, np.int64)] + [i * M + np.arange(len(p["scores"])) for i, p in enumerate(preds)])


def _host_tables(ev):
    """yms_map_accumulate_coco (host, the definition) on the downloaded epoch buffers, image = row // max_det"""
    sc, lb, rk, mt, ig = _download(ev)
    T, K = len(ev.iou_thresholds), ev.num_classes
    im = (np.arange(sc.size) // max(ev._max_det or 1, 1)).astype(np.int32)
    npig = np.ascontiguousarray(ev._npig.cpu().numpy()) if ev._dev is not None else np.zeros((K, 4), np.int32)
    prec = np.zeros((T, 101, K, 4, 3))
    rec = np.zeros((T, K, 4, 3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    assert L.lib().yms_map_accumulate_coco(int(sc.size), p(sc), p(lb), p(im), p(rk), p(mt), p(ig), T, K, p(npig),
                                           p(prec), p(rec)) == 0
    return prec, rec, npig


def _check_match(ev, preds, ref):
    """live rows == the restatement's per-image flags; dead rows are exactly (0, -1, -1, 0 masks)"""
    sc, lb, rk, mt, ig = _download(ev)
    T = len(ev.iou_thresholds)
    live = _live(ev, preds)
    cat = lambda k, ax: np.concatenate([f[k] for f in ref["per_image"]], axis=ax)
    ref_rank = cat(0, 0)
    kept = ref_rank < 100
    assert np.array_equal(rk[live], ref_rank)
    assert np.array_equal(sc[live], np.concatenate([p["scores"] for p in preds]).astype(np.float32))
    assert np.array_equal(lb[live], np.concatenate([p["labels"] for p in preds]).astype(np.int32))
    gm, gi = _bits(mt, T)[:, :, live], _bits(ig, T)[:, :, live]
    assert np.array_equal(gm[:, :, kept], cat(1, 2)[:, :, kept])
    assert np.array_equal(gi[:, :, kept], cat(2, 2)[:, :, kept])
    assert not gm[:, :, ~kept].any()                           # rank >= 100: never matched
    assert not (mt >> T).any() and not (ig >> T).any()
    dead = np.ones(sc.size, bool)
    dead[live] = False
    assert not sc[dead].any() and (lb[dead] == -1).all() and (rk[dead] == -1).all()
    assert not mt[:, dead].any() and not ig[:, dead].any()
    assert np.array_equal(ev._npig.cpu().numpy(), ref["npig"])


def _check_tables(ev, preds, targets, ref=None):
    """device tables == host accumulate on the same buffers == the restatement on the ragged data"""
    precision, recall, npig = ev.tables()
    hp, hr, _ = _host_tables(ev)
    assert precision.dtype == np.float64 and recall.dtype == np.float64
    assert np.array_equal(precision, hp)
    assert np.array_equal(recall, hr)
    ref = ref or C.coco_eval(preds, targets, ev.iou_thresholds)
    assert ref["precision"].shape == precision.shape, "the case must use every class up to num_classes - 1"
    assert np.array_equal(npig, ref["npig"])
    assert np.array_equal(precision, ref["precision"])
    assert np.array_equal(recall, ref["recall"])
    return precision, recall, npig, ref


def _check_summary(out, want):
    for k in KEYS:
        assert out[k].dtype == torch.float64 and out[k].ndim == 0
        assert abs(out[k].item() - float(want[k])) <= TOL, (k, out[k].item(), float(want[k]))
    for k in ("map_per_class", "mar_100_per_class"):
        assert set(out[k]) == set(want[k]), k
        for c, v in want[k].items():
            assert abs(out[k][c] - v) <= TOL, (k, c, out[k][c], v)


@functools.lru_cache(maxsize=None)
def _clustered():
    """the shared input and its restatement, computed once and never written to"""
    preds, targets = C.clustered(np.random.default_rng(11), 24)
    return preds, targets, C.coco_eval(preds, targets)


def _boxes_around(rng, gb, side, n, sigma=0.06):
    src = rng.integers(0, len(gb), n)
    db = (gb[src] + rng.normal(0, sigma, (n, 4)) * np.tile(side[src], 2)).astype(np.float32)
    db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
    return db, src


def _gts(rng, n, lo=10, hi=150):
    side = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    ctr = rng.uniform(100, 500, (n, 2))
    return np.concatenate([ctr - side / 2, ctr + side / 2], 1).astype(np.float32), side


# ------------------------------------------------------------------------------------------
# 1. matcher parity
# ------------------------------------------------------------------------------------------
def test_matcher_parity_clustered():
    preds, targets, ref = _clustered()
    ev = _run(preds, targets, batch=7)                         # 7 + 7 + 7 + 3 images
    _check_match(ev, preds, ref)
    # the input exercises what it is meant to
    assert max(np.bincount(p["labels"]).max() for p in preds if len(p["labels"])) > 100
    sc, lb, rk, mt, ig = _download(ev)
    assert ig[:, _live(ev, preds)].any() and (rk >= 100).any()
    allsc = np.concatenate([p["scores"] for p in preds])
    assert len(np.unique(allsc)) < len(allsc)
    # ... and equals yms_map_match_coco on the same images
    metric = MeanAveragePrecision()
    for i in range(0, len(preds), 7):
        metric.update(_torch(preds[i:i + 7]), _torch(targets[i:i + 7]))
    live = _live(ev, preds)
    assert np.array_equal(rk[live], np.concatenate(metric._rank))
    assert np.array_equal(mt[:, live], np.concatenate(metric._matched, 1))
    assert np.array_equal(ig[:, live], np.concatenate(metric._ignored, 1))


# ------------------------------------------------------------------------------------------
# 2. matcher edges
# ------------------------------------------------------------------------------------------
def test_150_ground_truths_300_detections_one_class():
    """Ground-truth and detection loops stride past 64 (and past 128) lanes; 300 > 100 detections."""
    rng = np.random.default_rng(5)
    gb, side = _gts(rng, 150)
    db, _ = _boxes_around(rng, gb, side, 300)
    preds = [{"boxes": db, "scores": (np.round(rng.random(300) * 64) / 64).astype(np.float32),
              "labels": np.zeros(300, np.int64)}]
    targets = [{"boxes": gb, "labels": np.zeros(150, np.int64)}]
    ev = _run(preds, targets)
    assert ev._max_det == 304
    ref = C.coco_eval(preds, targets)
    _check_match(ev, preds, ref)
    _check_tables(ev, preds, targets, ref)
    assert ref["per_image"][0][1].any()


def test_ground_truths_span_70_classes():
    """More classes in one image than the workgroup has waves, or a wave has lanes."""
    rng = np.random.default_rng(6)
    n = 90
    gl = np.concatenate([np.arange(70), rng.integers(0, 70, n - 70)])
    rng.shuffle(gl)
    gb, side = _gts(rng, n, 10, 200)
    db, src = _boxes_around(rng, gb, side, 200)
    dl = np.where(rng.random(200) < 0.9, gl[src], rng.integers(0, 75, 200))     # some classes without ground truth
    preds = [{"boxes": db, "scores": (np.round(rng.random(200) * 32) / 32).astype(np.float32),
              "labels": dl.astype(np.int64)}]
    targets = [{"boxes": gb, "labels": gl.astype(np.int64)}]
    ev = _run(preds, targets)
    ref = C.coco_eval(preds, targets)
    _check_match(ev, preds, ref)
    _check_tables(ev, preds, targets, ref)
    assert len(ev.compute()["map_per_class"]) == 70


@pytest.mark.parametrize("thresholds", [list(np.linspace(0.2, 0.95, 16)), [0.3]], ids=["T16", "T1"])
def test_threshold_counts(thresholds):
    """T = 16: all 64 (threshold, area) lanes live; T = 1: one lane per area range."""
    preds, targets, _ = _clustered()
    preds, targets = preds[:10], targets[:10]
    ev = _run(preds, targets, thresholds, batch=4)
    ref = C.coco_eval(preds, targets, thresholds)
    _check_match(ev, preds, ref)
    _check_tables(ev, preds, targets, ref)


def test_empty_images_empty_batch_and_no_ground_truth_columns():
    preds, targets, _ = _clustered()
    e4, e1, el = np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    none_d, none_t = {"boxes": e4, "scores": e1, "labels": el}, {"boxes": e4, "labels": el}
    ps = [preds[1], none_d, preds[2], none_d]
    ts = [targets[1], targets[2], none_t, none_t]
    ev = _run(ps, ts, batch=2)                                 # second batch: G = 0
    assert CocoEvaluator.pad_targets(ts[2:], "cuda")[0].shape == (2, 0, 4)
    ref = C.coco_eval(ps, ts)
    _check_match(ev, ps, ref)
    _check_tables(ev, ps, ts, ref)
    # a batch where every count is 0: all rows dead, tables all -1
    ev0 = _run([none_d, none_d], [none_t, none_t], K=3)
    sc, lb, rk, mt, ig = _download(ev0)
    assert sc.size == 16 and not sc.any() and (lb == -1).all() and (rk == -1).all() and not mt.any() and not ig.any()
    precision, recall, npig = ev0.tables()
    assert (precision == -1).all() and (recall == -1).all() and not npig.any()
    out = ev0.compute()
    assert all(out[k].item() == -1 for k in KEYS) and out["map_per_class"] == {} and out["classes"].numel() == 0


def test_counts_above_the_padded_widths_are_clamped():
    preds, targets, _ = _clustered()
    preds, targets = preds[:6], targets[:6]
    M = max(len(p["scores"]) for p in preds)                   # no padding row in the fullest image
    full = int(np.argmax([len(p["scores"]) for p in preds]))
    dets = _pad_dets(preds, M)
    gb, gl, gc = CocoEvaluator.pad_targets(targets, "cuda")
    gfull = int(torch.argmax(gc))
    a = CocoEvaluator(6)
    a.update(dets, gb, gl, gc)
    dc2, gc2 = dets[3].clone(), gc.clone()
    dc2[full] += 1000                                          # the device counts lie: clamped to max_det / G
    gc2[gfull] += 1000
    b = CocoEvaluator(6)
    b.update(dets[:3] + (dc2,), gb, gl, gc2)
    for x, y in zip(_download(a), _download(b)):
        assert np.array_equal(x, y)
    assert np.array_equal(a._npig.cpu().numpy(), b._npig.cpu().numpy())
    ref = C.coco_eval(preds, targets)
    _check_match(b, preds, ref)


def test_more_than_2048_ground_truth_columns_is_unsupported():
    dets = _pad_dets([{"boxes": np.array([[0, 0, 10, 10]], np.float32), "scores": np.ones(1, np.float32),
                       "labels": np.zeros(1, np.int64)}], 8)
    gb = torch.zeros((1, 2049, 4), device="cuda")
    gl = torch.zeros((1, 2049), dtype=torch.int32, device="cuda")
    gc = torch.full((1,), 2049, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"yms_map_match_coco_fixed failed.*status 2"):
        CocoEvaluator(1).update(dets, gb, gl, gc)
    CocoEvaluator(1).update(dets, gb[:, :2048], gl[:, :2048], gc.clamp(max=2048))      # the limit itself runs


# ------------------------------------------------------------------------------------------
# 3. every owned row is written, nothing else
# ------------------------------------------------------------------------------------------
def test_every_owned_row_is_written_and_no_other():
    preds, targets, ref = _clustered()
    preds, targets = preds[:5], targets[:5]
    M, B, K = _max_det(preds), 5, _top(preds, targets)
    row0, cap = M + 3, (B + 2) * M + 7
    db, ds, dl, dc = _pad_dets(preds, M)
    gb, gl, gc = CocoEvaluator.pad_targets(targets, "cuda")
    G = gl.shape[1]
    ff = lambda *shape: torch.full(shape, 0xFF, dtype=torch.uint8, device="cuda")
    score, label, rank = ff(cap * 4), ff(cap * 4), ff(cap * 4)
    matched, ignored = ff(4, cap * 2), ff(4, cap * 2)
    npig = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
    order = torch.empty(B * M, dtype=torch.int32, device="cuda")
    thr = C.IOU_THRS.copy()
    L.call("yms_map_match_coco_fixed", B, M, db.data_ptr(), ds.data_ptr(), dl.data_ptr(), dc.data_ptr(), G,
           gb.data_ptr(), gl.data_ptr(), gc.data_ptr(), 10, thr.ctypes.data_as(ctypes.c_void_p), K, cap, row0,
           score.data_ptr(), label.data_ptr(), rank.data_ptr(), matched.data_ptr(), ignored.data_ptr(),
           npig.data_ptr(), order.data_ptr(), L.stream_ptr(torch.device("cuda")))
    own = np.zeros(cap, bool)
    own[row0:row0 + B * M] = True
    sc, lb, rk = (t.cpu().numpy().view(dt) for t, dt in ((score, np.uint32), (label, np.int32), (rank, np.int32)))
    mt, ig = matched.cpu().numpy().view(np.uint16), ignored.cpu().numpy().view(np.uint16)
    # outside the block: as found
    assert (sc[~own] == 0xFFFFFFFF).all() and (lb[~own] == -1).all() and (rk[~own] == -1).all()
    assert (mt[:, ~own] == 0xFFFF).all() and (ig[:, ~own] == 0xFFFF).all()
    # inside: the evaluator's own rows (checked against the restatement by _check_match), dead rows included
    ev = _run(preds, targets, K=K)
    _check_match(ev, preds, C.coco_eval(preds, targets))
    for got, want in zip((sc.view(np.float32), lb, rk, mt, ig), _download(ev)):
        assert np.array_equal(got[..., own], want)
    dead = np.ones(B * M, bool)
    dead[_live(ev, preds)] = False
    assert dead.any()
    blk = lambda a: a[..., own][..., dead]
    assert (blk(sc) == 0).all() and (blk(lb) == -1).all() and (blk(rk) == -1).all()
    assert not blk(mt).any() and not blk(ig).any()
    assert np.array_equal(npig.cpu().numpy(), ev._npig.cpu().numpy())


# ------------------------------------------------------------------------------------------
# 4. accumulate parity, cell for cell
# ------------------------------------------------------------------------------------------
def test_accumulate_clustered():
    preds, targets, ref = _clustered()
    precision, recall, npig, _ = _check_tables(_run(preds, targets, batch=7), preds, targets, ref)
    assert (precision > 0).any() and (recall > 0).any()


def test_accumulate_empty_and_ignored_classes():
    """class 0: ordinary; class 1: detections, no ground truth (cells -1); class 2: ground truth, no
    detections (recall 0, precision 0); class 3: a large and a small ground truth whose detections are all
    small and miss the large one, so in the 'large' range every detection is ignored (cells 0, not -1)."""
    rng = np.random.default_rng(3)
    gb, side = _gts(rng, 6, 40, 90)
    db, _ = _boxes_around(rng, gb, side, 30)
    small = np.array([[10, 10, 30, 30]], np.float32)                                  # area 400: small
    large = np.array([[300, 300, 500, 500]], np.float32)                              # area 40000: large
    d3 = (small + rng.normal(0, 1.0, (12, 4))).astype(np.float32)
    preds = [{"boxes": np.concatenate([db, rng.uniform(0, 600, (9, 4)).astype(np.float32).cumsum(1), d3]),
              "scores": np.round(rng.random(51) * 16).astype(np.float32) / 16,
              "labels": np.concatenate([np.zeros(30), np.ones(9), np.full(12, 3)]).astype(np.int64)},
             {"boxes": db[:7], "scores": np.linspace(0.9, 0.3, 7).astype(np.float32), "labels": np.zeros(7, np.int64)}]
    targets = [{"boxes": np.concatenate([gb, gb[:2] + 200, small, large]),
                "labels": np.concatenate([np.zeros(6), np.full(2, 2), np.full(2, 3)]).astype(np.int64)},
               {"boxes": gb[:3], "labels": np.zeros(3, np.int64)}]
    ev = _run(preds, targets)
    precision, recall, npig, ref = _check_tables(ev, preds, targets)
    _check_match(ev, preds, ref)
    assert (precision[:, :, 1] == -1).all() and (recall[:, 1] == -1).all()
    assert npig[2, 0] == 2 and (recall[:, 2, 0] == 0).all() and (precision[:, :, 2, 0] == 0).all()
    sc, lb, rk, mt, ig = _download(ev)
    assert npig[3, 3] == 1 and (ig[3, lb == 3] == 0x3FF).all()                        # all ignored in 'large'
    assert (precision[:, :, 3, 3] == 0).all() and (recall[:, 3, 3] == 0).all()
    assert (precision[:, :, 3, 1] > 0).any()                                          # and found in 'small'


def test_accumulate_one_class_across_chunks_and_tiles():
    """40 images x 300 detections of one class, scores quantised to 1/64: the class' sorted segment is the
    40 x 100 kept rows = 62 chunks of ACC_CHUNK = 64 rows and a partial one of 32, the 12160 rows are 5 sort
    tiles of SORT_TILE = 2048 and a partial one (two workgroups), and the 65 score levels tie across images,
    chunks and tiles."""
    rng = np.random.default_rng(8)
    preds, targets = [], []
    for _ in range(40):
        gb, side = _gts(rng, 4, 12, 140)
        db, _ = _boxes_around(rng, gb, side, 300, 0.1)
        preds.append({"boxes": db, "scores": (np.round(rng.random(300) * 64) / 64).astype(np.float32),
                      "labels": np.zeros(300, np.int64)})
        targets.append({"boxes": gb, "labels": np.zeros(4, np.int64)})
    ev = _run(preds, targets, batch=16)
    n_rows = ev._n_images * ev._max_det
    sc, lb, rk, mt, ig = _download(ev)
    seg = int(((rk >= 0) & (rk < 100)).sum())
    assert seg >= 4 * ACC_CHUNK and seg % ACC_CHUNK != 0 and n_rows > 4 * SORT_TILE and n_rows % SORT_TILE != 0
    precision, recall, npig, _ = _check_tables(ev, preds, targets)
    assert 0 < recall[0, 0, 0, 2] <= 1 and len(np.unique(precision[0, :, 0, 0, 2])) > 10


def test_accumulate_no_rows_and_one_class():
    ev = CocoEvaluator(1)
    precision, recall, npig = ev.tables()                      # n_rows = 0, before any update
    hp, hr, _ = _host_tables(ev)
    ref = C.coco_eval([], [])
    assert np.array_equal(precision, hp) and np.array_equal(precision, ref["precision"]) and (precision == -1).all()
    assert np.array_equal(recall, hr) and np.array_equal(recall, ref["recall"])
    rng = np.random.default_rng(2)                             # K = 1 with data
    gb, side = _gts(rng, 5)
    db, _ = _boxes_around(rng, gb, side, 40)
    preds = [{"boxes": db, "scores": rng.random(40).astype(np.float32), "labels": np.zeros(40, np.int64)}]
    targets = [{"boxes": gb, "labels": np.zeros(5, np.int64)}]
    precision, _, _, _ = _check_tables(_run(preds, targets), preds, targets)
    assert precision.shape[2] == 1 and (precision > 0).any()


def test_accumulate_80_classes_mostly_empty():
    preds, targets, _ = _clustered()
    preds, targets = [dict(p) for p in preds[:8]], [dict(t) for t in targets[:8]]
    remap = np.array([0, 17, 18, 41, 63, 79])
    for d in preds + targets:
        d["labels"] = remap[d["labels"]]
    ev = _run(preds, targets, batch=3, K=80)
    precision, recall, npig, _ = _check_tables(ev, preds, targets)
    empty = np.setdiff1d(np.arange(80), remap)
    assert (precision[:, :, empty] == -1).all() and (precision[:, :, 79] > 0).any()
    assert ev.compute()["classes"].tolist() == sorted(set(np.concatenate([d["labels"] for d in preds + targets])))


# ------------------------------------------------------------------------------------------
# 5. end to end against MeanAveragePrecision
# ------------------------------------------------------------------------------------------
def _same_as_metric(ev, metric):
    out, want = ev.compute(), metric.compute()
    _check_summary(out, want)
    assert out["classes"].dtype == want["classes"].dtype and out["classes"].tolist() == want["classes"].tolist()
    for got, ref in zip(ev.tables(), metric.tables()):
        assert np.array_equal(got, ref)
    return out


def test_end_to_end_clustered():
    preds, targets, ref = _clustered()
    ev = _run(preds, targets, batch=7)
    metric = MeanAveragePrecision()
    for i in range(0, len(preds), 7):
        metric.update(_torch(preds[i:i + 7]), _torch(targets[i:i + 7]))
    out = _same_as_metric(ev, metric)
    _check_summary(out, ref["summary"])
    assert out["classes"].tolist() == list(range(6)) and 0.10 <= out["map"].item() <= 0.85


def test_end_to_end_from_detect():
    """detect() on random decoded predictions (A = 336, nc = 6, B = 3, multi_label, max_det 300) straight into
    update(); the list metric gets the same detections through to_list()."""
    from yms import ops
    rng = np.random.default_rng(4)
    B, A, nc = 3, 336, 6
    cxy = rng.uniform(60, 580, (B, A, 2))
    wh = np.exp(rng.uniform(np.log(10), np.log(260), (B, A, 2)))
    cls = rng.random((B, A, nc)) ** 3
    pred = _cuda(np.concatenate([cxy, wh, cls], 2).astype(np.float32))
    det = ops.detect(pred, 0.001, 0.6, multi_label=True, max_det=300)
    assert det.boxes.shape == (B, 300, 4) and not det.boxes.is_contiguous()           # a strided view
    lists = det.to_list()
    targets = []
    for b, d in enumerate(lists):
        pick = rng.choice(len(d["scores"]), 7, replace=False)
        gb = d["boxes"][pick].cpu().numpy() + rng.normal(0, 3, (7, 4)).astype(np.float32)
        gl = d["labels"][pick].cpu().numpy()
        gl[0] = 5 if b == 0 else gl[0]                                                 # the top class has ground truth
        targets.append({"boxes": gb, "labels": gl})
    ev = CocoEvaluator(nc)
    ev.update(det, *CocoEvaluator.pad_targets(targets, "cuda"))
    metric = MeanAveragePrecision()
    metric.update(lists, _torch(targets))
    out = _same_as_metric(ev, metric)
    assert out["map"].item() > 0


# ------------------------------------------------------------------------------------------
# 6. capacity growth and reset, 7. no host read, 8. determinism
# ------------------------------------------------------------------------------------------
def test_capacity_growth_and_reset():
    preds, targets, _ = _clustered()
    preds, targets = preds[:15], targets[:15]
    big = _run(preds, targets, K=6)
    want = big.tables()
    small = _run(preds, targets, batch=3, K=6, capacity_images=2)                      # 2 -> 4 -> 8 -> 16 images
    assert small._cap == 16 * small._max_det and big._cap == 1024 * big._max_det
    for got, ref in zip(small.tables(), want):
        assert np.array_equal(got, ref)
    for x, y in zip(_download(small), _download(big)):
        assert np.array_equal(x, y)
    first = small.compute()
    small.reset()
    assert small._n_images == 0 and not small._npig.any()
    M = small._max_det
    for i in range(0, 15, 3):
        small.update(_pad_dets(preds[i:i + 3], M), *CocoEvaluator.pad_targets(targets[i:i + 3], "cuda"))
    for got, ref in zip(small.tables(), want):
        assert np.array_equal(got, ref)
    again = small.compute()
    assert all(first[k].item() == again[k].item() for k in KEYS) and first["map_per_class"] == again["map_per_class"]
    with pytest.raises(ValueError, match="max_det"):
        small.update(_pad_dets(preds[:2], M + 8), *CocoEvaluator.pad_targets(targets[:2], "cuda"))


def test_update_makes_no_host_synchronisation():
    preds, targets, ref = _clustered()
    M = _max_det(preds)
    batches = [(_pad_dets(preds[i:i + 7], M), CocoEvaluator.pad_targets(targets[i:i + 7], "cuda"))
               for i in range(0, len(preds), 7)]
    strided = torch.zeros((7, M, 6), device="cuda")            # detect()'s own layout: boxes / scores are views
    strided[..., :4], strided[..., 4] = batches[0][0][0], batches[0][0][1]
    batches[0] = ((strided[..., :4], strided[..., 4]) + batches[0][0][2:], batches[0][1])
    ev = CocoEvaluator(6, capacity_images=8)                   # grows twice under the mode
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            batches[0][0][3][0].item()                         # the mode does catch a sync in this build
        for dets, gts in batches:
            ev.update(dets, *gts)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _check_match(ev, preds, ref)
    _check_tables(ev, preds, targets, ref)


def test_accumulate_is_deterministic():
    preds, targets, _ = _clustered()
    ev = _run(preds, targets, batch=7)
    a, b = ev.tables(), ev.tables()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # ... also on a dirty workspace: nothing is read before it is written
    T, K, n = 10, 6, ev._n_images * ev._max_det
    wsb = L.lib().yms_map_accumulate_coco_dev_ws_bytes(n, T, K)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device="cuda")
    precision = torch.full((T, 101, K, 4, 3), 7.0, dtype=torch.float64, device="cuda")
    recall = torch.full((T, K, 4, 3), 7.0, dtype=torch.float64, device="cuda")
    L.call("yms_map_accumulate_coco_dev", n, ev._cap, *[t.data_ptr() for t in ev._buf], T, K, ev._npig.data_ptr(),
           precision.data_ptr(), recall.data_ptr(), ws.data_ptr(), wsb, L.stream_ptr(torch.device("cuda")))
    assert precision.cpu().numpy().tobytes() == a[0].tobytes() and recall.cpu().numpy().tobytes() == a[1].tobytes()
