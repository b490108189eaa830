"""yms.ops.detect and its kernels (csrc/detect.hip) against the numpy restatement (tests/detect_ref.py),
bit for bit; yms.data.letterbox_normalize against tests/mosaic_ref.py; and the validation-loop
recipe end to end at toy size.

The input (``make_pred``): n = 4 images, A = 2100 anchors (a 320 x 320 input), every score on a 1/64
grid so that ties abound, conf = 0.25.  Image 0 is dense (uniform [0, 0.5) everywhere plus 12
clusters of 25 jittered boxes sharing a class with scores in [0.5, 1)); image 1 has nothing above
conf and one score exactly equal to it; image 2 has exactly K candidates; image 3 has 150
candidates, one NaN score and one score of exactly 1.0.  With seed 0 and (nc, K) = (80, 512) image 0
has 78951 candidates and the cap admits 212 of the 5332 at the threshold score; ``test_coverage``
asserts, on the restatement's output, every fact the cases below rely on, so a changed generator
cannot pass vacuously."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import detect_ref as R
import mosaic_ref as MR
from yms import _lib as L
from yms import data as D
from yms import ops

pytestmark = pytest.mark.gpu
F32 = np.float32
N, A, CONF, IOU, SEED = 4, 2100, 0.25, 0.45, 0
LB_FRAME = D.Letterbox(120, 200, 320, 320).frame      # r = 1.6, left 0, top 64


@functools.lru_cache(maxsize=None)
def make_pred(nc, K):
    rng = np.random.default_rng(SEED)
    p = np.zeros((N, A, 4 + nc), F32)
    p[..., :2] = rng.uniform(0, 320, (N, A, 2))
    p[..., 2:4] = rng.uniform(8, 80, (N, A, 2))
    # image 0: dense + clusters
    p[0, :, 4:] = rng.integers(0, 32, (A, nc)) / 64
    for a0 in rng.permutation(A)[:300].reshape(12, 25):
        cx, cy = rng.uniform(20, 300, 2)
        w, h = rng.uniform(20, 120, 2)
        c = rng.integers(0, nc)
        p[0, a0, 0] = cx + rng.uniform(-3, 3, 25)
        p[0, a0, 1] = cy + rng.uniform(-3, 3, 25)
        p[0, a0, 2] = w + rng.uniform(-3, 3, 25)
        p[0, a0, 3] = h + rng.uniform(-3, 3, 25)
        p[0, a0, 4 + c] = rng.integers(32, 64, 25) / 64
    # image 1: nothing above conf, one score equal to it
    p[1, :, 4:] = rng.integers(0, 16, (A, nc)) / 64
    p[1, 1234, 4 + nc // 2] = CONF
    # images 2 and 3: K resp. 150 candidates at distinct pairs on a floor at or below conf
    for b, m in ((2, K), (3, 150)):
        p[b, :, 4:] = rng.integers(0, 17, (A, nc)) / 64
        flat = rng.permutation(A * nc)[:m + 2]
        s = p[b, :, 4:].reshape(-1)
        s[flat[:m]] = rng.integers(17, 64, m) / 64
        if b == 3:
            s[flat[m]] = 1.0
            s[flat[m + 1]] = np.nan
        p[b, :, 4:] = s.reshape(A, nc)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref(nc, K, max_det, multi, agnostic, classes=None, frames=False):
    out = R.detect(make_pred(nc, K), CONF, IOU, multi, agnostic, classes, max_det, K,
                   [LB_FRAME] * N if frames else None)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def run(nc, K, max_det, multi, agnostic, classes=None, frames=False, pred=None):
    d = torch.tensor(make_pred(nc, K) if pred is None else pred).cuda()
    fr = torch.tensor([LB_FRAME] * d.shape[0], dtype=torch.float32).cuda() if frames else None
    return ops.detect(d, CONF, IOU, multi_label=multi, agnostic=agnostic, classes=classes, max_det=max_det,
                      max_nms=K, frames=fr)


def check(det, want):
    assert np.array_equal(det.counts.cpu().numpy(), want["count"])
    assert np.array_equal(det.candidates.cpu().numpy(), want["candidates"])
    assert np.array_equal(det.anchors.cpu().numpy(), want["anchor"])
    assert np.array_equal(det.labels.cpu().numpy(), want["det"][..., 5].astype(np.int32))
    assert np.array_equal(det.scores.cpu().numpy(), want["det"][..., 4])
    assert np.array_equal(det.boxes.cpu().numpy(), want["det"][..., :4])


def cut_in_tie(want, b):
    """max_det cut image b's kept rows between two equal scores."""
    m = want["count"][b]
    return want["kept"][b] > m and want["det"][b, m - 1, 4] in _beyond(want, b)


def _beyond(want, b):
    """Scores of image b's kept rows that the max_det cut dropped."""
    cand = want["cand"][b]
    kept = R.nms_rows(cand, IOU, False)
    sc = np.sort(cand["score"][kept])[::-1]
    return sc[want["count"][b]:]


def test_coverage():
    multi = ref(80, 512, 20, True, False)
    cand0 = multi["cand"][0]
    p0 = make_pred(80, 512)[0, :, 4:]
    thr = cand0["score"].min()
    at_thr, admitted = int((p0 == thr).sum()), int((cand0["score"] == thr).sum())
    print("candidates", multi["candidates"], "at the threshold key", at_thr, "admitted", admitted)
    assert multi["candidates"][0] > 512 and 0 < admitted < at_thr          # overflow, tie partly admitted
    assert multi["candidates"][1] == 0 and multi["count"][1] == 0           # the empty image
    assert multi["candidates"][2] == 512                                    # exactly K
    assert multi["candidates"][3] == 151 and np.isnan(make_pred(80, 512)[3]).sum() == 1
    assert multi["cand"][3]["score"].max() == 1.0
    assert all(cut_in_tie(multi, b) for b in (0, 2, 3))                     # the max_det cut falls in a tie
    agn, best = ref(80, 512, 20, True, True), ref(80, 512, 20, False, False)
    print("kept on image 0: agnostic / class-wise / best-class", agn["kept"][0], multi["kept"][0], best["kept"][0])
    assert len({int(agn["kept"][0]), int(multi["kept"][0]), int(best["kept"][0])}) == 3
    small = ref(3, 512, 20, True, False)
    assert small["candidates"][0] > 512 and small["candidates"][2] == 512
    # the letterbox frame clips boxes on both sides and leaves some wholly in the padding
    fr = ref(80, 512, 300, True, False, None, True)
    raw = ref(80, 512, 300, True, False)
    m = raw["count"][0]
    rb, fb = raw["det"][0, :m, :4], fr["det"][0, :m, :4]
    low = ((rb[:, 0] < 0) | (rb[:, 1] < 64)).sum()
    high = ((rb[:, 2] > 320) | (rb[:, 3] > 256)).sum()
    flat = ((fb[:, 3] - fb[:, 1]) == 0).sum()
    print("frame: clipped low", low, "high", high, "wholly in the padding", flat)
    assert low > 0 and high > 0 and flat > 0


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("K", [512, 64, 1])
@pytest.mark.parametrize("nc", [80, 3, 1])
def test_candidate_stage(nc, K, multi):
    """yms_det_candidates alone: rows, their order and the -1 fill, array-equal."""
    _candidate_stage(nc, K, multi, None)


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("nc", [80, 3])
def test_candidate_stage_class_filter(nc, multi):
    _candidate_stage(nc, 64, multi, (1, nc - 1))


@pytest.mark.parametrize("multi", [True, False])
def test_candidate_stage_many_classes(multi):
    """nc = 150: not a multiple of 4 (the scalar walk) over ten 16-class slabs, and the pick's
    second batch of 128 classes."""
    _candidate_stage(150, 64, multi, None)
    check(run(150, 64, 20, multi, False), ref(150, 64, 20, multi, False))


def _candidate_stage(nc, K, multi, classes):
    p = make_pred(nc, K)
    d = torch.tensor(p).cuda()
    i32 = dict(dtype=torch.int32, device="cuda")
    box = torch.full((N, K, 4), 7.0, device="cuda")
    score = torch.full((N, K), 7.0, device="cuda")
    label, anchor = torch.full((N, K), 7, **i32), torch.full((N, K), 7, **i32)
    count, total = torch.full((N,), 7, **i32), torch.full((N,), 7, **i32)
    mask = None
    if classes is not None:
        mask = torch.zeros(nc, dtype=torch.uint8)
        mask[list(classes)] = 1
        mask = mask.cuda()
    wsb = L.lib().yms_det_ws_bytes(N, A, nc, K)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device="cuda")        # scratch arrives dirty
    L.call("yms_det_candidates", N, A, nc, d.data_ptr(), ctypes.c_float(CONF), int(multi), L.ptr(mask), K,
           box.data_ptr(), score.data_ptr(), label.data_ptr(), anchor.data_ptr(), count.data_ptr(),
           total.data_ptr(), ws.data_ptr(), wsb, L.stream_ptr(d.device))
    for b in range(N):
        want = R.candidates(p[b], CONF, multi, classes, K)
        assert (int(count[b]), int(total[b])) == (want["count"], want["total"]), b
        assert np.array_equal(anchor[b].cpu().numpy(), want["anchor"]), b
        assert np.array_equal(label[b].cpu().numpy(), want["label"]), b
        assert np.array_equal(score[b].cpu().numpy(), want["score"]), b
        assert np.array_equal(box[b].cpu().numpy(), want["boxes"]), b


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("K", [512, 64])
@pytest.mark.parametrize("nc", [80, 3, 1])
def test_detect_end_to_end(nc, K, multi, agnostic):
    for max_det in (300, 20, 7):
        check(run(nc, K, max_det, multi, agnostic), ref(nc, K, max_det, multi, agnostic))


@pytest.mark.parametrize("nc", [80, 3])
@pytest.mark.parametrize("multi", [True, False])
def test_detect_class_filter(nc, multi):
    cls = (1, nc - 1)
    check(run(nc, 512, 20, multi, False, cls), ref(nc, 512, 20, multi, False, cls))


def test_detect_k1():
    for nc in (80, 1):
        check(run(nc, 1, 7, True, False), ref(nc, 1, 7, True, False))


def test_detect_big_segment_routes(monkeypatch):
    """YMS_NMS_CAP=64: segments above 64 candidate rows take the NMS's big-segment routes."""
    monkeypatch.setenv("YMS_NMS_CAP", "64")
    for nc, agnostic in ((80, True), (3, False), (1, False)):
        check(run(nc, 512, 300, True, agnostic), ref(nc, 512, 300, True, agnostic))


def test_detect_frames_bit_equal():
    check(run(80, 512, 300, True, False, None, True), ref(80, 512, 300, True, False, None, True))
    check(run(3, 64, 20, False, True, None, True), ref(3, 64, 20, False, True, None, True))


def test_best_class_equals_batched_nms_indices():
    """Best-class mode without a binding cap keeps, per image, the (anchor, label) set of
    batched_nms_indices.  The first 900 anchors: every count fits max_det = 1024."""
    p = np.ascontiguousarray(make_pred(80, 512)[:, :900])
    d = torch.tensor(p).cuda()
    det = ops.detect(d, CONF, IOU, max_det=1024, max_nms=900)
    _, _, keep, klbl, cnt = ops.batched_nms_indices(d, CONF, IOU)
    dc = det.counts.cpu().numpy()
    assert np.array_equal(dc, cnt.cpu().numpy()) and dc.max() <= 1024 and dc[0] > 300
    for b in range(N):
        got = set(zip(det.anchors[b, :dc[b]].tolist(), det.labels[b, :dc[b]].tolist()))
        assert got == set(zip(keep[b, :dc[b]].tolist(), klbl[b, :dc[b]].tolist())), b


def test_detect_argument_errors():
    d = torch.tensor(make_pred(3, 64)).cuda()
    for kw in (dict(conf=-0.1), dict(conf=float("nan")), dict(max_nms=0), dict(max_nms=65537), dict(max_det=0),
               dict(max_det=1025), dict(classes=[3]), dict(classes=[-1]), dict(frames=torch.zeros(3, 6, device="cuda"))):
        with pytest.raises(ValueError):
            ops.detect(d, **kw)
    with pytest.raises(RuntimeError):
        ops.detect(d.cpu())


def test_detect_does_not_sync():
    """After a warm-up call (workspaces, the class mask), detect() makes no synchronising call."""
    d = torch.tensor(make_pred(80, 512)).cuda()
    fr = torch.tensor([LB_FRAME] * N, dtype=torch.float32).cuda()
    kw = dict(multi_label=True, classes=(1, 79), max_det=20, max_nms=512, frames=fr)
    ops.detect(d, CONF, IOU, **kw)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            d[0, 0, 0].item()                         # the mode does catch a sync in this build
        det = ops.detect(d, CONF, IOU, **kw)
        det2 = ops.detect(d, CONF, IOU, agnostic=True, max_det=20, max_nms=512)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    check(det, ref(80, 512, 20, True, False, (1, 79), True))
    assert int(det2.counts.sum()) > 0


# ------------------------------------------------------------------------------------------
# letterbox_normalize
# ------------------------------------------------------------------------------------------
H, W = 96, 128
SOURCES = [(17, 200), (333, 517), (1, 1), (64, 64)]
LEVEL = 1.0 / (255.0 * min(D.IMAGENET_STD))


def gate(out, want, dtype, what):
    """test_mosaic_gpu.py's gate."""
    if dtype == torch.bfloat16:
        want = torch.from_numpy(np.array(want)).to(torch.bfloat16).float().numpy()
    diff = np.abs(out - want)
    share = (diff > 1e-6).mean()
    print(what, "share > 1e-6:", share, "max:", diff.max())
    assert share < 1e-3, (what, share)
    assert diff.max() <= 2 * LEVEL, (what, diff.max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_letterbox_normalize(dtype):
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCES]
    images.append(np.broadcast_to(np.array([10, 200, 77], np.uint8), (40, 90, 3)).copy())   # constant colour
    x, frames = D.letterbox_normalize(D.to_device(images, "cuda"), (H, W), dtype=dtype)
    assert x.shape == (len(images), 3, H, W) and x.dtype == dtype
    out = x.float().cpu().numpy()
    geo = [D.Letterbox(im.shape[0], im.shape[1], H, W) for im in images]
    assert np.array_equal(frames.host, F32([g.frame for g in geo]))
    assert np.array_equal(frames.tensor.cpu().numpy(), frames.host)
    for i, (im, g) in enumerate(zip(images, geo)):
        layers, r = MR.record_of(g.plan(), [im])
        gate(out[i], MR.mosaic_normalize(layers, r, H, W, D.IMAGENET_MEAN, D.IMAGENET_STD), dtype, im.shape)
    # the constant source: exactly its normalised colour inside the tile, exactly normalised 114 outside
    g = geo[-1]
    mean, std = F32(D.IMAGENET_MEAN), F32(D.IMAGENET_STD)
    sc, bb = F32(1) / (F32(255) * std), -mean / std

    def norm(rgb):
        v = (F32(rgb) * sc + bb).astype(F32)
        return torch.from_numpy(v).to(dtype).float().numpy() if dtype == torch.bfloat16 else v
    inside = np.zeros((H, W), bool)
    inside[g.top:g.top + g.nh, g.left:g.left + g.nw] = True
    assert inside.any() and (~inside).any()
    for c in range(3):
        assert (out[-1, c][inside] == norm([10, 200, 77])[c]).all()
        assert (out[-1, c][~inside] == norm([114, 114, 114])[c]).all()


def test_validation_recipe_end_to_end():
    """letterbox -> model -> detect(conf 0.001, multi-label) -> MeanAveragePrecision, at toy size."""
    from yms.metrics import MeanAveragePrecision
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    model = YOLOv8("n", 3).cuda().eval()
    model.head.stride = torch.tensor([8.0, 16.0, 32.0])
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((40, 90), (100, 60))]
    x, frames = D.letterbox_normalize(D.to_device(images, "cuda"), (64, 96))
    with torch.no_grad():
        pred = model(x)
    assert pred.shape == (2, 8 * 12 + 4 * 6 + 2 * 3, 7)
    det = ops.detect(pred, 0.001, 0.7, multi_label=True, frames=frames)
    preds = det.to_list()
    assert all(p["labels"].dtype == torch.int64 and len(p["boxes"]) == k for p, k in zip(preds, det.counts.tolist()))
    assert sum(len(p["boxes"]) for p in preds) > 0
    for p, (h0, w0) in zip(preds, ((40, 90), (100, 60))):
        b = p["boxes"]
        assert (b >= 0).all() and (b[:, [0, 2]] <= w0).all() and (b[:, [1, 3]] <= h0).all()
    metric = MeanAveragePrecision()
    metric.update(preds, [{"boxes": p["boxes"], "labels": p["labels"]} for p in preds])
    assert float(metric.compute()["map"]) == 1.0
