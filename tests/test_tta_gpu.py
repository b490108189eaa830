"""Test-time augmentation on the GPU: yms_tta_merge (csrc/tta.hip) bit for bit against tests/tta_ref.py,
detect(vote=True) (yms_det_finalize_vote) against the float64 restatement, predict_views' view
batches against tests/mosaic_ref.py, and detect_views / detect_tta end to end at toy size.

Box tolerance of the vote: the restatement and the kernel both sum in float64, in different orders.
A float64 sum of at most 65536 terms of magnitude <= 1e4 carries <= 7e-8 absolute error, so the two
quotients, each rounded once to fp32, can differ by one fp32 ulp at a near-tie and no more:
rtol 2^-23, atol 1e-6.  Everything else of a voted detection is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import detect_ref as R
import mosaic_ref as MR
import tta_ref as T
from test_detect_gpu import CONF, IOU, LB_FRAME, N, gate, make_pred
from test_tta_cpu import ORIGINALS, VIEWS, round_trip_case
from yms import _lib as L
from yms import data as D
from yms import ops, tta

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------
# 1. merge_views
# ------------------------------------------------------------------------------------------
M_A, M_ROWS, M_FLIPS = (21, 13, 5), [(0, 21), (3, 13), (0, 4)], (1, 2, 3)
M_SIZES = [(128, 160), (64, 96), (32, 64)]
M_FRAMES = [F32([[1.6, 1.6, 3, 17, 80, 60], [1.6, 1.6, 24, 5, 70, 75]]),
            F32([[0.8, 0.8, 11, 2, 100, 75], [0.8, 0.8, 1, 9, 110, 60]]),
            F32([[0.375, 0.375, 2, 7, 160, 48], [0.375, 0.375, 13, 1, 100, 80]])]


@functools.lru_cache(maxsize=None)
def merge_case(nc):
    rng = np.random.default_rng(nc)
    preds = []
    for (H, W), a in zip(M_SIZES, M_A):
        p = np.zeros((2, a, 4 + nc), F32)
        p[..., 0] = rng.uniform(0, W, (2, a))
        p[..., 1] = rng.uniform(0, H, (2, a))
        p[..., 2:4] = rng.uniform(1, 60, (2, a, 2))
        p[..., 4:] = rng.uniform(0, 1, (2, a, nc))
        preds.append(p)
    preds[0][1, 20, 4 + nc - 1] = np.nan
    preds[1][0, 5, 4] = np.inf
    preds[2][1, 3, 0] = -7.25                               # inside (0, 4): the last taken row
    preds[1][1, 12, 1] = -0.5
    for p in preds:
        p.setflags(write=False)
    return preds


def gpu_merge(preds, frames, sizes, flips, rows=None):
    out = tta.merge_views([torch.tensor(p).cuda() for p in preds], [torch.tensor(f).cuda() for f in frames],
                          sizes, flips, rows)
    return out.cpu().numpy()


@pytest.mark.parametrize("nc", [3, 4, 80])
def test_merge_bit_for_bit(nc):
    """nc = 3: rows of 7 floats (no row after the first is 16-byte aligned); 4 and 80: the float4 path."""
    preds = merge_case(nc)
    want = T.merge(preds, M_FRAMES, M_SIZES, M_FLIPS, M_ROWS)
    got = gpu_merge(preds, M_FRAMES, M_SIZES, M_FLIPS, M_ROWS)
    assert got.shape == want.shape == (2, 21 + 10 + 4, 4 + nc)
    assert np.isnan(want).sum() == 1 and np.isinf(want).sum() == 1 and (want[..., :2] < 0).any()
    assert np.array_equal(bits(got), bits(want))
    # the rows are where the prefix sums put them: view 1's row 3 is merged row 21, scores as bits
    assert np.array_equal(bits(got[:, 21, 4:]), bits(preds[1][:, 3, 4:]))
    # one view, the full range, every flip
    for fl in (0, 1, 2, 3):
        w1 = T.merge(preds[:1], M_FRAMES[:1], M_SIZES[:1], [fl])
        g1 = gpu_merge(preds[:1], M_FRAMES[:1], M_SIZES[:1], [fl])
        assert g1.shape == preds[0].shape and np.array_equal(bits(g1), bits(w1))


def test_merge_misaligned_base():
    """nc = 4 from a tensor whose storage starts 4 bytes off a 16-byte boundary: the scalar walk."""
    preds = merge_case(4)
    want = T.merge(preds[:1], M_FRAMES[:1], M_SIZES[:1], [3], [(2, 19)])
    flat = torch.zeros(preds[0].size + 1, device="cuda")
    flat[1:] = torch.tensor(preds[0]).cuda().reshape(-1)
    p = flat[1:].view(preds[0].shape)
    assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    got = tta.merge_views([p], [torch.tensor(M_FRAMES[0]).cuda()], M_SIZES[:1], [3], [(2, 19)])
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_merge_more_than_one_block():
    """8 views of 700 rows at nc = 5 (scalar) and nc = 8 (float4): many blocks, every view slot in use."""
    rng = np.random.default_rng(5)
    for nc in (5, 8):
        preds = [rng.uniform(-4, 300, (3, 700, 4 + nc)).astype(F32) for _ in range(8)]
        frames = [np.concatenate([np.repeat(rng.uniform(0.3, 2, (3, 1)), 2, 1), rng.uniform(0, 30, (3, 2)),
                                  rng.uniform(50, 400, (3, 2))], 1).astype(F32) for _ in range(8)]
        sizes = [(64 + 32 * v, 96 + 32 * v) for v in range(8)]
        flips = [v % 4 for v in range(8)]
        rows = [(v, 700 - 3 * v) for v in range(8)]
        want = T.merge(preds, frames, sizes, flips, rows)
        assert np.array_equal(bits(gpu_merge(preds, frames, sizes, flips, rows)), bits(want))


@pytest.mark.parametrize("flip", [0, 1, 2, 3])
def test_merge_geometry_round_trip(flip):
    """test_tta_cpu's round trip through the kernel: original pixels -> view pixels in float64 ->
    yms_tta_merge -> within 1e-3 px of where they started."""
    for orig in ORIGINALS:
        for size in VIEWS:
            boxes0, pred, frame = round_trip_case(*orig, size, flip)
            out = gpu_merge([pred], [F32([frame])], [size], [flip])
            err = np.abs(out[0, :, :4].astype(np.float64) - boxes0).max()
            print(orig, size, flip, "max error", err)
            assert err <= 1e-3


def test_merge_argument_errors():
    p = torch.zeros(2, 8, 7, device="cuda")
    f = torch.ones(2, 6, device="cuda")
    ok = dict(preds=[p, p], frames=[f, f], sizes=[(64, 64), (32, 32)], flips=(0, 1))
    assert tta.merge_views(**ok).shape == (2, 16, 7)
    for kw in (dict(rows=[(0, 8), (4, 4)]), dict(rows=[(0, 9), (0, 8)]), dict(rows=[(-1, 8), (0, 8)]),
               dict(rows=[(0, 8)]), dict(flips=(0, 4)), dict(frames=[f, f[:1]]), dict(frames=[f, f.double()]),
               dict(preds=[p, p[:, :, :6]]), dict(preds=[p, p[:1]]), dict(preds=[p] * 9, frames=[f] * 9,
                                                                         sizes=[(64, 64)] * 9, flips=(0,) * 9),
               dict(preds=[], frames=[], sizes=[], flips=())):
        with pytest.raises(ValueError):
            tta.merge_views(**{**ok, **kw})
    with pytest.raises(RuntimeError):
        tta.merge_views(**{**ok, "preds": [p.cpu(), p.cpu()]})
    # the C entry point itself: nviews outside 1..8 and a range outside the rows
    P, I = ctypes.c_void_p * 1, ctypes.c_int * 1
    o = torch.empty(2, 8, 7, device="cuda")
    args = lambda nv, a1: (2, 3, nv, P(p.data_ptr()), I(8), I(0), I(a1), I(64), I(64), I(0), P(f.data_ptr()),
                           o.data_ptr(), L.stream_ptr(p.device))
    assert L.lib().yms_tta_merge(*args(1, 8)) == 0
    for nv, a1 in ((0, 8), (9, 8), (1, 9), (1, 0)):
        assert L.lib().yms_tta_merge(*args(nv, a1)) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------
# 2. detect(vote=True)
# ------------------------------------------------------------------------------------------
SHAPES = [(80, 512, 300), (3, 64, 8)]                       # (nc, K, max_det)
RTOL, ATOL = 2.0 ** -23, 1e-6


@functools.lru_cache(maxsize=None)
def vote_ref(nc, K, max_det, multi, agnostic, frames=False):
    out = T.detect_vote(make_pred(nc, K), CONF, IOU, multi, agnostic, None, max_det, K,
                        [LB_FRAME] * N if frames else None)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def run(nc, K, max_det, multi, agnostic, frames=False, pred=None, **kw):
    d = torch.tensor(make_pred(nc, K) if pred is None else pred).cuda()
    fr = torch.tensor([LB_FRAME] * d.shape[0], dtype=torch.float32).cuda() if frames else None
    return ops.detect(d, CONF, IOU, multi_label=multi, agnostic=agnostic, max_det=max_det, max_nms=K, frames=fr, **kw)


def check_vote(det, want):
    assert np.array_equal(det.counts.cpu().numpy(), want["count"])
    assert np.array_equal(det.candidates.cpu().numpy(), want["candidates"])
    assert np.array_equal(det.anchors.cpu().numpy(), want["anchor"])
    assert np.array_equal(det.labels.cpu().numpy(), want["det"][..., 5].astype(np.int32))
    assert np.array_equal(det.scores.cpu().numpy(), want["det"][..., 4])
    got, ref = det.boxes.cpu().numpy().astype(np.float64), want["det"][..., :4].astype(np.float64)
    err = np.abs(got - ref) - (ATOL + RTOL * np.abs(ref))
    print("boxes: max |diff|", np.abs(got - ref).max(), "differing", int((got != ref).sum()), "of", got.size)
    assert (err <= 0).all()


def test_coverage():
    """On the restatement: the generated input has kept rows with two or more members, kept rows
    beyond max_det, and voting moves boxes -- at both shapes, class-wise and agnostic."""
    for nc, K, max_det in SHAPES:
        for agnostic in (False, True):
            v = vote_ref(nc, K, max_det, True, agnostic)
            plain = R.detect(make_pred(nc, K), CONF, IOU, True, agnostic, None, max_det, K)
            multi_member = sum(int((m >= 2).sum()) for m in v["members"])
            beyond = int((v["kept"] - v["count"]).max())
            moved = int((v["det"][..., :4] != plain["det"][..., :4]).any(-1).sum())
            print((nc, K, max_det, agnostic), "kept rows with >= 2 members", multi_member, "kept beyond max_det",
                  beyond, "detections moved by the vote", moved)
            assert multi_member > 0 and beyond > 0 and moved > 0
            assert np.array_equal(v["det"][..., 4:], plain["det"][..., 4:]) and np.array_equal(v["anchor"], plain["anchor"])


@pytest.mark.parametrize("frames", [False, True])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_detect_vote(shape, multi, agnostic, frames):
    nc, K, max_det = shape
    check_vote(run(nc, K, max_det, multi, agnostic, frames, vote=True), vote_ref(nc, K, max_det, multi, agnostic, frames))


def hand_pred():
    """One image, 2 classes, boxes as (cx, cy, w, h); conf 0.25, IoU 0.45.
      a0  (50, 50, 20, 20)  c0 .9          a1  (52, 50, 20, 20)  c0 .6   IoU(a0, a1) = 18 / 22
      a2  (51, 50, 20, 20)  c1 .8          overlaps a0 and a1 in space, another class
      a3  (150, 150, 0, 30) c0 .7          zero area: its overlap with anything, itself included, is NaN
      a4  (250, 50, 30, 30) c1 .5          alone
      a5  (250, 250, 10, 10)               nothing above conf
    Class-wise: kept a0 (members a0, a1), a2 (itself), a3 (none), a4 (itself).  Agnostic: a0 by score
    suppresses a2 and a1; kept a0 (members a0, a1, a2), a3, a4."""
    p = np.zeros((1, 6, 6), F32)
    p[0, :, :4] = [(50, 50, 20, 20), (52, 50, 20, 20), (51, 50, 20, 20), (150, 150, 0, 30), (250, 50, 30, 30),
                   (250, 250, 10, 10)]
    p[0, [0, 1, 3], 4] = (0.9, 0.6, 0.7)
    p[0, [2, 4], 5] = (0.8, 0.5)
    return p


@pytest.mark.parametrize("agnostic", [False, True])
def test_vote_hand_built(agnostic):
    p = hand_pred()
    want = T.detect_vote(p, CONF, IOU, True, agnostic, None, 8, 16)
    det = run(2, 16, 8, True, agnostic, pred=p, vote=True)
    check_vote(det, want)
    boxes, anchors = det.boxes.cpu().numpy()[0].astype(np.float64), det.anchors.cpu().numpy()[0]
    if agnostic:
        assert list(anchors[:3]) == [0, 3, 4] and det.counts.tolist() == [3]
        x = (0.9 * 50 + 0.6 * 52 + 0.8 * 51) / 2.3                   # the classes mix
    else:
        assert list(anchors[:4]) == [0, 2, 3, 4] and det.counts.tolist() == [4]
        x = (0.9 * 50 + 0.6 * 52) / 1.5                              # a2 (class 1) stays out
        assert np.array_equal(boxes[1], [41, 40, 61, 60])            # a2: its only member is itself
    np.testing.assert_allclose(boxes[0], [x - 10, 40, x + 10, 60], rtol=1e-6)
    k = 1 if agnostic else 2
    assert np.array_equal(boxes[k], [150, 135, 150, 165])            # the zero-area box keeps its own
    assert np.array_equal(boxes[k + 1], [235, 35, 265, 65])          # the lone box: itself


def test_vote_infinite_score_keeps_its_box():
    p = hand_pred()
    p[0, 0, 4] = np.inf
    want = T.detect_vote(p, CONF, IOU, True, False, None, 8, 16)
    det = run(2, 16, 8, True, False, pred=p, vote=True)
    check_vote(det, want)
    assert np.array_equal(det.boxes.cpu().numpy()[0, 0], F32([40, 40, 60, 60]))


def test_vote_false_is_todays_output():
    """vote=False, and the default, against detect_ref bit for bit on the input of the vote cases."""
    for nc, K, max_det in SHAPES:
        for multi, agnostic, frames in ((True, False, True), (False, True, False)):
            want = R.detect(make_pred(nc, K), CONF, IOU, multi, agnostic, None, max_det, K,
                            [LB_FRAME] * N if frames else None)
            for det in (run(nc, K, max_det, multi, agnostic, frames, vote=False), run(nc, K, max_det, multi, agnostic, frames)):
                assert np.array_equal(det.counts.cpu().numpy(), want["count"])
                assert np.array_equal(det.anchors.cpu().numpy(), want["anchor"])
                assert np.array_equal(det.labels.cpu().numpy(), want["det"][..., 5].astype(np.int32))
                assert np.array_equal(det.scores.cpu().numpy(), want["det"][..., 4])
                assert np.array_equal(det.boxes.cpu().numpy(), want["det"][..., :4])


# ------------------------------------------------------------------------------------------
# 3. predict_views' view batches, 4. end to end
# ------------------------------------------------------------------------------------------
SIZE, SCALES, FLIPS = (128, 128), (1, .75, .5), (0, 1, 2)
DET_KW = dict(conf=0.05, iou=0.6, multi_label=True, max_det=20)


class Spy(torch.nn.Module):
    """The model, recording every input batch it is given."""

    def __init__(self, model):
        super().__init__()
        self.model, self.head, self.seen = model, model.head, []

    def forward(self, x):
        self.seen.append(x)
        return self.model(x)


@functools.lru_cache(maxsize=None)
def toy():
    """(spy around an eval YOLOv8-n with 3 classes, host images, device images, its Views)."""
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    model = YOLOv8("n", 3).cuda().eval()
    model.head.stride = torch.tensor([8.0, 16.0, 32.0])
    with torch.no_grad():
        for branch in model.head.cls:                         # random weights clear no threshold: lift the class biases
            branch[2].bias.fill_(-2.0)
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((120, 200), (97, 131))]
    dev = D.to_device(images, "cuda")
    spy = Spy(model).eval()
    views = tta.predict_views(spy, dev, size=SIZE, scales=SCALES, flips=FLIPS)
    return spy, images, dev, views


def test_predict_views_batches():
    spy, images, _, views = toy()
    assert views.sizes == [(128, 128), (96, 96), (64, 64)] and views.flips == [0, 1, 2] and views.strides == (8, 16, 32)
    assert [tuple(p.shape) for p in views.preds] == [(2, 336, 7), (2, 189, 7), (2, 84, 7)]
    assert all(p.dtype == torch.float32 for p in views.preds) and len(spy.seen) == 3
    for x, fr, (H, W), fl in zip(spy.seen, views.frames, views.sizes, views.flips):
        assert tuple(x.shape) == (2, 3, H, W)
        out = x.float().cpu().numpy()
        pairs = tta.view_plans([im.shape[:2] for im in images], (H, W), fl)
        assert np.array_equal(fr.host, F32([D.Letterbox(im.shape[0], im.shape[1], H, W).frame for im in images]))
        assert np.array_equal(fr.tensor.cpu().numpy(), fr.host)
        for i, (im, (lb, plan)) in enumerate(zip(images, pairs)):
            assert len(plan.layers[0].stages) == bin(fl).count("1")
            layers, r = MR.record_of(plan, [im])
            gate(out[i], MR.mosaic_normalize(layers, r, H, W, D.IMAGENET_MEAN, D.IMAGENET_STD), torch.float32,
                 (im.shape, (H, W), fl))


def test_predict_views_needs_eval_mode():
    spy, _, dev, _ = toy()
    spy.train()
    try:
        with pytest.raises(RuntimeError):
            tta.predict_views(spy, dev, size=SIZE, scales=SCALES, flips=FLIPS)
    finally:
        spy.eval()


@pytest.mark.parametrize("trim", [False, True])
def test_detect_views_end_to_end(trim):
    _, _, _, views = toy()
    preds = [p.cpu().numpy() for p in views.preds]            # the one read-back
    frames = [f.host for f in views.frames]
    rows = T.trim_rows(views.sizes, (8, 16, 32)) if trim else None
    merged = T.merge(preds, frames, views.sizes, views.flips, rows)
    assert merged.shape[1] == (320 + 189 + 20 if trim else 336 + 189 + 84)
    ident = np.concatenate([np.tile(F32([1, 1, 0, 0]), (2, 1)), frames[0][:, 4:]], 1)
    assert np.array_equal(tta.identity_frames(views.frames[0]).cpu().numpy(), ident)
    want = R.detect(merged, DET_KW["conf"], DET_KW["iou"], True, False, None, DET_KW["max_det"], 30000, ident)
    print("candidates", want["candidates"], "kept", want["kept"], "count", want["count"])
    assert (want["candidates"] >= 10).all() and (want["count"] > 0).all()
    det = tta.detect_views(views, trim=trim, **DET_KW)
    assert np.array_equal(det.counts.cpu().numpy(), want["count"])
    assert np.array_equal(det.candidates.cpu().numpy(), want["candidates"])
    assert np.array_equal(det.anchors.cpu().numpy(), want["anchor"])
    assert np.array_equal(det.labels.cpu().numpy(), want["det"][..., 5].astype(np.int32))
    assert np.array_equal(det.scores.cpu().numpy(), want["det"][..., 4])
    assert np.array_equal(det.boxes.cpu().numpy(), want["det"][..., :4])
    # anchors are merged rows: each maps back to (view, anchor) and to the score it was given
    a = int(det.anchors[0, 0])
    v, va = views.locate(a, trim)
    assert float(det.scores[0, 0]) == preds[v][0, va, 4 + int(det.labels[0, 0])]
    # boxes are inside each original image
    for b, (h0, w0) in enumerate(((120, 200), (97, 131))):
        bx = det.boxes[b, :int(det.counts[b])]
        assert (bx >= 0).all() and (bx[:, [0, 2]] <= w0).all() and (bx[:, [1, 3]] <= h0).all()


def test_detect_tta_and_vote_end_to_end():
    spy, _, dev, views = toy()
    want = tta.detect_views(views, **DET_KW)
    det = tta.detect_tta(spy.model, dev, size=SIZE, scales=SCALES, flips=FLIPS, **DET_KW)
    assert det.boxes.shape == want.boxes.shape == (2, 20, 4) and det.scores.shape == (2, 20)
    assert det.anchors.shape == det.labels.shape == (2, 20) and det.counts.shape == (2,)
    assert (det.counts <= 20).all() and (det.counts > 0).all()
    # voting on the merged views: the restatement, to the vote's tolerance
    preds = [p.cpu().numpy() for p in views.preds]
    frames = [f.host for f in views.frames]
    merged = T.merge(preds, frames, views.sizes, views.flips)
    ident = np.concatenate([np.tile(F32([1, 1, 0, 0]), (2, 1)), frames[0][:, 4:]], 1)
    vref = T.detect_vote(merged, DET_KW["conf"], DET_KW["iou"], True, False, None, 20, 30000, ident)
    check_vote(tta.detect_views(views, vote=True, **DET_KW), vref)


def test_detect_views_does_not_sync():
    """After a warm-up call, merge_views + detect on the merged tensor make no synchronising call."""
    _, _, _, views = toy()
    tta.detect_views(views, vote=True, **DET_KW)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        det = tta.detect_views(views, trim=True, vote=True, **DET_KW)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(det.counts.sum()) > 0
